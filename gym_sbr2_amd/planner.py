"""Sampling planners on the fused lookahead: the sampler of candidate tapes (struct sbr_sampler), a thin MPPI loop and a thin
policy-rollout planner on the closed-loop lookahead.

Plumbing only: the candidates are drawn, scored and averaged inside libsbr_amd.so (sbr_lookahead_sampled, sbr_mppi_update,
sbr_lookahead_policy); nothing here does arithmetic on a candidate.  The sums formed here add the caller's terminal value to a
return and average an env's returns.  The exception is CycleSetpointSearch for the per-cycle env SBR-v2, and
RobustCycleSetpointSearch on top of it: their candidates are three numbers per cycle, drawn and refitted in torch, and scored by
sbr_cycle_lookahead or, over influent futures, by sbr_cycle_lookahead_scenarios."""
import ctypes as C
import functools

import numpy as np

from . import _capi


def _pair(v):
    return tuple(float(x) for x in np.broadcast_to(np.asarray(v, dtype=np.float64), (2,)))


class TapeSampler:
    """How candidate tapes are drawn around a nominal tape (include/sbr_amd.h, "THE SAMPLE"): Gaussian perturbations of std
    `sigma` (a number or a pair, for u_DO and u_EC), keyed by `seed`, the global env id, the candidate and the row, clamped into
    [lo, hi].  lo defaults to (0, 0), hi to the config's (act_DO_max, act_EC_max).  keep_nominal: candidate 0 of every env is the
    nominal tape itself, so the plan never scores worse than what it started from."""

    def __init__(self, sigma, seed=0, lo=None, hi=None, keep_nominal=True):
        self.sigma, self.seed, self.keep_nominal = _pair(sigma), int(seed), bool(keep_nominal)
        self.lo = None if lo is None else _pair(lo)
        self.hi = None if hi is None else _pair(hi)

    def with_seed(self, seed):
        return TapeSampler(self.sigma, seed, self.lo, self.hi, self.keep_nominal)

    def bounds(self, cfg):
        """(lo, hi) with the defaults filled in from `cfg`."""
        return (self.lo if self.lo is not None else (0.0, 0.0),
                self.hi if self.hi is not None else (float(cfg.act_DO_max), float(cfg.act_EC_max)))

    def c_struct(self, cfg):
        """struct sbr_sampler under the config `cfg` (an _capi.SbrConfig)."""
        lo, hi = self.bounds(cfg)
        s = _capi.SbrSampler()
        s.sigma, s.lo, s.hi = (C.c_float * 2)(*self.sigma), (C.c_float * 2)(*lo), (C.c_float * 2)(*hi)
        s.seed = self.seed & (2 ** 64 - 1)
        s.keep_nominal, s.reserved_ = int(self.keep_nominal), 0
        return s


class MppiPlanner:
    """Model-predictive path integral control of the live plants of `env` (an SbrOSVec or ShardedSbrOS): per decision, `fanout`
    tapes of `rows` rows are sampled around the nominal tape and scored from every env's current state (lookahead_sampled, the
    handle untouched), and the nominal tape becomes their softmax(return / temperature)-weighted mean (mppi_update).  Decision d
    draws under seed = sampler.seed + d.  `nominal` [rows, N, 2] starts at the middle of the sampler's bounds and may be
    assigned to (same shape, the env's action dtype).

        planner = MppiPlanner(env, rows=50, fanout=64, sampler=TapeSampler((0.3, 2.0)), temperature=5.0)
        while ...: env.step(planner.plan())

    A TERMINAL VALUE for what lies beyond the horizon: assign `planner.terminal_value`, a callable taking (obs_end [N, K, 18],
    state_end [N, K, 15]), float32, and returning a tensor [N, K] - the caller's critic, plain torch code.  plan() then scores
    with lookahead_sampled_end and weighs the candidates by return + where(done_end, 0, terminal_value(...)); with
    return_returns=True it returns those adjusted returns.  None (the default): the planner scores by the returns alone.
    """
    terminal_value = None

    def __init__(self, env, rows, fanout, sampler, temperature, hold=1):
        import torch
        self.env, self.rows, self.fanout, self.sampler = env, int(rows), int(fanout), sampler
        self.temperature, self.hold, self.decision = float(temperature), int(hold), 0
        vec = getattr(env, "env", env)             # a ShardedSbrOS holds its SbrOSVec
        lo, hi = sampler.bounds(vec.cfg)
        mid = torch.tensor([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2], dtype=vec.action_dtype, device=vec.device)
        # two buffers of rows + 1 rows: the update lands in rows 0 .. rows - 1 of the one the nominal tape is not in, its last row
        # is repeated behind it, and rows 1 .. rows are the next nominal tape - the update advanced by one decision, no tape copied
        self._bufs = [mid.expand(self.rows + 1, vec.num_envs, 2).contiguous() for _ in range(2)]
        self._cur = 0
        self.nominal = self._bufs[0][1:]

    def plan(self, return_returns=False):
        """One decision: the action [N, 2] to give to step() (a view that stays valid until the plan after next); with
        return_returns=True also the candidates' returns [N, K]."""
        sm = self.sampler.with_seed(self.sampler.seed + self.decision)
        if self.terminal_value is None:
            scored = self._score(sm)
        else:
            ret, obs_end, state_end, done_end = self.env.lookahead_sampled_end(self.nominal, self.fanout, sm, hold=self.hold)
            v = self.terminal_value(obs_end, state_end).double()
            scored = ((ret + v.masked_fill(done_end, 0.0)).contiguous(),)
        self._cur ^= 1
        buf = self._bufs[self._cur]
        self.env.mppi_update(self.nominal, scored[0], sm, self.temperature, out=buf[:self.rows])
        buf[self.rows].copy_(buf[self.rows - 1])
        self.nominal = buf[1:]
        self.decision += 1
        return (buf[0],) + scored if return_returns else buf[0]

    def _score(self, sm):
        """What the candidates drawn by `sm` around the nominal tape are worth without a terminal value: a tuple whose first member
        [N, K] float64 is what mppi_update weighs them by; plan(return_returns=True) returns all of it behind the action."""
        return (self.env.lookahead_sampled(self.nominal, self.fanout, sm, hold=self.hold),)


class RobustMppiPlanner(MppiPlanner):
    """MppiPlanner when the plant's kinetics are NOT known: the same loop - the two buffers, the seed per decision, mppi_update -
    with every candidate tape scored under every model of the table `env` holds (env.set_models(...); lookahead_sampled_models,
    one launch, the handle untouched).  All models of a candidate play the same tape, so two candidates differ by what they do and
    not by what they drew.  risk="mean" weighs a candidate by the mean of its M returns, risk="worst" by the smallest of them.
    The env's own config is scored only if it stands in the table.

        env.set_models(PlantModels.perturbed(env.cfg, 8, rel_std=0.1))
        planner = RobustMppiPlanner(env, rows=50, fanout=64, sampler=TapeSampler((0.3, 2.0)), temperature=5.0, risk="worst")
        while ...: env.step(planner.plan())

    plan(return_returns=True) returns (action, the statistic the candidates were weighed by [N, K], every branch's return
    [N, K, M]).  There is no terminal value: the lookahead over models has no _end form, and assigning one raises ValueError.
    """

    def __init__(self, env, rows, fanout, sampler, temperature, hold=1, risk="mean"):
        if risk not in ("mean", "worst"):
            raise ValueError('risk must be "mean" or "worst"')
        super().__init__(env, rows, fanout, sampler, temperature, hold)
        self.risk = risk

    @property
    def terminal_value(self):
        return None

    @terminal_value.setter
    def terminal_value(self, value):
        if value is not None:
            raise ValueError("RobustMppiPlanner takes no terminal_value: the lookahead over models has no _end form")

    def _score(self, sm):
        ret, mean, worst = self.env.lookahead_sampled_models(self.nominal, self.fanout, sm, hold=self.hold, return_stats=True)
        return (mean if self.risk == "mean" else worst), ret


class CycleSetpointSearch:
    """Which DO set-points should each plant of `env` (an SbrEnv2Vec) run in the cycle it is about to start?  A cross-entropy
    search on the per-cycle lookahead: per iteration, `K` tapes of `n_cycles` set-point triples are drawn per env around a
    per-env mean and std (start: 0.5 and 0.25), clamped to [0, 1] and scored from the env's current state (cycle_lookahead, the
    handle untouched); mean and std are refitted on the best elite_frac of them.  Candidates whose state came NEAR A POLE or
    went NON-FINITE (status), or whose return is NaN, are left out of the fit and cannot win.  Candidate 0 is always the best
    tape so far - the all-0.5 tape to begin with - so while that tape is itself clean the plan never scores worse than it.  An
    env none of whose candidates may win keeps its mean, its std and its best tape so far: only then - the all-0.5 tape is
    flagged and nothing clean has been drawn - can the returned tape be a flagged one and its value NaN; `status` [N] uint8 holds
    the winner's bits after plan(), check it before acting.  Plan d draws under seed + d.  The sampling and the fit are plain
    torch on the device; every return comes from libsbr_amd.so.

        search = CycleSetpointSearch(env, K=64, n_cycles=3, iters=4, elite_frac=0.25, seed=0)
        action, value = search.plan(); env.step(action); env.reset(influent=..., carry_over=True)
    """
    init_mean, init_std, min_std = 0.5, 0.25, 0.02

    def __init__(self, env, K, n_cycles=1, iters=3, elite_frac=0.25, seed=0):
        self.env, self.K, self.n_cycles, self.iters = env, int(K), int(n_cycles), int(iters)
        if self.K < 1 or self.n_cycles < 1 or self.iters < 1:
            raise ValueError("K, n_cycles and iters must be >= 1")
        self.n_elite, self.seed, self.decision = max(1, min(self.K, int(round(float(elite_frac) * self.K)))), int(seed), 0
        self.tape = self.status = None          # after plan(): the winning tape [n_cycles, N, 3] float64 and its status bits [N]

    def plan(self):
        """One decision: (the first cycle's action [N, 3] in the env's action dtype, the tape's return [N] float64 - exactly what
        cycle_lookahead returns for `self.tape`)."""
        import torch
        env, bad_bits = self.env, _capi.ST_NEAR_POLE | _capi.ST_NONFINITE
        gen = torch.Generator(device=env.device).manual_seed(self.seed + self.decision)
        shape = (self.n_cycles, env.num_envs, self.K, 3)
        mean = torch.full(shape[:2] + (1, 3), self.init_mean, dtype=torch.float64, device=env.device)
        std, best = torch.full_like(mean, self.init_std), mean.clone()
        for _ in range(self.iters):
            cand = (mean + std * torch.randn(shape, generator=gen, dtype=torch.float64, device=env.device)).clamp_(0.0, 1.0)
            cand[:, :, :1] = best
            cand = cand.to(env.action_dtype).double()            # the values the kernel integrates
            ret, status = self._score(cand)
            out = ((status & bad_bits) != 0) | ret.isnan()
            top, idx = ret.masked_fill(out, float("-inf")).topk(self.n_elite, dim=1)
            ok = top > float("-inf")                             # [N, n_elite]: the elite is a candidate that may win
            elite = cand.gather(2, idx[None, :, :, None].expand(self.n_cycles, -1, -1, 3))
            w, some = ok.double()[None, :, :, None], ok[:, 0][None, :, None, None]
            cnt = w.sum(2, keepdim=True).clamp_(min=1.0)
            fit = (elite * w).sum(2, keepdim=True) / cnt
            spread = (((elite - fit) ** 2 * w).sum(2, keepdim=True) / cnt).sqrt_().clamp_(min=self.min_std)
            mean, std = torch.where(some, fit, mean), torch.where(some, spread, std)     # an env with no such candidate keeps its fit ...
            win = idx[:, :1].masked_fill(~ok[:, :1], 0)                                   # ... and its best tape so far, candidate 0
            best = cand.gather(2, win[None, :, :, None].expand(self.n_cycles, -1, -1, 3))
            value, flags = ret.gather(1, win)[:, 0], status.gather(1, win)[:, 0]
        self.tape, self.status = best[:, :, 0], flags
        self.decision += 1
        return self.tape[0].to(env.action_dtype), value

    def _score(self, cand):
        """What the loop ranks the candidates [n_cycles, N, K, 3] by: (value [N, K] float64, status bits [N, K] uint8)."""
        return self.env.cycle_lookahead(cand, return_status=True)


class RobustCycleSetpointSearch(CycleSetpointSearch):
    """CycleSetpointSearch when the influent of the coming cycles is NOT known: the same cross-entropy loop, every candidate
    scored over `n_scen` influent futures - the same futures for all candidates of an env (cycle_lookahead_scenarios), so that two
    tapes differ by what they do and not by what they drew.  risk="mean" ranks a candidate by the mean of its n_scen returns,
    risk="worst" by the smallest of them.  One set of futures per plan(): env.influent_futures(n_cycles, n_scen, seed,
    first_draw = 1 + plans so far * n_cycles * n_scen) - cycle 0 under the influent the handle holds, later cycles drawn, no
    draw used twice and none the draw of reset(seed).  A candidate is left out of the fit and cannot win if ANY of its n_scen
    branches came near a pole or went non-finite; `status` [N] is the OR of the winner's branches' bits.  After plan(): `tape`,
    `status` as CycleSetpointSearch keeps them and `futures` [n_cycles, N, n_scen, 14]; the returned value is exactly
    cycle_lookahead_scenarios' mean (or worst) of `tape` on `futures`.

        search = RobustCycleSetpointSearch(env, K=64, n_scen=16, n_cycles=3, risk="worst")
        action, value = search.plan(); env.step(action); env.reset(influent=..., carry_over=True)

    UNCERTAIN PLANT KINETICS as well: assign `search.plant_models = True` on an env that holds a model table (env.set_models(...)).
    The candidates are then scored with cycle_lookahead_models on the same futures, and each future is an influent AND a plant:
    future s runs under model s % env.num_models, so n_scen a multiple of num_models gives every model the same number of
    influents.  The returned value is then cycle_lookahead_models' mean (or worst) of `tape` on `futures`.  False (the default):
    every future runs under the env's own config.
    """
    plant_models = False

    def __init__(self, env, K, n_scen, n_cycles=2, iters=3, elite_frac=0.25, seed=0, risk="mean"):
        super().__init__(env, K, n_cycles, iters, elite_frac, seed)
        self.n_scen, self.risk, self.futures = int(n_scen), risk, None
        if self.n_scen < 1:
            raise ValueError("n_scen must be >= 1")
        if risk not in ("mean", "worst"):
            raise ValueError('risk must be "mean" or "worst"')

    def plan(self):
        self.futures = self.env.influent_futures(self.n_cycles, self.n_scen, seed=self.seed,
                                                 first_draw=1 + self.decision * self.n_cycles * self.n_scen)
        return super().plan()

    def _score(self, cand):
        look = self.env.cycle_lookahead_models if self.plant_models else self.env.cycle_lookahead_scenarios
        _, mean, worst, status = look(cand, self.futures, return_stats=True, return_status=True)
        return (mean if self.risk == "mean" else worst), functools.reduce(lambda u, v: u | v, status.unbind(-1))


class PolicyRolloutPlanner:
    """Policy-guided planning on the closed-loop lookahead: per decision, `fanout` rollouts of `policy` (an MlpPolicy) over
    `n_steps` calls are run from every env's current state and observation (lookahead_policy, the handle untouched), branch 0
    at the policy's mean and the others under exploration noise of std `noise_std`; the first action of the best branch is the
    plan, and the mean of the env's returns is a Monte-Carlo estimate of the policy's value at that state.  Decision d draws
    under noise_seed + d.  `env` is an SbrOSVec or a ShardedSbrOS.

        planner = PolicyRolloutPlanner(env, policy, fanout=64, n_steps=50, hold=1, noise_std=(0.3, 2.0))
        while ...:
            action, value = planner.plan()
            env.step(action)

    terminal_value: a callable taking (obs_end [N, K, 18], state_end [N, K, 15]), float32, and returning a tensor [N, K] - the
    caller's critic.  Each branch is then scored by return + where(done_end, 0, terminal_value(...)), and the value is the mean
    of those scores.  Nothing on the path waits for the device."""

    def __init__(self, env, policy, fanout, n_steps, hold, noise_std, terminal_value=None, noise_seed=0):
        self.env, self.policy, self.fanout, self.n_steps, self.hold = env, policy, int(fanout), int(n_steps), int(hold)
        self.noise_std, self.terminal_value, self.noise_seed, self.decision = noise_std, terminal_value, int(noise_seed), 0

    def plan(self, obs=None):
        """One decision: (the action [N, 2] float32 to give to step(), the Monte-Carlo value [N] float64).  `obs` is the
        observation in force (None: the env's own obs buffer)."""
        end = self.terminal_value is not None
        out = self.env.lookahead_policy(self.policy, self.fanout, self.n_steps, hold=self.hold, obs=obs, noise_std=self.noise_std,
                                        noise_seed=self.noise_seed + self.decision, keep_mean=True, return_actions=True,
                                        return_end=end)
        ret, acts = out[0], out[1]
        if end:
            obs_end, state_end, done_end = out[2:]
            v = self.terminal_value(obs_end, state_end).double()
            ret = (ret + v.masked_fill(done_end, 0.0)).contiguous()
        best, _ = self.env.branch_best(ret)
        self.decision += 1
        pick = best.long()[:, None, None].expand(-1, 1, 2)
        return acts[0].gather(1, pick)[:, 0], ret.mean(dim=1)
