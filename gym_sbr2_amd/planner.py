"""Sampling planners on the fused lookahead: the sampler of candidate tapes (struct sbr_sampler), a thin MPPI loop and a thin
policy-rollout planner on the closed-loop lookahead.

Plumbing only: the candidates are drawn, scored and averaged inside libsbr_amd.so (sbr_lookahead_sampled, sbr_mppi_update,
sbr_lookahead_policy); nothing here does arithmetic on a candidate.  The sums formed here add the caller's terminal value to a
return and average an env's returns."""
import ctypes as C

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
            ret = self.env.lookahead_sampled(self.nominal, self.fanout, sm, hold=self.hold)
        else:
            ret, obs_end, state_end, done_end = self.env.lookahead_sampled_end(self.nominal, self.fanout, sm, hold=self.hold)
            v = self.terminal_value(obs_end, state_end).double()
            ret = (ret + v.masked_fill(done_end, 0.0)).contiguous()
        self._cur ^= 1
        buf = self._bufs[self._cur]
        self.env.mppi_update(self.nominal, ret, sm, self.temperature, out=buf[:self.rows])
        buf[self.rows].copy_(buf[self.rows - 1])
        self.nominal = buf[1:]
        self.decision += 1
        return (buf[0], ret) if return_returns else buf[0]


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
