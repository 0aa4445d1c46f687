"""Batched per-cycle environment `SBR-v2` on one MI355X: host-side mirror of the reference's SbrEnv2
(gym_SBR/envs/gym_SBR_env2.py:58).  One step() is a whole 12 h cycle (528 control intervals) in ONE kernel launch.
All numbers come from libsbr_amd.so; there is no CPU path."""
import ctypes as C

import torch

from . import _capi
from .vec_env import SbrOSVec, _ptr


class CycleLookahead:
    """SBR-v2's own fused calls, mixed into SbrEnv2Vec (whose class body is reset, step and the refusals and nothing else)."""

    # the per-branch rows of the last cycle: obs_end, diag_end, status (see _fanout_outputs)
    _CYCLE_END_ROWS = (((_capi.NCYC_OBS,), torch.float64), ((_capi.NCYC_DIAG,), torch.float64), ((), torch.uint8))

    def cycle_lookahead(self, candidates, return_rewards=False, return_best=False, return_end=False, return_status=False):
        """Read-only lookahead over whole cycles, one launch (sbr_cycle_lookahead): `candidates` is [n_cycles, N, K, 3], or
        [N, K, 3] for one cycle - K tapes of DO set-point triples per env, on the device in the env's action dtype (converted
        if needed) - each played from the env's CURRENT state under its stored influent, a later cycle starting where the one
        before it ended (reset(carry_over=True) with the env's own influent, then step).  The handle is left bit for bit as it
        was.  Returns the sum of the cycles' rewards per candidate [N, K] float64, then, in this order and only if asked for:
        the reward of every cycle [n_cycles, N, K] float64; best_index [N] int32 and best_return [N] float64 (the largest
        return, NaN counting as -inf, ties to the lowest index); obs_end [N, K, 3] and diag_end [N, K, 12] float64, the
        observation and the diagnostics step() reports for the candidate's last cycle (at least one cycle then); status [N, K]
        uint8, the _capi.ST_* bits the candidate's state showed at the start or the end of any of its cycles."""
        return CycleLookahead._cycle_fanout(self, "sbr_cycle_lookahead", candidates, None, None, return_rewards, False, return_best,
                                            return_end, return_status, futures=False, one_cycle=True)

    def _cycle_fanout(self, entry, candidates, influent, n_scen, return_rewards, return_stats, return_best, return_end, return_status,
                      futures=True, one_cycle=False, need_influent=True):
        """The front of the three lookaheads, `entry` the library's name of the one: the shape checks, n_scen, the 2^31 bound
        before anything is sized by it, the inputs on the device and kept alive, the outputs through _fanout_outputs, the call.
        What a method has at all: `futures`, a trailing axis of n_scen futures per candidate (influent, n_scen and return_stats
        are theirs); `one_cycle`, the [N,K,3] shorthand; need_influent False, futures that may come without influent - n_scen is
        then the caller's or num_models, and at most the 65535 rows of a grid's y axis.  Called through the class: the public
        methods check their arguments on whatever `self` they are given."""
        shape = tuple(getattr(candidates, "shape", ()))
        if one_cycle and len(shape) == 3:
            shape = (1,) + shape
            candidates = candidates[None]
        if not (len(shape) == 4 and shape[1] == self.num_envs and shape[2] >= 1 and shape[3] == _capi.NCYC_ACT):
            raise ValueError("candidates must have shape [n_cycles,N,K,3]%s with K >= 1" % (" or [N,K,3]" if one_cycle else ""))
        if futures and (need_influent or influent is not None):
            ishape = tuple(getattr(influent, "shape", ()))
            if not (len(ishape) == 4 and ishape[:2] == shape[:2] and ishape[2] >= 1 and ishape[3] == _capi.NX):
                raise ValueError("influent must have shape [n_cycles,N,S,14] with S >= 1 and candidates' n_cycles")
            if n_scen is not None and int(n_scen) != ishape[2]:
                raise ValueError("n_scen must be influent's S when both are given")
            n_scen = int(ishape[2])
        elif futures:
            n_scen = self.num_models if n_scen is None else int(n_scen)
        if futures and not need_influent and not 1 <= n_scen <= 65535:
            raise ValueError("n_scen must be in 1 .. 65535 (without influent and n_scen it is num_models: call set_models first)")
        n_cycles, fanout = int(shape[0]), int(shape[2])
        if self.num_envs * fanout * (n_scen or 1) >= 2 ** 31:    # before the outputs are sized by it
            raise ValueError("num_envs * K%s must stay below 2^31" % (" * S" if futures else ""))
        a = self._as_actions(candidates, shape)
        f = None if influent is None else self._dev(influent, torch.float64, ishape)
        self._keep_a = (a, f)
        ptrs, end_ptrs, results = self._fanout_outputs(fanout, n_cycles, 1, return_rewards, return_best,
                                                       (return_end, return_end, return_status), end_rows=self._CYCLE_END_ROWS,
                                                       n_scen=n_scen, return_stats=return_stats)
        ins = [_ptr(t) if n_cycles else None for t in ((a, f) if futures else (a,))]
        _capi.check(getattr(self.lib, entry)(self._h, n_cycles, fanout, *((n_scen,) if futures else ()), *ins, *ptrs, *end_ptrs,
                                             self._stream()), self._h)
        return results

    def draw_influent(self, rows, per_env, seed=0, scenario=None, first_draw=0):
        """Influent FUTURES without a reset (sbr_draw_influent): [rows, N, per_env, 14] float64, rows x per_env draws of the
        reset's influent mix per env; a row of 14 is what reset(influent=...) takes for one env.  Draw (r, i, s) has index
        d = first_draw + r*per_env + s and depends on (seed, the env's global id, d, its scenario) and on nothing else; d = 0 is
        the draw of reset(seed).  `scenario` [N] int32 is shared by an env's draws; None: drawn per draw on the device under
        cfg.random_scenario, otherwise scenario 0 (SbrEnv2's fixed one).  Nothing of the handle is written."""
        rows, per_env = int(rows), int(per_env)
        if rows < 1 or per_env < 1 or self.num_envs * rows * per_env >= 2 ** 31:      # before the output is sized by it
            raise ValueError("rows and per_env must be >= 1 with num_envs * rows * per_env below 2^31")
        if scenario is None and not self.cfg.random_scenario:
            scenario = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device)
        scen = self._keep = self._dev(scenario, torch.int32, (self.num_envs,))
        out = torch.empty((rows, self.num_envs, per_env, _capi.NX), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.sbr_draw_influent(self._h, C.c_uint64(int(seed)), rows, per_env, int(first_draw), _ptr(scen),
                                                   _ptr(out), self._stream()), self._h)
        return out

    def influent_futures(self, n_cycles, n_scen, seed=0, scenario=None, first_draw=0, current_first=True):
        """The `influent` of cycle_lookahead_scenarios, [n_cycles, N, n_scen, 14]: draw_influent(n_cycles, n_scen, ...), with
        current_first the first cycle of every future under the influent the handle holds - the cycle about to start is the one
        whose influent is known."""
        out = self.draw_influent(n_cycles, n_scen, seed, scenario, first_draw)
        if current_first:
            out[0] = self.influent().T[:, None, :]
        return out

    def cycle_lookahead_scenarios(self, candidates, influent, return_rewards=False, return_stats=False, return_best=False,
                                  return_end=False, return_status=False):
        """cycle_lookahead under UNCERTAIN influent, one launch (sbr_cycle_lookahead_scenarios): `candidates` is
        [n_cycles, N, K, 3] as for cycle_lookahead, `influent` [n_cycles, N, S, 14] float64 (draw_influent's layout) - S futures
        per env, and every candidate of an env is played against the same S (common random numbers).  Cycle c of branch
        (i, k, s) runs under influent[c, i, s]; the handle's stored influent is never read (influent_futures puts it into
        cycle 0) and the handle is left bit for bit as it was.  Returns the sum of the cycles' rewards per branch [N, K, S]
        float64, then, in this order and only if asked for: the reward of every cycle [n_cycles, N, K, S]; mean and worst
        [N, K], the mean over s (summed in s order, one division) and the smallest of a candidate's S returns, NaN if one of
        them is; best_index [N] int32 and best_value [N] float64, the winner among an env's means (cycle_lookahead's rule);
        obs_end [N, K, S, 3] and diag_end [N, K, S, 12] float64; status [N, K, S] uint8 - all as cycle_lookahead gives them."""
        return CycleLookahead._cycle_fanout(self, "sbr_cycle_lookahead_scenarios", candidates, influent, None, return_rewards,
                                            return_stats, return_best, return_end, return_status)

    def set_models(self, models):
        """The handle's table of plant MODELS (sbr_set_models): `models` is a models.PlantModels or a sequence of _capi.SbrConfig
        that differ from the env's config in the model fields only (models.MODEL_FIELDS); None or an empty sequence drops the
        table.  Replaces an earlier table, waiting for the device first.  reset(), step() and every other call keep
        integrating the env's own config."""
        from .models import set_table
        set_table(self, models)

    @property
    def num_models(self):
        """Models in the handle's table (sbr_num_models); 0 if none is set."""
        from .models import table_size
        return table_size(self)

    def cycle_lookahead_models(self, candidates, influent=None, n_scen=None, return_rewards=False, return_stats=False,
                               return_best=False, return_end=False, return_status=False):
        """cycle_lookahead_scenarios under UNCERTAIN PLANT KINETICS, one launch (sbr_cycle_lookahead_models): future s of every env
        runs under MODEL s % num_models of the table set_models() gave the handle, in every cycle - the env's own config is not
        integrated by any branch (put it into the table to have the nominal plant among the futures).  `candidates` is
        [n_cycles, N, K, 3]; `influent` [n_cycles, N, S, 14] as for cycle_lookahead_scenarios, so that a future is an influent
        AND a plant, or None: every cycle of every future then runs under the env's stored influent (cycle_lookahead's rule)
        and the futures differ by their model alone.  n_scen = S defaults to influent's S, or to num_models without influent; with
        both given they must agree.  At most 65535 futures.  The handle is left bit for bit as it was.  Results and their order
        are cycle_lookahead_scenarios': returns [N, K, S], then if asked for the rewards [n_cycles, N, K, S], mean and worst
        [N, K], best_index and best_value [N], obs_end [N, K, S, 3] and diag_end [N, K, S, 12], status [N, K, S]."""
        return CycleLookahead._cycle_fanout(self, "sbr_cycle_lookahead_models", candidates, influent, n_scen, return_rewards,
                                            return_stats, return_best, return_end, return_status, need_influent=False)


class SbrEnv2Vec(CycleLookahead, SbrOSVec):
    """N SBR-v2 environments.  reset() -> obs [N,3]; step(a [N,3] in [0,1]) -> obs [N,3], reward [N], done (all True).
    The three actions are the DO set-points (x 8 mg/L) of the two aerobic reaction phases and of the aerated idle phase."""

    def __init__(self, num_envs, **kw):
        super().__init__(num_envs, **kw)
        n, dev = self.num_envs, self.device
        self.cobs = torch.empty((n, _capi.NCYC_OBS), dtype=self.out_dtype, device=dev)
        self.diag = torch.empty((n, _capi.NCYC_DIAG), dtype=torch.float64, device=dev)
        self.all_done = torch.ones((n,), dtype=torch.uint8, device=dev)

    def reset(self, seed=0, scenario=None, rnd=None, influent=None, mask=None, carry_over=False):
        ins = self._reset_inputs(scenario, rnd, influent, mask)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.sbr_cycle_reset(self._h, C.c_uint64(int(seed)), *ins, 1 if carry_over else 0, _ptr(self.cobs),
                                                 self._stream()), self._h)
        return self.cobs

    def step(self, action, want_diag=True):
        a = self._action(action, (self.num_envs, _capi.NCYC_ACT))
        _capi.check(self.lib.sbr_cycle_step(self._h, _ptr(a), _ptr(self.cobs), _ptr(self.reward),
                                            _ptr(self.diag) if want_diag else None, self._stream()), self._h)
        return self.cobs, self.reward, self.all_done


# The fused entry points of SbrOSVec that SBR-v2 refuses, and what each is called in the refusal.
_REFUSED = {
    "rollout": "the fused random-policy rollout",
    "lookahead": "the read-only lookahead",
    "lookahead_sampled": "the sampled lookahead",
    "lookahead_end": "the read-only lookahead",
    "lookahead_sampled_end": "the sampled lookahead",
    "lookahead_policy": "the closed-loop lookahead",
    "collect_policy": "the fused policy collector",
    "reset_models": "the reset over domain-randomised envs",
    "collect_policy_models": "the fused policy collector over domain-randomised envs",
    "rollout_policy_models": "the fused policy rollout over domain-randomised envs",
    "lookahead_models": "the read-only lookahead over plant models",
    "lookahead_sampled_models": "the sampled lookahead over plant models",
    "branch_best": "the winner of a lookahead's branches",
    "mppi_update": "the MPPI tape update",
}


def _refusal(phrase):
    def refuse(self, *a, **k):            # before it looks at an argument
        raise NotImplementedError(phrase + " belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")
    return refuse


# The refusals of the step-level models calls sit on the mixin, beside the set_models and num_models they would read: SBR-v2's
# use of the table is cycle_lookahead_models.  (SbrEnv2Vec's own class body stays reset, step and the first nine.)
_ON_MIXIN = ("reset_models", "collect_policy_models", "rollout_policy_models", "lookahead_models", "lookahead_sampled_models")

for _name, _phrase in _REFUSED.items():
    setattr(CycleLookahead if _name in _ON_MIXIN else SbrEnv2Vec, _name, _refusal(_phrase))
