"""Batched per-cycle environment `SBR-v2` on one MI355X: host-side mirror of the reference's SbrEnv2
(gym_SBR/envs/gym_SBR_env2.py:58).  One step() is a whole 12 h cycle (528 control intervals) in ONE kernel launch.
All numbers come from libsbr_amd.so; there is no CPU path."""
import ctypes as C

import torch

from . import _capi
from .vec_env import SbrOSVec, _ptr


class CycleLookahead:
    """SBR-v2's own fused call, mixed into SbrEnv2Vec (whose class body is reset, step and the refusals and nothing else)."""

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
        shape = tuple(getattr(candidates, "shape", ()))
        if len(shape) == 3:
            shape = (1,) + shape
            candidates = candidates[None]
        if not (len(shape) == 4 and shape[1] == self.num_envs and shape[2] >= 1 and shape[3] == _capi.NCYC_ACT):
            raise ValueError("candidates must have shape [n_cycles,N,K,3] or [N,K,3] with K >= 1")
        n_cycles, fanout = int(shape[0]), int(shape[2])
        if self.num_envs * fanout >= 2 ** 31:                    # before the outputs are sized by it
            raise ValueError("num_envs * K must stay below 2^31")
        a = self._keep_a = self._as_actions(candidates, shape)
        ptrs, end_ptrs, results = self._fanout_outputs(fanout, n_cycles, 1, return_rewards, return_best,
                                                       (return_end, return_end, return_status), end_rows=self._CYCLE_END_ROWS)
        _capi.check(self.lib.sbr_cycle_lookahead(self._h, n_cycles, fanout, _ptr(a) if n_cycles else None, *ptrs, *end_ptrs,
                                                 self._stream()), self._h)
        return results


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
    "branch_best": "the winner of a lookahead's branches",
    "mppi_update": "the MPPI tape update",
}


def _refusal(phrase):
    def refuse(self, *a, **k):            # before it looks at an argument
        raise NotImplementedError(phrase + " belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")
    return refuse


for _name, _phrase in _REFUSED.items():
    setattr(SbrEnv2Vec, _name, _refusal(_phrase))
