"""Batched per-cycle environment `SBR-v2` on one MI355X: host-side mirror of the reference's SbrEnv2
(gym_SBR/envs/gym_SBR_env2.py:58).  One step() is a whole 12 h cycle (528 control intervals) in ONE kernel launch.
All numbers come from libsbr_amd.so; there is no CPU path."""
import ctypes as C

import torch

from . import _capi
from .vec_env import SbrOSVec, _ptr


class SbrEnv2Vec(SbrOSVec):
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
