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

    def rollout(self, *a, **k):
        raise NotImplementedError("the fused random-policy rollout belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")

    def lookahead(self, *a, **k):
        raise NotImplementedError("the read-only lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")

    def lookahead_sampled(self, *a, **k):
        raise NotImplementedError("the sampled lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")

    def lookahead_end(self, *a, **k):
        raise NotImplementedError("the read-only lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")

    def lookahead_sampled_end(self, *a, **k):
        raise NotImplementedError("the sampled lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")

    def lookahead_policy(self, *a, **k):
        raise NotImplementedError("the closed-loop lookahead belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")

    def collect_policy(self, *a, **k):
        raise NotImplementedError("the fused policy collector belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")

    def branch_best(self, *a, **k):
        raise NotImplementedError("the winner of a lookahead's branches belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")

    def mppi_update(self, *a, **k):
        raise NotImplementedError("the MPPI tape update belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch")
