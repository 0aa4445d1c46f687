"""Batched SBROS-v1 environment on one MI355X: the host-side mirror of the reference's SbrOS
(gym_SBR/envs/gym_SBR_oneshot.py:99) for N independent reactors.

PyTorch is used for device memory and streams only; every number comes out of libsbr_amd.so
(HIP kernels) through the C ABI of include/sbr_amd.h.  There is no CPU path.
"""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _capi

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "influent_tables.npz")


def load_influent_tables():
    """The eight influent scenarios of buffer_tank3.py:18-1197 as data: means, stds [8][14][48]
    (13 concentrations + flow q; captured from the reference by oracle/gen_golden.py)."""
    t = np.load(_DATA)
    return np.ascontiguousarray(t["means"], dtype=np.float64), np.ascontiguousarray(t["stds"], dtype=np.float64)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _one_or_all(out):
    """What a method with optional results returns: the tuple, or its only member."""
    return out if len(out) > 1 else out[0]


class PolicyCollection(collections.namedtuple("PolicyCollection", "obs actions rewards flags returns last_obs")):
    """What SbrOSVec.collect_policy returns (the shapes are given there)."""
    __slots__ = ()

    @property
    def taken(self):
        """[rows, N] bool: the decision was taken (the env's episode had not ended before it)."""
        return (self.flags & _capi.DF_TAKEN) != 0

    @property
    def ended(self):
        """[rows, N] bool: the env's episode ended during one of the decision's calls - the transition is terminal."""
        return (self.flags & _capi.DF_ENDED) != 0


# the handle of torch's current stream on a device: torch's own fast accessor (an int, no Stream object) where it exists
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)


class SbrOSVec:
    """N SBROS-v1 environments on one GPU.

    reset()  -> obs [N,18]                         (SbrOS.reset, :168-438; obs_DO[9] ++ obs_EC[9])
    step(a)  -> obs [N,18], state [N,15], reward [N], done [N] uint8   (SbrOS.step, :843-1273)
    action a: [N,2] float32 (or float64 with action_dtype=torch.float64, what the reference's step() receives)
    = (DO set-point, NO3 set-point), clipped to [0,8] x [0,15] as in the reference.
    """

    def __init__(self, num_envs, device=0, first_env_id=0, out_dtype=torch.float32, config=None, tables=None,
                 action_dtype=torch.float32, reward=None, random_scenario=None):
        if not torch.cuda.is_available():
            raise _capi.SbrError("SbrOSVec needs a HIP device (torch.cuda.is_available() is False); "
                                 "this package has no CPU fallback")
        self.lib = _capi.load()
        self.num_envs = int(num_envs)
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        self.first_env_id = int(first_env_id)
        self.cfg = config if config is not None else _capi.default_config()
        if reward is not None:                # "eqi_oci" (the reference's SBROS-v1 reward) | "g2anet" | "oci"
            if reward not in _capi.REWARD_KINDS:
                raise ValueError("reward must be one of %s" % sorted(_capi.REWARD_KINDS))
            self.cfg.reward_kind = _capi.REWARD_KINDS[reward]
        if random_scenario is not None:       # reset(scenario=None) draws one of the 8 scenarios per env (SbrEnv4, gym_SBR_env4.py:107)
            self.cfg.random_scenario = 1 if random_scenario else 0
        if out_dtype not in (torch.float32, torch.float64):
            raise ValueError("out_dtype must be torch.float32 or torch.float64")
        self.out_dtype = out_dtype
        self.cfg.out_f64 = 1 if out_dtype == torch.float64 else 0
        if action_dtype not in (torch.float32, torch.float64):
            raise ValueError("action_dtype must be torch.float32 or torch.float64")
        self.action_dtype = action_dtype
        self.cfg.act_f64 = 1 if action_dtype == torch.float64 else 0
        self._h = C.c_void_p()
        _capi.check(self.lib.sbr_create(self.num_envs, self.device.index, self.first_env_id, C.byref(self.cfg),
                                        C.byref(self._h)))
        means, stds = tables if tables is not None else load_influent_tables()
        means = np.ascontiguousarray(means, dtype=np.float64)
        stds = np.ascontiguousarray(stds, dtype=np.float64)
        assert means.shape == stds.shape == (_capi.NSCEN, _capi.NSERIES, _capi.NSAMP)
        _capi.check(self.lib.sbr_set_influent_tables(self._h, means.ctypes.data_as(C.c_void_p),
                                                     stds.ctypes.data_as(C.c_void_p)), self._h)
        n, dev = self.num_envs, self.device
        self._ashape = (n, 2)
        self._sbr_step = self.lib.sbr_step
        self._outs = [None] * 4
        self._step_out = None
        self.obs = torch.empty((n, _capi.NOBS), dtype=out_dtype, device=dev)
        self.state = torch.empty((n, _capi.NSTATE), dtype=out_dtype, device=dev)
        self.reward = torch.empty((n,), dtype=out_dtype, device=dev)
        self.done = torch.empty((n,), dtype=torch.uint8, device=dev)

    # The output buffers step() and reset() write.  They may be replaced by the caller (same shape, dtype and device, e.g. a
    # slice of a rollout buffer); their addresses are converted once here, so that the host side of a step is ~5 us of Python
    # (scripts/gpu_host_overhead.py).
    def _set_out(self, k, t):
        shape, dtype = (((self.num_envs, _capi.NOBS), self.out_dtype), ((self.num_envs, _capi.NSTATE), self.out_dtype),
                        ((self.num_envs,), self.out_dtype), ((self.num_envs,), torch.uint8))[k]
        if not (isinstance(t, torch.Tensor) and t.shape == shape and t.dtype == dtype and t.device == self.device
                and t.is_contiguous()):
            raise ValueError("output buffer %d must be a contiguous %s tensor of shape %s on %s" % (k, dtype, shape, self.device))
        self._outs[k] = t
        if all(o is not None for o in self._outs):
            self._step_out = tuple(C.c_void_p(o.data_ptr()) for o in self._outs)

    obs = property(lambda self: self._outs[0], lambda self, t: self._set_out(0, t))
    state = property(lambda self: self._outs[1], lambda self, t: self._set_out(1, t))
    reward = property(lambda self: self._outs[2], lambda self, t: self._set_out(2, t))
    done = property(lambda self: self._outs[3], lambda self, t: self._set_out(3, t))

    # ------------------------------------------------------------------ plumbing
    def _stream(self):
        return C.c_void_p(_raw_stream(self.device.index))

    def _dev(self, a, dtype, shape):
        if a is None:
            return None
        t = torch.as_tensor(a, dtype=dtype, device=self.device).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (tuple(shape), tuple(t.shape)))
        return t

    def _reset_inputs(self, scenario, rnd, influent, mask):
        """reset()'s optional inputs as device pointers; the tensors stay alive until the stream has consumed them."""
        n = self.num_envs
        self._keep = (self._dev(scenario, torch.int32, (n,)), self._dev(rnd, torch.float64, (n, _capi.NSAMP)),
                      self._dev(influent, torch.float64, (n, _capi.NX)), self._dev(mask, torch.uint8, (n,)))
        return [_ptr(t) for t in self._keep]

    def _as_actions(self, a, shape):
        """The caller's tensor as it is where the kernels can read it - contiguous, on the device, of the env's action dtype - or
        a converted copy of `shape`."""
        if isinstance(a, torch.Tensor) and a.dtype == self.action_dtype and a.is_contiguous() and a.device == self.device:
            return a
        return self._dev(a, self.action_dtype, shape)

    def _action(self, action, shape):
        """An action as a contiguous device tensor of the env's action dtype and of `shape` = (N, width), kept alive."""
        a = self._as_actions(action, shape)
        if a.shape != shape:
            raise ValueError("action must have shape [N,%d]" % shape[1])
        self._keep_a = a
        return a

    def _tape(self, actions, trailing, n_steps, hold):
        """What rollout_actions and lookahead ask of a tape: `hold` >= 1, the shape (rows,) + `trailing` (None = any size >= 1),
        enough rows for `n_steps` calls (None = all of them).  Returns (the tape on the device, kept alive; rows; n_steps)."""
        if hold < 1:
            raise ValueError("hold must be >= 1")
        shape = tuple(getattr(actions, "shape", ()))
        if not (len(shape) == 1 + len(trailing)
                and all(int(s) >= 1 if t is None else int(s) == t for s, t in zip(shape[1:], trailing))):
            raise ValueError("actions must have shape [R,N,K,2] with K >= 1" if None in trailing else "actions must have shape [R,N,2]")
        rows = int(shape[0])
        n_steps = rows * hold if n_steps is None else int(n_steps)
        if n_steps < 0:
            raise ValueError("n_steps must be >= 0")
        if -(-n_steps // hold) > rows:
            raise ValueError("%d calls with hold=%d need %d rows of actions, got %d" % (n_steps, hold, -(-n_steps // hold), rows))
        self._keep_a = self._as_actions(actions, shape)
        return self._keep_a, rows, n_steps

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            torch.cuda.synchronize(self.device)
            self.lib.sbr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ the gym-like surface
    def reset(self, seed=0, scenario=None, rnd=None, influent=None, mask=None, carry_over=False):
        """carry_over=True starts the new cycle from each env's own current state (multi-cycle operation: x0 := x,
        IV := x[0]; disabled in the reference, gym_SBR_oneshot.py:260-268) instead of the configured start state."""
        ins = self._reset_inputs(scenario, rnd, influent, mask)
        with torch.cuda.device(self.device):
            fn = self.lib.sbr_reset_carry if carry_over else self.lib.sbr_reset
            _capi.check(fn(self._h, C.c_uint64(int(seed)), *ins, _ptr(self.obs), self._stream()), self._h)
        return self.obs

    def step(self, action):
        a = action if (isinstance(action, torch.Tensor) and action.dtype == self.action_dtype and action.is_contiguous()
                       and action.device == self.device) else self._dev(action, self.action_dtype, self._ashape)
        if a.shape != self._ashape:
            raise ValueError("action must have shape [N,2]")
        o, s, r, d = self._step_out
        rc = self._sbr_step(self._h, a.data_ptr(), o, s, r, d, _raw_stream(self.device.index))
        if rc:
            _capi.check(rc, self._h)
        self._keep_a = a
        return tuple(self._outs)

    def enable_host_io(self):
        """Small batches driven from the host (the reference-shaped single env): allocate PINNED host buffers for the action
        and for obs/state/reward/done and let the kernel read and write them directly over PCIe (pinned host memory is
        device-accessible), so that a step costs one launch and one stream synchronisation instead of one host-to-device
        and four device-to-host copies.  Returns the numpy views that step_host() fills."""
        np_out = {torch.float32: np.float32, torch.float64: np.float64}
        n = self.num_envs
        self._h_act = torch.empty((n, 2), dtype=self.action_dtype).pin_memory()
        self._h_obs = torch.empty((n, _capi.NOBS), dtype=self.out_dtype).pin_memory()
        self._h_state = torch.empty((n, _capi.NSTATE), dtype=self.out_dtype).pin_memory()
        self._h_reward = torch.empty((n,), dtype=self.out_dtype).pin_memory()
        self._h_done = torch.empty((n,), dtype=torch.uint8).pin_memory()
        self._h_views = (self._h_act.numpy(), self._h_obs.numpy(), self._h_state.numpy(), self._h_reward.numpy(),
                         self._h_done.numpy())
        self._h_ptrs = tuple(C.c_void_p(t.data_ptr()) for t in (self._h_act, self._h_obs, self._h_state, self._h_reward, self._h_done))
        self._sbr_sync = self.lib.sbr_synchronize
        return self._h_views

    def step_host(self, action):
        """step() through the pinned host buffers of enable_host_io(): action is array-like [N,2]; returns numpy views of
        obs, state, reward, done, valid until the next call (the stream has been synchronised).  Two C calls - sbr_step and
        sbr_synchronize - with every pointer converted once in enable_host_io()."""
        self._h_views[0][...] = action
        st = _raw_stream(self.device.index)
        rc = self._sbr_step(self._h, *self._h_ptrs, st) or self._sbr_sync(self._h, st)
        if rc:
            _capi.check(rc, self._h)
        return self._h_views[1:]

    def capture_steps(self, actions):
        """Capture one step() per action tensor of `actions` (a sequence of [N,2] device tensors at fixed addresses) into a
        HIP graph and return it; graph.replay() then issues all of them with one host call (0.4 us per step instead of
        ~8 us through Python).  obs/state/reward/done hold the outputs of the LAST captured step after a replay.  Nothing in
        sbr_step allocates or synchronises, which is what makes it capturable."""
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        # capture_error_mode "thread_local": only THIS thread's calls are checked against the capture.  With a process group up,
        # RCCL's watchdog thread polls its events from another thread, which the default ("global") mode may take for an illegal call
        # during capture and invalidate the graph - in a multi-rank run, of all places.  sbr_step itself makes no such call.
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                for a in actions:
                    self.step(a)
        torch.cuda.current_stream(self.device).wait_stream(side)
        return g

    def rollout(self, n_steps, policy_seed=0, return_actions=False):
        """n_steps fused step() calls per env with the on-device uniform random policy; returns the
        per-env sum of rewards [N] float64 (and the sampled actions [n_steps,N,2] float32)."""
        ret = torch.empty((self.num_envs,), dtype=torch.float64, device=self.device)
        acts = (torch.empty((int(n_steps), self.num_envs, 2), dtype=torch.float32, device=self.device)
                if return_actions else None)
        _capi.check(self.lib.sbr_rollout(self._h, int(n_steps), C.c_uint64(int(policy_seed)), _ptr(ret), _ptr(acts),
                                         self._stream()), self._h)
        return (ret, acts) if return_actions else ret

    def rollout_actions(self, actions, n_steps=None, hold=1, return_rewards=False):
        """Fused step() calls per env under the CALLER's actions, one launch (sbr_rollout_actions): `actions` is a tape
        [R, N, 2] (converted to the env's action dtype on the device if needed) whose row r is in force for calls r*hold ..
        r*hold + hold - 1 of this launch; n_steps defaults to R * hold.  Returns the per-env sum of this launch's rewards [N]
        float64, with return_rewards=True also the reward of every call [n_steps, N] float64 (0 for a call an env skipped
        because its episode had ended)."""
        hold = int(hold)
        a, rows, n_steps = self._tape(actions, self._ashape, n_steps, hold)
        ret = torch.empty((self.num_envs,), dtype=torch.float64, device=self.device)
        rew = torch.empty((n_steps, self.num_envs), dtype=torch.float64, device=self.device) if return_rewards else None
        _capi.check(self.lib.sbr_rollout_actions(self._h, n_steps, hold, _ptr(a) if rows else None, _ptr(ret), _ptr(rew),
                                                 self._stream()), self._h)
        return (ret, rew) if return_rewards else ret

    def lookahead(self, actions, n_steps=None, hold=1, return_rewards=False, return_best=False):
        """Read-only lookahead, one launch (sbr_lookahead_actions): `actions` is [R, N, K, 2], K candidate tapes per env (converted
        to the env's action dtype on the device if needed), each played from the env's CURRENT state with the rows held as in
        rollout_actions; n_steps defaults to R * hold.  The handle is left bit for bit as it was.  Returns the sum of this
        launch's rewards per candidate [N, K] float64; with return_rewards=True also the reward of every call [n_steps, N, K]
        float64 (0 for a call a candidate skipped because its episode had ended); with return_best=True also best_index [N]
        int32 and best_return [N] float64: per env the largest return, NaN counting as -inf, ties to the lowest index."""
        return self._lookahead(actions, n_steps, hold, return_rewards, return_best, False)

    def lookahead_end(self, actions, n_steps=None, hold=1, return_rewards=False, return_best=False):
        """lookahead that also reports where every branch ended (sbr_lookahead_actions_end), for a terminal value on top of the
        returns: lookahead's results - the same bits - followed by obs_end [N, K, 18] float32, state_end [N, K, 15] float32 and
        done_end [N, K] bool.  For a candidate whose episode has not ended the two rows are what step() returns for the
        candidate's last call (float32 whatever the handle's output dtype); for one that is done (done_end) they are zeros.
        At least one call: n_steps = 0 is refused."""
        return self._lookahead(actions, n_steps, hold, return_rewards, return_best, True)

    # the per-branch end rows of the SBROS-v1 lookaheads as (trailing shape, dtype): obs_end, state_end, done_end (bool: one byte, 0 / 1)
    _END_ROWS = (((_capi.NOBS,), torch.float32), ((_capi.NSTATE,), torch.float32), ((), torch.bool))

    def _fanout_outputs(self, fanout, n_steps, hold, return_rewards, return_best, return_end, return_actions=False,
                        actions_dtype=None, end_rows=_END_ROWS, n_scen=None, return_stats=False):
        """What a fan-out launch writes, sized once for lookahead, lookahead_sampled and lookahead_policy (and their _end forms)
        and for SBR-v2's cycle_lookahead and cycle_lookahead_scenarios.  Returns (ptrs, end_ptrs, results).  `ptrs` is in the
        ABI's order: returns, rewards, best_index, best_return and - only for a call that has the output at all, actions_dtype
        not None - actions; `end_ptrs` is one pointer per entry of `end_rows` (obs_end, state_end, done_end unless the caller
        names its own); return_end is one flag for all of them or one per entry.  An output that was not asked for is a None
        pointer.  `results` is what the method returns, in the one public order: returns, rewards, best_index, best_return,
        actions, then the end rows - those asked for.  n_scen (cycle_lookahead_scenarios): a branch is (env, candidate, future),
        so the per-branch outputs gain a trailing axis of n_scen, and mean and worst [N, K] follow the rewards in both orders;
        the winners are reduced from the means, so return_best sizes mean too."""
        n, dev = self.num_envs, self.device
        per = (n, fanout) if n_scen is None else (n, fanout, n_scen)
        ret = torch.empty(per, dtype=torch.float64, device=dev)
        rew = torch.empty((n_steps,) + per, dtype=torch.float64, device=dev) if return_rewards else None
        stats = () if n_scen is None else tuple(torch.empty((n, fanout), dtype=torch.float64, device=dev) if w else None
                                                for w in (return_stats or return_best, return_stats))
        bi = torch.empty((n,), dtype=torch.int32, device=dev) if return_best else None
        br = torch.empty((n,), dtype=torch.float64, device=dev) if return_best else None
        acts = torch.empty((-(-n_steps // hold), n, fanout, 2), dtype=actions_dtype, device=dev) if return_actions else None
        wanted = return_end if isinstance(return_end, (tuple, list)) else (return_end,) * len(end_rows)
        ends = tuple(torch.empty(per + trailing, dtype=dtype, device=dev) if w else None
                     for (trailing, dtype), w in zip(end_rows, wanted))
        outs = (ret, rew) + stats + (bi, br) + ((acts,) if actions_dtype is not None else ())
        return ([_ptr(t) for t in outs], [_ptr(t) for t in ends],
                _one_or_all(tuple(t for t in (ret, rew) + (stats if return_stats else ()) + (bi, br, acts) + ends if t is not None)))

    def _lookahead(self, actions, n_steps, hold, return_rewards, return_best, end):
        hold = int(hold)
        a, rows, n_steps = self._tape(actions, (self.num_envs, None, 2), n_steps, hold)
        fanout = int(a.shape[2])
        ptrs, end_ptrs, results = self._fanout_outputs(fanout, n_steps, hold, return_rewards, return_best, end)
        fn = self.lib.sbr_lookahead_actions_end if end else self.lib.sbr_lookahead_actions
        _capi.check(fn(self._h, n_steps, hold, fanout, _ptr(a) if rows else None, *ptrs, *(end_ptrs if end else ()),
                       self._stream()), self._h)
        return results

    def lookahead_sampled(self, nominal, fanout, sampler, n_steps=None, hold=1, return_rewards=False, return_best=False,
                          return_actions=False):
        """lookahead over SAMPLED tapes, no candidate tensor (sbr_lookahead_sampled): `nominal` is one tape [R, N, 2]; candidate k
        of an env is that tape plus the Gaussian perturbation `sampler` (a planner.TapeSampler) draws for (seed, global env id,
        k, row), clamped - drawn in the lane that integrates it.  Everything else is lookahead's, and so are the results and
        their order: returns [N, K], then the per-call rewards [n_steps, N, K] and best_index, best_return [N] if asked for; with
        return_actions=True then the candidates exactly as they were integrated [R, N, K, 2] (the rows this launch uses; fed
        to lookahead they give the same bits)."""
        return self._lookahead_sampled(nominal, fanout, sampler, n_steps, hold, return_rewards, return_best, return_actions, False)

    def lookahead_sampled_end(self, nominal, fanout, sampler, n_steps=None, hold=1, return_rewards=False, return_best=False,
                              return_actions=False):
        """lookahead_sampled that also reports where every branch ended (sbr_lookahead_sampled_end): lookahead_sampled's results -
        the same bits - followed by obs_end [N, K, 18], state_end [N, K, 15] and done_end [N, K] as lookahead_end gives them."""
        return self._lookahead_sampled(nominal, fanout, sampler, n_steps, hold, return_rewards, return_best, return_actions, True)

    def _lookahead_sampled(self, nominal, fanout, sampler, n_steps, hold, return_rewards, return_best, return_actions, end):
        hold, fanout = int(hold), int(fanout)
        a, rows, n_steps = self._tape(nominal, self._ashape, n_steps, hold)
        sm = sampler.c_struct(self.cfg)
        ptrs, end_ptrs, results = self._fanout_outputs(fanout, n_steps, hold, return_rewards, return_best, end, return_actions,
                                                       self.action_dtype)
        fn = self.lib.sbr_lookahead_sampled_end if end else self.lib.sbr_lookahead_sampled
        _capi.check(fn(self._h, n_steps, hold, fanout, _ptr(a) if rows else None, C.byref(sm), *ptrs, *(end_ptrs if end else ()),
                       self._stream()), self._h)
        return results

    def branch_best(self, values):
        """The winner among each env's K values (sbr_branch_best), under the rule of lookahead's best_*: the largest value wins,
        NaN counts as -inf, ties go to the lowest index.  `values` is [N, K] (converted to float64 on the device if needed) -
        for instance a lookahead's returns with a terminal value added.  Returns (index [N] int32, value [N] float64)."""
        shape = tuple(getattr(values, "shape", ()))
        if not (len(shape) == 2 and shape[0] == self.num_envs and shape[1] >= 1):
            raise ValueError("values must have shape [N,K] with K >= 1")
        v = self._dev(values, torch.float64, shape)
        bi = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
        bv = torch.empty((self.num_envs,), dtype=torch.float64, device=self.device)
        self._keep_a = v
        _capi.check(self.lib.sbr_branch_best(self._h, int(shape[1]), _ptr(v), _ptr(bi), _ptr(bv), self._stream()), self._h)
        return bi, bv

    def mppi_update(self, nominal, returns, sampler, temperature, shift=0, out=None, return_weights=False):
        """The MPPI update of a nominal tape (sbr_mppi_update): `nominal` [R, N, 2] and `sampler` as given to lookahead_sampled,
        `returns` [N, K] as it wrote them.  Per env the candidates - drawn again, not read - are averaged under the weights
        softmax(returns / temperature) (a NaN return weighs 0; an env without a finite maximum keeps its tape); the result,
        advanced by `shift` rows with its last row repeated, is written to `out` [R, N, 2] (a new tensor by default; out=nominal
        updates in place).  Returns out, with return_weights=True also the normalised weights [N, K] float64."""
        shape = tuple(getattr(nominal, "shape", ()))
        if not (len(shape) == 3 and shape[0] >= 1 and shape[1:] == self._ashape):
            raise ValueError("nominal must have shape [R,N,2] with R >= 1")
        a = self._as_actions(nominal, shape)
        if out is not None and a is not nominal and out is nominal:
            raise ValueError("out=nominal needs nominal as a contiguous tensor of the env's action dtype on its device")
        if not (isinstance(returns, torch.Tensor) and returns.dtype == torch.float64 and returns.device == self.device
                and returns.is_contiguous() and returns.dim() == 2 and returns.shape[0] == self.num_envs and returns.shape[1] >= 1):
            raise ValueError("returns must be a contiguous float64 tensor of shape [N,K] on %s" % self.device)
        if out is None:
            out = torch.empty_like(a)
        elif not (isinstance(out, torch.Tensor) and out.dtype == self.action_dtype and out.device == self.device
                  and out.is_contiguous() and tuple(out.shape) == shape):
            raise ValueError("out must be a contiguous %s tensor of shape %s on %s" % (self.action_dtype, shape, self.device))
        sm = sampler.c_struct(self.cfg)
        w = torch.empty_like(returns) if return_weights else None
        self._keep_a = (a, returns)
        _capi.check(self.lib.sbr_mppi_update(self._h, shape[0], int(returns.shape[1]), _ptr(a), C.byref(sm), _ptr(returns),
                                             float(temperature), int(shift), _ptr(out), _ptr(w), self._stream()), self._h)
        return (out, w) if return_weights else out

    def rollout_policy(self, policy, n_steps, hold=1, obs=None, noise_std=None, noise_seed=0, return_actions=False,
                       return_rewards=False):
        """Fused step() calls per env in CLOSED loop under `policy` (an MlpPolicy, or a population from MlpPolicy.stack), one
        launch (sbr_rollout_policy): every `hold` calls the net maps the env's float32 observation to the two set-points.
        `obs` [N, 18] float32 is the observation in force and is updated in place for every env that is not done afterwards;
        obs=None uses self.obs (converted to float32 and back if the handle's outputs are float64).  noise_std (a number or a
        pair) adds Gaussian exploration noise keyed by noise_seed, the global env id and the env's call count.  Returns the
        per-env sum of this launch's rewards [N] float64, then - if asked for - the decisions [ceil(n_steps/hold), N, 2]
        float32 (exactly the values that were integrated; 0 where an env had finished) and the reward of every call
        [n_steps, N] float64."""
        n_steps, hold = int(n_steps), int(hold)
        n = self.num_envs
        o, pol = self._policy_inputs(policy, n_steps, hold, obs, noise_std, noise_seed)
        ret = torch.empty((n,), dtype=torch.float64, device=self.device)
        acts = torch.empty((-(-n_steps // hold), n, 2), dtype=torch.float32, device=self.device) if return_actions else None
        rew = torch.empty((n_steps, n), dtype=torch.float64, device=self.device) if return_rewards else None
        _capi.check(self.lib.sbr_rollout_policy(self._h, n_steps, hold, C.byref(pol), _ptr(o), _ptr(ret), _ptr(acts), _ptr(rew),
                                                self._stream()), self._h)
        self._policy_obs_back(obs, o)
        return _one_or_all((ret,) + ((acts,) if return_actions else ()) + ((rew,) if return_rewards else ()))

    def _policy_inputs(self, policy, n_steps, hold, obs, noise_std, noise_seed, in_place=True):
        """What rollout_policy, collect_policy and lookahead_policy hand the library: the observation (obs=None: self.obs, as
        float32) and the sbr_policy struct.  in_place: the launch writes the observation (lookahead_policy only reads it)."""
        if hold < 1:
            raise ValueError("hold must be >= 1")
        if n_steps < 0:
            raise ValueError("n_steps must be >= 0")
        own = obs is None
        o = self.obs if own else obs
        if own and o.dtype != torch.float32:
            o = o.to(torch.float32)
        if not (isinstance(o, torch.Tensor) and o.dtype == torch.float32 and o.device == self.device and o.is_contiguous()
                and tuple(o.shape) == (self.num_envs, _capi.NOBS)):
            raise ValueError("obs must be a contiguous float32 tensor of shape [N,%d] on %s%s"
                             % (_capi.NOBS, self.device, " (it is updated in place)" if in_place else ""))
        pol = policy.c_struct(self.device, noise_std=noise_std, noise_seed=noise_seed)
        self._keep_p = (policy, pol, o)
        return o, pol

    def _policy_obs_back(self, obs, o):
        if obs is None and o is not self.obs:   # a float64 handle: the rows of the envs that are not done come back, the others stay
            live = self.ctrl_row(_capi.C_DONE) == 0
            self.obs.copy_(torch.where(live[:, None], o.to(self.obs.dtype), self.obs))

    def collect_policy(self, policy, n_steps, hold=1, obs=None, noise_std=None, noise_seed=0):
        """rollout_policy as a COLLECTOR, one launch (sbr_collect_policy): the same calls with the same bits in the handle, `obs`
        and every shared result, plus what a gradient-based learner needs of every decision d (rows = ceil(n_steps/hold) of
        them).  `policy`, `hold`, `obs` (obs=None: self.obs), noise_std and noise_seed are rollout_policy's.  Returns a
        PolicyCollection:
          obs      [rows, N, 18] float32  the observation the net was applied to at decision d (zeros where the env had finished)
          actions  [rows, N, 2]  float32  the decisions exactly as they were integrated (0 where the env had finished)
          rewards  [n_steps, N]  float64  the reward of every call
          flags    [rows, N]     uint8    _capi.DF_TAKEN | _capi.DF_ENDED; .taken and .ended are the two bits as bool tensors
          returns  [N]           float64  the sum of this launch's rewards
          last_obs [N, 18]       float32  the in/out observation after the launch, for bootstrapping
        The action mean of a decision is the net applied to its row of `obs`; a learner recomputes it under autograd."""
        return self._collect(self.lib.sbr_collect_policy, (), policy, n_steps, hold, obs, noise_std, noise_seed)

    def _collect(self, fn, lead, policy, n_steps, hold, obs, noise_std, noise_seed):
        """collect_policy and collect_policy_models: the outputs sized once, `lead` what the entry point takes behind the handle."""
        n_steps, hold = int(n_steps), int(hold)
        n, dev = self.num_envs, self.device
        o, pol = self._policy_inputs(policy, n_steps, hold, obs, noise_std, noise_seed)
        rows = -(-n_steps // hold)
        ret = torch.empty((n,), dtype=torch.float64, device=dev)
        acts = torch.empty((rows, n, 2), dtype=torch.float32, device=dev)
        rew = torch.empty((n_steps, n), dtype=torch.float64, device=dev)
        obs_out = torch.empty((rows, n, _capi.NOBS), dtype=torch.float32, device=dev)
        # (a tensor without elements reports a NULL pointer, and the library refuses the call without either per-decision output:
        # with n_steps = 0 the flags are the zero rows of a one-row buffer, which is not written)
        flags = torch.empty((max(rows, 1), n), dtype=torch.uint8, device=dev)
        _capi.check(fn(self._h, *lead, n_steps, hold, C.byref(pol), _ptr(o), _ptr(ret), _ptr(acts), _ptr(rew), _ptr(obs_out),
                       _ptr(flags), self._stream()), self._h)
        self._policy_obs_back(obs, o)
        return PolicyCollection(obs_out, acts, rew, flags[:rows], ret, o)

    # ------------------------------------------------------------------ domain-randomised episodes: per-env plant models
    def set_models(self, models):
        """The handle's table of plant MODELS (sbr_set_models): `models` is a models.PlantModels or a sequence of _capi.SbrConfig
        that differ from the env's config in the model fields only (models.MODEL_FIELDS); None or an empty sequence drops the
        table.  Replaces an earlier table, waiting for the device first.  Only reset_models, collect_policy_models,
        rollout_policy_models (a plant per env) and lookahead_models, lookahead_sampled_models (every env under every model) read
        it: reset(), step() and every other call keep integrating the env's own config."""
        from .models import set_table
        set_table(self, models)

    @property
    def num_models(self):
        """Models in the handle's table (sbr_num_models); 0 if none is set."""
        from .models import table_size
        return table_size(self)

    def model_index(self, envs_per_model):
        """The plant of every env under THE RULE of reset_models / collect_policy_models, [N] int64, evaluated on the host: the env
        with global id g = first_env_id + i is model (g // envs_per_model) % num_models.  With one model envs_per_model is not read.
        ValueError where the library would refuse the rule: no table, or - with more than one model - envs_per_model or
        first_env_id not a (positive) multiple of 256."""
        m = int(self.num_models)
        if m < 1:
            raise ValueError("no model table: call set_models first")
        if m == 1:
            return torch.zeros((self.num_envs,), dtype=torch.int64)
        per = int(envs_per_model)
        if per < 256 or per % 256 or self.first_env_id < 0 or self.first_env_id % 256:
            raise ValueError("with more than one model envs_per_model must be a positive multiple of 256 and first_env_id a "
                             "non-negative multiple of 256")
        return torch.div(self.first_env_id + torch.arange(self.num_envs, dtype=torch.int64), per, rounding_mode="floor") % m

    def reset_models(self, envs_per_model, seed=0, scenario=None, rnd=None, influent=None, mask=None, carry_over=False):
        """reset() over DOMAIN-RANDOMISED envs, one launch (sbr_reset_models): env i starts its episode as plant model_index(
        envs_per_model)[i] of the table set_models() gave the handle - the fill phase, the status bits and the observation are
        that model's, bit for bit what a handle created with the model's config returns.  Every argument but envs_per_model is
        reset()'s."""
        ins = self._reset_inputs(scenario, rnd, influent, mask)
        with torch.cuda.device(self.device):
            _capi.check(self.lib.sbr_reset_models(self._h, int(envs_per_model), 1 if carry_over else 0, C.c_uint64(int(seed)), *ins,
                                                  _ptr(self.obs), self._stream()), self._h)
        return self.obs

    def collect_policy_models(self, policy, n_steps, envs_per_model, hold=1, obs=None, noise_std=None, noise_seed=0):
        """collect_policy over DOMAIN-RANDOMISED envs, one launch (sbr_collect_policy_models): env i runs its calls as plant
        model_index(envs_per_model)[i] of the handle's table - intervals, reward, status thresholds, step plan and terminal phases
        are that model's - and every bit of the handle and of the PolicyCollection is what a handle created with the model's
        config gives through collect_policy.  A population and the table vary independently.  Arguments otherwise, and the
        result, are collect_policy's."""
        return self._collect(self.lib.sbr_collect_policy_models, (int(envs_per_model),), policy, n_steps, hold, obs, noise_std,
                             noise_seed)

    def rollout_policy_models(self, policy, n_steps, envs_per_model, hold=1, obs=None, noise_std=None, noise_seed=0,
                              return_actions=False, return_rewards=False):
        """rollout_policy over DOMAIN-RANDOMISED envs (collect_policy_models' entry point without its two per-decision outputs):
        rollout_policy's arguments plus envs_per_model, rollout_policy's results."""
        n_steps, hold = int(n_steps), int(hold)
        n = self.num_envs
        o, pol = self._policy_inputs(policy, n_steps, hold, obs, noise_std, noise_seed)
        ret = torch.empty((n,), dtype=torch.float64, device=self.device)
        acts = torch.empty((-(-n_steps // hold), n, 2), dtype=torch.float32, device=self.device) if return_actions else None
        rew = torch.empty((n_steps, n), dtype=torch.float64, device=self.device) if return_rewards else None
        _capi.check(self.lib.sbr_collect_policy_models(self._h, int(envs_per_model), n_steps, hold, C.byref(pol), _ptr(o), _ptr(ret),
                                                       _ptr(acts), _ptr(rew), None, None, self._stream()), self._h)
        self._policy_obs_back(obs, o)
        return _one_or_all((ret,) + ((acts,) if return_actions else ()) + ((rew,) if return_rewards else ()))

    # ------------------------------------------------------------------ lookahead under uncertain plant kinetics: K tapes x M models
    def _models_branches(self, fanout):
        """M of a lookahead over (env, candidate, model) branches, checked before any output is sized by it."""
        m = int(self.num_models)
        if m < 1:
            raise ValueError("no model table: call set_models first")
        if fanout >= 1 and self.num_envs * fanout * m >= 2 ** 31:
            raise ValueError("num_envs * K * num_models must stay below 2^31")
        return m

    def lookahead_models(self, actions, n_steps=None, hold=1, return_rewards=False, return_stats=False, return_best=False):
        """lookahead under UNCERTAIN PLANT KINETICS, one launch (sbr_lookahead_actions_models): `actions` is [R, N, K, 2] as for
        lookahead, and every candidate of every env is played from the env's CURRENT state under EVERY model of the table
        set_models() gave the handle - branch (i, k, m) under the constants of model m.  The env's own config is integrated by no
        branch (put it into the table to have the nominal plant among the models); the handle is left bit for bit as it was.
        Returns the sum of this launch's rewards per branch [N, K, M] float64 - column m is, bit for bit, what lookahead returns
        on a handle created with model m's config that holds the env's state - then, in this order and only if asked for: the
        reward of every call [n_steps, N, K, M] (a strided store on the device: ask for it when it is needed); mean and worst
        [N, K], the mean over m (summed in m order, one division) and the smallest of a candidate's M returns, NaN if one of them
        is; best_index [N] int32 and best_value [N] float64, the winner among an env's means (lookahead's rule).  No _end form."""
        hold = int(hold)
        a, rows, n_steps = self._tape(actions, (self.num_envs, None, 2), n_steps, hold)
        fanout = int(a.shape[2])
        m = self._models_branches(fanout)
        ptrs, _, results = self._fanout_outputs(fanout, n_steps, hold, return_rewards, return_best, False, n_scen=m,
                                                return_stats=return_stats)
        _capi.check(self.lib.sbr_lookahead_actions_models(self._h, n_steps, hold, fanout, _ptr(a) if rows else None, *ptrs,
                                                          self._stream()), self._h)
        return results

    def lookahead_sampled_models(self, nominal, fanout, sampler, n_steps=None, hold=1, return_rewards=False, return_stats=False,
                                 return_best=False, return_actions=False):
        """lookahead_models over SAMPLED tapes (sbr_lookahead_sampled_models): `nominal` [R, N, 2] and `sampler` as for
        lookahead_sampled.  Candidate k of an env is keyed by (seed, global env id, k, row) and NOT by the model: all M models of
        a candidate play the same tape (common random numbers), so two models differ by the plant and not by what they drew.
        Results and their order are lookahead_models' - returns [N, K, M], column m the bits of lookahead_sampled on a handle
        created with model m's config; rewards; mean, worst; best_index, best_value - then with return_actions=True the
        candidates exactly as they were integrated [R, N, K, 2] (fed to lookahead_models they give the same bits)."""
        hold, fanout = int(hold), int(fanout)
        a, rows, n_steps = self._tape(nominal, self._ashape, n_steps, hold)
        m = self._models_branches(fanout)
        sm = sampler.c_struct(self.cfg)
        ptrs, _, results = self._fanout_outputs(fanout, n_steps, hold, return_rewards, return_best, False, return_actions,
                                                self.action_dtype, n_scen=m, return_stats=return_stats)
        _capi.check(self.lib.sbr_lookahead_sampled_models(self._h, n_steps, hold, fanout, _ptr(a) if rows else None, C.byref(sm),
                                                          *ptrs, self._stream()), self._h)
        return results

    def lookahead_policy(self, policy, fanout, n_steps, hold=1, obs=None, noise_std=None, noise_seed=0, keep_mean=False,
                         return_rewards=False, return_best=False, return_actions=False, return_end=False):
        """Read-only lookahead in CLOSED loop, one launch (sbr_lookahead_policy): `fanout` rollouts of `policy` (an MlpPolicy or
        a population) per env, each from the env's CURRENT state and its row of `obs` [N, 18] float32 (obs=None: self.obs,
        converted to float32 if the handle's outputs are float64), decisions every `hold` calls as in rollout_policy.  The handle
        and obs are left bit for bit as they were; nothing is copied back.  With noise_std, branch k of an env draws noise of its
        own, keyed by noise_seed, the global env id, k and the branch's call count - branch 0 what rollout_policy would draw;
        keep_mean=True runs branch 0 of every env without noise.  Returns the sum of this launch's rewards per branch [N, K]
        float64, then, in this order and only if asked for: the reward of every call [n_steps, N, K] float64; best_index [N]
        int32 and best_return [N] float64 (lookahead's rule); the decisions [ceil(n_steps/hold), N, K, 2] float32 exactly as
        they were integrated (fed to lookahead they give the same bits); obs_end [N, K, 18], state_end [N, K, 15] and done_end
        [N, K] as lookahead_end gives them (n_steps = 0 is then refused)."""
        n_steps, hold, fanout = int(n_steps), int(hold), int(fanout)
        if fanout < 1 or fanout > 2 ** 24 or self.num_envs * fanout >= 2 ** 31:      # before the outputs are sized by it
            raise ValueError("fanout must be in 1 .. 2^24 with num_envs * fanout below 2^31")
        o, pol = self._policy_inputs(policy, n_steps, hold, obs, noise_std, noise_seed, in_place=False)
        ptrs, end_ptrs, results = self._fanout_outputs(fanout, n_steps, hold, return_rewards, return_best, return_end,
                                                       return_actions, torch.float32)
        _capi.check(self.lib.sbr_lookahead_policy(self._h, n_steps, hold, fanout, C.byref(pol), 1 if keep_mean else 0, _ptr(o),
                                                  *ptrs, *end_ptrs, self._stream()), self._h)
        return results

    def enable_trace(self, n_envs=1, capacity=463):
        """Trajectory export: every step() appends one record (_capi.TR_*: t, x(14), Kla, EC, reward, done, the set-points in
        force, the NO3-PID's e/ie/dcv and the four reward diagnostics) for the first n_envs envs at index = calls since
        reset.  Returns the buffer [capacity, NTRACE, n_envs] float64 (NaN where nothing was written)."""
        self._trace = torch.full((int(capacity), _capi.NTRACE, int(n_envs)), float("nan"), dtype=torch.float64,
                                 device=self.device)
        _capi.check(self.lib.sbr_set_trace(self._h, _ptr(self._trace), int(n_envs), int(capacity), _capi.NTRACE), self._h)
        return self._trace

    def disable_trace(self):
        _capi.check(self.lib.sbr_set_trace(self._h, None, 0, 0, _capi.NTRACE), self._h)
        self._trace = None

    # ------------------------------------------------------------------ inspection / parity injection
    def get_state(self):
        x = torch.empty((_capi.NX, self.num_envs), dtype=torch.float64, device=self.device)
        ctrl = torch.empty((_capi.NCTRL, self.num_envs), dtype=torch.float64, device=self.device)
        _capi.check(self.lib.sbr_get_state(self._h, _ptr(x), _ptr(ctrl), self._stream()), self._h)
        return x, ctrl

    def set_state(self, x=None, ctrl=None):
        x = self._dev(x, torch.float64, (_capi.NX, self.num_envs))
        ctrl = self._dev(ctrl, torch.float64, (_capi.NCTRL, self.num_envs))
        _capi.check(self.lib.sbr_set_state(self._h, _ptr(x), _ptr(ctrl), self._stream()), self._h)
        torch.cuda.current_stream(self.device).synchronize()

    def influent(self):
        out = torch.empty((_capi.NX, self.num_envs), dtype=torch.float64, device=self.device)
        _capi.check(self.lib.sbr_get_influent(self._h, _ptr(out), self._stream()), self._h)
        return out

    def query(self, what):
        """One of the library's own decisions for this handle (sbr_query, _capi.Q_*): launch shapes and their thresholds, which
        depend on the device's CU count."""
        out = C.c_int64()
        _capi.check(self.lib.sbr_query(self._h, int(what), C.byref(out)), self._h)
        return int(out.value)

    def plan(self, out=None):
        """What cfg.scheme = 1 did in each env's last control interval ([N] int64): Butcher-5 step count (& 127) and
        _capi.PLAN_SLAVED if dissolved oxygen was held.  0 = nothing to report (cfg.scheme 0, or no step() since the reset)."""
        return self.ctrl_row(_capi.C_PLAN, out).to(torch.int64)

    def status(self):
        """Sticky domain-of-validity bits per env (int64; _capi.ST_NEGATIVE | ST_NEAR_POLE | ST_NONFINITE): the
        reference model has no guards and can be driven to negative ammonia / a Monod pole by aggressive policies."""
        return self.ctrl_row(_capi.C_STATUS).to(torch.int64)

    def ctrl_row(self, row, out=None):
        """One row of the controller/bookkeeping block ([N] float64), copied on the current stream without a host sync."""
        if out is None:
            out = torch.empty((self.num_envs,), dtype=torch.float64, device=self.device)
        _capi.check(self.lib.sbr_get_ctrl_row(self._h, int(row), _ptr(out), self._stream()), self._h)
        return out

    def episode_returns(self, out=None):
        """Sum of rewards since reset, per env ([N] float64)."""
        return self.ctrl_row(_capi.C_RETURN, out)

    def stats(self, values):
        v = self._dev(values, torch.float64, (values.numel(),))
        out = torch.empty((4,), dtype=torch.float64, device=self.device)
        _capi.check(self.lib.sbr_reduce_stats(self._h, _ptr(v), v.numel(), _ptr(out), self._stream()), self._h)
        s, mn, mx, cnt = out.tolist()
        return {"sum": s, "min": mn, "max": mx, "count": cnt, "mean": s / cnt if cnt else float("nan")}

    def eval_rhs(self, kind, x, kla, ec, loading=None):
        x = torch.as_tensor(x, dtype=torch.float64, device=self.device).contiguous()
        n = x.shape[0]
        kla = self._dev(kla, torch.float64, (n,))
        ec = self._dev(ec, torch.float64, (n,))
        ld = self._dev(loading, torch.float64, (n, _capi.NX))
        dx = torch.empty_like(x)
        _capi.check(self.lib.sbr_eval_rhs(self._h, int(kind), n, _ptr(x), _ptr(kla), _ptr(ec), _ptr(ld), _ptr(dx),
                                          self._stream()), self._h)
        return dx

    def eval_substeps(self, x0, kla, h, ec=None, loading=None, kind=0, n_sub=None):
        """RK4 nodes and node slopes of n independent integration spans (sbr_eval_substeps): x0 [n,14], kla / h [n] (h = substep
        length) -> xs, dxs [n, n_sub + 1, 14] float64.  kind 0 control interval (ec [n]; n_sub defaults to cfg.substeps), 1 fill
        (loading [n,14]), 2 idle, 3 settle + draw, then idle.  For trajectory export (SbrOS.trajectory(dense=True))."""
        x0 = torch.as_tensor(x0, dtype=torch.float64, device=self.device).contiguous()
        n = x0.shape[0]
        n_sub = int(self.cfg.substeps if n_sub is None else n_sub)
        kla, h = self._dev(kla, torch.float64, (n,)), self._dev(h, torch.float64, (n,))
        ec = self._dev(ec, torch.float64, (n,))
        ld = self._dev(loading, torch.float64, (n, _capi.NX))
        xs = torch.empty((n, n_sub + 1, _capi.NX), dtype=torch.float64, device=self.device)
        dxs = torch.empty_like(xs)
        _capi.check(self.lib.sbr_eval_substeps(self._h, int(kind), n, n_sub, _ptr(x0), _ptr(kla), _ptr(ec), _ptr(ld), _ptr(h),
                                               _ptr(xs), _ptr(dxs), self._stream()), self._h)
        return xs, dxs

    def draw_scenarios(self, seed):
        """The scenario every env draws at reset(seed, scenario=None) when the config has random_scenario = 1 ([N] int32)."""
        out = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
        _capi.check(self.lib.sbr_draw_scenarios(self._h, C.c_uint64(int(seed)), _ptr(out), self._stream()), self._h)
        return out

    def draw_normals(self, seed):
        out = torch.empty((self.num_envs, _capi.NSAMP), dtype=torch.float64, device=self.device)
        _capi.check(self.lib.sbr_draw_normals(self._h, C.c_uint64(int(seed)), _ptr(out), self._stream()), self._h)
        return out

    # ------------------------------------------------------------------ device timing (bench.py)
    def timer_start(self):
        _capi.check(self.lib.sbr_timer_start(self._h, self._stream()), self._h)

    def timer_stop(self):
        ms = C.c_float()
        _capi.check(self.lib.sbr_timer_stop(self._h, self._stream(), C.byref(ms)), self._h)
        return float(ms.value)
