"""k_step's one-wave scheme-1 builds mark their rare branches unlikely (profiles/r22_notes.md), which moves those blocks out of the
ordinary call's fall-through code: the direct-form output stores of ragged or misaligned waves, the dependent fetch of the
So[-1] / Sno[-1] rows, the per-lane ring form, the second and third ring append, the trace export - and changes where the terminal
phases are entered from.  Every one of them still does its job: call by call against the oracle from identical states, with the
gates of tests/test_step_spill_gpu.py (which are tests/test_gpu_parity.py's), at the smallest shapes that reach each block."""
import ctypes as C

import numpy as np
import pytest
from gpu_common import package, to_np

import test_step_spill_gpu as base            # check_call and the physical policy's actions: the module, so that its tests are not collected twice
from oracle import sbr_oracle as O  # the checker, never the thing under test

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return package()


def test_small_build_misaligned_traced_and_partly_reset_against_the_oracle(G, tables):
    """130 envs (64-thread build: two full waves and a ragged one), observation and state rows written 4 bytes off a 16-byte
    boundary (every wave takes the direct form), a trace buffer on, and every third lane reset again after call 20 (no wave's ring
    slot is uniform from there on; those lanes fetch their m1 rows again).  A whole episode of the lanes not reset: the first call
    after a reset, the double steps 51 and 275, the done call 462 with its terminal phases (the lanes reset again are 21 calls behind
    and do not end: a done call of part of a wave)."""
    import torch
    from gym_sbr2_amd import _capi
    means, stds = tables
    n, nt, shift = 130, 70, 1
    rs = np.random.RandomState(2201)
    scen = (4 + np.arange(n) % 4).astype(np.int32)
    rnd = rs.randn(n, 48)
    late = (np.arange(n) % 3 == 1)
    env = G.SbrOSVec(n, out_dtype=torch.float32)
    tr = env.enable_trace(n_envs=nt, capacity=470)
    ora = O.OracleBatch(n)
    env.reset(scenario=scen, rnd=rnd)
    ora.reset(ora.mix(means, stds, scen, rnd))
    obs = torch.full((n * 18 + 8,), -7.0, device="cuda")
    st = torch.full((n * 15 + 8,), -7.0, device="cuda")
    worst, done_at, two = 0.0, {}, []
    for c in range(463):
        if c == 21:
            env.reset(scenario=scen, rnd=rnd, mask=late.astype(np.uint8))
        a = base.actions(rs, n)
        x, ctrl = env.get_state()
        xb, cb = to_np(x).copy(), to_np(ctrl).copy()
        at = torch.from_numpy(a).cuda()
        rc = env.lib.sbr_step(env._h, C.c_void_p(at.data_ptr()), C.c_void_p(obs.data_ptr() + 4 * shift), C.c_void_p(st.data_ptr() + 4 * shift),
                              C.c_void_p(env.reward.data_ptr()), C.c_void_p(env.done.data_ptr()), None)
        assert rc == 0, c
        torch.cuda.synchronize()
        o_, s_ = to_np(obs), to_np(st)
        assert (o_[:shift] == -7).all() and (o_[shift + n * 18:] == -7).all() and (s_[:shift] == -7).all() and (s_[shift + n * 15:] == -7).all(), c
        o, s = o_[shift:shift + n * 18].reshape(n, 18).copy(), s_[shift:shift + n * 15].reshape(n, 15).copy()
        r, d = to_np(env.reward).copy(), to_np(env.done).copy()
        x, ctrl = env.get_state()
        xa, ca = to_np(x).copy(), to_np(ctrl).copy()
        g, _ = base.check_call(c, ora, (c, a, xb, cb, o, s, r, d, xa, ca))
        worst = max(worst, g)
        for i in np.nonzero(d)[0]:
            done_at.setdefault(int(i), c)
        if c == 0:
            dt0 = (ca[_capi.C_T] - cb[_capi.C_T]).max()
        elif np.all((ca[_capi.C_T] - cb[_capi.C_T])[~late] > 1.5 * dt0):
            two.append(c)
        if c <= 20:                                   # the trace record of this call (every lane's step count is still c)
            t = to_np(tr)
            assert np.array_equal(t[c, _capi.TR_REWARD, :].astype(np.float32), r[:nt]), c        # the record holds the float64 reward
            assert np.array_equal(t[c, _capi.TR_X0:_capi.TR_X0 + 14, :], xa[:, :nt]) and np.array_equal(t[c, _capi.TR_T, :], ca[_capi.C_T, :nt]), c
    assert two[:2] == [51, 275], two
    assert sorted(done_at) == list(np.nonzero(~late)[0]) and set(done_at.values()) == {462}, sorted(set(done_at.values()))
    assert np.abs(ca[_capi.C_QW][~late] / ora.envs["qw"][~late] - 1).max() < 1e-9          # the terminal phases ran for the lanes that ended
    t, lt = to_np(tr), late[:nt]                         # a record per call and lane: 463 of the lanes not reset again, 463 - 21 of the others
    assert np.isfinite(t[:463][:, :, ~lt]).all() and np.isfinite(t[:442][:, :, lt]).all()
    print("64-thread build, misaligned rows, trace on, masked reset, 463 calls in lockstep: worst gate %.3e" % worst)
    env.disable_trace(); env.close()


def test_wide_build_around_the_first_phase_boundary_against_the_oracle(G, tables):
    """49 408 envs = 193 x 256 (the 256-thread build, every wave full and aligned: the staged 16-byte stores), calls 46 - 56 in
    lockstep: anoxic calls, the double step 51, the first aerobic ones."""
    import torch
    from gym_sbr2_amd import _capi
    means, stds = tables
    n = 193 * 256
    rs = np.random.RandomState(2202)
    scen = (4 + np.arange(n) % 4).astype(np.int32)
    rnd = rs.randn(n, 48)
    env = G.SbrOSVec(n, out_dtype=torch.float32)
    ora = O.OracleBatch(n, nthreads=8)
    env.reset(scenario=scen, rnd=rnd)
    ora.reset(ora.mix(means, stds, scen, rnd))
    worst, spans = 0.0, []
    for c in range(57):
        a = base.actions(rs, n)
        if c < 46:                                    # on the device alone up to the boundary's neighbourhood
            env.step(torch.from_numpy(a).cuda())
            continue
        x, ctrl = env.get_state()
        xb, cb = to_np(x).copy(), to_np(ctrl).copy()
        o, s, r, d = env.step(torch.from_numpy(a).cuda())
        x, ctrl = env.get_state()
        ca = to_np(ctrl)
        g, _ = base.check_call(c, ora, (c, a, xb, cb, to_np(o), to_np(s), to_np(r), to_np(d), to_np(x), ca))
        worst = max(worst, g)
        spans.append(float((ca[_capi.C_T] - cb[_capi.C_T]).min()))
    assert int(ca[_capi.C_STEPS].min()) == 57
    assert spans[5] > 1.5 * spans[0] and spans[6] < 1.5 * spans[0], spans            # call 51 ran two intervals
    print("256-thread build, 49408 envs, calls 46-56 in lockstep: worst gate %.3e" % worst)
    env.close()
