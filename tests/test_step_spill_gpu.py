"""k_step reads its constants and pointers again behind the step loops instead of keeping them across (profiles/r12_notes.md): the
results must not move by a bit.  The two one-wave builds against the oracle, call by call in lockstep (the oracle is set to the
device's own state before each call), and the 64-thread build against arrays the PARENT commit's library wrote on the device
(tests/golden/step_spill_parent.npz: the same 130 envs, the same actions, after calls 50, 51, 52, 275 and 462)."""
import os

import numpy as np
import pytest
from conftest import GOLDEN, gate
from gpu_common import package, plans_agree, to_np

from oracle import sbr_oracle as O  # the checker, never the thing under test

pytestmark = pytest.mark.gpu

GOLDEN_CALLS = (50, 51, 52, 275, 462)         # around the first double step, the second one, the done call
ROWS = (("so_m1", "C_SO_M1"), ("so_m2", "C_SO_M2"), ("sno_m1", "C_SNO_M1"), ("sno_m2", "C_SNO_M2"), ("ie_do", "C_IE_DO"),
        ("ie_ec", "C_IE_EC"), ("ec_last", "C_EC_LAST"), ("kla_last", "C_KLA_LAST"))


@pytest.fixture(scope="module")
def G():
    return package()


def actions(rs, n):
    """One call's float32 actions under the physical policy: u_DO ~ U[0, 2.5], u_EC ~ U[0, 15]."""
    return np.column_stack([rs.uniform(0, 2.5, n), rs.uniform(0, 15, n)]).astype(np.float32)


def episode130(G):
    """130 envs (two full waves and a two-lane one: the 64-thread build), float32 in and out, a whole episode and ten calls after
    a reset.  Yields ("reset", scenario, rnd, obs) and per call (index, actions, x and ctrl before, obs, state, reward, done, x and
    ctrl after).  Seeds and order of the draws are part of the fixture under tests/golden/."""
    import torch
    n = 130
    rs = np.random.RandomState(1212)
    scen = (4 + np.arange(n) % 4).astype(np.int32)
    env = G.SbrOSVec(n, out_dtype=torch.float32)
    call = 0
    for calls in (463, 10):
        rnd = rs.randn(n, 48)
        obs0 = to_np(env.reset(scenario=scen, rnd=rnd)).copy()
        yield ("reset", scen, rnd, obs0)
        for _ in range(calls):
            a = actions(rs, n)
            x, ctrl = env.get_state()
            xb, cb = to_np(x).copy(), to_np(ctrl).copy()
            o, s, r, d = env.step(torch.from_numpy(a).cuda())
            x, ctrl = env.get_state()
            yield (call, a, xb, cb, to_np(o).copy(), to_np(s).copy(), to_np(r).copy(), to_np(d).copy(), to_np(x).copy(), to_np(ctrl).copy())
            call += 1
    env.close()


def check_call(c, ora, rec):
    """One call from identical states, at the tolerances of tests/test_gpu_parity.py (its 4096-env lockstep episode for the plant and
    the float32 outputs, its perturbed-constants episode for the controller rows)."""
    from gym_sbr2_amd import _capi
    _, a, xb, cb, o, s, r, d, x, ctrl = rec
    ora.load_state(xb, cb)
    oo, os_, orr, od = ora.step(a.astype(np.float64))
    assert np.array_equal(d, od), c
    assert np.array_equal(ctrl[_capi.C_STATUS], ora.envs["status"]), c
    g = gate(x.T, ora.envs["x"]).max()
    assert g < 1e-6, (c, g)
    assert np.allclose(o, oo, rtol=2e-7, atol=1e-7) and np.allclose(s, os_, rtol=2e-7, atol=1e-7), c
    assert np.allclose(r, orr, rtol=2e-7, atol=1e-10), c
    assert np.array_equal(ctrl[_capi.C_T], ora.envs["t"]), c
    for key, row in ROWS:
        assert np.allclose(ctrl[getattr(_capi, row)], ora.envs[key], rtol=1e-9, atol=1e-12), (c, key)
    assert np.abs(ctrl[_capi.C_KLA_HIST0:_capi.C_KLA_HIST0 + 10].T - ora.envs["kla_hist"]).max() < 1e-9, c
    assert np.abs(ctrl[_capi.C_RETURN] - ora.envs["ret"]).max() < 1e-12, c
    assert np.array_equal(ctrl[_capi.C_DONE], d.astype(np.float64)) and np.array_equal(ctrl[_capi.C_STEPS], cb[_capi.C_STEPS] + 1), c
    if od.all():
        assert np.abs(ctrl[_capi.C_QW] / ora.envs["qw"] - 1).max() < 1e-9, c
    plans_agree(ctrl, ora)
    return g, int(ora.envs["scheme_plan"].max()) & 127


@pytest.fixture(scope="module")
def run130(G):
    return list(episode130(G))


def test_small_build_whole_episode_and_after_a_reset_against_the_oracle(run130, tables):
    """(i) every call of the episode and of the ten behind the reset: obs, state, reward, done, plant and controller rows (SBR_C_PLAN
    included; SBR_C_KLA_SUM is the OCI reward's row, which these kernels do not carry).  Calls 51 and 275 run two intervals, 462
    is the done call."""
    means, stds = tables
    ora = O.OracleBatch(130)
    worst, done_calls, n_call = 0.0, [], 0
    for rec in run130:
        if rec[0] == "reset":
            _, scen, rnd, obs0 = rec
            oobs = ora.reset(ora.mix(means, stds, scen, rnd))
            assert np.abs(obs0 - oobs).max() < 1e-5
            continue
        g, _ = check_call(rec[0], ora, rec)
        worst = max(worst, g)
        if rec[7].all():
            done_calls.append(rec[0])
        n_call += 1
    assert n_call == 473 and done_calls == [462], done_calls
    two = [rec[0] for rec in run130 if rec[0] != "reset" and rec[0] < 463 and
           np.all(rec[9][0] - rec[3][0] > 1.5 * (run130[1][9][0] - run130[1][3][0]))]
    assert two[:2] == [51, 275], two                                  # the double steps are where the fixture says they are
    print("64-thread build, 473 calls in lockstep: worst gate %.3e" % worst)


def test_small_build_is_bit_identical_to_the_parent_commit(run130):
    """(iii) array_equal against what the parent commit's library produced on the device for the same envs and actions."""
    g = np.load(os.path.join(GOLDEN, "step_spill_parent.npz"))
    by_call = {rec[0]: rec for rec in run130 if rec[0] != "reset"}
    for c in GOLDEN_CALLS:
        _, a, xb, cb, o, s, r, d, x, ctrl = by_call[c]
        for name, got in (("obs", o), ("state", s), ("reward", r), ("done", d), ("x", x), ("ctrl", ctrl), ("action", a)):
            ref = g["%s_%d" % (name, c)]
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (c, name)


def test_wide_build_with_a_partial_last_wave_against_the_oracle(G, tables):
    """(ii) 49 216 envs: the smallest batch above SBR_SMALL_BATCH (256-thread workgroups) whose last wave is not full; calls 0-60,
    across the first phase boundary."""
    import torch
    from gym_sbr2_amd import _capi
    means, stds = tables
    n = 49152 + 64
    rs = np.random.RandomState(1213)
    scen = (4 + np.arange(n) % 4).astype(np.int32)
    rnd = rs.randn(n, 48)
    env = G.SbrOSVec(n, out_dtype=torch.float32)
    ora = O.OracleBatch(n, nthreads=8)
    obs0 = to_np(env.reset(scenario=scen, rnd=rnd))
    assert np.abs(obs0 - ora.reset(ora.mix(means, stds, scen, rnd))).max() < 1e-5
    worst = 0.0
    for c in range(61):
        a = actions(rs, n)
        x, ctrl = env.get_state()
        xb, cb = to_np(x).copy(), to_np(ctrl).copy()
        o, s, r, d = env.step(torch.from_numpy(a).cuda())
        x, ctrl = env.get_state()
        g, _ = check_call(c, ora, (c, a, xb, cb, to_np(o), to_np(s), to_np(r), to_np(d), to_np(x), to_np(ctrl)))
        worst = max(worst, g)
    assert int(to_np(ctrl)[_capi.C_STEPS].min()) == 61
    print("256-thread build, 49216 envs, 61 calls in lockstep: worst gate %.3e" % worst)
    env.close()
