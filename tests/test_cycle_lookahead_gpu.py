"""sbr_cycle_lookahead / SbrEnv2Vec.cycle_lookahead on the GPU: K tapes of whole cycles per env, each played from the live
handle's current state and stored influent, the handle left bit for bit as it was.

The checker of the bit-equality tests is the EXISTING per-cycle kernel on a second handle of N*K envs (cycle_kit.replicas with
the one future there is), driven through the existing API only: set_state with the live handle's get_state() columns repeated K
times, reset(influent = the live handle's, repeated, carry_over=True), then per cycle step(candidates[c]) and between cycles the
same reset again.  Both kernels inline the same device functions and the library is built with -ffp-contract=off, so everything is compared with ==
under the stated dtype conversions.  The independent checker is the C oracle (oracle/sbr_oracle.py), with the tolerances of the
float64 leg of tests/test_gpu_parity.py::test_cycle_env_sbr_v2_against_oracle_and_reference.

Builds of k_cycle_lookahead<ActT, SCH, WAVES> run here - all six: (f32 | f64, 1, 1) and (f32 | f64, 0, 2) in every test but
test_two_waves_build_of_scheme_1, which runs (f32 | f64, 1, 2): the explicit specialisations that every scheme-1 launch above
Q_FUSED_ONE_WAVE_MAX_ENVS branches takes (98 304 on a whole MI355X).

The NaN rule of best_index / best_return is k_branch_best's and is covered by that kernel's existing tests
(tests/test_lookahead_gpu.py, tests/test_lookahead_end_gpu.py): a candidate that drives a cycle to NaN cannot be forced cheaply."""
import ctypes as C

import numpy as np
import pytest
from cycle_kit import BUILDS, IDS, assert_goes_on_like, assert_sentinels, assert_untouched, candidates as _candidates
from cycle_kit import check_against_replicas, handle_bits, make_env as _env, replicas, sentinel_outputs, start
from gpu_common import host_best, package, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
EVERY = dict(return_rewards=True, return_best=True, return_end=True, return_status=True)


@pytest.fixture(scope="module")
def G():
    return package()


def _start(G, n, scheme, f64, carried, seed):
    """A live handle on all eight scenarios: fresh from reset(rnd=...), or after a cycle, a carried-over reset and another cycle."""
    return start(G, n, scheme, f64, seed, carried=carried, stepped=True)


def _check_against_replica(env, cand, rep):
    """Every output of cycle_lookahead(cand) against the replica's cycles `rep` (one entry per row of cand), with == on values."""
    return check_against_replicas(env, env.cycle_lookahead(cand, **EVERY), cand, None, rep)


@pytest.mark.parametrize("carried", [False, True], ids=["fresh", "after-a-carried-cycle"])
@pytest.mark.parametrize("scheme,f64", BUILDS, ids=IDS)
def test_same_bits_as_the_cycle_kernel_and_the_handle_is_untouched(G, scheme, f64, carried):
    """N = 300, K = 3: 900 branches - a partial last workgroup, and 256 % 3 != 0, so envs straddle workgroups.  Three cycles and
    one cycle against ONE replica run (its cycle 0 is the one-cycle launch's checker)."""
    n, k = 300, 3
    env, twin = _start(G, n, scheme, f64, carried, seed=31), _start(G, n, scheme, f64, carried, seed=31)
    cand = _candidates(env, 3, k, seed=32)
    before = handle_bits(env)
    rep = replicas(G, env, cand, f64=f64)
    _check_against_replica(env, cand, rep)
    _check_against_replica(env, cand[:1].contiguous(), rep[:1])
    # [N, K, 3] is one cycle
    assert same(env.cycle_lookahead(cand[0].contiguous()), env.cycle_lookahead(cand[:1].contiguous()))
    assert_untouched(env, before)
    assert_goes_on_like(env, twin, _candidates(env, 1, 1, seed=33)[0, :, 0].contiguous())
    env.close(); twin.close()


@pytest.mark.parametrize("n,k", [(1, 1), (2, 257), (257, 1)])
def test_addressing_edges(G, n, k):
    """One branch; one env spanning two workgroups (K = 257); K = 1, where the call is sbr_cycle_step on a copy, past one
    workgroup.  Two cycles each, against the replica."""
    env = _start(G, n, 1, False, False, seed=41)
    cand = _candidates(env, 2, k, seed=42)
    _check_against_replica(env, cand, replicas(G, env, cand))
    env.close()


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_two_waves_build_of_scheme_1(G, f64):
    """N = 1541, K = 64: 98 624 branches, above the limit of the one-wave build, so the launch takes the explicit specialisation
    k_cycle_lookahead<ActT, 1, 2> (its own body call, its own register cap, scratch) - as the replica's k_cycle takes its
    two-waves build.  Two cycles, every output, both tape types, and the handle untouched."""
    from gym_sbr2_amd import _capi
    n, k = 1541, 64
    env = _start(G, n, 1, f64, False, seed=45)
    assert n * k > env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS) >= n
    cand = _candidates(env, 2, k, seed=46)
    before = handle_bits(env)
    _check_against_replica(env, cand, replicas(G, env, cand, f64=f64))
    assert_untouched(env, before)
    env.close()


@pytest.mark.parametrize("scheme", [0, 1])
def test_against_the_c_oracle(G, tables, scheme):
    """The independent checker: N = 64, K = 4, two cycles, float64, against OracleCycleBatch(N*K) driven with reset(influent,
    carry_over) and step.  Tolerances of the float64 leg of test_cycle_env_sbr_v2_against_oracle_and_reference: reward 1e-11,
    obs 1e-9, diag rtol 1e-10 (atol 1e-12), on the branches whose status has NEAR_POLE clear - more than half of them."""
    from gym_sbr2_amd import _capi
    from oracle import sbr_oracle as O          # tests/conftest.py puts the repository root on sys.path
    means, stds = tables
    n, k = 64, 4
    rs = np.random.RandomState(51)
    scen = (np.arange(n) % 8).astype(np.int32)
    z = rs.randn(n, 48)
    env = _env(G, n, scheme, True)
    env.reset(scenario=scen, rnd=z)
    cand = _candidates(env, 2, k, seed=52)
    ret, rew, obs_end, diag_end, status = env.cycle_lookahead(cand, return_rewards=True, return_end=True, return_status=True)
    p = O.default_params(scheme=scheme)
    ora = O.OracleCycleBatch(n * k, params=p, nthreads=8)
    infl = np.repeat(O.OracleBatch(n, params=p).mix(means, stds, scen, z), k, axis=0)
    a = cand.cpu().numpy().reshape(2, n * k, 3)
    ora.reset(infl)
    _, r0, _ = ora.step(a[0])
    ora.reset(infl, carry_over=True)
    o1, r1, d1 = ora.step(a[1])
    clean = (status.cpu().numpy().reshape(-1).astype(int) & _capi.ST_NEAR_POLE) == 0
    rew, obs_end, diag_end = rew.cpu().numpy().reshape(2, -1), obs_end.cpu().numpy().reshape(-1, 3), diag_end.cpu().numpy().reshape(-1, 12)
    print("[info] scheme %d: %d of %d branches clear; reward %.2e %.2e, obs %.2e" % (
        scheme, clean.sum(), n * k, np.abs(rew[0] - r0)[clean].max(), np.abs(rew[1] - r1)[clean].max(), np.abs(obs_end - o1)[clean].max()))
    assert clean.sum() > n * k // 2
    assert np.abs(rew[0] - r0)[clean].max() < 1e-11 and np.abs(rew[1] - r1)[clean].max() < 1e-11
    assert np.abs(obs_end - o1)[clean].max() < 1e-9
    assert np.allclose(diag_end[clean], d1[clean], rtol=1e-10, atol=1e-12)
    assert np.array_equal(ret.cpu().numpy().reshape(-1), rew[0] + rew[1])
    env.close()


def test_winner_with_a_tie(G):
    """best_index / best_return are gpu_common.host_best of the returns; env 0 holds the same tape K times, so all of its
    returns tie and candidate 0 wins."""
    n, k = 8, 5
    env = _start(G, n, 1, False, False, seed=61)
    cand = _candidates(env, 1, k, seed=62)
    cand[:, 0] = cand[:, 0, :1]
    ret, bi, br = env.cycle_lookahead(cand, return_best=True)
    assert len(torch.unique(ret[0])) == 1 and int(bi[0]) == 0
    idx, val = host_best(ret)
    assert np.array_equal(bi.cpu().numpy(), idx) and np.array_equal(br.cpu().numpy(), val, equal_nan=True)
    env.close()


def test_no_cycle_writes_zeros_and_touches_nothing(G):
    n, k = 5, 3
    env = _start(G, n, 1, False, True, seed=71)
    x0, c0 = env.get_state()
    ret, rew, bi, br = env.cycle_lookahead(torch.empty((0, n, k, 3), device="cuda"), return_rewards=True, return_best=True)
    assert ret.shape == (n, k) and rew.shape == (0, n, k)
    assert bool((ret == 0).all()) and bool((bi == 0).all()) and bool((br == 0).all())
    for u, v in zip((x0, c0), env.get_state()):
        assert same(u, v)
    with pytest.raises(Exception, match="sbr_cycle_lookahead"):          # the end rows need a last cycle
        env.cycle_lookahead(torch.empty((0, n, k, 3), device="cuda"), return_end=True)
    env.close()


def test_refusals_leave_the_outputs_alone(G):
    """Every refusal that needs a live handle: SBR_ERR_INVALID, the entry point named, sentinel-filled outputs unchanged."""
    n, k = 4, 2
    env = _start(G, n, 1, False, False, seed=81)
    lib, h = env.lib, env._h
    cand = _candidates(env, 1, k, seed=82)
    outs, p = sentinel_outputs(n, k, 1)
    a = C.c_void_p(cand.data_ptr())
    p["br"] = p["bv"]
    full = (p["ret"], p["rew"], p["bi"], p["br"], p["obs"], p["diag"], p["st"])
    refusals = [
        (h, -1, k, a) + full,                                                     # n_cycles < 0
        (h, 1, 0, a) + full,                                                      # fanout < 1
        (h, 1, 2 ** 29, a) + full,                                                # N * fanout = 2^31
        (h, 1, k, None) + full,                                                   # NULL actions with n_cycles > 0
        (h, 1, k, a, None, p["rew"], p["bi"], None, p["obs"], p["diag"], p["st"]),      # best_index without returns
        (h, 1, k, a, None, p["rew"], None, p["br"], p["obs"], p["diag"], p["st"]),      # best_return without returns
        (h, 0, k, None, p["ret"], None, p["bi"], p["br"], p["obs"], None, None),        # obs_end with n_cycles = 0
        (h, 0, k, None, p["ret"], None, p["bi"], p["br"], None, p["diag"], None),       # diag_end with n_cycles = 0
        (h, 0, k, None, p["ret"], None, p["bi"], p["br"], None, None, p["st"]),         # status_out with n_cycles = 0
    ]
    for args in refusals:
        assert lib.sbr_cycle_lookahead(*args, None) == -1, args[1:4]
        assert b"sbr_cycle_lookahead" in lib.sbr_last_error(h), args[1:4]
    assert_sentinels(outs)
    env.close()


def test_setpoint_search_reports_what_the_lookahead_returns(G):
    """CycleSetpointSearch at N = 32, K = 16, two iterations: the reported return is cycle_lookahead of the reported action, bit
    for bit, and no worse than the all-0.5 action's on any env - candidate 0 of iteration 0."""
    from gym_sbr2_amd import _capi
    n = 32
    env = _start(G, n, 1, False, False, seed=91)
    x0, c0 = env.get_state()
    search = G.CycleSetpointSearch(env, K=16, n_cycles=1, iters=2, elite_frac=0.25, seed=5)
    action, value = search.plan()
    assert action.shape == (n, 3) and action.dtype == env.action_dtype and value.shape == (n,) and value.dtype == torch.float64
    assert bool(((action >= 0) & (action <= 1)).all())
    again, status = env.cycle_lookahead(action[:, None, :].contiguous(), return_status=True)
    assert same(value, again[:, 0]) and torch.equal(search.status, status[:, 0])
    half, half_status = env.cycle_lookahead(torch.full((n, 1, 3), 0.5, dtype=env.action_dtype, device="cuda"), return_status=True)
    assert not bool(((half_status | search.status[:, None]) & (_capi.ST_NEAR_POLE | _capi.ST_NONFINITE)).any())   # the all-0.5 tape is clean here
    assert bool((value >= half[:, 0]).all()), (value - half[:, 0]).min()
    for u, v in zip((x0, c0), env.get_state()):
        assert same(u, v)
    env.close()
