"""sbr_draw_influent and sbr_cycle_lookahead_scenarios on the GPU (SbrEnv2Vec.draw_influent, influent_futures,
cycle_lookahead_scenarios, RobustCycleSetpointSearch): influent futures drawn without a reset, and K candidate tapes per env each
played against the SAME S futures, the handle left bit for bit as it was.

The checker of the bit-equality tests is the EXISTING per-cycle kernel on a second handle of B = N*K*S envs (cycle_kit.replicas), driven
through the existing API only, as in tests/test_cycle_lookahead_gpu.py: set_state with the live handle's get_state() columns
repeated K*S times, then per cycle reset(influent = influent[c] expanded over k, carry_over=True) and step(candidates[c] expanded
over s).  Both kernels inline the same device functions and the library is built with -ffp-contract=off, so everything is compared
with == under the stated dtype conversions.  The draws are checked against the resets (the same mix in another kernel: ==) and
against gpu_common's host Philox.

Builds of k_cycle_lookahead_scenarios<ActT, SCH, WAVES> run here - all six: (f32 | f64, 1, 1) and (f32 | f64, 0, 2) in
test_same_bits_as_the_cycle_kernel, (f32, 1, 1) in the others, and (f32 | f64, 1, 2) in test_two_waves_build_of_scheme_1."""
import ctypes as C

import numpy as np
import pytest
from cycle_kit import ALL, BUILDS, IDS, assert_goes_on_like, assert_sentinels, assert_untouched as _assert_untouched
from cycle_kit import candidates as _candidates, check_against_replicas, handle_bits as _handle_bits, make_env as _env, replicas
from cycle_kit import scen as _scen, sentinel_outputs, start as _start
from gpu_common import host_best, normal_pair, package, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return package()


def _check_against_replica(G, env, cand, infl, f64=False):
    """Every output of cycle_lookahead_scenarios(cand, infl) against the per-cycle kernel under the same futures, with == on values."""
    s = infl.shape[2]
    return check_against_replicas(env, env.cycle_lookahead_scenarios(cand, infl, **ALL), cand, s, replicas(G, env, cand, infl, s, f64=f64))


# ---------------------------------------------------------------------------------------------- the draws
def test_draws_are_the_resets_draws_and_depend_on_nothing_but_seed_id_index_and_scenario(G):
    """N = 70 on all eight scenarios, global ids straddling 2^32."""
    n, seed, first = 70, 12345, 2 ** 32 - 35
    scen = _scen(n)
    env = _env(G, n, first_env_id=first)
    env.reset(seed=seed, scenario=scen)
    before = _handle_bits(env)
    one = env.draw_influent(1, 1, seed, scen)
    assert one.shape == (1, n, 1, 14) and one.dtype == torch.float64
    assert same(one[0, :, 0], env.influent().T.contiguous()), "d = 0 is the draw of reset(seed), all 14 entries"
    grid, d5 = env.draw_influent(3, 2, seed, scen, first_draw=0), env.draw_influent(1, 1, seed, scen, first_draw=5)
    assert same(grid[2, :, 1], d5[0, :, 0]) and same(grid[0, :, 0], one[0, :, 0])
    assert not torch.equal(grid[0, :, 0], grid[0, :, 1])
    part = _env(G, 30, first_env_id=first + 40)                            # another shard of the same global ids
    assert same(part.draw_influent(3, 2, seed, scen[40:], first_draw=0), grid[:, 40:].contiguous())
    part.close()
    # d = 5 against the reset's own mix of the host's normals under the stream word 0 + 256*5
    gid = first + np.arange(n)
    z0, z1 = normal_pair(np.arange(24)[None, :], 256 * 5, gid[:, None], seed)
    z = np.stack([z0, z1], axis=-1).reshape(n, 48)
    twin = _env(G, n, first_env_id=first)
    twin.reset(scenario=scen, rnd=z)
    want, got = twin.influent().T.cpu().numpy(), d5[0, :, 0].cpu().numpy()
    print("[info] draw 5 against the host's normals: largest relative difference %.2e"
          % (np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())
    assert np.allclose(got, want, rtol=1e-10, atol=0)
    twin.close()
    _assert_untouched(env, before)
    env.close()


def test_scenario_drawn_on_the_device_under_random_scenario(G):
    n, seed = 70, 77
    env = _env(G, n, random_scenario=True)
    env.reset(seed=seed)
    d = env.draw_influent(2, 3, seed)
    assert same(d[0, :, 0], env.influent().T.contiguous())                 # d = 0: sbr_draw_scenarios' value and the reset's normals
    scen = env.draw_scenarios(seed)
    assert same(env.draw_influent(1, 1, seed, scen)[0], d[0, :, :1].contiguous())
    assert len(torch.unique(d.reshape(-1, 14), dim=0)) == 2 * n * 3        # the other draws are draws of their own
    env.close()


def test_draw_refusals_leave_the_output_alone(G):
    n = 4
    env = _start(G, n, seed=5)
    before = _handle_bits(env)
    lib, h = env.lib, env._h
    out = torch.full((2 * n * 2 * 14,), -7.0, dtype=torch.float64, device="cuda")         # no influent entry is negative
    scen = torch.zeros((n,), dtype=torch.int32, device="cuda")
    o, sc = C.c_void_p(out.data_ptr()), C.c_void_p(scen.data_ptr())
    refusals = [(h, 0, 2, 2, 0, sc, None), (h, 0, 0, 2, 0, sc, o), (h, 0, 2, 0, 0, sc, o), (h, 0, 2, 2, -1, sc, o),
                (h, 0, 2, 2, 2 ** 24 - 3, sc, o), (h, 0, 2 ** 15, 2 ** 15, 0, sc, o), (h, 0, 2, 2, 0, None, o)]
    # NULL out; rows < 1; per_env < 1; first_draw < 0; a draw index of 2^24; N * rows * per_env = 2^32; NULL scenario, fixed config
    for args in refusals:
        assert lib.sbr_draw_influent(*args, None) == -1, args[1:5]
        assert b"sbr_draw_influent" in lib.sbr_last_error(h), args[1:5]
    assert lib.sbr_draw_influent(h, 0, 2, 2, 2 ** 24 - 4, sc, o, None) == 0          # the last draw index there is
    torch.cuda.synchronize()
    assert not bool((out == -7).any())
    out.fill_(-7.0)
    for args in refusals:
        assert lib.sbr_draw_influent(*args, None) == -1
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    _assert_untouched(env, before)
    env.close()


# ---------------------------------------------------------------------------------------------- the lookahead
@pytest.mark.parametrize("scheme,f64", BUILDS, ids=IDS)
def test_same_bits_as_the_cycle_kernel_and_the_handle_is_untouched(G, scheme, f64):
    """(N, K, S) = (13, 3, 7): 273 branches - a partial second workgroup, and neither 21 nor 7 divides 256, so envs and candidates
    straddle workgroups.  Three cycles under futures from draw_influent."""
    n, k, s = 13, 3, 7
    env, twin = _start(G, n, scheme, f64, seed=31), _start(G, n, scheme, f64, seed=31)
    cand = _candidates(env, 3, k, seed=32)
    infl = env.draw_influent(3, s, seed=9, scenario=_scen(n), first_draw=1)
    before = _handle_bits(env)
    _check_against_replica(G, env, cand, infl, f64)
    _assert_untouched(env, before)
    assert_goes_on_like(env, twin, _candidates(env, 1, 1, seed=33)[0, :, 0].contiguous())
    env.close(); twin.close()


def test_one_future_equal_to_the_stored_influent_is_cycle_lookahead(G):
    n, k = 37, 5
    env = _start(G, n, seed=41)
    cand = _candidates(env, 2, k, seed=42)
    infl = env.influent_futures(2, 1, seed=3)
    assert same(infl[0, :, 0], env.influent().T.contiguous()) and not torch.equal(infl[1], infl[0])
    infl[1] = infl[0]
    got = env.cycle_lookahead_scenarios(cand, infl, **ALL)
    ret, rew, bi, br, obs_end, diag_end, status = env.cycle_lookahead(cand, return_rewards=True, return_best=True, return_end=True,
                                                                      return_status=True)
    want = (ret[..., None], rew[..., None], ret, ret, bi, br, obs_end[:, :, None], diag_end[:, :, None], status[..., None])
    for name, u, v in zip("returns rewards mean worst best_index best_value obs_end diag_end status".split(), got, want):
        assert same(u, v.contiguous()), name
    env.close()


def test_identical_futures_give_identical_returns(G):
    n, k, s = 9, 3, 4
    env = _start(G, n, seed=43)
    cand = _candidates(env, 2, k, seed=44)
    infl = env.influent_futures(2, 1, seed=4).expand(2, n, s, 14).contiguous()
    ret, mean, worst = env.cycle_lookahead_scenarios(cand, infl, return_stats=True)
    for j in range(1, s):
        assert same(ret[..., j], ret[..., 0])
    assert same(mean, ret[..., 0].contiguous()) and same(worst, mean)
    env.close()


@pytest.mark.parametrize("n,k,s", [(1, 1, 1), (1, 1, 257), (1, 257, 1), (257, 1, 1), (2, 3, 300)])
def test_addressing_edges(G, n, k, s):
    """One branch; one candidate, one env and one future per branch past a workgroup; and n_scen > 256, where the influent row of a
    lane lies more than a workgroup's lanes behind the row of the workgroup's first env.  Two cycles each, against the replica."""
    env = _start(G, n, seed=51)
    cand = _candidates(env, 2, k, seed=52)
    infl = env.influent_futures(2, s, seed=6, scenario=_scen(n), first_draw=1)
    _check_against_replica(G, env, cand, infl)
    env.close()


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_two_waves_build_of_scheme_1(G, f64):
    """(N, K, S) = (193, 8, 64): 98 816 branches, above the limit of the one-wave build, so the launch takes the explicit
    specialisation k_cycle_lookahead_scenarios<ActT, 1, 2> - as the replica's k_cycle takes its two-waves build."""
    from gym_sbr2_amd import _capi
    n, k, s = 193, 8, 64
    env = _start(G, n, 1, f64, seed=55)
    assert n * k * s > env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS) >= n * k
    cand = _candidates(env, 2, k, seed=56)
    infl = env.influent_futures(2, s, seed=7, scenario=_scen(n), first_draw=1)
    before = _handle_bits(env)
    _check_against_replica(G, env, cand, infl, f64)
    _assert_untouched(env, before)
    env.close()


def test_no_cycle_writes_zeros_and_touches_nothing(G):
    n, k, s = 5, 3, 4
    env = _start(G, n, seed=71)
    before = _handle_bits(env)
    none = (torch.empty((0, n, k, 3), device="cuda"), torch.empty((0, n, s, 14), dtype=torch.float64, device="cuda"))
    ret, rew, mean, worst, bi, bv = env.cycle_lookahead_scenarios(*none, return_rewards=True, return_stats=True, return_best=True)
    assert ret.shape == (n, k, s) and rew.shape == (0, n, k, s) and mean.shape == worst.shape == (n, k)
    for t in (ret, mean, worst, bi, bv):
        assert bool((t == 0).all())
    _assert_untouched(env, before)
    with pytest.raises(Exception, match="sbr_cycle_lookahead_scenarios"):          # the end rows need a last cycle
        env.cycle_lookahead_scenarios(*none, return_end=True)
    env.close()


def test_refusals_leave_the_outputs_alone(G):
    """Every refusal that needs a live handle: SBR_ERR_INVALID, the entry point named, sentinel-filled outputs unchanged."""
    n, k, s = 4, 2, 3
    env = _start(G, n, seed=81)
    lib, h = env.lib, env._h
    cand = _candidates(env, 1, k, seed=82)
    infl = env.influent_futures(1, s)
    outs, p = sentinel_outputs(n, k, s)
    a, f = C.c_void_p(cand.data_ptr()), C.c_void_p(infl.data_ptr())
    full = tuple(p[name] for name in "ret rew mean worst bi bv obs diag st".split())

    def without(*names):
        return tuple(None if name in names else p[name] for name in "ret rew mean worst bi bv obs diag st".split())

    refusals = [
        (h, -1, k, s, a, f) + full,                                               # n_cycles < 0
        (h, 1, 0, s, a, f) + full,                                                # fanout < 1
        (h, 1, k, 0, a, f) + full,                                                # n_scen < 1
        (h, 1, 2 ** 29, 1, a, f) + full,                                          # N * fanout = 2^31
        (h, 1, 2 ** 15, 2 ** 14, a, f) + full,                                    # N * fanout * n_scen = 2^31
        (h, 1, k, s, None, f) + full,                                             # NULL actions with n_cycles > 0
        (h, 1, k, s, a, None) + full,                                             # NULL influent with n_cycles > 0
        (h, 1, k, s, a, f) + without("ret"),                                      # mean / worst without returns
        (h, 1, k, s, a, f) + without("ret", "mean", "bi", "bv"),                  # worst without returns
        (h, 1, k, s, a, f) + without("mean"),                                     # best_index / best_value without mean
        (h, 1, k, s, a, f) + without("mean", "bi"),                               # best_value without mean
        (h, 0, k, s, None, None) + without("rew", "diag", "st"),                  # obs_end with n_cycles = 0
        (h, 0, k, s, None, None) + without("rew", "obs", "st"),                   # diag_end with n_cycles = 0
        (h, 0, k, s, None, None) + without("rew", "obs", "diag"),                 # status_out with n_cycles = 0
    ]
    for args in refusals:
        assert lib.sbr_cycle_lookahead_scenarios(*args, None) == -1, args[1:4]
        assert b"sbr_cycle_lookahead_scenarios" in lib.sbr_last_error(h), args[1:4]
    assert_sentinels(outs)
    env.close()


def test_common_random_numbers_against_futures_of_their_own(G):
    """N = 32, K = 8, S = 8, two cycles: the winner when all candidates meet the same futures, and when each candidate is scored on
    futures of its own (eight calls with K = 1 and disjoint draws).  How often the two agree is information, not a
    gate: both are valid indices."""
    n, k, s = 32, 8, 8
    env = _start(G, n, seed=91)
    rs = np.random.RandomState(92)
    # candidates close to each other, as a search draws them late: where the futures' noise can decide
    cand = torch.from_numpy(0.5 + 0.05 * rs.randn(2, n, k, 3)).to(env.action_dtype).cuda()
    scen = _scen(n)
    _, bi, _ = env.cycle_lookahead_scenarios(cand, env.influent_futures(2, s, seed=1, scenario=scen, first_draw=1), return_best=True)
    means = []
    for j in range(k):
        fut = env.influent_futures(2, s, seed=1, scenario=scen, first_draw=1 + 2 * s * (j + 1))
        means.append(env.cycle_lookahead_scenarios(cand[:, :, j:j + 1].contiguous(), fut, return_stats=True)[1])
    own = host_best(torch.cat(means, dim=1))[0]
    bi = bi.cpu().numpy()
    assert ((bi >= 0) & (bi < k)).all() and ((own >= 0) & (own < k)).all()
    print("[info] common random numbers: the winner agrees with independent futures' on %d of %d envs" % ((bi == own).sum(), n))
    env.close()


@pytest.mark.parametrize("risk", ["mean", "worst"])
def test_robust_setpoint_search_reports_what_the_lookahead_returns(G, risk):
    """RobustCycleSetpointSearch at N = 16, K = 8, S = 4, two iterations, two cycles: the reported value is
    cycle_lookahead_scenarios of the reported tape on .futures, bit for bit, and not below the all-0.5 tape's on any env whose
    all-0.5 tape is clean - candidate 0 of iteration 0."""
    from gym_sbr2_amd import _capi
    n, s = 16, 4
    bad = _capi.ST_NEAR_POLE | _capi.ST_NONFINITE
    env = _start(G, n, seed=95)
    before = _handle_bits(env)
    search = G.RobustCycleSetpointSearch(env, K=8, n_scen=s, n_cycles=2, iters=2, elite_frac=0.25, seed=5, risk=risk)
    action, value = search.plan()
    assert action.shape == (n, 3) and action.dtype == env.action_dtype and value.shape == (n,) and value.dtype == torch.float64
    assert search.futures.shape == (2, n, s, 14) and same(search.futures[0, :, 0], env.influent().T.contiguous())
    assert same(search.futures, env.influent_futures(2, s, seed=5, first_draw=1))
    pick = 1 if risk == "mean" else 2
    again = env.cycle_lookahead_scenarios(search.tape[:, :, None, :].contiguous(), search.futures, return_stats=True, return_status=True)
    assert same(value, again[pick][:, 0].contiguous()) and same(action, search.tape[0].to(env.action_dtype))
    bits = again[3][:, 0]                                                  # [N, S]: the winner's branches
    assert torch.equal(search.status, bits[:, 0] | bits[:, 1] | bits[:, 2] | bits[:, 3])
    half = env.cycle_lookahead_scenarios(torch.full((2, n, 1, 3), 0.5, dtype=env.action_dtype, device="cuda"), search.futures,
                                         return_stats=True, return_status=True)
    clean = ((half[3][:, 0] & bad) == 0).all(dim=-1)
    assert bool(clean.any()) and bool((value[clean] >= half[pick][:, 0][clean]).all())
    _assert_untouched(env, before)
    env.close()
