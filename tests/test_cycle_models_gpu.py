"""sbr_set_models and sbr_cycle_lookahead_models on the GPU (SbrEnv2Vec.set_models, num_models, cycle_lookahead_models,
RobustCycleSetpointSearch.plant_models): K candidate tapes per env, each played against S futures, future s under MODEL
s % num_models of the handle's table, the handle left bit for bit as it was.

The checker is the EXISTING per-cycle kernel, through the existing API only, as in tests/test_cycle_scenarios_gpu.py: per model m
a second handle CREATED WITH THE CONFIG OF MODEL m (cycle_kit.replicas) for the futures s with s % M = m, N*K envs for each of
them, given the live handle's state through get_state / set_state, then per cycle reset(influent = the futures' rows expanded
over k, carry_over=True) and step(candidates[c] expanded over those futures).  Both kernels inline the same device functions and the library is built with -ffp-contract=off, so everything
is compared with == under the stated dtype conversions.  Where the models equal the handle's config the reference is
cycle_lookahead / cycle_lookahead_scenarios itself.

Builds of k_cycle_lookahead_models<ActT, SCH, WAVES> run here - all six: (f32 | f64, 1, 1) and (f32 | f64, 0, 2) in
test_same_bits_as_replicas_under_each_model, (f32, 1, 1) in the others, and (f32 | f64, 1, 2) in test_two_waves_build_of_scheme_1."""
import ctypes as C

import numpy as np
import pytest
from cycle_kit import ALL, BUILDS, IDS, NAMES, assert_goes_on_like, assert_sentinels, assert_untouched as _assert_untouched
from cycle_kit import candidates as _candidates, check_against_replicas, handle_bits as _handle_bits, replicas
from cycle_kit import scen as _scen, sentinel_outputs, start as _start
from gpu_common import package, same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return package()


def _model(env, **factors):
    """The handle's config with the named model fields multiplied."""
    from gym_sbr2_amd.models import copy_config
    cfg = copy_config(env.cfg)
    for name, factor in factors.items():
        setattr(cfg, name, getattr(cfg, name) * factor)
    return cfg


def _two_models(env):
    """Model 0 the handle's own config; model 1 a slower nitrifier, a faster heterotroph and warmer water."""
    return [_model(env), _model(env, muA=0.7, muH=1.2, So_sat=0.95)]


@pytest.mark.parametrize("scheme,f64", BUILDS, ids=IDS)
def test_same_bits_as_replicas_under_each_model(G, scheme, f64):
    """(N, K, S, M) = (70, 5, 3, 2): 350 pairs - two workgroups along x, the second partial, and 5 does not divide 256, so envs
    straddle workgroups; three rows of workgroups along y, and s % M wraps (futures 0 and 2 under model 0, future 1 under model 1).
    Futures 0 and 1 share their influent, so they differ by the plant alone.  Two cycles."""
    n, k, s = 70, 5, 3
    env = _start(G, n, scheme, f64, seed=31)
    models = _two_models(env)
    env.set_models(models)
    assert env.num_models == 2
    cand = _candidates(env, 2, k, seed=32)
    infl = env.draw_influent(2, s, seed=9, scenario=_scen(n), first_draw=1)
    infl[:, :, 1] = infl[:, :, 0]
    before = _handle_bits(env)
    got = env.cycle_lookahead_models(cand, infl, **ALL)
    _assert_untouched(env, before)
    check_against_replicas(env, got, cand, s, replicas(G, env, cand, infl, s, models, f64))
    ret = got[0]
    # the same tape and influent under another plant: another return
    assert float((ret[..., 0] != ret[..., 1]).double().mean()) > 0.9
    assert not torch.equal(ret[..., 0], ret[..., 2])                        # the same plant under another influent
    env.close()


def test_stored_influent_under_two_models(G):
    """influent=None: every cycle of every future under the influent the handle holds.  (N, K, S, M) = (37, 3, 3, 2), n_scen given."""
    n, k, s = 37, 3, 3
    env = _start(G, n, seed=41)
    models = _two_models(env)
    env.set_models(G.PlantModels(models, base=env.cfg))
    cand = _candidates(env, 2, k, seed=42)
    before = _handle_bits(env)
    got = env.cycle_lookahead_models(cand, n_scen=s, **ALL)
    _assert_untouched(env, before)
    check_against_replicas(env, got, cand, s, replicas(G, env, cand, None, s, models))
    assert same(got[0][..., 0], got[0][..., 2].contiguous()) and not torch.equal(got[0][..., 0], got[0][..., 1])
    assert env.cycle_lookahead_models(cand).shape == (n, k, 2)             # n_scen defaults to num_models
    env.close()


def test_one_model_equal_to_the_handles_config_is_cycle_lookahead(G):
    n, k, s = 37, 5, 2
    env = _start(G, n, seed=43)
    env.set_models([_model(env)])
    cand = _candidates(env, 2, k, seed=44)
    got = env.cycle_lookahead_models(cand, n_scen=s, **ALL)
    ret, rew, bi, br, obs_end, diag_end, status = env.cycle_lookahead(cand, return_rewards=True, return_best=True, return_end=True,
                                                                      return_status=True)

    def over_s(t, at):
        return t.unsqueeze(at).expand(*t.shape[:at], s, *t.shape[at:]).contiguous()

    mean = (ret + ret) / 2.0                                                 # ((0.0 + r) + r) / 2
    want = (over_s(ret, 2), over_s(rew, 3), mean, ret, bi, br, over_s(obs_end, 2), over_s(diag_end, 2), over_s(status, 2))
    for name, u, v in zip(NAMES, got, want):
        assert same(u, v.contiguous()), name
    env.close()


def test_models_equal_to_the_handles_config_are_cycle_lookahead_scenarios(G):
    n, k, s = 13, 3, 7
    env = _start(G, n, seed=45)
    env.set_models([_model(env), _model(env)])
    cand = _candidates(env, 2, k, seed=46)
    infl = env.influent_futures(2, s, seed=4, scenario=_scen(n), first_draw=1)
    for name, u, v in zip(NAMES, env.cycle_lookahead_models(cand, infl, **ALL), env.cycle_lookahead_scenarios(cand, infl, **ALL)):
        assert same(u, v), name
    env.close()


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_two_waves_build_of_scheme_1(G, f64):
    """(N, K) = (193, 8) as in tests/test_cycle_scenarios_gpu.py and the fewest futures that put the branch count above the limit of
    the one-wave build, which the library reports (on a whole MI355X: S = 64, 98 816 branches against 98 304), so the launch takes
    the explicit specialisation k_cycle_lookahead_models<ActT, 1, 2>.  One cycle, three identical models, against
    cycle_lookahead_scenarios - itself pinned to the cycle kernel there."""
    from gym_sbr2_amd import _capi
    n, k = 193, 8
    env = _start(G, n, 1, f64, seed=55)
    limit = env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS)
    s = limit // (n * k) + 1
    assert n * k * s > limit >= n * k * (s - 1) and s <= 65535, limit
    env.set_models([_model(env)] * 3)
    cand = _candidates(env, 1, k, seed=56)
    infl = env.influent_futures(1, s, seed=7, scenario=_scen(n), first_draw=1)
    before = _handle_bits(env)
    for name, u, v in zip(NAMES, env.cycle_lookahead_models(cand, infl, **ALL), env.cycle_lookahead_scenarios(cand, infl, **ALL)):
        assert same(u, v), name
    _assert_untouched(env, before)
    env.close()


def test_no_cycle_writes_zeros_and_touches_nothing(G):
    n, k, s = 5, 3, 4
    env = _start(G, n, seed=71)
    env.set_models(_two_models(env))
    before = _handle_bits(env)
    none = (torch.empty((0, n, k, 3), device="cuda"), torch.empty((0, n, s, 14), dtype=torch.float64, device="cuda"))
    for args in (none, (none[0], None, s)):
        ret, rew, mean, worst, bi, bv = env.cycle_lookahead_models(*args, return_rewards=True, return_stats=True, return_best=True)
        assert ret.shape == (n, k, s) and rew.shape == (0, n, k, s) and mean.shape == worst.shape == (n, k)
        for t in (ret, mean, worst, bi, bv):
            assert bool((t == 0).all())
    _assert_untouched(env, before)
    with pytest.raises(Exception, match="sbr_cycle_lookahead_models"):            # the end rows need a last cycle
        env.cycle_lookahead_models(*none, return_end=True)
    env.close()


def test_refusals_leave_the_outputs_and_the_table_alone(G):
    """Every refusal that needs a live handle: SBR_ERR_INVALID, the entry point named, sentinel-filled outputs unchanged."""
    from gym_sbr2_amd import _capi
    n, k, s = 4, 2, 3
    env = _start(G, n, seed=81)
    lib, h = env.lib, env._h
    cand = _candidates(env, 1, k, seed=82)
    infl = env.influent_futures(1, s)
    outs, p = sentinel_outputs(n, k, s)
    a, f = C.c_void_p(cand.data_ptr()), C.c_void_p(infl.data_ptr())
    order = "ret rew mean worst bi bv obs diag st".split()
    full = tuple(p[name] for name in order)

    def without(*names):
        return tuple(None if name in names else p[name] for name in order)

    # no table set: whatever else is right
    assert env.num_models == 0
    assert lib.sbr_cycle_lookahead_models(h, 1, k, s, a, f, *full, None) == -1
    assert lib.sbr_last_error(h) == b"sbr_cycle_lookahead_models: no model table: call sbr_set_models first"
    with pytest.raises(ValueError):
        env.cycle_lookahead_models(cand)                                          # no n_scen to take from an empty table
    # a table that may not stand: the handle keeps none, and says which model and which field
    bad = _model(env); bad.t_delta = bad.t_delta * 2
    arr = (_capi.SbrConfig * 2)(_model(env), bad)
    assert lib.sbr_set_models(h, 2, arr) == -1
    assert lib.sbr_last_error(h).startswith(b"sbr_set_models: models[1]: t_delta differs from the base config")
    for args in ((-1, arr), (2, None)):
        assert lib.sbr_set_models(h, *args) == -1 and lib.sbr_last_error(h).startswith(b"sbr_set_models: ")
    assert env.num_models == 0
    with pytest.raises(ValueError, match="t_delta differs"):
        env.set_models([_model(env), bad])
    env.set_models(_two_models(env))
    refusals = [
        (h, -1, k, s, a, f) + full,                                               # n_cycles < 0
        (h, 1, 0, s, a, f) + full,                                                # fanout < 1
        (h, 1, k, 0, a, f) + full,                                                # n_scen < 1
        (h, 1, k, 65536, a, f) + full,                                            # n_scen beyond the grid's y axis
        (h, 1, 2 ** 29, 1, a, f) + full,                                          # N * fanout = 2^31
        (h, 1, 2 ** 15, 2 ** 14, a, f) + full,                                    # N * fanout * n_scen = 2^31
        (h, 1, k, s, None, f) + full,                                             # NULL actions with n_cycles > 0
        (h, 1, k, s, a, f) + without("ret"),                                      # mean / worst without returns
        (h, 1, k, s, a, f) + without("mean"),                                     # best_index / best_value without mean
        (h, 0, k, s, None, None) + without("rew", "diag", "st"),                  # obs_end with n_cycles = 0
        (h, 0, k, s, None, None) + without("rew", "obs", "diag"),                 # status_out with n_cycles = 0
    ]
    for args in refusals:
        assert lib.sbr_cycle_lookahead_models(*args, None) == -1, args[1:4]
        assert b"sbr_cycle_lookahead_models" in lib.sbr_last_error(h), args[1:4]
    assert lib.sbr_cycle_lookahead_models(h, 1, k, 65536, a, f, *full, None) == -1
    assert b"n_scen must be <= 65535" in lib.sbr_last_error(h)
    assert_sentinels(outs)
    assert env.num_models == 2
    env.close()


def test_replacing_and_dropping_the_table_and_every_other_call_unchanged(G):
    """step() and cycle_lookahead_scenarios return the same bits with a table, with another one and with none; the models call
    follows the table in force."""
    n, k, s = 9, 3, 2
    env, twin = _start(G, n, seed=91), _start(G, n, seed=91)
    cand = _candidates(env, 2, k, seed=92)
    infl = env.influent_futures(2, s, seed=5, scenario=_scen(n), first_draw=1)
    scen_before = env.cycle_lookahead_scenarios(cand, infl, **ALL)
    two = _two_models(env)
    env.set_models(two)
    r2 = env.cycle_lookahead_models(cand, infl)
    env.set_models([two[1]])                                                       # replaced: every future under model 1
    assert env.num_models == 1
    r1 = env.cycle_lookahead_models(cand, infl)
    assert same(r1[..., 1], r2[..., 1].contiguous()) and not torch.equal(r1[..., 0], r2[..., 0])
    env.set_models([two[0]])                                                       # the handle's own config: the scenarios call
    assert same(env.cycle_lookahead_models(cand, infl), scen_before[0]) and same(r2[..., 0], scen_before[0][..., 0].contiguous())
    for name, u, v in zip(NAMES, env.cycle_lookahead_scenarios(cand, infl, **ALL), scen_before):
        assert same(u, v), name
    act = _candidates(env, 1, 1, seed=93)[0, :, 0].contiguous()
    env.set_models(two)
    assert_goes_on_like(env, twin, act)                                            # with a table, and a twin that never had one
    env.set_models(None)                                                           # dropped
    assert env.num_models == 0
    with pytest.raises(Exception, match="no model table"):
        env.cycle_lookahead_models(cand, infl)
    env.reset(scenario=_scen(n), rnd=np.random.RandomState(94).randn(n, 48), carry_over=True)
    twin.reset(scenario=_scen(n), rnd=np.random.RandomState(94).randn(n, 48), carry_over=True)
    for u, v in zip(env.get_state(), twin.get_state()):
        assert same(u, v)
    env.close(); twin.close()


@pytest.mark.parametrize("risk", ["mean", "worst"])
def test_robust_setpoint_search_over_plant_models(G, risk):
    """RobustCycleSetpointSearch with plant_models = True at N = 64, K = 8, S = 4, M = 2, two iterations, two cycles: the reported
    value is cycle_lookahead_models' mean (or worst) of the reported tape on .futures, bit for bit; under risk="worst" it is the
    minimum over the futures; under risk="mean" it is not cycle_lookahead_scenarios' value - the plants are in the score."""
    n, s = 64, 4
    env = _start(G, n, seed=95)
    env.set_models(G.PlantModels.perturbed(env.cfg, 2, rel_std=0.3, seed=1, fields=("muA", "muH", "kh")))
    before = _handle_bits(env)
    search = G.RobustCycleSetpointSearch(env, K=8, n_scen=s, n_cycles=2, iters=2, elite_frac=0.25, seed=5, risk=risk)
    search.plant_models = True
    action, value = search.plan()
    assert action.shape == (n, 3) and action.dtype == env.action_dtype and value.shape == (n,) and value.dtype == torch.float64
    assert search.futures.shape == (2, n, s, 14) and same(search.futures, env.influent_futures(2, s, seed=5, first_draw=1))
    tape = search.tape[:, :, None, :].contiguous()
    ret, mean, worst, status = env.cycle_lookahead_models(tape, search.futures, return_stats=True, return_status=True)
    assert same(value, (mean if risk == "mean" else worst)[:, 0].contiguous()) and same(action, search.tape[0].to(env.action_dtype))
    bits = status[:, 0]
    assert torch.equal(search.status, bits[:, 0] | bits[:, 1] | bits[:, 2] | bits[:, 3])
    if risk == "worst":
        assert same(value, ret[:, 0].min(dim=-1).values)
    else:
        assert not torch.equal(value, env.cycle_lookahead_scenarios(tape, search.futures, return_stats=True)[1][:, 0].contiguous())
    _assert_untouched(env, before)
    env.close()


def test_refusal_precedence_is_the_familys(G):
    """Two or three faults at once, for each of the three entry points: the text is that of the LAST failing check in the family's
    one ordered list - winners, mean / worst, n_cycles = 0 with end rows, NULL influent, NULL actions, the 2^31 bound with n_scen,
    the fan-out, n_scen's upper and lower bound, n_cycles < 0, no table, NULL env - and nothing is written.  (N, K, S) = (3, 2, 2);
    invalid arguments only, nothing is launched.  The texts were recorded from the three separate checks this list replaced."""
    n, k, s = 3, 2, 2
    env = _start(G, n, seed=85)
    lib, h = env.lib, env._h
    cand = _candidates(env, 1, k, seed=86)
    infl = env.influent_futures(1, s)
    outs, p = sentinel_outputs(n, k, s)
    a, f = C.c_void_p(cand.data_ptr()), C.c_void_p(infl.data_ptr())

    def refused(entry, want, handle=h, n_cycles=1, fanout=k, n_scen=s, actions=a, influent=f, drop=()):
        futures = entry != "sbr_cycle_lookahead"
        order = "ret rew mean worst bi bv obs diag st" if futures else "ret rew bi bv obs diag st"
        args = (handle, n_cycles, fanout) + ((n_scen, actions, influent) if futures else (actions,))
        args += tuple(None if name in drop else p[name] for name in order.split())
        assert getattr(lib, entry)(*args, None) == -1, (entry, want)
        got = lib.sbr_last_error(handle)
        assert got == (entry + ": " + want).encode(), (entry, want, got)

    END0 = "n_cycles = 0 has no last cycle for obs_end, diag_end or status_out"
    NO_ACT, NO_INFL = "NULL actions with n_cycles > 0", "NULL influent with n_cycles > 0"
    PAIRS, BRANCHES = "num_envs * fanout must stay below 2^31 branches", "num_envs * fanout * n_scen must stay below 2^31 branches"
    FANOUT, SCEN, CYCLES = "fanout must be >= 1", "n_scen must be >= 1", "n_cycles must be >= 0"
    STATS = "mean_out / worst_out are reduced from returns: give returns with them"
    GRID = "n_scen must be <= 65535 (the futures are the grid's y axis)"
    TABLE = "no model table: call sbr_set_models first"
    one = "sbr_cycle_lookahead"
    refused(one, END0, n_cycles=0, actions=None, drop=("ret", "rew"))                   # best_* without returns + end rows of no cycle
    refused(one, NO_ACT, actions=None, drop=("ret",))                                   # best_* without returns + NULL actions
    refused(one, FANOUT, n_cycles=0, actions=None, fanout=0, drop=("rew",))             # end rows of no cycle + fanout
    refused(one, PAIRS, actions=None, fanout=2 ** 30)                                   # NULL actions + N * fanout >= 2^31
    refused(one, CYCLES, n_cycles=-1, fanout=0, drop=("ret",))                          # best_*, fanout + n_cycles < 0
    refused(one, "NULL env", handle=None, n_cycles=-1, fanout=0)                        # fanout, n_cycles < 0 + NULL env
    for entry in ("sbr_cycle_lookahead_scenarios", "sbr_cycle_lookahead_models"):
        models = entry.endswith("models")
        if models:      # no table yet: it outranks everything but a NULL env
            assert env.num_models == 0
            refused(entry, TABLE, n_cycles=-1)                                        # n_cycles < 0 + no table
            refused(entry, TABLE, n_scen=0, fanout=0, drop=("mean",))                   # winners, fanout, n_scen < 1 + no table
            refused(entry, "NULL env", handle=None, n_cycles=-1)
            env.set_models(_two_models(env))
        refused(entry, STATS, drop=("ret", "mean"))                                     # winners without mean + worst without returns
        refused(entry, END0, n_cycles=0, actions=None, influent=None, drop=("ret", "rew"))          # mean / worst + end rows of no cycle
        if models:      # influent is optional here: its absence is no fault, and the check in front of it is reported
            refused(entry, STATS, influent=None, drop=("ret",))
            refused(entry, NO_ACT, actions=None, influent=None, drop=("ret",))          # mean / worst + NULL actions
        else:
            refused(entry, NO_INFL, influent=None, drop=("ret",))                       # mean / worst + NULL influent
            refused(entry, NO_ACT, actions=None, influent=None)                         # NULL influent + NULL actions
        refused(entry, BRANCHES, n_cycles=0, actions=None, influent=None, fanout=2 ** 15, n_scen=2 ** 15, drop=("rew",))      # end rows + 2^31
        refused(entry, BRANCHES, actions=None, fanout=2 ** 15, n_scen=2 ** 15)          # NULL actions + the 2^31 bound with n_scen
        refused(entry, FANOUT, actions=None, fanout=0)                                  # NULL actions + fanout
        refused(entry, PAIRS, actions=None, fanout=2 ** 30, drop=("mean",))             # winners, NULL actions + N * fanout >= 2^31
        if models:
            refused(entry, GRID, fanout=2 ** 15, n_scen=2 ** 16)                        # the 2^31 bound with n_scen + the grid's y axis
            refused(entry, GRID, fanout=0, n_scen=2 ** 16)                              # fanout + the grid's y axis
            refused(entry, CYCLES, n_cycles=-1, n_scen=2 ** 16)                         # the grid's y axis + n_cycles < 0
        refused(entry, SCEN, fanout=0, n_scen=0)                                        # fanout + n_scen < 1
        refused(entry, CYCLES, n_cycles=-1, n_scen=0)                                   # n_scen < 1 + n_cycles < 0
        refused(entry, CYCLES, n_cycles=-1, fanout=2 ** 15, n_scen=2 ** 15, drop=("ret",))          # mean / worst, 2^31 + n_cycles < 0
        refused(entry, "NULL env", handle=None, n_cycles=-1, n_scen=0, fanout=0)        # three faults + NULL env
    assert_sentinels(outs)
    env.close()
