"""sbr_check_model, sbr_set_models, sbr_num_models and sbr_cycle_lookahead_models without a GPU: the entry points are declared,
exported and bound; they refuse a NULL handle before anything is touched; sbr_check_model (host only) accepts exactly the model
fields; PlantModels.perturbed draws what it says; the Python surface exists and RobustCycleSetpointSearch routes to the models
call when asked (on a stand-in env); the kernels live in a translation unit of their own, and their gfx950 ISA (from the
once-per-run cross-compile of tests/isa.py) needs no more scratch than k_cycle's build of the same scheme and waves, stores no more
than the outputs need and - the condition that shows the model block is read with scalar loads - has no more vector loads than
k_cycle_lookahead_scenarios plus the stored-influent path.  The device-side checks are in tests/test_cycle_models_gpu.py."""
import ctypes as C
import inspect
import types

import numpy as np
import pytest
from cycle_kit import assert_declared_exported_and_bound, assert_null_env_refused, assert_unit_of_its_own, host_outputs
from isa import instructions, kernel_text, library_asm, meta, vector_stores

from gym_sbr2_amd import _capi

UNIT = "sbr_cycle_models.hip"
# (cfg.scheme, waves per SIMD) of the builds: scheme 0 has no one-wave build
BUILDS = ((1, 1), (1, 2), (0, 2))
K_MODELS = {(t,) + b: "_Z24k_cycle_lookahead_modelsI%sLi%dELi%dEE" % ((t,) + b) for t in "fd" for b in BUILDS}     # float32 / float64 tape
K_SCEN = {(t,) + b: "_Z27k_cycle_lookahead_scenariosI%sLi%dELi%dEE" % ((t,) + b) for t in "fd" for b in BUILDS}
K_CYCLE = {b: "_Z7k_cycleIffLi%dELi%dEE" % b for b in BUILDS}
ALL = sorted(K_MODELS)
ALL_IDS = ["%s-scheme%d-%dwave" % (("f32" if t == "f" else "f64"), s, w) for t, s, w in ALL]

MODEL_FIELDS = "Ya Yh fp ixb ixp muH Ks Koh Kno bH eta_g eta_h kh Kx muA Knh bA Koa ka So_sat".split()


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_and_bound({
        "sbr_check_model": (r"^int sbr_check_model\(const sbr_config\* base /\* NULL = defaults \*/, const sbr_config\* model\);", 2),
        "sbr_set_models": (r"^int sbr_set_models\(sbr_env\* env, int32_t n_models, const sbr_config\* models", 3),
        "sbr_num_models": (r"^int64_t sbr_num_models\(const sbr_env\* env\);", 1),
        "sbr_cycle_lookahead_models": (
            r"^int sbr_cycle_lookahead_models\(sbr_env\* env, int32_t n_cycles, int32_t fanout, int32_t n_scen,", 16)})
    assert _capi.SYMBOLS["sbr_num_models"][0] is C.c_int64
    assert _capi.SYMBOLS["sbr_cycle_lookahead_models"] == _capi.SYMBOLS["sbr_cycle_lookahead_scenarios"]


def test_null_env_is_refused_before_anything_is_touched():
    lib = _capi.load()
    bufs, p = host_outputs()
    outs = tuple(p[name] for name in "ret rew mean worst idx best obs diag st".split())
    assert_null_env_refused("sbr_cycle_lookahead_models", [(None, 1, 2, 2, p["tape"], p["infl"]) + outs + (None,),
                                                           (None, 1, 2, 2, p["tape"], None) + outs + (None,),
                                                           (None, -1, 0, 70000, None, None, None) + outs[1:] + (None,)], bufs)
    models = (_capi.SbrConfig * 2)(_capi.default_config(), _capi.default_config())
    models[1].t_delta = 7.0                            # not looked at: there is no config to check it against
    before = bytes(models)
    assert_null_env_refused("sbr_set_models", [(None, 2, models), (None, -1, None), (None, 0, None)], bufs)
    assert lib.sbr_num_models(None) == -1
    assert lib.sbr_last_error(None) == b"sbr_num_models: NULL env", lib.sbr_last_error(None)
    assert bytes(models) == before


# ---------------------------------------------------------------------------------------------- sbr_check_model
def _check(base, model):
    lib = _capi.load()
    rc = lib.sbr_check_model(None if base is None else C.byref(base), None if model is None else C.byref(model))
    return rc, (lib.sbr_last_error(None) or b"").decode()


def test_check_model_accepts_the_model_fields_and_nothing_else():
    base = _capi.default_config()
    assert [n for n, _ in _capi.SbrConfig._fields_[:19]] + ["So_sat"] == MODEL_FIELDS      # the struct's order
    assert _check(None, base)[0] == 0 and _check(base, base)[0] == 0
    for name in MODEL_FIELDS:                          # each alone, and against an explicit base as against the defaults
        m = _capi.default_config()
        setattr(m, name, getattr(m, name) * 1.0625)
        assert _check(base, m)[0] == 0 and _check(None, m)[0] == 0, name
    everything = _capi.default_config()
    for name in MODEL_FIELDS:
        setattr(everything, name, getattr(everything, name) * 0.9375)
    assert _check(base, everything)[0] == 0
    # every field outside the model fields, scalars and array entries, named in the refusal
    other = [n for n, _ in _capi.SbrConfig._fields_ if n not in MODEL_FIELDS]
    assert {"t_delta", "scheme", "reward_kind", "Kc_DO", "x0", "t_ratio", "out_f64"} <= set(other) and len(other) == 43
    for name in other:
        cur = getattr(base, name)
        if hasattr(cur, "__len__"):
            for k in (0, 2, 3, len(cur) - 1):
                m = _capi.default_config()
                getattr(m, name)[k] = cur[k] * 1.5
                rc, msg = _check(base, m)
                assert rc == -1 and msg.startswith("sbr_check_model: %s[%d] differs" % (name, k)), (name, k, msg)
        else:
            m = _capi.default_config()
            setattr(m, name, cur + 1 if isinstance(cur, int) else cur * 1.5 + 1.0)
            rc, msg = _check(base, m)
            assert rc == -1 and msg.startswith("sbr_check_model: %s differs" % name), (name, msg)
    # the first such field in the struct's order is the one named, model fields changed beside it or not
    m = _capi.default_config()
    m.muA, m.scheme, m.Kc_DO, m.x0[3] = 0.3, 0, 90.0, 1.0
    assert _check(base, m)[1].startswith("sbr_check_model: Kc_DO differs")
    # against another base: what differs is relative to the base given
    other_base = _capi.default_config(); other_base.scheme = 0
    m = _capi.default_config(); m.scheme, m.muH = 0, 5.0
    assert _check(other_base, m)[0] == 0 and _check(base, m)[1].startswith("sbr_check_model: scheme differs")


def test_check_model_gives_the_creation_check_of_an_invalid_model():
    base = _capi.default_config()
    m = _capi.default_config(); m.muA = 0.0
    assert _check(base, m) == (-1, "sbr_check_model: muH, muA, kh, eta_g, Koh, bH and Ya must be positive")
    m = _capi.default_config(); m.Koa = -1.0
    assert _check(None, m) == (-1, "sbr_check_model: Koa must be positive")
    assert _check(base, None) == (-1, "sbr_check_model: NULL model")


# ---------------------------------------------------------------------------------------------- PlantModels
def _values(cfg, fields):
    return [getattr(cfg, f) for f in fields]


def test_plant_models_perturbed():
    import gym_sbr2_amd
    from gym_sbr2_amd import models as M
    assert gym_sbr2_amd.PlantModels is M.PlantModels
    assert list(M.MODEL_FIELDS) == MODEL_FIELDS and len(M.MODEL_KINETICS) == 14 and set(M.MODEL_KINETICS) < set(MODEL_FIELDS)
    sig = inspect.signature(M.PlantModels.perturbed)
    assert list(sig.parameters) == ["cfg", "n", "rel_std", "seed", "fields", "clip", "keep_nominal"]
    assert [p.default for p in sig.parameters.values()][2:] == [0.1, 0, M.MODEL_KINETICS, 2.0, True]
    assert "VALIDITY DOMAIN" in M.PlantModels.perturbed.__doc__ and "several times faster" in M.PlantModels.perturbed.__doc__
    cfg = _capi.default_config()
    every = [n for n, _ in _capi.SbrConfig._fields_]
    a, b, c = (M.PlantModels.perturbed(cfg, 5, rel_std=0.2, seed=s) for s in (3, 3, 4))
    assert len(a) == 5 and bytes(a.c_array()) == bytes(b.c_array()) != bytes(c.c_array())         # deterministic in seed
    assert bytes(a[0]) == bytes(cfg)                                                              # keep_nominal: model 0 is cfg
    # z in field order, then model order; the factor exp(rel_std * z); nothing else moves
    factor = np.exp(0.2 * np.random.RandomState(3).standard_normal((14, 4)))
    kept = [f for f in every if f not in M.MODEL_KINETICS]
    for m in range(1, 5):
        for k, f in enumerate(M.MODEL_KINETICS):
            assert getattr(a[m], f) == getattr(cfg, f) * factor[k, m - 1] != getattr(cfg, f), (m, f)
        for f in kept:
            u, v = getattr(a[m], f), getattr(cfg, f)
            assert (list(u) == list(v)) if hasattr(u, "__len__") else u == v, (m, f)
    # named fields only; the yields and So_sat only if named
    d = M.PlantModels.perturbed(cfg, 3, rel_std=0.3, seed=1, fields=("muA", "So_sat", "Yh"), keep_nominal=False)
    assert len(d) == 3
    for m in range(3):
        assert all(getattr(d[m], f) != getattr(cfg, f) for f in ("muA", "So_sat", "Yh"))
        assert _values(d[m], [f for f in MODEL_FIELDS if f not in ("muA", "So_sat", "Yh")]) == _values(
            cfg, [f for f in MODEL_FIELDS if f not in ("muA", "So_sat", "Yh")])
    # clip: with rel_std = 3 most factors lie outside [1/1.25, 1.25] and land on its ends
    e = M.PlantModels.perturbed(cfg, 9, rel_std=3.0, seed=2, clip=1.25, keep_nominal=False)
    ratios = np.array([[getattr(e[m], f) / getattr(cfg, f) for f in M.MODEL_KINETICS] for m in range(9)])
    assert ratios.min() >= 0.8 * (1 - 1e-15) and ratios.max() <= 1.25 * (1 + 1e-15)
    assert np.isclose(ratios, 0.8).sum() > 20 and np.isclose(ratios, 1.25).sum() > 20
    with pytest.raises(ValueError):
        M.PlantModels.perturbed(cfg, 2, fields=("t_delta",))
    with pytest.raises(ValueError):
        M.PlantModels.perturbed(cfg, 0)
    # the constructor checks each config with the library, against the first or against a base, and copies
    bad = _capi.default_config(); bad.Kc_DO = 90.0
    with pytest.raises(ValueError, match="model 1: sbr_check_model: Kc_DO differs"):
        M.PlantModels([cfg, bad])
    with pytest.raises(ValueError, match="model 0: sbr_check_model: Kc_DO differs"):
        M.PlantModels([bad], base=cfg)
    assert len(M.PlantModels([bad, bad])) == 2                                                    # against the first of them
    own = M.PlantModels([cfg])
    cfg.muA = 9.0
    assert own[0].muA == 0.5 and bytes(own.c_array()) == bytes(own[0])


# ---------------------------------------------------------------------------------------------- the Python surface
def test_python_surface():
    pytest.importorskip("torch")
    from gym_sbr2_amd import cycle_env, planner
    from gym_sbr2_amd.cycle_env import CycleLookahead, SbrEnv2Vec
    want = {
        "set_models": (["self", "models"], []),
        "cycle_lookahead_models": (["self", "candidates", "influent", "n_scen", "return_rewards", "return_stats", "return_best",
                                    "return_end", "return_status"], [None, None] + [False] * 5),
    }
    for name, (params, defaults) in want.items():
        sig = inspect.signature(getattr(SbrEnv2Vec, name))
        assert list(sig.parameters) == params, name
        assert [p.default for p in sig.parameters.values() if p.default is not inspect.Parameter.empty] == defaults, name
        assert name not in cycle_env._REFUSED and name not in vars(SbrEnv2Vec) and getattr(SbrEnv2Vec, name) is vars(CycleLookahead)[name]
    assert isinstance(vars(CycleLookahead)["num_models"], property)

    class NoLibrary:                                   # any call into the library, num_models included, fails the test
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    one_env = types.SimpleNamespace(num_envs=1, lib=NoLibrary(), _h=None)
    ok_c, ok_i = np.zeros((1, 1, 1, 3)), np.zeros((1, 1, 2, 14))
    for cand, infl, n_scen in ((np.zeros((1, 1, 3)), ok_i, None), (np.zeros((1, 2, 1, 3)), None, 2), (ok_c, np.zeros((1, 1, 1, 13)), None),
                               (np.zeros((2, 1, 1, 3)), ok_i, None), (ok_c, ok_i, 3), (ok_c, None, 0), (ok_c, None, 65536),
                               (np.zeros((1, 1, 2 ** 16, 3)), None, 65535)):
        with pytest.raises(ValueError):
            SbrEnv2Vec.cycle_lookahead_models(one_env, cand, infl, n_scen)
    # the planner: the signature the scenarios test pins, the switch a class attribute that defaults to off
    assert list(inspect.signature(planner.RobustCycleSetpointSearch.__init__).parameters) == [
        "self", "env", "K", "n_scen", "n_cycles", "iters", "elite_frac", "seed", "risk"]
    assert vars(planner.RobustCycleSetpointSearch)["plant_models"] is False
    assert "s % env.num_models" in planner.RobustCycleSetpointSearch.__doc__


class _StandIn:
    """A CPU stand-in for SbrEnv2Vec whose two lookaheads are recorded.  The return of a branch is -|a - target_s|^2 summed over
    the tape; under cycle_lookahead_models the odd futures run a second 'plant' that moves their target by 0.2."""
    num_envs, num_models = 2, 2

    def __init__(self, torch):
        self.torch, self.device, self.action_dtype, self.calls = torch, torch.device("cpu"), torch.float32, []

    def influent_futures(self, n_cycles, n_scen, seed=0, scenario=None, first_draw=0, current_first=True):
        out = self.torch.zeros((n_cycles, self.num_envs, n_scen, 14), dtype=self.torch.float64)
        out[..., 1] = self.torch.tensor((0.1, 0.1, 0.3, 0.5), dtype=self.torch.float64)
        return out

    def _look(self, name, cand, influent, shift):
        self.calls.append((name, cand, influent))
        a = cand.to(self.action_dtype).double()
        target = influent[:, :, None, :, 1:2] + shift * (self.torch.arange(influent.shape[2]) % self.num_models)[:, None]
        ret = -((a[:, :, :, None, :] - target) ** 2).sum(dim=(0, 4))
        return ret, ret.mean(dim=2), ret.min(dim=2).values, self.torch.zeros(ret.shape, dtype=self.torch.uint8)

    def cycle_lookahead_scenarios(self, cand, influent, return_stats=False, return_status=False):
        assert return_stats and return_status
        return self._look("scenarios", cand, influent, 0.0)

    def cycle_lookahead_models(self, cand, influent=None, n_scen=None, return_stats=False, return_status=False):
        assert return_stats and return_status and n_scen is None
        return self._look("models", cand, influent, 0.2)


@pytest.mark.parametrize("risk", ["mean", "worst"])
def test_robust_search_routes_to_the_models_call(risk):
    torch = pytest.importorskip("torch")
    from gym_sbr2_amd.planner import RobustCycleSetpointSearch
    values = {}
    for on in (False, True):
        env = _StandIn(torch)
        search = RobustCycleSetpointSearch(env, K=16, n_scen=4, n_cycles=2, iters=3, elite_frac=0.25, seed=3, risk=risk)
        assert search.plant_models is False
        search.plant_models = on
        action, value = search.plan()
        assert [c[0] for c in env.calls] == ["models" if on else "scenarios"] * 3
        assert all(c[2] is search.futures and tuple(c[1].shape) == (2, 2, 16, 3) for c in env.calls)      # the plan's futures
        look = env.cycle_lookahead_models if on else env.cycle_lookahead_scenarios
        _, mean, worst, _ = look(search.tape[:, :, None, :], search.futures, return_stats=True, return_status=True)
        assert torch.equal(value, (mean if risk == "mean" else worst)[:, 0]) and torch.equal(action, search.tape[0].float())
        values[on] = value
    assert not torch.equal(values[False], values[True])                    # another score, not the same one under another name


# ---------------------------------------------------------------------------------------------- the unit and its ISA
def test_the_kernels_have_a_unit_of_their_own():
    assert_unit_of_its_own(UNIT, K_MODELS.values())                            # the six builds, nothing else


@pytest.fixture(scope="module")
def asm():
    return library_asm()


@pytest.mark.parametrize("build", ALL, ids=ALL_IDS)
def test_no_more_scratch_than_k_cycle(asm, build):
    """The yardstick is k_cycle's build of the same scheme and waves in the SAME compile (0, 92 B and 0 there today).  The register
    counts are printed and not asserted.  Measured (this compile, either tape): scheme 1 one wave 278 + 22 registers, no scratch;
    scheme 1 two waves 254 registers and 88 B; scheme 0 two waves 225 registers, no scratch."""
    mod, cyc = K_MODELS[build], K_CYCLE[build[1:]]
    figures = {k: (meta(asm, mod, k), meta(asm, cyc, k)) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size")}
    print("[info] k_cycle_lookahead_models against k_cycle, %s tape, scheme %d, %d wave(s): %s" % (build + (figures,)))
    assert figures["private_segment_fixed_size"][0] <= figures["private_segment_fixed_size"][1], figures


@pytest.mark.parametrize("build", ALL, ids=ALL_IDS)
def test_stores_no_more_than_the_outputs_need(asm, build):
    """returns 1, one rewards_out entry 1, the end rows 3 + 12 values, the status byte 1: 18 stores if none of them merge
    (measured: 11).  Nothing of the handle's rows is among them: k_cycle, which stores the plant, has 25."""
    stores = vector_stores(asm, K_MODELS[build])
    assert len(stores) <= 1 + 1 + 3 + 12 + 1, stores
    assert len(stores) < len(vector_stores(asm, K_CYCLE[build[1:]]))


def _vector_loads(asm, symbol):
    return [i for i in instructions(kernel_text(asm, symbol)) if i.split()[0].startswith(("global_load", "flat_load"))]


@pytest.mark.parametrize("build", ALL, ids=ALL_IDS)
def test_the_model_is_not_read_per_lane(asm, build):
    """A model is some 190 doubles.  Read per lane it would add hundreds of vector loads to the kernel; read as the sibling
    kernels read the handle's constants - wave-uniform, through scalar loads - it adds none.  The allowance over
    k_cycle_lookahead_scenarios' build is the second influent path (the env's stored influent: fourteen rows at the most).
    Measured: 28 / 29 (float32 / float64 tape) against 22 / 23."""
    mine, theirs = len(_vector_loads(asm, K_MODELS[build])), len(_vector_loads(asm, K_SCEN[build]))
    print("[info] vector loads, %s tape, scheme %d, %d wave(s): models %d, scenarios %d" % (build + (mine, theirs)))
    assert mine <= theirs + 14, (mine, theirs)
