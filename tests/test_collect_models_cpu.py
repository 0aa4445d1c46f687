"""sbr_reset_models and sbr_collect_policy_models without a GPU: the two entry points are declared, exported and bound; a NULL
handle is refused under the entry point's name before anything is touched; the Python surface exists on SbrOSVec, is forwarded by
the sharding wrapper and refused by SBR-v2, and model_index is the rule (on stand-ins); k_models_collect_policy lives in a unit of
its own; and its gfx950 ISA (from the once-per-run cross-compile of tests/isa.py) reads the model as the parent reads the handle's
constants - no more vector loads than k_collect_policy's same build, the tape kernel's arithmetic in the Butcher-5 step loops with
no scratch instruction in them, no scratch segment in the two 32-wide one-wave builds, and in the other builds the parent's own
scratch segment as the yardstick.  The device-side checks are in tests/test_collect_models_gpu.py."""
import collections
import ctypes as C
import inspect
import os
import re
import types

import pytest
from conftest import ROOT
from isa import b5_steps, f64_mix, flop_counts, instructions, kernel_names, kernel_text, library_asm, meta, unit_asms
from test_policy_rollout_cpu import _policy

from gym_sbr2_amd import _capi
from gym_sbr2_amd import build as B

UNIT = "sbr_policy_collect_models.hip"
# (H, OCI, cfg.scheme, waves per SIMD) of the 12 builds: scheme 0 has no one-wave build
BUILDS = [(h, oci, sch, wv) for h in (32, 64) for oci in (0, 1) for sch, wv in ((1, 1), (1, 2), (0, 2))]
IDS = ["h%d-%s-scheme%d-%dwave" % (h, "oci" if oci else "eqi", sch, wv) for h, oci, sch, wv in BUILDS]
K_MOD = {b: "_Z23k_models_collect_policyILi%dELb%dELi%dELi%dEE" % b for b in BUILDS}
K_COL = {b: "_Z16k_collect_policyILi%dELb%dELi%dELi%dEE" % b for b in BUILDS}
# k_reset_models<OutT, CARRY, BLK> and k_reset<OutT, CARRY, BLK>
RESETS = [(t, carry, blk) for t in "fd" for carry in (0, 1) for blk in (256, 512)]
NO_SCRATCH = ((32, 0, 1, 1), (32, 1, 1, 1))
# Scratch bytes a build of k_models_collect_policy may carry OVER k_collect_policy's same build in the same compile: the measured
# excess where a build stayed above the yardstick (DESIGN.md 3.12 records it next to the scalar-spill counts), 0 everywhere else.
SCRATCH_EXCESS = {}


def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "sbr_amd.h")) as f:
        header = f.read()
    want = {"sbr_reset_models": 10, "sbr_collect_policy_models": 12}
    for name, n_args in want.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert m.group(1).startswith("sbr_env* env, int64_t envs_per_model,"), name
    assert re.search(r"^#define SBR_ABI_VERSION 6$", header, re.M)
    lib = _capi.load()
    raw = C.CDLL(_capi.library_path())
    for name, n_args in want.items():
        assert getattr(raw, name) is not None
        res, args = _capi.SYMBOLS[name]
        fn = getattr(lib, name)
        assert fn.restype is res is C.c_int and list(fn.argtypes) == args and len(args) == n_args, name
        assert args[1] is C.c_int64, name
    # the parents' arguments behind the handle and envs_per_model (the reset's carry_over picks between its two parents)
    assert _capi.SYMBOLS["sbr_collect_policy_models"][1][2:] == _capi.SYMBOLS["sbr_collect_policy"][1][1:]
    assert _capi.SYMBOLS["sbr_reset_models"][1][3:] == _capi.SYMBOLS["sbr_reset"][1][1:] == _capi.SYMBOLS["sbr_reset_carry"][1][1:]
    assert lib.sbr_abi_version() == 6 == _capi.ABI_VERSION          # functions were added: no struct or record changed


def test_null_env_is_refused_before_anything_is_touched():
    lib = _capi.load()
    bufs = {name: (ct * n)(*[7] * n) for name, ct, n in (
        ("obs", C.c_float, 18), ("ret", C.c_double, 1), ("acts", C.c_float, 2), ("rew", C.c_double, 1), ("rows", C.c_float, 18),
        ("flags", C.c_uint8, 1), ("infl", C.c_double, 14), ("mask", C.c_uint8, 1), ("robs", C.c_float, 18))}
    p = {name: C.cast(v, C.c_void_p) for name, v in bufs.items()}
    pol = _policy()
    # no handle can exist without a device: every call is refused, and the entry point is named
    for epm in (256, 0, 300):
        for outs in ((p["rows"], p["flags"]), (None, None), (p["rows"], None)):
            rc = lib.sbr_collect_policy_models(None, epm, 3, 1, C.byref(pol), p["obs"], p["ret"], p["acts"], p["rew"], *outs, None)
            assert rc == -1 and lib.sbr_last_error(None) == b"sbr_collect_policy_models: NULL env", lib.sbr_last_error(None)
        for carry in (0, 1):
            for infl in (p["infl"], None):
                rc = lib.sbr_reset_models(None, epm, carry, 5, None, None, infl, p["mask"], p["robs"], None)
                assert rc == -1 and lib.sbr_last_error(None) == b"sbr_reset_models: NULL env", lib.sbr_last_error(None)
    # the policy checks are policy_error's, also here: the last failing check is reported
    rc = lib.sbr_collect_policy_models(None, 256, 3, 1, None, p["obs"], p["ret"], None, None, None, None, None)
    assert rc == -1 and lib.sbr_last_error(None) == b"sbr_collect_policy_models: NULL policy"
    bad = _policy(n_hidden=3)
    rc = lib.sbr_collect_policy_models(None, 256, 3, 1, C.byref(bad), p["obs"], p["ret"], None, None, None, None, None)
    assert rc == -1 and b"sbr_collect_policy_models: " in lib.sbr_last_error(None) and b"n_hidden" in lib.sbr_last_error(None)
    for name, v in bufs.items():
        assert list(v) == [7] * len(v), name


# ---------------------------------------------------------------------------------------------- the Python surface
def test_python_surface():
    torch = pytest.importorskip("torch")
    from gym_sbr2_amd import ShardedSbrOS, SbrEnv2Vec, SbrOSVec, cycle_env, models, sharding
    want = {
        "set_models": (["self", "models"], []),
        "model_index": (["self", "envs_per_model"], []),
        "reset_models": (["self", "envs_per_model", "seed", "scenario", "rnd", "influent", "mask", "carry_over"],
                         [0, None, None, None, None, False]),
        "collect_policy_models": (["self", "policy", "n_steps", "envs_per_model", "hold", "obs", "noise_std", "noise_seed"],
                                  [1, None, None, 0]),
        "rollout_policy_models": (["self", "policy", "n_steps", "envs_per_model", "hold", "obs", "noise_std", "noise_seed",
                                   "return_actions", "return_rewards"], [1, None, None, 0, False, False]),
    }
    for cls in (SbrOSVec, ShardedSbrOS):
        for name, (params, defaults) in want.items():
            sig = inspect.signature(getattr(cls, name))
            assert list(sig.parameters) == params, (cls, name)
            assert [p.default for p in sig.parameters.values() if p.default is not inspect.Parameter.empty] == defaults, (cls, name)
    assert isinstance(vars(SbrOSVec)["num_models"], property)
    # rollout_policy's arguments plus envs_per_model
    rp = list(inspect.signature(SbrOSVec.rollout_policy).parameters)
    assert [q for q in want["rollout_policy_models"][0] if q != "envs_per_model"] == rp
    # both classes' set_models / num_models go through ONE helper; the mixin keeps its own attributes (tests/test_cycle_models_cpu.py)
    for cls in (SbrOSVec, cycle_env.CycleLookahead):
        assert "set_table" in inspect.getsource(vars(cls)["set_models"]) and "lib.sbr_set_models" not in inspect.getsource(vars(cls)["set_models"])
        assert "table_size" in inspect.getsource(vars(cls)["num_models"].fget)
    assert SbrEnv2Vec.set_models is vars(cycle_env.CycleLookahead)["set_models"]
    calls = []
    lib = types.SimpleNamespace(sbr_num_models=lambda h: calls.append(h) or 3)
    assert models.table_size(types.SimpleNamespace(lib=lib, _h="handle")) == 3 and calls == ["handle"]
    # the new methods go through the shared policy inputs; the rollout form is the collector's entry point without its two outputs
    for name in ("collect_policy_models", "rollout_policy_models"):
        src = inspect.getsource(getattr(SbrOSVec, name)) + inspect.getsource(SbrOSVec._collect)
        assert "_policy_inputs" in src and "sbr_collect_policy_models" in src, name
    assert "None, None, self._stream()" in inspect.getsource(SbrOSVec.rollout_policy_models)
    # SBR-v2 refuses them in the words of its siblings, before it looks at an argument
    tail = "belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch"
    for name in ("reset_models", "collect_policy_models", "rollout_policy_models"):
        assert name in cycle_env._REFUSED
        with pytest.raises(NotImplementedError, match=tail):
            getattr(SbrEnv2Vec, name)(object())
    # the sharding wrapper forwards them to its SbrOSVec unchanged
    seen = []

    class Env:
        def __getattr__(self, name):
            return lambda *a, **k: seen.append((name, a, k)) or name

    sh = ShardedSbrOS.__new__(ShardedSbrOS)
    sh.env = Env()
    for name in want:
        assert name in sharding._FORWARDED
        assert getattr(sh, name)(1, 2, x=3) == name and seen[-1] == (name, (1, 2), {"x": 3})
        assert ("SbrOSVec.%s for this rank's block" % name) in getattr(ShardedSbrOS, name).__doc__
    assert torch is not None


def test_model_index_is_the_rule():
    torch = pytest.importorskip("torch")
    from gym_sbr2_amd import SbrOSVec

    def env(first, n, m):
        return types.SimpleNamespace(first_env_id=first, num_envs=n, num_models=m)

    for first, n, m, per in ((0, 600, 2, 256), (768, 512, 2, 256), (768, 1100, 3, 512), (0, 1100, 3, 256), (768, 300, 16, 256)):
        got = SbrOSVec.model_index(env(first, n, m), per)
        assert got.dtype == torch.int64 and tuple(got.shape) == (n,)
        assert got.tolist() == [((first + i) // per) % m for i in range(n)], (first, n, m, per)
    assert SbrOSVec.model_index(env(0, 600, 2), 256).tolist() == [0] * 256 + [1] * 256 + [0] * 88
    assert SbrOSVec.model_index(env(768, 512, 2), 256).tolist() == [1] * 256 + [0] * 256
    # one model: envs_per_model is not read, nor is first_env_id
    for per in (0, 300, None):
        assert SbrOSVec.model_index(env(64, 5, 1), per).tolist() == [0] * 5
    # where the library refuses the rule
    for first, m, per in ((0, 0, 256), (0, 2, 0), (0, 2, 300), (0, 2, -256), (64, 2, 256), (-256, 2, 256)):
        with pytest.raises(ValueError):
            SbrOSVec.model_index(env(first, 8, m), per)


# ---------------------------------------------------------------------------------------------- the unit and its ISA
def test_the_kernels_have_a_unit_of_their_own():
    assert os.path.join(os.path.dirname(B.SRC), UNIT) in B.SOURCES
    with open(B.SRC) as f:
        assert '#include "%s"' % UNIT in f.read()
    owners = collections.defaultdict(list)
    for unit, text in unit_asms().items():
        for k in kernel_names(text):
            if "k_models_collect_policy" in k:
                owners[k].append(unit)
    assert len(owners) == 12, sorted(owners)              # H x OCI x {(1, 1), (1, 2), (0, 2)}
    assert all(sum(k.startswith(prefix) for k in owners) == 1 for prefix in K_MOD.values()), sorted(owners)
    assert all(u == [UNIT] for u in owners.values()), dict(owners)
    # ... that unit owns nothing else, and the parent's unit still owns the parent's builds and nothing else
    assert all("k_models_collect_policy" in k for k in kernel_names(unit_asms()[UNIT]))
    parents = kernel_names(unit_asms()["sbr_policy_collect.hip"])
    assert len(parents) == 12 and all(k.startswith("_Z16k_collect_policyI") for k in parents), parents
    # k_reset_models sits next to k_reset
    resets = [k for k in kernel_names(unit_asms()["sbr_core.hip"]) if k.startswith("_Z14k_reset_modelsI")]
    assert len(resets) == 8 and not any("k_reset_models" in k for u, t in unit_asms().items() if u != "sbr_core.hip" for k in kernel_names(t))


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def _vector_loads(asm, symbol):
    return [i for i in instructions(kernel_text(asm, symbol)) if i.split()[0].startswith(("global_load", "flat_load", "buffer_load"))]


@pytest.mark.parametrize("build", BUILDS, ids=IDS)
def test_the_model_is_not_read_per_lane(asm, build):
    """A model is some 190 doubles.  Read per lane it would add hundreds of vector loads; read as the parent reads the handle's
    constants - wave-uniform, through scalar loads - it adds none: the allowance over k_collect_policy's same build is zero."""
    mine, theirs = len(_vector_loads(asm, K_MOD[build])), len(_vector_loads(asm, K_COL[build]))
    print("[info] vector loads %s: models %d, parent %d" % (build, mine, theirs))
    assert mine <= theirs, (build, mine, theirs)


@pytest.mark.parametrize("build", [b for b in BUILDS if b[2] == 1], ids=[i for b, i in zip(BUILDS, IDS) if b[2] == 1])
def test_step_loops_are_the_tape_kernels_and_hold_no_scratch(asm, build):
    import bench
    steps = b5_steps(kernel_text(asm, K_MOD[build]), 700)
    assert len(steps) >= 2, build
    flop = flop_counts(steps)
    assert flop[0] == bench.FP64_FLOP_PER_B5_STEP["plain"] and flop[-1] == bench.FP64_FLOP_PER_B5_STEP["dosing"], (build, flop)
    for l in steps:
        m = f64_mix(l)
        assert m["fma"] * 2 + m["mul"] + m["add"] + m["rcp"] in bench.FP64_FLOP_PER_B5_STEP.values(), (build, m)
        assert m["div"] == 0 and m["scratch"] == 0, (build, m)


@pytest.mark.parametrize("build", NO_SCRATCH, ids=["h32-eqi", "h32-oci"])
def test_the_32_wide_one_wave_builds_have_no_scratch_segment(asm, build):
    """The parent has none there and sits 116 and 93 registers below 512."""
    k = K_MOD[build]
    figures = {key: (meta(asm, k, key), meta(asm, K_COL[build], key)) for key in ("vgpr_count", "sgpr_spill_count", "private_segment_fixed_size")}
    print("[info] %s models / parent: %s" % (build, figures))
    assert meta(asm, k, "private_segment_fixed_size") == 0 and f64_mix(instructions(kernel_text(asm, k)))["scratch"] == 0, figures
    assert meta(asm, k, "vgpr_count") <= 512


@pytest.mark.parametrize("build", [b for b in BUILDS if b not in NO_SCRATCH], ids=[i for b, i in zip(BUILDS, IDS) if b not in NO_SCRATCH])
def test_scratch_against_the_parents_build(asm, build):
    """The yardstick is k_collect_policy's same build in the SAME compile (the two-waves builds carry 336 to 1 080 B there, the
    64-wide one-wave OCI build 44 B); SCRATCH_EXCESS is 0 unless a build was measured above it."""
    figures = {key: (meta(asm, K_MOD[build], key), meta(asm, K_COL[build], key))
               for key in ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    print("[info] %s models / parent: %s" % (build, figures))
    mine, theirs = figures["private_segment_fixed_size"]
    assert mine <= theirs + SCRATCH_EXCESS.get(build, 0), (build, figures)
    assert meta(asm, K_MOD[build], "vgpr_count") <= (512 if build[3] == 1 else 256)


@pytest.mark.parametrize("build", RESETS, ids=["%s-carry%d-%d" % (("f32" if t == "f" else "f64"), c, blk) for t, c, blk in RESETS])
def test_reset_models_has_no_more_scratch_than_k_reset(asm, build):
    mine, theirs = "_Z14k_reset_modelsI%sLb%dELi%dEE" % build, "_Z7k_resetI%sLb%dELi%dEE" % build
    figures = {key: (meta(asm, mine, key), meta(asm, theirs, key)) for key in ("vgpr_count", "sgpr_spill_count", "private_segment_fixed_size")}
    print("[info] k_reset_models / k_reset %s: %s" % (build, figures))
    assert figures["private_segment_fixed_size"][0] <= figures["private_segment_fixed_size"][1], figures
    assert len(_vector_loads(asm, mine)) <= len(_vector_loads(asm, theirs)), build
