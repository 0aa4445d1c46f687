"""sbr_lookahead_actions_models / sbr_lookahead_sampled_models without a GPU: the two entry points are declared, exported and bound; a
NULL handle is refused under the entry point's name before anything is touched; the Python surface exists on SbrOSVec, is forwarded
by the sharding wrapper and refused by SBR-v2; RobustMppiPlanner checks its arguments (on a stand-in env); the two kernels live in a
unit of their own; and their gfx950 ISA (from the once-per-run cross-compile of tests/isa.py) reads the model as the parents read
the handle's constants.  The device-side checks are in tests/test_lookahead_models_gpu.py."""
import collections
import ctypes as C
import inspect
import os
import re
import types

import pytest
from conftest import ROOT
from isa import b5_steps, f64_mix, flop_counts, instructions, kernel_names, kernel_text, library_asm, meta, unit_asms

from gym_sbr2_amd import _capi
from gym_sbr2_amd import build as B

UNIT = "sbr_lookahead_models.hip"
# (ActT, OCI, cfg.scheme, waves per SIMD) of the 12 builds of each kernel: scheme 0 has no one-wave build
BUILDS = [(t, oci, sch, wv) for t in "fd" for oci in (0, 1) for sch, wv in ((1, 1), (1, 2), (0, 2))]
IDS = ["%s-%s-scheme%d-%dwave" % ("f32" if t == "f" else "f64", "oci" if oci else "eqi", sch, wv) for t, oci, sch, wv in BUILDS]
KINDS = ("tape", "sampled")
K_MOD = {"tape": "_Z23k_models_lookahead_tapeI%sLb%dELi%dELi%dEE", "sampled": "_Z26k_models_lookahead_sampledI%sLb%dELi%dELi%dEE"}
K_PAR = {"tape": "_Z16k_lookahead_tapeI%sLb%dELi%dELi%dEE", "sampled": "_Z19k_lookahead_sampledI%sLb%dELi%dELi%dEE"}
CASES = [(kind, b) for kind in KINDS for b in BUILDS]
CASE_IDS = ["%s-%s" % (kind, i) for kind in KINDS for i in IDS]
# Scratch bytes a build may carry OVER its parent's same build in the same compile: the measured excess where a build stayed above
# the yardstick, 0 everywhere else.  No build does (every one carries less than its parent: DESIGN.md 3.13).
SCRATCH_EXCESS = {}


# ---------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "sbr_amd.h")) as f:
        header = f.read()
    want = {"sbr_lookahead_actions_models": 12, "sbr_lookahead_sampled_models": 14}
    for name, n_args in want.items():
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert m.group(1).startswith("sbr_env* env, int32_t n_steps, int32_t hold, int32_t fanout,"), name
    assert re.search(r"^#define SBR_ABI_VERSION 6$", header, re.M)
    lib = _capi.load()
    raw = C.CDLL(_capi.library_path())
    for name, n_args in want.items():
        assert getattr(raw, name) is not None
        res, args = _capi.SYMBOLS[name]
        fn = getattr(lib, name)
        assert fn.restype is res is C.c_int and list(fn.argtypes) == args and len(args) == n_args, name
    # the parents' arguments with mean_out and worst_out in front of the winners
    par, mod = _capi.SYMBOLS["sbr_lookahead_actions"][1], _capi.SYMBOLS["sbr_lookahead_actions_models"][1]
    assert mod == par[:7] + [C.c_void_p, C.c_void_p] + par[7:]
    par, mod = _capi.SYMBOLS["sbr_lookahead_sampled"][1], _capi.SYMBOLS["sbr_lookahead_sampled_models"][1]
    assert mod == par[:8] + [C.c_void_p, C.c_void_p] + par[8:]
    assert lib.sbr_abi_version() == 6 == _capi.ABI_VERSION          # functions were added: no struct or record changed


def test_null_env_is_refused_before_anything_is_touched():
    lib = _capi.load()
    bufs = {name: (ct * n)(*[7] * n) for name, ct, n in (
        ("tape", C.c_float, 2), ("ret", C.c_double, 1), ("rew", C.c_double, 1), ("mean", C.c_double, 1), ("worst", C.c_double, 1),
        ("bi", C.c_int32, 1), ("bv", C.c_double, 1), ("acts", C.c_float, 2))}
    p = {name: C.cast(v, C.c_void_p) for name, v in bufs.items()}
    sm = _capi.SbrSampler()
    sm.sigma, sm.lo, sm.hi = (C.c_float * 2)(0.3, 2.0), (C.c_float * 2)(0.0, 0.0), (C.c_float * 2)(8.0, 15.0)
    outs = (p["ret"], p["rew"], p["mean"], p["worst"], p["bi"], p["bv"])
    # no handle can exist without a device: every call is refused, and the entry point is named
    for n_steps, hold, fanout in ((3, 1, 1), (0, 1, 4), (-1, 0, 0)):
        rc = lib.sbr_lookahead_actions_models(None, n_steps, hold, fanout, p["tape"], *outs, None)
        assert rc == -1 and lib.sbr_last_error(None) == b"sbr_lookahead_actions_models: NULL env", lib.sbr_last_error(None)
        for sampler in (C.byref(sm), None):
            rc = lib.sbr_lookahead_sampled_models(None, n_steps, hold, fanout, p["tape"], sampler, *outs, p["acts"], None)
            assert rc == -1 and lib.sbr_last_error(None) == b"sbr_lookahead_sampled_models: NULL env", lib.sbr_last_error(None)
    for name, v in bufs.items():
        assert list(v) == [7] * len(v), name


def test_the_parents_checks_are_shared_and_not_copied():
    """lookahead_error / lookahead_sampled_error are declared in sbr_host.h and defined once, next to the parents' entry points."""
    csrc = os.path.dirname(B.SRC)
    text = {n: open(os.path.join(csrc, n)).read() for n in ("sbr_host.h", "sbr_tape.hip", "sbr_sampled.hip", UNIT)}
    for fn, owner in (("lookahead_error", "sbr_tape.hip"), ("lookahead_sampled_error", "sbr_sampled.hip")):
        assert re.search(r"SBR_INTERNAL std::string %s\(" % fn, text["sbr_host.h"]), fn
        assert re.search(r"^std::string %s\(" % fn, text[owner], re.M), fn
        assert not re.search(r"^(static )?std::string %s\(" % fn, text[UNIT], re.M) and ("%s(e, " % fn) in text[UNIT], fn
    for word in ("hold must be", "n_steps must be", "NULL actions", "NULL nominal", "sampler."):
        assert word not in text[UNIT], word


# ---------------------------------------------------------------------------------------------- the Python surface
SURFACE = {
    "lookahead_models": (["self", "actions", "n_steps", "hold", "return_rewards", "return_stats", "return_best"],
                         [None, 1, False, False, False]),
    "lookahead_sampled_models": (["self", "nominal", "fanout", "sampler", "n_steps", "hold", "return_rewards", "return_stats",
                                  "return_best", "return_actions"], [None, 1, False, False, False, False]),
}
CALLS = {
    "lookahead_models": (("tape", 7), dict(hold=2, return_stats=True)),
    "lookahead_sampled_models": (("nominal", 16, "sampler"), dict(hold=2, return_best=True, return_actions=True)),
}
REFUSALS = {
    "lookahead_models": "the read-only lookahead over plant models belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
    "lookahead_sampled_models": "the sampled lookahead over plant models belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch",
}


class _Recorder:
    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        return lambda *args, **kwargs: self.seen.append((name, args, kwargs)) or ("result of", name)


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_a_shard_forwards_with_the_signature_it_forwards_to(name):
    pytest.importorskip("torch")
    from gym_sbr2_amd import SbrOSVec, ShardedSbrOS
    params, defaults = SURFACE[name]
    for cls in (SbrOSVec, ShardedSbrOS):
        sig = inspect.signature(getattr(cls, name))
        assert list(sig.parameters) == params, (cls, name)
        assert [q.default for q in sig.parameters.values() if q.default is not inspect.Parameter.empty] == defaults, (cls, name)
    assert getattr(ShardedSbrOS, name) is not getattr(SbrOSVec, name)
    assert "rank's" in getattr(ShardedSbrOS, name).__doc__
    sh = object.__new__(ShardedSbrOS)
    sh.env = _Recorder()
    args, kwargs = CALLS[name]
    assert getattr(sh, name)(*args, **kwargs) == ("result of", name)
    (seen_name, seen_args, seen_kwargs), = sh.env.seen
    sig = inspect.signature(getattr(SbrOSVec, name))
    assert seen_name == name and sig.bind(None, *seen_args, **seen_kwargs).arguments == sig.bind(None, *args, **kwargs).arguments


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_sbr_v2_refuses_in_these_words_before_it_looks_at_an_argument(name):
    pytest.importorskip("torch")
    from gym_sbr2_amd import SbrEnv2Vec, cycle_env
    with pytest.raises(NotImplementedError) as e:
        getattr(SbrEnv2Vec, name)(None)
    assert str(e.value) == REFUSALS[name]
    # on the mixin, beside set_models and num_models: SbrEnv2Vec's own class body stays what it was
    assert name in cycle_env._ON_MIXIN and name in vars(cycle_env.CycleLookahead) and name not in vars(SbrEnv2Vec)


def test_the_methods_size_their_outputs_once_and_check_the_table_first():
    pytest.importorskip("torch")
    from gym_sbr2_amd import SbrOSVec
    for name, entry in (("lookahead_models", "sbr_lookahead_actions_models"), ("lookahead_sampled_models", "sbr_lookahead_sampled_models")):
        src = inspect.getsource(getattr(SbrOSVec, name))
        assert "_fanout_outputs" in src and "n_scen=m" in src and entry in src and "torch.empty" not in src, name
        assert src.index("_models_branches") < src.index("_fanout_outputs"), name
    stub = types.SimpleNamespace(num_models=0, num_envs=70)
    with pytest.raises(ValueError, match="no model table"):
        SbrOSVec._models_branches(stub, 5)
    stub.num_models = 3
    assert SbrOSVec._models_branches(stub, 5) == 3
    with pytest.raises(ValueError, match=r"2\^31"):
        SbrOSVec._models_branches(stub, 2 ** 24)                  # 70 x 2^24 x 3


# ---------------------------------------------------------------------------------------------- the planner, on a stand-in env
class _StubEnv:
    def __init__(self, torch, n=4, m=3):
        self.cfg, self.num_envs, self.m = _capi.default_config(), n, m
        self.action_dtype, self.device = torch.float32, torch.device("cpu")
        self.torch, self.calls = torch, []

    def lookahead_sampled_models(self, nominal, fanout, sampler, hold=1, return_stats=False):
        self.calls.append(("lookahead_sampled_models", sampler.seed, hold, return_stats))
        ret = self.torch.arange(self.num_envs * fanout * self.m, dtype=self.torch.float64).reshape(self.num_envs, fanout, self.m)
        return ret, ret.mean(dim=2), ret.min(dim=2).values

    def mppi_update(self, nominal, returns, sampler, temperature, out=None):
        self.calls.append(("mppi_update", returns.clone(), sampler.seed))
        out.copy_(nominal)
        return out


def test_robust_mppi_planner_arguments_and_scoring():
    torch = pytest.importorskip("torch")
    import gym_sbr2_amd
    from gym_sbr2_amd import MppiPlanner, RobustMppiPlanner, TapeSampler, planner
    assert gym_sbr2_amd.RobustMppiPlanner is planner.RobustMppiPlanner and issubclass(RobustMppiPlanner, MppiPlanner)
    sampler = TapeSampler((0.3, 2.0), seed=40)
    with pytest.raises(ValueError, match="risk"):
        RobustMppiPlanner(_StubEnv(torch), 5, 6, sampler, 1.0, risk="median")
    for risk in ("mean", "worst"):
        env = _StubEnv(torch)
        p = RobustMppiPlanner(env, 5, 6, sampler, 1.0, hold=2, risk=risk)
        assert p.risk == risk and p.terminal_value is None
        with pytest.raises(ValueError, match="terminal_value"):
            p.terminal_value = lambda obs, state: obs
        p.terminal_value = None
        for d in range(2):
            act, scored, full = p.plan(return_returns=True)
            look, upd = env.calls[-2:]
            assert look == ("lookahead_sampled_models", 40 + d, 2, True) and upd[0] == "mppi_update" and upd[2] == 40 + d
            assert full.shape == (4, 6, 3) and act.shape == (4, 2)
            want = full.mean(dim=2) if risk == "mean" else full.min(dim=2).values
            assert torch.equal(scored, want) and torch.equal(upd[1], want)
        assert p.decision == 2 and p.plan().shape == (4, 2)
    # everything else is the parent's: plan() itself is not overridden
    assert "plan" not in vars(RobustMppiPlanner) and "_score" in vars(RobustMppiPlanner)


# ---------------------------------------------------------------------------------------------- the unit and its ISA
def test_the_kernels_have_a_unit_of_their_own():
    assert os.path.join(os.path.dirname(B.SRC), UNIT) in B.SOURCES and len(B.SOURCES) == 12
    with open(B.SRC) as f:
        assert '#include "%s"' % UNIT in f.read()
    units = {u: kernel_names(t) for u, t in unit_asms().items()}
    for kind in KINDS:
        word = "k_models_lookahead_" + kind
        owners = collections.defaultdict(list)
        for unit, names in units.items():
            for k in names:
                if word in k:
                    owners[k].append(unit)
        assert len(owners) == 12 and all(u == [UNIT] for u in owners.values()), dict(owners)
        assert all(sum(k.startswith(K_MOD[kind] % b) for k in owners) == 1 for b in BUILDS), sorted(owners)
    # the unit holds the 24 builds and nothing else; the names do not contain the parents'
    assert len(units[UNIT]) == 24 and all("k_models_lookahead_" in k for k in units[UNIT]), units[UNIT]
    assert not any("k_lookahead_tape" in k or "k_lookahead_sampled" in k for k in units[UNIT])
    # the neighbours hold what they held
    def base(symbol):                                             # _Z<length><name>...: the kernel's name without its arguments
        m = re.match(r"_Z(\d+)", symbol)
        return symbol[m.end():m.end() + int(m.group(1))]

    count = lambda unit: collections.Counter(base(k) for k in units[unit])
    assert count("sbr_cycle_models.hip") == {"k_cycle_lookahead_models": 6}, count("sbr_cycle_models.hip")
    assert count("sbr_tape.hip") == {"k_rollout_tape": 12, "k_lookahead_tape": 12, "k_lookahead_tape_end": 12, "k_branch_best": 1}, count("sbr_tape.hip")
    assert count("sbr_sampled.hip") == {"k_lookahead_sampled": 12, "k_lookahead_sampled_end": 12, "k_mppi_update": 2}, count("sbr_sampled.hip")


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def _loads(asm, symbol, prefixes):
    return [i for i in instructions(kernel_text(asm, symbol)) if i.split()[0].startswith(prefixes)]


@pytest.mark.parametrize("kind,build", CASES, ids=CASE_IDS)
def test_vector_loads_equal_the_parents(asm, kind, build):
    """The statement "the model is read with scalar loads": per build, as many vector loads as the parent build - a model is some
    190 doubles, and read per lane it would add hundreds.  The constants come through s_load, and nothing through flat or buffer
    loads."""
    mine = len(_loads(asm, K_MOD[kind] % build, ("global_load", "flat_load")))
    theirs = len(_loads(asm, K_PAR[kind] % build, ("global_load", "flat_load")))
    print("[info] vector loads %s %s: models %d, parent %d" % (kind, build, mine, theirs))
    assert mine == theirs, (kind, build, mine, theirs)


@pytest.mark.parametrize("kind,build", CASES, ids=CASE_IDS)
def test_the_model_is_read_with_scalar_loads(asm, kind, build):
    """What the equality above stands for, asked directly: nothing comes through flat or buffer loads, and the constants come through
    s_load."""
    assert not _loads(asm, K_MOD[kind] % build, ("flat_load", "buffer_load")), (kind, build)
    assert len(_loads(asm, K_MOD[kind] % build, ("s_load",))) > 20, (kind, build)


@pytest.mark.parametrize("kind,build", CASES, ids=CASE_IDS)
def test_scratch_against_the_parents_build(asm, kind, build):
    """Where the parent build has no scratch segment the models build has none; elsewhere at most the parent's bytes."""
    k, par = K_MOD[kind] % build, K_PAR[kind] % build
    figures = {key: (meta(asm, k, key), meta(asm, par, key))
               for key in ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")}
    print("[info] %s %s models / parent: %s" % (kind, build, figures))
    mine, theirs = figures["private_segment_fixed_size"]
    if theirs == 0:
        assert mine == 0 and f64_mix(instructions(kernel_text(asm, k)))["scratch"] == 0, (kind, build, figures)
    assert mine <= theirs + SCRATCH_EXCESS.get((kind,) + build, 0), (kind, build, figures)
    assert meta(asm, k, "vgpr_count") <= (512 if build[3] == 1 else 256)


@pytest.mark.parametrize("kind,build", [c for c in CASES if c[1][2] == 1], ids=[i for c, i in zip(CASES, CASE_IDS) if c[1][2] == 1])
def test_step_loops_are_the_tape_kernels_and_hold_no_scratch(asm, kind, build):
    import bench
    steps = b5_steps(kernel_text(asm, K_MOD[kind] % build), 700)
    assert len(steps) >= 2, (kind, build)
    flop = flop_counts(steps)
    assert flop[0] == bench.FP64_FLOP_PER_B5_STEP["plain"] and flop[-1] == bench.FP64_FLOP_PER_B5_STEP["dosing"], (kind, build, flop)
    for l in steps:
        m = f64_mix(l)
        assert m["fma"] * 2 + m["mul"] + m["add"] + m["rcp"] in bench.FP64_FLOP_PER_B5_STEP.values(), (kind, build, m)
        assert m["div"] == 0 and m["scratch"] == 0, (kind, build, m)
