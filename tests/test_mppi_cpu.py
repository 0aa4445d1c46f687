"""sbr_lookahead_sampled and sbr_mppi_update without a GPU: both entry points are exported, declared and bound, struct sbr_sampler
has the header's layout, every refusal that needs no handle is made before anything is touched, the Python surface exists, and the
gfx950 ISA of the sampled fan-out kernel (k_lookahead_sampled, cross-compiled once per run by tests/isa.py) keeps what
tests/test_lookahead_cpu.py asserts for k_lookahead_tape: register budgets, no scratch in the one-wave build, nothing but
arithmetic in the Butcher-5 step loops, next to no vector stores."""
import ctypes as C
import inspect
import os
import re

import pytest
from conftest import ROOT
from isa import b5_steps, f64_mix, flop_counts, instructions, kernel_text, library_asm, meta, vector_stores

from gym_sbr2_amd import _capi

# k_lookahead_sampled<float, false, SCH, WAVES>: the float32 tape, the SBROS-v1 reward
K_SAMP = "_Z19k_lookahead_sampledIfLb0ELi1ELi1EE"       # scheme 1, register budget for one wave per SIMD (up to 98 304 branches)
K_SAMP_2W = "_Z19k_lookahead_sampledIfLb0ELi1ELi2EE"    # scheme 1, two waves per SIMD
K_SAMP_RK4 = "_Z19k_lookahead_sampledIfLb0ELi0ELi2EE"   # scheme 0, two waves per SIMD
K_MPPI = "_Z13k_mppi_updateIfE"
NAMES = ("sbr_lookahead_sampled", "sbr_mppi_update")


def test_symbols_are_exported_declared_and_bound():
    lib = _capi.load()
    raw = C.CDLL(_capi.library_path())
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sbr_amd.h")).read(), flags=re.S)
    for name, nargs in zip(NAMES, (12, 11)):
        assert name in _capi.SYMBOLS and getattr(raw, name) is not None
        res, args = _capi.SYMBOLS[name]
        assert getattr(lib, name).restype is res and list(getattr(lib, name).argtypes) == args and len(args) == nargs
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert lib.sbr_abi_version() == 6                  # added functions: no signature, struct or record width changed


def test_sampler_struct_has_the_headers_layout():
    s = _capi.SbrSampler
    assert C.sizeof(s) == 40
    assert [(n, getattr(s, n).offset, getattr(s, n).size) for n, _ in s._fields_] == [
        ("sigma", 0, 8), ("lo", 8, 8), ("hi", 16, 8), ("seed", 24, 8), ("keep_nominal", 32, 4), ("reserved_", 36, 4)]
    header = open(os.path.join(ROOT, "include", "sbr_amd.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header.split("typedef struct sbr_sampler {")[1].split("} sbr_sampler;")[0], flags=re.S)
    assert re.findall(r"(\w+)\s*(?:\[2\])?\s*[,;]", body) == ["sigma", "lo", "hi", "seed", "keep_nominal", "reserved_"]


def _sampler(**kw):
    s = _capi.SbrSampler()
    s.sigma, s.lo, s.hi = (C.c_float * 2)(0.5, 1.0), (C.c_float * 2)(0.0, 0.0), (C.c_float * 2)(8.0, 15.0)
    s.seed, s.keep_nominal, s.reserved_ = 3, 1, 0
    for k, v in kw.items():
        setattr(s, k, (C.c_float * 2)(*v) if isinstance(v, tuple) else v)
    return C.byref(s)


BAD_SAMPLERS = [dict(sigma=(-1.0, 1.0)), dict(sigma=(1.0, float("nan"))), dict(sigma=(float("inf"), 1.0)),
                dict(lo=(float("-inf"), 0.0)), dict(hi=(8.0, float("nan"))), dict(lo=(9.0, 0.0)), dict(reserved_=1)]


def test_lookahead_sampled_refuses_bad_arguments_without_a_device():
    lib = _capi.load()
    tape, acts = (C.c_float * 4)(), (C.c_float * 8)(*[7.0] * 8)
    ret, best, rew = (C.c_double * 4)(*[7.0] * 4), (C.c_double * 2)(*[7.0] * 2), (C.c_double * 4)(*[7.0] * 4)
    idx = (C.c_int32 * 2)(*[7] * 2)
    p, r, w, i, b, a = (C.cast(v, C.c_void_p) for v in (tape, ret, rew, idx, best, acts))
    ok = _sampler()
    # no handle can exist without a device: every refusal is decided before anything is touched.  (N * fanout >= 2^31 needs a
    # handle to have an N, and the refusals on a live handle are in tests/test_mppi_gpu.py.)
    refusals = [
        (None, 1, 1, 2, p, ok, r, w, i, b, a, None),           # NULL env
        (None, -1, 1, 2, p, ok, r, w, i, b, a, None),          # n_steps < 0
        (None, 1, 0, 2, p, ok, r, w, i, b, a, None),           # hold < 1
        (None, 1, 1, 0, p, ok, r, w, i, b, a, None),           # fanout < 1
        (None, 1, 1, 2 ** 24 + 1, p, ok, r, w, i, b, a, None),  # fanout > 2^24
        (None, 1, 1, 2, None, ok, r, w, i, b, a, None),        # NULL nominal with n_steps > 0
        (None, 1, 1, 2, p, None, r, w, i, b, a, None),         # NULL sampler
        (None, 1, 1, 2, p, ok, None, w, i, None, a, None),     # best_index without returns
        (None, 1, 1, 2, p, ok, None, w, None, b, a, None),     # best_return without returns
    ] + [(None, 1, 1, 2, p, _sampler(**kw), r, w, i, b, a, None) for kw in BAD_SAMPLERS]
    for args in refusals:
        assert lib.sbr_lookahead_sampled(*args) == -1, args
        assert b"sbr_lookahead_sampled" in lib.sbr_last_error(None), args
    assert list(ret) == [7.0] * 4 and list(rew) == [7.0] * 4 and list(best) == [7.0] * 2 and list(idx) == [7] * 2
    assert list(acts) == [7.0] * 8


def test_mppi_update_refuses_bad_arguments_without_a_device():
    lib = _capi.load()
    tape, out = (C.c_float * 4)(), (C.c_float * 4)(*[7.0] * 4)
    ret, wts = (C.c_double * 4)(*[1.0] * 4), (C.c_double * 4)(*[7.0] * 4)
    p, r, o, w = (C.cast(v, C.c_void_p) for v in (tape, ret, out, wts))
    ok = _sampler()
    refusals = [
        (None, 1, 2, p, ok, r, 1.0, 0, o, w, None),            # NULL env
        (None, 0, 2, p, ok, r, 1.0, 0, o, w, None),            # rows < 1
        (None, 1, 0, p, ok, r, 1.0, 0, o, w, None),            # fanout < 1
        (None, 1, 2 ** 24 + 1, p, ok, r, 1.0, 0, o, w, None),  # fanout > 2^24
        (None, 1, 2, None, ok, r, 1.0, 0, o, w, None),         # NULL nominal
        (None, 1, 2, p, None, r, 1.0, 0, o, w, None),          # NULL sampler
        (None, 1, 2, p, ok, None, 1.0, 0, o, w, None),         # NULL returns
        (None, 1, 2, p, ok, r, 1.0, 0, None, w, None),         # NULL nominal_out
        (None, 1, 2, p, ok, r, 0.0, 0, o, w, None),            # temperature not > 0
        (None, 1, 2, p, ok, r, -1.0, 0, o, w, None),
        (None, 1, 2, p, ok, r, float("nan"), 0, o, w, None),
        (None, 1, 2, p, ok, r, float("inf"), 0, o, w, None),   # temperature not finite
        (None, 1, 2, p, ok, r, 1e-320, 0, o, w, None),         # 1 / temperature not finite
        (None, 1, 2, p, ok, r, 1.0, -1, o, w, None),           # shift < 0
    ] + [(None, 1, 2, p, _sampler(**kw), r, 1.0, 0, o, w, None) for kw in BAD_SAMPLERS]
    for args in refusals:
        assert lib.sbr_mppi_update(*args) == -1, args
        assert b"sbr_mppi_update" in lib.sbr_last_error(None), args
    assert list(out) == [7.0] * 4 and list(wts) == [7.0] * 4


def test_python_surface_exists():
    import gym_sbr2_amd
    from gym_sbr2_amd import MppiPlanner, ShardedSbrOS, SbrOSVec, TapeSampler
    from gym_sbr2_amd.cycle_env import SbrEnv2Vec
    for cls in (SbrOSVec, ShardedSbrOS):
        sig = inspect.signature(cls.lookahead_sampled)
        assert list(sig.parameters) == ["self", "nominal", "fanout", "sampler", "n_steps", "hold", "return_rewards", "return_best",
                                        "return_actions"]
        assert [sig.parameters[k].default for k in list(sig.parameters)[4:]] == [None, 1, False, False, False]
        sig = inspect.signature(cls.mppi_update)
        assert list(sig.parameters) == ["self", "nominal", "returns", "sampler", "temperature", "shift", "out", "return_weights"]
        assert [sig.parameters[k].default for k in ("shift", "out", "return_weights")] == [0, None, False]
    with pytest.raises(NotImplementedError):
        SbrEnv2Vec.lookahead_sampled(None)
    with pytest.raises(NotImplementedError):
        SbrEnv2Vec.mppi_update(None)
    sig = inspect.signature(TapeSampler.__init__)
    assert list(sig.parameters) == ["self", "sigma", "seed", "lo", "hi", "keep_nominal"]
    assert [sig.parameters[k].default for k in ("seed", "lo", "hi", "keep_nominal")] == [0, None, None, True]
    sig = inspect.signature(MppiPlanner.__init__)
    assert list(sig.parameters) == ["self", "env", "rows", "fanout", "sampler", "temperature", "hold"]
    assert sig.parameters["hold"].default == 1 and callable(MppiPlanner.plan)
    assert gym_sbr2_amd.TapeSampler is TapeSampler
    # the defaults come from the config: lo = (0, 0), hi = (act_DO_max, act_EC_max)
    cfg = _capi.default_config()
    s = TapeSampler((0.25, 2.0), seed=2 ** 64 + 5).c_struct(cfg)
    assert isinstance(s, _capi.SbrSampler) and list(s.sigma) == [0.25, 2.0] and list(s.lo) == [0.0, 0.0]
    assert list(s.hi) == [C.c_float(cfg.act_DO_max).value, C.c_float(cfg.act_EC_max).value]
    assert (s.seed, s.keep_nominal, s.reserved_) == (5, 1, 0)
    s = TapeSampler(0.5, lo=(1.0, 2.0), hi=3.0, keep_nominal=False).c_struct(cfg)
    assert (list(s.sigma), list(s.lo), list(s.hi), s.keep_nominal) == ([0.5, 0.5], [1.0, 2.0], [3.0, 3.0], 0)


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def test_sampled_kernel_register_budgets_and_scratch(asm):
    assert meta(asm, K_SAMP, "private_segment_fixed_size") == 0
    assert f64_mix(instructions(kernel_text(asm, K_SAMP)))["scratch"] == 0
    assert meta(asm, K_SAMP_2W, "vgpr_count") <= 256
    assert meta(asm, K_SAMP_RK4, "vgpr_count") <= 256


def test_sampled_kernel_step_loops(asm):
    import bench
    for k in (K_SAMP, K_SAMP_2W):
        steps = b5_steps(kernel_text(asm, k))
        assert len(steps) >= 2, k
        flop = flop_counts(steps)
        assert flop[0] == bench.FP64_FLOP_PER_B5_STEP["plain"] and flop[-1] == bench.FP64_FLOP_PER_B5_STEP["dosing"], (k, flop)
        for l in steps:
            m = f64_mix(l)
            assert m["div"] == 0 and m["scratch"] == 0, (k, m)       # no v_div_fmas_f64, no scratch instruction in any step loop


def test_sampled_kernel_holds_next_to_no_stores(asm):
    """returns (twice: the n_steps = 0 path), rewards_out and actions_out (the first row, the later rows): fewer than 10."""
    for k in (K_SAMP, K_SAMP_2W, K_SAMP_RK4):
        assert len(vector_stores(asm, k)) < 10, (k, vector_stores(asm, k))


def test_update_kernel_is_small_and_spills_nothing(asm):
    assert meta(asm, K_MPPI, "private_segment_fixed_size") == 0
    assert f64_mix(instructions(kernel_text(asm, K_MPPI)))["scratch"] == 0
