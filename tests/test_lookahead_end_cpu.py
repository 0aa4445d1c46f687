"""sbr_lookahead_actions_end, sbr_lookahead_sampled_end and sbr_branch_best without a GPU: the entry points are exported and
bound, they refuse bad arguments before anything is touched, the Python surface exists, and the gfx950 ISA of the two new
kernels (float32 tape, SBROS-v1 reward; from the once-per-run cross-compile of tests/isa.py) keeps what
tests/test_lookahead_cpu.py asserts for their parents - register budgets, no scratch in the one-wave build, nothing but
arithmetic in the Butcher-5 step loops - with a store count bounded by what the outputs need.

The Python surface: the end outputs come from methods of their own, lookahead_end / lookahead_sampled_end (one per C entry
point), and the planner's terminal value is an attribute.  tests/test_lookahead_cpu.py and tests/test_mppi_cpu.py pin the
parameter lists of lookahead, lookahead_sampled and MppiPlanner.__init__ exactly, so those stay as they are."""
import ctypes as C
import inspect

import pytest
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from isa import b5_steps, f64_mix, flop_counts, instructions, kernel_text, library_asm, meta, vector_stores

from gym_sbr2_amd import _capi

# k_lookahead_tape_end<float, false, SCH, WAVES> and k_lookahead_sampled_end<float, false, SCH, WAVES>
K_END = {(sch, wv): "_Z20k_lookahead_tape_endIfLb0ELi%dELi%dEE" % (sch, wv) for sch, wv in ((1, 1), (1, 2), (0, 2))}
K_SEND = {(sch, wv): "_Z23k_lookahead_sampled_endIfLb0ELi%dELi%dEE" % (sch, wv) for sch, wv in ((1, 1), (1, 2), (0, 2))}
NEW = ("sbr_lookahead_actions_end", "sbr_lookahead_sampled_end", "sbr_branch_best")


def test_symbols_are_exported_and_bound():
    lib = _capi.load()
    raw = C.CDLL(_capi.library_path())
    for name, n_args in zip(NEW, (13, 15, 6)):
        assert name in _capi.SYMBOLS
        assert getattr(raw, name) is not None
        res, args = _capi.SYMBOLS[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and len(args) == n_args, name
    assert lib.sbr_abi_version() == 6                  # added functions: no signature, struct or record width changed


def _buffers():
    tape = (C.c_float * 8)()
    ret, best = (C.c_double * 4)(*[7.0] * 4), (C.c_double * 2)(*[7.0] * 2)
    idx = (C.c_int32 * 2)(*[7] * 2)
    rew = (C.c_double * 4)(*[7.0] * 4)
    obs, st, dn = (C.c_float * 72)(*[7.0] * 72), (C.c_float * 60)(*[7.0] * 60), (C.c_uint8 * 4)(*[7] * 4)
    return tape, ret, best, idx, rew, obs, st, dn


def _untouched(ret, best, idx, rew, obs, st, dn):
    assert list(ret) == [7.0] * 4 and list(rew) == [7.0] * 4 and list(best) == [7.0] * 2 and list(idx) == [7] * 2
    assert list(obs) == [7.0] * 72 and list(st) == [7.0] * 60 and list(dn) == [7] * 4


def test_lookahead_actions_end_refuses_without_a_device():
    lib = _capi.load()
    tape, ret, best, idx, rew, obs, st, dn = _buffers()
    p, r, w, i, b, o, s, d = (C.cast(a, C.c_void_p) for a in (tape, ret, rew, idx, best, obs, st, dn))
    call = lib.sbr_lookahead_actions_end
    # no handle can exist without a device: every refusal is decided before anything is touched (the refusals that need a
    # handle - all three end outputs NULL or n_steps = 0 on a live one, N * fanout >= 2^31 - are in tests/test_lookahead_end_gpu.py)
    refusals = [
        (None, 1, 1, 2, p, r, w, i, b, o, s, d, None),          # NULL env
        (None, -1, 1, 2, p, r, w, i, b, o, s, d, None),         # n_steps < 0
        (None, 0, 1, 2, p, r, w, i, b, o, s, d, None),          # n_steps = 0
        (None, 1, 0, 2, p, r, w, i, b, o, s, d, None),          # hold < 1
        (None, 1, 1, 0, p, r, w, i, b, o, s, d, None),          # fanout < 1
        (None, 1, 1, 2, None, r, w, i, b, o, s, d, None),       # NULL actions
        (None, 1, 1, 2, p, None, w, i, None, o, s, d, None),    # best_index without returns
        (None, 1, 1, 2, p, r, w, i, b, None, None, None, None),  # no end output
    ]
    for args in refusals:
        assert call(*args) == -1, args
        assert b"sbr_lookahead_actions_end" in lib.sbr_last_error(None), args
    _untouched(ret, best, idx, rew, obs, st, dn)


def test_lookahead_sampled_end_refuses_without_a_device():
    lib = _capi.load()
    tape, ret, best, idx, rew, obs, st, dn = _buffers()
    p, r, w, i, b, o, s, d = (C.cast(a, C.c_void_p) for a in (tape, ret, rew, idx, best, obs, st, dn))
    acts = (C.c_float * 8)(*[7.0] * 8)
    a = C.cast(acts, C.c_void_p)

    def sampler(**kw):
        sm = _capi.SbrSampler()
        sm.sigma, sm.lo, sm.hi = (C.c_float * 2)(0.3, 2.0), (C.c_float * 2)(0.0, 0.0), (C.c_float * 2)(2.5, 15.0)
        sm.seed, sm.keep_nominal, sm.reserved_ = 1, 1, 0
        for k, v in kw.items():
            setattr(sm, k, v)
        return C.byref(sm)

    ok = sampler()
    call = lib.sbr_lookahead_sampled_end
    refusals = [
        (None, 1, 1, 2, p, ok, r, w, i, b, a, o, s, d, None),          # NULL env
        (None, -1, 1, 2, p, ok, r, w, i, b, a, o, s, d, None),         # n_steps < 0
        (None, 0, 1, 2, p, ok, r, w, i, b, a, o, s, d, None),          # n_steps = 0
        (None, 1, 0, 2, p, ok, r, w, i, b, a, o, s, d, None),          # hold < 1
        (None, 1, 1, 0, p, ok, r, w, i, b, a, o, s, d, None),          # fanout < 1
        (None, 1, 1, 2 ** 24 + 1, p, ok, r, w, i, b, a, o, s, d, None),  # fanout > 2^24
        (None, 1, 1, 2, None, ok, r, w, i, b, a, o, s, d, None),       # NULL nominal
        (None, 1, 1, 2, p, None, r, w, i, b, a, o, s, d, None),        # NULL sampler
        (None, 1, 1, 2, p, sampler(sigma=(C.c_float * 2)(-1.0, 2.0)), r, w, i, b, a, o, s, d, None),
        (None, 1, 1, 2, p, sampler(lo=(C.c_float * 2)(3.0, 0.0)), r, w, i, b, a, o, s, d, None),       # lo > hi
        (None, 1, 1, 2, p, sampler(reserved_=1), r, w, i, b, a, o, s, d, None),
        (None, 1, 1, 2, p, ok, None, w, None, b, a, o, s, d, None),    # best_return without returns
        (None, 1, 1, 2, p, ok, r, w, i, b, a, None, None, None, None),  # no end output
    ]
    for args in refusals:
        assert call(*args) == -1, args
        assert b"sbr_lookahead_sampled_end" in lib.sbr_last_error(None), args
    _untouched(ret, best, idx, rew, obs, st, dn)
    assert list(acts) == [7.0] * 8


def test_branch_best_refuses_without_a_device():
    lib = _capi.load()
    vals, best, idx = (C.c_double * 4)(*[1.0] * 4), (C.c_double * 2)(*[7.0] * 2), (C.c_int32 * 2)(*[7] * 2)
    v, b, i = (C.cast(a, C.c_void_p) for a in (vals, best, idx))
    for args in [(None, 2, v, i, b, None), (None, 0, v, i, b, None), (None, -1, v, i, b, None), (None, 2, None, i, b, None),
                 (None, 2, v, None, None, None)]:
        assert lib.sbr_branch_best(*args) == -1, args
        assert b"sbr_branch_best" in lib.sbr_last_error(None), args
    assert list(best) == [7.0] * 2 and list(idx) == [7] * 2


def test_python_surface_exists():
    from gym_sbr2_amd import MppiPlanner, ShardedSbrOS, SbrOSVec
    from gym_sbr2_amd.cycle_env import SbrEnv2Vec
    for cls in (SbrOSVec, ShardedSbrOS):
        for name, parent in (("lookahead_end", "lookahead"), ("lookahead_sampled_end", "lookahead_sampled")):
            sig, psig = inspect.signature(getattr(cls, name)), inspect.signature(getattr(cls, parent))
            assert list(sig.parameters) == list(psig.parameters), (cls, name)          # the parent's arguments, word for word
            assert [p.default for p in sig.parameters.values()] == [p.default for p in psig.parameters.values()], (cls, name)
        assert list(inspect.signature(cls.branch_best).parameters) == ["self", "values"]
    for name in ("lookahead_end", "lookahead_sampled_end", "branch_best"):
        with pytest.raises(NotImplementedError):
            getattr(SbrEnv2Vec, name)(None)
    assert MppiPlanner.terminal_value is None and "terminal_value" in inspect.getsource(MppiPlanner.plan)


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def test_end_kernels_register_budgets_and_scratch(asm):
    for ks in (K_END, K_SEND):
        assert meta(asm, ks[1, 1], "private_segment_fixed_size") == 0
        assert f64_mix(instructions(kernel_text(asm, ks[1, 1])))["scratch"] == 0
        assert meta(asm, ks[1, 2], "vgpr_count") <= 256
        assert meta(asm, ks[0, 2], "vgpr_count") <= 256


def test_end_kernels_step_loops(asm):
    import bench
    for ks in (K_END, K_SEND):
        for k in (ks[1, 1], ks[1, 2]):
            steps = b5_steps(kernel_text(asm, k))
            assert len(steps) >= 2, k
            flop = flop_counts(steps)
            assert flop[0] == bench.FP64_FLOP_PER_B5_STEP["plain"] and flop[-1] == bench.FP64_FLOP_PER_B5_STEP["dosing"], (k, flop)
            for l in steps:
                m = f64_mix(l)
                assert m["div"] == 0 and m["scratch"] == 0, (k, m)   # no v_div_fmas_f64, no scratch instruction in any step loop


def test_end_kernels_store_no_more_than_their_outputs_need(asm):
    """The bound is what the outputs need in stores of the widest kind, 16 bytes (global_store_dwordx4), each source store
    compiled once: an obs_end row is 18 adjacent float32 = 72 bytes = 5 stores, a state_end row 15 = 60 bytes = 4, done_end 1,
    returns 1 and rewards_out (in the loop) 1: 12; the sampled kernel adds the actions_out pair: 13.  A build that loses the
    merging of a row's stores, or that stores a row once on the done and once on the not-done path, is above it.  Nothing of
    the handle's 14 + 25 rows is among them, and there is no n_steps = 0 path (the host refuses it)."""
    need = -(-18 * 4 // 16) + -(-15 * 4 // 16) + 1 + 2
    assert need == 12
    for key in K_END:
        assert len(vector_stores(asm, K_END[key])) <= need, (key, vector_stores(asm, K_END[key]))
        assert len(vector_stores(asm, K_SEND[key])) <= need + 1, (key, vector_stores(asm, K_SEND[key]))
