"""sbr_lookahead_actions without a GPU: the entry point is exported and refuses bad arguments before anything is touched, the
Python surface exists, and the gfx950 ISA of the read-only fan-out kernel (k_lookahead_tape, cross-compiled as
tests/test_tape_rollout_cpu.py does) keeps what is asserted there for k_rollout_tape - register budgets, no scratch in the
one-wave build, nothing but arithmetic in the Butcher-5 step loops - and holds next to no vector stores: the tape kernel writes
14 + 25 rows of the handle, this one writes none of them (tests/test_lookahead_gpu.py decides "read-only" on the device)."""
import ctypes as C
import inspect

import pytest
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from isa import (K_LOOK, K_LOOK_2W, K_LOOK_RK4, K_TAPE, b5_steps, f64_mix, flop_counts, instructions, kernel_text, library_asm, meta,
                 vector_stores as _vector_stores)

from gym_sbr2_amd import _capi


def test_symbol_is_exported_and_bound():
    lib = _capi.load()
    assert "sbr_lookahead_actions" in _capi.SYMBOLS
    assert getattr(C.CDLL(_capi.library_path()), "sbr_lookahead_actions") is not None
    res, args = _capi.SYMBOLS["sbr_lookahead_actions"]
    assert lib.sbr_lookahead_actions.restype is res and list(lib.sbr_lookahead_actions.argtypes) == args and len(args) == 10
    assert lib.sbr_abi_version() == 6                  # an added function: no signature, struct or record width changed


def test_bad_arguments_are_refused_without_a_device():
    lib = _capi.load()
    tape = (C.c_float * 8)()
    ret, best = (C.c_double * 4)(*[7.0] * 4), (C.c_double * 2)(*[7.0] * 2)
    idx = (C.c_int32 * 2)(*[7] * 2)
    rew = (C.c_double * 4)(*[7.0] * 4)
    p, r, w = C.cast(tape, C.c_void_p), C.cast(ret, C.c_void_p), C.cast(rew, C.c_void_p)
    i, b = C.cast(idx, C.c_void_p), C.cast(best, C.c_void_p)
    call = lib.sbr_lookahead_actions
    # no handle can exist without a device: every refusal below is decided before anything is touched.  (N * fanout >= 2^31
    # needs a handle to have an N: tests/test_lookahead_gpu.py::test_refusals_on_a_live_handle.)
    refusals = [
        (None, 1, 1, 2, p, r, w, i, b, None),          # NULL env
        (None, -1, 1, 2, p, r, w, i, b, None),         # n_steps < 0
        (None, 1, 0, 2, p, r, w, i, b, None),          # hold < 1
        (None, 1, 1, 0, p, r, w, i, b, None),          # fanout < 1
        (None, 1, 1, -3, p, r, w, i, b, None),
        (None, 1, 1, 2, None, r, w, i, b, None),       # NULL actions with n_steps > 0
        (None, 1, 1, 2, p, None, w, i, None, None),    # half an answer: best_index alone, no returns
        (None, 1, 1, 2, p, None, w, None, b, None),    # ... best_return alone, no returns
    ]
    for args in refusals:
        assert call(*args) == -1, args
        assert b"sbr_lookahead_actions" in lib.sbr_last_error(None), args
    assert list(ret) == [7.0] * 4 and list(rew) == [7.0] * 4 and list(best) == [7.0] * 2 and list(idx) == [7] * 2


def test_python_surface_exists():
    from gym_sbr2_amd import ShardedSbrOS, SbrOSVec
    from gym_sbr2_amd.cycle_env import SbrEnv2Vec
    for cls in (SbrOSVec, ShardedSbrOS):
        sig = inspect.signature(cls.lookahead)
        assert list(sig.parameters) == ["self", "actions", "n_steps", "hold", "return_rewards", "return_best"]
        assert [sig.parameters[k].default for k in ("n_steps", "hold", "return_rewards", "return_best")] == [None, 1, False, False]
    with pytest.raises(NotImplementedError):
        SbrEnv2Vec.lookahead(None)


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def test_lookahead_kernel_register_budgets_and_scratch(asm):
    assert meta(asm, K_LOOK, "private_segment_fixed_size") == 0
    assert f64_mix(instructions(kernel_text(asm, K_LOOK)))["scratch"] == 0
    assert meta(asm, K_LOOK, "vgpr_count") <= 320
    assert meta(asm, K_LOOK_2W, "vgpr_count") <= 256
    assert meta(asm, K_LOOK_RK4, "vgpr_count") <= 256


def test_lookahead_kernel_step_loops(asm):
    import bench
    for k in (K_LOOK, K_LOOK_2W):
        steps = b5_steps(kernel_text(asm, k))
        assert len(steps) >= 2, k
        flop = flop_counts(steps)
        assert flop[0] == bench.FP64_FLOP_PER_B5_STEP["plain"] and flop[-1] == bench.FP64_FLOP_PER_B5_STEP["dosing"], (k, flop)
        for l in steps:
            m = f64_mix(l)
            assert m["div"] == 0 and m["scratch"] == 0, (k, m)       # no v_div_fmas_f64, no scratch instruction in any step loop


def test_lookahead_kernel_holds_next_to_no_stores(asm):
    """returns, rewards_out and the n_steps = 0 path: fewer than 8 vector stores, where the tape kernel carries the 14 plant
    rows and the 25-row record on top of them."""
    for k in (K_LOOK, K_LOOK_2W, K_LOOK_RK4):
        assert len(_vector_stores(asm, k)) < 8, (k, _vector_stores(asm, k))
    assert len(_vector_stores(asm, K_TAPE)) >= 14 + 25 - 4          # (the record's rows: 25 internal ones, a few shared with public ones)
