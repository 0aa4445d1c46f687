"""sbr_rollout_actions without a GPU: the entry point is exported and refuses bad arguments, and the gfx950 ISA of the tape
kernel (k_rollout_tape, cross-compiled as tests/test_isa_cpu.py does) keeps what is asserted there for k_rollout - register
budgets, no scratch in the one-wave build, nothing but arithmetic in the Butcher-5 step loops."""
import ctypes as C

import pytest
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from isa import (K_ROLLOUT, K_TAPE, K_TAPE_2W, K_TAPE_F64, K_TAPE_RK4, b5_steps, f64_mix, flop_counts, instructions, kernel_text,
                 library_asm, meta, rk4_loops)

from gym_sbr2_amd import _capi


def test_symbol_is_exported_and_bad_arguments_are_refused_without_a_device():
    lib = _capi.load()
    assert "sbr_rollout_actions" in _capi.SYMBOLS and getattr(C.CDLL(_capi.library_path()), "sbr_rollout_actions") is not None
    tape = (C.c_float * 8)()
    ret = (C.c_double * 4)()
    p = C.cast(tape, C.c_void_p)
    # no handle can exist without a device: every refusal below is decided before anything is touched
    assert lib.sbr_rollout_actions(None, 1, 1, p, C.cast(ret, C.c_void_p), None, None) == -1      # NULL env
    assert lib.sbr_rollout_actions(None, 1, 0, p, None, None, None) == -1                          # hold = 0
    assert lib.sbr_rollout_actions(None, -1, 1, p, None, None, None) == -1                         # n_steps = -1
    assert lib.sbr_rollout_actions(None, 1, 1, None, None, None, None) == -1                       # NULL actions, n_steps > 0
    assert b"sbr_rollout_actions" in lib.sbr_last_error(None)
    assert list(ret) == [0.0] * 4


def test_python_surface_exists():
    from gym_sbr2_amd import ShardedSbrOS, SbrOSVec
    import inspect
    for cls in (SbrOSVec, ShardedSbrOS):
        sig = inspect.signature(cls.rollout_actions)
        assert list(sig.parameters) == ["self", "actions", "n_steps", "hold", "return_rewards"]
        assert (sig.parameters["n_steps"].default, sig.parameters["hold"].default, sig.parameters["return_rewards"].default) == (None, 1, False)


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def test_tape_kernel_register_budgets_and_scratch(asm):
    assert meta(asm, K_TAPE, "private_segment_fixed_size") == 0
    assert f64_mix(instructions(kernel_text(asm, K_TAPE)))["scratch"] == 0
    assert meta(asm, K_TAPE, "vgpr_count") <= 320
    assert meta(asm, K_TAPE_2W, "vgpr_count") <= 256
    assert meta(asm, K_TAPE_RK4, "vgpr_count") <= 256


def test_tape_kernel_step_loops(asm):
    import bench
    text = kernel_text(asm, K_TAPE)
    # scheme 1 carries no RK4 loop for the control intervals; scheme 0 keeps its two
    rk4 = lambda k: rk4_loops(kernel_text(asm, k))   # noqa: E731
    assert len(rk4(K_TAPE)) == 0 and len(rk4(K_TAPE_2W)) == 0 and len(rk4(K_TAPE_RK4)) >= 2
    for k in (K_TAPE, K_TAPE_2W):
        steps = b5_steps(kernel_text(asm, k))
        assert len(steps) >= 2, k
        flop = flop_counts(steps)
        assert flop[0] == bench.FP64_FLOP_PER_B5_STEP["plain"] and flop[-1] == bench.FP64_FLOP_PER_B5_STEP["dosing"], (k, flop)
        for l in steps:
            assert f64_mix(l)["div"] == 0, k                       # no v_div_fmas_f64 in any step loop
    for l in b5_steps(text):
        m = f64_mix(l)
        arith = m["fma"] + m["mul"] + m["add"] + m["rcp"]
        assert arith in (477, 537) and len(l) <= arith + 45 and m["scratch"] == 0 and m["lane"] <= 4, (len(l), m)


def test_tape_reads_are_one_load_per_lane_and_row(asm):
    """The pair (u_DO, u_EC) of a lane is one 8-byte load of the float32 tape and one 16-byte load of the float64 tape: against
    k_rollout, which reads the same rows of the handle, the tape kernel holds exactly two more loads - the first row before
    the loop over the calls, the next row inside it."""
    loads = lambda k, op: sum(1 for i in instructions(kernel_text(asm, k)) if i.split()[0] == op)   # noqa: E731
    assert loads(K_TAPE, "global_load_dwordx2") == loads(K_ROLLOUT, "global_load_dwordx2") + 2
    assert loads(K_TAPE, "global_load_dword") == 0 and loads(K_TAPE, "flat_load_dwordx2") == 0
    assert loads(K_TAPE_F64, "global_load_dwordx4") == 2
