"""Where the ordinary call's code lies in the text of k_step's one-wave scheme-1 builds (cross-compiled here, no GPU needed), held
where profiles/r22_notes.md found it.  scripts/analysis/step_layout.py walks the ordinary call (scripts/analysis/step_path.py)
and gives every instruction on it a byte offset from the assembler's own encodings.

Round 22 marked the rare branches of these builds unlikely (profiles/r22_notes.md).  K_STEP / K_STEP_SMALL, parent -> reached:

    bytes on the path (one step loop included)   17 284 / 17 260 -> 15 888 / 15 868   (kernel: 46 880 / 46 808 -> 46 508 / 46 432)
    64-byte lines the path touches               278 / 277 -> 254 / 254
    span of the path, first to last byte         32 892 / 32 820 -> 31 720 / 31 644 bytes
    untouched lines inside the span              236 / 236 -> 242 / 241
      ... holding a step loop the call skips     91 / 92 -> 91 / 92  (the interval's other regime, 45 lines; the idle phase's, 45)
      ... other                                  145 / 144 -> 151 / 149
    taken forward / backward branches            10 / 1 -> 8 / 2

The direct-form output stores, the trace export, the per-lane ring form, the further ring appends and the m1-row fetch now lie behind
s_endpgm.  The residue inside the span, and why hints do not remove it:
  * the other regime's controller and plan code around its step loop (2 716 bytes, 41 lines): either regime is an ordinary call, the
    path can be contiguous for one of them only;
  * the terminal phases around the idle loop (settler, draw: ~7 000 bytes, ~107 lines).  The end-of-episode test is a per-lane
    branch; marked unlikely, the compiler still lays the terminal phases in front of the join they fall into and moves the small
    block that only the not-done lanes run behind s_endpgm instead (hence the second backward branch).  Taking them out needs a
    non-inlined function with its own register allocation, which was not built;
  * one 280-byte fragment (3 lines) between the reward's blocks.
So the bounds are the reached values + 10 %, as tests/test_step_spill_cpu.py holds its counts."""
import importlib.util
import os

import pytest
from conftest import ROOT
from isa import K_STEP, K_STEP_SMALL, kernel_text, library_asm

# span in bytes, untouched lines that are not a skipped step loop, taken forward branches, lines touched
REACHED = {K_STEP: (31720, 151, 8, 254), K_STEP_SMALL: (31644, 149, 8, 254)}


@pytest.fixture(scope="module")
def asm():
    return library_asm()


@pytest.fixture(scope="module")
def step_layout():
    spec = importlib.util.spec_from_file_location("step_layout", os.path.join(ROOT, "scripts", "analysis", "step_layout.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("kernel", [K_STEP, K_STEP_SMALL])
def test_ordinary_path_does_not_scatter_further(asm, step_layout, kernel):
    span0, holes0, fwd0, lines0 = REACHED[kernel]
    r = step_layout.layout(kernel_text(asm, kernel))
    print(kernel, {k: v for k, v in r.items() if not k.startswith("_")})
    # the walk is the ordinary call's: entered at the preload header's target, one step loop run, ended at s_endpgm
    assert r["first"] == 256 and r["instructions"] > 2300 and r["lines"] > 200, r["first"]
    assert r["holes"] == r["holes_loops"] + r["holes_other"] and r["span_lines"] == r["lines"] + r["holes"]
    assert 40 <= r["holes_loops"] <= 110, r["holes_loops"]             # the two skipped step loops (439 - 442 instructions each)
    assert r["holes_other"] <= 1.1 * holes0, r["holes_other"]
    assert r["span"] <= 1.1 * span0, r["span"]
    assert r["taken_forward"] <= fwd0 and r["taken_backward"] <= 2 and r["lines"] <= 1.1 * lines0, (r["taken_forward"], r["lines"])


def test_offsets_follow_the_encodings(step_layout):
    """The sizes come from the assembler: 4-byte scalar and VOP1/VOP2 forms, 8 bytes with a literal or in the VOP3 / memory
    encodings, and .p2align pads."""
    text = "\n".join(["s_mov_b32 s0, 0", "s_mov_b32 s1, 0x12345", "v_fma_f64 v[0:1], v[2:3], v[4:5], v[6:7]",
                      "s_load_dword s2, s[4:5], 0x40", ".p2align 6", ".LBB0_1:", "v_mov_b32_e32 v0, s0", "s_endpgm"])
    assert step_layout.offsets(text) == [(0, 4), (4, 8), (12, 8), (20, 8), (64, 4), (68, 4)]
