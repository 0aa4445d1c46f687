"""The spill traffic of k_step's one-wave builds, held where profiles/r12_notes.md left it (cross-compiled here, no GPU needed).
k_step reads its wave-uniform constants and pointers again behind the step loops instead of keeping them across; before that the
compiler spilled 153 scalar registers into VGPR lanes and the kernel's straight-line code held 604 lane operations and 251 AGPR
moves.  Upper bounds: the counts reached + 10 %, so the traffic cannot grow back unnoticed.  Only lane, accumulator-move, spill,
scalar-load and wait counts are looked at - the arithmetic of the step loops is tests/test_isa_cpu.py's."""
import collections
import importlib.util
import os

import pytest
from conftest import ROOT
from isa import K_STEP, K_STEP_SMALL, _loops, f64_mix, kernel_text, library_asm, meta

PARENT_LANE, PARENT_SPILL = 604, 153           # k_step<float, float, 256, false, 1, 1> before
# reached: lane operations outside the step loops, AGPR moves outside them, spilled SGPRs, scalar loads, lgkmcnt waits (whole kernel)
REACHED = {K_STEP: (96, 16, 38, 150, 71), K_STEP_SMALL: (96, 8, 38, 150, 72)}


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def split(text):
    """(instructions inside the Butcher-5 step loops, instructions outside them)."""
    lines, loops = _loops(text)
    inside = set()
    for a, b in loops:
        body = [x for x in lines[a:b + 1] if not x.endswith(":")]
        if f64_mix(body)["rcp"] == 6 and len(body) < 580:
            inside.update(range(a, b + 1))
    ins = [l for i, l in enumerate(lines) if i in inside and not l.endswith(":")]
    out = [l for i, l in enumerate(lines) if i not in inside and not l.endswith(":")]
    return ins, out


@pytest.mark.parametrize("kernel", [K_STEP, K_STEP_SMALL])
def test_spill_traffic_of_the_one_wave_builds_stays_down(asm, kernel):
    lane0, acc0, spill0, load0, wait0 = REACHED[kernel]
    ins, out = split(kernel_text(asm, kernel))
    assert len(ins) > 2000, len(ins)                                   # the step loops were found
    c = collections.Counter(i.split()[0] for i in out)
    lane = c["v_readlane_b32"] + c["v_writelane_b32"]
    acc = sum(v for k, v in c.items() if k.startswith("v_accvgpr"))
    loads = sum(v for k, v in c.items() if k.startswith("s_load"))
    waits = sum(1 for i in out if i.startswith("s_waitcnt") and "lgkmcnt" in i)
    spill = meta(asm, kernel, "sgpr_spill_count")
    print(kernel, "lane %d accvgpr %d sgpr_spill %d s_load %d lgkmcnt waits %d" % (lane, acc, spill, loads, waits))
    assert f64_mix(ins)["lane"] == 0                                   # the loops themselves: no lane operation
    assert lane <= 1.1 * lane0 and 2 * lane <= PARENT_LANE, lane
    assert spill <= 1.1 * spill0 and 2 * spill <= PARENT_SPILL, spill
    assert acc <= 1.1 * acc0, acc
    assert loads <= 1.1 * load0 and waits <= 1.1 * wait0, (loads, waits)
    assert meta(asm, kernel, "vgpr_count") <= 336 and meta(asm, kernel, "private_segment_fixed_size") == 0


# The ORDINARY call (one interval, not done: scripts/analysis/step_path.py walks it through the assembly), outside the step loops.
# Parent: 2 567 / 2 552 instructions, 311 lane operations, 113 / 109 AGPR moves, 65 scalar loads, 39 lgkmcnt waits.
PARENT_PATH_WAITS = 39
PATH_REACHED = {K_STEP: (64, 0, 71, 2303), K_STEP_SMALL: (64, 0, 71, 2297)}     # lane, AGPR moves, scalar loads, instructions


@pytest.mark.parametrize("kernel", [K_STEP, K_STEP_SMALL])
def test_ordinary_call_path_of_the_one_wave_builds(asm, kernel):
    spec = importlib.util.spec_from_file_location("step_path", os.path.join(ROOT, "scripts", "analysis", "step_path.py"))
    sp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sp)
    blocks, path, decisions = sp.walk(kernel_text(asm, kernel))
    c = sp.counts(blocks, path)
    print(kernel, c)
    lane0, acc0, load0, n0 = PATH_REACHED[kernel]
    assert c["step_loops_run"] == 1 and len(decisions) > 40, (c, len(decisions))      # one interval, and the walk reached the stores
    assert c["lane"] <= 1.1 * lane0 and 2 * c["lane"] <= 311, c
    assert c["accvgpr"] <= 1.1 * acc0 and c["s_load"] <= 1.1 * load0 and c["instructions"] <= 1.1 * n0, c
    assert c["lgkm_wait"] <= PARENT_PATH_WAITS + 2, c                # the re-reads add at most two waits to a call
