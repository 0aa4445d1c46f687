"""The gfx950 assembly of the library, cross-compiled once per Python process, and what the ISA tests (tests/test_isa_cpu.py,
tests/test_tape_rollout_cpu.py, tests/test_policy_rollout_cpu.py, tests/test_lookahead_cpu.py) read from it: the mangled names
of the kernels, the parsers of the instruction text and of the code object's metadata, and the pickers of the integrators'
loops.  A plain module: pytest does not rewrite its asserts, so each carries its message."""
import collections
import functools
import os
import re
import shutil

import pytest

from gym_sbr2_amd import build as B

K_STEP = "_Z6k_stepIffLi256ELb0ELi1ELi1EE"  # k_step<float, float, 256, false, 1, 1>: the kernel bench.py times (scheme 1)
K_STEP_SMALL = "_Z6k_stepIffLi64ELb0ELi1ELi1EE"    # the 64-thread-workgroup build used up to 49152 envs
K_STEP_RK4 = "_Z6k_stepIffLi256ELb0ELi0ELi1EE"   # cfg.scheme = 0: ten RK4 substeps per interval
K_STEP_2W = "_Z6k_stepIffLi256ELb0ELi1ELi2EE"  # the same above 65536 envs: parked call state, two waves per SIMD
K_ROLLOUT = "_Z9k_rolloutILb0ELi1ELi1EE"      # k_rollout<false, 1, 1>: scheme 1, register budget for one wave per SIMD
K_ROLLOUT_2W = "_Z9k_rolloutILb0ELi1ELi2EE"
K_ROLLOUT_RK4 = "_Z9k_rolloutILb0ELi0ELi2EE"
K_CYCLE = "_Z7k_cycleIffLi1ELi1EE"
K_CYCLE_RK4 = "_Z7k_cycleIffLi0ELi2EE"
K_RESET = "_Z7k_resetIfLb0ELi256EE"
K_RESET_CARRY = "_Z7k_resetIfLb1ELi256EE"
K_RESET_WIDE = "_Z7k_resetIfLb0ELi512EE"      # above one wave per SIMD: 512-thread workgroups (one 84 KiB table copy per CU, two waves per SIMD)
K_CYCLE_RESET = "_Z13k_cycle_resetIfLb0EE"
# k_rollout_tape<float, false, SCH, WAVES>: the float32 tape, the SBROS-v1 reward
K_TAPE = "_Z14k_rollout_tapeIfLb0ELi1ELi1EE"        # scheme 1, register budget for one wave per SIMD (up to 98 304 envs)
K_TAPE_2W = "_Z14k_rollout_tapeIfLb0ELi1ELi2EE"     # scheme 1, two waves per SIMD
K_TAPE_RK4 = "_Z14k_rollout_tapeIfLb0ELi0ELi2EE"    # scheme 0, two waves per SIMD
K_TAPE_F64 = "_Z14k_rollout_tapeIdLb0ELi1ELi1EE"    # k_rollout_tape<double, false, 1, 1>: the float64 tape
# k_lookahead_tape<float, false, SCH, WAVES>: the float32 tape, the SBROS-v1 reward
K_LOOK = "_Z16k_lookahead_tapeIfLb0ELi1ELi1EE"       # scheme 1, register budget for one wave per SIMD (up to 98 304 branches)
K_LOOK_2W = "_Z16k_lookahead_tapeIfLb0ELi1ELi2EE"    # scheme 1, two waves per SIMD
K_LOOK_RK4 = "_Z16k_lookahead_tapeIfLb0ELi0ELi2EE"   # scheme 0, two waves per SIMD
# k_rollout_policy<H, false, SCH, WAVES>: the SBROS-v1 reward
K_POL = {(h, sch, wv): "_Z16k_rollout_policyILi%dELb0ELi%dELi%dEE" % (h, sch, wv)
         for h in (32, 64) for sch, wv in ((1, 1), (1, 2), (0, 2))}


@functools.lru_cache(maxsize=None)
def unit_asms():
    """{unit's file name: its assembly text} under the library's own flags, in the order of the build's SOURCES.  Minutes of
    hipcc (the units side by side), so once per process."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    return dict(zip(map(os.path.basename, B.SOURCES), B.compile_library()))


@functools.lru_cache(maxsize=None)
def library_asm():
    """The assembly text of the whole library: the units' texts one behind the other.  The module-scoped `asm` fixtures of the
    four test files all return this one string."""
    return "".join(unit_asms().values())


def kernel_names(asm):
    """The symbols of the kernels in the code objects' metadata: every `.name:` of every amdhsa.kernels list of the text (one
    list per translation unit; `.name:` one level deeper names a kernel ARGUMENT and does not match)."""
    assert "amdhsa.kernels:" in asm
    return re.findall(r"^    \.name:\s+(\S+)\n", asm, re.M)


def kernel_text(asm, symbol):
    m = re.search(r"^%s[^\n:]*:[^\n]*\n(.*?)\n\.Lfunc_end" % re.escape(symbol), asm, re.S | re.M)
    assert m, symbol
    return m.group(1)


def instructions(text):
    out = []
    for line in text.split("\n"):
        line = line.split(";")[0].strip()
        if line and not line.endswith(":") and not line.startswith("."):
            out.append(line)
    return out


def _loops(text):
    """(lines, [(first, last)]): the labels and instructions of a kernel, and per backward branch the indices of its target
    label and of the branch."""
    lines = []
    for raw in text.split("\n"):
        l = raw.split(";")[0].strip()
        if l and (l.endswith(":") or not l.startswith(".")):
            lines.append(l)
    label = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"s_(?:cbranch_\w+|branch)\s+(\.LBB\S+)", l)
        if m and m.group(1) in label and label[m.group(1)] < i:
            loops.append((label[m.group(1)], i))
    return lines, loops


def inner_loops(text):
    """[(instruction list)] of the innermost loops (backward branches that contain no other backward branch)."""
    lines, loops = _loops(text)
    inner = [lp for lp in loops if not any(o != lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
    return [[x for x in lines[a:b + 1] if not x.endswith(":")] for a, b in inner]


def all_loops(text):
    """[(instruction list)] of EVERY loop (one per backward branch, label to branch), nested or not."""
    lines, loops = _loops(text)
    return [[x for x in lines[a:b + 1] if not x.endswith(":")] for a, b in loops]


def f64_mix(ins):
    c = collections.Counter(i.split()[0] for i in ins)
    return {"fma": c["v_fma_f64"] + c["v_fmac_f64_e32"], "mul": c["v_mul_f64"], "add": c["v_add_f64"], "rcp": c["v_rcp_f64_e32"],
            "div": c["v_div_fmas_f64"], "lane": c["v_readlane_b32"] + c["v_writelane_b32"], "scratch": sum(v for k, v in c.items() if k.startswith("scratch_"))}


def meta(asm, symbol, key):
    """A field of the kernel's entry in the code object's metadata (amdhsa.kernels).  The entries are YAML maps whose keys are
    sorted, so some precede `.name` and some follow it: take the whole entry (it starts at `  - .agpr_count:`).  The text holds
    one amdhsa.kernels list per translation unit, each closed by its amdhsa.target line."""
    lists = re.findall(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.target:", asm, re.S | re.M)
    assert lists, "no kernel metadata in the text"
    for lst in lists:
        for blk in re.split(r"\n  - (?=\.agpr_count:)", "\n" + lst)[1:]:
            if re.search(r"\.name:\s+%s\S*\n" % re.escape(symbol), blk):
                m = re.search(r"^\s+\.%s:\s+(\d+)" % key, "\n    " + blk, re.M)
                assert m, (symbol, key)
                return int(m.group(1))
    raise AssertionError((symbol, "not in the metadata"))


def rk4_loops(text):
    """The RK4 substep loops of a kernel: innermost, unrolled by two - 8 reciprocals (a Butcher-5 step loop holds 6)."""
    return [l for l in inner_loops(text) if f64_mix(l)["rcp"] == 8 and f64_mix(l)["fma"] > 250]


def b5_steps(text, max_len=580):
    """The Butcher-5 step loops, picked as tests/test_isa_cpu.py::test_butcher5_step_loops picks them: six reciprocals, and no
    loop nested inside (a loop around a whole call holds dozens, and is longer than max_len)."""
    return [l for l in all_loops(text) if f64_mix(l)["rcp"] == 6 and len(l) < max_len]


def flop_counts(loops):
    """The distinct float64 operation counts of the loops, ascending (FMA = 2): what bench.py's FP64_FLOP_PER_* quote."""
    return sorted({m["fma"] * 2 + m["mul"] + m["add"] + m["rcp"] for m in map(f64_mix, loops)})


def vector_stores(asm, symbol):
    return [i for i in instructions(kernel_text(asm, symbol)) if i.split()[0].startswith(("global_store", "flat_store", "buffer_store"))]
