"""Where the ORDINARY call's instructions lie in k_step's text (profiles/r22_notes.md, tests/test_step_layout_cpu.py): the path
that scripts/analysis/step_path.py walks, with the byte offset of every instruction on it, counted in the 64-byte lines the
instruction cache holds.

Instruction sizes are not guessed from the mnemonics: the kernel's text goes through the assembler of the toolchain that compiled
it (llvm-mc -show-encoding), and the offsets follow from the encodings and the text's own .p2align directives.  The kernel's
entry is 256-byte aligned, so an offset's line is offset // 64.

The argument-preload header (the loads at the entry and the s_branch over the padding up to +256) is not on the path: a wave whose
leading arguments arrive in SGPRs enters at +256.  The path therefore starts at the header's branch target.

Reported per kernel:
  first, last      byte offsets of the path's first instruction and of the end of its last one; span = last - first
  lines            64-byte lines the path touches (the one step loop it runs included)
  holes            lines inside the span that the path does not touch, split into
    holes_loops      ... lines that hold (part of) a Butcher-5 step loop the path does not run (the other regime's loop), and
    holes_other      ... the rest: cold code - or padding - lying between hot code
  taken_forward    taken branches on the path whose target lies ahead (each one a jump over text the call does not run)
  taken_backward   taken branches to a lower address (the walk runs each loop once, so these are hot blocks laid out behind
                   their successors)
Usage: python scripts/analysis/step_layout.py sbr_core.s [-v] [kernel symbol ...]"""
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_path  # noqa: E402

LINE = 64


def llvm_mc():
    """The assembler next to the compiler that builds the library."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    roots = [os.environ.get("ROCM_PATH"), os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "/opt/rocm"]
    cands = [shutil.which("llvm-mc")] + [os.path.join(r, sub, "llvm-mc") for r in roots if r for sub in ("lib/llvm/bin", "llvm/bin", "bin")]
    for c in cands:
        if c and os.path.exists(c):
            return c
    raise RuntimeError("llvm-mc not found next to hipcc: instruction sizes cannot be determined")


def offsets(text, cpu="gfx950"):
    """[(offset, size)] of the kernel's instructions in text order - the order in which step_path.blocks_of() lists them."""
    keep, data = [], False
    for raw in text.split("\n"):
        l = raw.split(";")[0].strip()
        if l.startswith(".section"):
            data = ".text" not in l          # the kernel descriptor sits in .rodata in the middle of the listing
            continue
        if not l or data:
            continue
        if l.endswith(":") or not l.startswith(".") or l.startswith(".p2align"):
            keep.append(l)
    p = subprocess.run([llvm_mc(), "-triple=amdgcn-amd-amdhsa", "-mcpu=" + cpu, "-show-encoding"], input="\n".join(keep) + "\n",
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        raise RuntimeError("llvm-mc failed:\n" + p.stderr[-2000:])
    out, off = [], 0
    for l in p.stdout.split("\n"):
        m = re.search(r";\s*encoding:\s*\[(.*)\]", l)
        if m:
            size = m.group(1).count(",") + 1
            out.append((off, size))
            off += size
            continue
        m = re.match(r"\s*\.p2align\s+(\d+)", l)
        if m:
            a = 1 << int(m.group(1))
            off = (off + a - 1) // a * a
    return out


def layout(text):
    blocks, path, decisions = step_path.walk(text)
    offs = offsets(text)
    assert len(offs) == sum(len(ins) for _, ins in blocks), (len(offs), sum(len(ins) for _, ins in blocks))
    first_ins, n = [], 0                                   # index of each block's first instruction
    for _, ins in blocks:
        first_ins.append(n)
        n += len(ins)

    def extent(i):                                         # [begin, end) of block i in bytes; None for an empty block
        k = len(blocks[i][1])
        if k == 0:
            return None
        return offs[first_ins[i]][0], offs[first_ins[i] + k - 1][0] + offs[first_ins[i] + k - 1][1]

    seq = [i for i, _ in path]
    # the preload header: an entry block that only loads and branches over the padding
    if blocks[seq[0]][1] and blocks[seq[0]][1][-1].startswith("s_branch") and all(
            x.startswith(("s_load", "s_waitcnt", "s_branch")) for x in blocks[seq[0]][1]):
        seq = seq[1:]
    ins_offsets = [offs[first_ins[i] + j] for i in seq for j in range(len(blocks[i][1]))]
    first = min(o for o, _ in ins_offsets)
    last = max(o + s for o, s in ins_offsets)
    touched = set()
    for o, s in ins_offsets:
        touched.update(range(o // LINE, (o + s - 1) // LINE + 1))
    on_path = set(seq)
    loop_lines = set()
    for i, (_, ins) in enumerate(blocks):
        if i not in on_path and step_path.is_step_loop_block(ins):
            b, e = extent(i)
            loop_lines.update(range(b // LINE, (e - 1) // LINE + 1))
    span_lines = range(first // LINE, (last - 1) // LINE + 1)
    holes = [ln for ln in span_lines if ln not in touched]
    fwd = bwd = 0
    jumps = []
    for a, b in zip(seq, seq[1:]):
        if b != a + 1:
            ea, eb = extent(a), extent(b)
            while eb is None:                              # an empty block: the next one's address
                b += 1
                eb = extent(b)
            if eb[0] >= ea[1]:
                fwd += 1
            else:
                bwd += 1
            jumps.append((blocks[a][0], ea[1], eb[0]))
    return {"first": first, "last": last, "span": last - first, "path_bytes": sum(s for _, s in ins_offsets),
            "kernel_bytes": offs[-1][0] + offs[-1][1], "lines": len(touched), "span_lines": len(span_lines), "holes": len(holes),
            "holes_loops": sum(1 for h in holes if h in loop_lines), "holes_other": sum(1 for h in holes if h not in loop_lines),
            "taken_forward": fwd, "taken_backward": bwd, "instructions": len(ins_offsets),
            "_offsets": ins_offsets, "_jumps": jumps, "_holes": holes}


if __name__ == "__main__":
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"),
                    os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")]
    import isa
    args = [a for a in sys.argv[1:] if a != "-v"]
    asm = open(args[0]).read()
    for k in args[1:] or ["K_STEP", "K_STEP_SMALL"]:
        r = layout(isa.kernel_text(asm, getattr(isa, k, k)))
        print(k, {a: b for a, b in r.items() if not a.startswith("_")})
        if "-v" in sys.argv:
            for name, src, dst in r["_jumps"]:
                print("    taken branch at the end of %-12s 0x%05x -> 0x%05x (%+d bytes)" % (name, src, dst, dst - src))
            runs, hs = [], r["_holes"]                      # the holes as runs of lines
            for h in hs:
                if runs and runs[-1][1] == h - 1:
                    runs[-1][1] = h
                else:
                    runs.append([h, h])
            for a, b in runs:
                print("    untouched lines 0x%05x-0x%05x (%d)" % (a * LINE, (b + 1) * LINE, b - a + 1))
            if "-vv" in sys.argv:
                for o, s in r["_offsets"]:
                    print("    0x%05x %d" % (o, s))
