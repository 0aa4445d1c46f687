"""Two assemblies of the library (hipcc -S --cuda-device-only under gym_sbr2_amd/build.py's flags), kernel by kernel: what a
refactor of the device code has to show.  usage: python scripts/isa_compare.py before.s after.s [-o table.txt]

  * the kernels NAMED by --changed (prefixes of the demangled name; default: the seven fused kernels behind k_rollout): registers,
    spills, scratch and LDS from the code object's metadata, the float64 mix of the Butcher-5 and RK4 step loops as tests/isa.py
    picks them, the vector stores and the instruction count - one row per build, before -> after where they differ;
  * every OTHER kernel: the instruction text (instructions and local labels, the function number taken out of the labels) must
    be identical;
  * the kernels named by --added (none by default) are expected in `after` only and are listed with the same figures.
Exit status 1 if an unnamed kernel moved, if a named build grew in any figure but the instruction count's decrease, or if the
two kernel lists differ by anything but the added kernels."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import isa  # noqa: E402  (tests/isa.py: the parsers the ISA tests use)

FUSED = ("k_rollout_tape", "k_lookahead_tape", "k_lookahead_tape_end", "k_lookahead_sampled", "k_lookahead_sampled_end",
         "k_rollout_policy", "k_lookahead_policy")
META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def kernels(asm):
    return isa.kernel_names(asm)      # over every translation unit's metadata where the text is several units' one behind the other


def base_name(symbol):
    m = re.match(r"_Z(\d+)", symbol)
    return symbol[len(m.group(0)):len(m.group(0)) + int(m.group(1))] if m else symbol


def text_key(text):
    """Instructions and local labels of a kernel with what only counts through the translation unit taken out of the label
    names: the function number of .LBB<f>_<n>, and the unit-wide counter of the long-branch labels .Lpost_getpc<c>, which are
    numbered again in the order the kernel first names them."""
    out, getpc = [], {}
    for raw in text.split("\n"):
        l = raw.split(";")[0].strip()
        if l and (l.endswith(":") or not l.startswith(".")):
            l = re.sub(r"\.LBB\d+_", ".LBB_", l)
            out.append(re.sub(r"\.Lpost_getpc(\d+)", lambda m: ".Lpost_getpc#%d" % getpc.setdefault(m.group(1), len(getpc)), l))
    return out


def figures(asm, sym):
    text = isa.kernel_text(asm, sym)
    f = {k: isa.meta(asm, sym, k) for k in META}
    f["b5_mix"] = sorted(tuple(sorted(isa.f64_mix(l).items())) for l in isa.b5_steps(text))
    f["rk4_mix"] = sorted(tuple(sorted(isa.f64_mix(l).items())) for l in isa.rk4_loops(text))
    f["stores"] = len(isa.vector_stores(asm, sym))
    f["instructions"] = len(isa.instructions(text))
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before"); ap.add_argument("after")
    ap.add_argument("--changed", nargs="*", default=list(FUSED))
    ap.add_argument("--added", nargs="*", default=[], help="kernels expected in `after` only: listed with their figures")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    with open(a.before) as f:
        before = f.read()
    with open(a.after) as f:
        after = f.read()
    kb, ka = kernels(before), kernels(after)
    lines, bad = [], 0
    added = sorted(s for s in set(ka) - set(kb) if base_name(s) in a.added)
    if sorted(kb) != sorted(set(ka) - set(added)):
        bad += 1
        lines.append("kernel lists differ: only before %s, only after %s" % (sorted(set(kb) - set(ka)), sorted(set(ka) - set(kb) - set(added))))
    named = [s for s in kb if base_name(s) in a.changed and s in ka]
    others = [s for s in kb if base_name(s) not in a.changed and s in ka]
    moved = [s for s in others if text_key(isa.kernel_text(before, s)) != text_key(isa.kernel_text(after, s))]
    bad += len(moved)
    lines.append("%d kernels outside %s: instruction text identical in %d%s" % (
        len(others), ", ".join(a.changed), len(others) - len(moved), "".join("\n  MOVED " + s for s in moved)))
    lines.append("")
    lines.append("%d builds of the named kernels; a figure is `before` or `before->after`" % len(named))
    head = ("kernel", "vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds", "b5 loops", "rk4 loops", "f64 mix", "stores", "instr")
    rows = [head]
    for s in sorted(named):
        fb, fa = figures(before, s), figures(after, s)

        def cell(k):
            return str(fb[k]) if fb[k] == fa[k] else "%s->%s" % (fb[k], fa[k])
        same_mix = fb["b5_mix"] == fa["b5_mix"] and fb["rk4_mix"] == fa["rk4_mix"]
        ok = all(fb[k] == fa[k] for k in META) and same_mix and fb["stores"] == fa["stores"] and fa["instructions"] <= fb["instructions"]
        bad += 0 if ok else 1
        nb5 = "%d" % len(fb["b5_mix"]) if len(fb["b5_mix"]) == len(fa["b5_mix"]) else "%d->%d" % (len(fb["b5_mix"]), len(fa["b5_mix"]))
        nrk = "%d" % len(fb["rk4_mix"]) if len(fb["rk4_mix"]) == len(fa["rk4_mix"]) else "%d->%d" % (len(fb["rk4_mix"]), len(fa["rk4_mix"]))
        rows.append((s,) + tuple(cell(k) for k in META) + (nb5, nrk, "same" if same_mix else "DIFFERS", cell("stores"),
                                                          cell("instructions") + ("" if ok else "  <-- FAILS")))
    width = [max(len(r[i]) for r in rows) for i in range(len(head))]
    lines += ["  ".join(c.ljust(w) for c, w in zip(r, width)).rstrip() for r in rows]
    lines.append("")
    if added:
        lines.append("%d builds of the added kernels (%s), in `after` only" % (len(added), ", ".join(a.added)))
        rows = [head]
        for s in added:
            f = figures(after, s)
            mixes = sorted(set(f["b5_mix"] + f["rk4_mix"]))
            rows.append((s,) + tuple(str(f[k]) for k in META) + (str(len(f["b5_mix"])), str(len(f["rk4_mix"])),
                                                                 "%d distinct" % len(mixes), str(f["stores"]), str(f["instructions"])))
        width = [max(len(r[i]) for r in rows) for i in range(len(head))]
        lines += ["  ".join(c.ljust(w) for c, w in zip(r, width)).rstrip() for r in rows]
        lines.append("")
    lines.append("%d failures" % bad)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
