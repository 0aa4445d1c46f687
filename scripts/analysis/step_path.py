"""The instruction path of an ORDINARY call through k_step's assembly (single interval, not done, no trace, no m1 rows, wave full),
for profiles/r12_notes.md and tests/test_step_spill_cpu.py: walks the kernel text from its entry, takes at every conditional
branch the side an ordinary call takes, runs each step loop once and counts what lies on the way outside the step loops.

A conditional branch is decided by what its target or its fall-through holds - the rules are about the code, not about label
numbers, so they survive a recompile:
  * a side that leads (before the next join) into code only rare calls run is not taken: a second control interval or the idle
    phase (another step loop behind the first one run), the terminal phases (v_exp / v_rndne / v_div_fmas_f64), the IEEE division
    fallback of the row count, stores of the trace record (more than 20 global stores in a row of blocks), s_sleep;
  * `s_cbranch_execz` over a body is otherwise not taken, every other conditional branch is taken when its fall-through is rare
    and not taken when its target is.
Usage: python scripts/analysis/step_path.py sbr_amd.s [kernel symbol]"""
import collections
import re
import sys

RARE = re.compile(r"^(v_exp_|v_rndne_)")


def blocks_of(text):
    """[(label or None, [instructions])] split at labels and behind branches; label -> block index."""
    blocks, cur, name = [], [], "entry"
    for raw in text.split("\n"):
        l = raw.split(";")[0].strip()
        if not l or (l.startswith(".") and not l.endswith(":")):
            continue
        if l.endswith(":"):
            if cur or name is not None:               # (an empty block for a label that is followed by another label)
                blocks.append((name, cur))
            name, cur = l[:-1], []
            continue
        cur.append(l)
        if l.startswith(("s_cbranch", "s_branch", "s_endpgm")):
            blocks.append((name, cur))
            name, cur = None, []
    if cur:
        blocks.append((name, cur))
    index = {n: i for i, (n, _) in enumerate(blocks) if n}
    return blocks, index


def is_step_loop_block(ins):
    c = collections.Counter(i.split()[0] for i in ins)
    return c["v_rcp_f64_e32"] >= 5 and len(ins) > 300


def rare_ahead(blocks, index, start, seen_loop, depth=3):
    """Does straight-line code from block `start` (following fall-throughs and unconditional branches, not entering conditional
    targets) hold a rare marker or a further step loop within `depth` blocks?"""
    i, n = start, 0
    while i < len(blocks) and n < depth:
        ins = blocks[i][1]
        if any(RARE.match(x) for x in ins):
            return True
        if seen_loop and is_step_loop_block(ins):
            return True
        last = ins[-1] if ins else ""
        if last.startswith("s_endpgm"):
            return False
        m = re.match(r"s_branch\s+(\S+)", last)
        i = index[m.group(1)] if m else i + 1
        n += 1 if last.startswith("s_cbranch") else 0          # looks past `depth` conditional branches (their fall-throughs)
    return False


def walk(text):
    blocks, index = blocks_of(text)
    path, decisions, i, seen_loop, visited = [], [], 0, False, collections.Counter()
    while i < len(blocks):
        name, ins = blocks[i]
        visited[i] += 1
        if visited[i] > 2:
            raise RuntimeError("path does not terminate at %s\n%s" % (name, "\n".join(map(str, decisions))))
        loop = is_step_loop_block(ins)
        path.append((i, loop))
        last = ins[-1] if ins else ""
        if last.startswith("s_endpgm"):
            break
        m = re.match(r"s_branch\s+(\S+)", last)
        if m:
            i = index[m.group(1)]
            continue
        m = re.match(r"s_cbranch_(\w+)\s+(\S+)", last)
        if not m:
            i += 1
            continue
        kind, tgt = m.group(1), index[m.group(2)]
        if tgt <= i:                                  # a back edge: the loop body ran once
            seen_loop = seen_loop or any(l for _, l in path[-3:])
            decisions.append((name, last, "exit loop"))
            i += 1
            continue
        if loop or any(l for _, l in path[-2:]):
            seen_loop = True
        if blocks[i + 1][1] == ["s_sleep 25"]:        # the staggered entry: every other workgroup; the path without it
            decisions.append((name, last, "taken")); i = tgt; continue
        rare_t, rare_f = rare_ahead(blocks, index, tgt, seen_loop), rare_ahead(blocks, index, i + 1, seen_loop)
        if rare_f and not rare_t:
            take = True
        elif rare_t and not rare_f:
            take = False
        else:
            take = False if kind == "execz" else (kind in ("vccnz", "scc1") and False)
        decisions.append((name, last, "taken" if take else "not taken"))
        i = tgt if take else i + 1
    return blocks, path, decisions


def counts(blocks, path):
    out = [x for i, loop in path if not loop for x in blocks[i][1]]
    c = collections.Counter(x.split()[0] for x in out)
    return {"instructions": len(out), "lane": c["v_readlane_b32"] + c["v_writelane_b32"],
            "accvgpr": sum(v for k, v in c.items() if k.startswith("v_accvgpr")), "s_nop": c["s_nop"],
            "s_load": sum(v for k, v in c.items() if k.startswith("s_load")),
            "lgkm_wait": sum(1 for x in out if x.startswith("s_waitcnt") and "lgkmcnt" in x),
            "step_loops_run": sum(1 for _, loop in path if loop)}


if __name__ == "__main__":
    sys.path[:0] = ["tests", "."]
    import isa
    asm = open(sys.argv[1]).read()
    for k in sys.argv[2:] or ["K_STEP", "K_STEP_SMALL"]:
        blocks, path, decisions = walk(isa.kernel_text(asm, getattr(isa, k)))
        print(k, counts(blocks, path))
        if "-v" in sys.argv or True:
            for d in decisions:
                print("   ", d)
