"""What the read-only lookahead costs against the paths it replaces: 1024 live envs (influent scenarios 4..7, advanced 60 calls
through step), 64 candidate tapes per env = 65536 branches, a horizon of 50 calls, hold = 1, float32 tape (u_DO ~ U[0, 2.5],
u_EC ~ U[0, 15]); timed with device events in ONE process, the three legs interleaved:
  (a) lookahead with return_best                       k_lookahead_tape + k_branch_best on the live handle
  (b) rollout_actions on a 65536-env handle that holds the same state 64 times: the existing kernel on the same arithmetic
      (the state is put back before every run, outside the timed region)
  (c) today's whole path per decision: get_state on A, repeat_interleave, set_state on B, rollout_actions, torch max over K
Writes profiles/r09_lookahead.json (us per call and branch-steps/s of each leg, each leg's run-to-run spread, a/b, a/c,
library_source_hash).  Usage: python scripts/gpu_lookahead.py [runs] [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gym_sbr2_amd import SbrOSVec  # noqa: E402
from gym_sbr2_amd import build as B  # noqa: E402

N, K, CALLS, ADVANCE, SEED = 1024, 64, 50, 60, 1000
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r09_lookahead.json")

g = torch.Generator(device="cuda").manual_seed(SEED)
scale = torch.tensor([2.5, 15.0], device="cuda")
a_env = SbrOSVec(N)
a_env.reset(seed=SEED, scenario=(4 + torch.arange(N, device="cuda") % 4).to(torch.int32))
for _ in range(ADVANCE):
    a_env.step(torch.rand((N, 2), generator=g, device="cuda") * scale)
tape = torch.rand((CALLS, N, K, 2), generator=g, device="cuda") * scale
flat = tape.reshape(CALLS, N * K, 2)
b_env = SbrOSVec(N * K)
b_env.reset(influent=a_env.influent().T.repeat_interleave(K, dim=0))


def replicate():
    """A's state K times into B: the translation kernel each way and the K copies that leg (c) pays on every decision."""
    x, c = a_env.get_state()
    b_env.set_state(x.repeat_interleave(K, dim=1), c.repeat_interleave(K, dim=1))


def leg_a():
    _, bi, br = a_env.lookahead(tape, return_best=True)
    return bi, br


def leg_b():
    return b_env.rollout_actions(flat)


def leg_c():
    replicate()
    br, bi = b_env.rollout_actions(flat).reshape(N, K).max(dim=1)
    return bi, br


def timed(leg, prepare):
    if prepare:
        prepare()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = leg()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


legs = {"a": (leg_a, None), "b": (leg_b, replicate), "c": (leg_c, None)}
for f, prep in legs.values():                          # warm-up: every kernel loaded, the allocator settled
    timed(f, prep)
ms = {k: [] for k in legs}
outs = {}
for _ in range(RUNS):
    for k, (f, prep) in legs.items():
        t, outs[k] = timed(f, prep)
        ms[k].append(t)


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"us_per_call": med * 1e3 / CALLS, "branch_steps_per_s": N * K * CALLS / (med * 1e-3), "runs_ms": [round(t, 4) for t in ts],
            "spread_rel": (ts[-1] - ts[0]) / med}


res = {k: summary(v) for k, v in ms.items()}
a, b, c = (res[k]["us_per_call"] for k in "abc")
ret_a = a_env.lookahead(tape)
replicate()
ret_b = b_env.rollout_actions(flat).reshape(N, K)
out = {
    "what": "%d live envs (scenarios 4..7, %d calls in), %d tapes per env = %d branches, horizon %d calls, hold 1, float32 tape; "
            "device events, %d interleaved runs per leg, medians" % (N, ADVANCE, K, N * K, CALLS, RUNS),
    "device": torch.cuda.get_device_name(0),
    "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None),
    "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
    "library_source_hash": B.source_hash(),
    "a_lookahead_with_best": res["a"], "b_rollout_actions_on_replicated_state": res["b"], "c_replicate_rollout_actions_max": res["c"],
    "a_over_b_time": a / b, "a_over_c_time": a / c,
    "a_slower_than_b_rel": a / b - 1.0, "b_spread_rel": res["b"]["spread_rel"],
    "a_within_b_spread": bool(a / b - 1.0 <= res["b"]["spread_rel"]),
    "returns_a_equal_b_bitwise": bool(torch.equal(ret_a, ret_b)),
    "best_a_equal_c": bool(torch.equal(outs["a"][1], outs["c"][1])),
}
print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
a_env.close()
b_env.close()
