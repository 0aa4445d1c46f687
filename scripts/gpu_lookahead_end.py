"""What the end outputs of the lookahead cost, and what they cost today without them: 1024 live envs (influent scenarios 4..7,
advanced 60 calls through step), 64 sampled candidates per env = 65536 branches, a horizon of 50 calls, hold = 1, float32;
timed with device events in ONE process, the three legs interleaved:
  (a) lookahead_sampled with return_best                         k_lookahead_sampled + k_branch_best on the live handle
  (b) lookahead_sampled_end with return_best: the same and obs_end, state_end, done_end of every branch
  (c) the only path to those outputs without (b): the state replicated into a 65536-env handle (get_state, repeat_interleave,
      set_state - inside the timed region), rollout_actions over the first 49 calls of the candidates, one step() for the 50th
Acceptance: (b) is no slower than (c) by more than (c)'s own run-to-run spread.  b/a is reported, not gated.  The script
exits 1 if the acceptance does not hold, or if (b)'s returns and winners are not (a)'s bits or its end rows not (c)'s.
Writes profiles/r11_lookahead_end.json (us per call of each leg, each leg's run-to-run spread, b/a, b/c, library_source_hash).
Usage: python scripts/gpu_lookahead_end.py [runs] [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gym_sbr2_amd import SbrOSVec  # noqa: E402
from gym_sbr2_amd import build as B  # noqa: E402
from gym_sbr2_amd.planner import TapeSampler  # noqa: E402

N, K, CALLS, ADVANCE, SEED = 1024, 64, 50, 60, 1000
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r11_lookahead_end.json")

g = torch.Generator(device="cuda").manual_seed(SEED)
scale = torch.tensor([2.5, 15.0], device="cuda")
a_env = SbrOSVec(N)
a_env.reset(seed=SEED, scenario=(4 + torch.arange(N, device="cuda") % 4).to(torch.int32))
for _ in range(ADVANCE):
    a_env.step(torch.rand((N, 2), generator=g, device="cuda") * scale)
nominal = torch.rand((CALLS, N, 2), generator=g, device="cuda") * scale
sampler = TapeSampler((0.3, 2.0), seed=SEED)
# the candidates (a) and (b) draw in their lanes, as a tape for (c): drawn once, outside every timed region
flat = a_env.lookahead_sampled(nominal, K, sampler, return_actions=True)[1].reshape(CALLS, N * K, 2)
b_env = SbrOSVec(N * K)
b_env.reset(influent=a_env.influent().T.repeat_interleave(K, dim=0))


def leg_a():
    return a_env.lookahead_sampled(nominal, K, sampler, return_best=True)


def leg_b():
    return a_env.lookahead_sampled_end(nominal, K, sampler, return_best=True)


def leg_c():
    x, c = a_env.get_state()
    b_env.set_state(x.repeat_interleave(K, dim=1), c.repeat_interleave(K, dim=1))
    b_env.rollout_actions(flat, n_steps=CALLS - 1)
    obs, state, _, done = b_env.step(flat[CALLS - 1])
    return obs, state, done


def timed(leg):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = leg()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


legs = {"a": leg_a, "b": leg_b, "c": leg_c}
for f in legs.values():                                # warm-up: every kernel loaded, the allocator settled
    timed(f)
ms = {k: [] for k in legs}
outs = {}
for _ in range(RUNS):
    for k, f in legs.items():
        t, outs[k] = timed(f)
        ms[k].append(t)


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"us_per_call": med * 1e3 / CALLS, "ms_per_launch": med, "runs_ms": [round(t, 4) for t in ts], "spread_rel": (ts[-1] - ts[0]) / med}


res = {k: summary(v) for k, v in ms.items()}
a, b, c = (res[k]["ms_per_launch"] for k in "abc")
(ret_a, bi_a, br_a), (ret_b, bi_b, br_b, obs_b, state_b, done_b) = outs["a"], outs["b"]
obs_c, state_c, done_c = (t.reshape(N, K, -1) for t in outs["c"])
live = ~done_b
out = {
    "what": "%d live envs (scenarios 4..7, %d calls in), %d sampled candidates per env = %d branches, horizon %d calls, hold 1, "
            "float32; device events, %d interleaved runs per leg, medians" % (N, ADVANCE, K, N * K, CALLS, RUNS),
    "device": torch.cuda.get_device_name(0),
    "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None),
    "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
    "library_source_hash": B.source_hash(),
    "a_lookahead_sampled_with_best": res["a"], "b_lookahead_sampled_end_with_best": res["b"],
    "c_replicate_rollout_actions_49_step_1": res["c"],
    "b_over_a_time": b / a, "b_over_c_time": b / c,
    "b_slower_than_c_rel": b / c - 1.0, "c_spread_rel": res["c"]["spread_rel"],
    "b_within_c_spread": bool(b / c - 1.0 <= res["c"]["spread_rel"]),
    "end_bytes_per_branch": 18 * 4 + 15 * 4 + 1,
    "returns_and_best_b_equal_a_bitwise": bool(torch.equal(ret_a, ret_b) and torch.equal(bi_a, bi_b) and torch.equal(br_a, br_b)),
    "branches_done": int(done_b.sum()),
    "ends_b_equal_c_bitwise": bool(torch.equal(done_b, done_c[..., 0].bool()) and torch.equal(obs_b[live], obs_c[live])
                                   and torch.equal(state_b[live], state_c[live])),
}
print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
a_env.close()
b_env.close()
failed = [k for k in ("b_within_c_spread", "returns_and_best_b_equal_a_bitwise", "ends_b_equal_c_bitwise") if not out[k]]
if failed:
    sys.exit("FAILED: " + ", ".join(failed))
