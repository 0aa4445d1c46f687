"""What the in-kernel policy costs and what it saves: one SBROS-v1 episode (463 calls) at 65536 envs, influent scenarios 4..7,
under a 2 x 32 tanh MLP policy (seeded, set-points in [0, 2.5] x [0, 15]), timed with device events in ONE process, the four
legs interleaved:
  (a) sbr_rollout_policy    the fused closed-loop kernel, H = 32, hold = 1
  (b) sbr_step + torch      the same net in torch float32 (three addmm, three tanh, one addcmul) around env.step, per call
  (c) sbr_rollout_actions   the fused tape kernel replaying (a)'s reported actions
  (d) sbr_rollout_policy    (a) with the same net zero-padded to H = 64
Writes profiles/r08_policy_rollout.json (env-steps/s and us per call of each leg, the spread over its runs, a/b, (a - c) per
decision next to the FMA-count estimate, library_source_hash).  Usage: python scripts/gpu_policy_rollout.py [runs] [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_sbr2_amd import MlpPolicy, SbrOSVec, _capi  # noqa: E402
from gym_sbr2_amd import build as B  # noqa: E402

N, CALLS, SEED, NET_SEED = 65536, 463, 1000, 13
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r08_policy_rollout.json")

rs = np.random.RandomState(NET_SEED)
sizes = [18, 32, 32, 2]
layers = [(rs.randn(o, i) / np.sqrt(i), rs.randn(o) * 0.1) for i, o in zip(sizes[:-1], sizes[1:])]
pol32 = MlpPolicy(layers, activation="tanh", squash="tanh", low=(0, 0), high=(2.5, 15))
pol64 = pol32.widened(64)
env = SbrOSVec(N)
scen = (4 + torch.arange(N, device="cuda") % 4).to(torch.int32)
tw = [(torch.tensor(w, dtype=torch.float32, device="cuda").t().contiguous(), torch.tensor(b, dtype=torch.float32, device="cuda"))
      for w, b in layers]
scale = torch.from_numpy(pol32.act_scale).cuda()
bias = torch.from_numpy(pol32.act_bias).cuda()


def episode(leg):
    """One episode from a fresh reset; returns (milliseconds between the device events around the calls, returns [N])."""
    env.reset(seed=SEED, scenario=scen)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    ret = leg()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), ret


def leg_a():
    return env.rollout_policy(pol32, CALLS)


def leg_b():
    obs = env.obs
    for _ in range(CALLS):
        h = torch.tanh(torch.addmm(tw[0][1], obs, tw[0][0]))
        h = torch.tanh(torch.addmm(tw[1][1], h, tw[1][0]))
        a = torch.addcmul(bias, scale, torch.tanh(torch.addmm(tw[2][1], h, tw[2][0])))
        obs = env.step(a)[0]
    return env.episode_returns()


env.reset(seed=SEED, scenario=scen)
_, tape = env.rollout_policy(pol32, CALLS, return_actions=True)              # (a)'s decisions, as the tape of (c)


def leg_c():
    return env.rollout_actions(tape)


def leg_d():
    return env.rollout_policy(pol64, CALLS)


legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
for f in legs.values():                                # warm-up: every kernel loaded, the allocator settled
    episode(f)
ms = {k: [] for k in legs}
rets = {}
for _ in range(RUNS):
    for k, f in legs.items():
        t, rets[k] = episode(f)
        ms[k].append(t)
x, ctrl = env.get_state()
status = ctrl[_capi.C_STATUS].to(torch.int64)


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"us_per_call": med * 1e3 / CALLS, "env_steps_per_s": N * CALLS / (med * 1e-3), "runs_ms": [round(t, 4) for t in ts],
            "spread_rel": (ts[-1] - ts[0]) / med}


res = {k: summary(v) for k, v in ms.items()}
a, b, c, d = (res[k]["us_per_call"] for k in "abcd")
fma = {h: 18 * h + h * h + 2 * h for h in (32, 64)}
out = {
    "what": "one SBROS-v1 episode, %d envs x %d calls, scenarios 4..7, 2 x 32 tanh MLP policy; device events, %d interleaved runs per "
            "leg, medians" % (N, CALLS, RUNS),
    "device": torch.cuda.get_device_name(0),
    "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None),
    "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
    "library_source_hash": B.source_hash(),
    "a_sbr_rollout_policy_h32_hold1": res["a"], "b_torch_f32_net_around_sbr_step": res["b"], "c_sbr_rollout_actions_on_a_tape": res["c"],
    "d_sbr_rollout_policy_h64_hold1": res["d"],
    "a_over_b_time": a / b, "a_over_b_throughput": b / a,
    "a_faster_than_b_rel": 1.0 - a / b, "spread_rel_a_plus_b": res["a"]["spread_rel"] + res["b"]["spread_rel"],
    "acceptance_a_faster_than_b_by_more_than_the_spread": bool(1.0 - a / b > res["a"]["spread_rel"] + res["b"]["spread_rel"]),
    "net_us_per_decision_h32_a_minus_c": a - c, "net_us_per_decision_h64_d_minus_c": d - c,
    "estimate_us_per_decision_from_fma_count": {"h32": fma[32] * 4 / 2.4e3, "h64": fma[64] * 4 / 2.4e3,
                                                "assumes": "one fp32 FMA per 4 cycles per wave at 2.4 GHz, nothing else"},
    "returns_c_equal_a_bitwise": bool(torch.equal(rets["a"], rets["c"])),
    "returns_d_equal_a_bitwise": bool(torch.equal(rets["a"], rets["d"])),
    "returns_b_minus_a_max_abs": float((rets["b"] - rets["a"]).abs().max()),
    "envs_flagged": int(((status & 7) != 0).sum()),
}
print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
env.close()
