"""What collecting costs in the fused loop and what it saves a learner: one SBROS-v1 episode (463 calls) at 65536 envs, influent
scenarios 4..7, under the 2 x 32 tanh MLP policy of scripts/gpu_policy_rollout.py, every call a decision (hold = 1), timed with
device events in ONE process, the three legs interleaved:
  (a)  sbr_rollout_policy   the fused closed-loop kernel, H = 32: the returns only
  (a') sbr_collect_policy   the same loop with every output: obs_out, actions_out, rewards_out, flags_out, returns
  (b)  sbr_step + torch     the same net in torch float32 around env.step, per call, collecting the same tensors: the
                            observation the action was taken on, the action, the reward and the done flag of every call, copied
                            into buffers allocated before the clock starts
Writes profiles/r16_policy_collect.json (us per call and env-steps/s of each leg, the spread over its runs, a'/a, a'/b, the
extra bytes per env-decision, library_source_hash).  Usage: python scripts/gpu_policy_collect.py [runs] [out.json]"""
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
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r16_policy_collect.json")

rs = np.random.RandomState(NET_SEED)
sizes = [18, 32, 32, 2]
layers = [(rs.randn(o, i) / np.sqrt(i), rs.randn(o) * 0.1) for i, o in zip(sizes[:-1], sizes[1:])]
pol = MlpPolicy(layers, activation="tanh", squash="tanh", low=(0, 0), high=(2.5, 15))
env = SbrOSVec(N)
scen = (4 + torch.arange(N, device="cuda") % 4).to(torch.int32)
tw = [(torch.tensor(w, dtype=torch.float32, device="cuda").t().contiguous(), torch.tensor(b, dtype=torch.float32, device="cuda"))
      for w, b in layers]
scale = torch.from_numpy(pol.act_scale).cuda()
bias = torch.from_numpy(pol.act_bias).cuda()
# leg (b)'s collection, allocated outside the clock ((a') allocates its outputs inside it, through torch's caching allocator)
b_obs = torch.empty((CALLS, N, _capi.NOBS), dtype=torch.float32, device="cuda")
b_act = torch.empty((CALLS, N, 2), dtype=torch.float32, device="cuda")
b_rew = torch.empty((CALLS, N), dtype=env.reward.dtype, device="cuda")
b_done = torch.empty((CALLS, N), dtype=torch.uint8, device="cuda")


def episode(leg):
    """One episode from a fresh reset; returns (milliseconds between the device events around the calls, what the leg returns)."""
    env.reset(seed=SEED, scenario=scen)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = leg()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def leg_a():
    return env.rollout_policy(pol, CALLS)


def leg_a1():
    return env.collect_policy(pol, CALLS)


def leg_b():
    obs = env.obs
    for s in range(CALLS):
        b_obs[s].copy_(obs)
        h = torch.tanh(torch.addmm(tw[0][1], obs, tw[0][0]))
        h = torch.tanh(torch.addmm(tw[1][1], h, tw[1][0]))
        a = torch.addcmul(bias, scale, torch.tanh(torch.addmm(tw[2][1], h, tw[2][0])))
        b_act[s].copy_(a)
        obs, _, reward, done = env.step(a)
        b_rew[s].copy_(reward)
        b_done[s].copy_(done)
    return env.episode_returns()


legs = {"a": leg_a, "a1": leg_a1, "b": leg_b}
for f in legs.values():                                # warm-up: every kernel loaded, the allocator settled
    episode(f)
ms = {k: [] for k in legs}
outs = {}
for _ in range(RUNS):
    for k, f in legs.items():
        # the leg's last result goes back to torch's caching allocator first: (a') sizes 2.7 GB of outputs inside the clock, and
        # while the last ones are still held that is a fresh hipMalloc (one run of 71 ms against 10.4, before this line)
        outs.pop(k, None)
        t, outs[k] = episode(f)
        ms[k].append(t)
x, ctrl = env.get_state()
status = ctrl[_capi.C_STATUS].to(torch.int64)


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"us_per_call": med * 1e3 / CALLS, "env_steps_per_s": N * CALLS / (med * 1e-3), "runs_ms": [round(t, 4) for t in ts],
            "spread_rel": (ts[-1] - ts[0]) / med}


res = {k: summary(v) for k, v in ms.items()}
a, a1, b = (res[k]["us_per_call"] for k in ("a", "a1", "b"))
col = outs["a1"]
extra = _capi.NOBS * 4 + 1
out = {
    "what": "one SBROS-v1 episode, %d envs x %d calls, hold 1, scenarios 4..7, 2 x 32 tanh MLP policy; device events, %d interleaved "
            "runs per leg, medians" % (N, CALLS, RUNS),
    "device": torch.cuda.get_device_name(0),
    "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None),
    "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
    "library_source_hash": B.source_hash(),
    "a_sbr_rollout_policy_h32_returns_only": res["a"], "a1_sbr_collect_policy_h32_every_output": res["a1"],
    "b_torch_f32_net_around_sbr_step_collecting": res["b"],
    "a1_over_a_time": a1 / a, "a1_minus_a_us_per_call": a1 - a, "a1_minus_a_over_spread_of_a": (a1 - a) / (res["a"]["spread_rel"] * a),
    "a1_over_b_time": a1 / b, "a1_faster_than_b_rel": 1.0 - a1 / b, "spread_rel_a1_plus_b": res["a1"]["spread_rel"] + res["b"]["spread_rel"],
    "acceptance_a1_faster_than_b_by_more_than_the_spread": bool(1.0 - a1 / b > res["a1"]["spread_rel"] + res["b"]["spread_rel"]),
    "extra_bytes_per_env_decision_obs_out_and_flags_out": extra, "extra_mb_per_decision": extra * N / 1e6,
    "a1_output_bytes_per_env_call_in_all": extra + 8 + 8,
    "returns_a1_equal_a_bitwise": bool(torch.equal(col.returns, outs["a"])),
    "flags_all_taken_last_ended": bool((col.flags[:-1] == 1).all()) and bool((col.flags[-1] == 3).all()),
    "obs_a1_minus_b_max_abs": float((col.obs - b_obs).abs().max()),
    "returns_b_minus_a_max_abs": float((outs["b"] - outs["a"]).abs().max()),
    "envs_flagged": int(((status & 7) != 0).sum()),
}
print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
env.close()
