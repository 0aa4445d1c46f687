"""What the closed-loop lookahead costs next to the paths it replaces: 1024 live envs (influent scenarios 4..7, advanced 60 calls
through step), 64 branches per env = 65536 branches, a horizon of 50 calls, a 2 x 32 tanh net, exploration noise on, float32,
hold = 1 and hold = 8; timed with device events in ONE process, the three legs interleaved:
  (a) lookahead_policy with return_best                 k_lookahead_policy + k_branch_best on the live handle
  (b) rollout_policy on a 65536-env handle that holds the same state and observation 64 times (restored OUTSIDE the timed
      region): the same arithmetic per lane, plus the plant and record stores
  (c) today's whole path per decision, all of it timed: get_state, repeat_interleave, set_state, the observation replicated,
      rollout_policy on the 65536-env handle, torch max over each env's 64 returns
Acceptance, for each hold: (a) is no slower than (b) by more than (b)'s own run-to-run spread.  a/c is reported, not gated.
The script exits 1 if the acceptance does not hold, or if without noise (a)'s returns are not (b)'s bits.
Writes profiles/r13_lookahead_policy.json (us per call of each leg, each leg's run-to-run spread, a/b, a/c, library_source_hash).
Usage: python scripts/gpu_lookahead_policy.py [runs] [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gym_sbr2_amd import MlpPolicy, SbrOSVec  # noqa: E402
from gym_sbr2_amd import build as B  # noqa: E402

N, K, CALLS, ADVANCE, SEED, STD = 1024, 64, 50, 60, 1000, (0.3, 2.0)
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r13_lookahead_policy.json")

g = torch.Generator(device="cuda").manual_seed(SEED)
scale = torch.tensor([2.5, 15.0], device="cuda")
a_env = SbrOSVec(N)
a_env.reset(seed=SEED, scenario=(4 + torch.arange(N, device="cuda") % 4).to(torch.int32))
for _ in range(ADVANCE):
    a_env.step(torch.rand((N, 2), generator=g, device="cuda") * scale)
rs = np.random.RandomState(13)
sizes = [18, 32, 32, 2]
pol = MlpPolicy([(rs.randn(o, i) / np.sqrt(i), rs.randn(o) * 0.1) for i, o in zip(sizes[:-1], sizes[1:])], activation="tanh",
                squash="tanh", low=(0.0, 0.0), high=(2.5, 15.0))
b_env = SbrOSVec(N * K)
b_env.reset(influent=a_env.influent().T.repeat_interleave(K, dim=0))
obs_b = torch.empty((N * K, 18), device="cuda")


def restore_b():
    x, c = a_env.get_state()
    b_env.set_state(x.repeat_interleave(K, dim=1), c.repeat_interleave(K, dim=1))
    obs_b.copy_(a_env.obs.repeat_interleave(K, dim=0))


def timed(leg):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = leg()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"us_per_call": med * 1e3 / CALLS, "ms_per_launch": med, "runs_ms": [round(t, 4) for t in ts], "spread_rel": (ts[-1] - ts[0]) / med}


def measure(hold):
    def leg_a():
        return a_env.lookahead_policy(pol, K, CALLS, hold=hold, noise_std=STD, noise_seed=SEED, return_best=True)

    def leg_b():
        return b_env.rollout_policy(pol, CALLS, hold=hold, obs=obs_b, noise_std=STD, noise_seed=SEED)

    def leg_c():
        restore_b()
        ret = b_env.rollout_policy(pol, CALLS, hold=hold, obs=obs_b, noise_std=STD, noise_seed=SEED)
        return ret.reshape(N, K).max(dim=1)

    legs = {"a": leg_a, "b": leg_b, "c": leg_c}
    for f in legs.values():                            # warm-up: every kernel loaded, the allocator settled
        restore_b()
        timed(f)
    ms = {k: [] for k in legs}
    for _ in range(RUNS):
        for k, f in legs.items():
            restore_b()                                # (b) starts from the live state every time; outside its timed region
            t, _ = timed(f)
            ms[k].append(t)
    res = {k: summary(v) for k, v in ms.items()}
    a, b, c = (res[k]["ms_per_launch"] for k in "abc")
    # without noise the branches of (a) and the replicas of (b) run the same arithmetic on the same values
    restore_b()
    ret_a = a_env.lookahead_policy(pol, K, CALLS, hold=hold)
    ret_b = b_env.rollout_policy(pol, CALLS, hold=hold, obs=obs_b).reshape(N, K)
    return {
        "a_lookahead_policy_with_best": res["a"], "b_rollout_policy_on_replicas": res["b"],
        "c_replicate_rollout_policy_max": res["c"],
        "a_over_b_time": a / b, "a_over_c_time": a / c,
        "a_slower_than_b_rel": a / b - 1.0, "b_spread_rel": res["b"]["spread_rel"],
        "a_within_b_spread": bool(a / b - 1.0 <= res["b"]["spread_rel"]),
        "returns_a_equal_b_bitwise_without_noise": bool(torch.equal(ret_a, ret_b)),
    }


out = {
    "what": "%d live envs (scenarios 4..7, %d calls in), %d branches per env = %d branches, horizon %d calls, 2 x 32 tanh net, "
            "noise std %s, float32; device events, %d interleaved runs per leg, medians" % (N, ADVANCE, K, N * K, CALLS, STD, RUNS),
    "device": torch.cuda.get_device_name(0),
    "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None),
    "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
    "library_source_hash": B.source_hash(),
    "hold_1": measure(1), "hold_8": measure(8),
}
print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
a_env.close()
b_env.close()
failed = ["%s: %s" % (h, k) for h in ("hold_1", "hold_8") for k in ("a_within_b_spread", "returns_a_equal_b_bitwise_without_noise")
          if not out[h][k]]
if failed:
    sys.exit("FAILED: " + ", ".join(failed))
