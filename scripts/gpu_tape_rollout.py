"""What the action tape costs and what it saves: one SBROS-v1 episode (463 calls) at 65536 envs, influent scenarios 4..7, the
bench's physical policy (u_DO ~ U[0, 2.5], u_EC ~ U[0, 15]), timed with device events in ONE process, the three legs interleaved:
  (a) sbr_rollout           the fused kernel under its own Philox policy
  (b) sbr_rollout_actions   the fused kernel reading the same actions from a float32 tape, hold = 1
  (c) sbr_step              the same actions, one launch per call
Writes profiles/r07_tape_rollout.json (env-steps/s and us per call of each leg, the spread of (a) over its runs, b/a, b/c,
library_source_hash).  Usage: python scripts/gpu_tape_rollout.py [runs] [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gym_sbr2_amd import SbrOSVec, _capi  # noqa: E402
from gym_sbr2_amd import build as B  # noqa: E402

N, CALLS, SEED, PSEED = 65536, 463, 1000, 77
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r07_tape_rollout.json")

cfg = _capi.default_config()
cfg.act_DO_max = 2.5                                   # what the on-device policy of (a) draws from
env = SbrOSVec(N, config=cfg)
scen = (4 + torch.arange(N, device="cuda") % 4).to(torch.int32)


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
    return env.rollout(CALLS, policy_seed=PSEED)


env.reset(seed=SEED, scenario=scen)                    # the policy's Philox counter is the env's call count: record from a reset handle
_, tape = env.rollout(CALLS, policy_seed=PSEED, return_actions=True)       # the actions of (a), as the tape of (b) and (c)


def leg_b():
    return env.rollout_actions(tape)


def leg_c():
    for c in range(CALLS):
        env.step(tape[c])
    return env.episode_returns()


legs = {"a": leg_a, "b": leg_b, "c": leg_c}
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
a, b, c = (res[k]["us_per_call"] for k in "abc")
out = {
    "what": "one SBROS-v1 episode, %d envs x %d calls, scenarios 4..7, physical policy; device events, %d interleaved runs per leg, medians"
            % (N, CALLS, RUNS),
    "device": torch.cuda.get_device_name(0),
    "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None),
    "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
    "library_source_hash": B.source_hash(),
    "a_sbr_rollout": res["a"], "b_sbr_rollout_actions_hold1_f32": res["b"], "c_sbr_step": res["c"],
    "b_over_a_time": b / a, "b_over_c_throughput": c / b,
    "b_slower_than_a_rel": b / a - 1.0, "a_spread_rel": res["a"]["spread_rel"],
    "b_within_a_spread": bool(b / a - 1.0 <= res["a"]["spread_rel"]),
    "returns_b_equal_a_bitwise": bool(torch.equal(rets["a"], rets["b"])),
    "returns_c_minus_b_max_abs": float((rets["c"] - rets["b"]).abs().max()),
    "envs_near_pole_or_nonfinite": int(((status & (_capi.ST_NEAR_POLE | _capi.ST_NONFINITE)) != 0).sum()),
}
print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
env.close()
