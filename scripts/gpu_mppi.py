"""What one MPPI iteration costs with the candidates drawn on the device against today's path on the parent's entry points:
1024 live envs (influent scenarios 4..7, advanced 60 calls through step), 64 candidates per env = 65536 branches, a horizon of 50
rows, hold = 1, float32 tape, sigma = (0.3, 2), candidates clamped into [0, 2.5] x [0, 15]; timed with device events in ONE
process, the three legs interleaved:
  (a) lookahead_sampled with return_best + mppi_update(shift=1)      k_lookahead_sampled, k_branch_best, k_mppi_update
  (b) today: torch randn / scale / add / clamp into [R, N, K, 2], lookahead with return_best, softmax over K and the contraction
      against the candidates in torch, the shift
  (c) lookahead with return_best alone on (a)'s actions_out
  (s) lookahead_sampled with return_best alone: (s) against (c) prices the in-kernel draw, (a) - (s) the update
and torch.cuda.max_memory_allocated of (a) and of (b), each from a reset peak.
Writes profiles/r10_mppi.json (us per call and branch-steps/s of each leg, each leg's run-to-run spread, a/b, a/c, the two
memory peaks, library_source_hash).  Usage: python scripts/gpu_mppi.py [runs] [out.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from gym_sbr2_amd import SbrOSVec, TapeSampler  # noqa: E402
from gym_sbr2_amd import build as B  # noqa: E402

N, K, ROWS, ADVANCE, SEED, TEMP = 1024, 64, 50, 60, 1000, 5.0
RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r10_mppi.json")

g = torch.Generator(device="cuda").manual_seed(SEED)
scale = torch.tensor([2.5, 15.0], device="cuda")
sigma = torch.tensor([0.3, 2.0], device="cuda")
lo, hi = torch.zeros(2, device="cuda"), scale
env = SbrOSVec(N)
env.reset(seed=SEED, scenario=(4 + torch.arange(N, device="cuda") % 4).to(torch.int32))
for _ in range(ADVANCE):
    env.step(torch.rand((N, 2), generator=g, device="cuda") * scale)
nominal = torch.rand((ROWS, N, 2), generator=g, device="cuda") * scale
sampler = TapeSampler((0.3, 2.0), seed=SEED, lo=(0.0, 0.0), hi=(2.5, 15.0))
shifted = torch.clamp(torch.arange(ROWS, device="cuda") + 1, max=ROWS - 1)
tape_a = env.lookahead_sampled(nominal, K, sampler, return_actions=True)[1]


def leg_a():
    ret, bi, br = env.lookahead_sampled(nominal, K, sampler, return_best=True)
    return env.mppi_update(nominal, ret, sampler, TEMP, shift=1), br


def leg_b():
    cand = torch.randn((ROWS, N, K, 2), generator=g, device="cuda") * sigma + nominal[:, :, None, :]
    cand[:, :, 0] = nominal                                    # keep_nominal
    cand = torch.maximum(torch.minimum(cand, hi), lo)
    ret, bi, br = env.lookahead(cand, return_best=True)
    w = torch.softmax(ret / TEMP, dim=1)
    new = torch.einsum("nk,rnkc->rnc", w.to(torch.float32), cand)        # float32: the cheapest honest form of today's path
    return new[shifted], br


def leg_c():
    ret, bi, br = env.lookahead(tape_a, return_best=True)
    return None, br


def leg_s():
    ret, bi, br = env.lookahead_sampled(nominal, K, sampler, return_best=True)
    return None, br


def timed(leg):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    out = leg()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), out


legs = {"a": leg_a, "b": leg_b, "c": leg_c, "s": leg_s}
for f in legs.values():                                # warm-up: every kernel loaded, the allocator settled
    timed(f)
ms = {k: [] for k in legs}
outs = {}
for _ in range(RUNS):
    for k, f in legs.items():
        t, outs[k] = timed(f)
        ms[k].append(t)


def peak(leg):
    """Bytes torch allocated at most while `leg` ran, above what was allocated when it started."""
    global outs
    outs = {}
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    leg()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def summary(ts):
    ts = sorted(ts)
    med = ts[len(ts) // 2]
    return {"us_per_call": med * 1e3 / ROWS, "branch_steps_per_s": N * K * ROWS / (med * 1e-3), "runs_ms": [round(t, 4) for t in ts],
            "spread_rel": (ts[-1] - ts[0]) / med}


res = {k: summary(v) for k, v in ms.items()}
a, b, c = (res[k]["us_per_call"] for k in "abc")
best_a, best_c = outs["a"][1].clone(), outs["c"][1].clone()
new_a = outs["a"][0]
in_bounds = bool((new_a >= lo).all()) and bool((new_a <= hi).all())
peak_a, peak_b = peak(leg_a), peak(leg_b)
out = {
    "what": "%d live envs (scenarios 4..7, %d calls in), %d candidates per env = %d branches, horizon %d rows, hold 1, float32 tape, "
            "temperature %g; device events, %d interleaved runs per leg, medians" % (N, ADVANCE, K, N * K, ROWS, TEMP, RUNS),
    "device": torch.cuda.get_device_name(0),
    "gcn_arch": getattr(torch.cuda.get_device_properties(0), "gcnArchName", None),
    "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
    "library_source_hash": B.source_hash(),
    "a_lookahead_sampled_best_mppi_update": res["a"], "b_torch_candidates_lookahead_torch_update": res["b"],
    "c_lookahead_on_a_actions_out": res["c"], "s_lookahead_sampled_best_alone": res["s"],
    "a_over_b_time": a / b, "a_over_c_time": a / c, "s_over_c_time": res["s"]["us_per_call"] / c,
    "a_slower_than_b_rel": a / b - 1.0, "b_spread_rel": res["b"]["spread_rel"],
    "a_within_b_spread": bool(a / b - 1.0 <= res["b"]["spread_rel"]),
    "peak_bytes_a": peak_a, "peak_bytes_b": peak_b,
    "best_return_a_equal_c_bitwise": bool(torch.equal(best_a, best_c)),
    "update_a_inside_bounds": in_bounds,
}
print(json.dumps(out, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
env.close()
