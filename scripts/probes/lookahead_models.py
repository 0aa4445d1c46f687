"""lookahead_sampled_models against its parent and against the route it replaces: 4 096 envs from a live
mid-episode state (influent scenarios 4..7, 60 step() calls), a nominal tape of 50 rows, hold 1, n_steps 50.

Legs, interleaved in one process, the handle's event timer (sbr_timer_start / sbr_timer_stop) around each, every leg primed:
  (a)  env.lookahead_sampled(K = 64)                                        262 144 branches; the parent, whose instruction text
       is the parent commit's: the reference cost
  (b)  env.lookahead_sampled_models(K = 64), table = [the handle's config]  262 144 branches, M = 1
  (c)  env.lookahead_sampled_models(K = 8), table = 8 perturbed models      262 144 branches
  (d)  (c) with return_rewards, against (a) with return_rewards: the price of the store strided by M
  (e)  the route (c) replaces: 8 replica handles, each created with a model's config; per decision set_state into each of them,
       lookahead_sampled(K = 8) on each, one stream, the mean formed in torch                           8 x 32 768 branches
The table is set outside the timed windows (sbr_set_models allocates and waits for the device).

THE EXPECTATIONS, written before the first run and reported whether they hold or not:
  * (b) lies within twice (a)'s own run-to-run spread of (a): the same arithmetic over the same lanes, the constants read through
    the same scalar loads from another address;
  * (c) lies within a few per cent of (b): waves of different plants plan different step counts.  The margin is (b)'s spread plus
    the 1.3 % DESIGN.md 3.12 saw for sixteen plants;
  * (c) is ahead of (e);
  * (d)'s overhead is reported as a ratio, with no bar.

    python scripts/probes/lookahead_models.py --out lookahead_models.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gym_sbr2_amd as G  # noqa: E402
from gym_sbr2_amd import build  # noqa: E402
from gym_sbr2_amd.models import copy_config  # noqa: E402

SEED, LIVE_CALLS, MARGIN_3_12 = 1000, 60, 0.013


def stats(t):
    med = statistics.median(t)
    return {"runs": len(t), "median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_ms": round(max(t) - min(t), 4), "spread_pct": round(100 * (max(t) - min(t)) / med, 2)}


def measure(n, rows, k_wide, m, repeats, rel_std):
    k_small = k_wide // m
    env = G.SbrOSVec(n)
    scen = (4 + torch.arange(n, device="cuda") % 4).to(torch.int32)
    env.reset(seed=SEED, scenario=scen)
    gen = torch.Generator(device="cuda").manual_seed(SEED)
    for _ in range(LIVE_CALLS):
        u = torch.rand((n, 2), generator=gen, device="cuda")
        env.step(u * torch.tensor([2.5, 15.0], device="cuda"))
    tables = {1: G.PlantModels([env.cfg]), m: G.PlantModels.perturbed(env.cfg, m, rel_std=rel_std, seed=3)}
    reps = [G.SbrOSVec(n, config=copy_config(c)) for c in tables[m]]
    for r in reps:
        r.reset(influent=env.influent().T)
    nominal = torch.tensor([1.25, 7.5], device="cuda").expand(rows, n, 2).contiguous()
    sampler = G.TapeSampler((0.3, 2.0), seed=SEED, hi=(2.5, 15.0))

    def timed(fn):
        env.timer_start()
        out = fn()
        return env.timer_stop(), out

    def leg_a(rewards=False):
        return timed(lambda: env.lookahead_sampled(nominal, k_wide, sampler, return_rewards=rewards))

    def leg_models(size, fanout, rewards=False):
        env.set_models(tables[size])
        return timed(lambda: env.lookahead_sampled_models(nominal, fanout, sampler, return_rewards=rewards, return_stats=True))

    def route():
        x, c = env.get_state()
        rets = []
        for r in reps:
            r.set_state(x, c)
            rets.append(r.lookahead_sampled(nominal, k_small, sampler))
        return torch.stack(rets, dim=-1).mean(dim=-1)

    legs = {"a_lookahead_sampled_k%d" % k_wide: leg_a,
            "b_models_k%d_m1" % k_wide: lambda: leg_models(1, k_wide),
            "c_models_k%d_m%d" % (k_small, m): lambda: leg_models(m, k_small),
            "d_a_with_rewards": lambda: leg_a(True),
            "d_c_with_rewards": lambda: leg_models(m, k_small, True),
            "e_%d_replica_handles" % m: lambda: timed(route)}
    outs = {}
    for name, f in legs.items():                      # prime: every kernel loaded, the allocator settled
        outs[name] = f()[1]
    names = list(legs)
    equal_b = bool(torch.equal(outs[names[1]][0][:, :, 0], outs[names[0]]))
    mean_c, mean_e = outs[names[2]][1], outs[names[5]]
    times = {name: [] for name in legs}
    for _ in range(repeats):
        for name, f in legs.items():
            outs.pop(name, None)                      # the leg's last outputs go back to the caching allocator first
            t, outs[name] = f()
            times[name].append(t)
    res = {"n": n, "rows": rows, "hold": 1, "n_steps": rows, "k_wide": k_wide, "k_small": k_small, "models": m, "rel_std": rel_std,
           "live_calls": LIVE_CALLS, "repeats": repeats, "device": torch.cuda.get_device_name(0),
           "library_source_hash": build.source_hash(), "branches": n * k_wide,
           "b_returns_equal_a_bitwise": equal_b,
           "c_mean_against_e_mean_max_abs_diff": float((mean_c - mean_e).abs().max())}
    for name, t in times.items():
        res[name] = stats(t)
    a, b, c, da, dc, e = (res[name]["median_ms"] for name in names)
    res["b_over_a"], res["c_over_b"], res["e_over_c"] = round(b / a, 4), round(c / b, 4), round(e / c, 4)
    res["d_rewards_overhead_models"], res["d_rewards_overhead_parent"] = round(dc / c, 4), round(da / a, 4)
    res["d_c_with_rewards_over_a_with_rewards"] = round(dc / da, 4)
    res["expected_b_within_twice_the_spread_of_a"] = abs(b - a) <= 2 * res[names[0]]["spread_ms"]
    res["expected_c_within_margin_of_b"] = abs(c - b) <= res[names[1]]["spread_ms"] + MARGIN_3_12 * b
    res["expected_c_ahead_of_e"] = c < e
    for h in [env] + reps:
        h.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=50)
    ap.add_argument("--fanout", type=int, default=64, help="K of legs (a) and (b); legs (c) - (e) run K / models candidates")
    ap.add_argument("--models", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rel-std", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = measure(args.envs, args.rows, args.fanout, args.models, args.repeats, args.rel_std)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
