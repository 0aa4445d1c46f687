"""collect_policy_models / reset_models against their parents and against the route they replace: one SBROS-v1
episode of 463 calls at 65 536 envs, hold 1, the 2 x 32 tanh net of scripts/gpu_policy_collect.py, influent scenarios 4..7 (no env
flagged under the nominal plant).

Legs, interleaved in one process, the handle's event timer (sbr_timer_start / sbr_timer_stop) around each, every leg primed:
  (a)  env.collect_policy(pol, 463)                           the parent: its instruction text is the parent commit's
  (b)  env.collect_policy_models(pol, 463, 256), table = [the handle's config]     M = 1: the same plant read from the table
  (c)  env.collect_policy_models(pol, 463, 256), table = 16 perturbed models       M = 16, a plant per 256 envs
  (d)  16 handles of 4 096 envs, handle m created with model m's config, collect_policy on each, one after the other on one
       stream: the route (c) replaces (the same 65 536 env-episodes under the same 16 plants, 4 096 per plant; which env meets
       which plant differs from (c)'s rule, so the two are compared by their time alone)
  (e)  env.reset(...) against env.reset_models(256, ...) under the 16 models
The table is set outside the timed windows (sbr_set_models allocates and waits for the device).

THE EXPECTATION, written before the first run: (b)'s median lies within twice (a)'s own run-to-run spread of (a)'s median - the
model is read through the same scalar loads from another address - and (c) is well ahead of (d): 16 launches of 64 wavefronts
each leave fifteen sixteenths of the chip idle, so (d) should cost several times (c).  Whatever comes out is reported, the two
flags below included, also where they are false.

    python scripts/probes/collect_models.py --out collect_models.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gym_sbr2_amd as G  # noqa: E402
from gym_sbr2_amd import _capi, build  # noqa: E402
from gym_sbr2_amd.models import copy_config  # noqa: E402

CALLS, SEED, NET_SEED, PER = 463, 1000, 13, 256


def policy():
    rs = np.random.RandomState(NET_SEED)
    sizes = [18, 32, 32, 2]
    layers = [(rs.randn(o, i) / np.sqrt(i), rs.randn(o) * 0.1) for i, o in zip(sizes[:-1], sizes[1:])]
    return G.MlpPolicy(layers, activation="tanh", squash="tanh", low=(0, 0), high=(2.5, 15))


def stats(t):
    med = statistics.median(t)
    return {"runs": len(t), "median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_ms": round(max(t) - min(t), 4), "spread_pct": round(100 * (max(t) - min(t)) / med, 2)}


def measure(n, m, repeats, rel_std):
    pol = policy()
    env = G.SbrOSVec(n)
    scen = (4 + torch.arange(n, device="cuda") % 4).to(torch.int32)
    tables = {1: G.PlantModels([env.cfg]), m: G.PlantModels.perturbed(env.cfg, m, rel_std=rel_std, seed=3)}
    share = n // m
    parts = [G.SbrOSVec(share, first_env_id=k * share, config=copy_config(c)) for k, c in enumerate(tables[m])]

    def timed(fn):
        env.timer_start()
        out = fn()
        return env.timer_stop(), out

    def fresh(models=False):
        if models:
            env.reset_models(PER, seed=SEED, scenario=scen)
        else:
            env.reset(seed=SEED, scenario=scen)

    def leg_a():
        fresh()
        return timed(lambda: env.collect_policy(pol, CALLS))

    def leg_models(size):
        env.set_models(tables[size])
        fresh(models=True)
        return timed(lambda: env.collect_policy_models(pol, CALLS, PER))

    def leg_d():
        for k, p in enumerate(parts):
            p.reset(seed=SEED, scenario=scen[k * share:(k + 1) * share])
        return timed(lambda: [p.collect_policy(pol, CALLS).returns for p in parts])

    def leg_e(models):
        env.set_models(tables[m])
        return timed(lambda: fresh(models))[0]

    legs = {"a_collect_policy": leg_a, "b_models_m1": lambda: leg_models(1), "c_models_m%d" % m: lambda: leg_models(m),
            "d_%d_handles" % m: leg_d}
    outs = {}
    for name, f in legs.items():                      # prime: every kernel loaded, the allocator settled
        outs[name] = f()[1]
    leg_e(False); leg_e(True)
    equal_b = bool(torch.equal(outs["b_models_m1"].returns, outs["a_collect_policy"].returns))
    fresh()
    env.collect_policy(pol, CALLS)
    flagged = int(((env.status() & 7) != 0).sum())
    times = {name: [] for name in legs}
    times["e_reset"], times["e_reset_models_m%d" % m] = [], []
    for _ in range(repeats):
        for name, f in legs.items():
            outs.pop(name, None)                      # the leg's last outputs go back to the caching allocator first
            t, outs[name] = f()
            times[name].append(t)
        times["e_reset"].append(leg_e(False)); times["e_reset_models_m%d" % m].append(leg_e(True))
    res = {"n": n, "models": m, "envs_per_model": PER, "calls": CALLS, "hold": 1, "rel_std": rel_std, "repeats": repeats,
           "device": torch.cuda.get_device_name(0), "library_source_hash": build.source_hash(),
           "rollout_waves": env.query(_capi.Q_ROLLOUT_WAVES), "envs_flagged_under_the_nominal_plant": flagged,
           "b_returns_equal_a_bitwise": equal_b}
    for name, t in times.items():
        res[name] = stats(t)
    a, b, c, d = (res[name]["median_ms"] for name in legs)
    res["b_over_a"], res["c_over_a"], res["d_over_c"] = round(b / a, 4), round(c / a, 4), round(d / c, 4)
    res["reset_models_over_reset"] = round(res["e_reset_models_m%d" % m]["median_ms"] / res["e_reset"]["median_ms"], 4)
    res["expected_b_within_twice_the_spread_of_a"] = abs(b - a) <= 2 * res["a_collect_policy"]["spread_ms"]
    res["expected_c_well_ahead_of_d"] = d >= 2 * c
    for e in [env] + parts:
        e.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--models", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rel-std", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = measure(args.envs, args.models, args.repeats, args.rel_std)
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
