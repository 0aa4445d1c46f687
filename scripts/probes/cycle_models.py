"""cycle_lookahead_models against the lookahead it extends: K candidate set-point triples x S futures per env, one
cycle, scored from the live SBR-v2 handle's state, the futures on the grid's y axis and the plant of a future read from the
handle's model table.

Legs, alternated in one process, the handle's event timer (sbr_timer_start / sbr_timer_stop) around each, every leg primed:
  (a)  env.cycle_lookahead_scenarios(candidates [1, N, K, 3], futures [1, N, S, 14])   the call it extends: one plant, the future a lane
  (b)  env.cycle_lookahead_models(the same), table = [the handle's config]             M = 1: the same plant read from the table
  (c)  env.cycle_lookahead_models(the same), table = 4 perturbed models                M = 4: workgroups of one plant each
Checks that (b)'s returns are (a)'s, bit for bit.  The table is set outside the timed window (sbr_set_models allocates and waits).
Prints one JSON line per size and writes them to --out.

    python scripts/probes/cycle_models.py --out cycle_models.json
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
from gym_sbr2_amd import build  # noqa: E402


def measure(n, k, s, repeats, scheme):
    from gym_sbr2_amd import _capi
    cfg = _capi.default_config(); cfg.scheme = scheme
    rs = np.random.RandomState(1)
    scen = (np.arange(n) % 8).astype(np.int32)
    env = G.SbrEnv2Vec(n, config=cfg)
    env.reset(scenario=scen, rnd=rs.randn(n, 48))
    cand = torch.from_numpy(rs.uniform(0.1, 0.9, (1, n, k, 3))).float().cuda()
    futures = env.influent_futures(1, s, seed=2, scenario=scen, first_draw=1, current_first=False)
    tables = {1: G.PlantModels([env.cfg]), 4: G.PlantModels.perturbed(env.cfg, 4, rel_std=0.1, seed=3)}

    def timed(fn):
        env.timer_start(); fn()
        return env.timer_stop()

    def scenarios():
        return env.cycle_lookahead_scenarios(cand, futures)

    def models():
        return env.cycle_lookahead_models(cand, futures)

    env.set_models(tables[1])
    same = bool(torch.equal(models(), scenarios()))
    times = {"a_scenarios": [], "b_models_m1": [], "c_models_m4": []}
    for m in (1, 4):                               # prime every leg under either table
        env.set_models(tables[m]); models(); scenarios()
    torch.cuda.synchronize()
    for _ in range(repeats):                       # alternated: a, b, a, c, ...
        env.set_models(tables[1])
        times["a_scenarios"].append(timed(scenarios)); times["b_models_m1"].append(timed(models))
        env.set_models(tables[4])
        times["a_scenarios"].append(timed(scenarios)); times["c_models_m4"].append(timed(models))
    res = {"n": n, "k": k, "s": s, "lanes": n * k * s, "scheme": scheme, "repeats": repeats,
           "models_m1_returns_equal_scenarios": same,
           "lookahead_waves": 1 if (scheme == 1 and n * k * s <= env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS)) else 2,
           "library_source_hash": build.source_hash()}
    for name, t in times.items():
        med = statistics.median(t)
        res[name] = {"runs": len(t), "median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                     "spread_ms": round(max(t) - min(t), 4), "spread_pct": round(100 * (max(t) - min(t)) / med, 2)}
    a, b, c = (res[name] for name in times)
    res["b_over_a"] = round(b["median_ms"] / a["median_ms"], 4)
    res["c_over_a"] = round(c["median_ms"] / a["median_ms"], 4)
    # the expectation of DESIGN.md 3.11: (b)'s median is no more than (a)'s plus twice (a)'s own run-to-run spread in this run
    res["b_within_a_plus_twice_its_spread"] = b["median_ms"] <= a["median_ms"] + 2 * a["spread_ms"]
    env.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096], help="envs; lanes = envs * k * s")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--s", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scheme", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = [measure(n, args.k, args.s, args.repeats, args.scheme) for n in args.sizes]
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
