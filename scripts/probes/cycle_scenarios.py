"""cycle_lookahead_scenarios against the lookahead it extends: K candidate set-point triples x S influent futures
per env, one cycle, scored from the live SBR-v2 handle's state.

Legs, interleaved in one process, device events around each, every leg primed:
  (a)  env.cycle_lookahead_scenarios(candidates [1, N, K, 3], futures [1, N, S, 14])   the new call: returns only
  (b)  env.cycle_lookahead(candidates [N, K*S, 3])     the same number of branches under the stored influent: the kernel (a) extends
  (c)  env.draw_influent(1, S)                         drawing the futures (a) reads
Checks that with every future equal to the stored influent (a)'s returns are (b)'s, bit for bit.  Prints one JSON line per size
and writes them to --out.

    python scripts/probes/cycle_scenarios.py --out cycle_scenarios.json          (--scheme 0 for the RK4 scheme)
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


def timed(fn):
    """Milliseconds of one run of fn between two events on the current stream."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(); fn(); t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def measure(n, k, s, repeats, scheme):
    from gym_sbr2_amd import _capi
    cfg = _capi.default_config(); cfg.scheme = scheme
    rs = np.random.RandomState(1)
    scen = (np.arange(n) % 8).astype(np.int32)
    env = G.SbrEnv2Vec(n, config=cfg)
    env.reset(scenario=scen, rnd=rs.randn(n, 48))
    cand = torch.from_numpy(rs.uniform(0.1, 0.9, (1, n, k, 3))).float().cuda()
    wide = cand[0][:, :, None].expand(n, k, s, 3).reshape(n, k * s, 3).contiguous()      # (b)'s branch (k, s) runs (a)'s candidate k
    futures = env.influent_futures(1, s, seed=2, scenario=scen, first_draw=1, current_first=False)
    stored = env.influent_futures(1, s, scenario=scen)                                   # every future the stored influent
    same = bool(torch.equal(env.cycle_lookahead_scenarios(cand, stored).reshape(n, k * s), env.cycle_lookahead(wide)))
    legs = {
        "a_cycle_lookahead_scenarios": lambda: env.cycle_lookahead_scenarios(cand, futures),
        "b_cycle_lookahead": lambda: env.cycle_lookahead(wide),
        "c_draw_influent": lambda: env.draw_influent(1, s, seed=2, scenario=scen, first_draw=1),
    }
    for fn in legs.values():                       # prime every leg
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):                       # interleaved: a, b, c, a, b, c ...
        for name, fn in legs.items():
            times[name].append(timed(fn))
    res = {"n": n, "k": k, "s": s, "lanes": n * k * s, "scheme": scheme, "repeats": repeats,
           "returns_equal_cycle_lookahead_under_the_stored_influent": same,
           "lookahead_waves": 1 if (scheme == 1 and n * k * s <= env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS)) else 2,
           "library_source_hash": build.source_hash()}
    for name, t in times.items():
        med = statistics.median(t)
        res[name] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                     "spread_ms": round(max(t) - min(t), 4), "spread_pct": round(100 * (max(t) - min(t)) / med, 2)}
    a, b, c = (res[name] for name in legs)
    res["a_over_b"] = round(a["median_ms"] / b["median_ms"], 4)
    res["c_over_a"] = round(c["median_ms"] / a["median_ms"], 4)
    # the acceptance of DESIGN.md 3.10: (a)'s median is no more than (b)'s plus the larger of the two legs' run-to-run spreads
    res["a_within_b_plus_spread"] = a["median_ms"] <= b["median_ms"] + max(a["spread_ms"], b["spread_ms"])
    env.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096], help="envs; lanes = envs * k * s")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--s", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
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
