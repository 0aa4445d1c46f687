"""cycle_lookahead against what it replaces: K candidate set-point triples per env, one cycle, scored from the live
SBR-v2 handle's state.

Legs, interleaved in one process, device events around each, every leg primed:
  (a)  env.cycle_lookahead(candidates [N, K, 3])                      the new call: returns only
  (b)  replica.step(candidates as [N*K, 3]) on a handle of N*K envs   the k_cycle launch alone, the replica already holding the state
  (c)  get_state / influent of the live handle, repeat K times, set_state, reset(influent, carry_over=True), then (b):
       what a caller without the call pays per decision
Checks that (a)'s returns are the rewards of (b), cast to the output dtype, bit for bit.  Prints one JSON line per size and writes
them to --out.

    python scripts/probes/cycle_lookahead.py --out cycle_lookahead.json          (--scheme 0 for the RK4 scheme)
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


def timed(fn, repeats):
    """Milliseconds of `repeats` runs of fn, each between two events on the current stream."""
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(); fn(); t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def measure(n, k, repeats, scheme):
    from gym_sbr2_amd import _capi
    def config():
        cfg = _capi.default_config(); cfg.scheme = scheme
        return cfg

    rs = np.random.RandomState(1)
    env = G.SbrEnv2Vec(n, config=config())
    env.reset(scenario=(np.arange(n) % 8).astype(np.int32), rnd=rs.randn(n, 48))
    cand = torch.from_numpy(rs.uniform(0.1, 0.9, (n, k, 3))).float().cuda()
    flat = cand.reshape(n * k, 3)
    rep = G.SbrEnv2Vec(n * k, config=config())

    def replicate():
        x, c = env.get_state()
        rep.set_state(x.repeat_interleave(k, dim=1), c.repeat_interleave(k, dim=1))
        rep.reset(influent=env.influent().T.repeat_interleave(k, dim=0).contiguous(), carry_over=True)

    legs = {
        "a_cycle_lookahead": lambda: env.cycle_lookahead(cand),
        "b_replica_step": lambda: rep.step(flat, want_diag=False),
        "c_replicate_and_step": lambda: (replicate(), rep.step(flat, want_diag=False)),
    }
    replicate()
    ret = env.cycle_lookahead(cand)
    _, rew, _ = rep.step(flat, want_diag=False)
    same = bool(torch.equal(ret.reshape(-1).float(), rew))
    for fn in legs.values():                       # prime every leg
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in legs}
    for _ in range(repeats):                       # interleaved: a, b, c, a, b, c ...
        for name, fn in legs.items():
            times[name] += timed(fn, 1)
    res = {"n": n, "k": k, "lanes": n * k, "scheme": scheme, "repeats": repeats, "returns_equal_replica_rewards": same,
           "lookahead_waves": 1 if (scheme == 1 and n * k <= env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS)) else 2,
           "library_source_hash": build.source_hash()}
    for name, t in times.items():
        med = statistics.median(t)
        res[name] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                     "spread_pct": round(100 * (max(t) - min(t)) / med, 2)}
    res["a_over_b"] = round(res["a_cycle_lookahead"]["median_ms"] / res["b_replica_step"]["median_ms"], 4)
    res["a_over_c"] = round(res["a_cycle_lookahead"]["median_ms"] / res["c_replicate_and_step"]["median_ms"], 4)
    env.close(); rep.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--scheme", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = [measure(n, args.k, args.repeats, args.scheme) for n in args.sizes]
    for r in results:
        print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
