"""A/B timing of the fused entry points behind k_rollout under two libraries, each run in a process of its own (SBR_AMD_LIB).
usage: python scripts/gpu_fused_ab.py before.so after.so [--out log]

Order of the processes: before, before, before (the run-to-run spread of ONE library: what a ratio has to exceed to mean
anything), then after and before alternating, three of each.  Per entry point the device time of one launch (the handle's
events around it), median of 7 launches behind a 0.2 s warm-up; 20 calls, hold 2.  Lane counts: 65 536 (8192 envs x fanout 8 for
the lookaheads, 65 536 envs for the rollouts) - the one-wave builds - and 131 072 for `lookahead` again, the two-waves build.
A rollout starts every launch from the same reset state (a launch moves the handle); the lookaheads leave it alone."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import json, sys, time, warnings
sys.path.insert(0, %r)
import numpy as np, torch
from gym_sbr2_amd import SbrOSVec, MlpPolicy
from gym_sbr2_amd.planner import TapeSampler
warnings.simplefilter("ignore")
STEPS, HOLD, ROWS, K = 20, 2, 10, 8
rs = np.random.RandomState(3)
sizes = [18, 32, 32, 2]
pol = MlpPolicy([(rs.randn(o, i) / np.sqrt(i), rs.randn(o) * 0.1) for i, o in zip(sizes[:-1], sizes[1:])], low=(0.0, 0.0), high=(2.5, 15.0))
sm = TapeSampler((0.3, 2.0), seed=9)

def live(n):
    env = SbrOSVec(n)
    def again():
        env.reset(seed=1, scenario=(torch.arange(n, device="cuda") %% 8).to(torch.int32))
        a = torch.tensor([1.0, 5.0], device="cuda").expand(n, 2).contiguous()
        for _ in range(30): env.step(a)
    again()
    return env, again

def timed(env, launch, before=None):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.2:
        if before: before()
        launch()
        torch.cuda.synchronize()
    ts = []
    for _ in range(7):
        if before: before()
        torch.cuda.synchronize(); env.timer_start(); launch(); ts.append(env.timer_stop() * 1e3)
    return sorted(ts)[3]

out = {}
for n, tag in ((8192, "65536"), (16384, "131072")):
    env, _ = live(n)
    tape = torch.rand(ROWS, n, K, 2, device="cuda") * torch.tensor([2.5, 15.0], device="cuda")
    out["lookahead@" + tag] = timed(env, lambda: env.lookahead(tape, STEPS, hold=HOLD))
    if n == 8192:
        nom = tape[:, :, 0].contiguous()
        out["lookahead_end@" + tag] = timed(env, lambda: env.lookahead_end(tape, STEPS, hold=HOLD))
        out["lookahead_sampled_end@" + tag] = timed(env, lambda: env.lookahead_sampled_end(nom, K, sm, STEPS, hold=HOLD))
        out["lookahead_policy@" + tag] = timed(env, lambda: env.lookahead_policy(pol, K, STEPS, hold=HOLD, noise_std=(0.25, 2.0), keep_mean=True))
    env.close()
n = 65536
env, again = live(n)
x0, c0 = (t.clone() for t in env.get_state())
obs0 = env.obs.to(torch.float32).clone()
tape = torch.rand(ROWS, n, 2, device="cuda") * torch.tensor([2.5, 15.0], device="cuda")
back = lambda: env.set_state(x0, c0)
out["rollout_actions@65536"] = timed(env, lambda: env.rollout_actions(tape, STEPS, hold=HOLD), back)
obs = obs0.clone()
def back_obs():
    env.set_state(x0, c0); obs.copy_(obs0)
out["rollout_policy@65536"] = timed(env, lambda: env.rollout_policy(pol, STEPS, hold=HOLD, obs=obs), back_obs)
env.close()
print("RESULT " + json.dumps(out))
'''


def child(lib):
    env = dict(os.environ, SBR_AMD_LIB=os.path.abspath(lib))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:
        sys.exit("child under %s failed (%d): %s" % (lib, r.returncode, r.stderr[-2000:]))
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out:
        args.remove(out)
    before, after = args
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("before = %s, after = %s; us per launch of 20 calls, median of 7" % (os.path.basename(before), os.path.basename(after)))
    runs = []
    for name, lib in (("before", before),) * 3 + (("after", after), ("before", before)) * 3:
        r = child(lib)
        runs.append((name, r))
        say("%-6s %s" % (name, "  ".join("%s %.1f" % (k, v) for k, v in r.items())))
    say("")
    say("%-28s %10s %10s %8s %22s" % ("entry point @ lanes", "before", "after", "ratio", "before/before spread"))
    for k in runs[0][1]:
        b = [r[k] for n, r in runs if n == "before"]
        a = [r[k] for n, r in runs if n == "after"]
        mb, ma = statistics.median(b), statistics.median(a)
        say("%-28s %10.1f %10.1f %8.4f %10.4f .. %.4f" % (k, mb, ma, ma / mb, min(b) / mb, max(b) / mb))
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
