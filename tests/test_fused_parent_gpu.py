"""The fused entry points behind k_rollout after their refactor (k_lookahead_tape and
k_lookahead_tape_end are one body under two kernels, and all seven are launched through one host helper): their results must not
have moved by a bit.  Every output of rollout_actions, rollout_policy, lookahead, lookahead_end, lookahead_sampled,
lookahead_sampled_end and lookahead_policy against arrays the PARENT commit's library wrote on the device for the same inputs
(tests/golden/fused_parent.npz; `record()` below is what wrote them), compared as raw bits, NaNs included.

Shapes, the smallest that reach every branch of the shared code: 100 envs x fanout 3 = 300 branches, two workgroups, the second
partial with its first branch (256 = 85 * 3 + 1) in the middle of an env, so e0 / el of the branch addressing count; 5 calls under
hold = 2, so a row change falls inside the launch and the last row covers one call.  The envs are tests/plan_cases.py's: its 73
cases as they are (every branch of scheme 1's step-count rule, the NaN guard among them), 7 that finish with the first call of
the launch, 6 with its second, 14 done on entry.  Configurations: scheme 1 and 0, each with float32 tapes and a 32-wide net and
with float64 tapes and a population of 64-wide nets; exploration noise on, keep_mean = 1; and fanout 1 on its own.

The two-waves builds are chosen by the lane count (above 98 304 lanes on a whole MI355X) and are not reached at these shapes: for
them the check is the ISA comparison of profiles/r14_fused_isa.txt (registers, spills, scratch, LDS, the step loops' float64
mix and the store count of every build equal to the parent's)."""
import os
import warnings

import numpy as np
import plan_cases as PC
import pytest
from conftest import GOLDEN
from gpu_common import handle, package, to_np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, N_STEPS, HOLD, ROWS = 100, 5, 2, 3
STD = (0.25, 2.0)
#          name            scheme  float64 tapes  net width  fanout
CONFIGS = (("b5_f32_h32", 1, False, 32, 3),
           ("b5_f64_h64", 1, True, 64, 3),
           ("rk4_f32_h32", 0, False, 32, 3),
           ("rk4_f64_h64", 0, True, 64, 3),
           ("b5_fanout1", 1, False, 32, 1))
FIXTURE = os.path.join(GOLDEN, "fused_parent.npz")


def cases():
    """x [14, N], ctrl [NCTRL, N], the cases' own actions [N, 2]: see the module's docstring."""
    from gym_sbr2_amd import _capi
    T = PC.table()
    idx = np.arange(N) % T.n
    x, ctrl, act = T.x[idx].copy(), T.ctrl[idx].copy(), T.action[idx].copy()
    e = np.load(PC.GOLDEN)
    calls = int(e["n_calls"])
    for rows, back in ((slice(73, 80), 1), (slice(80, 86), 3)):       # from the episode's `back`-th last control interval
        ctrl[rows, _capi.C_T] = float(e["iv_t_start"][-back])
        ctrl[rows, _capi.C_STEPS] = calls - back
    ctrl[86:, _capi.C_DONE] = 1.0
    return np.ascontiguousarray(x.T), np.ascontiguousarray(ctrl.T), act


def _policy(width, population):
    from gym_sbr2_amd import MlpPolicy

    def one(seed):
        rs = np.random.RandomState(seed)
        sizes = [18, width, width, 2]
        layers = [(rs.randn(o, i) / np.sqrt(i), rs.randn(o) * 0.1) for i, o in zip(sizes[:-1], sizes[1:])]
        return MlpPolicy(layers, activation="tanh", squash="tanh", low=(0.0, 0.0), high=(2.5, 15.0))
    with warnings.catch_warnings():                      # the 64-wide net's cost is not what this file is about
        warnings.simplefilter("ignore", RuntimeWarning)
        return MlpPolicy.stack([one(31), one(32)], 256) if population else one(31)


def run(G, scheme, act64, width, fanout):
    """{name: numpy array} of everything the seven entry points return for one configuration, and the handle's state behind the
    two rollouts."""
    from gym_sbr2_amd.planner import TapeSampler
    adt = torch.float64 if act64 else torch.float32
    x, ctrl, act = cases()
    rs = np.random.RandomState(1400 + 10 * scheme + fanout)
    tape = np.stack([rs.uniform(0, 2.5, (ROWS, N, fanout)), rs.uniform(0, 15, (ROWS, N, fanout))], axis=-1)
    tape[0] = act[:, None, :]                              # the first call is the one the case was built for
    tape = torch.from_numpy(tape).to(adt).cuda()
    obs = torch.from_numpy(rs.randn(N, 18).astype(np.float32)).cuda()
    pol = _policy(width, population=width == 64)
    sampler = TapeSampler((0.3, 2.0), seed=9, keep_nominal=True)
    out = {}

    def fresh():
        env = handle(G, N, scheme, "eqi_oci", out_dtype=torch.float32, action_dtype=adt)
        env.reset(seed=0)
        env.set_state(x, ctrl)
        return env

    def keep(prefix, names, values):
        for name, v in zip(names, values):
            out[prefix + "." + name] = to_np(v).copy()

    env = fresh()
    keep("rollout_actions", ("returns", "rewards"), env.rollout_actions(tape[:, :, 0].contiguous(), N_STEPS, hold=HOLD, return_rewards=True))
    keep("rollout_actions", ("x", "ctrl"), env.get_state())
    env.close()
    env = fresh()
    o = obs.clone()
    keep("rollout_policy", ("returns", "actions", "rewards"),
         env.rollout_policy(pol, N_STEPS, hold=HOLD, obs=o, noise_std=STD, noise_seed=5, return_actions=True, return_rewards=True))
    keep("rollout_policy", ("obs", "x", "ctrl"), (o,) + tuple(env.get_state()))
    env.close()
    env = fresh()
    best = ("returns", "rewards", "best_index", "best_return")
    end = ("obs_end", "state_end", "done_end")
    keep("lookahead", best, env.lookahead(tape, N_STEPS, hold=HOLD, return_rewards=True, return_best=True))
    keep("lookahead_end", best + end, env.lookahead_end(tape, N_STEPS, hold=HOLD, return_rewards=True, return_best=True))
    nominal = tape[:, :, 0].contiguous()
    keep("lookahead_sampled", best + ("actions",),
         env.lookahead_sampled(nominal, fanout, sampler, N_STEPS, hold=HOLD, return_rewards=True, return_best=True, return_actions=True))
    keep("lookahead_sampled_end", best + ("actions",) + end,
         env.lookahead_sampled_end(nominal, fanout, sampler, N_STEPS, hold=HOLD, return_rewards=True, return_best=True,
                                   return_actions=True))
    keep("lookahead_policy", best + ("actions",) + end,
         env.lookahead_policy(pol, fanout, N_STEPS, hold=HOLD, obs=obs, noise_std=STD, noise_seed=5, keep_mean=True,
                              return_rewards=True, return_best=True, return_actions=True, return_end=True))
    env.close()
    return out


def record(G, path=FIXTURE):
    """Writes the fixture: to be run with the PARENT commit's library loaded."""
    arrays = {}
    for name, scheme, act64, width, fanout in CONFIGS:
        for key, v in run(G, scheme, act64, width, fanout).items():
            arrays[name + "." + key] = v
    np.savez_compressed(path, **arrays)
    return arrays


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def G():
    return package()


@pytest.fixture(scope="module")
def parent():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize("name,scheme,act64,width,fanout", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_output_is_bit_identical_to_the_parent_commit(G, parent, name, scheme, act64, width, fanout):
    got = run(G, scheme, act64, width, fanout)
    assert sorted(name + "." + k for k in got) == sorted(k for k in parent if k.startswith(name + "."))
    for key, v in got.items():
        ref = parent[name + "." + key]
        assert v.dtype == ref.dtype and v.shape == ref.shape and np.array_equal(bits(v), bits(ref)), (name, key)
    # the fixture is not a comparison of zeros, and holds the three kinds of env
    de, rew = got["lookahead_end.done_end"], got["lookahead.rewards"]
    assert de[86:].all() and de[73:86].all() and not de[:73].all()
    assert (rew[:, 86:] == 0).all() and (rew[0, 73:86] != 0).all() and (rew[1, 80:86] != 0).all()
    assert (rew[1:, 73:80] == 0).all() and (rew[2:, 80:86] == 0).all()
    assert (rew[4, :73] != 0).any() and np.isnan(got["rollout_actions.returns"]).any()
