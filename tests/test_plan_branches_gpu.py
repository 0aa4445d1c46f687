"""Scheme 1's step-count rule on the device, branch by branch, against the CPU oracle - and every kernel that inlines sbr_b5a
against that.  The cases are tests/plan_cases.py's table (held to its own conditions by tests/test_plan_branches_cpu.py): plans 1,
2 and 4 by z_ub, 2 and 4 by the n_s floor, slaved 130 and 132, knee counts 5 .. 63 and the stable 64, each in the dosing and in
the plain form, compared BY STATE; the guards and the overflowing cap by count.  One call per handle throughout."""
import numpy as np
import plan_cases as PC
import pytest
from gpu_common import package, plans_agree

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return package()


@pytest.fixture(scope="module")
def T():
    return PC.table()


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """torch.equal with NaN equal to NaN (the NaN guard case and the overflowing cap)."""
    if not a.is_floating_point():
        return torch.equal(a, b)
    return a.shape == b.shape and bool((torch.isnan(a) == torch.isnan(b)).all()) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def _handle(G, x, ctrl, action_dtype=torch.float64, reward=None):
    """A handle holding the cases x [n, 14], ctrl [n, NCTRL]: reset, then the injected state."""
    env = G.SbrOSVec(len(x), out_dtype=torch.float64, action_dtype=action_dtype, reward=reward)
    env.reset(seed=0)
    env.set_state(np.ascontiguousarray(x.T), np.ascontiguousarray(ctrl.T))
    return env


def _step(G, x, ctrl, action, action_dtype=torch.float64, reward=None):
    """One step() of the cases on a handle of their own: obs, state, reward, done, plant [14, n], controller rows [25, n]."""
    env = _handle(G, x, ctrl, action_dtype, reward)
    outs = [t.clone() for t in env.step(torch.from_numpy(np.ascontiguousarray(action)).to(action_dtype).cuda())]
    outs += list(env.get_state())
    env.close()
    return outs


def _pick(outs, idx):
    """The envs idx of what _step returned."""
    i = torch.as_tensor(idx, device="cuda")
    return [t[i] for t in outs[:4]] + [t[:, i] for t in outs[4:]]


def _lockstep(ora, oout, outs, compare, what):
    """The project's lockstep bar (test_perturbed_model_constants_and_derivative_action_against_oracle) on the envs `compare`;
    the plan on all.  Returns the gate of every env."""
    from gym_sbr2_amd import _capi
    o, s_, r, d, x, ctrl = (_np(t) for t in outs)
    oo, os_, orr, od = oout
    plans_agree(ctrl, ora)
    g = PC.gate(x.T, ora.envs["x"]).max(axis=1)
    c = compare
    assert g[c].max() < 1e-6, (what, g[c].max())
    assert np.array_equal(d, od) and np.abs(r[c] - orr[c]).max() < 1e-11, what
    assert np.abs(o[c] - oo[c]).max() < 1e-9 and np.abs(s_[c] - os_[c]).max() < 1e-9, what
    assert np.array_equal(ctrl[_capi.C_T], ora.envs["t"]) and np.array_equal(ctrl[_capi.C_STEPS], ora.envs["steps"]), what
    for row, key in ((_capi.C_SO_M1, "so_m1"), (_capi.C_SO_M2, "so_m2"), (_capi.C_SNO_M1, "sno_m1"), (_capi.C_SNO_M2, "sno_m2"),
                     (_capi.C_IE_DO, "ie_do"), (_capi.C_IE_EC, "ie_ec"), (_capi.C_EC_LAST, "ec_last"), (_capi.C_KLA_LAST, "kla_last")):
        assert np.allclose(ctrl[row][c], ora.envs[key][c], rtol=1e-9, atol=1e-12), (what, key)
    return g


@pytest.fixture(scope="module")
def first(G, T):
    """The table in its own order through step() with float64 actions: what every other layout and build must reproduce."""
    return _step(G, T.x, T.ctrl, T.action)


def test_step_in_lockstep_with_the_oracle_on_every_branch(G, T, first):
    """set_state + step(a) against load_state + step(a), float64 actions.  C_PLAN equals the oracle's plan on every case; on the
    state-compared ones the end state is inside 1e-6 gate, reward 1e-11, observations 1e-9, C_T equal.
    Measured on MI355X, worst gate per class, plain / dosing form (cases): 1, 2, 4 by z_ub 1.3e-11 (10) / 4.5e-11 (6); 2, 4 by the
    n_s floor 2.2e-11 (6) / 5.9e-11 (4); slaved 130, 132 1.3e-11 (5) / 5.2e-11 (6); knee 5 .. 63 and the stable 64 4.6e-11 (18) /
    1.7e-9 (9; knee63-anox-dose, then knee64-anox-dose 9.0e-10): 580 times under the bar, condition (a) allows 1e-9 of input noise."""
    ora, oout = PC.oracle_call(T.x, T.ctrl, T.action)
    g = _lockstep(ora, oout, first, T.compare, "table")
    assert np.array_equal(_np(first[5])[-1].astype(np.int64), T.plan)
    for cls in ("z", "s", "slaved", "knee"):
        for dose in (False, True):
            m = T.compare & (T.cls == cls) & (T.dose == dose)
            print("plan class %-6s %s: %2d cases, plans %s, worst gate %.3e" % (cls, "dosing" if dose else "plain ", m.sum(), sorted(set(T.plan[m].tolist())), g[m].max()))
    top = np.argsort(-np.where(T.compare, g, 0))[:3]
    print("worst three: " + ", ".join("%s %.3e" % (T.names[i], g[i]) for i in top))


def _layouts(T):
    """sorted by plan; interleaved: the first wavefront holds plans 1, 2, 4, 7, 41, 63, 130 and 132 in the dosing and in the plain
    form on neighbouring lanes, the other cases behind them alternating between the two forms as far as they last."""
    by_plan = np.argsort(T.plan, kind="stable")
    head = []
    for plan in (1, 2, 4, 7, 41, 63, 130, 132):
        for dose in (True, False):
            head.append(int(np.nonzero(T.compare & (T.plan == plan) & (T.dose == dose))[0][0]))
    rest = [i for i in range(T.n) if i not in head]
    dosing, plain = [i for i in rest if T.dose[i]], [i for i in rest if not T.dose[i]]
    tail = []
    while dosing or plain:
        tail += ([dosing.pop(0)] if dosing else []) + ([plain.pop(0)] if plain else [])
    mixed = np.array(head + tail)
    assert sorted(mixed.tolist()) == list(range(T.n)) and set(T.plan[mixed[:64]]) >= {1, 2, 4, 7, 41, 63, 64, 130, 132}
    assert T.dose[mixed[:64]].sum() >= 24 and (~T.dose[mixed[:64]]).sum() >= 24
    return by_plan, mixed


SINGLES = ("z1-anox-dose", "z4-aer-golden", "s4-anox-dose", "130-anox-dose", "132-anox-dose-big", "knee7-aer", "knee33-aer",
           "knee41-anox-dose", "knee63-anox-plain", "knee64-anox-dose", "guard-m1-anox-dose", "cap64-aer-x1e6")


def test_lane_mixes_give_every_env_the_same_bits(G, T, first):
    """The same cases sorted by plan, interleaved (one wavefront with 1 .. 63-step lanes, dosing next to plain), and a dozen of
    them alone on single-env handles - where a plain case runs the plain build, while in the table every wavefront doses: outputs,
    plant and controller rows are the same bits.  Pins the masking of lanes that finish early under wave-mates that run up to 64
    steps, and the Q == 0 lane of a dosing wave."""
    for order in _layouts(T):
        outs = _step(G, T.x[order], T.ctrl[order], T.action[order])
        for u, v in zip(outs, _pick(first, order)):
            assert _same(u, v)
    for name in SINGLES:
        i = T.names.index(name)
        outs = _step(G, T.x[i:i + 1], T.ctrl[i:i + 1], T.action[i:i + 1])
        for u, v in zip(outs, _pick(first, [i])):
            assert _same(u, v), name


def test_other_builds_of_k_step_give_the_same_bits(G, T, first):
    """The table tiled over handles that run the other builds of k_step - many 64-thread workgroups, 256-thread workgroups with
    one wave per SIMD, and above Q_STEP_TWO_WAVES_ABOVE_ENVS the parked two-waves build (ragged last workgroup) - one call each."""
    from gym_sbr2_amd import _capi
    probe = G.SbrOSVec(1)
    small, above = probe.query(_capi.Q_STEP_SMALL_BATCH_ENVS), probe.query(_capi.Q_STEP_TWO_WAVES_ABOVE_ENVS)
    probe.close()
    for n, block, waves in ((4096 + 37, 64, 1), (above, 256 if above > small else 64, 1), (above + 320, 256, 2)):
        idx = np.arange(n) % T.n
        env = _handle(G, T.x[idx], T.ctrl[idx])
        assert (env.query(_capi.Q_STEP_BLOCK), env.query(_capi.Q_STEP_WAVES)) == (block, waves), n
        outs = [t.clone() for t in env.step(torch.from_numpy(T.action[idx]).cuda())] + list(env.get_state())
        env.close()
        for u, v in zip(outs, _pick(first, idx)):
            assert _same(u, v), n


def _rows_but_plan(ctrl):
    from gym_sbr2_amd import _capi
    assert _capi.C_PLAN == ctrl.shape[0] - 1
    return ctrl[:-1]


@pytest.mark.parametrize("reward", ["eqi_oci", "oci"])
def test_fused_kernels_from_the_same_injected_state(G, T, reward):
    """k_rollout_tape, k_lookahead_tape, k_lookahead_sampled and k_rollout_policy, one call each from the table's states under
    float32 actions, against step() on a float32-action twin: returns and per-call rewards are the twin's reward bit for bit, and
    after the state-writing kernels so are the plant and every controller row but C_PLAN (which the rollouts leave 0).  With the
    lockstep test this ties every inlined copy of sbr_b5a to the oracle at every branch.  The tape kernel also runs its two-waves
    build, tiled above Q_FUSED_ONE_WAVE_MAX_ENVS."""
    from gym_sbr2_amd import _capi
    from gym_sbr2_amd.planner import TapeSampler
    from gym_sbr2_amd.policy import MlpPolicy
    f32 = torch.float32
    a32 = T.action.astype(np.float32)
    twin = _step(G, T.x, T.ctrl, a32, f32, reward)
    r, x_t, c_t = twin[2], twin[4], twin[5]
    # the twin itself against the oracle under the same float32 set-points (their rounding moves Kla and EC a little, and no plan)
    ora, oout = PC.oracle_call(T.x, T.ctrl, a32.astype(np.float64), reward_kind=_capi.REWARD_KINDS[reward])
    _lockstep(ora, oout, twin, T.compare, "float32 twin, " + reward)
    assert np.array_equal(_np(c_t)[-1].astype(np.int64), T.plan)
    act = torch.from_numpy(a32).cuda()

    def wrote_the_twin(env, idx=None):
        x, c = env.get_state()
        xt, ct = (x_t, c_t) if idx is None else (x_t[:, idx], c_t[:, idx])
        assert _same(x, xt) and _same(_rows_but_plan(c), _rows_but_plan(ct)) and bool((c[-1] == 0).all())

    # the tape kernel
    env = _handle(G, T.x, T.ctrl, f32, reward)
    ret, rew = env.rollout_actions(act[None], return_rewards=True)
    assert _same(ret, r) and _same(rew[0], r)
    wrote_the_twin(env)
    env.close()
    # both lookahead kernels: read-only
    env = _handle(G, T.x, T.ctrl, f32, reward)
    x0, c0 = env.get_state()
    ret, rew = env.lookahead(act[None, :, None, :].repeat(1, 1, 2, 1).contiguous(), return_rewards=True)
    assert ret.shape == (T.n, 2) and _same(ret[:, 0], r) and _same(ret[:, 1], r) and _same(rew[0, :, 0], r) and _same(rew[0, :, 1], r)
    ret, rew = env.lookahead_sampled(act[None], 2, TapeSampler(0.0, keep_nominal=False), return_rewards=True)
    assert ret.shape == (T.n, 2) and _same(ret[:, 0], r) and _same(ret[:, 1], r) and _same(rew[0, :, 0], r) and _same(rew[0, :, 1], r)
    x1, c1 = env.get_state()
    assert _same(x0, x1) and _same(c0, c1)
    env.close()
    # the policy kernel: a population of nets without hidden layers, weights 0, member k's bias = case k's action; 256 envs each
    per = 256
    pop = MlpPolicy.stack([MlpPolicy([(np.zeros((2, _capi.NOBS), np.float32), a32[k])], squash="none") for k in range(T.n)], per)
    idx = np.arange(T.n * per) // per
    env = _handle(G, T.x[idx], T.ctrl[idx], f32, reward)
    obs = torch.zeros((T.n * per, _capi.NOBS), dtype=f32, device="cuda")
    tidx = torch.as_tensor(idx, device="cuda")
    ret, acts, rew = env.rollout_policy(pop, 1, obs=obs, return_actions=True, return_rewards=True)
    assert torch.equal(acts[0], act[tidx])
    assert _same(ret, r[tidx]) and _same(rew[0], r[tidx])
    wrote_the_twin(env, tidx)
    env.close()
    # the tape kernel's two-waves build
    probe = G.SbrOSVec(1)
    n_big = probe.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS) + 100
    probe.close()
    idx = np.arange(n_big) % T.n
    tidx = torch.as_tensor(idx, device="cuda")
    env = _handle(G, T.x[idx], T.ctrl[idx], f32, reward)
    assert env.query(_capi.Q_ROLLOUT_WAVES) == 2
    ret, rew = env.rollout_actions(act[tidx][None].contiguous(), return_rewards=True)
    assert _same(ret, r[tidx]) and _same(rew[0], r[tidx])
    wrote_the_twin(env, tidx)
    env.close()


def test_done_call_runs_the_idle_phase_through_the_general_span(G, T):
    """The state-compared cases injected at the episode's last control interval (C_T, C_STEPS): the call runs that interval,
    settle and draw, and the idle phase through sbr_b5a_span - ceil(rows / 10) = 47 macro intervals of span / 47 with the reactor
    closed and Kla held, planned at 1 .. 27 steps and slaved (tests/test_plan_branches_cpu.py lists them).  Against the oracle's
    done call under the lockstep bar; done == 1 and C_QW to 1e-9 relative.
    Dropped (plan_cases.DONE_DROPPED): z1-aer-kla200 - its Snh = 0.3 is nitrified to -0.44 within the idle phase, the end state is
    outside the model's domain.
    Measured on MI355X: 63 cases, worst gate 2.3e-10 (knee41-anox-plain)."""
    from gym_sbr2_amd import _capi
    x, ctrl, action, names = T.at_last_call()
    outs = _step(G, x, ctrl, action)
    ora, oout = PC.oracle_call(x, ctrl, action)
    g = _lockstep(ora, oout, outs, np.ones(len(x), bool), "done call")
    c = _np(outs[5])
    assert oout[3].all() and np.all(c[_capi.C_DONE] == 1) and np.all(_np(outs[3]) == 1)
    assert np.abs(c[_capi.C_QW] / ora.envs["qw"] - 1).max() < 1e-9
    print("done call: %d cases, worst gate %.3e (%s)" % (len(x), g.max(), names[int(g.argmax())]))
