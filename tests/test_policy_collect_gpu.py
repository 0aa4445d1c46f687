"""sbr_collect_policy / SbrOSVec.collect_policy on the GPU: the fused policy collector against sbr_rollout_policy, which it repeats
with two more outputs.  Everything the two calls share is compared bit for bit on twin handles (same inputs, same net, same
noise key); obs_out is compared with the observation sbr_rollout_policy leaves in `obs` when the same calls are cut into one
launch per decision (the noise is keyed by the call count, so the cut changes no bit:
tests/test_policy_rollout_gpu.py::test_hold_and_split_launches); the flags are compared with what the handle says.

Inputs and nets are those of tests/test_policy_rollout_gpu.py (`_env`, `_policy`, inputs 202, net 13 = 2 x 32 tanh, net 51 =
1 x 64 relu, nets 23 / 24 as a population); the comparisons are bitwise and need no env to stay inside the model's domain.  300
envs where nothing else is said: one full workgroup and a partial wave of 44 lanes.

Which test runs which build of k_collect_policy<H, OCI, SCH, WAVES>:
  (32, no, 1, 1)  every test that is not named here
  (64, no, 1, 1)  test_other_builds[h64]
  (32, no, 0, 2)  test_other_builds[scheme0]
  (32, yes, 1, 1) test_other_builds[oci]
  (32, no, 1, 2)  test_two_waves_build
  the other seven builds are not run by any test."""
import ctypes as C

import numpy as np
import pytest
from gpu_common import STEPS, handle as _handle, inputs as _inputs, package, to_np as _np
from test_policy_rollout_gpu import _bound, _env, _policy, _same_state

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, HOLD, STD = 300, 8, (0.05, 0.3)
ROWS = -(-STEPS // HOLD)


@pytest.fixture(scope="module")
def G():
    return package()


def _raw(env, pol, n_steps, hold, obs, ret=None, acts=None, rew=None, obs_out=None, flags=None, noise_std=None, noise_seed=0):
    """sbr_collect_policy itself, on the caller's buffers (collect_policy always passes every output)."""
    from gym_sbr2_amd import _capi
    from gym_sbr2_amd.vec_env import _ptr
    s = pol.c_struct(env.device, noise_std=noise_std, noise_seed=noise_seed)
    _capi.check(env.lib.sbr_collect_policy(env._h, n_steps, hold, C.byref(s), _ptr(obs), _ptr(ret), _ptr(acts), _ptr(rew),
                                           _ptr(obs_out), _ptr(flags), env._stream()), env._h)


def _state(env):
    x, c = env.get_state()
    return x, c, env.obs.clone()


def _same(a, b):
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def _split(make, pol, n_steps, hold, rows, **noise):
    """A twin handle running sbr_rollout_policy in one launch per decision for the first `rows` decisions and the rest in one
    launch.  Returns the observation in force before each of those decisions, and the twin's end: actions, rewards, state.  (Its
    returns are per launch; the sum in call order since the reset is the state's C_RETURN row.)"""
    env = make()
    before, acts, rew = [], [], []
    at = 0
    for d in range(rows + 1):
        k = min(hold, n_steps - at) if d < rows else n_steps - at
        if k <= 0:
            break
        if d < rows:
            before.append(env.obs.clone())
        _, a, w = env.rollout_policy(pol, k, hold=hold, return_actions=True, return_rewards=True, **noise)
        acts.append(a); rew.append(w)
        at += k
    out = before, (torch.cat(acts), torch.cat(rew)) + _state(env)
    env.close()
    return out


@pytest.fixture(scope="module")
def ref(G):
    """Per noise setting, shared and left unchanged: handle A's sbr_rollout_policy and handle B's collect_policy over one episode
    of 463 calls, hold 8 (which does not divide 463), 300 envs, net 13."""
    inputs = _inputs(N, 202)
    pol = _policy(13, (32, 32))
    out = dict(inputs=inputs, pol=pol)
    for key, noise in (("plain", {}), ("noise", dict(noise_std=STD, noise_seed=7))):
        a_env, b_env = _env(G, N, inputs), _env(G, N, inputs)
        obs0 = a_env.obs.clone()
        ra = a_env.rollout_policy(pol, STEPS, hold=HOLD, return_actions=True, return_rewards=True, **noise)
        col = b_env.collect_policy(pol, STEPS, hold=HOLD, **noise)
        assert col.last_obs is b_env.obs
        out[key] = dict(noise=noise, obs0=obs0, a=tuple(ra) + _state(a_env), col=col, b=_state(b_env))
        a_env.close(); b_env.close()
    return out


@pytest.mark.parametrize("key", ["plain", "noise"])
def test_same_bits_as_rollout_policy(G, ref, key):
    """Check 1: the plant, every controller row, obs, returns, actions and rewards are sbr_rollout_policy's, with every output,
    with obs_out alone and with flags_out alone."""
    from gym_sbr2_amd import _capi
    r = ref[key]
    ret, acts, rew, x, c, obs = r["a"]
    col = r["col"]
    assert col.obs.shape == (ROWS, N, 18) and col.obs.dtype == torch.float32 and col.flags.shape == (ROWS, N) and col.flags.dtype == torch.uint8
    assert col.actions.shape == (ROWS, N, 2) and col.rewards.shape == (STEPS, N) and col.returns.shape == (N,)
    _same((x, c, obs), r["b"])
    for row in range(_capi.NCTRL):
        assert torch.equal(c[row], r["b"][1][row]), row
    assert torch.equal(col.returns, ret) and torch.equal(col.actions, acts) and torch.equal(col.rewards, rew)
    assert torch.equal(col.last_obs, obs) and bool((c[_capi.C_PLAN] == 0).all()) and bool((c[_capi.C_DONE] == 1).all())
    assert float(acts[..., 0].std()) > 1e-3 and float(acts[..., 1].std()) > 1e-3       # a policy, not a constant
    if key == "noise":
        assert not torch.equal(acts, ref["plain"]["a"][1])
    # the whole episode in one launch: every decision taken, the last one terminal
    assert bool((col.flags[:-1] == 1).all()) and bool((col.flags[-1] == 3).all())
    assert bool(col.taken.all()) and bool(col.ended[-1].all()) and not bool(col.ended[:-1].any())
    for which in ("obs_out", "flags"):
        env = _env(G, N, ref["inputs"])
        o = env.obs.clone()
        ret1 = torch.empty_like(ret); acts1 = torch.empty_like(acts); rew1 = torch.empty_like(rew)
        extra = torch.empty_like(col.obs) if which == "obs_out" else torch.empty_like(col.flags)
        _raw(env, ref["pol"], STEPS, HOLD, o, ret1, acts1, rew1, **{which: extra}, **r["noise"])
        x1, c1 = env.get_state()
        assert torch.equal(x1, x) and torch.equal(c1, c) and torch.equal(o, obs), which
        assert torch.equal(ret1, ret) and torch.equal(acts1, acts) and torch.equal(rew1, rew), which
        assert torch.equal(extra, col.obs if which == "obs_out" else col.flags), which
        env.close()


@pytest.mark.parametrize("key", ["plain", "noise"])
def test_obs_out_is_the_observation_in_force(G, ref, key):
    """Check 2: a twin handle runs sbr_rollout_policy in one launch of `hold` calls per decision; its obs buffer before launch d
    is obs_out[d], for every d."""
    r = ref[key]
    before, end = _split(lambda: _env(G, N, ref["inputs"]), ref["pol"], STEPS, HOLD, ROWS, **r["noise"])
    assert len(before) == ROWS
    # the cut changed no bit (but the twin's obs: every env is done in the end, and a done env's row stays as the launch before left it)
    _same(end[:4], r["a"][1:5])
    obs_out = r["col"].obs
    assert torch.equal(obs_out[0], r["obs0"])
    for d in range(ROWS):
        assert torch.equal(before[d], obs_out[d]), d
    assert not torch.equal(obs_out[1], obs_out[0]) and bool(torch.isfinite(obs_out).all())


def test_flags_and_skipped_rows(G, ref):
    """Check 3: 460 calls, then 16 calls with hold 5 from call 460 - the episode ends inside decision 0 - then a launch on the
    finished handle, then n_steps = 0."""
    pol = ref["pol"]
    env, twin = _env(G, N, ref["inputs"]), _env(G, N, ref["inputs"])
    c1 = env.collect_policy(pol, 460, hold=7)
    twin.rollout_policy(pol, 460, hold=7)
    assert c1.flags.shape == (66, N) and bool((c1.flags == 1).all())          # the short last decision (5 calls) like any other
    _same(_state(env), _state(twin))
    obs460 = env.obs.clone()
    c2 = env.collect_policy(pol, 16, hold=5)
    r2, a2, w2 = twin.rollout_policy(pol, 16, hold=5, return_actions=True, return_rewards=True)
    _same(_state(env), _state(twin))
    assert torch.equal(c2.returns, r2) and torch.equal(c2.actions, a2) and torch.equal(c2.rewards, w2)
    assert c2.flags.shape == (4, N) and bool((c2.flags[0] == 3).all()) and bool((c2.flags[1:] == 0).all())
    assert torch.equal(c2.obs[0], obs460) and bool((c2.obs[1:] == 0).all()) and bool((c2.actions[1:] == 0).all())
    assert bool((c2.actions[0] != 0).any()) and bool((c2.rewards[3:] == 0).all()) and bool((c2.rewards[:3] != 0).any())
    assert torch.equal(c2.last_obs, obs460) and torch.equal(env.obs, obs460)     # rows of done envs are left as they were
    # a third launch on the finished handle
    s2 = _state(env)
    c3 = env.collect_policy(pol, 7, hold=2)
    assert c3.flags.shape == (4, N) and bool((c3.flags == 0).all()) and bool((c3.obs == 0).all()) and bool((c3.actions == 0).all())
    assert bool((c3.returns == 0).all()) and bool((c3.rewards == 0).all())
    _same(_state(env), s2)
    # n_steps = 0: nothing is touched but returns
    o = env.obs.clone()
    ret = torch.full((N,), 7.0, dtype=torch.float64, device="cuda")
    acts = torch.full((2, N, 2), 5.0, device="cuda"); rew = torch.full((2, N), 5.0, dtype=torch.float64, device="cuda")
    rows = torch.full((2, N, 18), 5.0, device="cuda"); flags = torch.full((2, N), 9, dtype=torch.uint8, device="cuda")
    _raw(env, pol, 0, 3, o, ret, acts, rew, rows, flags)
    assert bool((ret == 0).all()) and bool((acts == 5).all()) and bool((rew == 5).all()) and bool((rows == 5).all()) and bool((flags == 9).all())
    assert torch.equal(o, obs460)
    _same(_state(env), s2)
    c0 = env.collect_policy(pol, 0)
    assert c0.obs.shape == (0, N, 18) and c0.flags.shape == (0, N) and c0.rewards.shape == (0, N) and bool((c0.returns == 0).all())
    # a fresh handle, n_steps = 0: the live state is left as well
    twin.reset(scenario=ref["inputs"][0], rnd=ref["inputs"][1])
    s0 = _state(twin)
    twin.collect_policy(pol, 0)
    _same(_state(twin), s0)
    env.close(); twin.close()


def test_some_envs_done_on_entry(G, ref):
    """Check 3, staggered: after 400 calls every third env is reset through reset(mask=...), then 63 calls end the others.  The
    collector then runs live and done envs side by side, in every wave."""
    from gym_sbr2_amd import _capi
    pol = ref["pol"]
    scen, rnd = ref["inputs"]
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    live = torch.from_numpy(mask.astype(bool)).cuda()

    def staggered():
        env = _env(G, N, ref["inputs"])
        env.rollout_policy(pol, 400, hold=HOLD)
        env.reset(scenario=scen, rnd=rnd, mask=mask)
        env.rollout_policy(pol, 63, hold=HOLD)
        return env

    env, twin = staggered(), staggered()
    done = env.ctrl_row(_capi.C_DONE) == 1
    assert torch.equal(done, ~live)
    o_in = env.obs.clone()
    col = env.collect_policy(pol, 10, hold=3, noise_std=STD, noise_seed=3)
    r, a, w = twin.rollout_policy(pol, 10, hold=3, noise_std=STD, noise_seed=3, return_actions=True, return_rewards=True)
    _same(_state(env), _state(twin))
    assert torch.equal(col.returns, r) and torch.equal(col.actions, a) and torch.equal(col.rewards, w)
    assert col.flags.shape == (4, N) and bool((col.flags[:, live] == 1).all()) and bool((col.flags[:, ~live] == 0).all())
    assert bool((col.obs[:, ~live] == 0).all()) and bool((col.actions[:, ~live] == 0).all())
    assert torch.equal(col.obs[0, live], o_in[live]) and bool((col.obs[1:, live].abs().sum(-1) > 0).all())
    assert torch.equal(col.last_obs[~live], o_in[~live]) and not torch.equal(col.last_obs[live], o_in[live])
    env.close(); twin.close()


def test_an_envs_result_does_not_depend_on_the_batch_around_it(G):
    """Check 4: a population built of two nets, 256 envs per member, on 1 024 envs (members net 23, net 24, net 23, net 24), against a
    512-env handle cut at global id 256 - across a member boundary - and a two-rank shard."""
    from gym_sbr2_amd import MlpPolicy, ShardedSbrOS
    n, calls, hold = 1024, 60, 7
    inputs = _inputs(n, 202)
    p0, p1 = _policy(23, (32, 32)), _policy(24, (32, 32))
    pop = MlpPolicy.stack([p0, p1, p0, p1], envs_per_policy=256)
    noise = dict(noise_std=STD, noise_seed=11)
    big = _env(G, n, inputs)
    obs0 = big.obs.clone()
    col = big.collect_policy(pop, calls, hold=hold, **noise)
    assert not torch.equal(col.actions[:, :256], col.actions[:, 256:512])

    def check(part, lo, hi, got):
        _same_state(big, part, cols=slice(lo, hi))
        assert torch.equal(got.obs, col.obs[:, lo:hi]) and torch.equal(got.flags, col.flags[:, lo:hi])
        assert torch.equal(got.actions, col.actions[:, lo:hi]) and torch.equal(got.rewards, col.rewards[:, lo:hi])
        assert torch.equal(got.returns, col.returns[lo:hi]) and torch.equal(got.last_obs, col.last_obs[lo:hi])

    part = _env(G, 512, inputs, first=256)
    check(part, 256, 768, part.collect_policy(pop, calls, hold=hold, obs=obs0[256:768].clone(), **noise))
    part.close()
    for rank in (0, 1):
        sh = ShardedSbrOS(n, rank=rank, world=2, device=0)
        assert (sh.start, sh.stop) == (512 * rank, 512 * rank + 512)
        sh.env.reset(scenario=inputs[0][sh.start:sh.stop], rnd=inputs[1][sh.start:sh.stop])
        check(sh.env, sh.start, sh.stop, sh.collect_policy(pop, calls, hold=hold, **noise))
        sh.close()
    big.close()


def _against_rollout(make, pol, n_steps, hold, rows=3):
    """Check 5 for one config: collect_policy on one handle, sbr_rollout_policy on its twin, cut into one launch per decision for
    the first `rows` decisions (check 2 on those rows) - outputs and handle bit for bit."""
    from gym_sbr2_amd import _capi
    env = make()
    obs0 = env.obs.clone()
    col = env.collect_policy(pol, n_steps, hold=hold)
    before, (acts, rew, x, c, obs) = _split(make, pol, n_steps, hold, rows)
    xe, ce, oe = _state(env)
    assert torch.equal(xe, x) and torch.equal(ce, c)
    live = c[_capi.C_DONE] == 0          # a done env's row of obs stays as the launch BEFORE left it, and the twin had several
    assert torch.equal(oe[live], obs[live]) and torch.equal(oe[~live], obs0[~live])
    assert torch.equal(col.returns, c[_capi.C_RETURN]) and torch.equal(col.actions, acts) and torch.equal(col.rewards, rew)
    assert len(before) == rows and torch.equal(before[0], obs0)
    for d in range(rows):
        assert torch.equal(before[d], col.obs[d]), d
    assert not torch.equal(col.obs[1], col.obs[0])
    assert float(acts[..., 0].std()) > 1e-3 and float(acts[..., 1].std()) > 1e-3
    env.close()
    return col


@pytest.mark.parametrize("build", ["h64", "scheme0", "oci"])
def test_other_builds(G, build):
    from gym_sbr2_amd import _capi
    if build == "h64":                     # a 1 x 64 relu net whose units >= 32 carry weight, 256 envs
        n = 256
        with pytest.warns(RuntimeWarning, match="64-wide"):
            pol = _policy(51, (64,), "relu")
        assert pol.width == 64 and np.any(pol.block[0, 18 * 32:18 * 64] != 0)
        scheme, reward = 1, "eqi_oci"
    else:
        n, pol = N, _policy(13, (32, 32))
        scheme, reward = (0, "eqi_oci") if build == "scheme0" else (1, "oci")
    inputs = _inputs(n, 202)

    def make():
        env = _handle(G, n, scheme, reward)
        env.reset(scenario=inputs[0], rnd=inputs[1])
        return env

    col = _against_rollout(make, pol, STEPS, HOLD)
    assert bool((col.flags[:-1] == 1).all()) and bool((col.flags[-1] == 3).all())
    assert _capi.REWARD_KINDS[reward] == (2 if build == "oci" else 0)


def test_two_waves_build(G):
    """98 624 envs (a ragged last workgroup) over 40 calls, which cross the first phase boundary; hold 8."""
    from gym_sbr2_amd import _capi
    n = 98304 + 320
    inputs = _inputs(n, 505)
    pol = _policy(13, (32, 32))

    def make():
        env = _env(G, n, inputs)
        assert env.query(_capi.Q_ROLLOUT_WAVES) == 2
        return env

    col = _against_rollout(make, pol, 40, 8)
    assert col.flags.shape == (5, n) and bool((col.flags == 1).all())


def test_the_rows_are_usable(ref):
    """Check 6: without noise, the net applied in float64 by torch to obs_out reproduces `actions`, each within the bound the
    lockstep test of sbr_rollout_policy derives for a float32 evaluation (tests/test_policy_rollout_gpu.py::_bound)."""
    pol, col = ref["pol"], ref["plain"]["col"]
    assert bool(col.taken.all())
    h = col.obs.reshape(-1, 18).to(torch.float64)
    for k, (w, b) in enumerate(pol.layers):
        h = torch.nn.functional.linear(h, torch.from_numpy(w).cuda().to(torch.float64), torch.from_numpy(b).cuda().to(torch.float64))
        h = torch.tanh(h)                                   # the hidden activation, and the squash behind the last layer
    mean = torch.from_numpy(pol.act_bias).cuda().to(torch.float64) + torch.from_numpy(pol.act_scale).cuda().to(torch.float64) * h
    want, bound = _bound(pol, _np(col.obs).reshape(-1, 18))
    assert np.abs(_np(mean) - want).max() <= 1e-12          # torch's forward is the checker's net
    ratio = np.abs(_np(col.actions).reshape(-1, 2).astype(np.float64) - _np(mean)) / bound
    print("worst |d a| / bound over %d actions: %.4f" % (ratio.size, ratio.max()))
    assert ratio.max() <= 1.0


def test_graph_capture_and_float64_handle(G, ref):
    """Nothing is allocated by the call: it is captured into a graph; and obs=None on a float64 handle is rollout_policy's."""
    pol = ref["pol"]
    env = _env(G, N, ref["inputs"])
    x0, c0 = env.get_state()
    o0 = env.obs.clone()
    o = o0.clone()
    eager = env.collect_policy(pol, 20, hold=3, obs=o)
    se = env.get_state()
    oe = o.clone()
    env.set_state(x0, c0)
    o.copy_(o0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            cap = env.collect_policy(pol, 20, hold=3, obs=o)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    _same(env.get_state(), se)
    assert torch.equal(o, oe) and not torch.equal(oe, o0)
    _same(tuple(cap)[:5], tuple(eager)[:5])
    env.close()
    e64, e32 = _env(G, N, ref["inputs"], out_dtype=torch.float64), _env(G, N, ref["inputs"])
    assert e64.obs.dtype == torch.float64
    c64, c32 = e64.collect_policy(pol, 30, hold=4), e32.collect_policy(pol, 30, hold=4)
    _same(tuple(c64), tuple(c32))
    assert c64.last_obs.dtype == torch.float32 and torch.equal(e64.obs, e32.obs.to(torch.float64))
    e64.close(); e32.close()
