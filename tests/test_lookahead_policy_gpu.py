"""sbr_lookahead_policy / SbrOSVec.lookahead_policy on the GPU: K closed-loop rollouts of the caller's MLP per env from the live
state, the handle untouched.

Three checkers, all existing entry points that earlier test files pin:
  * `rollout_policy` on a CLONE - a second N-env handle with the same first_env_id, given the live handle's influent, state and
    observation: without noise every branch, and under noise branch 0, is that rollout bit for bit (same inlined device
    functions, -ffp-contract=off);
  * `lookahead` / `lookahead_end` fed this call's own actions_out: returns, rewards, winners and end rows bit for bit;
  * the numpy Philox4x32-10 + Box-Muller of tests/gpu_common.py (anchored here to the device's sbr_draw_normals, as in
    tests/test_mppi_gpu.py) for the noise word.
Comparisons are torch.equal with NaN equal to NaN (`_same`).

Which test runs which build of k_lookahead_policy<H, OCI, SCH, WAVES> ((SCH, WAVES) = (1, 1) up to 98 304 BRANCHES, (1, 2) above,
(0, 2) for scheme 0; H from the net, OCI from reward "oci"):
  (32, no, 1, 1)   every test below that is not named here
  (64, no, 1, 1)   test_other_builds[h64]
  (32, no, 0, 2)   test_other_builds[scheme-0]
  (32, yes, 1, 1)  test_other_builds[oci-episode-end]
  (32, no, 1, 2)   test_other_builds[two-waves-by-branches]
test_other_builds[relu-none] (relu, squash "none") and [float64-actions] run (32, no, 1, 1) through its other branches.
Not run by any test: (64, no, 1, 2), (64, no, 0, 2), (32, yes, 1, 2), (32, yes, 0, 2) and the three (64, yes, ...) builds; they
differ from the ones above in template arguments the kernel only passes on to the shared device functions."""
import ctypes as C

import numpy as np
import pytest
from gpu_common import (STEPS, host_best as _host_best, live as _live, net as _net, normal_pair as _normal_pair, package,
                        same as _same)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOW, HIGH = (0.0, 0.0), (2.5, 15.0)
STD = (0.25, 2.0)                   # float32-representable: the std the device multiplies by is the one written here


@pytest.fixture(scope="module")
def G():
    return package()


def _clone(G, env, lo=0, hi=None, **kw):
    """(a second handle holding the envs lo .. hi - 1 of `env` - same global ids, influent and state -, their float32 obs)."""
    hi = env.num_envs if hi is None else hi
    b = G.SbrOSVec(hi - lo, first_env_id=env.first_env_id + lo, **kw)
    b.reset(influent=env.influent().T[lo:hi].contiguous())
    x, c = env.get_state()
    b.set_state(x[:, lo:hi].contiguous(), c[:, lo:hi].contiguous())
    return b, env.obs[lo:hi].to(torch.float32).clone()


def _policy(seed=13, widths=(32, 32), activation="tanh", squash="tanh"):
    from gym_sbr2_amd import MlpPolicy
    return MlpPolicy(_net(seed, widths), activation=activation, squash=squash, low=LOW, high=HIGH)


def _state_rows(env):
    x, c = env.get_state()
    return x, c, env.obs.clone()


def _untouched(env, before):
    from gym_sbr2_amd import _capi
    x0, c0, o0 = before
    x1, c1 = env.get_state()
    assert torch.equal(x0, x1) and _same(o0, env.obs)
    for row in range(_capi.NCTRL):                     # all 14 + 25 rows: the plan, the return and the call count included
        assert torch.equal(c0[row], c1[row]), row


def _all(env, pol, k, n_steps, hold, **kw):
    """lookahead_policy with everything asked for: (ret, rew, bi, br, acts, obs_end, state_end, done_end), shapes checked."""
    out = env.lookahead_policy(pol, k, n_steps, hold=hold, return_rewards=True, return_best=True, return_actions=True,
                               return_end=True, **kw)
    ret, rew, bi, br, acts, oe, se, de = out
    n, rows = env.num_envs, -(-n_steps // hold)
    assert ret.shape == (n, k) and ret.dtype == torch.float64 and rew.shape == (n_steps, n, k) and rew.dtype == torch.float64
    assert bi.shape == (n,) and bi.dtype == torch.int32 and br.shape == (n,) and br.dtype == torch.float64
    assert acts.shape == (rows, n, k, 2) and acts.dtype == torch.float32
    assert oe.shape == (n, k, 18) and oe.dtype == torch.float32 and se.shape == (n, k, 15) and se.dtype == torch.float32
    assert de.shape == (n, k) and de.dtype == torch.bool
    return out


def _against_lookahead(env, out, n_steps, hold):
    """`lookahead_end` fed the call's own actions_out gives the call's returns, rewards, winners and end rows."""
    ret, rew, bi, br, acts, oe, se, de = out
    tape = env.lookahead_end(acts, n_steps=n_steps, hold=hold, return_rewards=True, return_best=True)
    for name, u, v in zip(("returns", "rewards", "best_index", "best_return", "obs_end", "state_end", "done_end"),
                          (ret, rew, bi, br, oe, se, de), tape):
        assert _same(u, v), name
    assert bool((oe[de] == 0).all()) and bool((se[de] == 0).all())


def _against_clone(G, env, pol, out, n_steps, hold, branches=None, **kw):
    """Every branch in `branches` (default: all) equals `rollout_policy` on a clone of the handle: returns, rewards, actions."""
    noise = {k: kw.pop(k) for k in ("noise_std", "noise_seed") if k in kw}
    clone, obs = _clone(G, env, **kw)
    ret_c, acts_c, rew_c = clone.rollout_policy(pol, n_steps, hold=hold, obs=obs, return_actions=True, return_rewards=True, **noise)
    ret, rew, acts = out[0], out[1], out[4]
    for k in (range(ret.shape[1]) if branches is None else branches):
        assert _same(ret[:, k], ret_c), k
        assert _same(rew[:, :, k], rew_c), k
        assert _same(acts[:, :, k], acts_c), k
    clone.close()
    return ret_c, acts_c, rew_c


def _noise_bound_holds(acts, mean, counter, gid, seed):
    """acts, mean [rows, n, k, 2] (mean float64, or broadcastable); counter [rows]; gid [n].  For every (row, env, k, c), with z
    the numpy normal of block (counter, 3 + 256 k, g): |a - (m + std z)| <= 2^-24 |m + std z| + 1e-12 std - one float32 rounding,
    plus the device's double log / sqrt / sincos as bounded in tests/test_mppi_gpu.py.  Returns the worst ratio to the bound."""
    a = acts.double().cpu().numpy()
    k = a.shape[2]
    z = np.stack(_normal_pair(np.asarray(counter)[:, None, None], 3 + 256 * np.arange(k)[None, None, :], np.asarray(gid)[None, :, None],
                              seed), axis=-1)
    std = np.asarray(STD, dtype=np.float64)
    want = mean + std * z
    ratio = np.abs(a - want) / (2.0 ** -24 * np.abs(want) + 1e-12 * std)
    print("worst |a - (m + std z)| / bound: %.3g;  max |std z| %.3g" % (ratio.max(), np.abs(std * z).max()))
    return float(ratio.max()), z


# ------------------------------------------------------------------ 1
def test_the_handle_and_obs_are_untouched(G):
    """N = 5, K = 3, noise on: 15 branches in one wave, eight-scenario mix.  The handle stands after 30 step() calls; 40 calls
    under hold = 2 cross the double-step call 51."""
    n, k, n_steps, hold = 5, 3, 40, 2
    a_env, twin = _live(G, n, 30, seed=11), _live(G, n, 30, seed=11)
    pol = _policy()
    before = _state_rows(a_env)
    obs = a_env.obs.clone()
    ret, rew = a_env.lookahead_policy(pol, k, n_steps, hold=hold, noise_std=STD, noise_seed=5, return_rewards=True)
    ret2 = a_env.lookahead_policy(pol, k, n_steps, hold=hold, obs=obs, noise_std=STD, noise_seed=5)     # obs given = obs=None
    _untouched(a_env, before)
    assert torch.equal(obs, before[2]) and _same(ret, ret2)
    assert len(torch.unique(ret)) > 1 and bool((rew != 0).any())       # not a comparison of zeros
    act = torch.tensor([1.0, 5.0], device="cuda").expand(n, 2).contiguous()
    outs_a = [t.clone() for t in a_env.step(act)]
    outs_t = twin.step(act)
    for u, v in zip(outs_a, outs_t):
        assert torch.equal(u, v)
    (xa, ca), (xt, ct) = a_env.get_state(), twin.get_state()
    assert torch.equal(xa, xt) and torch.equal(ca, ct)
    a_env.close(); twin.close()


# ------------------------------------------------------------------ 2
@pytest.mark.parametrize("calls", [30, 440])
def test_without_noise_every_branch_is_rollout_policy_on_a_clone(G, calls):
    """Noise 0, N = 5, K = 3.  At call 440 of 463 the window runs past the episode end: every branch finishes with its 23rd call;
    23 step() calls later the handle is done on entry, and a branch done on entry gives zeros and done_end = 1."""
    n, k, n_steps, hold = 5, 3, 40, 2
    a_env = _live(G, n, calls, seed=21)
    pol = _policy()
    before = _state_rows(a_env)
    out = _all(a_env, pol, k, n_steps, hold)
    ret_c, acts_c, rew_c = _against_clone(G, a_env, pol, out, n_steps, hold)
    _against_lookahead(a_env, out, n_steps, hold)
    _untouched(a_env, before)
    assert bool((rew_c != 0).any()) and float(acts_c[..., 0].std()) > 1e-3
    if calls == 440:
        live = STEPS - calls
        rew, acts, de = out[1], out[4], out[7]
        assert bool(de.all()) and bool((rew[live:] == 0).all()) and bool((rew[:live] != 0).any())
        assert bool((acts[-(-live // hold):] == 0).all()) and bool((acts[(live - 1) // hold] != 0).any())
        act = torch.tensor([1.0, 5.0], device="cuda").expand(n, 2).contiguous()
        for _ in range(live):
            a_env.step(act)
        assert bool(a_env.done.bool().all())
        out = _all(a_env, pol, k, 6, hold, noise_std=STD)
        for t in out[:2] + out[3:7]:
            assert bool((t == 0).all())
        assert bool((out[2] == 0).all()) and bool(out[7].all())
    else:
        assert not bool(out[7].any())
    a_env.close()


# ------------------------------------------------------------------ 3
def test_branch_0_under_noise_and_keep_mean(G):
    n, k, n_steps, hold = 5, 3, 40, 2
    a_env = _live(G, n, 30, seed=31)
    pol = _policy()
    noisy = _all(a_env, pol, k, n_steps, hold, noise_std=STD, noise_seed=77)
    _against_clone(G, a_env, pol, noisy, n_steps, hold, branches=[0], noise_std=STD, noise_seed=77)
    kept = _all(a_env, pol, k, n_steps, hold, noise_std=STD, noise_seed=77, keep_mean=True)
    _against_clone(G, a_env, pol, kept, n_steps, hold, branches=[0])
    # returns [N, K], rewards [n_steps, N, K], actions [R, N, K, 2]: branches k >= 1 are what they were
    assert _same(noisy[0][:, 1:], kept[0][:, 1:]) and _same(noisy[1][:, :, 1:], kept[1][:, :, 1:])
    assert _same(noisy[4][:, :, 1:], kept[4][:, :, 1:])
    assert not torch.equal(noisy[4][:, :, 0], kept[4][:, :, 0])        # ... and branch 0 did change
    assert not torch.equal(noisy[4][:, :, 1], noisy[4][:, :, 2])       # the branches draw noise of their own
    a_env.close()


# ------------------------------------------------------------------ 4
def test_chain_to_the_tape_kernel_across_wavefronts_and_the_workgroup_boundary(G):
    """N = 4, K = 70: 280 branches - an env's branches straddle wavefronts and the 256-lane workgroup boundary.  Env 3: NaN
    ammonia injected through set_state (NaN observations, actions and returns: index 0, NaN)."""
    n, k, n_steps, hold = 4, 70, 12, 2
    a_env = _live(G, n, 60, seed=41)                   # in the aerated phase: the returns depend on the set-points
    x, c = a_env.get_state()
    x[10, 3] = float("nan")
    a_env.set_state(x, c)
    obs = a_env.obs.clone()
    obs[3, 2] = float("nan")
    pol = _policy()
    out = _all(a_env, pol, k, n_steps, hold, obs=obs, noise_std=STD, noise_seed=9)
    _against_lookahead(a_env, out, n_steps, hold)
    ret, bi, br = out[0], out[2], out[3]
    idx, val = _host_best(ret)
    assert np.array_equal(bi.cpu().numpy(), idx) and np.array_equal(br.cpu().numpy(), val, equal_nan=True)
    print("env 3 (NaN ammonia): %d of %d returns NaN, winner %d" % (int(torch.isnan(ret[3]).sum()), k, int(bi[3])))
    assert bool(torch.isfinite(ret[:3]).all()) and all(len(torch.unique(ret[i])) > 1 for i in range(3))
    a_env.close()


# ------------------------------------------------------------------ 5
def test_the_noise_is_what_the_header_says(G):
    """A policy without a hidden layer and with zero weights: the mean m is a constant, read from a noise-0 run.  Ids straddling
    2^32, N = 6, K = 5, three decisions under hold = 2: counter = the branch's calls since reset (2 + r hold), stream word
    3 + 256 k, key noise_seed.  A wrong counter word is off by O(std).  The same bits on a handle of 3 of those envs with K = 2."""
    from gym_sbr2_amd import MlpPolicy
    n, k, hold, rows, first, seed, steps0 = 6, 5, 2, 3, 2 ** 32 - 3, (5 << 32) + 1234, 2
    env = _live(G, n, steps0, seed=51, first=first)
    gid = first + np.arange(n)
    # the numpy generator first, against the device's own stream-0 draws (sbr_draw_normals: pair p of an env = block (p, 0, id))
    z_dev = env.draw_normals(seed).cpu().numpy()
    z0, z1 = _normal_pair(np.arange(24)[None, :], 0, gid[:, None], seed)
    assert np.abs(z_dev[:, 0::2] - z0).max() <= 1e-12 and np.abs(z_dev[:, 1::2] - z1).max() <= 1e-12
    pol = MlpPolicy([(np.zeros((2, 18)), np.array([0.3, -0.2]))], squash="tanh", low=LOW, high=HIGH)
    mean = env.lookahead_policy(pol, k, rows * hold, hold=hold, return_actions=True)[1]
    m = mean[0, 0, 0].double().cpu().numpy()
    assert bool((mean == mean[0, 0, 0]).all()) and 0.5 < m[0] < 2.0 and 4.0 < m[1] < 10.0
    acts = env.lookahead_policy(pol, k, rows * hold, hold=hold, noise_std=STD, noise_seed=seed, return_actions=True)[1]
    worst, z = _noise_bound_holds(acts, m, steps0 + hold * np.arange(rows), gid, seed)
    assert worst <= 1.0
    assert np.abs(z).max() > 1.0 and len(np.unique(z)) == z.size       # every (row, env, k, c) has a draw of its own
    part = _live(G, 3, steps0, seed=52, first=first + 3)
    acts_p = part.lookahead_policy(pol, 2, rows * hold, hold=hold, noise_std=STD, noise_seed=seed, return_actions=True)[1]
    assert torch.equal(acts_p, acts[:, 3:, :2])
    env.close(); part.close()


# ------------------------------------------------------------------ 6
def test_a_later_decision_reads_the_branchs_own_observation(G):
    """Noise on, K = 3, two decisions.  The observation before decision 1 is what `lookahead_end` reports for decision 0's
    actions; a scratch N K handle evaluates the net on it (rollout_policy, one call, noise 0: the exact float32 means)."""
    n, k, hold, seed, calls = 5, 3, 3, 99, 60
    a_env = _live(G, n, calls, seed=61)
    pol = _policy()
    acts = a_env.lookahead_policy(pol, k, 2 * hold, hold=hold, noise_std=STD, noise_seed=seed, return_actions=True)[1]
    obs_end, _, done_end = a_env.lookahead_end(acts[:1], n_steps=hold, hold=hold)[1:]
    assert not bool(done_end.any())
    scratch = G.SbrOSVec(n * k)
    scratch.reset()
    means = scratch.rollout_policy(pol, 1, obs=obs_end.reshape(-1, 18).clone(), return_actions=True)[1].reshape(1, n, k, 2)
    worst, _ = _noise_bound_holds(acts[1:], means.double().cpu().numpy(), [calls + hold], np.arange(n), seed)
    assert worst <= 1.0
    # the branches of an env stand at different observations, and their means differ: two branches have the same mean only
    # where they ended at the same observation, bit for bit (a kernel that read the env's shared row again would give K equal
    # means under K different observations).  Two different set-points CAN leave the same plant: while both PIDs sit at a
    # limit of Kla and EC the plant does not see the set-point - on the MI355X env 4 of this case ends branches 1 and 2 at
    # identical observations (means 1.1415067, 3.42499 twice; its branch 0 and all branches of envs 0 .. 3 differ)
    print("row-1 means:\n%s\nobservation components that differ between the branches of an env: %s"
          % (means[0].cpu().numpy(), [int((obs_end[i] != obs_end[i, :1]).any(dim=0).sum()) for i in range(n)]))
    for i in range(n):
        for p in range(k):
            for q in range(p + 1, k):
                same_obs = torch.equal(obs_end[i, p], obs_end[i, q])
                assert same_obs == torch.equal(means[0, i, p], means[0, i, q]), (i, p, q)
        assert len(torch.unique(obs_end[i], dim=0)) >= 2, i                # no env whose branches all coincide
    # ... and decision 0 is the mean on the env's own row of obs, shared by its branches
    mean0 = scratch.rollout_policy(pol, 1, obs=a_env.obs.repeat_interleave(k, dim=0), return_actions=True)[1].reshape(1, n, k, 2)
    worst0, _ = _noise_bound_holds(acts[:1], mean0.double().cpu().numpy(), [calls], np.arange(n), seed)
    assert worst0 <= 1.0
    a_env.close(); scratch.close()


# ------------------------------------------------------------------ 7
def test_population_boundary(G):
    """Two different nets, envs_per_policy = 256, N = 512, K = 5, noise 0: the boundary falls at branch 1280, a multiple of the
    workgroup size.  Envs 0 .. 255 equal a run under net 0 alone, envs 256 .. 511 one under net 1 alone on a handle with
    first_env_id = 256."""
    from gym_sbr2_amd import MlpPolicy
    n, k, n_steps, hold = 512, 5, 12, 2
    a_env = _live(G, n, 30, seed=71)
    p0, p1 = _policy(23), _policy(24)
    pop = MlpPolicy.stack([p0, p1], envs_per_policy=256)
    out = a_env.lookahead_policy(pop, k, n_steps, hold=hold, return_rewards=True, return_actions=True)
    lo = a_env.lookahead_policy(p0, k, n_steps, hold=hold, return_rewards=True, return_actions=True)
    part, obs = _clone(G, a_env, 256, 512)
    assert part.first_env_id == 256
    hi = part.lookahead_policy(p1, k, n_steps, hold=hold, obs=obs, return_rewards=True, return_actions=True)
    assert _same(out[0][:256], lo[0][:256]) and _same(out[1][:, :256], lo[1][:, :256]) and _same(out[2][:, :256], lo[2][:, :256])
    assert _same(out[0][256:], hi[0]) and _same(out[1][:, 256:], hi[1]) and _same(out[2][:, 256:], hi[2])
    assert not torch.equal(out[2][:, 256:], lo[2][:, 256:])            # the second net is another net
    # ... and a population member under noise is keyed by the env's global id: the shard draws what the whole handle draws
    out_n = a_env.lookahead_policy(pop, k, n_steps, hold=hold, noise_std=STD, noise_seed=3, return_actions=True)
    hi_n = part.lookahead_policy(pop, k, n_steps, hold=hold, obs=obs, noise_std=STD, noise_seed=3, return_actions=True)
    assert _same(out_n[0][256:], hi_n[0]) and _same(out_n[1][:, 256:], hi_n[1])
    a_env.close(); part.close()


# ------------------------------------------------------------------ 8
@pytest.mark.parametrize("build", ["h64", "scheme-0", "oci-episode-end", "relu-none", "float64-actions", "two-waves-by-branches"])
def test_other_builds(G, build):
    from gym_sbr2_amd import _capi
    kw, n, k, calls, n_steps, hold, pol = {}, 37, 2, 30, 40, 2, None
    if build == "h64":
        with pytest.warns(RuntimeWarning, match="64-wide"):
            pol = _policy(53, (64, 64))
        l2 = 18 * 64 + 64
        w2 = pol.block[0, l2:l2 + 64 * 64].reshape(64, 64)
        assert pol.width == 64 and np.any(w2[32:] != 0) and np.any(w2[:, 32:] != 0)      # units >= 32 carry weight
    elif build == "scheme-0":
        cfg = _capi.default_config()
        cfg.scheme = 0
        kw = {"config": cfg}
    elif build == "oci-episode-end":
        kw, n, k, calls = {"reward": "oci"}, 6, 3, 440
    elif build == "relu-none":
        pol = _policy(42, (32, 32), activation="relu", squash="none")
    elif build == "float64-actions":
        kw = {"action_dtype": torch.float64}
    else:
        # 1541 x 64 = 98 624 branches: above the 98 304 lanes the one-wave build serves, the handle's 1541 envs far below
        n, k, calls, n_steps, hold = 1541, 64, 25, 4, 2
    pol = pol or _policy()
    a_env = _live(G, n, calls, seed=81, **kw)
    if build == "two-waves-by-branches":
        assert a_env.query(_capi.Q_ROLLOUT_WAVES) == 1 and n * k > a_env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS)
    before = _state_rows(a_env)
    noisy = _all(a_env, pol, k, n_steps, hold, noise_std=STD, noise_seed=8)
    _against_lookahead(a_env, noisy, n_steps, hold)
    assert bool((noisy[1] != 0).any()) and len(torch.unique(noisy[0])) > 1
    if build != "two-waves-by-branches":
        plain = _all(a_env, pol, k, n_steps, hold)
        _against_lookahead(a_env, plain, n_steps, hold)
        _against_clone(G, a_env, pol, plain, n_steps, hold, **kw)
    if build == "oci-episode-end":
        live = STEPS - calls
        assert bool((noisy[1][live:] == 0).all()) and bool((noisy[1][live - 1] != 0).any()) and bool(noisy[7].all())
    if build == "float64-actions":
        assert noisy[4].dtype == torch.float32 and a_env.action_dtype == torch.float64
    _untouched(a_env, before)
    a_env.close()


# ------------------------------------------------------------------ 9
def test_refusals_and_n_steps_zero_on_a_live_handle(G):
    from gym_sbr2_amd import SbrEnv2Vec, _capi
    lib = _capi.load()
    n, k, n_steps = 128, 3, 4
    env = _live(G, n, 2, seed=91)
    pol = _policy()
    before = _state_rows(env)
    obs = env.obs.clone()
    ret = torch.full((n, k), 7.0, dtype=torch.float64, device="cuda")
    rew = torch.full((n_steps, n, k), 7.0, dtype=torch.float64, device="cuda")
    bi = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    br = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    acts = torch.full((n_steps, n, k, 2), 7.0, device="cuda")
    oe, se = torch.full((n, k, 18), 7.0, device="cuda"), torch.full((n, k, 15), 7.0, device="cuda")
    de = torch.full((n, k), 7, dtype=torch.uint8, device="cuda")
    filled = (ret, rew, bi, br, acts, oe, se, de)

    def call(why, n_steps=n_steps, hold=1, fanout=k, policy=True, keep_mean=0, obs_t=obs, returns=ret, ends=(None, None, None), **f):
        s = pol.c_struct(env.device)
        for name, v in f.items():
            setattr(s, name, v)
        p = lambda t: None if t is None else t.data_ptr()                                      # noqa: E731
        rc = lib.sbr_lookahead_policy(env._h, n_steps, hold, fanout, C.byref(s) if policy else None, keep_mean, p(obs_t), p(returns),
                                      rew.data_ptr(), bi.data_ptr(), br.data_ptr(), acts.data_ptr(), *[p(t) for t in ends], None)
        msg = lib.sbr_last_error(env._h)
        assert rc == -1 and b"sbr_lookahead_policy" in msg and why in msg, (why, rc, msg)

    call(b"NULL policy", policy=False)
    call(b"NULL obs", obs_t=None)
    call(b"NULL params", params=None)
    call(b"n_hidden", n_hidden=3)
    call(b"width", width=48)
    call(b"activation", activation=2)
    call(b"squash", squash=-1)
    call(b"n_policies", n_policies=0)
    call(b"noise_std", noise_std=(C.c_float * 2)(0.1, -0.1))
    call(b"noise_std", noise_std=(C.c_float * 2)(float("nan"), 0.0))
    call(b"envs_per_policy", n_policies=2, envs_per_policy=100)
    call(b"n_steps", n_steps=-1)
    call(b"hold", hold=0)
    call(b"fanout", fanout=0)
    call(b"2^24", fanout=2 ** 24 + 1)
    call(b"2^31", fanout=2 ** 24)                      # 128 x 2^24 = 2^31 branches
    call(b"keep_mean", keep_mean=2)
    call(b"keep_mean", keep_mean=-1)
    call(b"give returns", returns=None)
    call(b"n_steps = 0", n_steps=0, ends=(oe, None, None))
    call(b"n_steps = 0", n_steps=0, ends=(None, se, None))
    call(b"n_steps = 0", n_steps=0, ends=(None, None, de))
    with pytest.raises(ValueError):
        env.lookahead_policy(pol, k, n_steps, hold=0)
    with pytest.raises(ValueError):
        env.lookahead_policy(pol, 0, n_steps)
    with pytest.raises(ValueError):
        env.lookahead_policy(pol, 2 ** 24 + 1, n_steps)
    with pytest.raises(ValueError):
        env.lookahead_policy(pol, k, n_steps, obs=torch.zeros(n - 1, 18, device="cuda"))
    with pytest.raises(_capi.SbrError, match="sbr_lookahead_policy"):
        env.lookahead_policy(pol, k, n_steps, noise_std=(-1.0, 0.0))
    with pytest.raises(_capi.SbrError, match="n_steps = 0"):
        env.lookahead_policy(pol, k, 0, return_end=True)
    with pytest.raises(NotImplementedError):
        SbrEnv2Vec.lookahead_policy(None, pol, k, n_steps)
    torch.cuda.synchronize()
    _untouched(env, before)
    assert torch.equal(obs, before[2])
    for t in filled:
        assert bool((t == 7).all())
    # n_steps = 0: zero returns, winner index 0 and winner return 0; nothing else written, nothing read
    r0, b0, v0 = env.lookahead_policy(pol, k, 0, return_best=True)
    assert r0.shape == (n, k) and bool((r0 == 0).all()) and bool((b0 == 0).all()) and bool((v0 == 0).all())
    r0, w0, a0 = env.lookahead_policy(pol, k, 0, return_rewards=True, return_actions=True)
    assert w0.shape == (0, n, k) and a0.shape == (0, n, k, 2)
    _untouched(env, before)
    env.close()


def test_refusal_of_envs_past_the_population(G):
    """The one population refusal that needs a handle with more envs than the population covers."""
    from gym_sbr2_amd import MlpPolicy, _capi
    env = _live(G, 768, 1, seed=95)
    pop = MlpPolicy.stack([_policy(23), _policy(24)], envs_per_policy=256)
    before = _state_rows(env)
    with pytest.raises(_capi.SbrError, match="reach past"):
        env.lookahead_policy(pop, 2, 4)
    odd = _live(G, 8, 1, seed=96, first=100)
    with pytest.raises(_capi.SbrError, match="multiple of 256"):
        odd.lookahead_policy(pop, 2, 4)
    _untouched(env, before)
    env.close(); odd.close()


def test_graph_capture(G):
    """One lookahead_policy captured on a side stream, replayed twice with step() calls in between: each replay equals the eager
    call at that state.  Nothing in the call allocates or synchronises on the library's side (the results are allocated by
    torch inside the capture, from the graph's pool)."""
    n, k, n_steps, hold = 64, 8, 12, 2
    env = _live(G, n, 12, seed=101)
    pol = _policy()
    args = dict(hold=hold, noise_std=STD, noise_seed=4, keep_mean=True, return_rewards=True, return_best=True, return_actions=True,
                return_end=True)
    env.lookahead_policy(pol, k, n_steps, **args)      # loads the kernel outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            captured = env.lookahead_policy(pol, k, n_steps, **args)
    torch.cuda.current_stream().wait_stream(side)
    act = torch.tensor([1.5, 6.0], device="cuda").expand(n, 2).contiguous()
    seen = []
    for _ in range(2):
        env.step(act); env.step(act)
        g.replay()
        torch.cuda.synchronize()
        eager = env.lookahead_policy(pol, k, n_steps, **args)
        assert len(captured) == len(eager) == 8
        for u, v in zip(captured, eager):
            assert _same(u, v)
        seen.append(captured[0].clone())
    assert not torch.equal(seen[0], seen[1]) and bool((seen[1] != 0).any())
    env.close()


# ------------------------------------------------------------------ 10
def test_a_shard_equals_its_slice_of_the_unsharded_handle(G):
    """ShardedSbrOS.lookahead_policy on rank 1 of 2 (one process, one device), noise on: the rank's envs 6 .. 11 inside a handle
    of 12 and alone give the same bits - the noise is keyed by the global env id and the branch, not by the shard."""
    from gym_sbr2_amd import ShardedSbrOS
    n, k, n_steps, hold = 12, 3, 12, 2
    whole = _live(G, n, 30, seed=111)
    pol = _policy()
    sh = ShardedSbrOS(n, rank=1, world=2, device=0)
    assert (sh.start, sh.stop) == (6, 12) and sh.env.first_env_id == 6
    sh.env.reset(influent=whole.influent().T[6:].contiguous())
    x, c = whole.get_state()
    sh.env.set_state(x[:, 6:].contiguous(), c[:, 6:].contiguous())
    kw = dict(hold=hold, noise_std=STD, noise_seed=12, return_rewards=True, return_best=True, return_actions=True, return_end=True)
    full = whole.lookahead_policy(pol, k, n_steps, **kw)
    part = sh.lookahead_policy(pol, k, n_steps, obs=whole.obs[6:].clone(), **kw)
    for j, (u, v) in enumerate(zip(full, part)):
        assert _same(u[:, 6:] if j in (1, 4) else u[6:], v), j
    assert len(torch.unique(part[4][0, :, :, 0])) == 6 * k             # noise on: every branch decides for itself
    whole.close(); sh.close()


# ------------------------------------------------------------------ 11
def test_policy_rollout_planner(G):
    """plan() returns actions[0, i, best_index[i]] and the per-env mean of the (adjusted) returns; a terminal value that favours
    the last branch flips the winner of at least one env."""
    from gym_sbr2_amd import PolicyRolloutPlanner
    n, k, n_steps, hold = 6, 8, 10, 2
    env = _live(G, n, 60, seed=121)
    pol = _policy()
    before = _state_rows(env)
    ret, bi, br, acts = env.lookahead_policy(pol, k, n_steps, hold=hold, noise_std=STD, noise_seed=0, keep_mean=True,
                                             return_best=True, return_actions=True)
    plain = PolicyRolloutPlanner(env, pol, k, n_steps, hold, STD)
    act, value = plain.plan()
    pick = bi.long()
    assert act.shape == (n, 2) and act.dtype == torch.float32 and value.shape == (n,) and value.dtype == torch.float64
    assert torch.equal(act, acts[0, torch.arange(n), pick]) and torch.equal(value, ret.mean(dim=1)) and plain.decision == 1
    seen = {}

    def critic(o, s):
        seen["shapes"] = (tuple(o.shape), tuple(s.shape), o.dtype, s.dtype)
        v = 0.5 * o[..., 4] - 0.25 * s[..., 11]
        v[:, k - 1] += 1.0e6                           # beyond the horizon the last branch looks far better
        return v

    ret, acts, oe, se, de = env.lookahead_policy(pol, k, n_steps, hold=hold, noise_std=STD, noise_seed=5, keep_mean=True,
                                                 return_actions=True, return_end=True)
    want = ret + torch.where(de, torch.zeros_like(ret), critic(oe, se).double())
    idx, _ = _host_best(want)
    idx0, _ = _host_best(ret)
    assert not bool(de.any()) and np.all(idx == k - 1) and np.any(idx0 != k - 1)         # at least one winner flips
    withv = PolicyRolloutPlanner(env, pol, k, n_steps, hold, STD, terminal_value=critic, noise_seed=5)
    act, value = withv.plan()
    assert seen["shapes"] == ((n, k, 18), (n, k, 15), torch.float32, torch.float32)
    assert torch.equal(act, acts[0, :, k - 1]) and torch.equal(value, want.mean(dim=1))
    # decision d draws under noise_seed + d
    ret1, acts1, oe1, se1, de1 = env.lookahead_policy(pol, k, n_steps, hold=hold, noise_std=STD, noise_seed=6, keep_mean=True,
                                                      return_actions=True, return_end=True)
    act1, value1 = withv.plan()
    want1 = ret1 + torch.where(de1, torch.zeros_like(ret1), critic(oe1, se1).double())
    assert withv.decision == 2 and torch.equal(act1, acts1[0, :, k - 1]) and torch.equal(value1, want1.mean(dim=1))
    assert not torch.equal(acts1[0, :, 1:], acts[0, :, 1:]) and torch.equal(acts1[0, :, 0], acts[0, :, 0])     # branch 0: the mean
    _untouched(env, before)
    env.close()
