"""sbr_reset_models / sbr_collect_policy_models on the GPU: domain-randomised episodes - the envs of ONE handle as different plants -
against the route they replace.  The reference for a handle under test is always M REPLICA handles of the same N and first_env_id,
replica m created with config = models[m] and run through the PARENT call (reset / collect_policy / rollout_policy) on the same
inputs; the expected row of env i is replica model_index[i]'s row i.  Every comparison is bitwise (gpu_common.same: torch.equal with
NaN equal to NaN - a perturbed plant may leave the model's domain, on both sides alike).

Models are PlantModels.perturbed(cfg, M, rel_std=0.3, seed=...), model 0 the nominal config.  Inputs and nets are those of
tests/test_policy_rollout_gpu.py (inputs 202, net 13 = 2 x 32 tanh, net 51 = 1 x 64 relu, nets 23 / 24 as a population).

Which test runs which build of k_models_collect_policy<H, OCI, SCH, WAVES>:
  (32, no, 1, 1)  every test that is not named here
  (32, no, 0, 2)  test_other_builds[scheme0]
  (32, yes, 1, 1) test_other_builds[oci]
  (64, no, 1, 1)  test_other_builds[h64]
  (32, no, 1, 2)  test_two_waves_build (which also takes k_reset_models' 512-thread build)
  the other seven builds are not run by any test."""
import ctypes as C

import numpy as np
import pytest
from gpu_common import STEPS, inputs as _inputs, package, same as _same
from test_policy_rollout_gpu import _policy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

STD = (0.05, 0.3)
NOISE = dict(noise_std=STD, noise_seed=7)
FIELDS = (("obs", 1), ("actions", 1), ("rewards", 1), ("flags", 1), ("returns", 0), ("last_obs", 0))


@pytest.fixture(scope="module")
def G():
    return package()


def _eq(a, b):
    """Bitwise: torch.equal, with NaN equal to NaN for the float tensors."""
    return _same(a, b) if a.is_floating_point() else (a.dtype == b.dtype and torch.equal(a, b))


def _pick(ts, idx, dim):
    """Per env the entry of replica idx[env]: ts is one tensor per replica, the envs along `dim`."""
    st = torch.stack(list(ts)).movedim(dim + 1, 1)                    # [M, N, ...]
    return st[idx.to(st.device), torch.arange(st.shape[1], device=st.device)].movedim(0, dim)


class Kit:
    """A handle under test with a table of M models, and its M replicas: same N, first_env_id and dtypes, config = models[m]."""

    def __init__(self, G, n, m, inputs, per=256, first=0, seed=1, scheme=1, reward=None, **kw):
        from gym_sbr2_amd import PlantModels, _capi
        from gym_sbr2_amd.models import copy_config
        cfg = _capi.default_config(); cfg.scheme = scheme
        self.n, self.per, self.first = n, per, first
        self.scen = inputs[0][first:first + n] if len(inputs[0]) > n else inputs[0]
        self.rnd = inputs[1][first:first + n] if len(inputs[1]) > n else inputs[1]
        self.env = G.SbrOSVec(n, first_env_id=first, config=cfg, reward=reward, **kw)
        self.models = PlantModels.perturbed(self.env.cfg, m, rel_std=0.3, seed=seed)
        assert bytes(self.models[0]) == bytes(self.env.cfg)          # the nominal config is model 0
        self.env.set_models(self.models)
        assert self.env.num_models == m
        self.idx = self.env.model_index(per)
        self.reps = [G.SbrOSVec(n, first_env_id=first, config=copy_config(c), **kw) for c in self.models]

    def reset(self, **kw):
        kw = dict(dict(scenario=self.scen, rnd=self.rnd), **kw)
        self.env.reset_models(self.per, **kw)
        for r in self.reps:
            r.reset(**kw)

    def collect(self, pol, n_steps, hold, **noise):
        return self.env.collect_policy_models(pol, n_steps, self.per, hold=hold, **noise), [
            r.collect_policy(pol, n_steps, hold=hold, **noise) for r in self.reps]

    def check_state(self, what=""):
        """obs, the plant, every controller row and the stored influent."""
        assert _eq(self.env.obs, _pick([r.obs for r in self.reps], self.idx, 0)), what + " obs"
        got, want = self.env.get_state(), [r.get_state() for r in self.reps]
        assert _eq(got[0], _pick([w[0] for w in want], self.idx, 1)), what + " x"
        ctrl = _pick([w[1] for w in want], self.idx, 1)
        for row in range(ctrl.shape[0]):
            assert _eq(got[1][row], ctrl[row]), "%s ctrl row %d" % (what, row)
        assert _eq(self.env.influent(), _pick([r.influent() for r in self.reps], self.idx, 1)), what + " influent"

    def check_collection(self, col, cols, what=""):
        for f, dim in FIELDS:
            assert _eq(getattr(col, f), _pick([getattr(c, f) for c in cols], self.idx, dim)), "%s %s" % (what, f)

    def close(self):
        for e in [self.env] + self.reps:
            e.close()


def _raw(env, per, pol, n_steps, hold, obs, ret=None, acts=None, rew=None, obs_out=None, flags=None, noise_std=None, noise_seed=0):
    """sbr_collect_policy_models itself, on the caller's buffers."""
    from gym_sbr2_amd import _capi
    from gym_sbr2_amd.vec_env import _ptr
    s = pol.c_struct(env.device, noise_std=noise_std, noise_seed=noise_seed)
    _capi.check(env.lib.sbr_collect_policy_models(env._h, per, n_steps, hold, C.byref(s), _ptr(obs), _ptr(ret), _ptr(acts), _ptr(rew),
                                                  _ptr(obs_out), _ptr(flags), env._stream()), env._h)


def _snapshot(env):
    return env.get_state() + (env.influent(), env.obs.clone())


def _unchanged(env, snap):
    return all(_eq(a, b) for a, b in zip(_snapshot(env), snap))


# ------------------------------------------------------------------------------------------------------------ 1. reset
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_reset(G, out_dtype):
    """600 envs = two workgroups and a tail of 88, envs_per_model 256, two models: plants 0, 1, 0."""
    n = 600
    kit = Kit(G, n, 2, _inputs(n, 202), out_dtype=out_dtype)
    assert kit.idx.tolist() == [0] * 256 + [1] * 256 + [0] * 88
    pol = _policy(13, (32, 32))
    one = kit.idx == 1
    # the influent drawn on the device from the seed (the tables staged in LDS) ...
    kit.env.reset_models(256, seed=5)
    for r in kit.reps:
        r.reset(seed=5)
    kit.check_state("seed-drawn")
    assert kit.env.obs.dtype == out_dtype
    base = G.SbrOSVec(n, out_dtype=out_dtype)
    base.reset(seed=5)
    # ... and against vacuity: every env of plant 1 differs from what plain reset gives it, no env of plant 0 does
    differs = (kit.env.obs != base.obs).any(dim=1).cpu()
    assert bool(differs[one].all()) and not bool(differs[~one].any())
    assert _eq(kit.env.influent(), base.influent())                 # the draw reads nothing of the plant
    base.close()
    # the caller's normals and scenarios, then an explicit influent
    kit.reset()
    kit.check_state("rnd")
    infl = kit.env.influent().T.contiguous() * 1.03125
    kit.reset(scenario=None, rnd=None, influent=infl)
    kit.check_state("explicit influent")
    assert _eq(kit.env.influent()[1:], infl.T[1:])
    # some calls, then carry_over: the fill phase starts from each env's own state under its own model
    col, cols = kit.collect(pol, 20, 4)
    kit.check_collection(col, cols, "calls")
    before = kit.env.get_state()[0]
    kit.reset(carry_over=True, seed=9, scenario=None, rnd=None)
    kit.check_state("carry_over")
    assert not _eq(kit.env.get_state()[0], before)
    # a mask on every third env: the others keep every bit
    mask = (np.arange(n) % 3 == 0).astype(np.uint8)
    snap = _snapshot(kit.env)
    kit.reset(mask=mask, carry_over=True, influent=infl)
    kit.check_state("mask")
    kept = torch.from_numpy(mask == 0).cuda()
    now = _snapshot(kit.env)
    assert _eq(now[0][:, kept], snap[0][:, kept]) and _eq(now[1][:, kept], snap[1][:, kept]) and _eq(now[3][kept], snap[3][kept])
    assert not _eq(now[0][:, ~kept], snap[0][:, ~kept])
    kit.close()


# ------------------------------------------------------------------------------------------------------------ 2. a whole episode
N_EP, M_EP, CALLS, HOLD = 1100, 3, 470, 8


@pytest.fixture(scope="module")
def episode(G):
    """Shared and left unchanged: 1 100 envs under three models (plants 0, 1, 2, 0 and a tail of 76 under plant 1), 470 calls -
    seven more than the episode has - hold 8, with noise; the handle under test and its three replicas, kept open."""
    kit = Kit(G, N_EP, M_EP, _inputs(N_EP, 202), seed=2)
    assert kit.idx.tolist() == [0] * 256 + [1] * 256 + [2] * 256 + [0] * 256 + [1] * 76
    kit.reset()
    obs0 = kit.env.obs.clone()
    pol = _policy(13, (32, 32))
    col, cols = kit.collect(pol, CALLS, HOLD, **NOISE)
    yield dict(kit=kit, pol=pol, col=col, cols=cols, obs0=obs0)
    kit.close()


def test_a_whole_episode(episode):
    from gym_sbr2_amd import _capi
    kit, col, cols = episode["kit"], episode["col"], episode["cols"]
    rows = -(-CALLS // HOLD)
    assert col.obs.shape == (rows, N_EP, 18) and col.flags.shape == (rows, N_EP) and col.rewards.shape == (CALLS, N_EP)
    kit.check_state("episode")
    kit.check_collection(col, cols, "episode")
    assert col.last_obs is kit.env.obs and _eq(col.obs[0], episode["obs0"])
    # the done call (call 462, in decision 57) ran its terminal phases under each env's model; zero rows after it
    x, c = kit.env.get_state()
    assert bool((c[_capi.C_DONE] == 1).all()) and bool((c[_capi.C_STEPS] == STEPS).all())
    last = (STEPS - 1) // HOLD
    assert bool((col.flags[:last] == 1).all()) and bool((col.flags[last] == 3).all()) and bool((col.flags[last + 1:] == 0).all())
    assert bool((col.obs[last + 1:] == 0).all()) and bool((col.actions[last + 1:] == 0).all()) and bool((col.rewards[STEPS:] == 0).all())
    assert _eq(c[_capi.C_QW], _pick([r.get_state()[1][_capi.C_QW] for r in kit.reps], kit.idx, 0))
    assert float(col.actions[..., 0].std()) > 1e-3 and float(col.actions[..., 1].std()) > 1e-3       # a policy, not a constant
    # against vacuity: replica 0 IS a base-plant run of all 1 100 envs - plants 1 and 2 return something else, plant 0 the same
    other = (col.returns != cols[0].returns).cpu()
    assert bool(other[kit.idx != 0].all()) and not bool(other[kit.idx == 0].any())
    assert not bool(torch.isnan(col.returns[kit.idx.cuda() == 0]).any())


# ------------------------------------------------------------------------------------------------------------ 3. cuts and shards
def test_cut_into_launches(G, episode):
    """Launches of 5, 3 and the rest: against replicas cut the same way (a decision is taken on the calls s % hold == 0 of a
    LAUNCH, so a cut inside a decision moves the decisions for parent and child alike) - and, with hold 1, where a cut moves no
    decision, against the uncut launch as well."""
    pol = episode["pol"]
    kit = Kit(G, N_EP, M_EP, _inputs(N_EP, 202), seed=2)
    kit.reset()
    for k in (5, 3, CALLS - 8):
        col, cols = kit.collect(pol, k, HOLD, **NOISE)
        kit.check_collection(col, cols, "cut %d" % k)
    kit.check_state("cut")
    assert bool((col.flags[(STEPS - 9) // HOLD] == 3).all())
    # hold 1: 40 calls in one launch, then 5 + 3 + 32 on a second reset
    kit.reset()
    whole, cols = kit.collect(pol, 40, 1, **NOISE)
    kit.check_collection(whole, cols, "hold 1")
    state, whole_last = kit.env.get_state(), whole.last_obs.clone()
    kit.env.reset_models(256, scenario=kit.scen, rnd=kit.rnd)
    parts = [kit.env.collect_policy_models(pol, k, 256, hold=1, **NOISE) for k in (5, 3, 32)]
    for f in ("obs", "actions", "rewards", "flags"):
        assert _eq(torch.cat([getattr(p, f) for p in parts]), getattr(whole, f)), f
    assert _eq(kit.env.get_state()[0], state[0]) and _eq(kit.env.get_state()[1], state[1]) and _eq(parts[2].last_obs, whole_last)
    kit.close()


def test_optional_outputs_and_no_call(G):
    """n_steps = 0 on sentinel buffers; obs_out alone; flags_out alone; both NULL through rollout_policy_models."""
    n, calls, hold = 600, 30, 4
    pol = _policy(13, (32, 32))
    kit = Kit(G, n, 2, _inputs(n, 202))
    kit.reset()
    obs0 = kit.env.obs.clone()
    snap = _snapshot(kit.env)
    o = obs0.clone()
    ret = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    acts = torch.full((2, n, 2), 5.0, device="cuda"); rew = torch.full((2, n), 5.0, dtype=torch.float64, device="cuda")
    rows = torch.full((2, n, 18), 5.0, device="cuda"); flags = torch.full((2, n), 9, dtype=torch.uint8, device="cuda")
    _raw(kit.env, 256, pol, 0, 3, o, ret, acts, rew, rows, flags)
    assert bool((ret == 0).all()) and bool((acts == 5).all()) and bool((rew == 5).all()) and bool((rows == 5).all()) and bool((flags == 9).all())
    assert _eq(o, obs0) and _unchanged(kit.env, snap)
    c0 = kit.env.collect_policy_models(pol, 0, 256)
    assert c0.obs.shape == (0, n, 18) and c0.flags.shape == (0, n) and bool((c0.returns == 0).all()) and _unchanged(kit.env, snap)
    # the reference: every output
    full, cols = kit.collect(pol, calls, hold, **NOISE)
    kit.check_collection(full, cols, "full")
    end = _snapshot(kit.env)
    for which in ("obs_out", "flags", "neither"):
        kit.env.reset_models(256, scenario=kit.scen, rnd=kit.rnd)
        assert _unchanged(kit.env, snap)
        if which == "neither":
            r, a, w = kit.env.rollout_policy_models(pol, calls, 256, hold=hold, return_actions=True, return_rewards=True, **NOISE)
        else:
            o = kit.env.obs
            r = torch.empty_like(full.returns); a = torch.empty_like(full.actions); w = torch.empty_like(full.rewards)
            extra = torch.empty_like(full.obs) if which == "obs_out" else torch.empty_like(full.flags)
            _raw(kit.env, 256, pol, calls, hold, o, r, a, w, **{which: extra}, **NOISE)
            assert _eq(extra, full.obs if which == "obs_out" else full.flags), which
        assert _eq(r, full.returns) and _eq(a, full.actions) and _eq(w, full.rewards) and _unchanged(kit.env, end), which
    # ... and the rollout form alone, returns only, against the replicas' rollout_policy
    kit.reset()
    r = kit.env.rollout_policy_models(pol, calls, 256, hold=hold)
    assert _eq(r, _pick([q.rollout_policy(pol, calls, hold=hold) for q in kit.reps], kit.idx, 0))
    kit.check_state("rollout form")
    kit.close()


def test_an_envs_result_does_not_depend_on_the_batch_around_it(G):
    """The rule is keyed by the global env id: a 512-env handle at first_env_id 768 equals rows 768 .. 1279 of a 1 536-env handle,
    and a two-rank ShardedSbrOS equals the single handle."""
    from gym_sbr2_amd import ShardedSbrOS
    n, calls, hold = 1536, 40, 7
    inputs = _inputs(n, 202)
    pol = _policy(13, (32, 32))
    big = Kit(G, n, 2, inputs, seed=3)
    big.reset()
    big.check_state("big reset")
    obs0 = big.env.obs.clone()
    col, cols = big.collect(pol, calls, hold, **NOISE)
    big.check_collection(col, cols, "big")
    bx, bc = big.env.get_state()

    def check(env, lo, hi, got, reset_obs):
        assert _eq(reset_obs, obs0[lo:hi])
        x, c = env.get_state()
        assert _eq(x, bx[:, lo:hi]) and _eq(c, bc[:, lo:hi]) and _eq(env.influent(), big.env.influent()[:, lo:hi])
        for f, dim in FIELDS:
            assert _eq(getattr(got, f), getattr(col, f).narrow(dim, lo, hi - lo)), f

    part = G.SbrOSVec(512, first_env_id=768)
    part.set_models(big.models)
    assert part.model_index(256).tolist() == big.idx[768:1280].tolist() == [1] * 256 + [0] * 256
    o = part.reset_models(256, scenario=inputs[0][768:1280], rnd=inputs[1][768:1280]).clone()
    check(part, 768, 1280, part.collect_policy_models(pol, calls, 256, hold=hold, **NOISE), o)
    part.close()
    for rank in (0, 1):
        sh = ShardedSbrOS(n, rank=rank, world=2, device=0)
        assert (sh.start, sh.stop) == (768 * rank, 768 * rank + 768)
        sh.set_models(big.models)
        assert sh.model_index(256).tolist() == big.idx[sh.start:sh.stop].tolist()
        o = sh.reset_models(256, scenario=inputs[0][sh.start:sh.stop], rnd=inputs[1][sh.start:sh.stop]).clone()
        check(sh.env, sh.start, sh.stop, sh.collect_policy_models(pol, calls, 256, hold=hold, **NOISE), o)
        sh.close()
    big.close()


# ------------------------------------------------------------------------------------------------------------ 4. special tables
def test_one_model_is_the_parent(G):
    """M = 1 with the handle's own config: the bits of plain reset and collect_policy, envs_per_model not read, any first_env_id."""
    n = 300
    inputs = _inputs(n, 202)
    pol = _policy(13, (32, 32))
    env, twin = G.SbrOSVec(n, first_env_id=64), G.SbrOSVec(n, first_env_id=64)
    env.set_models([env.cfg])
    assert env.num_models == 1 and env.model_index(0).tolist() == [0] * n
    env.reset_models(0, seed=4); twin.reset(seed=4)
    assert _unchanged(env, _snapshot(twin))
    env.reset_models(300, scenario=inputs[0], rnd=inputs[1]); twin.reset(scenario=inputs[0], rnd=inputs[1])
    assert _unchanged(env, _snapshot(twin))
    a, b = env.collect_policy_models(pol, STEPS, -5, hold=8, **NOISE), twin.collect_policy(pol, STEPS, hold=8, **NOISE)
    assert all(_eq(p, q) for p, q in zip(a, b)) and _unchanged(env, _snapshot(twin))
    env.close(); twin.close()


def test_population_and_models_vary_independently(G):
    """Two nets at envs_per_policy 512, two models at envs_per_model 256, 1 024 envs: (net, plant) = (23, 0), (23, 1), (24, 0), (24, 1)."""
    from gym_sbr2_amd import MlpPolicy
    n = 1024
    pop = MlpPolicy.stack([_policy(23, (32, 32)), _policy(24, (32, 32))], envs_per_policy=512)
    kit = Kit(G, n, 2, _inputs(n, 202), seed=4)
    kit.reset()
    col, cols = kit.collect(pop, 60, 7, **NOISE)
    kit.check_collection(col, cols, "population")
    kit.check_state("population")
    # all four blocks differ: the same inputs would otherwise repeat every 4 envs' scenarios, not whole blocks
    blocks = [col.returns[k * 256:(k + 1) * 256] for k in range(4)]
    assert all(not _eq(blocks[i], blocks[j]) for i in range(4) for j in range(i))
    kit.close()


# ------------------------------------------------------------------------------------------------------------ 5. other builds
@pytest.mark.parametrize("build", ["scheme0", "oci", "h64"])
def test_other_builds(G, build):
    """A whole episode at 300 envs = 256 + 44 (plant 0, then a partial wave under plant 1), hold 8, against replicas."""
    from gym_sbr2_amd import _capi
    n = 300
    if build == "h64":                     # a 1 x 64 relu net whose units >= 32 carry weight
        with pytest.warns(RuntimeWarning, match="64-wide"):
            pol = _policy(51, (64,), "relu")
        assert pol.width == 64 and np.any(pol.block[0, 18 * 32:18 * 64] != 0)
        scheme, reward = 1, "eqi_oci"
    else:
        pol = _policy(13, (32, 32))
        scheme, reward = (0, "eqi_oci") if build == "scheme0" else (1, "oci")
    kit = Kit(G, n, 2, _inputs(n, 202), scheme=scheme, reward=reward, seed=5)
    assert kit.idx.tolist() == [0] * 256 + [1] * 44
    assert kit.env.cfg.scheme == scheme and kit.env.cfg.reward_kind == _capi.REWARD_KINDS[reward]
    assert all(r.cfg.scheme == scheme and r.cfg.reward_kind == _capi.REWARD_KINDS[reward] for r in kit.reps)
    assert kit.env.query(_capi.Q_ROLLOUT_WAVES) == (2 if scheme == 0 else 1)
    kit.reset()
    kit.check_state("reset")
    col, cols = kit.collect(pol, STEPS, 8, **NOISE)
    kit.check_collection(col, cols, build)
    kit.check_state(build)
    assert bool((col.flags[:-1] == 1).all()) and bool((col.flags[-1] == 3).all())
    assert bool((col.returns[256:] != cols[0].returns[256:]).all())
    kit.close()


def test_two_waves_build(G):
    """The next multiple of 256 above the one-wave limit of the fused kernels (98 560 envs on a whole MI355X), 40 calls, which cross
    the first phase boundary, hold 5; the reset runs in 512-thread workgroups, which span two models each."""
    from gym_sbr2_amd import _capi
    probe = G.SbrOSVec(1)
    n = (probe.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS) // 256 + 1) * 256
    probe.close()
    kit = Kit(G, n, 2, _inputs(n, 505), seed=6)
    assert kit.env.query(_capi.Q_ROLLOUT_WAVES) == 2 and kit.env.query(_capi.Q_RESET_BLOCK) == 512
    kit.reset()
    kit.check_state("reset")
    col, cols = kit.collect(_policy(13, (32, 32)), 40, 5)
    kit.check_collection(col, cols, "two waves")
    kit.check_state("two waves")
    assert col.flags.shape == (8, n) and bool((col.flags == 1).all())
    kit.close()


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_everything_as_it_was(G):
    from gym_sbr2_amd import PlantModels, _capi
    n = 300
    inputs = _inputs(n, 202)
    pol = _policy(13, (32, 32))
    for first in (0, 64):
        env = G.SbrOSVec(n, first_env_id=first)
        env.reset(scenario=inputs[0], rnd=inputs[1])
        env.collect_policy(pol, 10, hold=3)
        snap = _snapshot(env)
        o = env.obs.clone()
        ret = torch.full((n,), 7.0, dtype=torch.float64, device="cuda"); rows = torch.full((4, n, 18), 5.0, device="cuda")
        flags = torch.full((4, n), 9, dtype=torch.uint8, device="cuda")

        def refused(why, per):
            with pytest.raises(_capi.SbrError, match="sbr_collect_policy_models: .*" + why):
                _raw(env, per, pol, 10, 3, o, ret, None, None, rows, flags)
            with pytest.raises(_capi.SbrError, match="sbr_collect_policy_models: .*" + why):
                env.rollout_policy_models(pol, 10, per, hold=3)
            with pytest.raises(_capi.SbrError, match="sbr_reset_models: .*" + why):
                env.reset_models(per, scenario=inputs[0], rnd=inputs[1])
            assert _unchanged(env, snap) and _eq(o, snap[3]) and bool((ret == 7).all()) and bool((rows == 5).all()) and bool((flags == 9).all())

        refused("no model table", 256)
        with pytest.raises(ValueError):
            env.model_index(256)
        env.set_models(PlantModels.perturbed(env.cfg, 2, rel_std=0.3, seed=1))
        if first == 0:
            refused("envs_per_model must be a positive multiple of 256", 0)
            refused("envs_per_model must be a positive multiple of 256", 300)
            refused("envs_per_model must be a positive multiple of 256", -256)
            env.collect_policy_models(pol, 3, 256)                                 # the same handle, a valid call
            assert not _unchanged(env, snap)
        else:
            refused("first_env_id must be a non-negative multiple of 256", 256)
            refused("envs_per_model must be a positive multiple of 256", 300)      # the last failing check is reported
            with pytest.raises(ValueError):
                env.model_index(256)
        env.set_models(None)
        assert env.num_models == 0
        snap = _snapshot(env)
        o.copy_(snap[3])
        refused("no model table", 256)
        env.close()


# ------------------------------------------------------------------------------------------------------------ 7. table changes, capture
def test_table_changes_and_the_base_plant(G):
    """The table replaced between two launches: the second launch runs the new plants.  step(), reset() and collect_policy() give
    base-plant bits before, between and after - a twin handle that never had a table runs the same base calls."""
    from gym_sbr2_amd import PlantModels
    n = 600
    pol = _policy(13, (32, 32))
    kit = Kit(G, n, 2, _inputs(n, 202), seed=7)
    twin = G.SbrOSVec(n)
    act = torch.from_numpy(np.stack([np.full(n, 1.5), np.full(n, 6.0)], axis=-1)).float().cuda()

    def base_calls(what):
        outs = []
        for e in (kit.env, twin):
            e.reset(scenario=kit.scen, rnd=kit.rnd)
            step = [t.clone() for t in e.step(act)]
            col = e.collect_policy(pol, 12, hold=5, **NOISE)
            outs.append(step + list(col) + list(_snapshot(e)))
        assert all(_eq(p, q) for p, q in zip(*outs)), what

    base_calls("before")
    kit.reset()
    col, cols = kit.collect(pol, 25, 4, **NOISE)
    kit.check_collection(col, cols, "first table")
    base_calls("between")
    # another table, of another size: the same handle, new replicas
    old = kit.reps
    kit.models = PlantModels.perturbed(kit.env.cfg, 3, rel_std=0.3, seed=8)
    kit.env.set_models(kit.models)
    assert kit.env.num_models == 3
    kit.idx = kit.env.model_index(256)
    assert kit.idx.tolist() == [0] * 256 + [1] * 256 + [2] * 88
    from gym_sbr2_amd.models import copy_config
    kit.reps = [G.SbrOSVec(n, config=copy_config(c)) for c in kit.models]
    kit.reset()
    kit.check_state("second table reset")
    col2, cols2 = kit.collect(pol, 25, 4, **NOISE)
    kit.check_collection(col2, cols2, "second table")
    kit.check_state("second table")
    assert not _eq(col2.returns[256:], col.returns[256:]) and _eq(col2.returns[:256], col.returns[:256])
    base_calls("after")
    for e in old + [twin]:
        e.close()
    kit.close()


def test_graph_capture(G):
    """Nothing is allocated by the launch: one collect_policy_models is captured into a graph on one stream and replayed."""
    n = 600
    pol = _policy(13, (32, 32))
    kit = Kit(G, n, 2, _inputs(n, 202))
    kit.reset()
    env = kit.env
    x0, c0 = env.get_state()
    o0 = env.obs.clone()
    o = o0.clone()
    eager = env.collect_policy_models(pol, 20, 256, hold=3, obs=o)
    cols = [r.collect_policy(pol, 20, hold=3) for r in kit.reps]
    kit.check_collection(eager, cols, "eager")
    se, oe = env.get_state(), o.clone()
    env.set_state(x0, c0)
    o.copy_(o0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            cap = env.collect_policy_models(pol, 20, 256, hold=3, obs=o)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert all(_eq(p, q) for p, q in zip(env.get_state(), se))
    assert _eq(o, oe) and not _eq(oe, o0)
    assert all(_eq(p, q) for p, q in zip(tuple(cap)[:5], tuple(eager)[:5]))
    kit.close()
