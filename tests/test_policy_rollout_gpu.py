"""sbr_rollout_policy / SbrOSVec.rollout_policy on the GPU: the fused closed-loop rollout under the caller's MLP, checked
bit for bit by the tape kernel (the plant integrates the actions it reports) and in lockstep by sbr_step plus a float64
evaluation of the same net (the reported actions are the net's).

Inputs follow tests/test_tape_rollout_gpu.py::_inputs: influent scenario 4 + global id % 4, the influent's normal draws from a
seeded RandomState.  Policies are drawn from a seeded RandomState (`_net`), low = (0, 0), high = (2.5, 15).  Seeds, chosen on
the CPU: with each of them the C oracle, run in closed loop (OracleBatch.step(..., want_obs=True), the observation rounded to
float32, the same net evaluated in float64, the action rounded to float32), raises none of SBR_ST_NEGATIVE / SBR_ST_NEAR_POLE /
SBR_ST_NONFINITE on any env in 463 calls:
  inputs 202 at 512 envs, hold 1, with nets 14 (no hidden layer), 12 (1 x 32, tanh and relu), 13 (2 x 32 tanh), 42 (2 x 32 relu);
  inputs 303 at 512 envs with net 13, hold 8;  inputs 202 with nets 23 / 24 as a population of 2 x 256 envs;
  inputs 404 at 4096 envs with net 13;  inputs 202 with net 33 (2 x 20, padded);
  inputs 202 at 256 envs (the first 256 rows of the 512-env inputs), hold 1, with the 64-wide nets 52 (1 x 64 tanh), 51 (1 x 64
  relu), 53 (2 x 64, tanh and relu), 50 (48 + 64, tanh and relu), with net 71 rescaled for squash "none" (test_squash_none), and
  with net 13 under (scheme, reward) = (0, eqi_oci), (1, g2anet), (1, oci), (0, oci).
(Rejected by the same check, for the record: nets 11 and 15 without a hidden layer, 13 and 41 with relu, 21 / 22 as a
population, 31 as the 2 x 20 net - between 3 and 173 of the 512 envs reach negative ammonia under them; of the 64-wide nets
1 x 64 tanh 50, 51, 54 and relu 50, 60; 2 x 64 tanh 51, 52, 56 and relu 50, 52, 56; 48 + 64 tanh 51, 55 - 58 and relu 55, 56;
net 75 for squash "none".)
So the tolerance tests assert that no env is flagged and mask nothing.  (The bit-for-bit comparisons need no such condition;
the 98 624-env case and the population of 64-wide nets make none.)

Which test runs which build of k_rollout_policy<H, OCI, SCH, WAVES> (the host picks H from the net, OCI from reward "oci", and
(SCH, WAVES) = (1, 1) up to 98 304 envs, (1, 2) above, (0, 2) for scheme 0):
  (32, no, 1, 1)  every test below that is not named here;  its reward "g2anet" branch: test_schemes_and_rewards_...[1-g2anet]
  (32, no, 1, 2)  test_two_waves_build_above_98304_envs_matches_small_handles
  (32, no, 0, 2)  test_schemes_and_rewards_against_the_tape_kernel[0-eqi_oci]
  (32, yes, 1, 1) test_schemes_and_rewards_against_the_tape_kernel[1-oci]
  (32, yes, 0, 2) test_schemes_and_rewards_against_the_tape_kernel[0-oci]
  (64, no, 1, 1)  test_the_64_wide_net_with_real_weights, test_population_of_64_wide_nets, test_padding_changes_no_bit
  (64, no, 1, 2)  test_two_waves_build_above_98304_envs_matches_small_handles (its second half)
  (32, yes, 1, 2), (64, no, 0, 2) and the three (64, yes, ...) builds are not run by any test.
pl.squash == 0: test_squash_none; every other test squashes with tanh."""
import numpy as np
import pytest
from gpu_common import (CONFIGS, FLAGS, STEPS, handle as _handle, inputs as _inputs, net as _net, no_flags, package,
                        to_np as _np)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LOW, HIGH = (0.0, 0.0), (2.5, 15.0)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def G():
    return package()


def _policy(seed, widths, activation="tanh"):
    from gym_sbr2_amd import MlpPolicy
    return MlpPolicy(_net(seed, widths), activation=activation, squash="tanh", low=LOW, high=HIGH)


def _env(G, n, inputs, first=0, **kw):
    scen, rnd = inputs
    env = G.SbrOSVec(n, first_env_id=first, **kw)
    env.reset(scenario=scen[first:first + n] if len(scen) > n else scen, rnd=rnd[first:first + n] if len(rnd) > n else rnd)
    return env


def _same_state(a, b, cols=slice(None)):
    from gym_sbr2_amd import _capi
    xa, ca = a.get_state()
    xb, cb = b.get_state()
    assert torch.equal(xa[:, cols] if cols != slice(None) else xa, xb)
    ca = ca[:, cols] if cols != slice(None) else ca
    for row in range(_capi.NCTRL):
        assert torch.equal(ca[row], cb[row]), row


def _no_flags(env):
    from gym_sbr2_amd import _capi
    no_flags(env.ctrl_row(_capi.C_STATUS))


def _bound(pol, o, member=0):
    """Per sample, in float64: the action means of the PACKED net on observations o [n, 18], and the bound on what a float32
    evaluation with fmaf chains (k ascending) and <= 5 ulp tanhf may differ from them, the input itself being off by up to
    2 u |o| (k_step's and the fused kernel's float32 observations may round differently).  u = 2^-24.
      per layer: e_pre = (in + 1) u (|W| |h| + |b|) + |W| e;   e_h = e_pre + 5 u |h_out|   (both activations are 1-Lipschitz)
      finally:   |d a| <= scale (e_pre + 5 u) + u |a|;   with squash "none":  a = pre,  |d a| <= e_pre + u |a|."""
    blk = pol.block[member].astype(np.float64)
    h = np.asarray(o, dtype=np.float64)
    e = 2 * U * np.abs(h)
    fan_in, at = 18, 0
    for k in range(pol.n_hidden + 1):
        out = 2 if k == pol.n_hidden else pol.width
        w = blk[at:at + out * fan_in].reshape(out, fan_in)
        b = blk[at + out * fan_in:at + out * fan_in + out]
        at += out * fan_in + out
        pre = h @ w.T + b
        e_pre = (fan_in + 1) * U * (np.abs(h) @ np.abs(w).T + np.abs(b)) + e @ np.abs(w).T
        if k < pol.n_hidden:
            h = np.tanh(pre) if pol.activation == "tanh" else np.maximum(pre, 0.0)
            e = e_pre + 5 * U * np.abs(h)
        fan_in = out
    scale, bias = pol.act_scale.astype(np.float64), pol.act_bias.astype(np.float64)
    if pol.squash == "none":          # scale 1, bias 0: the kernel's fmaf(1, y, 0) is exact, a = pre and |d a| <= e_pre + u |a|
        return pre, e_pre + U * np.abs(pre)
    a = bias + scale * np.tanh(pre)
    return a, scale * (e_pre + 5 * U) + U * np.abs(a)


def _lockstep(G, n, inputs, pol, acts, obs0):
    """A fresh handle steps the reported actions through sbr_step while the net is evaluated in float64 on ITS observations:
    the worst |d a| / bound over all calls (`_bound`), and the observation after call 199.  No env may be flagged."""
    c_env = _env(G, n, inputs)
    assert torch.equal(c_env.obs, obs0)
    worst, obs199 = 0.0, None
    for s in range(acts.shape[0]):
        mean, bound = _bound(pol, _np(c_env.obs))
        ratio = np.abs(_np(acts[s]).astype(np.float64) - mean) / bound
        worst = max(worst, float(ratio.max()))
        c_env.step(acts[s])
        if s == 199:
            obs199 = c_env.obs.clone()
    _no_flags(c_env)
    c_env.close()
    return worst, obs199


@pytest.fixture(scope="module")
def ref(G):
    """One 2 x 32 tanh episode at 512 envs, shared and left unchanged: handle A's fused closed-loop run, and handle C stepping
    A's reported actions through sbr_step while the net is evaluated in float64 on C's observations."""
    from gym_sbr2_amd import _capi
    n = 512
    inputs = _inputs(n, 202)
    pol = _policy(13, (32, 32))
    a_env = _env(G, n, inputs)
    obs0 = a_env.obs.clone()
    ret, acts, rew = a_env.rollout_policy(pol, STEPS, return_actions=True, return_rewards=True)
    xa, ca = a_env.get_state()
    worst, obs199 = _lockstep(G, n, inputs, pol, acts, obs0)
    out = dict(n=n, inputs=inputs, pol=pol, ret=ret, acts=acts, rew=rew, x=xa, c=ca, obs_end=a_env.obs.clone(), obs0=obs0,
               worst_ratio=worst, obs199=obs199, status=ca[_capi.C_STATUS].clone())
    a_env.close()
    return out


def test_n_steps_zero_touches_nothing_and_bad_arguments_are_refused_on_a_live_handle(G):
    from gym_sbr2_amd import _capi
    env = _env(G, 64, _inputs(64, 202))
    pol = _policy(12, (32,))
    x0, c0 = env.get_state()
    o0 = env.obs.clone()
    ret = env.rollout_policy(pol, 0)
    x1, c1 = env.get_state()
    assert torch.equal(ret, torch.zeros_like(ret)) and torch.equal(x0, x1) and torch.equal(c0, c1) and torch.equal(env.obs, o0)
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, hold=0)
    with pytest.raises(ValueError):
        env.rollout_policy(pol, 5, obs=torch.zeros(63, 18, device="cuda"))
    with pytest.raises(_capi.SbrError, match="sbr_rollout_policy"):
        env.rollout_policy(pol, 5, noise_std=(-1.0, 0.0))
    x1, c1 = env.get_state()
    assert torch.equal(x0, x1) and torch.equal(c0, c1) and torch.equal(env.obs, o0)
    env.close()


@pytest.mark.parametrize("widths,activation,seed", [((), "tanh", 14), ((), "relu", 14), ((32,), "tanh", 12), ((32,), "relu", 12),
                                                    ((32, 32), "tanh", 13), ((32, 32), "relu", 42)])
def test_the_plant_integrates_the_actions_it_reports(G, widths, activation, seed):
    """Handle A runs the closed loop; handle B is fed A's reported actions as a tape.  Both kernels inline the same device
    functions: plant, every controller row, returns and rewards agree bit for bit."""
    from gym_sbr2_amd import _capi
    n = 512
    inputs = _inputs(n, 202)
    pol = _policy(seed, widths, activation)
    a_env, b_env = _env(G, n, inputs), _env(G, n, inputs)
    obs0 = a_env.obs.clone()
    ret_a, acts, rew_a = a_env.rollout_policy(pol, STEPS, return_actions=True, return_rewards=True)
    assert acts.shape == (STEPS, n, 2) and acts.dtype == torch.float32 and rew_a.shape == (STEPS, n)
    ret_b, rew_b = b_env.rollout_actions(acts, return_rewards=True)
    _same_state(a_env, b_env)
    assert torch.equal(ret_a, ret_b) and torch.equal(rew_a, rew_b)
    _, c = a_env.get_state()
    assert bool((c[_capi.C_DONE] == 1).all()) and bool((c[_capi.C_STEPS] == STEPS).all()) and bool((c[_capi.C_PLAN] == 0).all())
    _no_flags(a_env)
    assert float(acts[..., 0].std()) > 1e-3 and float(acts[..., 1].std()) > 1e-3       # a policy, not a constant
    a_env.close(); b_env.close()
    # ... and they are THIS net's (its layer offsets, its activation): the lockstep check of test_the_reported_actions_are_the_nets
    if not (widths == (32, 32) and activation == "tanh"):          # that one is the shared `ref` episode
        worst, _ = _lockstep(G, n, inputs, pol, acts, obs0)
        print("%s %s: worst |d a| / bound %.4f" % (widths, activation, worst))
        assert worst <= 1.0


def _bits_then_lockstep(G, n, inputs, pol):
    """The body of test_the_plant_integrates_the_actions_it_reports for any net: handle A in closed loop, handle B on A's
    reported actions as a tape (bit for bit), then `_lockstep`.  Returns (acts, obs0, worst |d a| / bound)."""
    from gym_sbr2_amd import _capi
    a_env, b_env = _env(G, n, inputs), _env(G, n, inputs)
    obs0 = a_env.obs.clone()
    ret_a, acts, rew_a = a_env.rollout_policy(pol, STEPS, return_actions=True, return_rewards=True)
    assert acts.shape == (STEPS, n, 2) and acts.dtype == torch.float32 and rew_a.shape == (STEPS, n)
    ret_b, rew_b = b_env.rollout_actions(acts, return_rewards=True)
    _same_state(a_env, b_env)
    assert torch.equal(ret_a, ret_b) and torch.equal(rew_a, rew_b)
    _, c = a_env.get_state()
    assert bool((c[_capi.C_DONE] == 1).all()) and bool((c[_capi.C_STEPS] == STEPS).all()) and bool((c[_capi.C_PLAN] == 0).all())
    _no_flags(a_env)
    a_env.close(); b_env.close()
    worst, _ = _lockstep(G, n, inputs, pol, acts, obs0)
    return acts, obs0, worst


@pytest.mark.parametrize("widths,activation,seed", [((64,), "tanh", 52), ((64,), "relu", 51), ((64, 64), "tanh", 53),
                                                    ((64, 64), "relu", 53), ((48, 64), "tanh", 50), ((48, 64), "relu", 50)])
def test_the_64_wide_net_with_real_weights(G, widths, activation, seed):
    """The H = 64 build (scheme 1, one wave) under nets whose hidden units 32 .. 63 carry weight: every output group j0 = 0 .. 56 of
    sbr_mlp_layer<18,64,8> and <64,64,8>, their bias addresses and the advance of the block pointer between the layers decide
    bits here.  256 envs (one workgroup), a whole episode: bits against the tape kernel, then each of the 463 x 256 x 2 reported
    actions inside its bound against the float64 net on sbr_step's observations.
    Measured on the MI355X, worst |d a| / bound: (64,) tanh 0.0197, relu 0.0138; (64, 64) tanh 0.0026, relu 0.0020; (48, 64)
    tanh 0.0027, relu 0.0039.
    What the check can see.  Zeroing the bias (-0.112) of unit 40 of layer 2 in the checker's copy of the (64, 64) tanh block
    moves the float64 mean of call 0 by up to 20.2 bounds, and by more than one bound on every env (asserted below).  One
    float of layer 2 at a unit >= 32 changed in the block the lockstep check reads, on a scratch copy of this case: on the
    MI355X W2[40][33] + 0.001 gives worst = 0.41, W2[63][5] + 0.001 gives 0.59, W2[32][63] + 0.0001 gives 0.02 - the bound is
    a worst-case sum and such a change stays inside it; the ratio grows in proportion, so the case fails from about +0.0025 on.
    The errors it is there for, a float read from a wrong address, are larger: with the same actions taken from the oracle in
    closed loop (the CPU stand-in of this check) W2[40][33] + 0.01 gives 4.1, + 0.1 gives 40, W2[40][33] := W2[40][34] 104,
    W2[63][5] := W2[62][5] 39, b2[40] := b2[41] 226, and the case fails."""
    n = 256
    inputs = _inputs(n, 202)
    with pytest.warns(RuntimeWarning, match="64-wide"):
        pol = _policy(seed, widths, activation)
    assert pol.width == 64 and pol.n_hidden == len(widths)
    acts, obs0, worst = _bits_then_lockstep(G, n, inputs, pol)
    assert float(acts[..., 0].std()) > 1e-3 and float(acts[..., 1].std()) > 1e-3       # a policy, not a constant
    print("%s %s: worst |d a| / bound %.4f, action std %.3f and %.3f" % (widths, activation, worst, float(acts[..., 0].std()),
                                                                         float(acts[..., 1].std())))
    assert worst <= 1.0
    if widths == (64, 64):
        l2 = 18 * 64 + 64                                                              # where layer 2 starts in the block
        w2 = pol.block[0, l2:l2 + 64 * 64].reshape(64, 64)
        assert np.any(w2[32:] != 0) and np.any(w2[:, 32:] != 0)                        # a full layer, not a padded one
        if activation == "tanh":
            # the check has teeth: without the bias of hidden unit 40 of layer 2 the float64 mean leaves the bound
            unit = 40
            cut = pol.widened(64)
            cut.block = pol.block.copy()
            assert cut.block[0, l2 + 64 * 64 + unit] != 0
            cut.block[0, l2 + 64 * 64 + unit] = 0.0
            o = _np(obs0)
            mean, bound = _bound(pol, o)
            moved = np.abs(_bound(cut, o)[0] - mean) / bound
            print("bias of unit %d of layer 2 zeroed: |d mean| / bound up to %.1f" % (unit, moved.max()))
            assert (moved.max(axis=1) > 1.0).any()


def test_squash_none(G):
    """pl.squash == 0 on the device: the two outputs of the net ARE the set-points (scale 1, bias 0).  Net 71 (2 x 32 tanh) with
    the last layer scaled by (0.4, 2.0) and shifted by (1.25, 7.5), so that they are set-points: with it the oracle in closed
    loop (module docstring) flags no env at 256 envs, inputs 202, and the actions span 0.95 .. 1.42 and 6.1 .. 7.1 (seeds 70,
    72 - 74 and 76 - 79 pass as well, 75 does not).  Bits against the tape kernel, then the lockstep check with `_bound`'s
    squash-free last step.  Measured on the MI355X: worst |d a| / bound = 0.0424; actions 0.951 .. 1.420 and 6.124 .. 7.073."""
    from gym_sbr2_amd import MlpPolicy
    n = 256
    inputs = _inputs(n, 202)
    layers = _net(71, (32, 32))
    w, b = layers[-1]
    layers[-1] = (w * np.array([0.4, 2.0])[:, None], np.array([1.25, 7.5]) + b)
    pol = MlpPolicy(layers, squash="none")
    assert pol.squash == "none" and pol.width == 32
    assert np.array_equal(pol.act_scale, np.ones(2, np.float32)) and np.array_equal(pol.act_bias, np.zeros(2, np.float32))
    acts, _, worst = _bits_then_lockstep(G, n, inputs, pol)
    a = _np(acts)
    print("squash none: actions %.3f .. %.3f and %.3f .. %.3f, worst |d a| / bound %.4f"
          % (a[..., 0].min(), a[..., 0].max(), a[..., 1].min(), a[..., 1].max(), worst))
    assert 0.9 < a[..., 0].min() and a[..., 0].max() < 1.5 and 6.0 < a[..., 1].min() and a[..., 1].max() < 7.2     # unsquashed, unclipped
    assert float(acts[..., 0].std()) > 1e-3 and float(acts[..., 1].std()) > 1e-3
    assert worst <= 1.0


@pytest.mark.parametrize("scheme,reward", CONFIGS)
def test_schemes_and_rewards_against_the_tape_kernel(G, scheme, reward):
    """The policy builds behind a non-default config - scheme 0 (RK4 x substeps, always the two-waves build), the G2ANET reward (a
    run-time branch of the non-OCI builds) and the operating-cost reward (the OCI builds: their own record load / store, the
    running sum(Kla) row, the terminal phases and the end-of-cycle reward inside the done call) - against the tape kernel of
    the same config on the reported actions: plant, every controller row (C_KLA_SUM and C_QW included), returns and per-call
    rewards bit for bit.  Net 13 (2 x 32 tanh), 256 envs, inputs 202: the oracle in closed loop flags no env under any of the
    four configs, and under "oci" it penalises 134 of the 256 envs on the done call.  Measured on the MI355X: 134 of 256
    done-call rewards below -200 under both schemes (-245.52 .. 0.4811)."""
    from gym_sbr2_amd import _capi
    n = 256
    inputs = _inputs(n, 202)
    pol = _policy(13, (32, 32))

    def handle():
        env = _handle(G, n, scheme, reward)
        env.reset(scenario=inputs[0], rnd=inputs[1])
        return env

    a_env, b_env = handle(), handle()
    assert a_env.query(_capi.Q_ROLLOUT_WAVES) == (2 if scheme == 0 else 1)
    ret_a, acts, rew_a = a_env.rollout_policy(pol, STEPS, return_actions=True, return_rewards=True)
    ret_b, rew_b = b_env.rollout_actions(acts, return_rewards=True)
    _same_state(a_env, b_env)
    assert torch.equal(ret_a, ret_b) and torch.equal(rew_a, rew_b)
    _, c = a_env.get_state()
    assert bool((c[_capi.C_DONE] == 1).all()) and bool((c[_capi.C_STEPS] == STEPS).all()) and bool((c[_capi.C_PLAN] == 0).all())
    assert torch.equal(c[_capi.C_RETURN], ret_a) and bool(torch.isfinite(ret_a).all())
    _no_flags(a_env); _no_flags(b_env)
    assert float(acts[..., 0].std()) > 1e-3 and float(acts[..., 1].std()) > 1e-3
    last = _np(rew_a[STEPS - 1])
    print("scheme %d, %s: done-call reward %.4f .. %.4f, %d of %d below -200" % (scheme, reward, last.min(), last.max(),
                                                                                 (last < -200).sum(), n))
    if reward == "oci":                   # the ammonia penalty of the end-of-cycle reward: both sides occur
        assert (last < -200).any() and (last > -200).any()
    a_env.close(); b_env.close()


def test_population_of_64_wide_nets(G):
    """Two full 2 x 64 nets as a population of 2 x 256 envs, hold 8: the second wave's block starts `stride` = 5 506 floats into
    the parameters.  Each half equals the single-policy run of a 256-env handle with those global ids, bit for bit."""
    from gym_sbr2_amd import MlpPolicy
    n, hold = 512, 8
    inputs = _inputs(n, 202)
    with pytest.warns(RuntimeWarning, match="64-wide"):
        p0, p1 = _policy(53, (64, 64)), _policy(57, (64, 64))
    pop = MlpPolicy.stack([p0, p1], envs_per_policy=256)
    assert pop.width == 64 and pop.block.shape == (2, 5506)
    big = _env(G, n, inputs)
    ret, acts = big.rollout_policy(pop, STEPS, hold=hold, return_actions=True)
    assert acts.shape == (58, n, 2)
    for first, member in ((0, p0), (256, p1)):
        part = _env(G, 256, inputs, first=first)
        r, a = part.rollout_policy(member, STEPS, hold=hold, return_actions=True)
        _same_state(big, part, cols=slice(first, first + 256))
        assert torch.equal(r, ret[first:first + 256]) and torch.equal(a, acts[:, first:first + 256])
        part.close()
    assert not torch.equal(acts[:, :256], acts[:, 256:])
    big.close()


def test_the_reported_actions_are_the_nets(ref):
    """All 463 x 512 x 2 reported actions against the float64 net on sbr_step's observations, each within ITS derived bound
    (`_bound`).  Measured on the MI355X: worst |d a| / bound = 0.0061."""
    print("worst |d a| / bound over %d actions: %.4f" % (STEPS * ref["n"] * 2, ref["worst_ratio"]))
    assert int((ref["status"].to(torch.int64) & FLAGS).count_nonzero()) == 0
    assert ref["worst_ratio"] <= 1.0


def test_hold_and_split_launches(G, ref):
    from gym_sbr2_amd import _capi
    n, hold = 512, 8
    pol = ref["pol"]
    # hold = 8: 58 decisions, and the tape kernel holding those rows 8 calls each leaves the same bits
    inputs = _inputs(n, 303)
    a_env, b_env = _env(G, n, inputs), _env(G, n, inputs)
    ret_a, acts, rew_a = a_env.rollout_policy(pol, STEPS, hold=hold, return_actions=True, return_rewards=True)
    assert acts.shape == (58, n, 2)
    ret_b, rew_b = b_env.rollout_actions(acts, n_steps=STEPS, hold=hold, return_rewards=True)
    _same_state(a_env, b_env)
    assert torch.equal(ret_a, ret_b) and torch.equal(rew_a, rew_b)
    _no_flags(a_env)
    a_env.close(); b_env.close()
    # 200 + 263 calls with obs carried through = one launch of 463
    env = _env(G, n, ref["inputs"])
    r1, a1, w1 = env.rollout_policy(pol, 200, return_actions=True, return_rewards=True)
    o200 = _np(env.obs)
    r2, a2, w2 = env.rollout_policy(pol, 263, return_actions=True, return_rewards=True)
    x, c = env.get_state()
    assert torch.equal(x, ref["x"]) and torch.equal(c, ref["c"])
    assert torch.equal(torch.cat([a1, a2]), ref["acts"]) and torch.equal(torch.cat([w1, w2]), ref["rew"])
    # the carried observation is sbr_step's after call 199, to one float32 ulp per component
    want = _np(ref["obs199"])
    ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(o200)))
    assert np.all(np.abs(o200.astype(np.float64) - want.astype(np.float64)) <= ulp)
    # every env is done now: its obs row stays as the 200-call launch left it ... and a further launch is ignored
    assert torch.equal(env.obs, torch.from_numpy(o200).cuda())
    o_done = env.obs.clone()
    r3, a3, w3 = env.rollout_policy(pol, 3, return_actions=True, return_rewards=True)
    x3, c3 = env.get_state()
    assert bool((r3 == 0).all()) and bool((w3 == 0).all()) and bool((a3 == 0).all())
    assert torch.equal(x3, ref["x"]) and torch.equal(c3, ref["c"]) and torch.equal(env.obs, o_done)
    env.close()
    # n_steps = 470: the calls after the done call are skipped
    env = _env(G, n, ref["inputs"])
    rp, ap, wp = env.rollout_policy(pol, 470, return_actions=True, return_rewards=True)
    x, c = env.get_state()
    assert wp.shape == (470, n) and bool((wp[STEPS:] == 0).all()) and torch.equal(wp[:STEPS], ref["rew"])
    assert torch.equal(ap[:STEPS], ref["acts"]) and torch.equal(rp, ref["ret"]) and torch.equal(x, ref["x"]) and torch.equal(c, ref["c"])
    assert bool((c[_capi.C_DONE] == 1).all())
    env.close()


def test_population(G):
    from gym_sbr2_amd import MlpPolicy, _capi
    n = 512
    inputs = _inputs(n, 202)
    p0, p1 = _policy(23, (32, 32)), _policy(24, (32, 32))
    pop = MlpPolicy.stack([p0, p1], envs_per_policy=256)
    big = _env(G, n, inputs)
    ret, acts = big.rollout_policy(pop, STEPS, return_actions=True)
    _no_flags(big)
    for first, member in ((0, p0), (256, p1)):
        part = _env(G, 256, inputs, first=first)
        r, a = part.rollout_policy(member, STEPS, return_actions=True)
        _same_state(big, part, cols=slice(first, first + 256))
        assert torch.equal(r, ret[first:first + 256]) and torch.equal(a, acts[:, first:first + 256])
        part.close()
    assert not torch.equal(acts[:, :256], acts[:, 256:])
    # the sub-handle running the population picks its member by GLOBAL id
    part = _env(G, 256, inputs, first=256)
    r, a = part.rollout_policy(pop, STEPS, return_actions=True)
    assert torch.equal(r, ret[256:]) and torch.equal(a, acts[:, 256:])
    part.close()
    # a handle that does not start on a workgroup boundary, or reaches past the population, is refused
    odd = _env(G, 256, inputs, first=100)
    with pytest.raises(_capi.SbrError, match="sbr_rollout_policy.*first_env_id"):
        odd.rollout_policy(pop, 5)
    odd.close()
    far = _env(G, 256, (inputs[0][:256], inputs[1][:256]), first=512)
    with pytest.raises(_capi.SbrError, match="sbr_rollout_policy"):
        far.rollout_policy(pop, 5)
    far.close(); big.close()


def test_an_envs_result_does_not_depend_on_the_batch_around_it(G):
    from gym_sbr2_amd import ShardedSbrOS
    n, lo, hi = 4096, 1000, 2024
    inputs = _inputs(n, 404)
    pol = _policy(13, (32, 32))
    big = _env(G, n, inputs)
    obs0 = big.obs.clone()
    ret, acts = big.rollout_policy(pol, STEPS, return_actions=True)
    _no_flags(big)
    part = G.SbrOSVec(hi - lo, first_env_id=lo)
    part.reset(scenario=inputs[0][lo:hi], rnd=inputs[1][lo:hi])
    o = obs0[lo:hi].clone()                                     # its slice of obs, passed explicitly
    r, a = part.rollout_policy(pol, STEPS, obs=o, return_actions=True)
    _same_state(big, part, cols=slice(lo, hi))
    assert torch.equal(r, ret[lo:hi]) and torch.equal(a, acts[:, lo:hi])
    sh = ShardedSbrOS(n, rank=1, world=4, device=0)
    assert (sh.start, sh.stop) == (1024, 2048)
    sh.env.reset(scenario=inputs[0][1024:2048], rnd=inputs[1][1024:2048])
    r, a = sh.rollout_policy(pol, STEPS, obs=obs0[1024:2048].clone(), return_actions=True)
    _same_state(big, sh.env, cols=slice(1024, 2048))
    assert torch.equal(r, ret[1024:2048]) and torch.equal(a, acts[:, 1024:2048])
    big.close(); part.close(); sh.close()


def test_two_waves_build_above_98304_envs_matches_small_handles(G):
    from gym_sbr2_amd import _capi
    n, hold = 98304 + 320, 8                           # not a multiple of 256: the last workgroup is ragged
    inputs = _inputs(n, 505)
    pol = _policy(13, (32, 32))
    assert pol.width == 32
    env = _env(G, n, inputs)
    assert env.query(_capi.Q_ROLLOUT_WAVES) == 2
    ret, acts = env.rollout_policy(pol, STEPS, hold=hold, return_actions=True)
    x, c = env.get_state()
    assert bool((c[_capi.C_DONE] == 1).all()) and bool((c[_capi.C_STEPS] == STEPS).all()) and bool(torch.isfinite(ret).all())
    for first in (0, n // 2 + 37, n - 64):
        small = _env(G, 64, inputs, first=first)
        assert small.query(_capi.Q_ROLLOUT_WAVES) == 1
        rs, as_ = small.rollout_policy(pol, STEPS, hold=hold, return_actions=True)
        xs, cs = small.get_state()
        assert torch.equal(rs, ret[first:first + 64]) and torch.equal(as_, acts[:, first:first + 64])
        assert torch.equal(xs, x[:, first:first + 64]) and torch.equal(cs, c[:, first:first + 64])
        small.close()
    # ... and the H = 64 two-waves build, on the same handle after a reset: the full 2 x 64 tanh net of seed 53, 58 decisions
    with pytest.warns(RuntimeWarning, match="64-wide"):
        wide = _policy(53, (64, 64))
    assert wide.width == 64
    env.reset(scenario=inputs[0], rnd=inputs[1])
    ret_w, acts_w = env.rollout_policy(wide, STEPS, hold=hold, return_actions=True)
    x, c = env.get_state()
    assert bool((c[_capi.C_DONE] == 1).all()) and bool((c[_capi.C_STEPS] == STEPS).all())
    assert not torch.equal(acts_w, acts)
    for first in (0, n // 2 + 37, n - 64):
        small = _env(G, 64, inputs, first=first)
        assert small.query(_capi.Q_ROLLOUT_WAVES) == 1
        rs, as_ = small.rollout_policy(wide, STEPS, hold=hold, return_actions=True)
        xs, cs = small.get_state()
        assert torch.equal(rs, ret_w[first:first + 64]) and torch.equal(as_, acts_w[:, first:first + 64])
        assert torch.equal(xs, x[:, first:first + 64]) and torch.equal(cs, c[:, first:first + 64])
        small.close()
    env.close()


def test_padding_changes_no_bit(G):
    from gym_sbr2_amd import MlpPolicy
    n = 512
    inputs = _inputs(n, 202)
    layers = _net(33, (20, 20))
    narrow = MlpPolicy(layers, low=LOW, high=HIGH)
    assert narrow.width == 32
    padded, fan_in = [], 18
    for k, (w, b) in enumerate(layers):                 # the same net, padded to 64 by hand
        out = 2 if k == 2 else 64
        wp, bp = np.zeros((out, fan_in)), np.zeros(out)
        wp[:w.shape[0], :w.shape[1]] = w; bp[:b.shape[0]] = b
        padded.append((wp, bp)); fan_in = out
    wide = MlpPolicy(padded, low=LOW, high=HIGH)
    assert wide.width == 64
    a_env, b_env = _env(G, n, inputs), _env(G, n, inputs)
    ra, aa = a_env.rollout_policy(narrow, STEPS, return_actions=True)
    rb, ab = b_env.rollout_policy(wide, STEPS, return_actions=True)
    assert torch.equal(aa, ab) and torch.equal(ra, rb)
    _same_state(a_env, b_env)
    _no_flags(a_env)
    a_env.close(); b_env.close()


def test_noise(G):
    n, calls, std = 512, 64, (0.05, 0.3)
    inputs = _inputs(n, 202)
    pol = _policy(13, (32, 32))

    def run(seed, first=0, m=n):
        env = _env(G, m, inputs, first=first)
        out = env.rollout_policy(pol, calls, noise_std=std, noise_seed=seed, return_actions=True)
        x, c = env.get_state()
        env.close()
        return out + (x, c)

    r1, a1, x1, c1 = run(7)
    r2, a2, x2, c2 = run(7)
    assert torch.equal(a1, a2) and torch.equal(r1, r2) and torch.equal(x1, x2) and torch.equal(c1, c2)
    r3, a3, _, _ = run(8)
    assert not torch.equal(a1, a3)
    rs, as_, xs, cs = run(7, first=256, m=256)          # keyed by the GLOBAL env id
    assert torch.equal(as_, a1[:, 256:]) and torch.equal(rs, r1[256:]) and torch.equal(xs, x1[:, 256:]) and torch.equal(cs, c1[:, 256:])
    # recover z in lockstep: sbr_step replays the noisy actions, the float64 net gives the means
    c_env = _env(G, n, inputs)
    sd = np.asarray(std)
    z, dz = [], 0.0
    for s in range(calls):
        mean, bound = _bound(pol, _np(c_env.obs))
        a = _np(a1[s]).astype(np.float64)
        z.append((a - mean) / sd)
        dz = max(dz, float(((bound + U * np.abs(a)) / sd).max()))       # + the rounding of the noisy action to float32
        c_env.step(a1[s])
    c_env.close()
    z = np.concatenate(z).ravel()
    cnt = z.size
    assert cnt == calls * n * 2
    print("noise: mean z %.5f (bound %.5f), var z %.5f, recovered to %.2e" % (z.mean(), 5 / np.sqrt(cnt), z.var(), dz))
    assert abs(z.mean()) < 5 / np.sqrt(cnt)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / cnt) + 2 * dz * np.abs(z).mean() + dz * dz


def test_graph_capture(G):
    n = 512
    env = _env(G, n, _inputs(n, 202))
    pol = _policy(13, (32, 32))
    x0, c0 = env.get_state()
    o0 = env.obs.clone()
    o = o0.clone()
    env.set_state(x0, c0)
    ret_e = env.rollout_policy(pol, 20, obs=o)          # eager (also puts the parameter block on the device)
    xe, ce = env.get_state()
    oe = o.clone()
    env.set_state(x0, c0)
    o.copy_(o0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            ret_g = env.rollout_policy(pol, 20, obs=o)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    xg, cg = env.get_state()
    assert torch.equal(xg, xe) and torch.equal(cg, ce) and torch.equal(ret_g, ret_e) and torch.equal(o, oe)
    assert not torch.equal(oe, o0)
    env.close()


def test_float64_handle_uses_its_own_obs_and_leaves_done_rows_alone(G):
    """obs=None on a float64 handle: the observation goes in as float32 and comes back for the envs that are not done; the rows
    of done envs keep their float64 values."""
    n = 256
    inputs = _inputs(n, 202)
    pol = _policy(13, (32, 32))
    e64, e32 = _env(G, n, inputs, out_dtype=torch.float64), _env(G, n, inputs)
    assert e64.obs.dtype == torch.float64
    r64, a64 = e64.rollout_policy(pol, 30, return_actions=True)
    r32, a32 = e32.rollout_policy(pol, 30, return_actions=True)
    assert torch.equal(a64, a32) and torch.equal(r64, r32) and torch.equal(e64.obs, e32.obs.to(torch.float64))
    e64.rollout_policy(pol, STEPS - 31)
    e64.step(torch.zeros(n, 2, device="cuda"))                      # the done call through sbr_step: float64 post-terminal rows
    done_rows = e64.obs.clone()
    assert not torch.equal(done_rows, done_rows.to(torch.float32).to(torch.float64))     # values float32 cannot hold
    e64.rollout_policy(pol, 5)
    assert torch.equal(e64.obs, done_rows)
    e64.close(); e32.close()
