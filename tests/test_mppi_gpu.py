"""sbr_lookahead_sampled / sbr_mppi_update on the GPU: candidate tapes drawn in the lane that integrates them, and the MPPI update
of the nominal tape with the candidates drawn again.

The checker of the sampled lookahead is the EXISTING lookahead (`lookahead`, itself pinned bit for bit to the tape kernel by
tests/test_lookahead_gpu.py) fed the new kernel's own actions_out: same inlined device functions, -ffp-contract=off, so returns,
per-call rewards and the winner are compared with torch.equal - no tolerance.  The sample itself is checked against the numpy
Philox4x32-10 + Box-Muller of tests/gpu_common.py, first anchored here to the device's sbr_draw_normals; the update against float64 on the
host, with the bounds derived in the tests' docstrings.

Which test runs which build of k_lookahead_sampled<ActT, OCI, SCH, WAVES> ((SCH, WAVES) = (1, 1) up to 98 304 BRANCHES, (1, 2) above,
(0, 2) for scheme 0):
  (f32, no, 1, 1)   every test below that is not named here
  (f64, no, 1, 1)   test_the_sample_is_what_the_header_says, test_other_builds[float64-tape], test_update_against_float64_on_the_host[float64]
  (f32, no, 0, 2)   test_other_builds[scheme-0]
  (f32, yes, 1, 1)  test_other_builds[oci-episode-end]
  (f32, no, 1, 2)   test_other_builds[two-waves-by-branches]
The other seven builds differ from these in template arguments the kernel only passes on to the shared device functions and
are not run here.  k_mppi_update<float> and <double> both run in test_update_against_float64_on_the_host."""
import math

import numpy as np
import pytest
from gpu_common import STEPS, live as _live, nominal as _nominal, normal_pair as _normal_pair, package, same as _same

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return package()


def _against_lookahead(env, nominal, fanout, sampler, n_steps, hold):
    """lookahead_sampled with everything asked for, and `lookahead` on its actions_out: every result equal bit for bit.
    Returns (returns, rewards, best_index, best_return, actions)."""
    ret, rew, bi, br, acts = env.lookahead_sampled(nominal, fanout, sampler, n_steps=n_steps, hold=hold, return_rewards=True,
                                                   return_best=True, return_actions=True)
    rows = -(-n_steps // hold)
    assert acts.shape == (rows, env.num_envs, fanout, 2) and acts.dtype == env.action_dtype
    assert ret.shape == (env.num_envs, fanout) and rew.shape == (n_steps, env.num_envs, fanout)
    ret_l, rew_l, bi_l, br_l = env.lookahead(acts, n_steps=n_steps, hold=hold, return_rewards=True, return_best=True)
    assert _same(ret, ret_l) and _same(rew, rew_l) and torch.equal(bi, bi_l) and _same(br, br_l)
    return ret, rew, bi, br, acts


def test_same_bits_as_lookahead_on_its_own_actions_and_the_handle_is_untouched(G):
    """N = 5, K = 3: 15 branches in one wave, lanes of different envs side by side, eight-scenario mix.  The handle stands after 30
    step() calls; 40 calls under hold = 2 cross the double-step call 51."""
    from gym_sbr2_amd import TapeSampler, _capi
    n, k, n_steps, hold = 5, 3, 40, 2
    a_env, twin = _live(G, n, 30, seed=11), _live(G, n, 30, seed=11)
    nominal = _nominal(n_steps // hold, n, seed=12)
    x0, c0 = a_env.get_state()
    obs0 = a_env.obs.clone()
    assert bool((c0[_capi.C_PLAN] != 0).all()) and bool((c0[_capi.C_STEPS] == 30).all())
    ret, rew, bi, br, acts = _against_lookahead(a_env, nominal, k, TapeSampler((0.3, 2.0), seed=5), n_steps, hold)
    assert ret.dtype == torch.float64 and rew.dtype == torch.float64 and bi.dtype == torch.int32
    x1, c1 = a_env.get_state()
    assert torch.equal(x0, x1) and torch.equal(obs0, a_env.obs)
    for row in range(_capi.NCTRL):                     # every row: the plan, the return and the call count included
        assert torch.equal(c0[row], c1[row]), row
    assert bool((rew != 0).any()) and len(torch.unique(ret)) > 1       # not a comparison of zeros
    assert len(torch.unique(acts[:, 0, :, 0])) > k                     # ... nor of one tape: the candidates differ by row and k
    # the handle goes on as if nothing had happened: the next step() gives the bits of a twin that never looked ahead
    act = _nominal(1, n, seed=13)[0]
    outs_a = [t.clone() for t in a_env.step(act)]
    outs_t = twin.step(act)
    for u, v in zip(outs_a, outs_t):
        assert torch.equal(u, v)
    (xa, ca), (xt, ct) = a_env.get_state(), twin.get_state()
    assert torch.equal(xa, xt) and torch.equal(ca, ct)
    a_env.close(); twin.close()


def test_the_sample_is_what_the_header_says(G):
    """z = a - nominal on a float64-action handle (nominal = (1, 5), sigma = (1, 1), clamps far away) against the numpy generator
    above: counter (r, 4 + 256 k, g_lo, g_hi), key seed.  |dz| <= 1e-12: the device's double log, sqrt and sincos are good to a
    few ulp and |z| < 9, and a - 1 or a - 5 loses at most half an ulp of |a| < 16 (2e-15) - an honest difference is near 1e-14,
    a wrong counter word is off by O(1).  The ids straddle 2^32, so the high id word is in the counter too."""
    from gym_sbr2_amd import TapeSampler
    n, k, rows, first, seed = 6, 5, 3, 2 ** 32 - 3, (5 << 32) + 1234
    env = _live(G, n, 2, seed=21, first=first, action_dtype=torch.float64)
    gid = first + np.arange(n)
    # the numpy generator first, against the device's own stream-0 draws (sbr_draw_normals: pair p of an env = block (p, 0, id))
    z_dev = env.draw_normals(seed).cpu().numpy()
    z0, z1 = _normal_pair(np.arange(24)[None, :], 0, gid[:, None], seed)
    assert np.abs(z_dev[:, 0::2] - z0).max() <= 1e-12 and np.abs(z_dev[:, 1::2] - z1).max() <= 1e-12
    nominal = torch.tensor([1.0, 5.0], dtype=torch.float64, device="cuda").expand(rows, n, 2).contiguous()
    wide = TapeSampler((1.0, 1.0), seed=seed, lo=(-100.0, -100.0), hi=(100.0, 100.0), keep_nominal=False)
    acts = env.lookahead_sampled(nominal, k, wide, return_actions=True)[1]
    z = (acts - nominal[:, :, None, :]).cpu().numpy()                  # [rows, n, k, 2]
    z0, z1 = _normal_pair(np.arange(rows)[:, None, None], 4 + 256 * np.arange(k)[None, None, :], gid[None, :, None], seed)
    print("max |dz|: %.3g %.3g" % (np.abs(z[..., 0] - z0).max(), np.abs(z[..., 1] - z1).max()))
    assert np.abs(z[..., 0] - z0).max() <= 1e-12 and np.abs(z[..., 1] - z1).max() <= 1e-12
    assert np.abs(z).max() > 1.0
    # a float32 handle's candidates are the float64 handle's cast to float32 (nominal, lo, hi float32-representable; the clamps
    # now bite: rounding to float32 is monotonic, so clamping before or after it is the same)
    tight = TapeSampler((1.0, 1.0), seed=seed, lo=(0.5, 0.0), hi=(1.5, 5.5), keep_nominal=False)
    env32 = _live(G, n, 1, seed=22, first=first)
    a64 = env.lookahead_sampled(nominal, k, tight, return_actions=True)[1]
    a32 = env32.lookahead_sampled(nominal.to(torch.float32), k, tight, return_actions=True)[1]
    assert a32.dtype == torch.float32 and torch.equal(a32, a64.to(torch.float32))
    assert bool((a64[..., 0] == 0.5).any()) and bool((a64[..., 0] == 1.5).any()) and bool((a64[..., 1] == 5.5).any())
    env.close(); env32.close()


def test_the_sample_is_independent_of_n_fanout_hold_state_and_shard(G):
    """A: 70 envs from id 0, K = 5, hold 1, 3 calls in.  B: the envs 64 .. 69 alone, K = 3, hold 3, 9 calls in.  The candidates of
    (g, k < 3, r) are the same bits."""
    from gym_sbr2_amd import TapeSampler
    rows = 4
    a_env, b_env = _live(G, 70, 3, seed=31), _live(G, 6, 9, seed=32, first=64)
    nominal = _nominal(rows, 70, seed=33)
    sm = TapeSampler((0.4, 3.0), seed=77, keep_nominal=False)
    acts_a = a_env.lookahead_sampled(nominal, 5, sm, return_actions=True)[1]
    acts_b = b_env.lookahead_sampled(nominal[:, 64:].contiguous(), 3, sm, hold=3, return_actions=True)[1]
    assert acts_b.shape == (rows, 6, 3, 2) and torch.equal(acts_a[:, 64:, :3], acts_b)
    assert len(torch.unique(acts_b)) > rows * 6 * 3
    a_env.close(); b_env.close()


def test_clamp_keep_nominal_and_zero_sigma(G):
    """K = 70: an env's branches cross wavefronts and the 256-lane workgroup boundary.  The nominal tape is partly outside
    [lo, hi]."""
    from gym_sbr2_amd import TapeSampler
    n, k, rows = 4, 70, 6
    lo, hi = (0.5, 1.0), (2.0, 12.0)
    env = _live(G, n, 60, seed=41)                     # in the aerated phase: the returns depend on the set-points
    nominal = _nominal(rows, n, seed=42, lo=(-1.0, -3.0), hi=(4.0, 20.0))
    lo_t, hi_t = torch.tensor(lo, device="cuda"), torch.tensor(hi, device="cuda")
    clamped = torch.maximum(torch.minimum(nominal, hi_t), lo_t)
    assert bool((clamped != nominal).any()) and bool((clamped == nominal).any())
    ret, _, _, _, acts = _against_lookahead(env, nominal, k, TapeSampler((0.3, 2.0), seed=9, lo=lo, hi=hi), rows, 1)
    assert torch.equal(acts[:, :, 0], clamped)                         # candidate 0: the nominal tape itself, clamped
    assert torch.equal(ret[:, 0], env.lookahead(clamped[:, :, None, :].contiguous())[:, 0])
    assert bool((acts >= lo_t).all()) and bool((acts <= hi_t).all())
    assert bool((acts[..., 0] == lo[0]).any()) and bool((acts[..., 1] == hi[1]).any()) and len(torch.unique(ret)) > n
    # sigma = 0: every candidate is the clamped nominal tape, every return the same
    ret0, acts0 = env.lookahead_sampled(nominal, k, TapeSampler(0.0, seed=9, lo=lo, hi=hi, keep_nominal=False), return_actions=True)
    assert torch.equal(acts0, clamped[:, :, None, :].expand(rows, n, k, 2)) and torch.equal(ret0, ret[:, :1].expand(n, k))
    # keep_nominal = False: candidate 0 is perturbed like the others, the others are what they were
    acts1 = env.lookahead_sampled(nominal, k, TapeSampler((0.3, 2.0), seed=9, lo=lo, hi=hi, keep_nominal=False), return_actions=True)[1]
    assert bool((acts1[:, :, 0] != clamped).any()) and torch.equal(acts1[:, :, 1:], acts[:, :, 1:])
    env.close()


@pytest.mark.parametrize("build", ["float64-tape", "scheme-0", "oci-episode-end", "two-waves-by-branches"])
def test_other_builds(G, build):
    from gym_sbr2_amd import TapeSampler, _capi
    kw, n, k, calls, n_steps = {}, 37, 2, 25, 30
    if build == "float64-tape":
        kw = {"action_dtype": torch.float64}
    elif build == "scheme-0":
        cfg = _capi.default_config()
        cfg.scheme = 0
        kw = {"config": cfg}
    elif build == "oci-episode-end":
        # the handle stands at call 440 of 463: every branch ends with its 23rd call, the end-of-cycle reward inside it
        kw, n, k, calls, n_steps = {"reward": "oci"}, 6, 3, 440, 40
    else:
        # 1541 x 64 = 98 624 branches: above the 98 304 lanes the one-wave build serves, the handle's 1541 envs far below
        n, k, calls, n_steps = 1541, 64, 25, 4
    env = _live(G, n, calls, seed=51, **kw)
    if build == "two-waves-by-branches":
        assert env.query(_capi.Q_ROLLOUT_WAVES) == 1 and n * k > env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS)
    nominal = _nominal(n_steps, n, seed=52, dtype=env.action_dtype)
    x0, c0 = env.get_state()
    ret, rew, _, _, _ = _against_lookahead(env, nominal, k, TapeSampler((0.3, 2.0), seed=3), n_steps, 1)
    assert bool((rew != 0).any()) and len(torch.unique(ret)) > 1
    if build == "oci-episode-end":
        live = STEPS - 440
        assert bool((rew[live:] == 0).all()) and bool((rew[live - 1] != 0).any())
    x1, c1 = env.get_state()
    assert torch.equal(x0, x1) and torch.equal(c0, c1)
    env.close()


def _host_update(acts, ret, temperature):
    """Weights [N, K] and u [R, N, 2] in float64 on the host, every sum exact (math.fsum) and rounded once."""
    a, r = acts.double().cpu().numpy(), ret.cpu().numpy()
    key = np.where(np.isnan(r), -np.inf, r)
    m = key.max(axis=1)
    inv = 1.0 / temperature
    w = np.zeros_like(key)
    u = np.full((a.shape[0], a.shape[1], 2), np.nan)
    for i in range(key.shape[0]):
        if not np.isfinite(m[i]):
            continue
        e = np.exp((key[i] - m[i]) * inv)              # the argument is formed as on the device: same bits
        s = math.fsum(e)
        w[i] = e / s
        for row in range(a.shape[0]):
            for c in range(2):
                u[row, i, c] = math.fsum(e * a[row, i, :, c]) / s
    return w, u


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
def test_update_against_float64_on_the_host(G, dtype):
    """N = 4, K = 70, R = 6; the inputs of the host side are actions_out and the returns.
    weights: the argument of exp is the same bits on both sides, the two exp differ by <= 2 ulp, the device's S adds K such
    terms in 1 + 6 levels: 8 * 2^-52 relative.  Output, float64 tape: K products and a sum of K terms of magnitude <= max|lo, hi|
    under weights that sum to 1: (K + 16) * 2^-52 * max|lo, hi|; float32 tape: one float32 ulp at max|lo, hi| more, because the
    rounding to float32 may flip."""
    from gym_sbr2_amd import TapeSampler
    n, k, rows, temp = 4, 70, 6, 0.5
    lo, hi = (0.0, 0.0), (2.5, 15.0)
    env = _live(G, n, 60, seed=61, action_dtype=dtype)  # in the aerated phase: the returns depend on the set-points
    nominal = _nominal(rows, n, seed=62, dtype=dtype)
    sm = TapeSampler((0.3, 2.0), seed=17, lo=lo, hi=hi)
    ret, bi, _, acts = env.lookahead_sampled(nominal, k, sm, return_best=True, return_actions=True)
    ret = ret.clone()
    ret[2, 5:40:3] = float("nan")                      # env 2: some NaN returns; env 3: nothing but NaN
    ret[3, :] = float("nan")
    out, w = env.mppi_update(nominal, ret, sm, temp, return_weights=True)
    assert out.dtype == dtype and out.shape == nominal.shape and w.shape == (n, k) and w.dtype == torch.float64
    w_h, u_h = _host_update(acts, ret, temp)
    w_d, u_d = w.cpu().numpy(), out.double().cpu().numpy()
    rel = np.abs(w_d[:3] - w_h[:3]) / np.where(w_h[:3] > 0, w_h[:3], 1.0)
    bound = (k + 16) * 2.0 ** -52 * 15.0 + (float(np.spacing(np.float32(15.0))) if dtype == torch.float32 else 0.0)
    err = np.abs(u_d[:, :3] - u_h[:, :3]).max()
    print("weights: max rel %.3g (bound %.3g)   output: max abs %.3g (bound %.3g)" % (rel.max(), 8 * 2.0 ** -52, err, bound))
    assert rel.max() <= 8 * 2.0 ** -52 and err <= bound
    assert np.all(w_d[2, 5:40:3] == 0.0) and abs(w_d[2].sum() - 1.0) < 1e-14 and np.all(w_d[:2] > 0)
    assert len(np.unique(w_d[0])) > 1                                  # not a uniform average
    assert np.all(w_d[3] == 0.0) and torch.equal(out[:, 3], nominal[:, 3])      # no finite maximum: the tape bit for bit
    assert bool((out[:, :3] >= torch.tensor(lo, device="cuda")).all()) and bool((out[:, :3] <= torch.tensor(hi, device="cuda")).all())
    # temperature -> 0 with a unique maximum: the tape of the winner, bit for bit
    good = ret[:3]
    top = good.nan_to_num(nan=-math.inf).max(dim=1)
    assert all(int((good[i] == top.values[i]).sum()) == 1 for i in range(3)) and torch.equal(top.indices[:2].int(), bi[:2])
    cold, w_c = env.mppi_update(nominal, ret, sm, 1e-300, return_weights=True)
    for i in range(3):
        assert torch.equal(cold[:, i], acts[:, i, int(top.indices[i])]), i
        assert float(w_c[i, int(top.indices[i])]) == 1.0 and float(w_c[i].sum()) == 1.0
    # temperature -> inf: the weights are exactly 1 / K (envs without a NaN)
    w_u = env.mppi_update(nominal, ret, sm, 1e300, return_weights=True)[1]
    assert bool((w_u[:2] == 1.0 / k).all())
    # shift: output row r is u[min(r + shift, rows - 1)]; in place gives the bits of out of place
    for shift in (0, 1, rows, rows + 3):
        exp = out[torch.clamp(torch.arange(rows) + shift, max=rows - 1).cuda()]
        got = env.mppi_update(nominal, ret, sm, temp, shift=shift)
        assert _same(got, exp), shift
        buf = nominal.clone()
        assert env.mppi_update(buf, ret, sm, temp, shift=shift, out=buf) is buf
        assert _same(buf, exp), shift
    # K = 1: the weight is 1 and the update is the candidate itself
    ret1, acts1 = env.lookahead_sampled(nominal, 1, TapeSampler((0.3, 2.0), seed=17, lo=lo, hi=hi, keep_nominal=False), return_actions=True)
    out1, w1 = env.mppi_update(nominal, ret1, TapeSampler((0.3, 2.0), seed=17, lo=lo, hi=hi, keep_nominal=False), temp, return_weights=True)
    assert torch.equal(out1, acts1[:, :, 0]) and bool((w1 == 1.0).all()) and bool((out1 != nominal).any())
    env.close()


def test_update_is_independent_of_position(G):
    """The envs 64 .. 69 inside a handle of 70 and alone in a handle of 6 that starts at id 64: same returns, same arguments,
    same bits.  The update reads nothing of the plant, so the handles are not even reset."""
    from gym_sbr2_amd import TapeSampler
    rows, k = 4, 70
    a_env, b_env = G.SbrOSVec(70), G.SbrOSVec(6, first_env_id=64)
    nominal = _nominal(rows, 70, seed=71)
    ret = torch.from_numpy(np.random.RandomState(72).uniform(-3, 3, (70, k))).cuda()
    sm = TapeSampler((0.3, 2.0), seed=23)
    out_a, w_a = a_env.mppi_update(nominal, ret, sm, 0.7, shift=1, return_weights=True)
    out_b, w_b = b_env.mppi_update(nominal[:, 64:].contiguous(), ret[64:].contiguous(), sm, 0.7, shift=1, return_weights=True)
    assert torch.equal(out_a[:, 64:], out_b) and torch.equal(w_a[64:], w_b)
    assert bool((out_a != nominal).any())
    a_env.close(); b_env.close()


def test_refusals_on_a_live_handle(G):
    import ctypes as C

    from gym_sbr2_amd import TapeSampler, _capi
    lib = _capi.load()
    n, k, rows = 128, 3, 4
    env = _live(G, n, 2, seed=81)
    nominal = _nominal(rows, n, seed=82)
    x0, c0 = env.get_state()
    ret = torch.full((n, k), 7.0, dtype=torch.float64, device="cuda")
    bi = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    br = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    acts = torch.full((rows, n, k, 2), 7.0, device="cuda")
    out = torch.full((rows, n, 2), 7.0, device="cuda")
    wts = torch.full((n, k), 7.0, dtype=torch.float64, device="cuda")
    ok = TapeSampler((0.3, 2.0)).c_struct(env.cfg)
    reserved = TapeSampler((0.3, 2.0)).c_struct(env.cfg)
    reserved.reserved_ = 1
    crossed = TapeSampler((0.3, 2.0), lo=(1.0, 0.0), hi=(0.5, 15.0)).c_struct(env.cfg)
    # 128 x 2^24 = 2^31 branches; 2^24 + 1 candidates; reserved_ = 1; lo > hi
    for fanout, sm, what in ((2 ** 24, ok, b"2^31"), (2 ** 24 + 1, ok, b"2^24"), (k, reserved, b"reserved_"), (k, crossed, b"lo")):
        assert lib.sbr_lookahead_sampled(env._h, rows, 1, fanout, nominal.data_ptr(), C.byref(sm), ret.data_ptr(), None, bi.data_ptr(),
                                         br.data_ptr(), acts.data_ptr(), None) == -1
        msg = lib.sbr_last_error(env._h)
        assert b"sbr_lookahead_sampled" in msg and what in msg, msg
        assert lib.sbr_mppi_update(env._h, rows, fanout, nominal.data_ptr(), C.byref(sm), ret.data_ptr(), 1.0, 0, out.data_ptr(),
                                   wts.data_ptr(), None) == -1
        msg = lib.sbr_last_error(env._h)
        assert b"sbr_mppi_update" in msg and what in msg, msg
    with pytest.raises(ValueError, match=r"\[R,N,2\]"):
        env.lookahead_sampled(nominal[:, :7], k, TapeSampler(1.0))
    with pytest.raises(ValueError, match=r"\[R,N,2\]"):
        env.mppi_update(nominal[:, :7], ret, TapeSampler(1.0), 1.0)
    torch.cuda.synchronize()
    x1, c1 = env.get_state()
    assert torch.equal(x0, x1) and torch.equal(c0, c1)
    assert bool((ret == 7.0).all()) and bool((bi == 7).all()) and bool((br == 7.0).all()) and bool((acts == 7.0).all())
    assert bool((out == 7.0).all()) and bool((wts == 7.0).all())
    # n_steps = 0: zeros, no nominal needed, the handle as it was
    assert lib.sbr_lookahead_sampled(env._h, 0, 1, k, None, C.byref(ok), ret.data_ptr(), None, bi.data_ptr(), br.data_ptr(), None,
                                     None) == 0
    torch.cuda.synchronize()
    x1, c1 = env.get_state()
    assert bool((ret == 0).all()) and bool((bi == 0).all()) and bool((br == 0).all()) and torch.equal(x0, x1) and torch.equal(c0, c1)
    env.close()


def test_mppi_planner(G):
    """3 decisions on 8 envs: each action is the manual lookahead_sampled -> mppi_update composition bit for bit, the handle
    advances only through step(), and a second planner with the same seed on a twin handle agrees."""
    from gym_sbr2_amd import MppiPlanner, TapeSampler, _capi
    n, rows, k, temp = 8, 5, 6, 0.8
    env, twin = _live(G, n, 60, seed=91), _live(G, n, 60, seed=91)
    sampler = TapeSampler((0.3, 2.0), seed=1000, hi=(2.5, 15.0))
    p1, p2 = MppiPlanner(env, rows, k, sampler, temp), MppiPlanner(twin, rows, k, sampler, temp)
    assert p1.nominal.shape == (rows, n, 2) and p1.nominal.dtype == env.action_dtype and p1.decision == 0
    assert bool((p1.nominal == torch.tensor([1.25, 7.5], device="cuda")).all())
    for d in range(3):
        nom = p1.nominal.clone()
        sm = sampler.with_seed(1000 + d)
        ret = env.lookahead_sampled(nom, k, sm)
        manual = env.mppi_update(nom, ret, sm, temp)
        advanced = env.mppi_update(nom, ret, sm, temp, shift=1)
        assert torch.equal(advanced[:-1], manual[1:]) and torch.equal(advanced[-1], manual[-1])
        x0, c0 = env.get_state()
        act, ret_p = p1.plan(return_returns=True)
        x1, c1 = env.get_state()
        assert torch.equal(x0, x1) and torch.equal(c0, c1) and bool((c1[_capi.C_STEPS] == 60 + d).all())
        assert act.shape == (n, 2) and torch.equal(act, manual[0]) and torch.equal(ret_p, ret)
        assert torch.equal(p1.nominal, advanced) and p1.decision == d + 1
        assert bool((act != nom[0]).any())
        act2 = p2.plan()
        assert torch.equal(act2, act) and torch.equal(p2.nominal, p1.nominal)
        o1 = [t.clone() for t in env.step(act)]
        o2 = twin.step(act2)
        assert all(torch.equal(u, v) for u, v in zip(o1, o2))
    env.close(); twin.close()
