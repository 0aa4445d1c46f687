"""sbr_rollout_actions / SbrOSVec.rollout_actions on the GPU: the fused rollout under the CALLER's action tape against
sbr_rollout (same bits when fed its sampled actions), against sbr_step replaying the tape, and against the C oracle.

Inputs (`_inputs`): influent scenario 4 + global id % 4, the influent's normal draws from a seeded RandomState, float32 actions
u_DO ~ U[0, 2.5], u_EC ~ U[0, 15] (bench.py's physical policy).  With the seeds used here the C oracle raises none of
SBR_ST_NEGATIVE / SBR_ST_NEAR_POLE / SBR_ST_NONFINITE on any env over the 463 calls (checked on the CPU: seed 202 at 512 envs
with hold 1, seed 303 at 512 envs with hold 8, seed 404 at 4096 envs with hold 1), so every comparison with a tolerance covers
ALL envs: the tests assert that no env is flagged and mask nothing out.  (The bit-for-bit comparisons need no such condition.)
Seed 202 at 256 envs with hold 1 was checked in the same way under scheme 0 and scheme 1 (the reward does not enter the plant).

Which test runs which build of k_rollout_tape<ActT, OCI, SCH, WAVES> (the host picks ActT from action_dtype, OCI from reward
"oci", and (SCH, WAVES) = (1, 1) up to 98 304 envs, (1, 2) above, (0, 2) for scheme 0):
  (f32, no, 1, 1)  every test below that is not named here;  its reward "g2anet" branch: test_schemes_and_rewards_...[1-g2anet]
  (f64, no, 1, 1)  test_same_bits_as_sbr_rollout_on_its_sampled_actions[float64]
  (f32, no, 1, 2)  test_two_waves_build_above_98304_envs_matches_small_handles
  (f32, no, 0, 2)  test_schemes_and_rewards_equal_sbr_step_and_the_oracle[0-eqi_oci]
  (f32, yes, 1, 1) test_schemes_and_rewards_equal_sbr_step_and_the_oracle[1-oci]
  (f32, yes, 0, 2) test_schemes_and_rewards_equal_sbr_step_and_the_oracle[0-oci], test_float64_tape_in_the_scheme_0_oci_build
  (f64, yes, 0, 2) test_float64_tape_in_the_scheme_0_oci_build
  (f64, no, 0, 2) and (f64, yes, 1, 1) are covered only through their siblings: the float64 tape in (f64, yes, 0, 2) and
  (f64, no, 1, 1), their plant and reward in the float32 builds of the same config.  (f32, yes, 1, 2), (f64, no, 1, 2) and
  (f64, yes, 1, 2) are not run by any test.
tests/test_policy_rollout_gpu.py runs the f32 builds of the four non-default configs once more, on a policy's actions."""
import numpy as np
import pytest
from conftest import gate
from gpu_common import CONFIGS, FLAGS, STEPS, handle as _handle, inputs as _inputs, no_flags, package, to_np as _np

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import sbr_oracle as O  # noqa: E402  (the checker, never the thing under test)


@pytest.fixture(scope="module")
def G():
    return package()


def _state(env):
    x, c = env.get_state()
    return x, c


def _no_flags(ctrl):
    from gym_sbr2_amd import _capi
    no_flags(ctrl[_capi.C_STATUS])


def test_bad_arguments_are_refused_on_a_live_handle(G):
    from gym_sbr2_amd import _capi
    lib = _capi.load()
    env = G.SbrOSVec(64)
    env.reset(seed=1)
    a = torch.zeros(1, 64, 2, device="cuda")
    ret = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    assert lib.sbr_rollout_actions(env._h, 1, 0, a.data_ptr(), None, None, None) == -1 and b"sbr_rollout_actions" in lib.sbr_last_error(env._h)
    assert lib.sbr_rollout_actions(env._h, -1, 1, a.data_ptr(), None, None, None) == -1
    assert lib.sbr_rollout_actions(env._h, 1, 1, None, None, None, None) == -1
    assert lib.sbr_rollout_actions(None, 1, 1, a.data_ptr(), None, None, None) == -1
    # n_steps = 0: nothing happens to the handle, returns = 0 (also without a tape)
    x0, c0 = _state(env)
    assert lib.sbr_rollout_actions(env._h, 0, 1, None, ret.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    x1, c1 = _state(env)
    assert torch.equal(ret, torch.zeros_like(ret)) and torch.equal(x0, x1) and torch.equal(c0, c1)
    with pytest.raises(ValueError):
        env.rollout_actions(torch.zeros(3, 63, 2))
    with pytest.raises(ValueError):
        env.rollout_actions(a, hold=0)
    env.close()


@pytest.mark.parametrize("tape_dtype", ["float32", "float64"])
def test_same_bits_as_sbr_rollout_on_its_sampled_actions(G, tape_dtype):
    """Both kernels inline the same device functions with the same history type and the library is built with
    -ffp-contract=off: fed the actions sbr_rollout sampled, the tape kernel leaves the same bits - no tolerance.  (The uniform
    policy over the whole action box leaves the model's domain on most envs; bit equality does not care.)"""
    from gym_sbr2_amd import _capi
    n = 512
    scen, rnd, _ = _inputs(n, seed=101, first=1000, rows=1)
    dt = getattr(torch, tape_dtype)
    a_env = G.SbrOSVec(n, first_env_id=1000)
    b_env = G.SbrOSVec(n, first_env_id=1000, action_dtype=dt)
    a_env.reset(scenario=scen, rnd=rnd); b_env.reset(scenario=scen, rnd=rnd)
    ret_a, acts = a_env.rollout(STEPS, policy_seed=11, return_actions=True)
    ret_b = b_env.rollout_actions(acts.to(dt))
    xa, ca = _state(a_env); xb, cb = _state(b_env)
    assert torch.equal(xa, xb)
    for row in range(_capi.NCTRL):                     # every row, the plan row (0 on both) included
        assert torch.equal(ca[row], cb[row]), row
    assert bool((cb[_capi.C_PLAN] == 0).all()) and bool((cb[_capi.C_DONE] == 1).all()) and bool((cb[_capi.C_STEPS] == STEPS).all())
    assert torch.equal(ret_a, ret_b)
    a_env.close(); b_env.close()


def test_equals_sbr_step_and_the_oracle_on_the_callers_tape(G, tables):
    from gym_sbr2_amd import _capi
    means, stds = tables
    n = 512
    scen, rnd, tape = _inputs(n, seed=202, rows=STEPS)
    t_env = G.SbrOSVec(n)
    s_env = G.SbrOSVec(n, out_dtype=torch.float64)
    t_env.reset(scenario=scen, rnd=rnd); s_env.reset(scenario=scen, rnd=rnd)
    dev_tape = torch.from_numpy(tape).cuda()
    ret, rew = t_env.rollout_actions(dev_tape, return_rewards=True)
    assert rew.shape == (STEPS, n) and rew.dtype == torch.float64 and ret.shape == (n,)
    # ---- sbr_step replaying the rows: the bounds of test_gpu_parity.py::test_fused_rollout_equals_step_by_step_and_oracle
    tot = torch.zeros(n, dtype=torch.float64, device="cuda")
    for c in range(STEPS):
        _, _, r, _ = s_env.step(dev_tape[c])
        tot += r
    xt, ct = _state(t_env); xs, cs = _state(s_env)
    _no_flags(ct); _no_flags(cs)
    keep = [r_ for r_ in range(_capi.NCTRL) if r_ != _capi.C_PLAN]
    g_step = gate(_np(xt).T, _np(xs).T).max()
    print("tape vs sbr_step: worst gate %.3e, worst |d return| %.3e" % (g_step, float((ret - tot).abs().max())))
    assert g_step < 1e-6 and torch.allclose(ct[keep], cs[keep], rtol=1e-11, atol=1e-13)
    for row in (_capi.C_T, _capi.C_DONE, _capi.C_STEPS, _capi.C_STATUS):
        assert torch.equal(ct[row], cs[row])
    assert torch.allclose(ret, tot, rtol=0, atol=1e-12)
    assert bool((ct[_capi.C_PLAN] == 0).all()) and bool((ct[_capi.C_DONE] == 1).all())
    # ---- the oracle, free-running on the same float32 values: ALL envs
    ora = O.OracleBatch(n, nthreads=8)
    ora.reset(ora.mix(means, stds, scen, rnd))
    orew = np.empty((STEPS, n))
    for c in range(STEPS):
        _, _, orew[c], od = ora.step(tape[c].astype(np.float64), want_obs=False)
    assert np.all(od == 1) and np.count_nonzero(ora.envs["status"].astype(np.int64) & FLAGS) == 0
    oret = np.zeros(n)
    for c in range(STEPS):
        oret += orew[c]
    d_ret = np.abs(_np(ret) - oret).max()
    g_ora = gate(_np(xt).T, ora.envs["x"]).max()
    d_rew = np.abs(_np(rew) - orew).max()
    print("tape vs oracle: worst |d return| %.3e, worst gate %.3e, worst per-call |d reward| %.3e" % (d_ret, g_ora, d_rew))
    assert d_ret < 1e-10 and g_ora < 1e-6
    # per-call rewards: the float64 device-against-oracle reward bound of the lockstep tests, test_gpu_parity.py:545
    # (test_two_waves_per_simd_kernel_build_matches_oracle: np.abs(_np(r)[pick] - orr).max() < 1e-12)
    assert d_rew < 1e-12
    # ---- rewards_out added in call order IS returns
    acc = np.zeros(n)
    for c in range(STEPS):
        acc = acc + _np(rew[c])
    assert np.array_equal(acc, _np(ret)) and np.array_equal(_np(ct[_capi.C_RETURN]), _np(ret))
    t_env.close(); s_env.close()


OCI_COEF = 8.000000000006622 / 1800 * 1.32 * (0.002 / 24)      # d(end-of-cycle reward) / d(sum(Kla)), test_gpu_parity.py::test_oci_reward_option


@pytest.mark.parametrize("scheme,reward", CONFIGS)
def test_schemes_and_rewards_equal_sbr_step_and_the_oracle(G, tables, scheme, reward):
    """test_equals_sbr_step_and_the_oracle_on_the_callers_tape for the tape builds behind a non-default config: scheme 0 (RK4 x
    substeps, always the two-waves build), the G2ANET reward (a run-time branch of the non-OCI builds) and the operating-cost
    reward (the OCI builds: their own record load / store, the running sum(Kla) row, the terminal phases and the end-of-cycle
    reward inside the done call).  256 envs, a float32 tape of seed 202, a whole episode; sbr_step and the oracle run the same
    config.  Checked on the CPU: under both schemes the oracle flags no env on this tape.

    eqi_oci, g2anet: the bounds of test_equals_sbr_step_and_the_oracle_on_the_callers_tape, unchanged.
    oci: against sbr_step the same gate and rows, |return - sum| < 1e-8; against the oracle every number of
    test_gpu_parity.py::test_oci_reward_option, all 256 envs being "clean" here: per-call reward within 1e-10 on calls 0 .. 461;
    on the done call the same envs penalised, |d reward| < 1e-8, sum(Kla) within 1e-6 relative, |d Qw| < 1e-8, and with those
    two differences removed the rewards equal to 1e-12 (the formula is the same).  The penalty is -246 where the effluent
    ammonia (Snh before settling) is >= 4.  On the tape of seed 202 the oracle penalises 178 of the 256 envs under either
    scheme (the other rewards are >= 0.47) and no env's Snh is closer to 4 than 3.47e-3 relative (scheme 1: 3.472e-3, scheme 0:
    3.473e-3; oracle with cfg.terminal = 0, on the CPU), 347 times the state gate's 1e-5: the comparison cannot flip.
    Measured on the MI355X (every bound above holds under scheme 0 as it stands):
      against sbr_step  state, every row and the returns equal bit for bit under (1, g2anet), (1, oci), (0, oci);
                        (0, eqi_oci): gate 0, |d return| and worst row difference 1.6e-15
      against the oracle, scheme 1: gate 2.1e-9; |d return| g2anet 6.8e-13, oci 2.8e-14; per-call |d reward| 2.9e-15, 5.6e-17
                          scheme 0: gate 9.2e-9; |d return| eqi_oci 3.9e-14, oci 2.8e-14; per-call |d reward| 2.2e-16, 5.6e-17
      oci done call, 178 envs penalised on both sides:  scheme 1  |d reward| 2.2e-16, sum(Kla) 2.9e-15 relative, |d Qw| 4.8e-15,
                          formula 2.6e-16;  scheme 0  |d reward| 2.8e-14, sum(Kla) 9.2e-15, |d Qw| 2.5e-14, formula 2.7e-14."""
    from gym_sbr2_amd import _capi
    means, stds = tables
    n = 256
    oci = reward == "oci"
    scen, rnd, tape = _inputs(n, seed=202, rows=STEPS)
    t_env = _handle(G, n, scheme, reward)
    s_env = _handle(G, n, scheme, reward, out_dtype=torch.float64)
    t_env.reset(scenario=scen, rnd=rnd); s_env.reset(scenario=scen, rnd=rnd)
    dev_tape = torch.from_numpy(tape).cuda()
    ret, rew = t_env.rollout_actions(dev_tape, return_rewards=True)
    assert rew.shape == (STEPS, n) and rew.dtype == torch.float64 and ret.shape == (n,)
    # ---- sbr_step replaying the rows
    tot = torch.zeros(n, dtype=torch.float64, device="cuda")
    for c in range(STEPS):
        _, _, r, _ = s_env.step(dev_tape[c])
        tot += r
    xt, ct = _state(t_env); xs, cs = _state(s_env)
    _no_flags(ct); _no_flags(cs)
    keep = [r_ for r_ in range(_capi.NCTRL) if r_ != _capi.C_PLAN]
    g_step = gate(_np(xt).T, _np(xs).T).max()
    d_tot = float((ret - tot).abs().max())
    print("scheme %d, %s: tape vs sbr_step: worst gate %.3e, worst |d return| %.3e, worst row difference %.3e (relative %.3e)"
          % (scheme, reward, g_step, d_tot, float((ct[keep] - cs[keep]).abs().max()),
             float(((ct[keep] - cs[keep]).abs() / cs[keep].abs().clamp_min(1e-300)).max())))
    assert g_step < 1e-6 and torch.allclose(ct[keep], cs[keep], rtol=1e-11, atol=1e-13)
    for row in (_capi.C_T, _capi.C_DONE, _capi.C_STEPS, _capi.C_STATUS):
        assert torch.equal(ct[row], cs[row])
    if oci:                               # the done call's reward carries the two free-running quantities (test_oci_reward_option)
        assert d_tot < 1e-8
    else:
        assert torch.allclose(ret, tot, rtol=0, atol=1e-12)
    assert bool((ct[_capi.C_PLAN] == 0).all()) and bool((ct[_capi.C_DONE] == 1).all())
    # ---- the oracle, free-running on the same float32 values: ALL envs
    par = O.default_params(scheme=scheme); par.reward_kind = _capi.REWARD_KINDS[reward]
    ora = O.OracleBatch(n, par, nthreads=8)
    ora.reset(ora.mix(means, stds, scen, rnd))
    orew = np.empty((STEPS, n))
    for c in range(STEPS):
        _, _, orew[c], od = ora.step(tape[c].astype(np.float64), want_obs=False)
    assert np.all(od == 1) and np.count_nonzero(ora.envs["status"].astype(np.int64) & FLAGS) == 0
    oret = np.zeros(n)
    for c in range(STEPS):
        oret += orew[c]
    d_ret = np.abs(_np(ret) - oret).max()
    g_ora = gate(_np(xt).T, ora.envs["x"]).max()
    calls = STEPS - 1 if oci else STEPS                    # the OCI done call has its own bounds below
    d_rew = np.abs(_np(rew)[:calls] - orew[:calls]).max()
    print("scheme %d, %s: tape vs oracle: worst |d return| %.3e, worst gate %.3e, worst per-call |d reward| %.3e"
          % (scheme, reward, d_ret, g_ora, d_rew))
    assert g_ora < 1e-6
    if not oci:
        assert d_ret < 1e-10 and d_rew < 1e-12
    else:
        assert d_rew < 1e-10
        r, orr = _np(rew)[STEPS - 1], orew[STEPS - 1]
        ks, oks = _np(ct[_capi.C_KLA_SUM]), ora.envs["kla_sum"]
        dqw = _np(ct[_capi.C_QW]) - ora.envs["qw"]
        formula = np.abs((r - orr) + 0.05 * dqw + OCI_COEF * (ks - oks)).max()
        print("scheme %d, oci, done call: %d of %d envs penalised, |d reward| %.3e, sum(Kla) relative %.3e, |d Qw| %.3e, formula "
              "%.3e" % (scheme, (orr < -200).sum(), n, np.abs(r - orr).max(), np.abs(ks / oks - 1).max(), np.abs(dqw).max(), formula))
        assert np.array_equal(r < -200, orr < -200) and (orr < -200).any() and (orr > 0).any() and np.all((orr < -200) | (orr > 0))
        assert oks.min() > 1000.0
        assert np.abs(r - orr).max() < 1e-8 and np.abs(ks / oks - 1).max() < 1e-6 and np.abs(dqw).max() < 1e-8
        assert formula < 1e-12
        assert d_ret < 1e-8 + (STEPS - 1) * 1e-10         # what the bounds on its 463 terms leave for their sum
    # ---- rewards_out added in call order IS returns
    acc = np.zeros(n)
    for c in range(STEPS):
        acc = acc + _np(rew[c])
    assert np.array_equal(acc, _np(ret)) and np.array_equal(_np(ct[_capi.C_RETURN]), _np(ret))
    t_env.close(); s_env.close()


def test_float64_tape_in_the_scheme_0_oci_build(G):
    """action_dtype = float64 with scheme 0 and the operating-cost reward: the tape of the test above cast to float64 leaves the
    bits of the float32-tape handle of the same config - plant, every controller row, returns and per-call rewards.  (Both
    kernels cast the lane's pair to double before anything else, and float32 -> float64 is exact.)"""
    from gym_sbr2_amd import _capi
    n = 256
    scen, rnd, tape = _inputs(n, seed=202, rows=STEPS)
    e32 = _handle(G, n, 0, "oci")
    e64 = _handle(G, n, 0, "oci", action_dtype=torch.float64)
    assert e64.cfg.act_f64 == 1 and e32.cfg.act_f64 == 0
    e32.reset(scenario=scen, rnd=rnd); e64.reset(scenario=scen, rnd=rnd)
    t32 = torch.from_numpy(tape).cuda()
    t64 = t32.to(torch.float64)
    ret32, rew32 = e32.rollout_actions(t32, return_rewards=True)
    ret64, rew64 = e64.rollout_actions(t64, return_rewards=True)
    x32, c32 = _state(e32); x64, c64 = _state(e64)
    assert torch.equal(x32, x64)
    for row in range(_capi.NCTRL):
        assert torch.equal(c32[row], c64[row]), row
    assert torch.equal(ret32, ret64) and torch.equal(rew32, rew64)
    assert bool((c64[_capi.C_DONE] == 1).all()) and bool((c64[_capi.C_STEPS] == STEPS).all())
    last = _np(rew64[STEPS - 1])
    assert (last < -200).any() and (last > 0).any()
    e32.close(); e64.close()


def test_hold_and_split_launches(G):
    from gym_sbr2_amd import _capi
    n, hold = 512, 8
    rows = -(-STEPS // hold)
    assert rows == 58
    scen, rnd, short = _inputs(n, seed=303, rows=rows)
    long_tape = torch.from_numpy(np.repeat(short, hold, axis=0)[:STEPS].copy()).cuda()
    short = torch.from_numpy(short).cuda()
    env = G.SbrOSVec(n)

    def run(f):
        env.reset(scenario=scen, rnd=rnd)
        out = f()
        x, c = _state(env)
        return out, x, c

    (ret_l, rew_l), x_l, c_l = run(lambda: env.rollout_actions(long_tape, return_rewards=True))
    _no_flags(c_l)
    assert bool((c_l[_capi.C_DONE] == 1).all()) and bool((c_l[_capi.C_STEPS] == STEPS).all())
    # hold = 8 with the 58-row tape = the 463-row tape that repeats each row 8 times, bit for bit
    (ret_h, rew_h), x_h, c_h = run(lambda: env.rollout_actions(short, n_steps=STEPS, hold=hold, return_rewards=True))
    assert torch.equal(x_h, x_l) and torch.equal(c_h, c_l) and torch.equal(ret_h, ret_l) and torch.equal(rew_h, rew_l)
    # two launches = one launch (the row index is launch-relative: the second launch gets the rest of the tape)
    ((r1, w1), (r2, w2)), x_2, c_2 = run(lambda: (env.rollout_actions(long_tape[:200], return_rewards=True),
                                                  env.rollout_actions(long_tape[200:], return_rewards=True)))
    assert torch.equal(x_2, x_l) and torch.equal(c_2, c_l)
    assert torch.equal(torch.cat([w1, w2]), rew_l)
    assert torch.equal(r1, _seq_sum(rew_l[:200])) and torch.equal(r2, _seq_sum(rew_l[200:]))
    assert torch.allclose(r1 + r2, ret_l, rtol=0, atol=1e-12)
    # more calls than the episode has: the calls after the done call are skipped
    pad = torch.cat([long_tape, long_tape[:7]])
    (ret_p, rew_p), x_p, c_p = run(lambda: env.rollout_actions(pad, n_steps=470, return_rewards=True))
    assert rew_p.shape == (470, n) and bool((rew_p[STEPS:] == 0).all()) and torch.equal(rew_p[:STEPS], rew_l)
    assert torch.equal(ret_p, ret_l) and bool((c_p[_capi.C_DONE] == 1).all()) and torch.equal(x_p, x_l) and torch.equal(c_p, c_l)
    # a finished env ignores a further launch altogether
    ret_z, rew_z = env.rollout_actions(long_tape[:3], return_rewards=True)
    x_z, c_z = _state(env)
    assert bool((ret_z == 0).all()) and bool((rew_z == 0).all()) and torch.equal(x_z, x_l) and torch.equal(c_z, c_l)
    # too few rows
    with pytest.raises(ValueError):
        env.rollout_actions(short, n_steps=STEPS, hold=7)
    with pytest.raises(ValueError):
        env.rollout_actions(long_tape[:10], n_steps=11)
    env.close()


def _seq_sum(rows):
    """sum over dim 0 in row order, one addition per row (what the kernel's accumulator does)."""
    acc = torch.zeros_like(rows[0])
    for r in rows:
        acc = acc + r
    return acc


def test_an_envs_result_does_not_depend_on_the_batch_around_it(G):
    """A 4096-env handle against a handle holding envs 1000 .. 2023 of it (a cut that is no multiple of 64, so the envs sit in
    other lanes and other workgroups) and against a rank of a sharded batch, each fed its slice of the tape: bit for bit."""
    from gym_sbr2_amd import ShardedSbrOS, _capi
    n, lo, hi = 4096, 1000, 2024
    scen, rnd, tape = _inputs(n, seed=404, rows=STEPS)
    tape = torch.from_numpy(tape).cuda()
    big = G.SbrOSVec(n)
    big.reset(scenario=scen, rnd=rnd)
    ret = big.rollout_actions(tape)
    x, c = _state(big)
    _no_flags(c)
    assert bool((c[_capi.C_DONE] == 1).all())
    part = G.SbrOSVec(hi - lo, first_env_id=lo)
    part.reset(scenario=scen[lo:hi], rnd=rnd[lo:hi])
    ret_p = part.rollout_actions(tape[:, lo:hi])              # a strided view: made contiguous on the way in
    x_p, c_p = _state(part)
    assert torch.equal(ret_p, ret[lo:hi]) and torch.equal(x_p, x[:, lo:hi]) and torch.equal(c_p, c[:, lo:hi])
    sh = ShardedSbrOS(n, rank=1, world=4, device=0)
    assert (sh.start, sh.stop) == (1024, 2048)
    sh.env.reset(scenario=scen[sh.start:sh.stop], rnd=rnd[sh.start:sh.stop])
    ret_s, rew_s = sh.rollout_actions(tape[:, sh.start:sh.stop], return_rewards=True)
    x_s, c_s = _state(sh.env)
    assert torch.equal(ret_s, ret[1024:2048]) and torch.equal(x_s, x[:, 1024:2048]) and torch.equal(c_s, c[:, 1024:2048])
    assert rew_s.shape == (STEPS, 1024)
    big.close(); part.close(); sh.close()


def test_two_waves_build_above_98304_envs_matches_small_handles(G):
    """Above 1.5 waves per SIMD (98 304 envs on the MI355X) the launch runs the 256-register build: a ragged batch of that size
    against 64-env handles with the same global ids (the one-wave build) and their slices of the tape, bit for bit - as
    test_gpu_parity.py::test_configs4_fused_rollout_at_full_size does for sbr_rollout.  58 rows held 8 calls each.  (Holding a
    random set-point pair for 8 calls takes a few envs of a batch this size out of the model's domain - the oracle flags 13 of the
    98 624; bit equality between the two builds does not care, so nothing is asserted about the flags here.)"""
    from gym_sbr2_amd import _capi
    n, hold = 98304 + 320, 8                           # not a multiple of 256: the last workgroup is ragged
    scen, rnd, tape = _inputs(n, seed=505, rows=58)
    tape = torch.from_numpy(tape).cuda()
    env = G.SbrOSVec(n)
    assert env.query(_capi.Q_ROLLOUT_WAVES) == 2
    env.reset(scenario=scen, rnd=rnd)
    ret, rew = env.rollout_actions(tape, n_steps=STEPS, hold=hold, return_rewards=True)
    x, c = _state(env)
    assert bool((c[_capi.C_DONE] == 1).all()) and bool((c[_capi.C_STEPS] == STEPS).all()) and bool(torch.isfinite(ret).all())
    assert torch.equal(c[_capi.C_RETURN], ret)
    for first in (0, n // 2 + 37, n - 64):
        small = G.SbrOSVec(64, first_env_id=first)
        assert small.query(_capi.Q_ROLLOUT_WAVES) == 1
        small.reset(scenario=scen[first:first + 64], rnd=rnd[first:first + 64])
        rs, ws = small.rollout_actions(tape[:, first:first + 64], n_steps=STEPS, hold=hold, return_rewards=True)
        xs, cs = _state(small)
        assert torch.equal(rs, ret[first:first + 64]) and torch.equal(xs, x[:, first:first + 64]) and torch.equal(cs, c[:, first:first + 64])
        assert torch.equal(ws, rew[:, first:first + 64])
        small.close()
    env.close()
