"""sbr_lookahead_actions / SbrOSVec.lookahead on the GPU: K action tapes per env, each played from the live handle's current
state, the handle left bit for bit as it was.

The checker throughout is the EXISTING tape kernel on a second handle B of N*K envs (`_checker`): B is reset with A's influent
repeated K times, given A's state (get_state -> repeat_interleave -> set_state) and run through rollout_actions on the tape
reshaped to [R, N*K, 2].  Both kernels inline the same device functions and the library is built with -ffp-contract=off, so
returns and per-call rewards are compared with torch.equal - no tolerance anywhere in this file.

Which test runs which build of k_lookahead_tape<ActT, OCI, SCH, WAVES> (ActT from action_dtype, OCI from reward "oci", (SCH, WAVES)
= (1, 1) up to 98 304 BRANCHES, (1, 2) above, (0, 2) for scheme 0):
  (f32, no, 1, 1)   every test below that is not named here
  (f32, yes, 1, 1)  test_past_the_episode_end[oci]
  (f64, no, 1, 1)   test_other_builds_equal_the_tape_kernel[float64-tape]
  (f32, no, 0, 2)   test_other_builds_equal_the_tape_kernel[scheme-0]
  (f32, no, 1, 2)   test_other_builds_equal_the_tape_kernel[two-waves-by-branches]
The other seven builds differ from these in template arguments the kernel only passes on to the shared device functions
(tests/test_tape_rollout_gpu.py runs those under every argument) and are not run here."""
import numpy as np
import pytest
from gpu_common import STEPS, host_best as _host_best, live as _live, package, tape as _tape

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return package()


def _checker(G, a_env, tape, n_steps, hold, **kw):
    """The tape kernel on a handle of N*K envs holding A's state K times: returns [N, K], rewards [n_steps, N, K]."""
    rows, n, k = tape.shape[:3]
    b_env = G.SbrOSVec(n * k, **kw)
    b_env.reset(influent=a_env.influent().T.repeat_interleave(k, dim=0))
    x, c = a_env.get_state()
    b_env.set_state(x.repeat_interleave(k, dim=1), c.repeat_interleave(k, dim=1))
    ret, rew = b_env.rollout_actions(tape.reshape(rows, n * k, 2), n_steps=n_steps, hold=hold, return_rewards=True)
    torch.cuda.synchronize()
    b_env.close()
    return ret.reshape(n, k), rew.reshape(n_steps, n, k)


def _same(a, b):
    """torch.equal with NaN equal to NaN (a NaN plant gives NaN rewards on both sides)."""
    return a.shape == b.shape and bool((torch.isnan(a) == torch.isnan(b)).all()) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def _check_best(ret, bi, br):
    idx, val = _host_best(ret)
    assert bi.dtype == torch.int32 and br.dtype == torch.float64 and bi.shape == br.shape == (ret.shape[0],)
    assert np.array_equal(bi.cpu().numpy(), idx), (bi.cpu().numpy(), idx)
    assert np.array_equal(br.cpu().numpy(), val, equal_nan=True), (br.cpu().numpy(), val)


def test_same_bits_as_the_tape_kernel_and_the_handle_is_untouched(G):
    """N = 5, K = 3: 15 branches in one wave, lanes of different envs side by side, eight-scenario mix.  A stands after 30 step()
    calls; the window of 40 calls under hold = 2 crosses the double-step call 51."""
    from gym_sbr2_amd import _capi
    n, k, n_steps, hold = 5, 3, 40, 2
    a_env, twin = _live(G, n, 30, seed=11), _live(G, n, 30, seed=11)
    tape = _tape(n_steps // hold, n, k, seed=12)
    x0, c0 = a_env.get_state()
    obs0 = a_env.obs.clone()
    assert bool((c0[_capi.C_PLAN] != 0).all()) and bool((c0[_capi.C_STEPS] == 30).all())
    ret, rew, bi, br = a_env.lookahead(tape, hold=hold, return_rewards=True, return_best=True)
    assert ret.shape == (n, k) and ret.dtype == torch.float64 and rew.shape == (n_steps, n, k) and rew.dtype == torch.float64
    x1, c1 = a_env.get_state()
    assert torch.equal(x0, x1) and torch.equal(obs0, a_env.obs)
    for row in range(_capi.NCTRL):                     # every row: the plan, the return and the call count included
        assert torch.equal(c0[row], c1[row]), row
    ret_b, rew_b = _checker(G, a_env, tape, n_steps, hold)
    assert torch.equal(ret, ret_b) and torch.equal(rew, rew_b)
    assert bool((rew != 0).any()) and len(torch.unique(ret)) > 1       # not a comparison of zeros
    _check_best(ret, bi, br)
    # the handle goes on as if nothing had happened: the next step() gives the bits of a twin that never looked ahead
    act = _tape(1, n, 1, seed=13)[0, :, 0]
    outs_a = [t.clone() for t in a_env.step(act)]
    outs_t = twin.step(act)
    for u, v in zip(outs_a, outs_t):
        assert torch.equal(u, v)
    (xa, ca), (xt, ct) = a_env.get_state(), twin.get_state()
    assert torch.equal(xa, xt) and torch.equal(ca, ct)
    a_env.close(); twin.close()


@pytest.mark.parametrize("reward", ["eqi_oci", "oci"])
def test_past_the_episode_end(G, reward):
    """A stands at call 440 of 463: every branch ends with its 23rd call and skips the other 17 (reward 0).  Under reward "oci"
    the end-of-cycle reward is part of the done call, so it is inside the branch return and equals the tape kernel's."""
    from gym_sbr2_amd import _capi
    n, k, n_steps = 6, 3, 40
    a_env = _live(G, n, 440, seed=21, reward=reward)
    tape = _tape(n_steps, n, k, seed=22)
    x0, c0 = a_env.get_state()
    ret, rew = a_env.lookahead(tape, return_rewards=True)
    ret_b, rew_b = _checker(G, a_env, tape, n_steps, 1, reward=reward)
    assert torch.equal(ret, ret_b) and torch.equal(rew, rew_b)
    live = STEPS - 440
    assert bool((rew[live:] == 0).all()) and bool((rew[live - 1] != 0).any())
    assert torch.equal(rew.sum(0), rew[:live].sum(0))
    x1, c1 = a_env.get_state()
    assert torch.equal(x0, x1) and torch.equal(c0, c1)
    assert bool((c1[_capi.C_DONE] == 0).all()) and bool((c1[_capi.C_STEPS] == 440).all())
    a_env.close()


def test_fanout_of_one_equals_rollout_actions_on_a_clone(G):
    n, n_steps = 70, 12
    a_env, clone = _live(G, n, 5, seed=31), _live(G, n, 5, seed=31)
    tape = _tape(n_steps, n, 1, seed=32)
    ret, rew, bi, br = a_env.lookahead(tape, return_rewards=True, return_best=True)
    ret_c, rew_c = clone.rollout_actions(tape[:, :, 0].contiguous(), return_rewards=True)
    assert torch.equal(ret[:, 0], ret_c) and torch.equal(rew[:, :, 0], rew_c)
    assert bool((bi == 0).all()) and torch.equal(br, ret_c)
    a_env.close(); clone.close()


def test_fanout_across_waves_and_best_of_k_with_ties_and_nan(G):
    """N = 4, K = 70: 280 branches - an env's branches straddle wavefronts and the 256-lane workgroup boundary, and the
    winner's reduction strides (70 > 64 lanes).  Env 1: its winning tape is copied to another candidate (an exact tie at the
    maximum).  Env 2: all 70 tapes identical (a 70-way tie: index 0).  Env 3: NaN ammonia injected through set_state."""
    n, k, n_steps = 4, 70, 10
    a_env = _live(G, n, 20, seed=41)
    x, c = a_env.get_state()
    x[10, 3] = float("nan")
    a_env.set_state(x, c)
    tape = _tape(n_steps, n, k, seed=42)
    tape[:, 2, :, :] = tape[:, 2, :1, :]
    first = a_env.lookahead(tape)
    k_win = int(_host_best(first)[0][1])
    k_dup = k_win + 9 if k_win < k - 9 else k_win - 9      # one copy of the winner's tape, above or below it
    tape[:, 1, k_dup, :] = tape[:, 1, k_win, :]
    ret, rew, bi, br = a_env.lookahead(tape, return_rewards=True, return_best=True)
    ret_b, rew_b = _checker(G, a_env, tape, n_steps, 1)
    assert _same(ret, ret_b) and _same(rew, rew_b)
    assert bool(torch.isfinite(ret[:3]).all())
    assert float(ret[1, k_dup]) == float(ret[1, k_win]) and bool((ret[2] == ret[2, 0]).all())
    _check_best(ret, bi, br)
    assert int(bi[1]) == min(k_win, k_dup) and int(bi[2]) == 0
    # one of the pair alone is allowed next to returns (the C call below passes best_index only)
    from gym_sbr2_amd import _capi
    only = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ret2 = torch.empty_like(ret)
    assert _capi.load().sbr_lookahead_actions(a_env._h, n_steps, 1, k, tape.data_ptr(), ret2.data_ptr(), None, only.data_ptr(), None,
                                              None) == 0
    torch.cuda.synchronize()
    assert torch.equal(only, bi) and _same(ret2, ret)
    a_env.close()


@pytest.mark.parametrize("build", ["float64-tape", "scheme-0", "two-waves-by-branches"])
def test_other_builds_equal_the_tape_kernel(G, build):
    from gym_sbr2_amd import _capi
    kw, n, k, calls, n_steps = {}, 37, 2, 25, 30
    if build == "float64-tape":
        kw = {"action_dtype": torch.float64}
    elif build == "scheme-0":
        cfg = _capi.default_config()
        cfg.scheme = 0
        kw = {"config": cfg}
    else:
        # 1541 x 64 = 98 624 branches: above the 98 304 lanes the one-wave build serves, while the HANDLE's 1541 envs are far
        # below it - the budget goes by the branches
        n, k, calls, n_steps = 1541, 64, 25, 20
    a_env = _live(G, n, calls, seed=51, **kw)
    if build == "two-waves-by-branches":
        assert a_env.query(_capi.Q_ROLLOUT_WAVES) == 1 and n * k > a_env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS)
    tape = _tape(n_steps, n, k, seed=52, dtype=a_env.action_dtype)
    x0, c0 = a_env.get_state()
    ret, rew, bi, br = a_env.lookahead(tape, return_rewards=True, return_best=True)
    ret_b, rew_b = _checker(G, a_env, tape, n_steps, 1, **kw)
    assert torch.equal(ret, ret_b) and torch.equal(rew, rew_b)
    _check_best(ret, bi, br)
    x1, c1 = a_env.get_state()
    assert torch.equal(x0, x1) and torch.equal(c0, c1)
    a_env.close()


def test_refusals_on_a_live_handle(G):
    from gym_sbr2_amd import _capi
    lib = _capi.load()
    n, k = 8, 3
    a_env = _live(G, n, 3, seed=61)
    tape = _tape(4, n, k, seed=62)
    with pytest.raises(ValueError, match=r"\[R,N,K,2\]"):
        a_env.lookahead(tape[:, :7])                                  # N - 1 envs
    with pytest.raises(ValueError, match=r"\[R,N,K,2\]"):
        a_env.lookahead(tape.reshape(4, n * k, 2))                    # the tape kernel's shape
    with pytest.raises(ValueError, match="9 calls with hold=2 need 5 rows of actions, got 4"):
        a_env.lookahead(tape, n_steps=9, hold=2)
    with pytest.raises(ValueError):
        a_env.lookahead(tape, hold=0)
    x0, c0 = a_env.get_state()
    ret = torch.full((n, k), 7.0, dtype=torch.float64, device="cuda")
    bi = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    br = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    call = lib.sbr_lookahead_actions
    assert call(a_env._h, 4, 1, 0, tape.data_ptr(), ret.data_ptr(), None, bi.data_ptr(), br.data_ptr(), None) == -1      # fanout = 0
    assert b"sbr_lookahead_actions" in lib.sbr_last_error(a_env._h)
    assert call(a_env._h, 4, 1, 2 ** 28, tape.data_ptr(), ret.data_ptr(), None, None, None, None) == -1                  # 8 x 2^28 = 2^31 branches
    assert call(a_env._h, 4, 1, k, tape.data_ptr(), None, None, bi.data_ptr(), None, None) == -1                         # half an answer
    torch.cuda.synchronize()
    x1, c1 = a_env.get_state()
    assert torch.equal(x0, x1) and torch.equal(c0, c1)
    assert bool((ret == 7.0).all()) and bool((bi == 7).all()) and bool((br == 7.0).all())
    # n_steps = 0: returns 0, winner 0 with return 0, no tape needed, the handle as it was
    assert call(a_env._h, 0, 1, k, None, ret.data_ptr(), None, bi.data_ptr(), br.data_ptr(), None) == 0
    torch.cuda.synchronize()
    x1, c1 = a_env.get_state()
    assert bool((ret == 0).all()) and bool((bi == 0).all()) and bool((br == 0).all()) and torch.equal(x0, x1) and torch.equal(c0, c1)
    a_env.close()
