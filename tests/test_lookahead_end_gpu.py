"""sbr_lookahead_actions_end / sbr_lookahead_sampled_end / sbr_branch_best on the GPU: the lookahead reports where every branch
ended - observation, state, done flag - and the winner of adjusted returns is a call of its own.

The checker of the end outputs (`_end_checker`) is built on existing guarantees only.  A second handle B of N*K envs holds the
live handle's influent and state K times (get_state -> repeat_interleave -> set_state), is advanced by rollout_actions over the
first n_steps - 1 calls of the tape and then by ONE step() with the action in force on the last call: step's obs, state and done
are the expected obs_end, state_end and done_end of the branches that are not done; a done branch reports zeros.  The lookahead's
branch equals the tape kernel on a clone (tests/test_lookahead_gpu.py), the tape kernel leaves the record in a form k_step
continues from (tests/test_tape_rollout_gpu.py), and the new kernels run k_step's own row writers on the same values; the
library is built with -ffp-contract=off.  So every comparison is torch.equal - no tolerance anywhere in this file (rows of an env
with an injected NaN are compared with NaN equal to NaN).  A second, independent witness for constant tapes is the row
rollout_policy writes back on exit under a net of zero weights.

Which test runs which build of k_lookahead_tape_end / k_lookahead_sampled_end<ActT, OCI, SCH, WAVES> (ActT from action_dtype, OCI
from reward "oci", (SCH, WAVES) = (1, 1) up to 98 304 BRANCHES, (1, 2) above, (0, 2) for scheme 0):
  (f32, no, 1, 1)   every test below that is not named here (both kernels)
  (f32, yes, 1, 1)  test_finished_and_running_branches_in_one_launch[oci] (both kernels)
  (f64, no, 1, 1)   test_other_builds[float64-tape] (both kernels)
  (f32, no, 0, 2)   test_other_builds[scheme-0] (both kernels)
  (f32, no, 1, 2)   test_other_builds[two-waves-by-branches] (both kernels)
The other seven builds of each differ from these in template arguments the kernel only passes on to the shared device functions
(tests/test_tape_rollout_gpu.py runs those under every argument) and are not run here."""
import numpy as np
import pytest
from gpu_common import (STEPS, host_best as _host_best, live as _live, nominal as _nominal, package, same as _same,
                        tape as _tape)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    return package()


def _sampler(seed=5):
    from gym_sbr2_amd.planner import TapeSampler
    return TapeSampler((0.3, 2.0), seed=seed)


def _end_checker(G, a_env, tape, n_steps, hold, **kw):
    """The expected (obs_end [N, K, 18], state_end [N, K, 15], done_end [N, K] bool) of the tapes [R, N, K, 2]: see the file's
    docstring.  step() reports done = 1 also for an env that was done before the call, which is done_end's rule."""
    rows, n, k = tape.shape[:3]
    b_env = G.SbrOSVec(n * k, **kw)
    b_env.reset(influent=a_env.influent().T.repeat_interleave(k, dim=0))
    x, c = a_env.get_state()
    b_env.set_state(x.repeat_interleave(k, dim=1), c.repeat_interleave(k, dim=1))
    flat = tape.reshape(rows, n * k, 2)
    if n_steps > 1:
        b_env.rollout_actions(flat, n_steps=n_steps - 1, hold=hold)
    obs, state, _, done = b_env.step(flat[(n_steps - 1) // hold])
    assert obs.dtype == torch.float32 and state.dtype == torch.float32
    done = done.bool()
    obs = torch.where(done[:, None], torch.zeros_like(obs), obs).reshape(n, k, -1)
    state = torch.where(done[:, None], torch.zeros_like(state), state).reshape(n, k, -1)
    torch.cuda.synchronize()
    b_env.close()
    return obs, state, done.reshape(n, k)


def _ends_are(got, want, same=torch.equal):
    (o, s, d), (ow, sw, dw) = got, want
    assert o.dtype == torch.float32 and s.dtype == torch.float32 and d.dtype == torch.bool
    assert o.shape == ow.shape and s.shape == sw.shape and d.shape == dw.shape
    assert torch.equal(d, dw), (d, dw)
    assert same(o, ow), (o - ow).abs().max()
    assert same(s, sw), (s - sw).abs().max()
    assert bool((o[d] == 0).all()) and bool((s[d] == 0).all())


def _both_kernels(G, a_env, tape, nominal, n_steps, hold, same=torch.equal, **kw):
    """lookahead_end on `tape` and lookahead_sampled_end around `nominal`: the parents' outputs are the parents' bits, the end
    outputs are the checker's (the sampled kernel's on its own actions_out).  Returns lookahead_end's results."""
    k = tape.shape[2]
    out = a_env.lookahead_end(tape, n_steps=n_steps, hold=hold, return_rewards=True, return_best=True)
    old = a_env.lookahead(tape, n_steps=n_steps, hold=hold, return_rewards=True, return_best=True)
    assert len(out) == 7
    for u, v in zip(out[:4], old):
        assert same(u, v)
    _ends_are(out[4:], _end_checker(G, a_env, tape, n_steps, hold, **kw), same)
    sm = _sampler()
    outs = a_env.lookahead_sampled_end(nominal, k, sm, n_steps=n_steps, hold=hold, return_rewards=True, return_best=True,
                                       return_actions=True)
    olds = a_env.lookahead_sampled(nominal, k, sm, n_steps=n_steps, hold=hold, return_rewards=True, return_best=True,
                                   return_actions=True)
    assert len(outs) == 8
    for u, v in zip(outs[:5], olds):
        assert same(u, v)
    _ends_are(outs[5:], _end_checker(G, a_env, outs[4], n_steps, hold, **kw), same)
    return out


def test_one_wave_mixed_envs_and_the_handle_is_untouched(G):
    """N = 5, K = 3: 15 branches in one wave, lanes of different envs side by side, eight-scenario mix.  A stands after 30 step()
    calls; the window of 40 calls under hold = 2 crosses the double-step call 51."""
    from gym_sbr2_amd import _capi
    n, k, n_steps, hold = 5, 3, 40, 2
    a_env, twin = _live(G, n, 30, seed=11), _live(G, n, 30, seed=11)
    tape, nominal = _tape(n_steps // hold, n, k, seed=12), _nominal(n_steps // hold, n, seed=14)
    x0, c0 = a_env.get_state()
    obs0 = a_env.obs.clone()
    ret, rew, bi, br, obs_end, state_end, done_end = _both_kernels(G, a_env, tape, nominal, n_steps, hold)
    assert obs_end.shape == (n, k, _capi.NOBS) and state_end.shape == (n, k, _capi.NSTATE) and done_end.shape == (n, k)
    assert not bool(done_end.any())
    assert bool((obs_end != 0).any(dim=2).all()) and bool((state_end != 0).any(dim=2).all())       # not a comparison of zeros
    for i in range(n):                                   # ... and the candidates of an env end in different places
        assert not torch.equal(obs_end[i, 0], obs_end[i, 1]) and not torch.equal(state_end[i, 0], state_end[i, 2])
    x1, c1 = a_env.get_state()
    assert torch.equal(x0, x1) and torch.equal(obs0, a_env.obs)
    for row in range(_capi.NCTRL):                     # every row: the plan, the return and the call count included
        assert torch.equal(c0[row], c1[row]), row
    # the handle goes on as if nothing had happened: the next step() gives the bits of a twin that never looked ahead
    act = _tape(1, n, 1, seed=13)[0, :, 0]
    outs_a = [t.clone() for t in a_env.step(act)]
    outs_t = twin.step(act)
    for u, v in zip(outs_a, outs_t):
        assert torch.equal(u, v)
    (xa, ca), (xt, ct) = a_env.get_state(), twin.get_state()
    assert torch.equal(xa, xt) and torch.equal(ca, ct)
    a_env.close(); twin.close()


def test_constant_tape_ends_where_the_policy_kernel_ends(G):
    """The second witness: under a net without a hidden layer and with zero weights the policy kernel plays the constant action
    b, and on exit writes back the observation of every env that is not done - the row obs_end holds for that constant tape."""
    from gym_sbr2_amd import MlpPolicy
    n, n_steps = 70, 12
    a_env, clone = _live(G, n, 33, seed=31), _live(G, n, 33, seed=31)
    b = np.array([1.25, 6.5], dtype=np.float32)
    pol = MlpPolicy([(np.zeros((2, 18), np.float32), b)], squash="none")
    o = clone.obs.to(torch.float32).clone()
    _, acts = clone.rollout_policy(pol, n_steps, obs=o, return_actions=True)
    assert bool((acts == torch.from_numpy(b).cuda()).all())             # the float32 value that was integrated
    tape = acts[:, :, None, :].contiguous()
    _, obs_end, _, done_end = a_env.lookahead_end(tape)
    assert not bool(done_end.any()) and torch.equal(obs_end[:, 0], o)
    a_env.close(); clone.close()


@pytest.mark.parametrize("reward", ["eqi_oci", "oci"])
def test_finished_and_running_branches_in_one_launch(G, reward):
    """N = 6, 40 calls.  Envs 0 - 2 were reset by mask 20 calls in and stand at call 443 of 463: their branches end with their
    20th call.  Env 3 ran all 463 calls: done on entry.  Envs 4, 5 were reset by mask at call 433 and stand at call 30: running."""
    from gym_sbr2_amd import _capi
    n, k, n_steps = 6, 3, 40
    rs = np.random.RandomState(21)
    a_env = G.SbrOSVec(n, reward=reward)
    scen, rnd = (np.arange(n) % 8).astype(np.int32), rs.randn(n, 48)
    a_env.reset(scenario=scen, rnd=rnd)
    acts = np.stack([rs.uniform(0, 2.5, (STEPS, n)), rs.uniform(0, 15, (STEPS, n))], axis=-1)
    acts = torch.from_numpy(acts).to(a_env.action_dtype).cuda()
    for c in range(STEPS):
        if c == 20:
            a_env.reset(scenario=scen, rnd=rnd, mask=np.array([1, 1, 1, 0, 0, 0], np.uint8))
        if c == 433:
            a_env.reset(scenario=scen, rnd=rnd, mask=np.array([0, 0, 0, 0, 1, 1], np.uint8))
        a_env.step(acts[c])
    x0, c0 = a_env.get_state()
    assert c0[_capi.C_STEPS].tolist() == [443, 443, 443, 463, 30, 30] and c0[_capi.C_DONE].tolist() == [0, 0, 0, 1, 0, 0]
    tape, nominal = _tape(n_steps, n, k, seed=22), _nominal(n_steps, n, seed=23)
    ret, rew, bi, br, obs_end, state_end, done_end = _both_kernels(G, a_env, tape, nominal, n_steps, 1, reward=reward)
    want = torch.tensor([1, 1, 1, 1, 0, 0], dtype=torch.bool, device="cuda")[:, None].expand(n, k)
    assert torch.equal(done_end, want)
    assert bool((obs_end[:4] == 0).all()) and bool((state_end[:4] == 0).all())
    assert bool((obs_end[4:] != 0).any(dim=2).all()) and bool((state_end[4:] != 0).any(dim=2).all())
    assert bool((rew[:, 3] == 0).all()) and bool((rew[19, :3] != 0).all()) and bool((rew[20:, :3] == 0).all())
    x1, c1 = a_env.get_state()
    assert torch.equal(x0, x1) and torch.equal(c0, c1)
    a_env.close()


def test_branches_across_wavefronts_and_the_workgroup_boundary(G):
    """N = 4, K = 70: 280 branches - an env's branches straddle wavefronts and the 256-lane workgroup boundary, the second
    workgroup holds 24 branches.  Env 3: NaN ammonia injected through set_state; its rows are compared with NaN equal to NaN,
    the other envs' exactly."""
    n, k, n_steps = 4, 70, 8
    a_env = _live(G, n, 20, seed=41)
    x, c = a_env.get_state()
    x[10, 3] = float("nan")
    a_env.set_state(x, c)
    tape, nominal = _tape(n_steps, n, k, seed=42), _nominal(n_steps, n, seed=43)
    out = _both_kernels(G, a_env, tape, nominal, n_steps, 1, same=_same)
    obs_end, state_end, done_end = out[4:]
    want = _end_checker(G, a_env, tape, n_steps, 1)
    assert torch.equal(obs_end[:3], want[0][:3]) and torch.equal(state_end[:3], want[1][:3])          # exact where nothing is NaN
    assert bool(torch.isfinite(obs_end[:3]).all()) and bool(torch.isnan(obs_end[3]).any()) and not bool(done_end.any())
    a_env.close()


@pytest.mark.parametrize("build", ["float64-tape", "scheme-0", "two-waves-by-branches"])
def test_other_builds(G, build):
    from gym_sbr2_amd import _capi
    kw, n, k, calls, n_steps = {}, 37, 2, 25, 8
    if build == "float64-tape":
        kw = {"action_dtype": torch.float64}
    elif build == "scheme-0":
        cfg = _capi.default_config()
        cfg.scheme = 0
        kw = {"config": cfg}
    else:
        # 1541 x 64 = 98 624 branches: above the 98 304 lanes the one-wave build serves, while the HANDLE's 1541 envs are far
        # below it - the budget goes by the branches.  The checker is a 98 624-env handle, for the tapes and for the sampled
        # kernel's own actions_out.
        n, k = 1541, 64
    a_env = _live(G, n, calls, seed=51, **kw)
    if build == "two-waves-by-branches":
        assert a_env.query(_capi.Q_ROLLOUT_WAVES) == 1 and n * k > a_env.query(_capi.Q_FUSED_ONE_WAVE_MAX_ENVS)
    tape = _tape(n_steps, n, k, seed=52, dtype=a_env.action_dtype)
    nominal = _nominal(n_steps, n, seed=53, dtype=a_env.action_dtype)
    x0, c0 = a_env.get_state()
    out = _both_kernels(G, a_env, tape, nominal, n_steps, 1, **kw)
    assert not bool(out[6].any()) and bool((out[4] != 0).any(dim=2).all())
    x1, c1 = a_env.get_state()
    assert torch.equal(x0, x1) and torch.equal(c0, c1)
    a_env.close()


def test_optional_outputs_and_refusals_on_a_live_handle(G):
    from gym_sbr2_amd import _capi
    lib = _capi.load()
    n, k, n_steps = 8, 3, 4
    a_env = _live(G, n, 3, seed=61)
    tape, nominal = _tape(n_steps, n, k, seed=62), _nominal(n_steps, n, seed=63)
    sm = _sampler().c_struct(a_env.cfg)
    import ctypes as C
    ret_all, obs_all, st_all, dn_all = a_env.lookahead_end(tape)
    rets_all, obss_all, sts_all, dns_all = a_env.lookahead_sampled_end(nominal, k, _sampler())

    def fresh():
        return (torch.full((n, k), 7.0, dtype=torch.float64, device="cuda"), torch.full((n, k, 18), 7.0, device="cuda"),
                torch.full((n, k, 15), 7.0, device="cuda"), torch.full((n, k), 7, dtype=torch.uint8, device="cuda"))

    def tape_call(n_steps, fanout, ret, o, s, d, bi=None):
        return lib.sbr_lookahead_actions_end(a_env._h, n_steps, 1, fanout, tape.data_ptr(), None if ret is None else ret.data_ptr(),
                                             None, None if bi is None else bi.data_ptr(), None, None if o is None else o.data_ptr(),
                                             None if s is None else s.data_ptr(), None if d is None else d.data_ptr(), None)

    def sampled_call(n_steps, fanout, ret, o, s, d):
        return lib.sbr_lookahead_sampled_end(a_env._h, n_steps, 1, fanout, nominal.data_ptr(), C.byref(sm), ret.data_ptr(), None,
                                             None, None, None, None if o is None else o.data_ptr(),
                                             None if s is None else s.data_ptr(), None if d is None else d.data_ptr(), None)

    # each of the three alone: the same bits as all together, the other two untouched
    for call, (r_w, o_w, s_w, d_w) in ((tape_call, (ret_all, obs_all, st_all, dn_all)), (sampled_call, (rets_all, obss_all, sts_all, dns_all))):
        for which in range(3):
            ret, o, s, d = fresh()
            picked = [t if j == which else None for j, t in enumerate((o, s, d))]
            assert call(n_steps, k, ret, *picked) == 0
            torch.cuda.synchronize()
            assert torch.equal(ret, r_w)
            assert torch.equal(o, o_w) if which == 0 else bool((o == 7.0).all())
            assert torch.equal(s, s_w) if which == 1 else bool((s == 7.0).all())
            assert torch.equal(d.bool(), d_w) and bool((d <= 1).all()) if which == 2 else bool((d == 7).all())
    # returns may be left out too
    ret, o, s, d = fresh()
    assert tape_call(n_steps, k, None, o, None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(o, obs_all)
    # the refusals that need a handle: nothing written
    x0, c0 = a_env.get_state()
    ret, o, s, d = fresh()
    bi = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    for call, name in ((tape_call, b"sbr_lookahead_actions_end"), (sampled_call, b"sbr_lookahead_sampled_end")):
        assert call(n_steps, k, ret, None, None, None) == -1            # all three NULL: the caller wants the parent
        assert name in lib.sbr_last_error(a_env._h)
        assert call(0, k, ret, o, s, d) == -1                           # n_steps = 0
        assert call(n_steps, 0, ret, o, s, d) == -1                     # the parents' refusals: fanout = 0
        assert call(n_steps, 2 ** 28, ret, o, s, d) == -1               # 8 x 2^28 = 2^31 branches
        assert call(-1, k, ret, o, s, d) == -1
    assert tape_call(n_steps, k, None, o, s, d, bi=bi) == -1            # best_index without returns
    with pytest.raises(Exception):
        a_env.lookahead_end(tape, n_steps=0)
    torch.cuda.synchronize()
    x1, c1 = a_env.get_state()
    assert torch.equal(x0, x1) and torch.equal(c0, c1)
    assert bool((ret == 7.0).all()) and bool((o == 7.0).all()) and bool((s == 7.0).all()) and bool((d == 7).all()) and bool((bi == 7).all())
    a_env.close()


def test_branch_best(G):
    """N = 4, K = 70 (the reduction strides: 70 > 64 lanes).  Env 1: an exact tie at the maximum; env 2: a 70-way tie; env 3:
    all NaN (index 0, value NaN).  K = 1.  And on a lookahead's own returns: the call's best_*."""
    from gym_sbr2_amd import _capi
    n, k = 4, 70
    a_env = _live(G, n, 3, seed=71)
    rs = np.random.RandomState(72)
    v = rs.randn(n, k)
    v[0, 5] = np.nan
    v[1, 40] = v[1, 13] = v[1].max() + 1.0
    v[2, :] = -3.25
    v[3, :] = np.nan
    vals = torch.from_numpy(v).cuda()
    bi, bv = a_env.branch_best(vals)
    idx, val = _host_best(vals)
    assert bi.dtype == torch.int32 and bv.dtype == torch.float64 and bi.shape == bv.shape == (n,)
    assert np.array_equal(bi.cpu().numpy(), idx) and np.array_equal(bv.cpu().numpy(), val, equal_nan=True)
    assert bi.tolist()[1:] == [13, 0, 0] and np.isnan(float(bv[3]))
    bi1, bv1 = a_env.branch_best(vals[:, 7:8].contiguous())
    assert bool((bi1 == 0).all()) and np.array_equal(bv1.cpu().numpy(), v[:, 7], equal_nan=True)
    ret, bi_l, br_l = a_env.lookahead(_tape(6, n, k, seed=73), return_best=True)
    bi2, bv2 = a_env.branch_best(ret)
    assert torch.equal(bi2, bi_l) and torch.equal(bv2, br_l)
    # one output alone; refusals with nothing written
    lib = _capi.load()
    only = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    assert lib.sbr_branch_best(a_env._h, k, vals.data_ptr(), only.data_ptr(), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(only, bi)
    only.fill_(7)
    assert lib.sbr_branch_best(a_env._h, 0, vals.data_ptr(), only.data_ptr(), None, None) == -1
    assert lib.sbr_branch_best(a_env._h, 2 ** 29, vals.data_ptr(), only.data_ptr(), None, None) == -1     # 4 x 2^29 = 2^31
    assert lib.sbr_branch_best(a_env._h, k, None, only.data_ptr(), None, None) == -1
    assert lib.sbr_branch_best(a_env._h, k, vals.data_ptr(), None, None, None) == -1
    assert b"sbr_branch_best" in lib.sbr_last_error(a_env._h)
    torch.cuda.synchronize()
    assert bool((only == 7).all())
    with pytest.raises(ValueError):
        a_env.branch_best(vals[:3])
    a_env.close()


def test_planner_with_a_terminal_value(G):
    from gym_sbr2_amd.planner import MppiPlanner
    n, k, rows = 6, 16, 5
    sm = _sampler(seed=81)

    def planner(env, tv):
        p = MppiPlanner(env, rows=rows, fanout=k, sampler=sm, temperature=2.0)
        p.terminal_value = tv
        return p

    # a critic of zeros: the bits of a planner without one, over three decisions
    e0, e1 = _live(G, n, 10, seed=82), _live(G, n, 10, seed=82)
    p0, p1 = planner(e0, None), planner(e1, lambda o, s: torch.zeros(o.shape[:2], device=o.device))
    for _ in range(3):
        a0, a1 = p0.plan(), p1.plan()
        assert torch.equal(a0, a1) and torch.equal(p0.nominal, p1.nominal)
        e0.step(a0); e1.step(a1)
    e0.close()
    # a critic that is not trivial: the returns are lookahead_sampled's plus the masked value, the action mppi_update's on them
    seen = {}

    def critic(o, s):
        seen["shapes"] = (tuple(o.shape), tuple(s.shape), o.dtype, s.dtype)
        return 3.0 * o[..., 4] - 0.5 * s[..., 11] + 1.0

    p2 = planner(e1, critic)
    nominal, d = p2.nominal.clone(), p2.decision
    sm_d = sm.with_seed(sm.seed + d)
    ret, obs_end, state_end, done_end = e1.lookahead_sampled_end(nominal, k, sm_d)
    assert torch.equal(ret, e1.lookahead_sampled(nominal, k, sm_d))
    want = ret + torch.where(done_end, torch.zeros_like(ret), critic(obs_end, state_end).double())
    act, got = p2.plan(return_returns=True)
    assert seen["shapes"] == ((n, k, 18), (n, k, 15), torch.float32, torch.float32)
    assert torch.equal(got, want) and not torch.equal(got, ret)
    by_hand = e1.mppi_update(nominal, want.contiguous(), sm_d, 2.0)
    assert torch.equal(act, by_hand[0])
    e1.close()


def test_graph_capture(G):
    """One lookahead_sampled_end captured on a side stream and replayed: nothing in the call allocates or synchronises on the
    library's side (the results are allocated by torch inside the capture, from the graph's pool)."""
    n, k, rows = 64, 8, 6
    env = _live(G, n, 12, seed=91)
    nominal, sm = _nominal(rows, n, seed=92), _sampler(seed=93)
    eager = env.lookahead_sampled_end(nominal, k, sm, return_best=True)          # also loads the kernel outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            captured = env.lookahead_sampled_end(nominal, k, sm, return_best=True)
    torch.cuda.current_stream().wait_stream(side)
    g.replay()
    torch.cuda.synchronize()
    assert len(captured) == len(eager) == 6
    for u, v in zip(captured, eager):
        assert torch.equal(u, v)
    assert bool((eager[3] != 0).any())
    env.close()
