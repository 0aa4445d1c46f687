"""sbr_rollout_policy without a GPU: the two entry points are exported and bound, every refusal is decided before anything is
touched, MlpPolicy packs what the header describes (zero padding is neutral), and the gfx950 ISA of k_rollout_policy
(cross-compiled as tests/test_tape_rollout_cpu.py does) keeps its register contract: no scratch in the one-wave build, 256
registers in the others, nothing but the tape kernel's arithmetic in the Butcher-5 step loops, the net really unrolled."""
import collections
import ctypes as C
import inspect

import numpy as np
import pytest
from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)
from isa import K_POL, K_TAPE, K_TAPE_2W, b5_steps, f64_mix, flop_counts, instructions, kernel_text, library_asm, meta

from gym_sbr2_amd import _capi


def _policy(**kw):
    blk = (C.c_float * 5506)()
    f = dict(params=C.cast(blk, C.c_void_p), n_hidden=2, width=32, activation=0, squash=1, n_policies=1, envs_per_policy=0,
             act_scale=(C.c_float * 2)(4.0, 7.5), act_bias=(C.c_float * 2)(4.0, 7.5), noise_std=(C.c_float * 2)(0.0, 0.0),
             noise_seed=0)
    f.update(kw)
    p = _capi.SbrPolicy(**f)
    p._keep = blk
    return p


def test_symbols_are_exported_and_bound():
    lib = _capi.load()
    raw = C.CDLL(_capi.library_path())
    for name in ("sbr_rollout_policy", "sbr_policy_param_count"):
        assert name in _capi.SYMBOLS and getattr(raw, name) is not None and getattr(lib, name).argtypes is not None
    assert lib.sbr_abi_version() == 6


def test_param_count():
    lib = _capi.load()
    from gym_sbr2_amd.policy import param_count
    want = {(0, 32): 38, (0, 0): 38, (1, 32): 674, (2, 32): 1730, (1, 64): 1346, (2, 64): 5506}
    for (nh, w), n in want.items():
        assert lib.sbr_policy_param_count(nh, w) == n, (nh, w)
        if w:
            assert param_count(nh, w) == n
    assert lib.sbr_policy_param_count(3, 32) == -1 and lib.sbr_policy_param_count(1, 48) == -1


def test_every_refusal_is_decided_before_anything_is_touched():
    """No handle can exist without a device, so every call below is refused; the message names the LAST failing check, which
    shows that the argument under test was looked at."""
    lib = _capi.load()
    obs = (C.c_float * 18)(*([0.25] * 18))
    ret = (C.c_double * 1)(7.0)
    o, r = C.cast(obs, C.c_void_p), C.cast(ret, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def refused(why, n_steps=1, hold=1, policy=True, obs_ptr=o, **kw):
        p = _policy(**kw) if policy else None
        rc = lib.sbr_rollout_policy(None, n_steps, hold, C.byref(p) if p is not None else None, obs_ptr, r, None, None, None)
        msg = lib.sbr_last_error(None)
        assert rc == -1 and b"sbr_rollout_policy" in msg and why in msg, (why, rc, msg)

    refused(b"NULL env")
    refused(b"NULL policy", policy=False)
    refused(b"NULL params", params=None)
    refused(b"NULL obs", obs_ptr=None)
    refused(b"n_steps", n_steps=-1)
    refused(b"hold", hold=0)
    refused(b"n_hidden", n_hidden=3)
    refused(b"n_hidden", n_hidden=-1)
    refused(b"width", width=48)
    refused(b"width", n_hidden=1, width=0)
    refused(b"NULL env", n_hidden=0, width=0)             # without a hidden layer the width is not looked at
    refused(b"activation", activation=2)
    refused(b"squash", squash=-1)
    refused(b"n_policies", n_policies=0)
    refused(b"noise_std", noise_std=(C.c_float * 2)(0.1, -0.1))
    refused(b"noise_std", noise_std=(C.c_float * 2)(nan, 0.0))
    refused(b"noise_std", noise_std=(C.c_float * 2)(0.0, inf))
    refused(b"envs_per_policy", n_policies=2, envs_per_policy=100)
    refused(b"envs_per_policy", n_policies=2, envs_per_policy=0)
    refused(b"NULL env", n_policies=2, envs_per_policy=512)
    assert list(ret) == [7.0] and list(obs) == [0.25] * 18


def _net(rs, widths, scale=0.5):
    sizes = [18] + list(widths) + [2]
    return [(rs.randn(o, i) * scale / np.sqrt(i), rs.randn(o) * 0.1) for i, o in zip(sizes[:-1], sizes[1:])]


def test_padding_is_neutral_and_the_block_is_laid_out_like_linear():
    from gym_sbr2_amd.policy import MlpPolicy
    rs = np.random.RandomState(5)
    layers = _net(rs, (20, 20))
    pol = MlpPolicy(layers, activation="tanh", squash="tanh", low=(0, 0), high=(2.5, 15))
    assert (pol.n_hidden, pol.width) == (2, 32) and pol.block.shape == (1, 1730) and pol.block.dtype == np.float32
    # the layout: W0 [32][18], b0 [32], W1 [32][32], b1 [32], W2 [2][32], b2 [2]
    blk = pol.block[0]
    w0 = blk[:576].reshape(32, 18)
    assert np.array_equal(w0[:20], layers[0][0].astype(np.float32)) and not w0[20:].any()
    assert np.array_equal(blk[576:596], layers[0][1].astype(np.float32)) and not blk[596:608].any()
    w1 = blk[608:608 + 1024].reshape(32, 32)
    assert np.array_equal(w1[:20, :20], layers[1][0].astype(np.float32)) and not w1[20:].any() and not w1[:, 20:].any()
    w2 = blk[1664:1728].reshape(2, 32)
    assert np.array_equal(w2[:, :20], layers[2][0].astype(np.float32)) and not w2[:, 20:].any()
    assert np.array_equal(blk[1728:], layers[2][1].astype(np.float32))
    # evaluated in float64 from the packed block = the unpadded net on the float32 parameters, exactly
    o = rs.uniform(-1, 1, (257, 18))
    h = o
    for k, (w, b) in enumerate(layers):
        h = h @ w.astype(np.float32).astype(np.float64).T + b.astype(np.float32).astype(np.float64)
        h = np.tanh(h)
    want = np.float32([1.25, 7.5]).astype(np.float64) + np.float32([1.25, 7.5]).astype(np.float64) * h
    got = pol.mean_f64(o)
    # (a sum over 32 terms of which 12 are exact zeros is the sum over the 20: numpy's pairwise order may differ by rounding)
    assert np.abs(got - want).max() <= 8 * np.finfo(np.float64).eps * np.abs(want).max()
    wide = pol.widened(64)
    assert wide.width == 64 and wide.block.shape == (1, 5506)
    assert np.abs(wide.mean_f64(o) - want).max() <= 8 * np.finfo(np.float64).eps * np.abs(want).max()


def test_sequential_and_pairs_give_the_same_block():
    torch = pytest.importorskip("torch")
    from gym_sbr2_amd.policy import MlpPolicy
    torch.manual_seed(3)
    seq = torch.nn.Sequential(torch.nn.Linear(18, 24), torch.nn.ReLU(), torch.nn.Linear(24, 40), torch.nn.ReLU(), torch.nn.Linear(40, 2))
    a = MlpPolicy(seq)
    pairs = [(m.weight.detach().numpy(), m.bias.detach().numpy()) for m in seq if isinstance(m, torch.nn.Linear)]
    b = MlpPolicy(pairs, activation="relu")
    assert a.activation == "relu" and (a.n_hidden, a.width) == (2, 64) and np.array_equal(a.block, b.block)
    lin = MlpPolicy(torch.nn.Sequential(torch.nn.Linear(18, 2)))
    assert (lin.n_hidden, lin.block.shape) == (0, (1, 38))
    pop = MlpPolicy.stack([MlpPolicy(_net(np.random.RandomState(s), (20,))) for s in (1, 2, 3)], envs_per_policy=256)
    assert pop.block.shape == (3, 674) and (pop.n_policies, pop.envs_per_policy) == (3, 256)


def test_bad_shapes_raise():
    from gym_sbr2_amd.policy import MlpPolicy
    rs = np.random.RandomState(0)
    for bad in ([(rs.randn(20, 17), rs.randn(20)), (rs.randn(2, 20), rs.randn(2))],          # 17 inputs
                [(rs.randn(20, 18), rs.randn(20)), (rs.randn(3, 20), rs.randn(3))],          # 3 outputs
                [(rs.randn(20, 18), rs.randn(20)), (rs.randn(2, 21), rs.randn(2))],          # widths do not chain
                [(rs.randn(65, 18), rs.randn(65)), (rs.randn(2, 65), rs.randn(2))],          # wider than 64
                [(rs.randn(20, 18), rs.randn(19)), (rs.randn(2, 20), rs.randn(2))],          # bias of another length
                _net(rs, (8, 8, 8)),                                                           # three hidden layers
                []):
        with pytest.raises(ValueError):
            MlpPolicy(bad)
    with pytest.raises(ValueError):
        MlpPolicy(_net(rs, (8,)), activation="gelu")
    with pytest.raises(ValueError):
        MlpPolicy(_net(rs, (8,)), squash="sigmoid")
    with pytest.raises(ValueError):
        MlpPolicy.stack([MlpPolicy(_net(rs, (8,)))], envs_per_policy=100)
    with pytest.raises(ValueError):
        MlpPolicy.stack([MlpPolicy(_net(rs, (8,))), MlpPolicy(_net(rs, (8, 8)))], envs_per_policy=256)


def test_widened_keeps_the_action_range_and_works_on_a_population():
    from gym_sbr2_amd.policy import MlpPolicy
    rs = np.random.RandomState(9)
    o = rs.uniform(-1, 1, (33, 18))
    a, b = (MlpPolicy(_net(rs, (20, 12)), low=(0.5, 1), high=(2.5, 9)) for _ in range(2))
    with pytest.warns(RuntimeWarning, match="64-wide"):
        MlpPolicy(_net(rs, (40,)))                                   # the slow build is never picked silently
    wa = a.widened(64)
    assert wa.width == 64 and np.array_equal(wa.act_scale, a.act_scale) and np.array_equal(wa.act_bias, a.act_bias)
    assert np.allclose(wa.mean_f64(o), a.mean_f64(o), rtol=0, atol=1e-14) and np.array_equal(wa.pack(64), wa.block[0])
    pop = MlpPolicy.stack([a, b], envs_per_policy=256)
    wp = pop.widened(64)
    assert wp.block.shape == (2, 5506) and (wp.n_policies, wp.envs_per_policy) == (2, 256)
    assert np.array_equal(wp.block[1], b.pack(64)) and np.allclose(wp.mean_f64(o, member=1), b.mean_f64(o), rtol=0, atol=1e-14)
    with pytest.raises(ValueError):
        pop.pack(32)


def test_a_module_behind_the_last_linear_is_refused():
    torch = pytest.importorskip("torch")
    from gym_sbr2_amd.policy import MlpPolicy
    nn = torch.nn
    for tail in (nn.ReLU(), nn.Tanh()):
        with pytest.raises(ValueError, match="last Linear"):
            MlpPolicy(nn.Sequential(nn.Linear(18, 8), nn.Tanh(), nn.Linear(8, 2), tail))
    with pytest.raises(ValueError):
        MlpPolicy(nn.Sequential(nn.Linear(18, 8), nn.Linear(8, 2)))          # a hidden layer without its activation


def test_python_surface_exists():
    import gym_sbr2_amd
    from gym_sbr2_amd import ShardedSbrOS, SbrOSVec
    assert gym_sbr2_amd.MlpPolicy.__name__ == "MlpPolicy"
    for cls in (SbrOSVec, ShardedSbrOS):
        sig = inspect.signature(cls.rollout_policy)
        assert list(sig.parameters) == ["self", "policy", "n_steps", "hold", "obs", "noise_std", "noise_seed", "return_actions", "return_rewards"]
        d = {k: v.default for k, v in sig.parameters.items()}
        assert (d["hold"], d["obs"], d["noise_std"], d["noise_seed"], d["return_actions"], d["return_rewards"]) == (1, None, None, 0, False, False)


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def test_policy_kernel_register_budgets_and_scratch(asm):
    for h in (32, 64):
        k = K_POL[h, 1, 1]
        assert meta(asm, k, "private_segment_fixed_size") == 0, h
        assert f64_mix(instructions(kernel_text(asm, k)))["scratch"] == 0, h
        assert meta(asm, k, "vgpr_count") <= 512
        assert meta(asm, K_POL[h, 1, 2], "vgpr_count") <= 256 and meta(asm, K_POL[h, 0, 2], "vgpr_count") <= 256


def test_policy_kernel_step_loops_are_the_tape_kernels(asm):
    import bench
    tape_scratch = {1: max(f64_mix(l)["scratch"] for l in b5_steps(kernel_text(asm, K_TAPE), 700)),
                    2: max(f64_mix(l)["scratch"] for l in b5_steps(kernel_text(asm, K_TAPE_2W), 700))}
    for h in (32, 64):
        for wv in (1, 2):
            k = K_POL[h, 1, wv]
            steps = b5_steps(kernel_text(asm, k), 700)
            assert len(steps) >= 2, k
            flop = flop_counts(steps)
            assert flop[0] == bench.FP64_FLOP_PER_B5_STEP["plain"] and flop[-1] == bench.FP64_FLOP_PER_B5_STEP["dosing"], (k, flop)
            for l in steps:
                m = f64_mix(l)
                assert m["fma"] + m["mul"] + m["add"] + m["rcp"] in (477, 537), (k, m)
                assert m["div"] == 0, k                               # no v_div_fmas_f64 in any step loop
                assert m["scratch"] <= tape_scratch[wv], (k, m["scratch"], tape_scratch[wv])


def test_the_net_is_unrolled_into_scalar_fmas(asm):
    fma32 = lambda k: sum(v for op, v in collections.Counter(i.split()[0] for i in instructions(kernel_text(asm, k))).items()   # noqa: E731
                          if op.startswith("v_fma_f32") or op.startswith("v_fmac_f32"))
    assert fma32(K_POL[32, 1, 1]) >= 18 * 32 + 32 * 32 + 2 * 32
    assert fma32(K_POL[64, 1, 1]) >= 18 * 64 + 64 * 64 + 2 * 64
    # the weights come through the scalar data path: the net adds no per-lane load to the kernel (18 for the observation)
    gl = lambda k: sum(1 for i in instructions(kernel_text(asm, k)) if i.startswith("global_load") or i.startswith("flat_load"))   # noqa: E731
    assert gl(K_POL[32, 1, 1]) <= gl(K_TAPE) + 18 and gl(K_POL[64, 1, 1]) <= gl(K_TAPE) + 18
