"""One handle through every translation unit of the library (gym_sbr2_amd/build.py SOURCES): the units are compiled apart and
linked without relocatable device code, so each registers a code object of its own with the runtime, and an entry point can only
launch a kernel of its own unit.  One process, 64 envs, scheme 1, float32: at least one kernel of every unit is launched, every
call returns finite results of the documented shapes, and the read-only calls leave the handle as it was.  What the kernels
compute is pinned elsewhere (the parity tests and the goldens of test_fused_parent_gpu.py / test_step_spill_gpu.py)."""
import numpy as np
import pytest
from gpu_common import package

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N, K = 64, 2


def _finite(t, shape, dtype):
    assert tuple(t.shape) == shape and t.dtype == dtype, (tuple(t.shape), t.dtype)
    assert bool(torch.isfinite(t.to(torch.float64)).all())
    return t


def test_one_handle_launches_a_kernel_of_every_unit():
    G = package()
    from gym_sbr2_amd import MlpPolicy, TapeSampler, _capi
    rs = np.random.RandomState(4)
    env = G.SbrOSVec(N)
    assert env.query(_capi.Q_SCHEME) == 1 and env.out_dtype == torch.float32
    # ---- the calls that move the handle.  sbr_core.hip: k_fill (create), k_reset
    _finite(env.reset(scenario=(np.arange(N) % 8).astype(np.int32), rnd=rs.randn(N, 48)), (N, 18), torch.float32)
    a = torch.from_numpy(np.stack([rs.uniform(0, 2.5, N), rs.uniform(0, 15, N)], axis=-1)).to(torch.float32).cuda()
    o, s, r, d = env.step(a)                                                                  # sbr_core.hip: k_step
    _finite(o, (N, 18), torch.float32); _finite(s, (N, 15), torch.float32); _finite(r, (N,), torch.float32)
    assert tuple(d.shape) == (N,) and not bool(d.any())
    ret, acts = env.rollout(2, policy_seed=3, return_actions=True)                            # sbr_rollout.hip: k_rollout
    _finite(ret, (N,), torch.float64); _finite(acts, (2, N, 2), torch.float32)
    tape = torch.from_numpy(np.stack([rs.uniform(0, 2.5, (2, N)), rs.uniform(0, 15, (2, N))], axis=-1)).to(torch.float32).cuda()
    ret, rew = env.rollout_actions(tape, return_rewards=True)                                 # sbr_tape.hip: k_rollout_tape
    _finite(ret, (N,), torch.float64); _finite(rew, (2, N), torch.float64)
    sizes = [18, 32, 32, 2]
    pol = MlpPolicy([(rs.randn(o_, i_) / np.sqrt(i_), rs.randn(o_) * 0.1) for i_, o_ in zip(sizes[:-1], sizes[1:])],
                    activation="tanh", squash="tanh", low=(0.0, 0.0), high=(2.5, 15.0))
    ret, pacts = env.rollout_policy(pol, 2, return_actions=True)                              # sbr_policy.hip: k_rollout_policy
    _finite(ret, (N,), torch.float64); _finite(pacts, (2, N, 2), torch.float32); _finite(env.obs, (N, 18), torch.float32)
    # ---- the read-only calls: the handle is bit for bit what it was
    x0, c0 = env.get_state()                                                                  # sbr_core.hip: k_export
    _finite(x0, (_capi.NX, N), torch.float64)
    assert tuple(c0.shape) == (_capi.NCTRL, N) and c0.dtype == torch.float64
    assert bool((c0[_capi.C_STEPS] == 7).all())                   # 1 + 2 + 2 + 2 calls, counted across four units' kernels
    obs0 = env.obs.clone()
    cand = torch.from_numpy(np.stack([rs.uniform(0, 2.5, (2, N, K)), rs.uniform(0, 15, (2, N, K))], axis=-1)).to(torch.float32).cuda()
    ret, rew, bi, br = env.lookahead(cand, return_rewards=True, return_best=True)             # sbr_tape.hip: k_lookahead_tape, k_branch_best
    _finite(ret, (N, K), torch.float64); _finite(rew, (2, N, K), torch.float64); _finite(br, (N,), torch.float64)
    assert tuple(bi.shape) == (N,) and bi.dtype == torch.int32 and bool(((bi >= 0) & (bi < K)).all())
    sm = TapeSampler((0.3, 2.0), seed=5)
    sret, sbi, sbr, sacts = env.lookahead_sampled(tape, K, sm, return_best=True, return_actions=True)   # sbr_sampled.hip, then sbr_tape.hip's k_branch_best
    _finite(sret, (N, K), torch.float64); _finite(sbr, (N,), torch.float64); _finite(sacts, (2, N, K, 2), torch.float32)
    assert tuple(sbi.shape) == (N,) and bool(((sbi >= 0) & (sbi < K)).all())
    pret, pbi, pbr = env.lookahead_policy(pol, K, 2, noise_std=(0.25, 2.0), noise_seed=1, return_best=True)   # sbr_policy_lookahead.hip, then k_branch_best
    _finite(pret, (N, K), torch.float64); _finite(pbr, (N,), torch.float64)
    assert tuple(pbi.shape) == (N,) and bool(((pbi >= 0) & (pbi < K)).all())
    bi2, bv2 = env.branch_best(sret)                                                          # sbr_tape.hip on its own
    assert torch.equal(bi2, sbi) and torch.equal(bv2, sbr)
    new, w = env.mppi_update(tape, sret, sm, temperature=0.5, return_weights=True)            # sbr_sampled.hip: k_mppi_update
    _finite(new, (2, N, 2), torch.float32); _finite(w, (N, K), torch.float64)
    assert bool(((w.sum(dim=1) - 1.0).abs() < 1e-12).all())
    x1, c1 = env.get_state()
    assert torch.equal(x0, x1) and torch.equal(env.obs, obs0)
    same = (c0 == c1) | (torch.isnan(c0) & torch.isnan(c1))
    assert bool(same.all()), same.logical_not().nonzero()[:5]
    env.close()
