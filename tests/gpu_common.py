"""What the GPU tests share (the fused entry points: tests/test_tape_rollout_gpu.py, tests/test_policy_rollout_gpu.py,
tests/test_lookahead_gpu.py; the plan rule: tests/test_gpu_parity.py, tests/test_plan_branches_gpu.py): the package behind their `G` fixtures, the seeded inputs, handles behind a non-default config
and the check that no env left the model's domain.  A plain module: pytest does not rewrite its asserts, so each carries its
message."""
import os

import numpy as np

STEPS = 463                     # calls of one SBROS-v1 episode
FLAGS = 1 | 2 | 4               # SBR_ST_NEGATIVE | SBR_ST_NEAR_POLE | SBR_ST_NONFINITE
CONFIGS = [(0, "eqi_oci"), (1, "g2anet"), (1, "oci"), (0, "oci")]      # (cfg.scheme, reward) of the non-default builds


def package():
    """gym_sbr2_amd, once it is certain that the in-tree library runs on a device: what the files' `G` fixtures return."""
    import torch

    import gym_sbr2_amd
    from gym_sbr2_amd import _capi
    assert torch.cuda.is_available(), "these tests need the GPU box"
    lib = _capi.load()
    assert _capi.library_path().endswith(os.path.join("gym_sbr2_amd", "lib", "libsbr_amd.so")), "the in-tree .so is what runs"
    assert lib.sbr_device_count() >= 1, "no HIP device"
    return gym_sbr2_amd


def to_np(t):
    return t.detach().cpu().numpy()


def inputs(n, seed, first=0, rows=0):
    """scenario [n] int32 (4 + global id % 4) and rnd [n, 48] float64 for the envs with global ids first .. first + n - 1; with
    rows > 0 also a tape [rows, n, 2] float32, u_DO ~ U[0, 2.5], u_EC ~ U[0, 15].  The order of the draws is part of the tests:
    their seeds were validated against the oracle for exactly these."""
    rs = np.random.RandomState(seed)
    scen = (4 + (first + np.arange(n)) % 4).astype(np.int32)
    rnd = rs.randn(n, 48)
    if not rows:
        return scen, rnd
    tape = np.stack([rs.uniform(0, 2.5, (rows, n)), rs.uniform(0, 15, (rows, n))], axis=-1).astype(np.float32)
    return scen, rnd, tape


def handle(G, n, scheme, reward, **kw):
    """An SbrOSVec of n envs under cfg.scheme and the named reward (not reset)."""
    from gym_sbr2_amd import _capi
    cfg = _capi.default_config(); cfg.scheme = scheme
    env = G.SbrOSVec(n, config=cfg, reward=reward, **kw)
    assert env.cfg.scheme == scheme and env.cfg.reward_kind == _capi.REWARD_KINDS[reward], (scheme, reward)
    assert env.query(_capi.Q_ROLLOUT_WAVES) == (2 if scheme == 0 else 1), (scheme, env.query(_capi.Q_ROLLOUT_WAVES))
    return env


def no_flags(status):
    """`status`: the C_STATUS row of a handle, [N] float64 on the device."""
    st = to_np(status).astype(np.int64)
    assert np.count_nonzero(st & FLAGS) == 0, "%d envs flagged" % np.count_nonzero(st & FLAGS)


def plans_agree(ctrl, ora, where=None, pick=None):
    """the plan of cfg.scheme = 1 - Butcher-5 step count and the slaved bit of the env's last interval - as the
    DEVICE reports it (SBR_C_PLAN, from the meta row) equals the oracle's for the same call.  A decision that flipped (a rounded
    double on the other side of 0.3 / 1.0 / 1e-9) would show as a ~1e-2-gate mismatch otherwise indistinguishable from a wrong kernel."""
    from gym_sbr2_amd import _capi
    dev = np.asarray(ctrl[_capi.C_PLAN]).astype(np.int64)
    if pick is not None:
        dev = dev[pick]
    ref = ora.envs["scheme_plan"].astype(np.int64) & 0xff
    if where is not None:
        dev, ref = dev[where], ref[where]
    bad = np.nonzero(dev != ref)[0]
    assert bad.size == 0, ("plan flipped on %d envs; first: device %d, oracle %d" % (bad.size, dev[bad[0]], ref[bad[0]]))
    return dev
