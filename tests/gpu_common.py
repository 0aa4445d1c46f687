"""What the GPU tests share (the fused entry points: tests/test_tape_rollout_gpu.py, tests/test_policy_rollout_gpu.py,
tests/test_lookahead_gpu.py, tests/test_lookahead_end_gpu.py, tests/test_mppi_gpu.py, tests/test_lookahead_policy_gpu.py; the plan
rule: tests/test_gpu_parity.py, tests/test_plan_branches_gpu.py): the package behind their `G` fixtures, the seeded inputs, handles
behind a non-default config, the check that no env left the model's domain, and what the fan-out tests build on - a live handle,
seeded tapes and nets, the host's Philox, winner rule and mean / worst rule, torch.equal with NaN equal to NaN.  A plain module: pytest does not
rewrite its asserts, so each carries its message; torch is imported inside the helpers that need it."""
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


# ------------------------------------------------------------------ the fan-out tests (lookahead, _end, sampled / MPPI, policy)
def live(G, n, calls, seed, first=0, **kw):
    """A handle of n envs with global ids first .. (scenario = id % 8), advanced `calls` calls through step() under varied
    actions: its controller record is then in the form k_step leaves (implicit So[-1] / Sno[-1], the Kla ring rotated, a
    non-zero plan row)."""
    import torch
    rs = np.random.RandomState(seed)
    env = G.SbrOSVec(n, first_env_id=first, **kw)
    env.reset(scenario=((first + np.arange(n)) % 8).astype(np.int32), rnd=rs.randn(n, 48))
    acts = np.stack([rs.uniform(0, 2.5, (calls, n)), rs.uniform(0, 15, (calls, n))], axis=-1)
    acts = torch.from_numpy(acts).to(env.action_dtype).cuda()
    for c in range(calls):
        env.step(acts[c])
    return env


def tape(rows, n, k, seed, dtype=None):
    """K candidate tapes per env [rows, n, k, 2] on the device (dtype: float32 unless given), u_DO ~ U[0, 2.5], u_EC ~ U[0, 15]."""
    import torch
    rs = np.random.RandomState(seed)
    t = np.stack([rs.uniform(0, 2.5, (rows, n, k)), rs.uniform(0, 15, (rows, n, k))], axis=-1)
    return torch.from_numpy(t).to(torch.float32 if dtype is None else dtype).cuda()


def nominal(rows, n, seed, dtype=None, lo=(0.0, 0.0), hi=(2.5, 15.0)):
    """One tape per env [rows, n, 2] on the device: the draws of tape(rows, n, 1, seed) under the default bounds."""
    import torch
    rs = np.random.RandomState(seed)
    t = np.stack([rs.uniform(lo[0], hi[0], (rows, n)), rs.uniform(lo[1], hi[1], (rows, n))], axis=-1)
    return torch.from_numpy(t).to(torch.float32 if dtype is None else dtype).cuda()


def net(seed, widths):
    """The layers [(W, b)] of an 18 -> widths -> 2 MLP."""
    rs = np.random.RandomState(seed)
    sizes = [18] + list(widths) + [2]
    return [(rs.randn(o, i) / np.sqrt(i), rs.randn(o) * 0.1) for i, o in zip(sizes[:-1], sizes[1:])]


def same(a, b):
    """torch.equal with NaN equal to NaN (a NaN plant gives NaN rows on both sides)."""
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool((torch.isnan(a) == torch.isnan(b)).all()) and torch.equal(
        torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


def host_best(v):
    """The header's rule on the host: NaN -> -inf, first maximum; the value is the winner's entry as it stands."""
    r = v.cpu().numpy()
    idx = np.argmax(np.where(np.isnan(r), -np.inf, r), axis=1).astype(np.int32)
    return idx, r[np.arange(r.shape[0]), idx]


def host_stats(ret):
    """mean and worst of returns [N, K, S] as the header defines them: a float64 loop over s, then one division; the smallest,
    NaN if any is NaN."""
    r = ret.cpu().numpy()
    acc = np.zeros(r.shape[:2])
    for s in range(r.shape[2]):
        acc = acc + r[:, :, s]
    with np.errstate(invalid="ignore"):
        worst = np.where(np.isnan(r).any(axis=2), np.nan, r.min(axis=2))
    return acc / float(r.shape[2]), worst


# Philox4x32-10 + Box-Muller in numpy (include/sbr_amd.h)
_M32 = np.uint64(0xFFFFFFFF)


def philox(c, key):
    """c: four uint64 arrays holding 32-bit words; key: the 64-bit seed."""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & _M32 for v in c)
    k0, k1 = np.uint64(key & 0xFFFFFFFF), np.uint64((key >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c0, c1, c2, c3


def normal_pair(counter, stream, gid, seed):
    """(z0, z1) of Philox block (counter, stream, gid_lo, gid_hi) under key `seed`; the arguments broadcast."""
    counter, stream, gid = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in (counter, stream, gid)))
    c = philox((counter, stream, gid & _M32, gid >> np.uint64(32)), seed)

    def u53(hi, lo):                                   # uniform in (0, 1]
        return (((hi << np.uint64(32)) | lo) >> np.uint64(11)).astype(np.float64) + 1.0

    u1, u2 = u53(c[0], c[1]) * 2.0 ** -53, u53(c[2], c[3]) * 2.0 ** -53
    rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586476925286766559 * u2
    return rad * np.cos(ang), rad * np.sin(ang)


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
