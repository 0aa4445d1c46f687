"""What the tests of SBR-v2's three read-only lookaheads share (sbr_cycle_lookahead, _scenarios, _models: tests/test_cycle_*_gpu.py
and tests/test_cycle_*_cpu.py): the live handle, seeded candidates, the handle's bits before and after, the per-cycle kernel as
the checker of every output, and on the CPU side the entry points' declaration, their NULL-env refusal and their translation
unit.  A plain module like gpu_common: pytest does not rewrite its asserts, so each carries its message; torch is imported inside
the helpers that need it.  The order and number of the RNG draws are part of the tests."""
import ctypes as C
import os
import re

import numpy as np
from gpu_common import host_best, host_stats, same

BUILDS = [(0, False), (0, True), (1, False), (1, True)]          # (cfg.scheme, float64 outputs and actions)
IDS = ["scheme%d-%s" % (s, "f64" if d else "f32") for s, d in BUILDS]
ALL = dict(return_rewards=True, return_stats=True, return_best=True, return_end=True, return_status=True)
NAMES = "returns rewards mean worst best_index best_value obs_end diag_end status".split()


# ---------------------------------------------------------------------------------------------- on the GPU
def make_env(G, n, scheme=1, f64=False, cfg=None, **kw):
    """An SbrEnv2Vec of n envs (not reset) under a copy of `cfg`, or under the default config with cfg.scheme = scheme."""
    import torch
    from gym_sbr2_amd import _capi
    from gym_sbr2_amd.models import copy_config
    if cfg is None:
        cfg = _capi.default_config(); cfg.scheme = scheme
    dt = torch.float64 if f64 else torch.float32
    env = G.SbrEnv2Vec(n, config=copy_config(cfg), out_dtype=dt, action_dtype=dt, **kw)
    assert env.cfg.scheme == cfg.scheme, (env.cfg.scheme, cfg.scheme)
    return env


def scen(n):
    return (np.arange(n) % 8).astype(np.int32)


def start(G, n, scheme=1, f64=False, seed=0, carried=True, stepped=False):
    """A live handle on all eight scenarios.  carried: after a cycle and a carried-over reset - plant and stored influent are
    both its own; otherwise fresh from reset(rnd=...).  stepped: one more cycle behind the carried-over reset."""
    import torch
    rs = np.random.RandomState(seed)
    env = make_env(G, n, scheme, f64)
    env.reset(scenario=scen(n), rnd=rs.randn(n, 48))
    if carried:
        env.step(torch.from_numpy(rs.uniform(0.1, 0.9, (n, 3))).cuda())
        env.reset(scenario=scen(n), rnd=rs.randn(n, 48), carry_over=True)
        if stepped:
            env.step(torch.from_numpy(rs.uniform(0.1, 0.9, (n, 3))).cuda())
    return env


def candidates(env, n_cycles, k, seed):
    """[n_cycles, N, K, 3] ~ U(-0.2, 1.2) in the handle's action dtype: out-of-range values included (the kernel clips)."""
    import torch
    a = np.random.RandomState(seed).uniform(-0.2, 1.2, (n_cycles, env.num_envs, k, 3))
    return torch.from_numpy(a).to(env.action_dtype).cuda()


def handle_bits(env):
    x, c = env.get_state()
    return x, c, env.influent()


def assert_untouched(env, before):
    import torch
    from gym_sbr2_amd import _capi
    x, c, infl = handle_bits(env)
    assert torch.equal(before[0], x), "the plant moved"
    assert torch.equal(before[2], infl), "the stored influent moved"
    for row in range(_capi.NCTRL):
        assert same(before[1][row], c[row]), "controller row %d moved" % row


def assert_goes_on_like(env, twin, act):
    """The handle goes on as if nothing had happened: its next step() gives the bits of a twin that never looked ahead."""
    obs_a, rew_a, _ = env.step(act)
    obs_t, rew_t, _ = twin.step(act)
    assert same(obs_a, obs_t) and same(rew_a, rew_t) and same(env.diag, twin.diag), "the step after the lookahead differs"
    for u, v in zip(env.get_state(), twin.get_state()):
        assert same(u, v), "the state after the step differs"


def replicas(G, env, cand, infl=None, n_scen=1, models=None, f64=False):
    """The checker: the EXISTING per-cycle kernel, through the existing API only.  Per cycle c: (reward, cobs [.., 3],
    diag [.., 12], the C_STATUS row), every entry shaped [N, K, S, ..].  Future s runs on a handle created with the config
    models[s % M] - the live handle's own with models None - that holds the live handle's state and is fed, per cycle,
    reset(influent = infl[c, :, s], or the live handle's stored influent with infl None, carry_over=True) and step(cand[c]).
    The futures of one config share one handle of N*K*(their number) envs, rows in (env, candidate, future) order: one handle
    of N*K*S envs under the handle's own config."""
    import torch
    from gym_sbr2_amd import _capi
    n_cycles, n, k = cand.shape[:3]
    cfgs = [env.cfg] if models is None else models
    x, ctrl = env.get_state()
    stored = env.influent().T.contiguous()
    shapes = ((), (3,), (_capi.NCYC_DIAG,), ())
    out = [[None] * 4 for _ in range(n_cycles)]
    for m, cfg in enumerate(cfgs[:n_scen]):
        mine = list(range(m, n_scen, len(cfgs)))                                # the futures under this config
        s, b = len(mine), n * k * len(mine)
        rep = make_env(G, b, cfg=cfg, f64=f64)
        rep.set_state(x.repeat_interleave(k * s, dim=1), ctrl.repeat_interleave(k * s, dim=1))
        for c in range(n_cycles):
            rows = stored[:, None].expand(n, s, _capi.NX) if infl is None else infl[c][:, mine]
            rep.reset(influent=rows[:, None].expand(n, k, s, _capi.NX).reshape(b, _capi.NX).contiguous(), carry_over=True)
            obs, rew, _ = rep.step(cand[c][:, :, None].expand(n, k, s, 3).reshape(b, 3).contiguous())
            parts = (rew, obs, rep.diag, rep.ctrl_row(_capi.C_STATUS).to(torch.int64))
            for q, (part, trailing) in enumerate(zip(parts, shapes)):
                if out[c][q] is None:
                    out[c][q] = torch.empty((n, k, n_scen) + trailing, dtype=part.dtype, device=part.device)
                out[c][q][:, :, mine] = part.reshape((n, k, s) + trailing)
        torch.cuda.synchronize()
        rep.close()
    return [tuple(cyc) for cyc in out]


def check_against_replicas(env, got, cand, n_scen, rep):
    """Every output of a lookahead called with every return_* flag against the replicas' cycles `rep`, with == on values.
    n_scen None: cycle_lookahead's seven results, [N, K] per branch, the winners reduced from the returns; otherwise the nine of
    cycle_lookahead_scenarios / _models, [N, K, S] per branch, mean and worst as gpu_common.host_stats has them and the winners
    reduced from the means."""
    import torch
    n_cycles, (n, k) = cand.shape[0], tuple(cand.shape[1:3])
    if n_scen is None:
        ret, rew, bi, bv, obs_end, diag_end, status = got
        rep = [tuple(t.squeeze(2) for t in cyc) for cyc in rep]
        per, scored = (n, k), ret
    else:
        ret, rew, mean, worst, bi, bv, obs_end, diag_end, status = got
        per, scored = (n, k, n_scen), mean
        assert mean.shape == worst.shape == (n, k) and mean.dtype == worst.dtype == torch.float64, (mean.shape, mean.dtype)
        hm, hw = host_stats(ret)
        assert np.array_equal(mean.cpu().numpy(), hm, equal_nan=True), "mean"
        assert np.array_equal(worst.cpu().numpy(), hw, equal_nan=True), "worst"
    assert ret.shape == per and ret.dtype == torch.float64, (ret.shape, ret.dtype)
    assert rew.shape == (n_cycles,) + per and rew.dtype == torch.float64, (rew.shape, rew.dtype)
    assert obs_end.shape == per + (3,) and diag_end.shape == per + (12,), (obs_end.shape, diag_end.shape)
    assert obs_end.dtype == diag_end.dtype == torch.float64, (obs_end.dtype, diag_end.dtype)
    assert status.shape == per and status.dtype == torch.uint8, (status.shape, status.dtype)
    acc, st = torch.zeros_like(ret), torch.zeros_like(rep[0][3])
    for c in range(n_cycles):
        assert same(rew[c].to(env.out_dtype), rep[c][0]), "reward of cycle %d" % c
        acc = acc + rew[c]
        st |= rep[c][3]
    assert same(ret, acc), "returns are the float64 sum of rewards_out in cycle order"
    assert same(obs_end.to(env.out_dtype), rep[n_cycles - 1][1]), "obs_end"
    assert same(diag_end, rep[n_cycles - 1][2]), "diag_end"
    assert torch.equal(status.to(torch.int64), st), "status"
    idx, val = host_best(scored)
    assert np.array_equal(bi.cpu().numpy(), idx), "best_index"
    assert np.array_equal(bv.cpu().numpy(), val, equal_nan=True), "best_value"
    assert bool((rew != 0).any()), "a comparison of zeros"
    if ret.numel() > 1:
        assert len(torch.unique(ret)) > 1, "a comparison of one value"
    return ret


def sentinel_outputs(n, k, n_scen):
    """Every output of the family for (n, k, n_scen), filled with 7 on the device: ({name: tensor}, {name: its pointer})."""
    import torch
    b = n * k * n_scen
    outs = {name: torch.full(shape, 7, dtype=dt, device="cuda") for name, shape, dt in (
        ("ret", (b,), torch.float64), ("rew", (b,), torch.float64), ("mean", (n * k,), torch.float64), ("worst", (n * k,), torch.float64),
        ("bi", (n,), torch.int32), ("bv", (n,), torch.float64), ("obs", (b, 3), torch.float64), ("diag", (b, 12), torch.float64),
        ("st", (b,), torch.uint8))}
    return outs, {name: C.c_void_p(t.data_ptr()) for name, t in outs.items()}


def assert_sentinels(outs):
    import torch
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert bool((t == 7).all()), name + " was written"


# ---------------------------------------------------------------------------------------------- without a GPU
def assert_declared_exported_and_bound(entries):
    """entries: {symbol: (a regular expression its declaration in include/sbr_amd.h matches, its number of arguments)}."""
    from conftest import ROOT

    from gym_sbr2_amd import _capi
    with open(os.path.join(ROOT, "include", "sbr_amd.h")) as f:
        header = f.read()
    assert "#define SBR_ABI_VERSION 6" in header, "the header's ABI version"
    lib = _capi.load()
    raw = C.CDLL(_capi.library_path())
    for name, (declaration, n_args) in entries.items():
        assert re.search(declaration, header, re.M), name + " is not declared as expected"
        assert getattr(raw, name) is not None, name
        res, args = _capi.SYMBOLS[name]
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args and len(args) == n_args, name
    assert lib.sbr_abi_version() == 6, "added functions: no signature, struct or record width changed"
    return lib


def host_outputs():
    """Host stand-ins for the family's outputs, filled with 7, and a tape and an influent to point at: (bufs, pointers by name).
    No handle can exist without a device, so no call that gets them writes them."""
    bufs = {name: (ct * n)(*[7] * n) for name, ct, n in (
        ("ret", C.c_double, 4), ("rew", C.c_double, 4), ("mean", C.c_double, 2), ("worst", C.c_double, 2), ("idx", C.c_int32, 2),
        ("best", C.c_double, 2), ("obs", C.c_double, 12), ("diag", C.c_double, 48), ("st", C.c_uint8, 4), ("draws", C.c_double, 28))}
    p = {name: C.cast(v, C.c_void_p) for name, v in bufs.items()}
    p["tape"], p["infl"] = C.cast((C.c_float * 12)(), C.c_void_p), C.cast((C.c_double * 28)(), C.c_void_p)
    return bufs, p


def assert_null_env_refused(entry, calls, bufs):
    """NULL env is the last check: it names the entry point whatever else is wrong with `calls`, and `bufs` keep their 7s."""
    from gym_sbr2_amd import _capi
    lib = _capi.load()
    for args in calls:
        assert getattr(lib, entry)(*args) == -1, (entry, args)
        assert lib.sbr_last_error(None) == (entry + ": NULL env").encode(), lib.sbr_last_error(None)
    for name, v in bufs.items():
        assert list(v) == [7] * len(v), name + " was written"


def assert_unit_of_its_own(unit, builds, others=()):
    """`unit` is one of the library's sources, and it alone holds the kernels `builds` (the mangled names of a lookahead's six
    builds, up to their parameter lists) and one kernel per prefix of `others` - and no kernel besides."""
    from isa import kernel_names, unit_asms

    from gym_sbr2_amd import build as B
    assert os.path.join(os.path.dirname(B.SRC), unit) in B.SOURCES, unit
    want = sorted(builds)
    stem = want[0][:want[0].index("I")]                                      # _Z<length><name>, in front of the template arguments
    owners = {u for u, text in unit_asms().items() if any(n.startswith((stem,) + tuple(others)) for n in kernel_names(text))}
    assert owners == {unit}, owners
    names = sorted(kernel_names(unit_asms()[unit]))
    rest = [n for n in names if n.startswith(tuple(others))] if others else []
    assert len(rest) == len(others) and len(names) == len(want) + len(others), names
    assert sorted(n[:len(want[0])] for n in names if n not in rest) == want, names
