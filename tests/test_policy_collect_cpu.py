"""sbr_collect_policy without a GPU: the entry point is declared, exported and bound, every refusal is decided before anything is
touched, the Python surface exists on all three classes, and the gfx950 ISA of k_collect_policy (cross-compiled once per run,
tests/isa.py) keeps k_rollout_policy's contract: one owning unit, no scratch in the one-wave builds, 256 registers in the
others, the tape kernel's arithmetic in the Butcher-5 step loops, the same net and no more per-lane loads."""
import collections
import ctypes as C
import inspect
import os
import re

import pytest
from conftest import ROOT
from isa import K_POL, K_TAPE, K_TAPE_2W, b5_steps, f64_mix, flop_counts, instructions, kernel_names, kernel_text, library_asm, meta, unit_asms
from test_policy_rollout_cpu import _policy

from gym_sbr2_amd import _capi

# k_collect_policy<H, false, SCH, WAVES>: the SBROS-v1 reward; the builds of tests/isa.py's K_POL
K_COL = {(h, sch, wv): "_Z16k_collect_policyILi%dELb0ELi%dELi%dEE" % (h, sch, wv) for h in (32, 64) for sch, wv in ((1, 1), (1, 2), (0, 2))}


def test_symbol_is_declared_exported_and_bound():
    lib = _capi.load()
    raw = C.CDLL(_capi.library_path())
    assert "sbr_collect_policy" in _capi.SYMBOLS and raw.sbr_collect_policy is not None
    assert len(lib.sbr_collect_policy.argtypes) == 11
    assert lib.sbr_abi_version() == 6 == _capi.ABI_VERSION
    with open(os.path.join(ROOT, "include", "sbr_amd.h")) as f:
        header = f.read()
    m = re.search(r"^int sbr_collect_policy\(([^;]*)\);", header, re.M)
    assert m and len(m.group(1).split(",")) == 11
    assert re.search(r"^#define SBR_DF_TAKEN %d$" % _capi.DF_TAKEN, header, re.M)
    assert re.search(r"^#define SBR_DF_ENDED %d$" % _capi.DF_ENDED, header, re.M)
    assert (_capi.DF_TAKEN, _capi.DF_ENDED) == (1, 2)
    assert re.search(r"^#define SBR_ABI_VERSION 6$", header, re.M)


def test_every_refusal_is_decided_before_anything_is_touched():
    """As tests/test_policy_rollout_cpu.py checks sbr_rollout_policy: no handle can exist without a device, so every call is
    refused, and the message names the LAST failing check, which shows that the argument under test was looked at."""
    lib = _capi.load()
    obs = (C.c_float * 18)(*([0.25] * 18))
    ret = (C.c_double * 1)(7.0)
    rows = (C.c_float * 18)(*([0.5] * 18))
    flags = (C.c_uint8 * 1)(9)
    o, r = C.cast(obs, C.c_void_p), C.cast(ret, C.c_void_p)
    oo, fo = C.cast(rows, C.c_void_p), C.cast(flags, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def refused(why, n_steps=1, hold=1, policy=True, obs_ptr=o, obs_out=oo, flags_out=fo, **kw):
        p = _policy(**kw) if policy else None
        rc = lib.sbr_collect_policy(None, n_steps, hold, C.byref(p) if p is not None else None, obs_ptr, r, None, None, obs_out,
                                    flags_out, None)
        msg = lib.sbr_last_error(None)
        assert rc == -1 and b"sbr_collect_policy: " in msg and why in msg, (why, rc, msg)

    # every refusal of sbr_rollout_policy
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
    # its own: without either per-decision output it is sbr_rollout_policy, and says so
    refused(b"both NULL: call sbr_rollout_policy", obs_out=None, flags_out=None)
    refused(b"NULL env", obs_out=None)                    # one of the two is enough
    refused(b"NULL env", flags_out=None)
    refused(b"NULL env", n_steps=0)                       # n_steps = 0 is a valid call
    assert list(ret) == [7.0] and list(obs) == [0.25] * 18 and list(rows) == [0.5] * 18 and list(flags) == [9]


def test_python_surface_exists():
    from gym_sbr2_amd import ShardedSbrOS, SbrEnv2Vec, SbrOSVec
    from gym_sbr2_amd.vec_env import PolicyCollection
    for cls in (SbrOSVec, ShardedSbrOS):
        sig = inspect.signature(cls.collect_policy)
        assert list(sig.parameters) == ["self", "policy", "n_steps", "hold", "obs", "noise_std", "noise_seed"]
        d = {k: v.default for k, v in sig.parameters.items()}
        assert (d["hold"], d["obs"], d["noise_std"], d["noise_seed"]) == (1, None, None, 0)
    assert PolicyCollection._fields == ("obs", "actions", "rewards", "flags", "returns", "last_obs")
    assert isinstance(PolicyCollection.taken, property) and isinstance(PolicyCollection.ended, property)
    # SBR-v2 refuses it in the words of its siblings
    sib = inspect.getsource(SbrEnv2Vec.lookahead_policy)
    src = inspect.getsource(SbrEnv2Vec.collect_policy)
    tail = "belongs to SBROS-v1; SBR-v2 already runs a whole cycle per launch"
    assert "NotImplementedError" in src and tail in src and tail in sib


def test_flag_views():
    torch = pytest.importorskip("torch")
    from gym_sbr2_amd.vec_env import PolicyCollection
    f = torch.tensor([[0, 1, 3]], dtype=torch.uint8)
    c = PolicyCollection(None, None, None, f, None, None)
    assert c.taken.tolist() == [[False, True, True]] and c.ended.tolist() == [[False, False, True]]
    assert c.taken.dtype == torch.bool and c.ended.dtype == torch.bool


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def test_collector_kernels_are_owned_by_exactly_one_unit():
    from gym_sbr2_amd import build as B
    assert os.path.join(os.path.dirname(B.SRC), "sbr_policy_collect.hip") in B.SOURCES
    with open(B.SRC) as f:
        assert '#include "sbr_policy_collect.hip"' in f.read()
    owners = collections.defaultdict(list)
    for unit, text in unit_asms().items():
        for k in kernel_names(text):
            if "k_collect_policy" in k:
                owners[k].append(unit)
    assert len(owners) == 12, sorted(owners)              # H x OCI x {(1, 1), (1, 2), (0, 2)}
    assert all(sum(k.startswith(prefix) for k in owners) == 1 for prefix in K_COL.values()), sorted(owners)
    assert all(u == ["sbr_policy_collect.hip"] for u in owners.values()), dict(owners)
    # ... and that unit owns nothing else
    assert all("k_collect_policy" in k for k in kernel_names(unit_asms()["sbr_policy_collect.hip"]))


def test_collector_register_budgets_and_scratch(asm):
    for h in (32, 64):
        k = K_COL[h, 1, 1]
        assert meta(asm, k, "private_segment_fixed_size") == 0, h
        assert f64_mix(instructions(kernel_text(asm, k)))["scratch"] == 0, h
        assert meta(asm, k, "vgpr_count") <= 512
        assert meta(asm, K_COL[h, 1, 2], "vgpr_count") <= 256 and meta(asm, K_COL[h, 0, 2], "vgpr_count") <= 256


def test_collector_step_loops_are_the_tape_kernels(asm):
    import bench
    tape_scratch = {1: max(f64_mix(l)["scratch"] for l in b5_steps(kernel_text(asm, K_TAPE), 700)),
                    2: max(f64_mix(l)["scratch"] for l in b5_steps(kernel_text(asm, K_TAPE_2W), 700))}
    for h in (32, 64):
        for wv in (1, 2):
            k = K_COL[h, 1, wv]
            steps = b5_steps(kernel_text(asm, k), 700)
            assert len(steps) >= 2, k
            flop = flop_counts(steps)
            assert flop[0] == bench.FP64_FLOP_PER_B5_STEP["plain"] and flop[-1] == bench.FP64_FLOP_PER_B5_STEP["dosing"], (k, flop)
            for l in steps:
                m = f64_mix(l)
                assert m["fma"] + m["mul"] + m["add"] + m["rcp"] in (477, 537), (k, m)
                assert m["div"] == 0, k                               # no v_div_fmas_f64 in any step loop
                assert m["scratch"] <= tape_scratch[wv], (k, m["scratch"], tape_scratch[wv])


def test_the_net_and_the_loads_are_the_rollout_kernels(asm):
    fma32 = lambda k: sum(v for op, v in collections.Counter(i.split()[0] for i in instructions(kernel_text(asm, k))).items()   # noqa: E731
                          if op.startswith("v_fma_f32") or op.startswith("v_fmac_f32"))
    gl = lambda k: sum(1 for i in instructions(kernel_text(asm, k)) if i.startswith("global_load") or i.startswith("flat_load"))   # noqa: E731
    for key in K_COL:
        assert fma32(K_COL[key]) == fma32(K_POL[key]), (key, fma32(K_COL[key]), fma32(K_POL[key]))
        assert gl(K_COL[key]) <= gl(K_POL[key]), (key, gl(K_COL[key]), gl(K_POL[key]))


def test_the_rows_go_out_through_ordinary_vector_stores(asm):
    """The observation row and the flag byte add vector stores to k_rollout_policy's and nothing else that writes memory."""
    for key in K_COL:
        ops = collections.Counter(i.split()[0] for i in instructions(kernel_text(asm, K_COL[key])))
        pol = collections.Counter(i.split()[0] for i in instructions(kernel_text(asm, K_POL[key])))
        stores = lambda c: sum(v for op, v in c.items() if op.startswith(("global_store", "flat_store")))   # noqa: E731
        assert ops["global_store_byte"] >= 1, key
        assert stores(ops) > stores(pol), key
        new = set(ops) - set(pol)
        assert not any(op.startswith(("ds_", "global_atomic", "flat_atomic", "buffer_")) for op in new), (key, sorted(new))
