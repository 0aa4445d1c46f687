"""sbr_lookahead_policy without a GPU: the entry point is declared, exported and bound, a NULL env is refused, the three Python
surfaces exist, and the gfx950 ISA of k_lookahead_policy (tests/isa.py) stays inside its parent's budget: k_rollout_policy of
the same build, read from the same assembly, is the bound on registers, scratch and vector stores - not a literal."""
import ctypes as C
import inspect
import os
import re

import pytest
from conftest import ROOT
from isa import K_POL, b5_steps, f64_mix, flop_counts, instructions, kernel_text, library_asm, meta, vector_stores

from gym_sbr2_amd import _capi

BUILDS = [(h, sch, wv) for h in (32, 64) for sch, wv in ((1, 1), (1, 2), (0, 2))]      # the SBROS-v1 reward: OCI = false
# k_lookahead_policy<H, false, SCH, WAVES>
K_LOOK_POL = {(h, sch, wv): "_Z18k_lookahead_policyILi%dELb0ELi%dELi%dEE" % (h, sch, wv) for h, sch, wv in BUILDS}
ARGS = ["self", "policy", "fanout", "n_steps", "hold", "obs", "noise_std", "noise_seed", "keep_mean", "return_rewards",
        "return_best", "return_actions", "return_end"]


def test_the_header_declares_it_and_the_binding_binds_it():
    with open(os.path.join(ROOT, "include", "sbr_amd.h")) as f:
        header = f.read()
    m = re.search(r"\nint sbr_lookahead_policy\(([^;]*)\);", header)
    assert m, "include/sbr_amd.h does not declare sbr_lookahead_policy"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["sbr_env* env", "int32_t n_steps", "int32_t hold", "int32_t fanout", "const sbr_policy* policy",
                      "int32_t keep_mean", "const float* obs", "double* returns", "double* rewards_out", "int32_t* best_index",
                      "double* best_return", "float* actions_out", "float* obs_end", "float* state_end", "uint8_t* done_end",
                      "void* stream"], params
    assert "#define SBR_ABI_VERSION 6" in header
    res, args = _capi.SYMBOLS["sbr_lookahead_policy"]
    assert res is C.c_int and len(args) == len(params)
    assert args[4] == C.POINTER(_capi.SbrPolicy) and [args[k] for k in (1, 2, 3, 5)] == [C.c_int32] * 4
    lib = _capi.load()
    raw = C.CDLL(_capi.library_path())
    assert getattr(raw, "sbr_lookahead_policy") is not None and lib.sbr_lookahead_policy.argtypes is not None
    assert lib.sbr_abi_version() == 6


def test_a_null_env_is_refused():
    lib = _capi.load()
    blk = (C.c_float * 1730)()
    pol = _capi.SbrPolicy(params=C.cast(blk, C.c_void_p), n_hidden=2, width=32, activation=0, squash=1, n_policies=1,
                          envs_per_policy=0, act_scale=(C.c_float * 2)(1.25, 7.5), act_bias=(C.c_float * 2)(1.25, 7.5),
                          noise_std=(C.c_float * 2)(0.0, 0.0), noise_seed=0)
    obs = (C.c_float * 18)(*([0.25] * 18))
    ret = (C.c_double * 3)(7.0, 7.0, 7.0)
    rc = lib.sbr_lookahead_policy(None, 1, 1, 3, C.byref(pol), 0, C.cast(obs, C.c_void_p), C.cast(ret, C.c_void_p), None, None, None,
                                  None, None, None, None, None)
    msg = lib.sbr_last_error(None)
    assert rc == -1 and b"sbr_lookahead_policy" in msg and b"NULL env" in msg, (rc, msg)       # SBR_ERR_INVALID
    assert list(ret) == [7.0] * 3 and list(obs) == [0.25] * 18


def test_python_surfaces_exist():
    import gym_sbr2_amd
    from gym_sbr2_amd import SbrEnv2Vec, SbrOSVec, ShardedSbrOS
    for cls in (SbrOSVec, ShardedSbrOS):
        sig = inspect.signature(cls.lookahead_policy)
        assert list(sig.parameters) == ARGS, cls
        d = {k: v.default for k, v in sig.parameters.items()}
        assert [d[k] for k in ARGS[4:]] == [1, None, None, 0, False, False, False, False, False], cls
    sig = inspect.signature(gym_sbr2_amd.PolicyRolloutPlanner.__init__)
    assert list(sig.parameters)[:8] == ["self", "env", "policy", "fanout", "n_steps", "hold", "noise_std", "terminal_value"]
    assert sig.parameters["terminal_value"].default is None and callable(gym_sbr2_amd.PolicyRolloutPlanner.plan)
    # SBR-v2 refuses as its siblings do, before it looks at an argument (no handle can exist without a device)
    with pytest.raises(NotImplementedError, match="SBROS-v1"):
        SbrEnv2Vec.lookahead_policy(None)
    with pytest.raises(NotImplementedError, match="SBROS-v1"):
        SbrEnv2Vec.lookahead(None)


@pytest.fixture(scope="module")
def asm():
    return library_asm()


def test_every_build_exists_and_stays_inside_k_rollout_policys_budget(asm):
    for b in BUILDS:
        k, parent = K_LOOK_POL[b], K_POL[b]
        text = kernel_text(asm, k)                                         # asserts that the mangled name is there
        regs = meta(asm, k, "vgpr_count") + meta(asm, k, "agpr_count")
        regs_p = meta(asm, parent, "vgpr_count") + meta(asm, parent, "agpr_count")
        scr, scr_p = meta(asm, k, "private_segment_fixed_size"), meta(asm, parent, "private_segment_fixed_size")
        st, st_p = len(vector_stores(asm, k)), len(vector_stores(asm, parent))
        print("%s: registers %d (parent %d), scratch %d B (parent %d), vector stores %d (parent %d), %d instructions"
              % (b, regs, regs_p, scr, scr_p, st, st_p, len(instructions(text))))
        assert regs <= regs_p, (b, regs, regs_p)
        assert scr <= scr_p, (b, scr, scr_p)
        assert st <= st_p, (b, st, st_p)                                   # the parent has the plant and record stores on top
        if b[2] == 1:                                                      # the one-wave builds: no scratch segment at all
            assert scr == 0 and f64_mix(instructions(text))["scratch"] == 0, (b, scr)


def test_the_step_loops_hold_the_integrators_arithmetic_and_no_scratch(asm):
    import bench
    for b in BUILDS:
        if b[1] != 1:
            continue                                                       # scheme 0 has no Butcher-5 step loop
        steps = b5_steps(kernel_text(asm, K_LOOK_POL[b]), 700)
        assert len(steps) >= 2, b
        flop = flop_counts(steps)
        assert flop[0] == bench.FP64_FLOP_PER_B5_STEP["plain"] and flop[-1] == bench.FP64_FLOP_PER_B5_STEP["dosing"], (b, flop)
        for l in steps:
            m = f64_mix(l)
            assert m["div"] == 0 and m["scratch"] == 0, (b, m)
