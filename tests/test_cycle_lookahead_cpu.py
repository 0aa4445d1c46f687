"""sbr_cycle_lookahead without a GPU: the entry point is declared, exported and bound, it refuses a NULL handle before anything is
touched, the Python surface exists, the kernel lives in a translation unit of its own, and its gfx950 ISA (from the once-per-run
cross-compile of tests/isa.py) needs no more registers and no more scratch than k_cycle's build of the same scheme and waves,
with a store count bounded by its outputs.  The device-side refusals are in tests/test_cycle_lookahead_gpu.py."""
import inspect

import pytest
from cycle_kit import assert_declared_exported_and_bound, assert_null_env_refused, assert_unit_of_its_own, host_outputs
from isa import library_asm, meta, vector_stores

from gym_sbr2_amd import _capi

UNIT = "sbr_cycle_lookahead.hip"
# (cfg.scheme, waves per SIMD) of the builds: scheme 0 has no one-wave build.  float32 tape, float32 outputs of k_cycle.
BUILDS = ((1, 1), (1, 2), (0, 2))
K_LOOK = {b: "_Z17k_cycle_lookaheadIfLi%dELi%dEE" % b for b in BUILDS}
K_CYCLE = {b: "_Z7k_cycleIffLi%dELi%dEE" % b for b in BUILDS}


def test_symbol_is_declared_exported_and_bound():
    assert_declared_exported_and_bound({"sbr_cycle_lookahead": (
        r"^int sbr_cycle_lookahead\(sbr_env\* env, int32_t n_cycles, int32_t fanout, const void\* actions,", 12)})


def test_null_env_is_refused_before_anything_is_touched():
    bufs, p = host_outputs()
    outs = tuple(p[name] for name in "rew idx best obs diag st".split())
    assert_null_env_refused("sbr_cycle_lookahead", [(None, 1, 2, p["tape"], p["ret"]) + outs + (None,),
                                                    (None, -1, 0, None, None) + outs + (None,)], bufs)


def test_python_surface():
    pytest.importorskip("torch")
    import gym_sbr2_amd
    from gym_sbr2_amd import cycle_env, planner
    from gym_sbr2_amd.cycle_env import SbrEnv2Vec
    sig = inspect.signature(SbrEnv2Vec.cycle_lookahead)
    assert list(sig.parameters) == ["self", "candidates", "return_rewards", "return_best", "return_end", "return_status"]
    assert [p.default for p in sig.parameters.values()][2:] == [False] * 4
    assert "cycle_lookahead" not in cycle_env._REFUSED and "cycle_lookahead" not in vars(SbrEnv2Vec)
    assert SbrEnv2Vec.cycle_lookahead is cycle_env.CycleLookahead.cycle_lookahead
    with pytest.raises(ValueError):                    # it looks at its arguments: not a refusal
        SbrEnv2Vec.cycle_lookahead(None, [[0.5, 0.5, 0.5]])
    assert gym_sbr2_amd.CycleSetpointSearch is planner.CycleSetpointSearch
    assert list(inspect.signature(planner.CycleSetpointSearch.__init__).parameters) == ["self", "env", "K", "n_cycles", "iters",
                                                                                         "elite_frac", "seed"]
    assert not hasattr(gym_sbr2_amd.ShardedSbrOS, "cycle_lookahead")      # sharding of the per-cycle env is out of scope


def test_setpoint_search_on_a_stand_in_env():
    """The search's own logic, on the CPU, around a stand-in for the env: return = -|a - 0.3|^2 summed over the tape.  Env 0 is
    ordinary; every candidate of env 1 is flagged NEAR_POLE; env 2 flags whatever lies above 0.4 (the all-0.5 start included) and
    returns NaN above 0.8.  A flagged or NaN candidate never wins where a clean one exists, an env without one keeps the
    all-0.5 tape, and `status` says which is which."""
    torch = pytest.importorskip("torch")
    from gym_sbr2_amd.planner import CycleSetpointSearch

    class Env:
        num_envs, device, action_dtype = 3, torch.device("cpu"), torch.float32

        def cycle_lookahead(self, cand, return_status=False):
            a = cand.to(self.action_dtype).double()
            ret = -((a - 0.3) ** 2).sum(dim=(0, 3))
            st = torch.zeros(ret.shape, dtype=torch.uint8)
            st[1] = _capi.ST_NEAR_POLE
            st[2] = torch.where((a[..., 0] > 0.4).any(0)[2], _capi.ST_NEAR_POLE, 0).to(torch.uint8)
            ret[2] = torch.where((a[..., 0] > 0.8).any(0)[2], float("nan"), ret[2])
            return ret, st

    env = Env()
    search = CycleSetpointSearch(env, K=32, n_cycles=2, iters=4, elite_frac=0.25, seed=3)
    action, value = search.plan()
    ret, st = env.cycle_lookahead(search.tape[:, :, None, :])
    assert torch.equal(value, ret[:, 0]) and torch.equal(search.status, st[:, 0]) and torch.equal(action, search.tape[0].float())
    half = env.cycle_lookahead(torch.full((2, 3, 1, 3), 0.5, dtype=torch.float64))[0][:, 0]
    assert value[0] > half[0] and int(search.status[0]) == 0                      # the search moved towards 0.3
    assert torch.equal(search.tape[:, 1], torch.full((2, 3), 0.5, dtype=torch.float64)) and int(search.status[1]) == _capi.ST_NEAR_POLE
    assert int(search.status[2]) == 0 and bool((search.tape[:, 2, 0] <= 0.4).all()) and not bool(value.isnan().any())


def test_the_kernel_has_a_unit_of_its_own():
    # the six builds, float32 and float64 tapes, and no other kernel: k_branch_best stays sbr_tape.hip's
    assert_unit_of_its_own(UNIT, ["_Z17k_cycle_lookaheadI%sLi%dELi%dEE" % ((t,) + b) for t in "fd" for b in BUILDS])


@pytest.fixture(scope="module")
def asm():
    return library_asm()


@pytest.mark.parametrize("build", BUILDS, ids=["scheme%d-%dwave" % b for b in BUILDS])
def test_no_more_registers_and_no_more_scratch_than_k_cycle(asm, build):
    """The yardstick is k_cycle's build of the same scheme and waves in the SAME compile, not a number written here: the
    lookahead drops the state stores and adds a loop around the cycle, so it has no reason to need more.
    Measured (this compile): scheme 1 one wave 272 registers against 278, no scratch in either; scheme 0 two waves 221 against
    225, no scratch in either; scheme 1 two waves 254 registers against 255 and 68 B of scratch against 92 B - both builds want
    more than the 256 registers two waves per SIMD leave them and spill beyond, and the lookahead's is held to 254 by an
    attribute of its own (left to the allocator it names 256)."""
    look, cyc = K_LOOK[build], K_CYCLE[build]
    figures = {k: (meta(asm, look, k), meta(asm, cyc, k)) for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size")}
    print("[info] k_cycle_lookahead against k_cycle, scheme %d, %d wave(s): %s" % (build + (figures,)))
    assert figures["private_segment_fixed_size"][0] <= figures["private_segment_fixed_size"][1], figures
    assert figures["vgpr_count"][0] <= figures["vgpr_count"][1], figures


@pytest.mark.parametrize("build", BUILDS, ids=["scheme%d-%dwave" % b for b in BUILDS])
def test_stores_no_more_than_the_outputs_need(asm, build):
    """returns 1, one rewards_out entry 1, the end rows 3 + 12 values, the status byte 1: 18 stores if none of them merge (the
    backend merges adjacent doubles of a row into 16-byte stores: measured 11).  Nothing of the handle's 14 + 25 + 14 rows is
    among them: k_cycle, which stores the plant, has 25."""
    stores = vector_stores(asm, K_LOOK[build])
    assert len(stores) <= 1 + 1 + 3 + 12 + 1, stores
    assert len(stores) < len(vector_stores(asm, K_CYCLE[build]))
