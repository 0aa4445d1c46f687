"""sbr_draw_influent and sbr_cycle_lookahead_scenarios without a GPU: the entry points are declared, exported and bound, they
refuse a NULL handle before anything is touched, the Python surface exists, RobustCycleSetpointSearch optimises what it says it
does (on a stand-in env), the kernels live in a translation unit of their own, and their gfx950 ISA (from the once-per-run
cross-compile of tests/isa.py) needs no more scratch than k_cycle's build of the same scheme and waves, with a store count bounded
by the outputs.  The device-side checks are in tests/test_cycle_scenarios_gpu.py."""
import inspect
import types

import numpy as np
import pytest
from cycle_kit import assert_declared_exported_and_bound, assert_null_env_refused, assert_unit_of_its_own, host_outputs
from isa import kernel_names, library_asm, meta, unit_asms, vector_stores

from gym_sbr2_amd import _capi

UNIT = "sbr_cycle_scenarios.hip"
# (cfg.scheme, waves per SIMD) of the builds: scheme 0 has no one-wave build
BUILDS = ((1, 1), (1, 2), (0, 2))
K_SCEN = {(t,) + b: "_Z27k_cycle_lookahead_scenariosI%sLi%dELi%dEE" % ((t,) + b) for t in "fd" for b in BUILDS}     # float32 / float64 tape
K_CYCLE = {b: "_Z7k_cycleIffLi%dELi%dEE" % b for b in BUILDS}
K_STATS = "_Z16k_scenario_stats"
ALL = sorted(K_SCEN)
ALL_IDS = ["%s-scheme%d-%dwave" % (("f32" if t == "f" else "f64"), s, w) for t, s, w in ALL]


def test_symbols_are_declared_exported_and_bound():
    assert_declared_exported_and_bound({
        "sbr_draw_influent": (r"^int sbr_draw_influent\(sbr_env\* env, uint64_t seed, int32_t rows, int32_t per_env, int32_t first_draw,", 8),
        "sbr_cycle_lookahead_scenarios": (
            r"^int sbr_cycle_lookahead_scenarios\(sbr_env\* env, int32_t n_cycles, int32_t fanout, int32_t n_scen,", 16)})


def test_null_env_is_refused_before_anything_is_touched():
    bufs, p = host_outputs()
    outs = tuple(p[name] for name in "ret rew mean worst idx best obs diag st".split())
    assert_null_env_refused("sbr_cycle_lookahead_scenarios", [(None, 1, 2, 2, p["tape"], p["infl"]) + outs + (None,),
                                                              (None, -1, 0, 0, None, None, None) + outs[1:] + (None,)], bufs)
    assert_null_env_refused("sbr_draw_influent", [(None, 0, 1, 2, 0, None, p["draws"], None), (None, 0, 0, 0, -1, None, None, None)], bufs)


def test_python_surface():
    pytest.importorskip("torch")
    import gym_sbr2_amd
    from gym_sbr2_amd import cycle_env, planner
    from gym_sbr2_amd.cycle_env import CycleLookahead, SbrEnv2Vec
    want = {
        "draw_influent": (["self", "rows", "per_env", "seed", "scenario", "first_draw"], [0, None, 0]),
        "influent_futures": (["self", "n_cycles", "n_scen", "seed", "scenario", "first_draw", "current_first"], [0, None, 0, True]),
        "cycle_lookahead_scenarios": (["self", "candidates", "influent", "return_rewards", "return_stats", "return_best", "return_end",
                                       "return_status"], [False] * 5),
    }
    for name, (params, defaults) in want.items():
        sig = inspect.signature(getattr(SbrEnv2Vec, name))
        assert list(sig.parameters) == params, name
        assert [p.default for p in sig.parameters.values() if p.default is not inspect.Parameter.empty] == defaults, name
        assert name not in cycle_env._REFUSED and name not in vars(SbrEnv2Vec) and getattr(SbrEnv2Vec, name) is vars(CycleLookahead)[name]
    one_env = types.SimpleNamespace(num_envs=1)
    for cand, infl in ((np.zeros((1, 3)), np.zeros((1, 1, 1, 14))), (np.zeros((1, 1, 1, 3)), np.zeros((1, 1, 1, 13))),
                       (np.zeros((2, 1, 1, 3)), np.zeros((1, 1, 1, 14)))):      # it looks at its arguments: not a refusal
        with pytest.raises(ValueError):
            SbrEnv2Vec.cycle_lookahead_scenarios(one_env, cand, infl)
    assert gym_sbr2_amd.RobustCycleSetpointSearch is planner.RobustCycleSetpointSearch
    assert list(inspect.signature(planner.RobustCycleSetpointSearch.__init__).parameters) == [
        "self", "env", "K", "n_scen", "n_cycles", "iters", "elite_frac", "seed", "risk"]
    assert inspect.signature(planner.RobustCycleSetpointSearch.__init__).parameters["risk"].default == "mean"
    with pytest.raises(ValueError):
        planner.RobustCycleSetpointSearch(None, 4, 2, risk="median")
    # the output sizer's present callers pass neither of the new keywords
    sizer = inspect.signature(gym_sbr2_amd.SbrOSVec._fanout_outputs).parameters
    assert sizer["n_scen"].default is None and sizer["return_stats"].default is False


class _StandIn:
    """A CPU stand-in for SbrEnv2Vec.  Future s of every env holds a target in entry 1 - 0.1, 0.1, 0.1, 0.5 - and the return of a
    branch is -|a - target|^2 summed over the tape: the mean over s is best at a = 0.2, the minimum over s at a = 0.3.  Env 1 flags
    branch s = 0 of every candidate whose first set-point exceeds 0.4 in any cycle: the all-0.5 start included."""
    num_envs, action_dtype = 2, None
    targets = (0.1, 0.1, 0.1, 0.5)

    def __init__(self, torch):
        self.torch, self.device, self.action_dtype, self.first_draws = torch, torch.device("cpu"), torch.float32, []

    def influent_futures(self, n_cycles, n_scen, seed=0, scenario=None, first_draw=0, current_first=True):
        self.first_draws.append(first_draw)
        out = self.torch.zeros((n_cycles, self.num_envs, n_scen, 14), dtype=self.torch.float64)
        out[..., 1] = self.torch.tensor(self.targets, dtype=self.torch.float64)
        return out

    def cycle_lookahead_scenarios(self, cand, influent, return_stats=False, return_status=False):
        torch = self.torch
        a = cand.to(self.action_dtype).double()                                     # [C, N, K, 3]
        ret = -((a[:, :, :, None, :] - influent[:, :, None, :, 1:2]) ** 2).sum(dim=(0, 4))      # [N, K, S]
        st = torch.zeros(ret.shape, dtype=torch.uint8)
        st[1, :, 0] = torch.where((a[..., 0] > 0.4).any(0)[1], _capi.ST_NEAR_POLE, 0).to(torch.uint8)
        return ret, ret.mean(dim=2), ret.min(dim=2).values, st


def test_robust_setpoint_search_on_a_stand_in_env():
    torch = pytest.importorskip("torch")
    from gym_sbr2_amd.planner import RobustCycleSetpointSearch
    plans = {}
    for risk in ("mean", "worst"):
        env = _StandIn(torch)
        search = RobustCycleSetpointSearch(env, K=64, n_scen=4, n_cycles=2, iters=6, elite_frac=0.25, seed=3, risk=risk)
        action, value = search.plan()
        ret, mean, worst, st = env.cycle_lookahead_scenarios(search.tape[:, :, None, :], search.futures)
        score = mean if risk == "mean" else worst
        assert torch.equal(value, score[:, 0]) and torch.equal(action, search.tape[0].float())
        assert torch.equal(search.status, st[:, 0].amax(dim=-1))                    # one bit in play: the OR is the maximum
        half = env.cycle_lookahead_scenarios(torch.full((2, 2, 1, 3), 0.5, dtype=torch.float64), search.futures)
        assert value[0] > half[1 if risk == "mean" else 2][0, 0]                    # it moved away from the all-0.5 start ...
        # ... and a candidate with one flagged branch of four never wins where a clean one exists: env 1 ends at or below 0.4
        assert int(search.status[1]) == 0 and bool((search.tape[:, 1, 0] <= 0.4).all())
        plans[risk] = (mean[0, 0], worst[0, 0], search.tape[:, 0])
        search.plan()
        assert env.first_draws == [1, 1 + 2 * 4]                                    # 1 + plans so far * n_cycles * n_scen
    # each risk optimises its own score - its tape beats the other's under it - and every set-point ended closer to its optimum
    # (0.2 under the mean, 0.3 under the minimum over s) than the all-0.5 start was: by less than 0.3 and 0.2
    assert plans["mean"][0] > plans["worst"][0] and plans["worst"][1] > plans["mean"][1], plans
    assert float((plans["mean"][2] - 0.2).abs().max()) < 0.3 and float((plans["worst"][2] - 0.3).abs().max()) < 0.2, plans


def test_the_kernels_have_a_unit_of_their_own():
    # the six lookahead builds, the mean / worst kernel, nothing else
    assert_unit_of_its_own(UNIT, K_SCEN.values(), others=(K_STATS,))
    assert any(n.startswith("_Z15k_draw_influent") for n in kernel_names(unit_asms()["sbr_core.hip"]))      # beside the resets


@pytest.fixture(scope="module")
def asm():
    return library_asm()


@pytest.mark.parametrize("build", ALL, ids=ALL_IDS)
def test_no_more_scratch_than_k_cycle(asm, build):
    """The yardstick is k_cycle's build of the same scheme and waves in the SAME compile (0, 92 B and 0 there today).  The register
    count is printed and not asserted: in a one-wave build anything up to 512 costs no occupancy, and the two-waves builds are
    capped by their launch bounds (and the scheme-1 one by its own attribute).  Measured (this compile, either tape): scheme 1 one
    wave 270 registers, no scratch; scheme 1 two waves 254 registers and 64 B; scheme 0 two waves 220 registers, no scratch."""
    scen, cyc = K_SCEN[build], K_CYCLE[build[1:]]
    figures = {k: (meta(asm, scen, k), meta(asm, cyc, k)) for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size")}
    print("[info] k_cycle_lookahead_scenarios against k_cycle, %s tape, scheme %d, %d wave(s): %s" % (build + (figures,)))
    assert figures["private_segment_fixed_size"][0] <= figures["private_segment_fixed_size"][1], figures


@pytest.mark.parametrize("build", ALL, ids=ALL_IDS)
def test_stores_no_more_than_the_outputs_need(asm, build):
    """returns 1, one rewards_out entry 1, the end rows 3 + 12 values, the status byte 1: 18 stores if none of them merge
    (measured: 11).  Nothing of the handle's rows is among them: k_cycle, which stores the plant, has 25."""
    stores = vector_stores(asm, K_SCEN[build])
    assert len(stores) <= 1 + 1 + 3 + 12 + 1, stores
    assert len(stores) < len(vector_stores(asm, K_CYCLE[build[1:]]))
