"""The case table of tests/plan_cases.py, held to its own rules on the CPU oracle: which branches of scheme 1's step-count rule
it reaches (the census), that every state-compared case is well conditioned (a) and far from every threshold of the rule (b),
and that the NumPy restatement of the integrator equals the C oracle bit for bit on every case.  No GPU."""
import numpy as np
import plan_cases as PC
import pytest

from oracle import sbr_oracle as O
from oracle import sbr_ref as R


@pytest.fixture(scope="module")
def T():
    return PC.table()


@pytest.fixture(scope="module")
def run(T):
    """The oracle's call on every case, and the decisions of its interval under the Kla and EC the controllers delivered."""
    ora, out = PC.oracle_call(T.x, T.ctrl, T.action)
    dec = [PC.interval_decisions(T.x[i], ora.envs["span"][i], ora.envs["kla_last"][i], ora.envs["ec_last"][i]) for i in range(T.n)]
    return ora, out, dec


def test_controllers_deliver_the_kla_and_ec_of_the_table_and_the_oracle_runs_the_listed_plan(T, run):
    ora, out, dec = run
    assert 60 <= T.n <= 100
    assert np.array_equal(ora.envs["kla_last"], T.kla) and np.array_equal(ora.envs["ec_last"], T.ec)
    assert np.array_equal(ora.envs["scheme_plan"] & 0xff, T.plan) and np.array_equal(ora.envs["n_intervals"], np.ones(T.n, np.int32))
    assert not out[3].any()
    for i in range(T.n):
        if np.isfinite(T.x[i]).all():
            assert dec[i]["plan"] == T.plan[i], (T.names[i], dec[i])
    # what is compared by state ends finite and inside the model's domain; the cap's case overflows
    xe = ora.envs["x"]
    assert np.isfinite(xe[T.compare]).all() and (xe[T.compare] >= -1e-9).all()
    assert np.all(ora.envs["status"][T.compare] == 0)
    assert not np.isfinite(xe[T.names.index("cap64-aer-x1e6")]).all()


def test_census_of_plan_classes_in_both_forms(T, run):
    dec = run[2]
    got = set()
    for i in range(T.n):
        d, dose, cmp_ = dec[i], bool(T.dose[i]), bool(T.compare[i])
        if not np.isfinite(T.x[i]).all():
            cls = "guard-nan"
        elif d["slaved"]:
            cls = "slaved"
        elif d["knee"] and not d["in_domain"]:
            cls = "guard-m1" if not abs(d["m1"] - 0.5) <= 0.5 else "guard-m3"
            assert d["q"] >= 5.0 and not cmp_, T.names[i]                  # without the guard the count would not be 4
        elif d["knee"] and not d["q"] < 64.0:
            cls = "cap"
            assert not cmp_, T.names[i]
        elif d["n_s"] > d["n_z"]:
            cls = "s"
        elif d["knee"] and d["n_z"] > 4:
            cls = "knee"
        else:
            cls = "z"
        assert cls.split("-")[0] == T.cls[i], (T.names[i], cls)
        got.add((cls, int(T.plan[i]), dose, cmp_))
    for dose in (False, True):
        for plan in (1, 2, 4):
            assert ("z", plan, dose, True) in got, (plan, dose)
        for plan in (2, 4):
            assert ("s", plan, dose, True) in got, (plan, dose)
        for plan in (130, 132):
            assert ("slaved", plan, dose, True) in got, (plan, dose)
        knee = sorted(p for c, p, ds, cm in got if c == "knee" and ds == dose and cm)
        inner = [p for p in knee if 5 <= p <= 63]
        assert len(inner) >= 6 and any(p % 2 for p in inner) and any(p >= 32 for p in inner), (dose, knee)
        assert inner[0] <= 7 and inner[-1] == 63 and 64 in knee, (dose, knee)     # spread over the range; 64 from q in [63, 64)
        assert ("guard-m3", 4, dose, False) in got and ("guard-m1", 4, dose, False) in got, dose
    assert ("guard-nan", 4, False, False) in got
    assert ("cap", 64, False, False) in got and ("cap", 64, True, False) in got
    # the wavefront the GPU file interleaves
    for plan in (1, 2, 4, 7, 41, 63, 130, 132):
        assert plan in T.plan[T.compare & T.dose] and plan in T.plan[T.compare & ~T.dose], plan
    for i in np.nonzero((T.cls == "knee") & (T.plan == 64))[0]:
        assert 63.0 <= dec[i]["q"] < 64.0, T.names[i]


def test_condition_a_conditioning_and_condition_b_distance_from_thresholds(T, run):
    dec = run[2]
    cond = PC.conditioning(T.x[T.compare], T.ctrl[T.compare], T.action[T.compare])
    print("condition (a): worst %.2e gate (%s)" % (cond.max(), np.array(T.names)[T.compare][cond.argmax()]))
    assert cond.max() <= PC.COND_A, np.array(T.names)[T.compare][cond > PC.COND_A]
    worst = min((PC.threshold_margin(dec[i]) + (T.names[i],) for i in np.nonzero(T.compare)[0]))
    print("condition (b): nearest threshold %.2e relative (%s, %s)" % worst)
    assert worst[0] >= PC.COND_B, worst


def test_numpy_restatement_equals_the_c_oracle_on_every_case(T, run):
    ora = run[0]
    for i in range(T.n):
        span, kla, ec = float(ora.envs["span"][i]), float(ora.envs["kla_last"][i]), float(ora.envs["ec_last"][i])
        x_c, n_c = O.reaction_interval(T.x[i], span, kla, ec)
        with np.errstate(all="ignore"):               # the NaN guard case and the overflowing cap
            x_py, n_py = R.b5a_macro(0, T.x[i], span, kla, ec)
        assert n_c == n_py == (T.plan[i] & 127), T.names[i]
        assert np.array_equal(x_c, x_py, equal_nan=True), T.names[i]
        assert np.array_equal(x_c, ora.envs["x"][i], equal_nan=True), T.names[i]      # and it is what the call ran


def test_done_call_cases_pass_both_conditions_through_the_idle_phase(T):
    """The cases the GPU file injects at the episode's last interval: the call runs that interval, settle and draw, and the idle
    phase as ceil(rows / 10) macro intervals.  (a) and (b) for every macro interval of it; the NumPy oracle, whose plans are
    recorded, ends on the C oracle's bits.  DONE_DROPPED lists what does not qualify - and indeed does not."""
    x, ctrl, action, names = T.at_last_call()
    assert len(names) == int(T.compare.sum()) - len(PC.DONE_DROPPED) and set(PC.DONE_DROPPED) <= set(T.names)
    ora, out = PC.oracle_call(x, ctrl, action)
    xe = ora.envs["x"]
    assert out[3].all() and np.isfinite(ora.envs["qw"]).all() and np.isfinite(xe).all() and (xe >= -1e-9).all()
    cond = PC.conditioning(x, ctrl, action)
    assert cond.max() <= PC.COND_A, np.array(names)[cond > PC.COND_A]
    counts, worst = set(), (1.0, "", "")
    for i, name in enumerate(names):
        seen, x_py, done = PC.trace_call(x[i], ctrl[i], action[i])
        assert done and len(seen) >= 40 and np.array_equal(x_py, xe[i]), name
        worst = min(worst, min(PC.threshold_margin(d) for d in seen) + (name,))
        counts |= {d["plan"] for d in seen[1:]}
    print("done call: condition (a) worst %.2e gate; (b) nearest threshold %.2e (%s, %s); idle plans %s"
          % ((cond.max(),) + worst + (sorted(counts),)))
    assert worst[0] >= PC.COND_B, worst
    assert {1, 2, 4, 130} <= counts and max(c for c in counts if c < 128) >= 20      # the general-span h = hm / n at many n
    for name in PC.DONE_DROPPED:
        i = T.names.index(name)
        c = T.ctrl[i].copy()
        c[O.C_T], c[O.C_STEPS] = PC.last_call()
        assert (PC.oracle_call(T.x[i], c, T.action[i])[0].envs["x"] < -1e-9).any(), name
