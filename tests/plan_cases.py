"""The case table of tests/test_plan_branches_cpu.py and tests/test_plan_branches_gpu.py: plant and controller states that put
ONE call of cfg.scheme = 1 on every branch of its step-count rule (sbr_b5a in gym_sbr2_amd/csrc/sbr_device.h, b5a_macro in
oracle/sbr_oracle.c, b5a_plan in oracle/sbr_ref.py), in the dosing and in the plain form.  A plain module like tests/isa.py and
tests/gpu_common.py: pytest does not rewrite its asserts, so each carries its message.

A case starts from a reaction interval of the golden episode const_2_5 - the first aerobic one, or an anoxic one in which the
carbon controller is in force - and changes what SPEC says: the two biomasses scaled together, So / Ss / Sno / Snh set, and the
Kla and EC the two PIDs are to deliver.  The controllers get there through their own arithmetic: the memories So[-1] = So[-2] and
Sno[-1] = Sno[-2] are the plant's, the integrators are zero, and
  * a Kla (EC) strictly inside its range is C_KLA_LAST (C_EC_LAST) with the set-point on the memory (error 0: the velocity
    form returns its bias);
  * Kla_max is set-point 8 above a bias of 200 (the upper clamp and its anti-windup), Kla = 0 the set-point 0 above a bias of 0
    (the lower clamp wherever So > 0);
  * EC_max is set-point 0 under the nitrate in the tank (upper clamp), EC = 0 the set-point 15 above it (lower clamp).
An aerobic interval never doses and an anoxic one never aerates (gym_SBR_oneshot.py:1877-2051), so the DOSING form of a plan is an
anoxic case with EC > 0 - and, on the device, every lane that shares a wavefront with one.
"""
import os

import numpy as np

from oracle import sbr_oracle as O
from oracle import sbr_params as P
from oracle import sbr_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sbros_const_2_5.npz")
NCTRL = O.C_KLA_SUM + 2                 # SBR_NCTRL; the last row is SBR_C_PLAN
EPS = 2.0 ** -50                        # condition (a): relative perturbation of the start state
COND_A, COND_B = 1e-9, 1e-6             # (a) in units of the parity gate; (b) relative distance from a threshold
PERTURBED = (2, 5, 6, 8, 9, 10)         # Ss, Xbh, Xba, So, Sno, Snh
ANOXIC_IV = 0                           # the first anoxic interval of the episode: the carbon controller doses at EC_max
KLA_BIAS = 200.0
# state-compared cases that do NOT qualify for the done call (Table.at_last_call), and why
DONE_DROPPED = {"z1-aer-kla200": "Snh = 0.3 is nitrified to -0.44 within the idle phase: the end state is outside the model's domain"}

# (name, class, base, biomass scale, overrides {state index: value}, Kla, EC, plan, compare the state?)
# class: "z" the count comes from z_ub (1, 2) or is the knee's floor (4); "s" from the n_s floor alone; "slaved"; "knee" n > 4;
# "guard" a Monod factor outside [0, 1]; "cap" the overflowing cap of 64
SPEC = []


def _spec(name, cls, base, scale, over, kla, ec, plan, compare=True):
    SPEC.append((name, cls, base, float(scale), dict(over), float(kla), float(ec), int(plan), bool(compare)))


_golden = {}


def base_state(base):
    """(x[14], t) at the start of the golden interval a case is derived from."""
    if not _golden:
        e = np.load(GOLDEN)
        i1 = int(np.where(e["iv_kind"] == 1)[0][0])
        assert e["iv_kind"][ANOXIC_IV] == 0, "the anoxic base interval moved"
        _golden["aerobic"] = (e["iv_x_start"][i1].copy(), float(e["iv_t_start"][i1]))
        _golden["anoxic"] = (e["iv_x_start"][ANOXIC_IV].copy(), float(e["iv_t_start"][ANOXIC_IV]))
        _golden["last"] = (e["iv_x_start"][-1].copy(), float(e["iv_t_start"][-1]), int(e["n_calls"]))
    x, t = _golden[base][:2]
    return x.copy(), t


def last_call():
    """(t, calls before it) of the episode's last control interval: a call injected there is the done call."""
    base_state("aerobic")
    return _golden["last"][1], _golden["last"][2] - 1


def make_case(base, scale, over, kla, ec):
    """x[14], ctrl[NCTRL], action[2] (float64) of one case."""
    x, t = base_state(base)
    x[5] *= scale; x[6] *= scale
    for i, v in over.items():
        x[int(i)] = v
    ctrl = np.zeros(NCTRL)
    ctrl[O.C_T] = t
    ctrl[O.C_SO_M1] = ctrl[O.C_SO_M2] = x[8]
    ctrl[O.C_SNO_M1] = ctrl[O.C_SNO_M2] = x[9]
    ctrl[O.C_STEPS] = 100.0
    a_do, a_ec = 2.0, 5.0
    if base == "aerobic":
        assert ec == 0.0, "an aerobic interval does not dose"
        if kla == P.KLA_MAX and x[8] <= 7.0:
            a_do, bias = P.ACT_DO_MAX, KLA_BIAS
        elif kla == 0.0:
            a_do, bias = 0.0, 0.0
        else:
            a_do, bias = x[8], kla
        assert 0.0 <= a_do <= P.ACT_DO_MAX, "So outside the action box"
        ctrl[O.C_KLA_HIST0:O.C_KLA_LAST + 1] = bias
    else:
        assert kla == 0.0, "an anoxic interval does not aerate"
        if ec == P.EC_MAX:
            a_ec = 0.0
        elif ec == 0.0:
            a_ec = P.ACT_EC_MAX
        else:
            a_ec = x[9]
            ctrl[O.C_EC_LAST] = ec
        assert 0.0 < x[9] < P.ACT_EC_MAX, "Sno outside the action box"
    return x, ctrl, np.array([a_do, a_ec])


def decisions(x, k1, span, kla):
    """Every decision variable of the plan with the arithmetic of oracle/sbr_ref.py::b5a_plan, and the counts they lead to."""
    ss, xbh, xba, so, sno, snh = x[2], x[5], x[6], x[8], x[9], x[10]
    p2 = ss + k1[2] * span
    ss_hi = p2 if p2 > ss else ss
    p10 = snh + k1[10] * span
    snh_hi = p10 if p10 > snh else snh
    c1 = ((1 - P.YH) / P.YH) * P.MUH * xbh
    c3 = ((4.57 - P.YA) / P.YA) * P.MUA * xba
    m1s, m3s = ss / (P.KS + ss), snh / (P.KNH + snh)
    m1, m3 = ss_hi / (P.KS + ss_hi), snh_hi / (P.KNH + snh_hi)
    a1, a3 = c1 * m1, c3 * m3

    def lam(s):
        return a1 * P.KOH / ((P.KOH + s) * (P.KOH + s)) + a3 * P.KOA / ((P.KOA + s) * (P.KOA + s)) + kla
    sat_span = kla * P.SO_SAT * span
    slaved = (abs(so) < R.B5A_SO_SLAVED) and (sat_span < R.B5A_SO_SLAVED)
    slope_hi = k1[8] - c1 * (m1 - m1s) * (so / (P.KOH + so)) - c3 * (m3 - m3s) * (so / (P.KOA + so))
    slope = slope_hi if slope_hi < k1[8] else k1[8]
    proj = so + slope * span
    lo1 = proj if proj < so else so
    so_lo = lo1 if lo1 > 0.0 else 0.0
    z_ub = lam(so_lo) * span
    q = lam(0.0) * span / R.B5A_Z_STAB
    in_domain = abs(m1 - 0.5) <= 0.5 and abs(m3 - 0.5) <= 0.5
    knee = (not slaved) and not (z_ub < R.B5A_Z2)
    if slaved:
        n_z = 2
    elif z_ub < R.B5A_Z1:
        n_z = 1
    elif z_ub < R.B5A_Z2:
        n_z = 2
    else:
        n_z = 4 if (q < 4.0 or not in_domain) else (R.B5A_N_MAX if not (q < float(R.B5A_N_MAX)) else int(q) + 1)
    zs = max(abs(k1[2]) * span / (P.KS + abs(ss)), abs(k1[10]) * span / (P.KNH + abs(snh)), abs(k1[9]) * span / (P.KNO + abs(sno)))
    n_s = 1 if zs < R.B5A_ZS1 else (2 if zs < R.B5A_ZS2 else 4)
    return dict(z_ub=z_ub, q=q, zs=zs, so=so, sat_span=sat_span, m1=m1, m3=m3, slaved=slaved, knee=knee, in_domain=in_domain,
                n_z=n_z, n_s=n_s, n=max(n_z, n_s), plan=max(n_z, n_s) + (128 if slaved else 0))


def threshold_margin(d):
    """Condition (b): the smallest relative distance of a decision variable from a threshold it is compared with (absolute
    where the threshold is 0), and the variable's name.  q counts only where the knee's count is read from it."""
    def rel(v, t):
        return abs(v - t) / t if t != 0 else abs(v)
    m = [(rel(d["z_ub"], R.B5A_Z1), "z_ub/0.3"), (rel(d["z_ub"], R.B5A_Z2), "z_ub/1.0"),
         (rel(d["zs"], R.B5A_ZS1), "zs/0.15"), (rel(d["zs"], R.B5A_ZS2), "zs/0.5"),
         (rel(abs(d["so"]), R.B5A_SO_SLAVED), "|So|/1e-9"), (rel(d["sat_span"], R.B5A_SO_SLAVED), "kla So_sat span/1e-9"),
         (rel(d["m1"], 0.0), "m1/0"), (rel(d["m1"], 1.0), "m1/1"), (rel(d["m3"], 0.0), "m3/0"), (rel(d["m3"], 1.0), "m3/1")]
    if d["knee"]:
        q = d["q"]
        m.append((rel(q, 4.0), "q/4"))
        m.append((rel(q, 64.0), "q/64"))
        if 4.0 <= q < 64.0:
            m.append((min(q - np.floor(q), np.floor(q) + 1.0 - q) / q, "q/integer"))
    return min(m)


def interval_decisions(x, span, kla, ec):
    """decisions() of one reaction interval from its start state, with the first stage slope of the form the oracle integrates."""
    x = np.asarray(x, dtype=np.float64)
    k1 = R.rhs_reaction_w(x, x[0], kla, ec) if ec != 0 else R.rhs_reaction(x, 0.0, kla, ec)
    return decisions(x, k1, span, kla)


def oracle_call(x, ctrl, action, reward_kind=0):
    """load_state + one step of the C oracle for cases stacked along axis 0: the OracleBatch afterwards, and what step returned."""
    x, ctrl, action = np.atleast_2d(x), np.atleast_2d(ctrl), np.atleast_2d(action)
    p = O.default_params()
    p.reward_kind = reward_kind
    ora = O.OracleBatch(len(x), params=p)
    ora.load_state(x.T, ctrl.T)
    out = ora.step(action)
    return ora, out


def gate(x, ref):
    """The parity gate (tests/conftest.py)."""
    x, ref = np.asarray(x), np.asarray(ref)
    return np.abs(x - ref) / (P.RTOL_GATE * np.abs(ref) + P.RTOL_GATE * P.STATE_SCALE)


def conditioning(x, ctrl, action):
    """Condition (a) for stacked cases: the largest movement of the oracle's end state, in gates, when Ss, Xbh, Xba, So, Sno and
    Snh of the start state move by a relative 2^-50, either way.  The controller rows are inputs both sides read bit for bit, and
    stay."""
    x, ctrl = np.atleast_2d(x), np.atleast_2d(ctrl)
    ref = oracle_call(x, ctrl, action)[0].envs["x"].copy()
    worst = np.zeros(len(x))
    for sign in (1.0, -1.0):
        f = 1.0 + sign * EPS
        x2 = x.copy()
        x2[:, PERTURBED] *= f
        worst = np.maximum(worst, gate(oracle_call(x2, ctrl, action)[0].envs["x"], ref).max(axis=1))
    return worst


class Table:
    """The cases stacked: names, cls, plan, compare, dose [n]; x [n, 14], ctrl [n, NCTRL], action [n, 2]; kla, ec [n] as wanted."""

    def __init__(self, spec):
        self.names = [s[0] for s in spec]
        assert len(set(self.names)) == len(self.names), "case names must be unique"
        self.cls = np.array([s[1] for s in spec])
        self.base = np.array([s[2] for s in spec])
        built = [make_case(s[2], s[3], s[4], s[5], s[6]) for s in spec]
        self.x = np.array([b[0] for b in built])
        self.ctrl = np.array([b[1] for b in built])
        self.action = np.array([b[2] for b in built])
        self.kla = np.array([s[5] for s in spec])
        self.ec = np.array([s[6] for s in spec])
        self.plan = np.array([s[7] for s in spec], dtype=np.int64)
        self.compare = np.array([s[8] for s in spec], dtype=bool)
        self.dose = self.ec != 0.0
        self.n = len(spec)

    def at_last_call(self):
        """The state-compared cases (but DONE_DROPPED) with C_T and C_STEPS of the episode's last control interval (aerobic: Kla
        from the case's DO set-point, no dosing): x, ctrl, action, names."""
        t, steps = last_call()
        keep = np.array([i for i in np.nonzero(self.compare)[0] if self.names[i] not in DONE_DROPPED])
        ctrl = self.ctrl[keep].copy()
        ctrl[:, O.C_T] = t
        ctrl[:, O.C_STEPS] = steps
        return self.x[keep].copy(), ctrl, self.action[keep].copy(), [self.names[i] for i in keep]


def trace_call(x, ctrl, action):
    """One call of the NumPy oracle (oracle/sbr_ref.py, RK4 mode, scheme 1) from an injected state, recording the decisions of
    every macro interval it plans - the reaction interval(s) and, on the done call, the macro intervals of the idle phase.
    Returns (list of decisions, end state, done)."""
    env = R.SbrOsRef(integrator="rk4", scheme=1)
    env.x, env.t = np.array(x, dtype=np.float64), float(ctrl[O.C_T])
    env.so_m1, env.so_m2, env.sno_m1, env.sno_m2 = (float(ctrl[r]) for r in (O.C_SO_M1, O.C_SO_M2, O.C_SNO_M1, O.C_SNO_M2))
    env.ie_do, env.ie_ec = float(ctrl[O.C_IE_DO]), float(ctrl[O.C_IE_EC])
    env.kla_hist = [float(v) for v in ctrl[O.C_KLA_HIST0:O.C_KLA_LAST + 1]]
    env.kla_last, env.ec_last, env.ec_prev = float(ctrl[O.C_KLA_LAST]), float(ctrl[O.C_EC_LAST]), float(ctrl[O.C_EC_LAST])
    env.u_do, env.u_ec, env.done = 0.0, 0.0, False
    seen, plan = [], R.b5a_plan

    def recording(xs, k1, span, kla):
        seen.append(decisions(xs, k1, span, kla))
        return plan(xs, k1, span, kla)
    R.b5a_plan = recording
    try:
        done = env.step(action)[3]
    finally:
        R.b5a_plan = plan
    return seen, (env.x_after_idle if done else env.x), done


# ----------------------------------------------------------------------------------------------------------------------
# The table.  Chosen by a grid search on the CPU oracle (biomass x 0.1 .. 40, So, Ss, Sno, Snh, Kla, EC); a case that failed
# condition (a) or (b) was replaced, not masked (tests/test_plan_branches_cpu.py holds every entry to both).
_spec('z1-aer-kla200', 'z', 'aerobic', 0.1, {8: 0, 2: 0.5, 10: 0.3}, 200, 0, 1)
_spec('z1-aer-off', 'z', 'aerobic', 0.1, {8: 0.05, 2: 0.5}, 0, 0, 1)
_spec('z1-anox-plain', 'z', 'anoxic', 0.1, {8: 0.5}, 0, 0, 1)
_spec('z1-anox-dose', 'z', 'anoxic', 0.1, {8: 0.5}, 0, 0.0005, 1)
_spec('z1-anox-dose-1e-4', 'z', 'anoxic', 0.1, {8: 0.5, 2: 40}, 0, 0.0001, 1)
_spec('z2-aer-kla200', 'z', 'aerobic', 0.1, {8: 0}, 200, 0, 2)
_spec('z2-aer-kla240', 'z', 'aerobic', 0.1, {8: 1e-10, 2: 0.5}, 240, 0, 2)
_spec('z2-anox-plain', 'z', 'anoxic', 0.1, {8: 0.05}, 0, 0, 2)
_spec('z2-anox-dose', 'z', 'anoxic', 0.1, {8: 0.05}, 0, 0.0005, 2)
_spec('z2-anox-dose-1e-4', 'z', 'anoxic', 0.1, {8: 0.05, 2: 40, 9: 5}, 0, 0.0001, 2)
_spec('z4-aer-kla200', 'z', 'aerobic', 0.1, {8: 0, 2: 40}, 200, 0, 4)
_spec('z4-aer-golden', 'z', 'aerobic', 1, {}, 200, 0, 4)
_spec('z2-aer-so0.5-kla240', 'z', 'aerobic', 1, {8: 0.5}, 240, 0, 2)
_spec('z4-anox-plain', 'z', 'anoxic', 0.3, {8: 0.05}, 0, 0, 4)
_spec('z4-anox-dose', 'z', 'anoxic', 0.3, {8: 0.05}, 0, 0.0005, 4)
_spec('z4-anox-dose-1e-4', 'z', 'anoxic', 0.3, {8: 0.05, 2: 40, 9: 0.2}, 0, 0.0001, 4)
_spec('s2-aer-off', 's', 'aerobic', 1, {8: 2}, 0, 0, 2)
_spec('s2-aer-kla240', 's', 'aerobic', 1, {8: 2, 2: 0.5}, 240, 0, 2)
_spec('s2-anox-plain', 's', 'anoxic', 1, {8: 6, 9: 0.2}, 0, 0, 2)
_spec('s2-anox-dose', 's', 'anoxic', 0.1, {8: 0.5, 2: 0.5}, 0, 0.0005, 2)
_spec('s2-anox-dose-b', 's', 'anoxic', 0.1, {8: 0.05, 2: 0.5, 9: 5}, 0, 0.0005, 2)
_spec('s4-aer-off', 's', 'aerobic', 3, {8: 6}, 0, 0, 4)
_spec('s4-aer-kla200', 's', 'aerobic', 3, {8: 2, 2: 0.5}, 200, 0, 4)
_spec('s4-anox-plain', 's', 'anoxic', 3, {8: 6, 9: 0.2}, 0, 0, 4)
_spec('s4-anox-dose', 's', 'anoxic', 3, {8: 6, 9: 0.2}, 0, 0.0005, 4)
_spec('s4-anox-dose-1e-4', 's', 'anoxic', 5, {8: 6, 2: 0.5, 9: 0.2}, 0, 0.0001, 4)
_spec('130-aer-off', 'slaved', 'aerobic', 0.1, {8: 0}, 0, 0, 130)
_spec('130-aer-off-1e-10', 'slaved', 'aerobic', 1, {8: 1e-10}, 0, 0, 130)
_spec('130-anox-plain', 'slaved', 'anoxic', 1, {8: -7.6552e-14}, 0, 0, 130)
_spec('130-anox-dose', 'slaved', 'anoxic', 1, {}, 0, 0.0005, 130)
_spec('130-anox-dose-1e-4', 'slaved', 'anoxic', 0.3, {8: 1e-10, 9: 5}, 0, 0.0001, 130)
_spec('130-anox-dose-big', 'slaved', 'anoxic', 8, {8: 0, 2: 0.5}, 0, 0.0005, 130)
_spec('132-anox-plain', 'slaved', 'anoxic', 3, {8: -7.6552e-14, 2: 40}, 0, 0, 132)
_spec('132-anox-plain-b', 'slaved', 'anoxic', 3, {8: 1e-10, 2: 40, 9: 0.2}, 0, 0, 132)
_spec('132-anox-dose', 'slaved', 'anoxic', 3, {8: 0, 2: 40}, 0, 0.0005, 132)
_spec('132-anox-dose-1e-4', 'slaved', 'anoxic', 3, {8: -7.6552e-14, 2: 40, 9: 0.2}, 0, 0.0001, 132)
_spec('132-anox-dose-big', 'slaved', 'anoxic', 8, {8: 1e-10, 2: 40}, 0, 0.0005, 132)
_spec('knee5-aer', 'knee', 'aerobic', 2.1979, {8: 0}, 200, 0, 5)
_spec('knee6-aer', 'knee', 'aerobic', 2.687, {8: 0.05}, 240, 0, 6)
_spec('knee7-aer', 'knee', 'aerobic', 3.1828, {8: 0}, 240, 0, 7)
_spec('knee9-aer', 'knee', 'aerobic', 4.1809, {8: 1e-10}, 200, 0, 9)
_spec('knee11-aer', 'knee', 'aerobic', 5.2055, {8: 0.05}, 0.0, 0, 11)
_spec('knee13-aer', 'knee', 'aerobic', 6.1574, {8: 0.5}, 240, 0, 13)
_spec('knee17-aer', 'knee', 'aerobic', 8.1468, {8: 0}, 200, 0, 17)
_spec('knee25-aer', 'knee', 'aerobic', 12.113, {8: 0.05}, 200, 0, 25)
_spec('knee32-aer', 'knee', 'aerobic', 15.576, {8: 0}, 240, 0, 32)
_spec('knee33-aer', 'knee', 'aerobic', 16.079, {8: 0.5}, 200, 0, 33)
_spec('knee41-aer', 'knee', 'aerobic', 20.044, {8: 0}, 200, 0, 41)
_spec('knee47-aer', 'knee', 'aerobic', 23.013, {8: 2}, 240, 0, 47)
_spec('knee55-aer', 'knee', 'aerobic', 26.976, {8: 0}, 240, 0, 55)
_spec('knee63-aer', 'knee', 'aerobic', 30.948, {8: 0}, 200, 0, 63)
_spec('knee64-aer', 'knee', 'aerobic', 31.444, {8: 0}, 200, 0, 64)
_spec('knee5-anox-dose', 'knee', 'anoxic', 1.7158, {8: 0.05}, 0, 0.0005, 5)
_spec('knee7-anox-dose', 'knee', 'anoxic', 2.4785, {8: 0.5}, 0, 0.0005, 7)
_spec('knee11-anox-dose', 'knee', 'anoxic', 4.0034, {8: 0.05}, 0, 0.0001, 11)
_spec('knee17-anox-dose', 'knee', 'anoxic', 6.2915, {8: 0.5}, 0, 0.0005, 17)
_spec('knee25-anox-dose', 'knee', 'anoxic', 9.3404, {8: 0.05}, 0, 0.0005, 25)
_spec('knee32-anox-dose', 'knee', 'anoxic', 12.011, {8: 0.5}, 0, 0.0001, 32)
_spec('knee41-anox-dose', 'knee', 'anoxic', 15.439, {8: 0.05}, 0, 0.0005, 41)
_spec('knee63-anox-dose', 'knee', 'anoxic', 23.822, {8: 0.05}, 0, 0.0005, 63)
_spec('knee64-anox-dose', 'knee', 'anoxic', 24.203, {8: 0.05}, 0, 0.0005, 64)
_spec('knee7-anox-plain', 'knee', 'anoxic', 2.4784, {8: 0.05}, 0, 0, 7)
_spec('knee41-anox-plain', 'knee', 'anoxic', 15.443, {8: 0.5}, 0, 0, 41)
_spec('knee63-anox-plain', 'knee', 'anoxic', 23.822, {8: 0.05}, 0, 0, 63)
_spec('guard-m1-aer', 'guard', 'aerobic', 3, {8: 0, 2: -10.5}, 200, 0, 4, compare=False)
_spec('guard-m3-aer', 'guard', 'aerobic', 3, {8: 0, 10: -1.2}, 200, 0, 4, compare=False)
_spec('guard-nan-aer', 'guard', 'aerobic', 3, {8: 0, 10: float("nan")}, 200, 0, 4, compare=False)
_spec('guard-m1-anox-dose', 'guard', 'anoxic', 3, {8: 0.05, 2: -10.5}, 0, 0.0005, 4, compare=False)
_spec('guard-m3-anox-dose', 'guard', 'anoxic', 3, {8: 0.05, 10: -1.2}, 0, 0.0005, 4, compare=False)
_spec('guard-m3-anox-plain', 'guard', 'anoxic', 3, {8: 0.05, 10: -1.2}, 0, 0, 4, compare=False)
_spec('cap64-aer-x45', 'cap', 'aerobic', 45, {8: 0}, 200, 0, 64, compare=False)
_spec('cap64-aer-x1e6', 'cap', 'aerobic', 1000000.0, {8: 0}, 200, 0, 64, compare=False)
_spec('cap64-anox-dose-x45', 'cap', 'anoxic', 45, {8: 0.05}, 0, 0.0005, 64, compare=False)

_table = []


def table():
    """The table, built once per process."""
    if not _table:
        _table.append(Table(SPEC))
    return _table[0]
