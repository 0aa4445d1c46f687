"""ctypes front-end of oracle/sbr_oracle.c (TEST INFRASTRUCTURE - CPU oracle, layer 2): the plant in fp64 under the
product's two integration schemes (scheme 1, the default: adaptive Butcher-5; scheme 0: RK4 x substeps).

Only tests/, scripts/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.  The library's C ABI is
declared once, in ABI below; lib() applies it to whichever build it loads and nothing else sets restype or argtypes.
"""
import contextlib
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libsbr_oracle.so")
NX, NOBS, NSTATE, KLA_HIST = 14, 18, 15, 10
NRND = 48             # standard normals per influent draw
NCYC_DIAG = 12        # qw, EQI, OCI, Ntot, COD, Snh, BOD5, Sno (effluent), mean Kla of phases 3, 5, 8, Xf
NKLA_LOG = (6, 256)   # sbro_cycle_step's per-interval Kla log: six PID phases, NaN-padded

# rows of the product's PUBLIC controller block that load_state reads (include/sbr_amd.h, SBR_C_*).  Written out here
# because the oracle imports nothing from the product; tests/test_capi_cpu.py holds them equal to the binding's.
C_T, C_SO_M1, C_SO_M2, C_SNO_M1, C_SNO_M2, C_IE_DO, C_IE_EC, C_EC_LAST = range(8)
C_KLA_HIST0 = 8
C_KLA_LAST = C_KLA_HIST0 + KLA_HIST - 1
C_QW, C_RETURN, C_STEPS, C_DONE, C_STATUS, C_KLA_SUM = range(C_KLA_LAST + 1, C_KLA_LAST + 7)


class Params(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "Ya Yh fp ixb ixp muH Ks Koh Kno bH eta_g eta_h kh Kx muA Knh bA Koa ka "
        "WV IV dt t_delta t_cycle T_fill T3_0 T3_end T4_end T5_end t_settle t_draw "
        "So_sat Kla_min Kla_max Kc_DO tauI_DO tauD_DO EC_min EC_max Kc_EC tauI_EC tauD_EC EC_conc "
        "act_DO_max act_EC_max biomass_setpoint Qeff settler_area settler_vmax").split()] + [
        ("t_ratio", C.c_double * 8), ("cyc_Kc", C.c_double), ("cyc_tauI", C.c_double), ("cyc_tauD", C.c_double),
        ("cyc_dt", C.c_double),
        ("x0", C.c_double * NX), ("substeps", C.c_int32), ("out_f64", C.c_int32),
        ("terminal", C.c_int32), ("reward_kind", C.c_int32), ("act_f64", C.c_int32), ("random_scenario", C.c_int32),
        ("scheme", C.c_int32), ("reserved_", C.c_int32)]


class Env(C.Structure):
    _fields_ = [("x", C.c_double * NX), ("t", C.c_double),
                ("so_m1", C.c_double), ("so_m2", C.c_double), ("sno_m1", C.c_double), ("sno_m2", C.c_double),
                ("ie_do", C.c_double), ("ie_ec", C.c_double),
                ("kla_last", C.c_double), ("ec_last", C.c_double), ("ec_prev", C.c_double),
                ("u_do", C.c_double), ("u_ec", C.c_double),
                ("kla_hist", C.c_double * KLA_HIST),
                ("qw", C.c_double), ("ret", C.c_double), ("steps", C.c_double), ("done", C.c_double),
                ("status", C.c_double), ("kla_sum", C.c_double), ("influent", C.c_double * NX), ("x_start", C.c_double * NX), ("span", C.c_double),
                ("n_rows", C.c_int32), ("n_intervals", C.c_int32), ("scheme_steps", C.c_int32), ("scheme_plan", C.c_int32)]


ENV_DTYPE = np.dtype(Env)      # OracleBatch.envs, a record array, IS the C array of sbro_env

# every non-static sbro_* function of sbr_oracle.c: name -> (restype, argtypes)
_i, _i32, _i64, _u32, _u64, _d = C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_double
_dp, _fp, _u8p, _pp, _ep = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(Params), C.POINTER(Env)
ABI = {
    "sbro_default_params": (None, [_pp]),
    "sbro_sizeof_env": (_i, []),
    "sbro_sizeof_params": (_i, []),
    "sbro_rhs_reaction": (None, [_pp, _dp, _d, _d, _dp]),
    "sbro_rhs_fill": (None, [_pp, _dp, _d, _dp, _dp]),
    "sbro_rhs_idle": (None, [_pp, _dp, _d, _dp]),
    "sbro_eval_rhs": (None, [_pp, _i, _i64, _dp, _dp, _dp, _dp, _dp]),
    "sbro_set_plan_knobs": (None, [_d]),
    "sbro_reaction_interval": (_i, [_pp, _dp, _d, _d, _d]),
    "sbro_reaction_interval_plan": (_i, [_pp, _dp, _d, _d, _d]),
    "sbro_rk4": (None, [_pp, _i, _dp, _d, _i, _d, _d, _dp]),
    "sbro_influent_mix": (None, [_dp, _dp, _dp, _dp]),
    "sbro_draw_normals": (None, [_u64, _u64, _dp]),
    "sbro_policy_action": (None, [_pp, _u64, _u64, _u32, _fp]),
    "sbro_scenario_draw": (_i32, [_u64, _u64]),
    "sbro_reset": (None, [_pp, _ep, _dp, _dp]),
    "sbro_reset_carry": (None, [_pp, _ep, _dp, _dp]),
    "sbro_reward_g2anet": (_d, [_dp]),
    "sbro_reward_oci": (_d, [_d, _d, _d, _i32, _d, _d, _d, _d]),
    "sbro_reward_parts": (None, [_pp, _ep, _dp]),
    "sbro_step": (None, [_pp, _ep, _dp, _dp, _dp, _dp, _u8p]),
    "sbro_batch_reset": (None, [_pp, _i64, _ep, _dp, _dp, _i]),
    "sbro_batch_reset_carry": (None, [_pp, _i64, _ep, _dp, _dp, _i]),
    "sbro_batch_step": (None, [_pp, _i64, _ep, _dp, _dp, _dp, _dp, _u8p, _i]),
    "sbro_batch_rollout": (None, [_pp, _i64, _ep, _i64, _i32, _u64, _dp, _i]),
    "sbro_cycle_step": (None, [_pp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "sbro_cycle_reset_state": (None, [_dp, _dp, _dp]),
    "sbro_batch_cycle_step": (None, [_pp, _i64, _dp, _dp, _dp, _dp, _dp, _dp, _i]),
}


def _src_hash():
    import hashlib
    h = hashlib.sha256()
    for name in ("sbr_oracle.c", "Makefile"):
        with open(os.path.join(_HERE, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def build(force=False):
    """Stale = the library was built from other sources (content hash next to it; mtimes do not survive a copied tree).
    Serialised by a file lock so that several processes can call this at once."""
    import fcntl
    tag = _LIB + ".srchash"

    def stale():
        return not (os.path.exists(_LIB) and os.path.exists(tag) and open(tag).read().strip() == _src_hash())
    if force or stale():
        with open(_LIB + ".lock", "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if force or stale():
                subprocess.check_call(["make", "-C", _HERE, "-s", "-B", "libsbr_oracle.so"])
                with open(tag, "w") as f:
                    f.write(_src_hash() + "\n")
    return _LIB


_lib = None
_variant = ""          # "" = strict build (no FMA contraction); "_fma" = same source with -mfma -ffp-contract=fast


def use_variant(suffix):
    """Switch to another build of the SAME source (tests/test_oracle_golden.py uses "_fma" as a control for how
    far pure rounding differences get amplified by the closed loop).  Returns the previous variant."""
    global _lib, _variant
    prev = _variant
    if suffix != _variant:
        if suffix:
            subprocess.check_call(["make", "-C", _HERE, "-s", "libsbr_oracle%s.so" % suffix])
        _lib, _variant = None, suffix
    return prev


def lib():
    global _lib
    if _lib is None:
        so = C.CDLL(build() if not _variant else os.path.join(_HERE, "libsbr_oracle%s.so" % _variant))
        for name, (res, args) in ABI.items():
            fn = getattr(so, name)
            fn.restype, fn.argtypes = res, args
        assert so.sbro_sizeof_env() == C.sizeof(Env) == ENV_DTYPE.itemsize, "oracle env layout drifted"
        assert so.sbro_sizeof_params() == C.sizeof(Params), "oracle params layout drifted"
        _lib = so
    return _lib


def default_params(scheme=None):
    """The reference's constants; scheme as the product's sbr_default_config() (1 = adaptive Butcher-5) unless given
    (0 = RK4 x substeps)."""
    p = Params()
    lib().sbro_default_params(C.byref(p))
    if scheme is not None:
        p.scheme = int(scheme)
    return p


def _p(a, t=C.c_double):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class OracleBatch:
    """N environments stepped by the C oracle (fp64, OpenMP over envs; the integrator is params.scheme: 1 = adaptive
    Butcher-5, the default, 0 = RK4 x substeps)."""

    def __init__(self, n, params=None, nthreads=1, first_env_id=0):
        self.n, self.nthreads, self.first_env_id = int(n), int(nthreads), int(first_env_id)
        self.p = params if params is not None else default_params()
        self.envs = np.zeros(self.n, dtype=ENV_DTYPE)

    def _envp(self):
        return self.envs.ctypes.data_as(C.POINTER(Env))

    def mix(self, means, stds, scenario, rnd):
        """influent_mixed [n][14] from tables[8,14,48], scenario [n], rnd [n][48]."""
        out = np.empty((self.n, NX))
        means, stds, rnd = _f64(means), _f64(stds), _f64(rnd)
        for i in range(self.n):
            s = int(scenario[i])
            lib().sbro_influent_mix(_p(means[s]), _p(stds[s]), _p(rnd[i]), _p(out[i]))
        return out

    def normals(self, seed):
        out = np.empty((self.n, NRND))
        for i in range(self.n):
            lib().sbro_draw_normals(seed, self.first_env_id + i, _p(out[i]))
        return out

    def scenarios(self, seed):
        """The scenario each env draws at a reset with cfg.random_scenario = 1 (np.random.choice(8, 1), gym_SBR_env4.py:107)."""
        return np.array([lib().sbro_scenario_draw(seed, self.first_env_id + i) for i in range(self.n)], dtype=np.int32)

    def reward_parts(self):
        """[n][4]: EQI2, OCI2, AE_OCI2, EC_OCI2 of the call just made (module_reward_EQIOCI.py:109-112)."""
        out = np.empty((self.n, 4))
        envs = self._envp()
        for i in range(self.n):
            lib().sbro_reward_parts(C.byref(self.p), C.byref(envs[i]), _p(out[i]))
        return out

    # load_state: env field <- row of the product's controller block.  The set-points in force (u_do, u_ec) have no row and
    # the EC before EC[-1] takes EC[-1]'s: they are temporaries of one call (every interval overwrites them first)
    _CTRL_ROW = {"t": C_T, "so_m1": C_SO_M1, "so_m2": C_SO_M2, "sno_m1": C_SNO_M1, "sno_m2": C_SNO_M2, "ie_do": C_IE_DO,
                 "ie_ec": C_IE_EC, "ec_last": C_EC_LAST, "ec_prev": C_EC_LAST, "kla_last": C_KLA_LAST, "qw": C_QW,
                 "ret": C_RETURN, "steps": C_STEPS, "done": C_DONE, "status": C_STATUS, "kla_sum": C_KLA_SUM}

    def load_state(self, x, ctrl):
        """Overwrite the plant/controller state from the product's PUBLIC layout: x [14][n], ctrl [24][n]
        (rows as in include/sbr_amd.h).  Used to re-synchronise the oracle to the device before a call."""
        x, ctrl = np.asarray(x, dtype=np.float64), np.asarray(ctrl, dtype=np.float64)
        e = self.envs
        e["x"] = x.T
        for name, row in self._CTRL_ROW.items():
            e[name] = ctrl[row]
        e["kla_hist"] = ctrl[C_KLA_HIST0:C_KLA_HIST0 + KLA_HIST].T

    def _reset(self, fn, influent):
        influent = _f64(np.broadcast_to(influent, (self.n, NX)))
        obs = np.empty((self.n, NOBS))
        fn(C.byref(self.p), self.n, self._envp(), _p(influent), _p(obs), self.nthreads)
        return obs

    def reset(self, influent):
        return self._reset(lib().sbro_batch_reset, influent)

    def reset_carry(self, influent):
        """New cycle from each env's own current state (x0 := x, IV := x[0])."""
        return self._reset(lib().sbro_batch_reset_carry, influent)

    def step(self, action, want_obs=True):
        # float64 actions, like the reference; to mirror the product (float32 action tensors) pass
        # actions.astype(np.float32) - the values are then used exactly
        action = _f64(np.broadcast_to(action, (self.n, 2)))
        obs = np.empty((self.n, NOBS)) if want_obs else None
        state = np.empty((self.n, NSTATE)) if want_obs else None
        reward = np.empty(self.n)
        done = np.empty(self.n, dtype=np.uint8)
        lib().sbro_batch_step(C.byref(self.p), self.n, self._envp(), _p(action), _p(obs), _p(state), _p(reward),
                              _p(done, C.c_uint8), self.nthreads)
        return obs, state, reward, done

    def rollout(self, n_steps, policy_seed):
        ret = np.empty(self.n)
        lib().sbro_batch_rollout(C.byref(self.p), self.n, self._envp(), self.first_env_id, n_steps, policy_seed, _p(ret),
                                 self.nthreads)
        return ret

    def policy_actions(self, n_steps, policy_seed):
        """actions [n_steps][n][2] of the on-device random policy, for calls 0..n_steps-1."""
        out = np.empty((n_steps, self.n, 2), dtype=np.float32)
        a = (C.c_float * 2)()
        for s in range(n_steps):
            for i in range(self.n):
                lib().sbro_policy_action(C.byref(self.p), policy_seed, self.first_env_id + i, s, a)
                out[s, i] = a[0], a[1]
        return out


def eval_rhs(kind, x, kla, ec, loading=None, params=None):
    p = params if params is not None else default_params()
    x = _f64(x)
    dx = np.empty_like(x)
    ld = None if loading is None else _f64(loading)
    lib().sbro_eval_rhs(C.byref(p), kind, len(x), _p(x), _p(_f64(kla)), _p(_f64(ec)), _p(ld), _p(dx))
    return dx


def rhs_reaction(x, kla, ec=0.0, params=None):
    """dx/dt [14] of one state in a reaction phase."""
    p = params if params is not None else default_params()
    d = np.empty(NX)
    lib().sbro_rhs_reaction(C.byref(p), _p(_f64(x)), kla, ec, _p(d))
    return d


def rk4(kind, x, span, n, kla, ec=0.0, loading=None, params=None):
    p = params if params is not None else default_params(scheme=0)
    x = np.array(x, dtype=np.float64)
    ld = None if loading is None else _f64(loading)
    lib().sbro_rk4(C.byref(p), kind, _p(x), span, n, kla, ec, _p(ld))
    return x


def _reaction_interval(fn, x, span, kla, ec, params, scheme):
    p = params if params is not None else default_params()
    p.scheme = scheme
    x = np.array(x, dtype=np.float64)
    return x, int(fn(C.byref(p), _p(x), span, kla, ec))


def reaction_interval(x, span, kla, ec=0.0, params=None, scheme=1):
    """One reaction interval by the scheme-aware integrator of the C oracle (scheme 1: the adaptive Butcher-5 of round 5).
    Returns (x_end, step count; 0 = fell back to RK4, -1 = scheme 0)."""
    return _reaction_interval(lib().sbro_reaction_interval, x, span, kla, ec, params, scheme)


def reaction_interval_plan(x, span, kla, ec=0.0, params=None, scheme=1):
    """The same, returning the plan code instead: step count + 128 if the oxygen mode was slaved (-1 = scheme 0)."""
    return _reaction_interval(lib().sbro_reaction_interval_plan, x, span, kla, ec, params, scheme)


@contextlib.contextmanager
def plan_knobs(zr_stab):
    """The study-only stability floor of scheme 1's plan (sbr_oracle.c, ZR_STAB; a global of the loaded library) for
    the duration of a with block; off (0.0) again on the way out, whatever happened inside."""
    knobs = lib().sbro_set_plan_knobs
    knobs(zr_stab)
    try:
        yield
    finally:
        knobs(0.0)


def reward_g2anet(x):
    """cfg.reward_kind = 1 (module_reward_continuous_G2ANET.py): the reward of one state x [14], or of each row of x [n][14]."""
    x = _f64(x)
    fn = lib().sbro_reward_g2anet
    return fn(_p(x)) if x.ndim == 1 else np.array([fn(_p(row)) for row in x])


def reward_oci(so_sat, kla_last, kla_sum, batch_type, qin, qw, q_eff, snh_eff):
    """cfg.reward_kind = 2 (module_reward_continuous.py:4-65), one call of the reference's function."""
    return lib().sbro_reward_oci(so_sat, kla_last, kla_sum, batch_type, qin, qw, q_eff, snh_eff)


class OracleCycleBatch:
    """N per-cycle (`SBR-v2`) environments stepped by the C oracle: one step() = one whole 12 h cycle."""

    def __init__(self, n, params=None, nthreads=1):
        self.n, self.nthreads = int(n), int(nthreads)
        self.p = params if params is not None else default_params()
        self.x = np.tile(np.array(self.p.x0[:], dtype=np.float64), (self.n, 1))
        self.influent = np.zeros((self.n, NX))

    def reset(self, influent, carry_over=False):
        self.influent = _f64(np.broadcast_to(influent, (self.n, NX))).copy()
        if not carry_over:
            self.x = np.tile(np.array(self.p.x0[:], dtype=np.float64), (self.n, 1))
        st = np.empty((self.n, 3))
        for i in range(self.n):
            lib().sbro_cycle_reset_state(_p(self.x[i]), _p(self.influent[i]), _p(st[i]))
        return st

    def step(self, action):
        action = _f64(np.broadcast_to(action, (self.n, 3)))
        st, rew, diag = np.empty((self.n, 3)), np.empty(self.n), np.empty((self.n, NCYC_DIAG))
        self.x = np.ascontiguousarray(self.x)
        lib().sbro_batch_cycle_step(C.byref(self.p), self.n, _p(self.x), _p(self.influent), _p(action), _p(st), _p(rew),
                                    _p(diag), self.nthreads)
        return st, rew, diag

    def step_logged(self, i, action):
        """One env, with the per-interval Kla of the six PID phases (6 x 256, NaN-padded)."""
        log = np.full(NKLA_LOG, np.nan)
        st, rew, diag = np.empty(3), np.empty(1), np.empty(NCYC_DIAG)
        x = np.ascontiguousarray(self.x[i]).copy()
        lib().sbro_cycle_step(C.byref(self.p), _p(x), _p(np.ascontiguousarray(self.influent[i])), _p(_f64(action)), _p(st),
                              _p(rew), _p(diag), _p(log))
        self.x[i] = x
        return st, float(rew[0]), diag, log
