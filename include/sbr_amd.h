/*
 * sbr_amd.h - C ABI of the MI355X-native batched SBR environment (libsbr_amd.so).
 *
 * Drop-in boundary for ONE path of SungKu/gym-SBR2: the step-level env `SBROS-v1`
 * (gym_SBR/envs/gym_SBR_oneshot.py::SbrOS; registered at gym_SBR/__init__.py:11).  The
 * reference has no FFI - its boundary is the gym.Env protocol - so each entry point names the
 * Python method it replaces.  All array arguments are DEVICE pointers (HIP, e.g.
 * torch.Tensor.data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream).
 * No torch types, no C++ types.  Every call returns 0 on success or a negative sbr_status; the
 * message is available from sbr_last_error().  Nothing here ever falls back to the CPU.
 *
 * Layouts
 *   action  [N][2]  ActT      (u_DO set-point, u_EC set-point)   gym_SBR_oneshot.py:843,862,898
 *                             ActT = float32 (cfg.act_f64 = 0) or float64 (cfg.act_f64 = 1, what the reference's
 *                             step() receives; the NO3 loop's gain makes EC sensitive to set-point rounding)
 *   obs     [N][18] OutT      obs_DO[9] ++ obs_EC[9]             gym_SBR_oneshot.py:1027-1114
 *   state   [N][15] OutT      [t, x0..x13] / x_1_state           gym_SBR_oneshot.py:1020-1025
 *   reward  [N]     OutT                                         module_reward_EQIOCI.py:4-115
 *   done    [N]     uint8                                        gym_SBR_oneshot.py:1122-1124
 *   OutT = float32 (cfg.out_f64 = 0, the RL path) or float64 (cfg.out_f64 = 1, parity checks).
 *   Internal plant/controller state is float64, struct-of-arrays [field][N] (sbr_get_state).
 */
#ifndef SBR_AMD_H
#define SBR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBR_NX 14          /* V Si Ss Xi Xs Xbh Xba Xp So Sno Snh Snd Xnd Salk (gym_SBR_oneshot.py:185-188) */
#define SBR_NOBS 18
#define SBR_NSTATE 15
#define SBR_NACT 2
#define SBR_NSCEN 8        /* influent scenarios, buffer_tank3.py:18-1197 */
#define SBR_NSAMP 48       /* samples per influent series */
#define SBR_NSERIES 14     /* 13 concentrations + flow q */
#define SBR_KLA_HIST 10    /* Kla values the reward can look back on (current + 9) */
/* controller/bookkeeping doubles per env exposed by sbr_get_state/sbr_set_state, in this order.  This is the PUBLIC
 * layout; the kernels keep a leaner internal one (Kla history as a ring, packed bookkeeping) and translate. */
#define SBR_NCTRL 25
enum {
    SBR_C_T = 0,           /* running time t (days)                     gym_SBR_oneshot.py:1357 */
    SBR_C_SO_M1, SBR_C_SO_M2, SBR_C_SNO_M1, SBR_C_SNO_M2,   /* So[-1] So[-2] Sno[-1] Sno[-2]  :1959-1961 */
    SBR_C_IE_DO, SBR_C_IE_EC,                               /* PID integrals                  :1893,:1923 */
    SBR_C_EC_LAST,                                          /* EC[-1] */
    SBR_C_KLA_HIST0,                                        /* 10 entries, oldest first; the last is Kla[-1] */
    SBR_C_KLA_LAST = SBR_C_KLA_HIST0 + SBR_KLA_HIST - 1,
    SBR_C_QW,                                               /* wastage flow of the last terminal step :2376 */
    SBR_C_RETURN,                                           /* sum of rewards since reset */
    SBR_C_STEPS,                                            /* step() calls since reset (as double) */
    SBR_C_DONE,                                             /* 1.0 once the episode ended */
    SBR_C_STATUS,                                           /* sticky SBR_ST_* bits since reset (as double) */
    SBR_C_KLA_SUM,                                          /* sum(Kla) of the episode's whole list, in append order:
                                                               the 252 reset entries (:323), one per interval, idle's.
                                                               Advanced only with reward_kind 2 (else: its reset value) */
    SBR_C_PLAN                                              /* (round 6) what cfg.scheme = 1 did in the LAST control interval
                                                               sbr_step ran for this env: its Butcher-5 step count (1 .. 64)
                                                               + SBR_PLAN_SLAVED if dissolved oxygen was held during the
                                                               steps.  0 = nothing to report: cfg.scheme = 0, no sbr_step
                                                               since the reset / sbr_set_state / sbr_rollout.  The reference's
                                                               counterpart is LSODA's infodict (nst, nfe) at its odeint call
                                                               sites (gym_SBR_oneshot.py:1953, :2041).  sbr_set_state keeps
                                                               the value given (0 .. 255).  Costs no memory traffic: it shares
                                                               the internal row of steps / status / done */
};
#define SBR_PLAN_SLAVED 128
#define SBR_PLAN_STEPS(code) ((int)(code) & 127)
/* (The reference's u_DO / u_EC globals and the EC value before EC[-1] are temporaries of one step() call - every
 * interval overwrites them before use - so they are not part of the state.) */

/* Domain-of-validity flags.  The ASM1 rate expressions x/(K+x) have poles at x = -K and the reference has no
 * guards (gym_SBR_oneshot.py:1660-1685): heterotrophic growth takes up ammonia without an ammonia limitation, so an
 * aggressive policy can drive Snh (also So, Sno) below zero and towards a pole, after which the reference - and this
 * library, which reproduces it - returns numbers without physical meaning.  The numerics are NOT altered; these
 * bits, checked at the end of every control interval, only make the condition visible. */
#define SBR_ST_NEGATIVE 1   /* one of Ss, Xs, Xbh, So, Sno, Snh was below -1e-6 */
#define SBR_ST_NEAR_POLE 2  /* Ss, So, Sno or Snh came within 50 % of a Monod pole (x < -K/2): parity to 1e-5 between
                               any two fp64 implementations holds only while this bit is clear (tests/) */
#define SBR_ST_NONFINITE 4  /* a state component is NaN or infinite */

typedef enum {
    SBR_OK = 0,
    SBR_ERR_INVALID = -1,      /* bad argument */
    SBR_ERR_NO_DEVICE = -2,    /* no HIP device / wrong architecture */
    SBR_ERR_HIP = -3,          /* a HIP runtime call failed */
    SBR_ERR_ALLOC = -4
} sbr_status;

/* Every constant of the path.  sbr_default_config() fills in the reference's values
 * (SURVEY.md Appendix A lists file:line for each). */
typedef struct sbr_config {
    /* ASM1 stoichiometry / kinetics                              gym_SBR_oneshot.py:116-119 */
    double Ya, Yh, fp, ixb, ixp;
    double muH, Ks, Koh, Kno, bH, eta_g, eta_h, kh, Kx, muA, Knh, bA, Koa, ka;
    /* plant + time grid                                          gym_SBR_oneshot.py:25-37 */
    double WV, IV, dt, t_delta, t_cycle;
    double T_fill, T3_0, T3_end, T4_end, T5_end;      /* phase scalars, module_batch_time.py:3-116 */
    double t_settle, t_draw;                          /* t_ratio[5], t_ratio[6] (fractions of t_cycle) */
    /* controllers                                                gym_SBR_oneshot.py:80-96 */
    double So_sat, Kla_min, Kla_max, Kc_DO, tauI_DO, tauD_DO;
    double EC_min, EC_max, Kc_EC, tauI_EC, tauD_EC, EC_conc;
    double act_DO_max, act_EC_max;                    /* action clipping :865-870, :901-906 */
    /* terminal phases                                            gym_SBR_oneshot.py:123-124, :2189-2218 */
    double biomass_setpoint, Qeff, settler_area, settler_vmax;
    /* per-cycle env SBR-v2 (gym_SBR_env2.py:32-48, SBR_model_FB.py:18-29): the eight phase fractions of the cycle and
     * the positional DO-PID of sub_phases_FB.py:178-271 (DO_control_par = [Kc, tauI, delt, ..., tauD = [9]]) */
    double t_ratio[8];
    double cyc_Kc, cyc_tauI, cyc_tauD, cyc_dt;
    double x0[SBR_NX];                                /* episode start state :201-203 */
    /* integrator */
    int32_t substeps;          /* RK4 substeps per control interval (10 => h = dt) */
    int32_t out_f64;           /* 0: obs/state/reward are float32; 1: float64 */
    int32_t terminal;          /* 1: run settle/draw/idle on the done step (reference behaviour) */
    int32_t reward_kind;       /* 0: EQI/OCI reward of module_reward_EQIOCI.py (SBROS-v1); 1: the piecewise-linear reward of
                                  module_reward_continuous_G2ANET.py:4-45 (used by the variant gym_SBR_oneshot_copy.py:17,614);
                                  2: the operating-cost reward of module_reward_continuous.py:4-65 (SbrEnv3/SbrEnv4): its
                                  reaction-interval branch (0.5 - AE of the Kla just applied) on every call, and on the
                                  done call, when the terminal phases run, its end-of-cycle branch (sum(Kla) of the whole
                                  episode, pumping of Qw and Qeff, -246 if the effluent ammonia is >= 4 g/m3) */
    int32_t act_f64;           /* 0: sbr_step reads float32 actions; 1: float64.  A finished env ignores step()
                                  until sbr_reset either way (the reference leaves resetting to the caller) */
    int32_t random_scenario;   /* what sbr_reset / sbr_cycle_reset do when `scenario` is NULL: 0 = the fixed scenario of the
                                  reference class (6 for SbrOS :180, 0 for SbrEnv2 :104); 1 = draw one of the 8 scenarios
                                  per env and reset on the device, uniformly, as SbrEnv4.reset does with
                                  np.random.choice(8, 1) (gym_SBR_env4.py:107): Philox4x32-10 keyed by `seed`, stream 2,
                                  subsequence = GLOBAL env id (sbr_draw_scenarios returns the same draw) */
    int32_t scheme;            /* how the control intervals of sbr_step / sbr_rollout (reaction_dxdt :1658-1787, odeint call sites
                                  :1953, :2041), the idle phase of the done call (:2587) and the reaction and idle intervals of
                                  sbr_cycle_step are integrated.  (The fill phase - sbr_reset, :1647, and sbr_cycle_step's first
                                  phase - is integrated with RK4, h = dt, under either scheme.)
                                  0: classical RK4, `substeps` substeps per control interval (40 right-hand-side evaluations).
                                  1 (default, round 5): Butcher's fifth-order scheme with 1, 2 or 4 steps chosen per env and
                                  interval from the env's own state - dissolved oxygen, the system's one stiff mode, is held
                                  where it is slaved to zero, and an env whose oxygen mode is stiffer than the reference plant's
                                  takes more steps, as does one whose substrate, ammonia or nitrate moves across its
                                  half-saturation constant within the interval: ~10 evaluations per interval, and closer to the
                                  reference's trajectories than scheme 0 (closed loop, worst 0.36 of the 1e-5 gate against 0.51).
                                  `substeps` then only sets the fill intervals of sbr_cycle_step; the idle phase is cut into
                                  ceil(rows / 10) macro intervals.  sbr_eval_substeps replays RK4 nodes under either scheme.
                                  VALIDITY DOMAIN of scheme 1 (round 6).  The step count is a start-of-interval plan, not an error
                                  estimate.  What it bounds by construction: the oxygen mode's rate times the step (<= 2.5 of
                                  Butcher-5's real stability limit 3.39, whatever the kinetic constants and the biomass).  What it
                                  ASSUMES: every other mode (uptake of Ss, Snh, Sno; hydrolysis) has |lambda| * t_delta below
                                  ~2.5 - with the reference's constants they stay below 1.0 on every captured interval, 2.2 in
                                  the idle phase's thickened sludge.  Pinned to the reference on 24 fitted + 10 held-out
                                  episodes (closed loop <= 0.373 of the gate), 36 000 intervals of the per-cycle env, and probed
                                  off-regime: on random states of a plant with muH, muA, kh up to 4 x faster it misses the gate
                                  on 134 of 2 836 states (11 beyond 30 gates) where scheme 0 misses 420 (239): scheme 0's fixed
                                  h = dt is unstable once the oxygen rate times dt exceeds 2.785, scheme 1's count grows with
                                  it (tests/test_oracle_golden.py::test_scheme1_under_perturbed_kinetic_constants,
                                  ..._plan_on_states_far_from_the_reference_regime).  A configuration with kinetics several
                                  times faster than the reference's or a longer t_delta is outside what either scheme was
                                  validated on: check it against a fine solution (sbr_eval_substeps with many substeps) first.
                                  OUTSIDE THE MODEL'S DOMAIN (the Monod factor of Ss or Snh outside [0, 1]: a concentration
                                  negative towards or beyond its pole, or NaN - SBR_ST_NEAR_POLE is then set or about to be) the
                                  oxygen rate is no longer bounded and the step count is NOT raised above the knee's four: the
                                  state is garbage either way (the reference has no guards), and a launch lasts as long as its
                                  slowest wavefront - one such env at the cap of 64 steps made a whole 65 536-env batch
                                  several times slower (round 6).  In-domain states are unaffected.
                                  What scheme 1 did is observable per env and call: SBR_C_PLAN, SBR_TR_PLAN. */
    int32_t reserved_;         /* keeps the struct a multiple of 8 bytes; MUST be 0: sbr_create rejects anything else with
                                  SBR_ERR_INVALID (round 6), so that a later round can give the word a meaning */
} sbr_config;

typedef struct sbr_env sbr_env;      /* opaque handle: owns all device state for N envs on one GPU */

/* library / configuration ---------------------------------------------------------------- */
const char* sbr_version(void);
/* Bumped whenever a signature, a struct layout or a record width of this header changes.  A consumer compiled against this
 * header checks sbr_abi_version() == SBR_ABI_VERSION once after loading the library (round 4 = 4: sbr_set_trace takes the
 * record width, SBR_NTRACE = 34; round 5 = 5: sbr_config.scheme; round 6 = 6: SBR_NCTRL = 25 with SBR_C_PLAN, SBR_NTRACE = 36 with
 * SBR_TR_PLAN / SBR_TR_PLAN_FIRST, sbr_query, sbr_config.reserved_ checked). */
#define SBR_ABI_VERSION 6
int sbr_abi_version(void);
int sbr_default_config(sbr_config* cfg);
int sbr_device_count(void);          /* HIP devices visible; 0 if none (never throws) */
/* Host-side helper, no device needed: the reference's control interval has len(t_range) = int(((t + t_delta) - t)/dt) output
 * rows (gym_SBR_oneshot.py:1339, :1384), 9 or 10 depending on the rounding of (t + t_delta) - t, and the reward's look-back
 * depends on it.  The kernels decide it with two comparisons: out2[0] / out2[1] = the smallest doubles s for which the IEEE
 * quotient s/dt reaches 9.0 / 10.0 (rows = 10 iff span >= out2[1], 9 iff out2[0] <= span < out2[1]; any other span takes the
 * division itself).  cfg NULL = defaults. */
int sbr_rows_thresholds(const sbr_config* cfg, double* out2);

/* lifetime: replaces SbrOS.__init__ (gym_SBR_oneshot.py:103-166) for N instances.
 * first_env_id: global id of local env 0 (multi-GPU sharding: RNG streams and scenario
 * assignment depend on the GLOBAL id, so results do not depend on world size). */
int sbr_create(int64_t n_envs, int device_id, int64_t first_env_id, const sbr_config* cfg /* NULL = defaults */,
               sbr_env** out);
int sbr_destroy(sbr_env* env);
const char* sbr_last_error(const sbr_env* env /* NULL = creation errors */);
int64_t sbr_num_envs(const sbr_env* env);

/* What the library decided for this handle from its size and the device it sits on (round 6).  The launch shapes depend on the
 * device's CU count - a partitioned MI355X has fewer than 256 - so a consumer that wants to NAME the kernel a handle runs
 * (bench.py's `config.kernel`, a profiler's filter) asks instead of repeating thresholds.  out receives one integer. */
enum {
    SBR_Q_ONE_WAVE_ENVS = 0,            /* envs that put one wavefront on every SIMD of the device: CUs x 4 x 64 (MI355X: 65536) */
    SBR_Q_STEP_SMALL_BATCH_ENVS,        /* up to this many envs sbr_step launches 64-thread workgroups (49152) */
    SBR_Q_STEP_BLOCK,                   /* workgroup size of THIS handle's sbr_step launches: 64 or 256 */
    SBR_Q_STEP_WAVES,                   /* 1 or 2: which register budget of k_step THIS handle runs (2 = two waves per SIMD:
                                           cfg.scheme = 1 and more envs than SBR_Q_STEP_TWO_WAVES_ABOVE_ENVS) */
    SBR_Q_STEP_TWO_WAVES_ABOVE_ENVS,
    SBR_Q_FUSED_ONE_WAVE_MAX_ENVS,      /* up to this many envs sbr_rollout / sbr_cycle_step run their uncapped-register build */
    SBR_Q_ROLLOUT_WAVES,                /* 1 or 2 for THIS handle's sbr_rollout (and sbr_cycle_step under cfg.scheme = 1) */
    SBR_Q_RESET_BLOCK,                  /* workgroup size of THIS handle's sbr_reset launches: 256 or 512 */
    SBR_Q_SCHEME                        /* cfg.scheme in force */
};
int sbr_query(const sbr_env* env, int32_t what, int64_t* out);

/* influent data: replaces the literals of buffer_tank3.py:18-1197.  means/stds are HOST pointers,
 * [SBR_NSCEN][SBR_NSERIES][SBR_NSAMP] float64; copied to the device once. */
int sbr_set_influent_tables(sbr_env* env, const double* means_host, const double* stds_host);

/* reset: replaces SbrOS.reset() (gym_SBR_oneshot.py:168-438) = influent draw
 * (buffer_tank3.py:68-107) + fill phase (Sim_filling :1585-1654) + reset observation.
 *   scenario  [N] int32 or NULL (NULL = scenario 6 for every env, as the reference :180)
 *   rnd       [N][48] float64 or NULL; NULL => drawn on the device: Philox4x32-10 keyed by `seed`,
 *             subsequence = global env id, Box-Muller (the reference draws np.random.randn(48))
 *   influent  [N][14] float64 or NULL; if given it REPLACES the draw (entry 0 is overwritten by
 *             Qin/T_fill as at :287)
 *   mask      [N] uint8 or NULL; if given only envs with mask != 0 are reset
 *   obs       [N][18] OutT or NULL */
int sbr_reset(sbr_env* env, uint64_t seed, const int32_t* scenario, const double* rnd, const double* influent,
              const uint8_t* mask, void* obs, void* stream);

/* multi-cycle operation: like sbr_reset, but every selected env starts the new cycle from ITS OWN current
 * state - x0 := x (normally the state after the idle phase), inoculum volume IV := x[0], inflow := (WV - IV)/T_fill -
 * instead of cfg.x0 / cfg.IV.  This is what the reference prepares (x0_new, IV_new at gym_SBR_env2.py:152-153) and then
 * leaves disabled (gym_SBR_oneshot.py:260-268: "IV = IV_init  # IV_new"), so there is no reference output to compare
 * with: parity is pinned device-vs-oracle only. */
int sbr_reset_carry(sbr_env* env, uint64_t seed, const int32_t* scenario, const double* rnd, const double* influent,
                    const uint8_t* mask, void* obs, void* stream);

/* trajectory export (replaces the growing lists of SbrOS.trajectory(), gym_SBR_oneshot.py:1275-1288): while a trace
 * buffer is set, every sbr_step call appends one record for each of the first n_envs environments at index = calls since
 * reset (records beyond capacity are dropped).  buf is [capacity][SBR_NTRACE][n_envs] float64, DEVICE pointer, owned by
 * the caller; buf = NULL switches tracing off.  Record (SBR_TR_*): t, x[14] (end of the call), Kla, EC (of the call's last
 * interval), reward, done, the clipped set-points u_DO / u_EC in force (:862-870, :898-906), the NO3-PID's e_EC, ie_EC,
 * dcv_EC (:1918-1926, :2006-2014) and the four diagnostics sbr_reward appends (module_reward_EQIOCI.py:109-112):
 * EQI2, OCI2 = AE_OCI2 + EC_OCI2, AE_OCI2, EC_OCI2; then what a consumer needs to rebuild the reference's sub-interval rows
 * (sbr_eval_substeps): the number of control intervals the call ran (1, or 2 on a phase-boundary call) and the Kla / EC of
 * the FIRST of them (equal to SBR_TR_KLA / SBR_TR_EC when the call ran one); and (round 4) the NO3-PID's e_EC, ie_EC, dcv_EC
 * of that FIRST interval too: the reference appends to these three lists once per INTERVAL (:1918-1926, :2006-2014), so a
 * phase-boundary call contributes two entries each (equal to SBR_TR_E_EC / _IE_EC / _DCV_EC when the call ran one).
 * (Round 6) SBR_TR_PLAN / SBR_TR_PLAN_FIRST: what cfg.scheme = 1 did in the call's last / first interval, coded like SBR_C_PLAN
 * (step count + SBR_PLAN_SLAVED; equal when the call ran one interval; 0 under cfg.scheme = 0).
 * record_width must be SBR_NTRACE of the header the caller was compiled against: the record grew from 28 to 31 to 34 to 36 doubles
 * over the rounds, and a buffer sized for an older width would be overrun silently - a mismatch is SBR_ERR_INVALID. */
#define SBR_NTRACE 36
enum { SBR_TR_T = 0, SBR_TR_X0 = 1, SBR_TR_KLA = 15, SBR_TR_EC, SBR_TR_REWARD, SBR_TR_DONE, SBR_TR_U_DO, SBR_TR_U_EC,
       SBR_TR_E_EC, SBR_TR_IE_EC, SBR_TR_DCV_EC, SBR_TR_R_EQI, SBR_TR_R_OCI, SBR_TR_R_AE, SBR_TR_R_EC,
       SBR_TR_N_IV, SBR_TR_KLA_FIRST, SBR_TR_EC_FIRST, SBR_TR_E_EC_FIRST, SBR_TR_IE_EC_FIRST, SBR_TR_DCV_EC_FIRST,
       SBR_TR_PLAN, SBR_TR_PLAN_FIRST };
int sbr_set_trace(sbr_env* env, double* buf, int64_t n_envs, int64_t capacity, int32_t record_width);

/* step: replaces SbrOS.step(action) (gym_SBR_oneshot.py:843-1273): phase logic, both PIDs,
 * one (at phase boundaries two) control interval(s) of RK4, reward, observations, and on the last
 * call of an episode the settle/draw/idle phases.  Any of obs/state/reward/done may be NULL. */
int sbr_step(sbr_env* env, const void* action, void* obs, void* state, void* reward, uint8_t* done,
             void* stream);

/* ---- per-cycle environment `SBR-v2`: gym_SBR/envs/gym_SBR_env2.py::SbrEnv2, registered at
 * gym_SBR/__init__.py:5.  One step() = one whole 12 h cycle: SBR_model_FB.run (SBR_model_FB.py:8-295) over the phase
 * simulators of sub_phases_FB.py, reward module_reward.py:4-51.  A handle is used EITHER for sbr_reset/sbr_step OR for
 * these two calls.
 *   action [N][3] ActT in [0,1] (clipped): DO set-points of phases 3, 5 and 8 are action*8   gym_SBR_env2.py:133,184-186
 *   obs    [N][3] OutT: reset: [V0 + 0.66, (COD0 + COD_in - 5145)/10, (Snh0 + Snh_in)/30]       :108-119
 *                       step:  [Qeff, COD_eff, Snh_eff/30]                                      :164-169
 *   diag   [N][SBR_NCYC_DIAG] float64 or NULL: Qw, EQI, OCI, effluent Ntot COD Snh BOD5 Sno, mean Kla of phases 3/5/8, Xf */
#define SBR_NCYC_ACT 3
#define SBR_NCYC_OBS 3
#define SBR_NCYC_DIAG 12
/* replaces SbrEnv2.reset(): influent draw (scenario NULL = 0 as at :104; rnd/influent/mask as in sbr_reset) and the reset
 * observation.  carry_over != 0 keeps every env's current state as the start state of the next cycle (x0_new / IV_new,
 * :152-153, disabled upstream at :85-97) instead of cfg.x0. */
int sbr_cycle_reset(sbr_env* env, uint64_t seed, const int32_t* scenario, const double* rnd, const double* influent,
                    const uint8_t* mask, int32_t carry_over, void* obs, void* stream);
/* replaces SbrEnv2.step(action): every call is a complete episode (done is always true, :161). */
int sbr_cycle_step(sbr_env* env, const void* action, void* obs, void* reward, double* diag, void* stream);

/* read-only lookahead over WHOLE CYCLES: `fanout` candidate tapes of n_cycles cycles per env, each played from the env's CURRENT
 * state and stored influent in one launch, the handle left bit for bit as it was (which three DO set-points should this plant
 * run in the cycle it is about to start, and what does the choice do to the sludge over the next cycles?).
 * A BRANCH is j = i*fanout + k: env i, candidate k; there are B = N*fanout < 2^31 of them.
 *   actions     [n_cycles][B][3] ActT, DEVICE pointer - a [n_cycles][N][fanout][3] array has this layout.  Clipped to [0,1] as in
 *               sbr_cycle_step.
 *   returns     [B] float64 or NULL: sum of the branch's rewards, added in cycle order from 0.0
 *   rewards_out [n_cycles][B] float64 or NULL: the reward of every cycle - the double sbr_cycle_step casts to OutT
 *   best_index  [N] int32 or NULL, best_return [N] float64 or NULL: the winner among each env's `fanout` returns under the rule
 *               of sbr_lookahead_actions (the largest wins, NaN compares as -inf, ties go to the lowest k), reduced FROM
 *               `returns` by a second kernel on the same stream: give returns with them
 *   obs_end     [B][SBR_NCYC_OBS] float64 or NULL: Qeff, COD_eff, Snh_eff/30 of the branch's LAST cycle - the doubles
 *               sbr_cycle_step casts to OutT
 *   diag_end    [B][SBR_NCYC_DIAG] float64 or NULL: the diag row of the branch's last cycle
 *   status_out  [B] uint8 or NULL: the OR of the SBR_ST_* bits of the branch's state at the start and at the end of every cycle
 *               of the launch, to mask candidates that left the model's domain
 * Cycle 0 of a branch is sbr_cycle_step on a copy of env i.  Cycle c > 0 starts from the branch's own state after the aerated
 * idle of cycle c - 1 under env i's stored influent: what sbr_cycle_reset(carry_over = 1, influent = the env's own) followed
 * by sbr_cycle_step computes, with the same bits in every output.
 * NOTHING of the handle is written - not the plant, not a controller row, not the influent - and nothing is allocated
 * (graph-capturable).  The register budget of the launch goes by B, not by N.
 * n_cycles = 0 writes returns = 0, best_index = 0 and best_return = 0 and reads nothing.
 * SBR_ERR_INVALID, before anything is touched (the last failing check is reported): NULL env; n_cycles < 0; fanout < 1;
 * N*fanout >= 2^31; actions NULL with n_cycles > 0; best_index or best_return given while returns is NULL; obs_end, diag_end or
 * status_out given with n_cycles = 0. */
int sbr_cycle_lookahead(sbr_env* env, int32_t n_cycles, int32_t fanout, const void* actions,
                        double* returns, double* rewards_out, int32_t* best_index, double* best_return,
                        double* obs_end, double* diag_end, uint8_t* status_out, void* stream);

/* sbr_cycle_lookahead under UNCERTAIN influent: `fanout` candidate tapes per env, each played against `n_scen` influent futures -
 * the SAME n_scen futures for every candidate of an env (common random numbers), so that candidates are compared on futures and
 * not on noise.  sbr_cycle_lookahead plays every later cycle under the influent the env was last reset with, the one thing an
 * operator does not know; here every cycle of every future has an influent of its own, and the env's STORED influent is never read.
 * A BRANCH is j = (i*fanout + k)*n_scen + s: env i, candidate k, future s; there are B = N*fanout*n_scen < 2^31 of them.
 *   actions     [n_cycles][N*fanout][3] ActT, DEVICE pointer: sbr_cycle_lookahead's tape, not expanded over s
 *   influent    [n_cycles][N*n_scen][SBR_NX] float64, DEVICE pointer: sbr_draw_influent's layout, not expanded over k.  Cycle c of
 *               branch j runs under entries 1..13 of influent[c][i*n_scen + s] and forms entry 0 from its own volume - what
 *               sbr_cycle_reset(carry_over = 1, influent = that row) followed by sbr_cycle_step computes, with the same bits in
 *               every output.  A caller who wants cycle 0 under the influent the env holds puts it into row 0.
 *   returns     [B] float64 or NULL: sum of the branch's rewards, added in cycle order from 0.0
 *   rewards_out [n_cycles][B] float64 or NULL: the reward of every cycle
 *   mean_out    [N*fanout] float64 or NULL: ((..(0.0 + r_0) + r_1 ..) + r_{S-1}) / (double)S over the candidate's n_scen returns in
 *               s order, one IEEE division; a NaN propagates
 *   worst_out   [N*fanout] float64 or NULL: the smallest of the candidate's n_scen returns, NaN if any of them is NaN.  Both are
 *               reduced FROM `returns` by a second kernel on the same stream: give returns with them
 *   best_index  [N] int32 or NULL, best_value [N] float64 or NULL: the winner among each env's `fanout` entries of mean_out under
 *               the rule of sbr_lookahead_actions, reduced FROM `mean_out`: give mean_out with them (a caller who plans for the
 *               worst case passes worst_out to sbr_branch_best)
 *   obs_end [B][SBR_NCYC_OBS], diag_end [B][SBR_NCYC_DIAG] float64, status_out [B] uint8, each or NULL: as in sbr_cycle_lookahead
 * NOTHING of the handle is written and nothing is allocated (graph-capturable).  The register budget of the launch goes by B.
 * n_cycles = 0 writes returns = mean_out = worst_out = 0, best_index = 0 and best_value = 0 and reads nothing.
 * SBR_ERR_INVALID, before anything is touched (the last failing check is reported): NULL env; n_cycles < 0; n_scen < 1;
 * fanout < 1; N*fanout*n_scen >= 2^31; actions or influent NULL with n_cycles > 0; obs_end, diag_end or status_out given with
 * n_cycles = 0; mean_out or worst_out given while returns is NULL; best_index or best_value given while mean_out is NULL. */
int sbr_cycle_lookahead_scenarios(sbr_env* env, int32_t n_cycles, int32_t fanout, int32_t n_scen,
                                  const void* actions, const double* influent,
                                  double* returns, double* rewards_out, double* mean_out, double* worst_out,
                                  int32_t* best_index, double* best_value,
                                  double* obs_end, double* diag_end, uint8_t* status_out, void* stream);

/* ---- the per-cycle lookahead under UNCERTAIN PLANT KINETICS: futures over MODELS.  Every branch of the two calls above integrates
 * the one plant the handle was created with.  The influent is half of what an operator does not know; the other half is the sludge:
 * the ASM1 rate constants (muA above all), the yields, and the oxygen saturation, which moves with temperature.  A handle can hold
 * a TABLE of plant models, and sbr_cycle_lookahead_models plays future s under model s % n_models of it - without a second
 * handle per model.  sbr_reset / sbr_step / sbr_cycle_step and every other call keep integrating the handle's own config and return
 * the same bits with or without a table.
 *
 * The MODEL FIELDS of sbr_config, the only ones in which a model may differ from the config of the handle:
 *     Ya, Yh, fp, ixb, ixp, muH, Ks, Koh, Kno, bH, eta_g, eta_h, kh, Kx, muA, Knh, bA, Koa, ka, So_sat.
 * Everything else - the time grid, the phase schedule, the controllers, the terminal phases, x0, the integrator, the dtypes, the
 * reward kind - picks a kernel build, a loop count or a schedule the handle has already fixed, and must be equal byte for byte.
 * A model is folded on the host exactly as sbr_create folds its config, so it carries its own stoichiometry, Monod denominators,
 * scheme-1 step plan and SBR_ST_* pole thresholds.  cfg.scheme's VALIDITY DOMAIN (above) applies to every model on its own:
 * kinetics several times faster than the reference's are outside what either scheme was validated on. */

/* Host only, no device needed.  SBR_OK if `model` is a valid config (what sbr_create checks) that differs from `base` (NULL =
 * the defaults) in model fields only.  Otherwise SBR_ERR_INVALID, and sbr_last_error(NULL) names this entry point and the first
 * field of the struct outside the model fields that differs ("t_delta", "x0[3]", ...), or - the model fields alone differing -
 * says what sbr_create would say about the config. */
int sbr_check_model(const sbr_config* base /* NULL = defaults */, const sbr_config* model);

/* The handle's model table: n_models configs, HOST pointer, each checked like sbr_check_model(the handle's config, model), folded
 * and copied to a device table the handle owns.  Replaces an earlier table; n_models = 0 drops it; sbr_destroy frees it.  The
 * allocation and the copy happen here and never at a launch, and the call waits for the device before an earlier table is freed
 * (a launch that reads it may be in flight).  Nothing else of the handle changes.  SBR_ERR_INVALID, before anything is touched
 * (the last failing check is reported): NULL env; n_models < 0; models NULL with n_models > 0; a model that fails the check
 * (named by its index). */
int sbr_set_models(sbr_env* env, int32_t n_models, const sbr_config* models /* HOST, [n_models] */);
/* models in the handle's table, 0 if none is set.  NULL env: SBR_ERR_INVALID, reported through sbr_last_error(NULL). */
int64_t sbr_num_models(const sbr_env* env);

/* sbr_cycle_lookahead_scenarios with two differences.
 *  (1) Future s runs under MODEL s % n_models of the handle's table, in every cycle: kinetics, stoichiometry, So_sat, the step plan
 *      of cfg.scheme = 1, the thresholds behind status_out.  The handle's own constants are not read by any branch: a caller who wants
 *      the nominal plant among the futures puts the handle's config into the table.  (n_scen and n_models are independent: n_scen =
 *      n_models gives every model one future, n_scen = 3 n_models three influents per model.)
 *  (2) influent may be NULL: every cycle of every future then runs under the env's STORED influent - sbr_cycle_lookahead's rule -
 *      and the futures differ by their model alone.  Otherwise [n_cycles][N*n_scen][SBR_NX] as in the scenarios call.
 * Everything else is that call's: a BRANCH is j = (i*fanout + k)*n_scen + s and B = N*fanout*n_scen < 2^31; the layouts of
 * `actions` ([n_cycles][N*fanout][3], not expanded over s) and of every output; mean_out / worst_out / best_index / best_value
 * and what they are reduced from; cycle c of branch j computing what sbr_cycle_reset(carry_over = 1, influent = its row) followed
 * by sbr_cycle_step computes on a handle CREATED WITH THAT MODEL's config and holding the branch's state, with the same bits in
 * every output.  NOTHING of the handle is written and nothing is allocated (graph-capturable).  The futures are the y axis of
 * the launch grid, so that a model stays uniform across a wavefront; the register budget of the launch goes by B.
 * n_cycles = 0 writes returns = mean_out = worst_out = 0, best_index = 0 and best_value = 0 and reads nothing.
 * SBR_ERR_INVALID, before anything is touched (the last failing check is reported): NULL env; no model table set; n_cycles < 0;
 * n_scen < 1; n_scen > 65535; fanout < 1; N*fanout*n_scen >= 2^31; actions NULL with n_cycles > 0; obs_end, diag_end or status_out
 * given with n_cycles = 0; mean_out or worst_out given while returns is NULL; best_index or best_value given while mean_out is
 * NULL. */
int sbr_cycle_lookahead_models(sbr_env* env, int32_t n_cycles, int32_t fanout, int32_t n_scen,
                               const void* actions, const double* influent,
                               double* returns, double* rewards_out, double* mean_out, double* worst_out,
                               int32_t* best_index, double* best_value,
                               double* obs_end, double* diag_end, uint8_t* status_out, void* stream);

/* fused rollout with an on-device uniform random policy (BASELINE.json configs[4]): n_steps step()
 * calls per env in ONE kernel, plant state held in registers; actions ~ U[0,act_DO_max] x
 * U[0,act_EC_max] from Philox keyed by policy_seed, subsequence = global env id, counter = call index.
 *   returns [N] float64 or NULL: sum of the rewards of these n_steps calls
 *   actions_out [n_steps][N][2] float32 or NULL: the sampled actions (for replay through sbr_step) */
int sbr_rollout(sbr_env* env, int32_t n_steps, uint64_t policy_seed, double* returns, float* actions_out,
                void* stream);

/* fused rollout over an action tape: n_steps fused step() calls per env in ONE kernel under the CALLER's actions
 * (open-loop evaluation of set-point sequences, replay of logged episodes, schedule sweeps).
 *   actions     [ceil(n_steps / hold)][N][2] ActT (float32, or float64 with cfg.act_f64 = 1), DEVICE pointer.
 *               Row r is in force for calls r*hold .. r*hold + hold - 1 OF THIS LAUNCH
 *               (row index is launch-relative, not the call count since reset). hold >= 1.
 *   returns     [N] float64 or NULL: sum of the rewards of this launch's calls, added in call order
 *   rewards_out [n_steps][N] float64 or NULL: the reward of every call; 0.0 for a call the env skipped
 *               because its episode had ended (before or during the launch)
 * Semantics otherwise exactly sbr_rollout's: a finished env ignores the remaining rows, the terminal phases
 * run once for the done call, SBR_C_PLAN reads 0 afterwards, no trace records, nothing allocated
 * (graph-capturable).  Fed the actions sbr_rollout sampled (actions_out), an env ends with the same bits.
 * n_steps = 0 leaves the handle as it is and writes returns = 0.  SBR_ERR_INVALID: NULL env, n_steps < 0, hold < 1,
 * actions NULL with n_steps > 0. */
int sbr_rollout_actions(sbr_env* env, int32_t n_steps, int32_t hold, const void* actions,
                        double* returns, double* rewards_out, void* stream);

/* read-only lookahead: `fanout` action tapes per env, each played from the env's CURRENT state, the handle left bit for bit as
 * it was (receding-horizon planning: score K candidate set-point sequences per live plant, pick, then sbr_step).
 * A BRANCH is j = i*fanout + k: env i, candidate k; there are B = N*fanout of them.
 *   actions     [ceil(n_steps / hold)][B][2] ActT, DEVICE pointer - a [rows][N][fanout][2] array has this layout.  Rows are
 *               held and indexed exactly as in sbr_rollout_actions.
 *   returns     [B] float64 or NULL: sum of the launch's rewards of the branch, added in call order
 *   rewards_out [n_steps][B] float64 or NULL: the reward of every call; 0.0 for a call the branch skipped
 *   best_index  [N] int32 or NULL, best_return [N] float64 or NULL: the winner among each env's `fanout` returns.
 *               The largest return wins; a NaN return compares as -inf; ties go to the lowest k.  best_return is the winner's
 *               entry of `returns` as it stands - so if all of an env's returns are NaN: index 0 and best_return = NaN.
 *               The two are reduced FROM `returns` by a second kernel on the same stream: `returns` must be given whenever
 *               either of them is (the call owns no memory and allocates none).
 * Branch j starts from env i's plant and controller record as they are - also in the form sbr_step leaves them - and runs the
 * calls sbr_rollout_actions would run on an env in that state, in the same order: its returns and rewards are the same bits.
 * A branch whose episode ends skips its remaining calls; the terminal phases behind the done call are not run (they change
 * only state that is discarded here; the end-of-cycle reward of reward_kind 2 is part of the done call and is included).
 * NOTHING of the handle is written: the plant, every controller row (SBR_C_PLAN and SBR_C_RETURN included) and the trace stay
 * as they are.  Nothing is allocated (graph-capturable).  The register budget of the launch goes by B, not by N.
 * n_steps = 0 writes returns = 0, best_index = 0 and best_return = 0 and reads nothing of the state.
 * SBR_ERR_INVALID, before anything is touched: NULL env; n_steps < 0; hold < 1; fanout < 1; N*fanout >= 2^31; actions NULL
 * with n_steps > 0; best_index or best_return given while returns is NULL. */
int sbr_lookahead_actions(sbr_env* env, int32_t n_steps, int32_t hold, int32_t fanout, const void* actions, double* returns,
                          double* rewards_out, int32_t* best_index, double* best_return, void* stream);

/* SAMPLED lookahead and the MPPI tape update: a sampling planner's whole iteration (perturb the nominal tape K times, score,
 * weight, average, advance) without a candidate tensor anywhere.  A candidate is a pure function of (seed, GLOBAL env id,
 * candidate, row), so the branch that integrates it draws it in its own lane and the update draws it again.
 *
 * THE SAMPLE a(g, k, r, c): env with GLOBAL id g, candidate k, launch-relative row r, component c (0 = u_DO, 1 = u_EC).
 *   (z_0, z_1)  one Box-Muller pair of Philox4x32-10, built as sbr_rollout_policy builds its noise pair: key = seed,
 *               counter = (r, 4 + 256*k, g_lo, g_hi) - stream 4 (0 - 3 are taken), k in the upper 24 bits of the stream word
 *   v = (double)nominal[r][i][c] + (double)sigma[c] * z_c          one multiply, one add, not fused
 *   a = (ActT)v, then a < lo ? lo : (a > hi ? hi : a) with lo[c], hi[c] cast to ActT (a NaN nominal stays NaN)
 *   keep_nominal = 1 and k = 0: v = nominal[r][i][c], no noise - candidate 0 is the (clamped) nominal tape itself.
 * ActT is the handle's action type (float32, or float64 with cfg.act_f64 = 1).  The sample depends on nothing else: not on
 * N, fanout, hold, the handle's state or the shard. */
typedef struct sbr_sampler {
    float sigma[2];        /* std of the perturbation of (u_DO, u_EC); >= 0, finite */
    float lo[2], hi[2];    /* candidates are clamped into [lo, hi]; finite, lo <= hi */
    uint64_t seed;
    int32_t keep_nominal;  /* 1: candidate 0 of every env is the nominal tape itself (clamped, no noise) */
    int32_t reserved_;     /* MUST be 0 */
} sbr_sampler;             /* 40 bytes */

/* sbr_lookahead_actions over SAMPLED tapes: branch j = i*fanout + k plays the tape a(g, k, ., .) of env i (global id g) from
 * env i's current state.
 *   nominal     [ceil(n_steps / hold)][N][2] ActT, DEVICE pointer: the tape the candidates are drawn around
 *   actions_out [ceil(n_steps / hold)][N*fanout][2] ActT or NULL: the candidates exactly as they were integrated
 *   returns, rewards_out, best_index, best_return: the layouts, the rule of the winner and the requirement (returns with
 *               best_*) of sbr_lookahead_actions
 * In every other respect the call IS sbr_lookahead_actions: rows held `hold` calls and launch-relative, a done branch skips its
 * remaining calls with reward 0, no terminal phases, the end-of-cycle reward of reward_kind 2 inside the done call, the
 * register budget by N*fanout, NOTHING of the handle written, nothing allocated, n_steps = 0 writes zeros and reads nothing.
 * Fed this call's actions_out, sbr_lookahead_actions returns the same bits in returns, rewards_out and best_*.
 * SBR_ERR_INVALID, before anything is touched: NULL env or sampler; a negative or non-finite sigma; a non-finite lo or hi, or
 * lo > hi; reserved_ != 0; fanout < 1 or > 2^24; N*fanout >= 2^31; n_steps < 0; hold < 1; nominal NULL with n_steps > 0;
 * best_index or best_return given while returns is NULL. */
int sbr_lookahead_sampled(sbr_env* env, int32_t n_steps, int32_t hold, int32_t fanout, const void* nominal,
                          const sbr_sampler* sampler, double* returns, double* rewards_out, int32_t* best_index,
                          double* best_return, void* actions_out, void* stream);

/* WHERE EACH BRANCH ENDED: sbr_lookahead_actions / sbr_lookahead_sampled that also report the end of every branch, for a
 * terminal value (the caller's critic on the end observation or state) added to the branch's return.  Every shared argument
 * follows the parent's contract word for word: returns, rewards_out, best_* and actions_out hold the parent's bits, NOTHING of
 * the handle is written, nothing is allocated (graph-capturable), the register budget goes by N*fanout.
 *   done_end    [B] uint8 or NULL: 1 if the branch's episode had ended on entry or ended during the launch, else 0
 *   obs_end     [B][SBR_NOBS] float32 or NULL: for a branch that is not done, the observation sbr_step returns for the branch's
 *               last call (the row sbr_rollout_policy leaves in obs); for a done branch SBR_NOBS zeros
 *   state_end   [B][SBR_NSTATE] float32 or NULL: likewise the state row of sbr_step; for a done branch SBR_NSTATE zeros
 * The three are float32 whatever cfg.out_f64 says (as the observation of sbr_rollout_policy is): the float32 rows of sbr_step
 * bit for bit, the float64 rows rounded once.  A done branch reports zeros because its plant stopped at the done call without
 * the terminal phases - a state no other entry point reports; mask a terminal value with done_end.
 * best_* are reduced from `returns` as they stand; for the winner of returns ADJUSTED by the caller use sbr_branch_best.
 * SBR_ERR_INVALID, before anything is touched: every refusal of the parent; obs_end, state_end and done_end all NULL (call the
 * parent); n_steps = 0 (there is no end state to report that the handle does not already hold). */
int sbr_lookahead_actions_end(sbr_env* env, int32_t n_steps, int32_t hold, int32_t fanout, const void* actions,
                              double* returns, double* rewards_out, int32_t* best_index, double* best_return, float* obs_end,
                              float* state_end, uint8_t* done_end, void* stream);
int sbr_lookahead_sampled_end(sbr_env* env, int32_t n_steps, int32_t hold, int32_t fanout, const void* nominal,
                              const sbr_sampler* sampler, double* returns, double* rewards_out, int32_t* best_index,
                              double* best_return, void* actions_out, float* obs_end, float* state_end, uint8_t* done_end,
                              void* stream);

/* the winner among each env's `fanout` values, under the rule of sbr_lookahead_actions' best_*, as a call of its own - for
 * returns the caller has adjusted (a terminal value added).
 *   values      [N*fanout] float64, DEVICE pointer
 *   best_index  [N] int32 or NULL, best_value [N] float64 or NULL
 * The largest value wins; NaN compares as -inf; ties go to the lowest k; best_value is the winner's entry as it stands.
 * Nothing of the handle is read but its size; nothing is allocated (graph-capturable).
 * SBR_ERR_INVALID, before anything is touched: NULL env or values; both outputs NULL; fanout < 1; N*fanout >= 2^31. */
int sbr_branch_best(sbr_env* env, int32_t fanout, const double* values, int32_t* best_index, double* best_value, void* stream);

/* the MPPI update of the nominal tape from the returns of sbr_lookahead_sampled (same nominal, sampler, fanout and rows).
 * Per env, over its `fanout` returns: key_k = returns[k] with NaN replaced by -inf; m = max key; if m is finite
 * w_k = exp((key_k - m) * inv), inv = 1.0 / temperature formed once on the host (a key of -inf gives w_k = 0), S = sum w_k and
 *   u[r][c] = (ActT)(sum_k w_k * (double)a(g, k, r, c) / S)      a: the sample above, drawn again - a convex combination
 * of the candidates, so inside [lo, hi].  If m is not finite (every return NaN or -inf, or one +inf) u[r] = nominal[r] bit for
 * bit and the weights are 0.  Output row r is u[min(r + shift, rows - 1)]: shift = 1 advances the tape by one decision and
 * repeats the last row (receding horizon).  The sums run in an order fixed by k alone, so an env's output depends on its
 * global id, its returns and the arguments - not on N, its position in the handle or the world size.
 *   nominal_out [rows][N][2] ActT, DEVICE pointer; MAY be the same pointer as nominal (any shift), not otherwise overlapping
 *   weights_out [N*fanout] float64 or NULL: w_k / S
 * Nothing of the handle is read but its size, id offset and action type; nothing is allocated (graph-capturable).
 * SBR_ERR_INVALID, before anything is touched: NULL env, sampler, nominal, returns or nominal_out; the sampler refusals
 * above; fanout < 1 or > 2^24; N*fanout >= 2^31; rows < 1; temperature not > 0, or temperature or 1/temperature not finite;
 * shift < 0. */
int sbr_mppi_update(sbr_env* env, int32_t rows, int32_t fanout, const void* nominal, const sbr_sampler* sampler,
                    const double* returns, double temperature, int32_t shift, void* nominal_out, double* weights_out,
                    void* stream);

/* fused rollout in CLOSED loop under the caller's policy: n_steps fused step() calls per env in ONE kernel, the action of a
 * decision call being a small MLP applied to the env's float32 observation, evaluated on the device next to the plant
 * (policy evaluation, evolution strategies and populations, collectors).
 *
 * The net maps the 18 observation values to 2 outputs through n_hidden hidden layers of `width` units.  One policy's
 * parameter block holds its layers in order, each as torch.nn.Linear stores it: W [out][in] row-major, then b [out]; `in`
 * is 18 for the first layer, `out` is 2 for the last, and sbr_policy_param_count() floats in all (38 without a hidden layer).
 * The width is exactly 32 or 64; a narrower net is zero-padded by the caller, which changes no bit: a padded unit is
 * act(0) = 0 and fma(0, h, acc) = acc.  Arithmetic: float32; every pre-activation is acc = b[j], then
 * acc = fmaf(W[j][k], h[k], acc) for k ascending; hidden units pass through tanhf or max(., 0); the two outputs y become
 * the action mean a = fmaf(act_scale, squash ? tanhf(y) : y, act_bias).  With noise_std != 0 the action is
 * (float)((double)a_k + noise_std_k * z_k), (z_0, z_1) one Box-Muller pair of Philox4x32-10 keyed by noise_seed, stream 3,
 * subsequence = GLOBAL env id, counter = the env's calls since reset.  The env clips the action afterwards, as always.
 *
 * A population: n_policies blocks back to back; the env with GLOBAL id g runs policy g / envs_per_policy (n_policies = 1:
 * every env runs the one policy and envs_per_policy is not read). */
typedef struct sbr_policy {
    const float* params;        /* DEVICE pointer, n_policies blocks of sbr_policy_param_count() floats */
    int32_t n_hidden;           /* 0, 1 or 2 hidden layers */
    int32_t width;              /* hidden width: 32 or 64 (ignored when n_hidden = 0) */
    int32_t activation;         /* hidden activation: 0 tanh, 1 relu */
    int32_t squash;             /* 0: a = bias + scale*y   1: a = bias + scale*tanh(y) */
    int64_t n_policies;         /* >= 1 */
    int64_t envs_per_policy;    /* env with GLOBAL id g runs policy g / envs_per_policy */
    float act_scale[2], act_bias[2];
    float noise_std[2];         /* 0, 0 = deterministic */
    uint64_t noise_seed;
} sbr_policy;
/* floats in one policy's parameter block; -1 for a shape sbr_rollout_policy refuses */
int64_t sbr_policy_param_count(int32_t n_hidden, int32_t width);
/*   obs         [N][18] float32, DEVICE pointer, in and out (whatever cfg.out_f64 says).  On entry the observation in force:
 *               what sbr_reset or sbr_step last returned for each env.  On exit the current observation of every env that
 *               is not done; a done env's row is left as it was (the post-terminal observation is sbr_step's business).
 *   hold        a decision is taken on the calls s of THIS launch with s % hold == 0 and held for `hold` calls
 *   returns     [N] float64 or NULL: sum of the rewards of this launch's calls, added in call order
 *   actions_out [ceil(n_steps / hold)][N][2] float32 or NULL: row s / hold is the decision of call s - exactly the value
 *               that is cast to double and integrated; 0 for a decision an env skipped because its episode had ended
 *   rewards_out [n_steps][N] float64 or NULL, as in sbr_rollout_actions
 * Semantics otherwise exactly sbr_rollout_actions': a finished env skips its remaining calls, the terminal phases run once
 * for the done call, SBR_C_PLAN reads 0 afterwards, no trace records, nothing allocated (graph-capturable); fed its own
 * actions_out as a tape, sbr_rollout_actions leaves the same bits.  n_steps = 0 touches nothing and writes returns = 0.
 * SBR_ERR_INVALID: NULL env, policy, params or obs; n_steps < 0; hold < 1; n_hidden outside 0..2; width other than 32 or 64
 * with n_hidden > 0; an unknown activation or squash; n_policies < 1; a negative or non-finite noise_std; with
 * n_policies > 1: envs_per_policy or the handle's first_env_id not a (positive) multiple of 256, or
 * first_env_id + N > n_policies * envs_per_policy. */
int sbr_rollout_policy(sbr_env* env, int32_t n_steps, int32_t hold, const sbr_policy* policy, float* obs, double* returns,
                       float* actions_out, double* rewards_out, void* stream);

/* sbr_rollout_policy as a COLLECTOR: the same launch, which also reports, for every decision, the observation it was taken on
 * and whether its transition is terminal - the (obs_d, action_d, reward_d, ended_d) a gradient-based learner needs.
 * Every argument shared with sbr_rollout_policy follows that contract word for word and yields THE SAME BITS: the handle's
 * plant and every controller row, obs on exit, returns, actions_out and rewards_out - for populations, noise and any hold;
 * done envs skip their calls, the terminal phases run once for the done call, SBR_C_PLAN reads 0 afterwards, nothing is
 * allocated (graph-capturable).  With rows = ceil(n_steps / hold), decision d taken on call s = d*hold of the launch:
 *   obs_out     [rows][N][SBR_NOBS] float32 or NULL: the 18 values the net was applied to at decision d, exactly the float32
 *               values the net's first layer reads.  Row 0 is the env's row of obs on entry.  For an env whose episode had ended
 *               before the decision: SBR_NOBS zeros (actions_out holds 0 there)
 *   flags_out   [rows][N] uint8 or NULL: SBR_DF_TAKEN - the decision was taken; SBR_DF_ENDED - the env's episode ended during
 *               one of this decision's calls (the transition is terminal).  So 0 (skipped), 1 or 3.  A short last decision
 *               (n_steps not a multiple of hold) is reported like any other
 * The action MEAN of a decision is a pure function of its obs_out row under the arithmetic fixed at sbr_policy, and is not
 * reported.  n_steps = 0 touches nothing, writes returns = 0 and leaves obs_out and flags_out unwritten.
 * SBR_ERR_INVALID, before anything is touched (the last failing check is reported): every refusal of sbr_rollout_policy;
 * obs_out and flags_out both NULL (call sbr_rollout_policy). */
#define SBR_DF_TAKEN 1
#define SBR_DF_ENDED 2
int sbr_collect_policy(sbr_env* env, int32_t n_steps, int32_t hold, const sbr_policy* policy, float* obs, double* returns,
                       float* actions_out, double* rewards_out, float* obs_out, uint8_t* flags_out, void* stream);

/* ---- Domain-randomised episodes of SBROS-v1: the handle's own envs as DIFFERENT PLANTS -------------------------------------------
 * A learner that has to survive a plant whose muA, bA or So_sat it does not know trains on many plants at once.  With a model
 * table on the handle (sbr_set_models above) the two calls below run every env under a model of that table - one launch, one obs_out,
 * one flags_out, global env ids and populations lined up as ever - where one handle per model would take a launch per model.
 * THE RULE.  The env with global id g (the handle's first_env_id + its index) is plant (g / envs_per_model) % n_models.  It is keyed
 * by the global id: it does not depend on N, on the shard or on the world size.  envs_per_model is an argument of each call and no
 * state of the handle.  These two calls apply the rule and no others: sbr_reset, sbr_step, sbr_rollout*, sbr_collect_policy, every
 * lookahead but the two *_models forms further down (which play every env under every model) and the trace export keep integrating
 * the handle's own config, with the bits they return without a table.
 * CONDITIONS, checked before anything is touched (the last failing check is reported): a table is set (n_models >= 1); with
 * n_models > 1, envs_per_model is a positive multiple of 256 and the handle's first_env_id a non-negative multiple of 256, so that a
 * wavefront never holds two plants (a model's constants are wave-uniform scalar loads, as the handle's own are); with one model
 * envs_per_model is not read.
 * WHAT IS COMPUTED.  Every output bit - the plant, every controller row, the stored influent, and every buffer of the call - is what a
 * second handle CREATED WITH THAT MODEL's config and the same first_env_id leaves for the same inputs through the parent call
 * (sbr_reset / sbr_reset_carry; sbr_collect_policy or sbr_rollout_policy).  The table may be replaced between two launches
 * (sbr_set_models waits for the device); nothing is allocated by either call (graph-capturable). */

/* sbr_reset (carry_over = 0) / sbr_reset_carry (carry_over != 0) with the fill phase, the SBR_ST_* bits and the observation under
 * each env's own model.  Everything else is the parent's: the influent draw keyed by seed and global id (it reads nothing of the
 * plant), scenario, rnd, an explicit influent, mask, and obs in either output dtype.
 * SBR_ERR_INVALID: NULL env; the conditions above; no influent given and sbr_set_influent_tables never called. */
int sbr_reset_models(sbr_env* env, int64_t envs_per_model, int32_t carry_over, uint64_t seed, const int32_t* scenario,
                     const double* rnd, const double* influent, const uint8_t* mask, void* obs, void* stream);

/* sbr_collect_policy's loop with every constant read from the env's model: the control intervals, the reward, the SBR_ST_*
 * thresholds, the step plan of cfg.scheme = 1 and the terminal phases.  Arguments, layouts and semantics are sbr_collect_policy's
 * word for word, with one difference: obs_out and flags_out may BOTH be NULL - the call is then the models form of
 * sbr_rollout_policy, and leaves its bits.  A population (policy->n_policies > 1) and a model table vary independently: the policy
 * of an env is block g / envs_per_policy, its plant (g / envs_per_model) % n_models.
 * SBR_ERR_INVALID, before anything is touched (the last failing check is reported): every refusal of sbr_rollout_policy; the
 * conditions above. */
int sbr_collect_policy_models(sbr_env* env, int64_t envs_per_model, int32_t n_steps, int32_t hold, const sbr_policy* policy,
                              float* obs, double* returns, float* actions_out, double* rewards_out, float* obs_out,
                              uint8_t* flags_out, void* stream);

/* ---- the step-level lookahead under UNCERTAIN PLANT KINETICS: K tapes x M models -------------------------------------------------
 * sbr_lookahead_actions / sbr_lookahead_sampled integrate the handle's own plant.  The two calls below play every candidate tape of
 * every env under EVERY model of the handle's table (sbr_set_models above; M = sbr_num_models(env)) in one launch, and reduce
 * mean / worst / winner on the device: "which tape is good if muA, bA or So_sat is not what I think?" without a handle, a copy of
 * the live state and a launch per model.  (The rule of the two calls above - a plant per env - is NOT applied here: every env
 * meets every model.)
 * A BRANCH is (env i, candidate k, model m), j = (i*fanout + k)*M + m; there are B = N*fanout*M < 2^31 of them.  Branch (i, k, m)
 * plays candidate k of env i from env i's CURRENT plant and controller record under the constants of model m: intervals, reward,
 * SBR_ST_* thresholds, the step plan of cfg.scheme = 1.  The handle's own config is integrated by NO branch: a caller who wants
 * the nominal plant among the models puts the handle's config into the table.
 *   actions     [ceil(n_steps / hold)][N*fanout][2] ActT, nominal [ceil(n_steps / hold)][N][2] ActT: exactly the parents' inputs,
 *               not expanded over m
 *   returns     [B] float64 or NULL: the per-branch sum of the launch's rewards, added in call order
 *   rewards_out [n_steps][B] float64 or NULL: the reward of every call, 0.0 for a call a finished branch skipped.  A STRIDED
 *               store: the lanes of a wavefront hold neighbouring (i, k) of one m, so each call writes 64 doubles M apart - ask
 *               for it when the per-call rewards are needed, not by default
 *   mean_out, worst_out [N*fanout] float64 or NULL: over a candidate's M returns - the rule of sbr_cycle_lookahead_scenarios:
 *               summed in m order and divided once; the smallest return; NaN if one of them is.  Reduced FROM `returns`, which
 *               must be given with them
 *   best_index  [N] int32 or NULL, best_value [N] float64 or NULL: the winner among an env's `fanout` MEANS under
 *               sbr_lookahead_actions' rule; reduced FROM mean_out, which must be given with them
 *   actions_out [ceil(n_steps / hold)][N*fanout][2] ActT or NULL (sampled call): the candidates as integrated.  A candidate is
 *               a(g, k, r, c) - keyed by (seed, global env id, k, row) and NOT by m: all models of a candidate play the SAME
 *               tape (common random numbers), so that two models differ by the plant and not by what they drew.  Stored once,
 *               by the branches of model 0
 * THE CONTRACT.  returns[i][k][m] and rewards_out[.][i][k][m] carry the bits sbr_lookahead_actions gives for candidate k of env
 * i on a second handle CREATED WITH MODEL m's config and the same first_env_id that holds env i's state (sbr_get_state /
 * sbr_set_state); the sampled call likewise the bits of sbr_lookahead_sampled on such a handle.  With the handle's own config at
 * table index m, column m holds the bits of the parent call on the handle itself.  Fed its own actions_out,
 * sbr_lookahead_actions_models returns the bits of sbr_lookahead_sampled_models.
 * In every other respect the calls are their parents: rows held `hold` calls and launch-relative, a done branch skips its
 * remaining calls, no terminal phases, the end-of-cycle reward of reward_kind 2 inside the done call.  NOTHING of the handle is
 * written, nothing is allocated (graph-capturable).  The models are the y axis of the launch grid, so that a model stays uniform
 * across a wavefront and is read with scalar loads; the register budget of the launch goes by B.
 * n_steps = 0 writes returns = mean_out = worst_out = 0, best_index = 0 and best_value = 0 and reads nothing of the state, the
 * tape or the table.
 * NOT HERE: _end forms (where each branch ended), a policy lookahead over models, sbr_step under a model.
 * SBR_ERR_INVALID, before anything is touched (the last failing check is reported): every refusal of the parent but the one
 * about best_* (here: best_index or best_value given while mean_out is NULL); no model table set; more than 65535 models;
 * N*fanout*M >= 2^31; mean_out or worst_out given while returns is NULL. */
int sbr_lookahead_actions_models(sbr_env* env, int32_t n_steps, int32_t hold, int32_t fanout, const void* actions,
                                 double* returns, double* rewards_out, double* mean_out, double* worst_out,
                                 int32_t* best_index, double* best_value, void* stream);
int sbr_lookahead_sampled_models(sbr_env* env, int32_t n_steps, int32_t hold, int32_t fanout, const void* nominal,
                                 const sbr_sampler* sampler, double* returns, double* rewards_out, double* mean_out,
                                 double* worst_out, int32_t* best_index, double* best_value, void* actions_out, void* stream);

/* CLOSED-LOOP lookahead: `fanout` rollouts of the caller's policy per env, each from the env's CURRENT state and observation, the
 * handle left bit for bit as it was (Monte-Carlo value and advantage estimates at the states the learner visits, policy-guided
 * MPC, n-step returns plus a critic on obs_end).  sbr_rollout_policy in the read-only, K-branches-per-env form of
 * sbr_lookahead_actions.
 * A BRANCH is j = i*fanout + k: env i, branch k; there are B = N*fanout < 2^31 of them.  Branch j starts from env i's plant and
 * controller record as they are - also in the form sbr_step leaves them - and from env i's row of obs, and runs exactly the
 * calls sbr_rollout_policy would run on an env in that state under that policy: a decision on the calls s of this launch with
 * s % hold == 0, the same float32 arithmetic of the net, the same clipping.  Without noise every branch of an env returns the
 * bits sbr_rollout_policy returns for a copy of the env; fed this call's actions_out, sbr_lookahead_actions(_end) returns the
 * same bits in returns, rewards_out, best_* and the end outputs.
 *   policy      as in sbr_rollout_policy.  A population: the policy of a branch is its ENV's, global id g / envs_per_policy.
 *               With n_policies > 1 the conditions of sbr_rollout_policy apply unchanged (envs_per_policy and the handle's
 *               first_env_id multiples of 256) and are enough for any fanout: a policy boundary then falls at a branch index
 *               (multiple of 256)*fanout, so no workgroup of 256 branches straddles two policies.
 *   noise       with noise_std != 0 the noise of branch k is the Box-Muller pair of the Philox4x32-10 block keyed by noise_seed
 *               with counter = (the BRANCH's calls since reset, 3 + 256*k, g_lo, g_hi): sbr_rollout_policy's construction with
 *               k in the upper 24 bits of the stream word (as the sampler carries its candidate in stream 4), hence
 *               fanout <= 2^24.  Branch 0 draws exactly what sbr_rollout_policy would draw next for that env.  The noise
 *               depends on (noise_seed, g, k, call count) and on nothing else: not on N, fanout or the shard.
 *   keep_mean   1: branch 0 of every env runs WITHOUT noise - the policy's mean action, the closed-loop counterpart of the
 *               sampler's keep_nominal; the other branches are unchanged.  0 or 1.
 *   obs         [N][18] float32, DEVICE pointer, const: the observation in force of every env (what sbr_reset, sbr_step or
 *               sbr_rollout_policy last left for it), shared by the env's branches and NOT written
 *   returns     [B] float64 or NULL: sum of the launch's rewards of the branch, added in call order
 *   rewards_out [n_steps][B] float64 or NULL: the reward of every call; 0.0 for a call the branch skipped
 *   best_index  [N] int32 or NULL, best_return [N] float64 or NULL: the winner among each env's returns under the rule of
 *               sbr_lookahead_actions, reduced FROM `returns` by a second kernel on the same stream: give returns with them
 *   actions_out [ceil(n_steps / hold)][B][2] float32 or NULL: row s / hold is the decision of call s, exactly the value that is
 *               cast to double and integrated; 0 for a decision a branch skipped because its episode had ended
 *   obs_end     [B][SBR_NOBS] float32, state_end [B][SBR_NSTATE] float32, done_end [B] uint8, each or NULL: where the branch
 *               ended, under the words of sbr_lookahead_actions_end - float32 whatever cfg.out_f64 says, zeros for a done branch
 * NOTHING of the handle is written and obs is not written; nothing is allocated (graph-capturable).  No terminal phases run
 * (they change only state that is discarded here); the end-of-cycle reward of reward_kind 2 is part of the done call and is
 * included.  The register budget of the launch goes by B, not by N.  n_steps = 0 writes returns = 0, best_index = 0 and
 * best_return = 0 and reads nothing.
 * SBR_ERR_INVALID, before anything is touched (the last failing check is reported): every policy refusal of
 * sbr_rollout_policy; NULL env, policy or obs; n_steps < 0; hold < 1; fanout < 1 or > 2^24; N*fanout >= 2^31; keep_mean other
 * than 0 or 1; best_index or best_return given while returns is NULL; obs_end, state_end or done_end given with n_steps = 0. */
int sbr_lookahead_policy(sbr_env* env, int32_t n_steps, int32_t hold, int32_t fanout, const sbr_policy* policy,
                         int32_t keep_mean, const float* obs, double* returns, double* rewards_out,
                         int32_t* best_index, double* best_return, float* actions_out,
                         float* obs_end, float* state_end, uint8_t* done_end, void* stream);

/* batch statistics of a per-env float64 vector (e.g. episode returns): wavefront reductions
 * + one atomic per wave.  out4 = {sum, min, max, count} float64, DEVICE pointer. */
int sbr_reduce_stats(sbr_env* env, const double* values, int64_t n, double* out4, void* stream);

/* parity injection / inspection: x is [SBR_NX][N], ctrl is [SBR_NCTRL][N], float64, DEVICE pointers.
 * An injected volume x[0] is taken as it is.  The dosing integrator expands 1/(V/V0) to third order in Q t_delta / V0
 * (sbr_create checks EC_max t_delta <= 1e-4 min(IV, WV), i.e. <= 7e-7 for the reference plant): a state injected with a
 * volume below ~1 % of IV would carry a truncation (Q t_delta / V0)^4 above 1e-16 into its dosing intervals. */
int sbr_get_state(sbr_env* env, double* x, double* ctrl, void* stream);
int sbr_set_state(sbr_env* env, const double* x, const double* ctrl, void* stream);

/* one row of the ctrl block (SBR_C_* index), e.g. SBR_C_RETURN for the episode returns: out is [N] float64, DEVICE
 * pointer; asynchronous on `stream`, no host synchronisation (sbr_get_state translates all SBR_NCTRL rows). */
int sbr_get_ctrl_row(sbr_env* env, int32_t row, double* out, void* stream);

/* the flow-weighted influent each env was reset with (buffer_tank3.py:87-107; entry 0 = Qin/T_fill,
 * gym_SBR_oneshot.py:287): out is [SBR_NX][N] float64, DEVICE pointer. */
int sbr_get_influent(sbr_env* env, double* out, void* stream);

/* standalone right-hand sides for known-answer tests (gym_SBR_oneshot.py:1658-1787, :1424-1583,
 * :2424-2552).  x [n][14], kla [n], ec [n], loading [n][14] or NULL, dx [n][14]; DEVICE pointers.
 * kind: 0 reaction, 1 filling (needs loading), 2 idle. */
int sbr_eval_rhs(sbr_env* env, int32_t kind, int64_t n, const double* x, const double* kla, const double* ec,
                 const double* loading, double* dx, void* stream);

/* Dense output of one integration span, for trajectory export: the reference returns odeint's solution on an output grid
 * of its own - linspace(t, t + t_delta, int(t_delta/dt)) = 9 or 10 points per control interval, 252 points over the fill
 * phase, 463 over the idle phase - and appends those rows to t_t / x_t / So_t ... (gym_SBR_oneshot.py:296-313, :1339, :1369,
 * :1959-1961, :1122-1155); a fixed-step integrator has its own nodes instead.  For n independent spans given by start state
 * x0 [n][14], the held Kla [n] and the substep length h [n] (days), this writes the n_sub + 1 RK4 nodes xs [n][n_sub + 1][14]
 * (node 0 = the start state; with n_sub = cfg.substeps and h = span/n_sub the last node is the state sbr_step ends the
 * interval in, to rounding) and the right-hand side at every node dxs [n][n_sub + 1][14]: values and slopes for cubic-Hermite
 * interpolation onto any grid.  kind 0: a control interval (reaction_dxdt :1658-1787, ec [n] held); 1: the fill phase
 * (filling_dxdt :1424-1583, loading [n][14] with loading[0] = the inflow); 2: the idle phase (idle_dxdt :2424-2552); 3: settle
 * and draw (Sim_Settling_Drawing :2264-2420) applied to x0 first, then the idle phase - node 0 is the reactor after the draw.
 * ec may be NULL unless kind == 0, loading unless kind == 1.  DEVICE pointers.  Not on the stepping path.
 * The nodes are RK4's under EITHER cfg.scheme.  Under cfg.scheme = 0 they are the states sbr_step itself passed through (the last
 * node equals its end state to 1e-12).  Under cfg.scheme = 1 sbr_step integrated the interval with adaptive Butcher-5 steps: the
 * replayed rows are then another discretisation of the same interval from the same start state - inside the parity gate of the
 * reference's rows like the stepped states, but their last node differs from the state sbr_step returned by the two schemes'
 * distance (~1e-2 of the gate; up to 2e-5 relative after the idle phase).  A consumer that needs rows ending exactly on the
 * stepped states pins the last row to the record (gym_sbr2_amd's trajectory(dense=True) does) or runs cfg.scheme = 0. */
int sbr_eval_substeps(sbr_env* env, int32_t kind, int64_t n, int32_t n_sub, const double* x0, const double* kla, const double* ec,
                      const double* loading, const double* h, double* xs, double* dxs, void* stream);

/* device-side normal draws used by sbr_reset when rnd == NULL, exposed for tests: out [N][48]. */
int sbr_draw_normals(sbr_env* env, uint64_t seed, double* out, void* stream);

/* the scenario each env gets from sbr_reset(seed, scenario = NULL) when cfg.random_scenario = 1: out [N] int32, DEVICE
 * pointer (replaces np.random.choice(8, 1), gym_SBR_env4.py:107). */
int sbr_draw_scenarios(sbr_env* env, uint64_t seed, int32_t* out, void* stream);

/* influent FUTURES without a reset: `rows` x `per_env` draws of the reset's influent mix per env (scenario tables + 48 normals,
 * buffer_tank3.py:68-107), nothing of the handle written, nothing allocated (graph-capturable).
 *   out      [rows][N][per_env][SBR_NX] float64, DEVICE pointer.  A row of 14 is what sbr_cycle_reset takes as one env's `influent`
 *            and what sbr_get_influent returns for it: entries 1..13 the flow-weighted means, entry 0 the 0.66 of
 *            buffer_tank3.py:107 (no consumer reads it).  out[c] is one cycle's `influent` of sbr_cycle_lookahead_scenarios with
 *            n_scen = per_env.
 *   draw (r, i, s) has index d = first_draw + r*per_env + s.  Its 48 normals are the Box-Muller pairs of Philox4x32-10 under key
 *            `seed` at counters (pair 0..23, 0 + 256*d, g_lo, g_hi), g the GLOBAL env id: the draw index in the upper 24 bits of
 *            the stream word.  d = 0 is exactly the draw of sbr_reset / sbr_cycle_reset(seed, rnd = NULL).  A draw depends on
 *            (seed, g, d, scenario) and on nothing else - not on N, rows, per_env or the shard.
 *   scenario [N] int32 or NULL, shared by an env's draws.  NULL with cfg.random_scenario = 1: draw d takes Philox block
 *            (0, 2 + 256*d, g_lo, g_hi) under `seed` (d = 0: sbr_draw_scenarios' value).  NULL with cfg.random_scenario = 0 is
 *            refused: sbr_reset and sbr_cycle_reset fix different scenarios, so the caller names one.
 * SBR_ERR_INVALID, before anything is touched (the last failing check is reported): NULL env or out; rows < 1 or per_env < 1;
 * first_draw < 0; first_draw + rows*per_env > 2^24; N*rows*per_env >= 2^31; sbr_set_influent_tables never called; NULL scenario
 * without cfg.random_scenario. */
int sbr_draw_influent(sbr_env* env, uint64_t seed, int32_t rows, int32_t per_env, int32_t first_draw,
                      const int32_t* scenario, double* out, void* stream);

/* Block the calling host thread until everything queued on `stream` has finished (hipStreamSynchronize on the handle's
 * device).  For host-driven callers: the reference's step() returns finished numbers, so the reference-shaped single env
 * reads its pinned-host outputs after sbr_step + sbr_synchronize - two C calls per step, no other runtime binding needed. */
int sbr_synchronize(sbr_env* env, void* stream);

/* timing helper for bench.py: average device time (ms) per sbr_step launch between two marks,
 * measured with HIP events on `stream` (the stream the kernels are launched on). */
int sbr_timer_start(sbr_env* env, void* stream);
int sbr_timer_stop(sbr_env* env, void* stream, float* elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* SBR_AMD_H */
