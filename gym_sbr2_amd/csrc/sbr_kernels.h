// sbr_kernels.h - what more than one kernel family of libsbr_amd.so uses on the device: the handle's buffers and their
// addressing, the write-through stores, the internal controller record and its codec, the action-pair load of the tape
// kernels and the end-of-branch rows of the lookaheads.  Templates, SBR_DEV functions, types and macros only: a kernel lives
// in the one translation unit whose entry points launch it ("Source layout").
#pragma once
#include <hip/hip_runtime.h>

#define SBR_BLOCK 256     // threads per workgroup of the stepping kernels: four waves, one per SIMD.  Measured at N = 65536
                          // (round 1): 64 -> 23.0 us, 128 -> 22.8, 256 -> 22.65 per k_step launch (fewer workgroups to dispatch)
#include "sbr_device.h"

#define SBR_RESET_BLOCK 256     // k_reset stages 84 KiB of tables in LDS: one block per CU, so make it four waves

// ------------------------------------------------------------------------------------------- state I/O
struct SbrBuf {
    double* trace;  // [capacity][SBR_NTRACE][n_trace] or NULL
    int64_t n_trace, trace_cap;
    double* x;      // [14][N]
    double* ctrl;   // [R_NROWS][N]
    double* infl;   // [14][N]
    int64_t n;
    int64_t first_env_id;
#ifdef SBR_STAMPS
    unsigned long long* stamps;   // diagnostic build only (scripts/probes/step_timeline.py): [waves][16] s_memrealtime ticks
#endif
};
// Diagnostic build -DSBR_STAMPS: lane 0 of every wave records the 100 MHz real-time counter at up to sixteen points of k_step.
// The stamps go to a buffer of their own that nothing else reads; the product build contains none of this.
#ifdef SBR_STAMPS
#define SBR_STAMP(k, drain)                                                                                   \
    do {                                                                                                      \
        if (drain) __builtin_amdgcn_s_waitcnt(0);                                                             \
        if (b.stamps != nullptr && (l & 63u) == 0u)                                                           \
            b.stamps[(uint64_t)((i0 + l) >> 6) * 16 + (k)] = __builtin_amdgcn_s_memrealtime();               \
    } while (0)
#else
#define SBR_STAMP(k, drain) do { } while (0)
#endif

// The stepping kernels' stores leave the CU as agent-scope write-through (sc1).  Plain stores leave ~21 MB dirty in the L2s
// for the end-of-kernel write-back, which then sits between two dependent launches; written through, the bytes drain while
// other waves still compute.  Measured per k_step launch (profiles/r02_notes.md): 65536 envs 16.06 -> 15.5 us, 131072 envs
// 28.6 -> 23.1 us; non-temporal (nt) stores gain half of that at 65536 and nothing at 131072; sc0 sc1 equals sc1.
template <typename T>
SBR_DEV void st_out(T* p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
typedef unsigned int sbr_u32x4 __attribute__((ext_vector_type(4)));
// The output staging of k_step reuses the wave's LDS parking region (declared double[]) for rows of OutT and reads it back as
// 16-byte chunks: accesses through these may_alias types are visible to alias analysis (round 4 saw the float32
// staging stores hoisted over the parked double loads).  The compiler barriers at the call sites stay as defence in depth.
typedef sbr_u32x4 __attribute__((may_alias)) sbr_u32x4_alias;
typedef float __attribute__((may_alias)) sbr_f32_alias;
typedef double __attribute__((may_alias)) sbr_f64_alias;
template <typename T> struct SbrAliasOf;
template <> struct SbrAliasOf<float> { using type = sbr_f32_alias; };
template <> struct SbrAliasOf<double> { using type = sbr_f64_alias; };
// The sc1 modifier has no builtin for a 16-byte store, hence inline assembly - and inline assembly is invisible to the
// compiler's hazard recognizer: on gfx940+ a VMEM store of more than 64 bits reads its data registers for two more cycles, and a
// VALU instruction that overwrites them inside that window corrupts the stored value (seen in round 4, once the stores were
// issued back to back: the 64-bit address of the NEXT store was formed in the low half of the data registers of the previous
// one).  The s_nop supplies the two wait states the compiler would have inserted for a store it knows.
SBR_DEV void st_out16(sbr_u32x4* p, sbr_u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v) : "memory");
}

// Addressing.  An env is (i0, l): i0 = first env of the workgroup (wave-uniform, lives in SGPRs), l = threadIdx.x.  Every
// access is written as (uniform pointer advanced to row and workgroup)[l], so the row arithmetic runs on the scalar unit
// and the lane contributes one 32-bit offset (global_load v, v_off, s[base:base+1]).  The first version formed a 64-bit
// address per lane and row: 173 VALU instructions and ~60 VGPRs of k_step.
#define XROW(j) (b.x + ((int64_t)(j) * b.n + i0))[l]
#define CTRL(f) (b.ctrl + ((int64_t)(f) * b.n + i0))[l]
#define INFL(j) (b.infl + ((int64_t)(j) * b.n + i0))[l]

SBR_DEV void load_x(const SbrBuf& b, int64_t i0, uint32_t l, double (&x)[SBR_NX]) {
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) x[j] = XROW(j);
}
SBR_DEV void store_x(const SbrBuf& b, int64_t i0, uint32_t l, const double (&x)[SBR_NX]) {
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) st_out(&XROW(j), x[j]);
}
// INTERNAL controller layout [R_NROWS][N] (the public one of sbr_amd.h is produced by k_export / consumed by k_import):
//  * the Kla history is a RING: the value of the j-th interval since reset sits in slot (j-1) % 10, where the interval
//    count k is recovered from the running time, k = round((t - T_fill)/t_delta); a step writes ONE slot, not ten, and
//    (round 4) READS three: next to the ring the handle keeps Kla[-1] and the sum of the eight entries before it, from which
//    the reward's window follows incrementally (SbrHistInc in sbr_device.h);
//  * steps, plan, two flags, status bits and the done flag share one row (SbrMeta);
//  * So[-1] and Sno[-1] are IMPLICIT after an ordinary step (round 4): every interval ends with So.append(x_out[-1][8]),
//    Sno.append(x_out[-1][9]) (:1955-1956, :2043-2044), so after a step the two values ARE x[8] and x[9] and k_step neither
//    stores nor loads their rows (meta's m1i bit says so).  Whoever writes values that are NOT the plant's - the reset (Ss in
//    the Sno memory, :1652), an import, a rollout, the done call (the terminal phases move x afterwards) - stores the rows and
//    leaves the bit clear; the next step then fetches them in a second, dependent load (once per episode);
//  * rows only read when tauD != 0 (So[-2], Sno[-2]), only at the end of an episode (Qw) or only by the operating-cost
//    reward (the running sum of Kla) come last.
// Per env-step the step kernel reads 11 controller rows (t, two integrals, EC[-1], return, meta, Kla[-1], w8, three ring
// slots) and writes 11 (those minus the three slots, plus So[-2], Sno[-2] and one ring slot): 176 B, where the public layout
// would take 20 + 24 rows (352 B) and rounds 2-3 took 18 + 11 (232 B).
enum { R_T = 0, R_SO_M1, R_SNO_M1, R_IE_DO, R_IE_EC, R_EC_LAST, R_RET, R_META, R_KLA_LAST, R_W8, R_RING0,
       R_SO_M2 = R_RING0 + SBR_KLA_HIST, R_SNO_M2, R_QW, R_KSUM, R_NROWS };
#define SBR_MAX_STEPS ((1 << 17) - 1)

// The R_META row: an integer < 2^31 held in a double,
//   meta = steps*16384 + plan*64 + m1i*32 + idle*16 + status*2 + done.
// `steps`: calls of the episode, saturating at SBR_MAX_STEPS.  `plan`: what cfg.scheme = 1 did in the last control interval
// k_step ran for this env (step count + 128 if dissolved oxygen was held; 0 = none reported: scheme 0, a reset, a rollout) -
// SBR_C_PLAN of the public layout; it rides in this row so that reporting it moves no extra byte.  `idle`: the done call of
// k_step appended one more Kla than t accounts for (Sim_idle's, :2578): the ring's oldest entry then sits one slot further than
// ring_k(t) says.  `m1i`: So[-1], Sno[-1] are x[8], x[9] and their rows are stale (set by an ordinary k_step call only).
// `status`: the sticky SBR_ST_* bits.  `done`: the episode has ended; step() leaves the env alone until a reset.
struct SbrMeta {
    int steps = 0, status = 0;
    bool done = false, idle = false, m1i = false;
    int plan = 0;
    __host__ __device__ static constexpr double pack(SbrMeta m) {
        return (double)((m.steps << kStepsShift) + ((m.plan & 0xff) << kPlanShift) + (m.m1i ? kM1i : 0) + (m.idle ? kIdle : 0) +
                        m.status * 2 + (m.done ? kDone : 0));
    }
    static constexpr int kDone = 1, kIdle = 16, kM1i = 32, kPlanShift = 6, kStepsShift = 14;
    SBR_DEV static SbrMeta unpack(double m) {
        const int v = (int)m;
        SbrMeta r;
        r.done = (v & kDone) != 0; r.status = (v >> 1) & 7; r.idle = (v & kIdle) != 0; r.m1i = (v & kM1i) != 0;
        r.plan = (v >> kPlanShift) & 0xff; r.steps = v >> kStepsShift;
        return r;
    }
    SBR_DEV static int next_steps(int steps) { return steps < SBR_MAX_STEPS ? steps + 1 : steps; }
};

SBR_DEV int ring_k(const SbrPar& p, double t) {             // intervals since reset, from the running time
    double q = __builtin_fma(t - p.T_fill, p.inv_t_delta, 0.5);
    if (!(q >= 0.0)) q = 0.0;                                // also catches NaN
    if (q > 2e9) q = 2e9;
    return (int)q;
}
SBR_DEV int ring_wrap(int s) { return s >= SBR_KLA_HIST ? s - SBR_KLA_HIST : s; }       // for 0 <= s < 20
// the two rows k_step keeps next to the ring (SbrHistInc), from a history in logical order (oldest first, hist[9] = Kla[-1])
SBR_DEV double hist_w8(const double (&hist)[SBR_KLA_HIST]) {
    double s = hist[1];
#pragma unroll
    for (int j = 2; j <= 8; ++j) s = s + hist[j];
    return s;
}

// the rows every step rewrites; with_m1 = false leaves So[-1] and Sno[-1] implicit (the caller then sets meta's m1i bit)
SBR_DEV void store_ctl(const SbrBuf& b, int64_t i0, uint32_t l, const SbrCtl& c, bool with_m1 = true) {
    st_out(&CTRL(R_T), c.t); st_out(&CTRL(R_SO_M2), c.so_m2); st_out(&CTRL(R_SNO_M2), c.sno_m2);
    if (with_m1) { st_out(&CTRL(R_SO_M1), c.so_m1); st_out(&CTRL(R_SNO_M1), c.sno_m1); }
    st_out(&CTRL(R_IE_DO), c.ie_do); st_out(&CTRL(R_IE_EC), c.ie_ec); st_out(&CTRL(R_EC_LAST), c.ec_last);
}

// An env's whole controller record.  k_step keeps its own sequence (one memory round trip, implicit m1 rows, ring appends);
// every other kernel that reads or writes the record goes through load_record / store_record.  KSUM: whether the running sum
// of Kla is read / written (only the operating-cost reward maintains it).
struct SbrRecord {
    SbrCtl c;                      // t, the two PIDs' memories and integrals, EC[-1], Kla[-1]; the per-call fields cleared
    double hist[SBR_KLA_HIST];     // the Kla history in logical order (oldest first)
    double ret, qw, ksum;
    SbrMeta meta;
};
// The general form: So[-1] / Sno[-1] are the plant's x[8] / x[9] when meta's m1i bit says so, the ring's oldest entry sits at
// ring_k(t) + idle.  Kla[-1] is taken from the ring, not from R_KLA_LAST.
template <bool KSUM>
SBR_DEV void load_record(const SbrPar& p, const SbrBuf& b, int64_t i0, uint32_t l, double x8, double x9, SbrRecord& r) {
    SbrCtl& c = r.c;
    r.meta = SbrMeta::unpack(CTRL(R_META));
    c.t = CTRL(R_T);
    c.so_m1 = x8; c.sno_m1 = x9;
    if (!r.meta.m1i) { c.so_m1 = CTRL(R_SO_M1); c.sno_m1 = CTRL(R_SNO_M1); }
    c.ie_do = CTRL(R_IE_DO); c.ie_ec = CTRL(R_IE_EC); c.ec_last = CTRL(R_EC_LAST);
    c.so_m2 = CTRL(R_SO_M2); c.sno_m2 = CTRL(R_SNO_M2);
    c.ec_prev = c.ec_last; c.u_do = 0.0; c.u_ec = 0.0;
    c.n_new = 0; c.st_new = 0; c.span = 0.0; c.rows = 9; c.plans = 0;
    const int kb = (ring_k(p, c.t) + (r.meta.idle ? 1 : 0)) % SBR_KLA_HIST;
#pragma unroll
    for (int j = 0; j < SBR_KLA_HIST; ++j) r.hist[j] = CTRL(R_RING0 + ring_wrap(kb + j));
    c.kla_last = r.hist[SBR_KLA_HIST - 1];
    r.ret = CTRL(R_RET); r.qw = CTRL(R_QW); r.ksum = KSUM ? CTRL(R_KSUM) : 0.0;
}
// The explicit form, which every writer but k_step leaves: So[-1] / Sno[-1] in their rows, m1i and idle clear, the ring in
// plain order for ring_k(t), R_KLA_LAST / R_W8 derived from it.  The eight rows of store_ctl go out written through, the rest
// plainly.
template <bool KSUM>
SBR_DEV void store_record(const SbrPar& p, const SbrBuf& b, int64_t i0, uint32_t l, const SbrRecord& r) {
    store_ctl(b, i0, l, r.c);
    const int kb = ring_k(p, r.c.t) % SBR_KLA_HIST;
#pragma unroll
    for (int j = 0; j < SBR_KLA_HIST; ++j) CTRL(R_RING0 + ring_wrap(kb + j)) = r.hist[j];
    CTRL(R_KLA_LAST) = r.hist[SBR_KLA_HIST - 1]; CTRL(R_W8) = hist_w8(r.hist);
    CTRL(R_RET) = r.ret; CTRL(R_META) = SbrMeta::pack({r.meta.steps, r.meta.status, r.meta.done, false, false, r.meta.plan});
    CTRL(R_QW) = r.qw;
    if (KSUM) CTRL(R_KSUM) = r.ksum;
}

// A plant model of the handle's table (sbr_set_models) as the kernels that integrate it hold it: a byte pointer in the constant
// address space, so that every constant read through it is a scalar load (k_cycle_lookahead_models, k_models_collect_policy,
// k_reset_models).
typedef const __attribute__((address_space(4))) char* SbrConstBytes;
// The model of the WAVE that holds the env with global id gid, under the rule of sbr_reset_models / sbr_collect_policy_models:
// model (gid / envs_per_model) % n_models.  The host has checked that envs_per_model and the handle's first env id are multiples
// of 256 where the table holds more than one model, so a wave never holds two; the readfirstlane makes the index - and with it
// the address - a scalar.  With one model envs_per_model is not read.
SBR_DEV SbrConstBytes sbr_wave_model(const SbrPar* __restrict__ table, uint32_t n_models, int64_t envs_per_model, uint64_t gid) {
    uint32_t m = 0;
    if (n_models > 1) m = __builtin_amdgcn_readfirstlane((uint32_t)((gid / (uint64_t)envs_per_model) % n_models));
    return (SbrConstBytes)(table + m);
}

// A lane's pair of a row as one load (global_load_dwordx2 / dwordx4; the tape only has to be aligned like its elements).  The
// compiler barrier behind it keeps the load where it is written: without it the compiler sank the fetch of the next row to the
// end of the call, behind the integration it is meant to overlap, and its whole latency came back in front of the next call's
// first PID.  (A volatile load stays in place too, but the backend waits for it on the spot: s_waitcnt vmcnt(0) behind the load.)
typedef float __attribute__((ext_vector_type(2), aligned(4), may_alias)) sbr_act2_f32;
typedef double __attribute__((ext_vector_type(2), aligned(8), may_alias)) sbr_act2_f64;
template <typename T> struct SbrAct2;
template <> struct SbrAct2<float> { using type = sbr_act2_f32; };
template <> struct SbrAct2<double> { using type = sbr_act2_f64; };
template <typename ActT>
SBR_DEV void tape_load(const ActT* row /* the workgroup's part of a row */, uint32_t l, ActT& a0, ActT& a1) {
    const typename SbrAct2<ActT>::type v = *reinterpret_cast<const typename SbrAct2<ActT>::type*>(row + 2 * l);
    asm volatile("" ::: "memory");
    a0 = v.x; a1 = v.y;
}

// The per-cycle lookaheads (sbr_cycle_lookahead.hip, sbr_cycle_scenarios.hip).  A lane's three set-points of a row (a wave's 64
// triples are contiguous where its lanes' rows are: 768 or 1536 bytes).  The compiler barrier keeps the loads where they are
// written, as in tape_load.
template <typename ActT>
SBR_DEV void cycle_row_load(const ActT* row /* the workgroup's part of a row */, uint32_t l, ActT& a0, ActT& a1, ActT& a2) {
    const ActT* mine = row + 3 * l;
    a0 = mine[0]; a1 = mine[1]; a2 = mine[2];
    asm volatile("" ::: "memory");
}
// el of the addressing (sbr_tape.hip): the env of branch j minus e0, the env of the workgroup's first branch, an env holding
// `fanout` consecutive branches.  <= 256; the mask changes no value, it keeps a row access at scalar base + one 32-bit lane offset.
SBR_DEV uint32_t cycle_env_of(uint32_t j, uint32_t fanout, uint32_t e0u) { return (j / fanout - e0u) & 511u; }

// Where a branch ENDED (sbr_lookahead_actions_end / sbr_lookahead_sampled_end), for a terminal value on top of its return: stored
// once per launch and branch, behind the loop.  Each output is optional (wave-uniform tests).  A branch that is not done: the
// rows k_step forms for a call that does not end the episode - sbr_write_obs / sbr_write_state of the plant, the last interval's
// start values (x6) and the running time c.t, which is sbr_finish_step's t_obs for such a call - the observation as
// k_rollout_policy writes it back on exit.  A done branch (on entry or during the launch): zeros; its plant stopped at the done
// call without the terminal phases, a state no other entry point reports.  float32 whatever cfg.out_f64 says, like the policy
// kernel's observation.  Plain per-lane stores, 72 and 60 bytes per lane at a lane stride of 72 and 60: the wave's rows are
// contiguous, so every byte of the lines it touches is written.  The 18 + 15 stores of the source are adjacent, and the backend
// merges them into 16-byte ones (5 per obs_end row, 4 per state_end row) - once per launch, not per call,
// where k_step transposes its rows through LDS on every call.
SBR_DEV void sbr_store_branch_end(int64_t j0, uint32_t l, bool done, double t, const double (&x)[SBR_NX], const SbrX6Reg& x6,
                                  float* __restrict__ obs_end, float* __restrict__ state_end, uint8_t* __restrict__ done_end) {
    if (done_end) (done_end + j0)[l] = (uint8_t)(done ? 1 : 0);
    if (obs_end) {
        float o[SBR_NOBS];
#pragma unroll
        for (int k = 0; k < SBR_NOBS; ++k) o[k] = 0.0f;
        if (!done) {
            double xa6[SBR_NXD];
            x6.get(xa6);
            sbr_write_obs<float>(o, 1, t, x, xa6, x);
        }
        float* mine = obs_end + j0 * SBR_NOBS + l * (uint32_t)SBR_NOBS;
#pragma unroll
        for (int k = 0; k < SBR_NOBS; ++k) mine[k] = o[k];
    }
    if (state_end) {
        float sv[SBR_NSTATE];
#pragma unroll
        for (int k = 0; k < SBR_NSTATE; ++k) sv[k] = 0.0f;
        if (!done) sbr_write_state<float>(sv, 1, t, x);
        float* mine = state_end + j0 * SBR_NSTATE + l * (uint32_t)SBR_NSTATE;
#pragma unroll
        for (int k = 0; k < SBR_NSTATE; ++k) mine[k] = sv[k];
    }
}
