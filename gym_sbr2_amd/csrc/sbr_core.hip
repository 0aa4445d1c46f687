// sbr_core.hip - the handle of libsbr_amd.so (gfx950), k_step and everything that is not a fused kernel.  See include/sbr_amd.h
// for the contract.  Kernels (all one-lane-per-env over SoA float64 state, 256-thread workgroups = four wavefronts, one per SIMD
// of a CU, so a launch of N envs is N/64 independent waves that the dispatcher spreads over the 1024 SIMDs):
//   k_reset    influent mix (tables in LDS) + fill phase (252 RK4 substeps under either scheme) + controller init + obs
//   k_reset_models   k_reset with every env under its own plant model of the handle's table (sbr_reset_models)
//   k_step     one SbrOS.step(): phase logic, 2 PIDs, the interval's integration (cfg.scheme 1: adaptive Butcher-5 steps per lane,
//              sbr_b5a; scheme 0: 10 RK4 substeps; x2 at phase boundaries), reward,
//              obs/state, and the terminal phases on the last call of an episode
//   k_cycle_reset   the reset of the per-cycle env SBR-v2 (its step, k_cycle, is a fused kernel: sbr_rollout.hip)
//   k_export, k_import, k_m1_explicit   public <-> internal controller layout; implicit So[-1] / Sno[-1] made explicit
//   k_stats    wavefront (DPP) reductions of a per-env vector -> {sum,min,max,count}
//   k_draw_influent   influent futures without a reset: the reset's mix per (env, draw) into a caller's buffer (sbr_draw_influent)
//   k_rhs, k_substeps, k_normals, k_scenarios, k_fill   known-answer helpers for the parity tests, the scenario draw, handle init
// What bounds them and how the arithmetic is organised for it: sbr_device.h (sbr_rates, sbr_rk4), DESIGN.md sections 3 and 5.
// k_step is here and not in a unit of its own because its register allocation, and k_substeps', comes out differently when the
// two are compiled apart (same instructions, other registers; profiles/r15_units_isa.txt): the layout follows the machine code.
// Entry points: create / destroy / config / query, tables, the resets (sbr_reset_models among them), trace, step, state get / set, influent and its futures, stats, the
// known-answer helpers, synchronize and the timers.  The calling thread's error text (sbr_last_error(NULL)) lives here.
#include "sbr_host.h"

static constexpr int kTableDoubles = SBR_NSCEN * SBR_NSERIES * SBR_NSAMP;   // 5376 doubles = 42 KiB (the layout in HBM)
// In LDS a scenario's block of 14 x 48 doubles is padded to 674: 672 doubles are 1344 dwords = 0 mod 64 banks, so lanes
// that hold the eight different scenarios (scenario = env id mod 8) would all hit the same bank pair on every table read
// (8-way conflict); 674 puts scenario s on banks 4s, 4s+1.
#define SBR_TSTRIDE (SBR_NSERIES * SBR_NSAMP + 2)
static constexpr int kLdsTableDoubles = 2 * SBR_NSCEN * SBR_TSTRIDE;        // means then stds: 86 272 B

// public <-> internal translation (sbr_get_state / sbr_set_state / sbr_get_ctrl_row); only_row < 0 = all rows
__global__ __launch_bounds__(SBR_BLOCK) void k_export(SbrPar p, SbrBuf b, double* __restrict__ out, int only_row) {
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SBR_BLOCK, i = i0 + l;
    if (i >= b.n) return;
    SbrRecord r;
    load_record<true>(p, b, i0, l, XROW(8), XROW(9), r);
    double v[SBR_NCTRL];
    v[SBR_C_T] = r.c.t; v[SBR_C_SO_M1] = r.c.so_m1; v[SBR_C_SO_M2] = r.c.so_m2;
    v[SBR_C_SNO_M1] = r.c.sno_m1; v[SBR_C_SNO_M2] = r.c.sno_m2;
    v[SBR_C_IE_DO] = r.c.ie_do; v[SBR_C_IE_EC] = r.c.ie_ec; v[SBR_C_EC_LAST] = r.c.ec_last;
#pragma unroll
    for (int j = 0; j < SBR_KLA_HIST; ++j) v[SBR_C_KLA_HIST0 + j] = r.hist[j];
    v[SBR_C_QW] = r.qw; v[SBR_C_RETURN] = r.ret; v[SBR_C_STEPS] = (double)r.meta.steps;
    v[SBR_C_DONE] = r.meta.done ? 1.0 : 0.0; v[SBR_C_STATUS] = (double)r.meta.status; v[SBR_C_KLA_SUM] = r.ksum;
    v[SBR_C_PLAN] = (double)r.meta.plan;
    if (only_row >= 0) {
#pragma unroll
        for (int k = 0; k < SBR_NCTRL; ++k) if (k == only_row) out[i] = v[k];
    } else {
#pragma unroll
        for (int k = 0; k < SBR_NCTRL; ++k) out[(int64_t)k * b.n + i] = v[k];
    }
}
// makes implicit So[-1] / Sno[-1] explicit (sbr_set_state with a plant only)
__global__ __launch_bounds__(SBR_BLOCK) void k_m1_explicit(SbrBuf b) {
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SBR_BLOCK;
    if (i0 + l >= b.n) return;
    SbrMeta m = SbrMeta::unpack(CTRL(R_META));
    if (m.m1i) {
        CTRL(R_SO_M1) = XROW(8); CTRL(R_SNO_M1) = XROW(9);
        m.m1i = false;
        CTRL(R_META) = SbrMeta::pack(m);
    }
}
__global__ __launch_bounds__(SBR_BLOCK) void k_import(SbrPar p, SbrBuf b, const double* __restrict__ in) {
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SBR_BLOCK, i = i0 + l;
    if (i >= b.n) return;
#define IN(r) in[(int64_t)(r) * b.n + i]
    SbrRecord r;
    r.c.t = IN(SBR_C_T); r.c.so_m1 = IN(SBR_C_SO_M1); r.c.so_m2 = IN(SBR_C_SO_M2);
    r.c.sno_m1 = IN(SBR_C_SNO_M1); r.c.sno_m2 = IN(SBR_C_SNO_M2);
    r.c.ie_do = IN(SBR_C_IE_DO); r.c.ie_ec = IN(SBR_C_IE_EC); r.c.ec_last = IN(SBR_C_EC_LAST);
#pragma unroll
    for (int j = 0; j < SBR_KLA_HIST; ++j) r.hist[j] = IN(SBR_C_KLA_HIST0 + j);
    r.qw = IN(SBR_C_QW); r.ret = IN(SBR_C_RETURN); r.ksum = IN(SBR_C_KLA_SUM);
    double st = IN(SBR_C_STEPS);
    st = st >= 0.0 ? (st < (double)SBR_MAX_STEPS ? st : (double)SBR_MAX_STEPS) : 0.0;
    double pl = IN(SBR_C_PLAN);
    pl = pl >= 0.0 ? (pl < 255.0 ? pl : 255.0) : 0.0;       // also catches NaN
    r.meta.steps = (int)st; r.meta.status = (int)IN(SBR_C_STATUS) & 7; r.meta.done = IN(SBR_C_DONE) != 0.0; r.meta.plan = (int)pl;
    store_record<true>(p, b, i0, l, r);
#undef IN
}

// scenario of cfg.random_scenario = 1: uniform over the 8 scenarios (np.random.choice(8, 1), gym_SBR_env4.py:107), Philox
// stream 2 keyed by the seed of this reset, subsequence = global env id; draw d of sbr_draw_influent: stream word 2 + 256 * d
SBR_DEV int sbr_scenario_draw(uint64_t seed, uint64_t gid, uint32_t stream = 2u) {
    uint32_t c[4] = {0u, stream, (uint32_t)gid, (uint32_t)(gid >> 32)};
    sbr_philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (int)(c[0] & (SBR_NSCEN - 1));
}

// copy the influent tables [2][8][14][48] from HBM into the padded LDS image (whole workgroup; caller synchronises)
template <int BLK = SBR_RESET_BLOCK>
SBR_DEV void stage_tables(double* lds, const double* __restrict__ tables) {
    for (int k = threadIdx.x; k < 2 * kTableDoubles; k += BLK)
        lds[k + 2 * (k / (SBR_NSERIES * SBR_NSAMP))] = tables[k];
}

// influent_mixed for one lane (buffer_tank3.py:68-107): series = mean + std*rnd with ONE rnd vector shared by all series,
// flow-weighted means, sums accumulated in sample order like python's sum().  ld[1..13]; ld[0] is set by the caller.
// `stream`: the stream word of the device's own normals (sbr_normal_pair; the resets draw under 0).
SBR_DEV void influent_lane(const double* lds, bool need_tables, int s, const double* __restrict__ rnd,
                           const double* __restrict__ influent, uint64_t seed, uint64_t gid, int64_t i, double (&ld)[SBR_NX],
                           uint32_t stream = 0u) {
    if (need_tables) {
        s = s < 0 ? 0 : (s >= SBR_NSCEN ? SBR_NSCEN - 1 : s);        // never index LDS out of range
        const double* mu = lds + s * SBR_TSTRIDE;
        const double* sd = lds + (SBR_NSCEN + s) * SBR_TSTRIDE;
        double acc[13], sq = 0.0;
#pragma unroll
        for (int j = 0; j < 13; ++j) acc[j] = 0.0;
        for (int kk = 0; kk < SBR_NSAMP; kk += 2) {
            double z[2];
            if (rnd) { z[0] = rnd[i * SBR_NSAMP + kk]; z[1] = rnd[i * SBR_NSAMP + kk + 1]; }
            else sbr_normal_pair(seed, gid, (uint32_t)(kk >> 1), z[0], z[1], stream);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int k = kk + u;
                const double q = mu[13 * SBR_NSAMP + k] + sd[13 * SBR_NSAMP + k] * z[u];
                sq = sq + q;
#pragma unroll
                for (int j = 0; j < 13; ++j) acc[j] = acc[j] + (mu[j * SBR_NSAMP + k] + sd[j * SBR_NSAMP + k] * z[u]) * q;
            }
        }
        const double rsq = sbr_rcp(sq);                               // one reciprocal for the 13 flow-weighted means (1 ulp each)
#pragma unroll
        for (int j = 0; j < 13; ++j) ld[1 + j] = acc[j] * rsq;
    } else {
#pragma unroll
        for (int j = 1; j < SBR_NX; ++j) ld[j] = influent[i * SBR_NX + j];
    }
    ld[0] = 0.66;                                                    // buffer_tank3.py:107; callers overwrite it
}
// which scenario an env is reset with: the caller's tensor, else a device draw (cfg.random_scenario), else the fixed one
SBR_DEV int pick_scenario(const SbrPar& p, const int32_t* __restrict__ scenario, int fixed, uint64_t seed, uint64_t gid, int64_t i) {
    if (scenario) return scenario[i];
    return p.random_scenario ? sbr_scenario_draw(seed, gid) : fixed;
}

// ------------------------------------------------------------------------------------------- reset
// SbrOS.reset :168-438.  Influent tables (means, stds: 2 x 42 KiB) are staged in LDS once per
// workgroup; every lane then walks the 48 samples of ITS scenario (same scenario => LDS broadcast).
// BLK = 512 (launches with more wavefronts than the device has SIMDs): the 84 KiB of tables allow one workgroup per CU, so eight
// waves per workgroup are what puts two on a SIMD.
template <typename OutT, bool CARRY, int BLK = SBR_RESET_BLOCK>
__global__ __launch_bounds__(BLK) void k_reset(SbrPar p, SbrBuf b, const double* __restrict__ tables,
                                                    uint64_t seed, const int32_t* __restrict__ scenario,
                                                    const double* __restrict__ rnd, const double* __restrict__ influent,
                                                    const uint8_t* __restrict__ mask, OutT* __restrict__ obs) {
    extern __shared__ __attribute__((aligned(16))) double lds[];   // [2][8][SBR_TSTRIDE]
    const bool need_tables = (influent == nullptr);
    if (need_tables) {
        stage_tables<BLK>(lds, tables);
        __syncthreads();
    }
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * BLK, i = i0 + l;
    if (i >= b.n) return;
    if (mask != nullptr && mask[i] == 0) return;
    const uint64_t gid = (uint64_t)(b.first_env_id + i);

    double ld[SBR_NX];
    influent_lane(lds, need_tables, pick_scenario(p, scenario, 6 /* :180 */, seed, gid, i), rnd, influent, seed, gid, i, ld);

    // ---- start state: cfg.x0 / cfg.IV (:197-203), or with CARRY this env's own current state (x0_new / IV_new)
    double x[SBR_NX], x0[SBR_NX];
    double iv = p.IV, qin = p.qin;
    if (CARRY) {
        load_x(b, i0, l, x0);
        iv = x0[0]; qin = p.WV - iv;
        ld[0] = qin * p.inv_T_fill;
    } else {
#pragma unroll
        for (int j = 0; j < SBR_NX; ++j) {
            x0[j] = p.x0[j];
            // held in VGPRs from here on: read again from the argument registers after the fill loop (the observation's start
            // values, So[-2], Sno[-2]) they kept 17 SGPRs too many alive across it - spill slots, i.e. a scratch segment
            asm volatile("" : "+v"(x0[j]));
        }
        ld[0] = p.load0;                                             // :287
    }
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) { x[j] = x0[j]; INFL(j) = ld[j]; }

    // ---- fill phase, Sim_filling :1585-1654.  DO-PID at t_start == 0: ie = 0, dcv = 0, set-point 0
    SbrRecord rec;
    SbrCtl& c = rec.c;
    const double e = 0.0 - x0[8];
    double ie = 0.0;
    double kla = p.Kc_DO * e + p.KcI_DO * ie;
    if (kla > p.Kla_max) { kla = p.Kla_max; ie = ie - e * p.dt; }
    if (kla < p.Kla_min) { kla = p.Kla_min; ie = ie - e * p.dt; }
    sbr_rk4<2>(p, x, p.h_fill, p.fill_rows, kla, ld[0], ld);        // RK4 under either scheme (see sbr_cycle_phase)
    c.t = p.T_fill;
    c.so_m2 = x0[8]; c.so_m1 = x[8];
    c.sno_m2 = x0[9]; c.sno_m1 = x[2];                               // :1652 stores Ss in the Sno memory
    c.ie_do = ie; c.ie_ec = 0.0; c.ec_last = 0.0; c.ec_prev = 0.0;
    c.u_do = 0.0; c.u_ec = 15.0;                                     // :212-213
#pragma unroll
    for (int j = 0; j < SBR_KLA_HIST; ++j) rec.hist[j] = ((SBR_KLA_HIST - 1 - j) % 2 == 0) ? kla : 0.0;   // [0,k]*126, :323
    c.kla_last = kla;
    rec.ret = 0.0; rec.qw = 0.0;
    rec.meta.status = sbr_status_bits(p, x);
    rec.ksum = 0.0;                                  // python's sum() over the list [0, k]*126, left to right
    for (int j = 0; j < p.fill_rows / 2; ++j) rec.ksum = rec.ksum + kla;
    store_x(b, i0, l, x);
    store_record<true>(p, b, i0, l, rec);
    if (obs) {   // volume blend of influent and post-fill state, :346-361
        double xr[SBR_NX];
        const double rwv = sbr_rcp(qin + iv);
#pragma unroll
        for (int j = 0; j < SBR_NX; ++j) xr[j] = (qin * ld[j] + x[j] * iv) * rwv;
        double x06[SBR_NXD];
        sbr_take6(x0, x06);
        sbr_write_obs<OutT>(obs + i * SBR_NOBS, 1, c.t, xr, x06, x);
    }
}

// k_reset over DOMAIN-RANDOMISED envs (sbr_reset_models): k_reset's body word for word - REPEATED and not shared, so that k_reset's
// register allocation stays where it is - with `p` the model of the lane's WAVE in the handle's table (sbr_wave_model: model
// (global id / envs_per_model) % n_models) and not the handle's own constants.  The fill phase, the status bits, the controller's
// start values and the observation are then the model's; the influent draw reads nothing of the plant.  A 512-thread workgroup
// may span two models: each wave reads its own.  The table's address is formed behind the bounds and mask tests, from the first
// lane the wave still has; the lanes it still has all belong to one model.
template <typename OutT, bool CARRY, int BLK = SBR_RESET_BLOCK>
__global__ __launch_bounds__(BLK) void k_reset_models(const SbrPar* __restrict__ table, uint32_t n_models, int64_t envs_per_model, SbrBuf b,
                                                      const double* __restrict__ tables, uint64_t seed,
                                                      const int32_t* __restrict__ scenario, const double* __restrict__ rnd,
                                                      const double* __restrict__ influent, const uint8_t* __restrict__ mask,
                                                      OutT* __restrict__ obs) {
    extern __shared__ __attribute__((aligned(16))) double lds[];   // [2][8][SBR_TSTRIDE]
    const bool need_tables = (influent == nullptr);
    if (need_tables) {
        stage_tables<BLK>(lds, tables);
        __syncthreads();
    }
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * BLK, i = i0 + l;
    if (i >= b.n) return;
    if (mask != nullptr && mask[i] == 0) return;
    const uint64_t gid = (uint64_t)(b.first_env_id + i);
    const SbrPar& p = *(const SbrPar*)sbr_wave_model(table, n_models, envs_per_model, gid);

    double ld[SBR_NX];
    influent_lane(lds, need_tables, pick_scenario(p, scenario, 6 /* :180 */, seed, gid, i), rnd, influent, seed, gid, i, ld);

    double x[SBR_NX], x0[SBR_NX];
    double iv = p.IV, qin = p.qin;
    if (CARRY) {
        load_x(b, i0, l, x0);
        iv = x0[0]; qin = p.WV - iv;
        ld[0] = qin * p.inv_T_fill;
    } else {
#pragma unroll
        for (int j = 0; j < SBR_NX; ++j) {
            x0[j] = p.x0[j];
            asm volatile("" : "+v"(x0[j]));                          // held in VGPRs across the fill loop: see k_reset
        }
        ld[0] = p.load0;
    }
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) { x[j] = x0[j]; INFL(j) = ld[j]; }

    SbrRecord rec;
    SbrCtl& c = rec.c;
    const double e = 0.0 - x0[8];
    double ie = 0.0;
    double kla = p.Kc_DO * e + p.KcI_DO * ie;
    if (kla > p.Kla_max) { kla = p.Kla_max; ie = ie - e * p.dt; }
    if (kla < p.Kla_min) { kla = p.Kla_min; ie = ie - e * p.dt; }
    sbr_rk4<2>(p, x, p.h_fill, p.fill_rows, kla, ld[0], ld);
    c.t = p.T_fill;
    c.so_m2 = x0[8]; c.so_m1 = x[8];
    c.sno_m2 = x0[9]; c.sno_m1 = x[2];
    c.ie_do = ie; c.ie_ec = 0.0; c.ec_last = 0.0; c.ec_prev = 0.0;
    c.u_do = 0.0; c.u_ec = 15.0;
#pragma unroll
    for (int j = 0; j < SBR_KLA_HIST; ++j) rec.hist[j] = ((SBR_KLA_HIST - 1 - j) % 2 == 0) ? kla : 0.0;
    c.kla_last = kla;
    rec.ret = 0.0; rec.qw = 0.0;
    rec.meta.status = sbr_status_bits(p, x);
    rec.ksum = 0.0;
    for (int j = 0; j < p.fill_rows / 2; ++j) rec.ksum = rec.ksum + kla;
    store_x(b, i0, l, x);
    store_record<true>(p, b, i0, l, rec);
    if (obs) {
        double xr[SBR_NX];
        const double rwv = sbr_rcp(qin + iv);
#pragma unroll
        for (int j = 0; j < SBR_NX; ++j) xr[j] = (qin * ld[j] + x[j] * iv) * rwv;
        double x06[SBR_NXD];
        sbr_take6(x0, x06);
        sbr_write_obs<OutT>(obs + i * SBR_NOBS, 1, c.t, xr, x06, x);
    }
}

// ------------------------------------------------------------------------------------------- step
// All loads of a lane are issued up front, with addresses that depend on nothing loaded (they are asynchronous; the first
// use waits): ONE exposed memory round trip per launch.  Measured alternatives that were WORSE (profiles/r01_notes.md):
// loading the Kla history and the bookkeeping rows after the integration (+2.4 us: serial round trips).
// The template parameter BLK is the workgroup size.  256 threads (four waves, one per SIMD of a CU; the kernel comes out at
// ~250 VGPRs - tests/test_isa_cpu.py holds it to <= 256 - i.e. two waves per SIMD, which batches above 65536 envs use to overlap the memory phases of one wave with the
// arithmetic of the other and to issue FMAs at 4.43 instead of 5.19 cycles) is the fastest from ~32768 envs up; below that
// 64-thread workgroups win - one wave per workgroup spreads a batch over four times as many CUs, each with its own path to
// memory and its own LDS (profiles/r02_ab_block.log: 1024 .. 16384 envs 12.45 -> 11.6 us per launch, 32768: 12.65 -> 12.1,
// 49152: 13.0 -> 12.8; 65536: 13.85 against 14.03, so 256 from there on).
// Values that only have to SURVIVE the integration (the Kla ring, return, packed steps/status/done, the six xdot start
// values) are parked in LDS, not in VGPRs and not in scratch: a ~100-cycle round trip instead of a trip through L2/HBM, and
// the RK4 loop keeps its registers (keeping them in VGPRs was measured: +0.6 us).  Slot j of lane l of wave w is at
// park[(w*NSLOT + j)*64 + l] (conflict-free).
// LDS slots of a lane in k_step: return, meta, the Kla window sum w8, the six xdot start values (and the OCI running sum);
// the region is sized for the output transposes (64 float64 observation rows: 9216 B = 18 slots).
#define SBR_PK_RET 0
#define SBR_PK_META 1
#define SBR_PK_W8 2
#define SBR_PK_X6 3
#define SBR_PK_KSUM (SBR_PK_X6 + SBR_NXD)
#define SBR_NPARK 20
#define SBR_NPARK_2W 32     // k_step<.., WAVES = 2>: + the parked values (SbrPark, behind the six start values and the OCI sum)
static_assert(SBR_PK_KSUM + 1 + PK_CALL_END <= SBR_NPARK_2W && SBR_PK_KSUM + 1 + PK_TERM_END <= SBR_NPARK_2W,
              "the LDS region of the two-waves build is too small for its parked values");

// One output row per lane (obs: 18 values, state: 15) -> the caller's row-major tensor.  A full wavefront owns 64
// consecutive rows, i.e. ONE contiguous block of 64 x NV x sizeof(OutT) bytes (4608 B of float32 observations): the rows go
// through the wave's own LDS region and leave as 16-byte-per-lane stores (obs + state: 9 store instructions per lane).
// Written directly, every lane stores NV separate dwords at a 72- or 60-byte stride: 33 store instructions, each touching
// 36 cache lines; with all 1024 waves in their epilogue at once those stores queue behind each other (measured with the
// stamp build: 2.8 us of a 17.6 us launch).  Waves that are not full (last wave of a ragged batch) and misaligned
// destinations take the direct form.  LDS operations of one wave execute in issue order, so the region can be reused
// without a workgroup barrier; the wave barrier keeps the compiler from reordering across it.
template <typename OutT, int NV>
SBR_DEV void store_rows(OutT* __restrict__ rows /* out + i0*NV: first row of the workgroup */, uint32_t l, char* stage,
                        bool wide, const OutT (&v)[NV]) {
    constexpr int RB = NV * (int)sizeof(OutT);                 // bytes per row
    constexpr int CH = 64 * RB / 16;                           // 16-byte chunks per wave
    const uint32_t lane = l & 63u;
    char* wdst = reinterpret_cast<char*>(rows + (size_t)(l & ~63u) * NV);
    if (wide && (reinterpret_cast<uintptr_t>(wdst) & 15u) == 0) {
        asm volatile("" ::: "memory");                         // see store_rows2: the staging stores must not overtake the parked loads
        typename SbrAliasOf<OutT>::type* mine = reinterpret_cast<typename SbrAliasOf<OutT>::type*>(stage + lane * RB);
#pragma unroll
        for (int k = 0; k < NV; ++k) mine[k] = v[k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        constexpr int NR = (CH + 63) / 64;
        sbr_u32x4 ch[NR];                                      // every chunk into registers first, then the stores (see store_rows2)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int c = r * 64 + (int)lane;
            if ((r + 1) * 64 <= CH || c < CH) ch[r] = *reinterpret_cast<const sbr_u32x4_alias*>(stage + c * 16);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int c = r * 64 + (int)lane;
            if ((r + 1) * 64 <= CH || c < CH) st_out16(reinterpret_cast<sbr_u32x4*>(wdst + c * 16), ch[r]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
#pragma unroll
        for (int k = 0; k < NV; ++k) rows[(size_t)l * NV + k] = v[k];
    }
}

// Two row sets at once (observation rows first, state rows behind them in the staging region): stage both, ONE wave barrier,
// read every 16-byte chunk into registers, then issue the stores.  The stores are inline assembly with a memory clobber (the
// sc1 modifier has no builtin for 16 bytes), which the compiler will not move an LDS read across: read-store-read-store cost
// one exposed LDS round trip per chunk (nine per call until round 4).  `stage` must hold 64 (RB_A + RB_B) bytes.
// COLD_DIRECT: the direct form (ragged wave, misaligned destination) is marked unlikely and laid out behind the caller's hot code.
template <typename OutT, int NA, int NB, bool COLD_DIRECT = false>
SBR_DEV void store_rows2(OutT* __restrict__ rows_a, OutT* __restrict__ rows_b, uint32_t l, char* stage, bool wide,
                         const OutT (&va)[NA], const OutT (&vb)[NB]) {
    constexpr int RA = NA * (int)sizeof(OutT), RBB = NB * (int)sizeof(OutT);
    constexpr int CA = 64 * RA / 16, CB = 64 * RBB / 16;         // 16-byte chunks per wave
    constexpr int NRA = (CA + 63) / 64, NRB = (CB + 63) / 64;
    const uint32_t lane = l & 63u;
    char* wa = reinterpret_cast<char*>(rows_a + (size_t)(l & ~63u) * NA);
    char* wb = reinterpret_cast<char*>(rows_b + (size_t)(l & ~63u) * NB);
    if (SBR_USUAL_IF(COLD_DIRECT, wide && ((reinterpret_cast<uintptr_t>(wa) | reinterpret_cast<uintptr_t>(wb)) & 15u) == 0)) {
        // The staging region is the wave's parking space, whose slots were read as float64 just before: to the compiler's
        // type-based alias analysis a float32 store and a float64 load never alias, so without this barrier it may hoist the
        // staging stores above those loads (seen in round 4: rows 27.. of the float32 outputs held parked values).
        asm volatile("" ::: "memory");
        char* sa = stage;
        char* sb = stage + 64 * RA;
        typename SbrAliasOf<OutT>::type* ma = reinterpret_cast<typename SbrAliasOf<OutT>::type*>(sa + lane * RA);
        typename SbrAliasOf<OutT>::type* mb = reinterpret_cast<typename SbrAliasOf<OutT>::type*>(sb + lane * RBB);
#pragma unroll
        for (int k = 0; k < NA; ++k) ma[k] = va[k];
#pragma unroll
        for (int k = 0; k < NB; ++k) mb[k] = vb[k];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        sbr_u32x4 ca[NRA], cb[NRB];
#pragma unroll
        for (int r = 0; r < NRA; ++r) {
            const int c = r * 64 + (int)lane;
            if ((r + 1) * 64 <= CA || c < CA) ca[r] = *reinterpret_cast<const sbr_u32x4_alias*>(sa + c * 16);
        }
#pragma unroll
        for (int r = 0; r < NRB; ++r) {
            const int c = r * 64 + (int)lane;
            if ((r + 1) * 64 <= CB || c < CB) cb[r] = *reinterpret_cast<const sbr_u32x4_alias*>(sb + c * 16);
        }
#pragma unroll
        for (int r = 0; r < NRA; ++r) {
            const int c = r * 64 + (int)lane;
            if ((r + 1) * 64 <= CA || c < CA) st_out16(reinterpret_cast<sbr_u32x4*>(wa + c * 16), ca[r]);
        }
#pragma unroll
        for (int r = 0; r < NRB; ++r) {
            const int c = r * 64 + (int)lane;
            if ((r + 1) * 64 <= CB || c < CB) st_out16(reinterpret_cast<sbr_u32x4*>(wb + c * 16), cb[r]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    } else {
#pragma unroll
        for (int k = 0; k < NA; ++k) rows_a[(size_t)l * NA + k] = va[k];
#pragma unroll
        for (int k = 0; k < NB; ++k) rows_b[(size_t)l * NB + k] = vb[k];
    }
}

// The model constants (SbrPar, 1.2 KB) travel in the kernel-argument segment and the compiler fetches them with scalar
// loads where it needs them - in pieces, because ~60 doubles do not fit the scalar register file at once.  The argument
// segment of a launch is a fresh buffer in device memory that no cache has seen: the first touch of each of its 64-byte lines
// is a miss in the scalar cache that goes out to L2 / memory, and every such piece sits behind its own s_waitcnt ON the
// wave's critical path (PMC, round 4: SQ_WAIT_ANY is what grew when an unrelated code change added two late scalar loads,
// +0.3 us per launch).  So every line of the segment is touched ONCE, all at the same time, at wave start: the misses
// overlap each other and the ~2 us of global-load latency, and every later scalar load of a constant hits the scalar cache.
// The loads target one scratch SGPR whose value is never used (measured: profiles/r04_ab_kernarg_warm_modes.log).
#define SBR_WARM_LINES                                                                                                            \
        "s_load_dword %0, %1, 0x40\n s_load_dword %0, %1, 0x80\n s_load_dword %0, %1, 0xc0\n s_load_dword %0, %1, 0x100\n"        \
        "s_load_dword %0, %1, 0x140\n s_load_dword %0, %1, 0x180\n s_load_dword %0, %1, 0x1c0\n s_load_dword %0, %1, 0x200\n"     \
        "s_load_dword %0, %1, 0x240\n s_load_dword %0, %1, 0x280\n s_load_dword %0, %1, 0x2c0\n s_load_dword %0, %1, 0x300\n"     \
        "s_load_dword %0, %1, 0x340\n s_load_dword %0, %1, 0x380\n s_load_dword %0, %1, 0x3c0\n s_load_dword %0, %1, 0x400\n"     \
        "s_load_dword %0, %1, 0x440\n s_load_dword %0, %1, 0x480\n s_load_dword %0, %1, 0x4c0\n s_load_dword %0, %1, 0x500\n"     \
        "s_load_dword %0, %1, 0x538\n s_load_dword %0, %1, 0x548\n"
// k_step's argument segment: four pointers / sizes, the flags word (+ padding), four pointers, SbrPar, SbrBuf.  The touched
// offsets must stay inside it (a scalar load past the segment may fault) and reach its last line.
static constexpr size_t kStepParOffset = 72;                  // where SbrPar lies in the segment, behind the leading arguments (SbrStepLead)
static constexpr size_t kStepKernargBytes = kStepParOffset + sizeof(SbrPar) + sizeof(SbrBuf);
static_assert(kStepKernargBytes >= 0x548 + 4 && kStepKernargBytes <= 0x548 + 56,
              "SbrPar / SbrBuf changed size: adjust the offsets of SBR_WARM_LINES to cover k_step's argument segment");
// In two halves, issue at wave start and wait after the wave's global loads have gone out: the scratch register stays allocated
// (an in/out operand of the second statement) until the loads have landed, so the compiler cannot hand it to anything else
// while they are in flight.  (One statement placed after the global loads was measured too: +0.2 us per launch.)
SBR_DEV uint32_t sbr_warm_kernarg_issue() {
    auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    uint32_t t;
    asm volatile(SBR_WARM_LINES : "=&s"(t) : "s"(kp) : "memory");
    return t;
}
SBR_DEV void sbr_warm_kernarg_wait(uint32_t t) { asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t) : : "memory"); }

// Constants and pointers that are needed on BOTH sides of the step loops are not kept across them.  ~60 wave-uniform doubles do not
// fit the scalar register file next to the loops' own constants: held live (or loaded once for both control intervals, or for the
// ordinary path and the terminal phases alike) the compiler spills them into VGPR lanes - 153 spilled dwords, 604 lane operations,
// 251 AGPR moves of store addresses in a call's straight-line code (profiles/r12_notes.md).  The argument segment is warm in the
// scalar cache (SBR_WARM_LINES), so whatever follows a step loop reads its constants AGAIN from there: an empty asm statement
// hides the segment pointer's origin, and loads through it can neither be merged with the ones in front of the loop nor hoisted
// over it.  The pointer stays in SGPRs and in the constant address space (scalar loads); it must be re-made on a wave-uniform path -
// a pointer merged behind a divergent branch would become a per-lane value and its loads vector loads.
// sbr_kernarg_again / sbr_par_again / SbrStepLead describe k_step's argument segment and are for k_step alone.
typedef const __attribute__((address_space(4))) char* SbrKernargPtr;
SBR_DEV SbrKernargPtr sbr_kernarg_again() {
    SbrKernargPtr kp = (SbrKernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return kp;
}
SBR_DEV const SbrPar& sbr_par_again() { return *(const SbrPar*)(sbr_kernarg_again() + kStepParOffset); }
template <typename OutT, typename ActT>
struct SbrStepLead {          // k_step's leading arguments as they lie in the segment: same order and types as its parameter list (keep in step)
    double* bx; double* bctrl; int64_t bn; const ActT* action; uint32_t flags, pad_; OutT* obs; OutT* state; OutT* reward; uint8_t* done;
};
static_assert(sizeof(SbrStepLead<float, float>) == kStepParOffset && sizeof(SbrStepLead<double, double>) == kStepParOffset,
              "k_step's leading arguments changed: SbrStepLead and kStepParOffset must follow");
template <bool AGAIN>         // the PA of sbr_run_intervals; false (the two-waves build, which parks in LDS instead): the caller's own
struct SbrParAgain {
    SBR_DEV const SbrPar& again(const SbrPar& p) const {
        if constexpr (AGAIN) return sbr_par_again();
        else return p;
    }
};

// The leading arguments (14 dwords) are what the first global loads need; the library is built with
// -mllvm -amdgpu-kernarg-preload-count=16, so a wave starts with them in SGPRs and issues its loads without waiting for a
// scalar load of the argument segment (two serial scalar round trips before: n for the bounds test, then the pointers).
// `flags` carries every decision that shapes the LOAD phase (bit 0: the So[-2] / Sno[-2] rows are needed - derivative action
// or a trace buffer), taken on the host: until round 4 that test read two fields of `p` and one of `b0`, and the s_waitcnt
// in front of it held back EVERY global load of the wave for a scalar round trip to the argument segment.
#define SBR_KF_NEED_M2 1u
#define SBR_KF_STAGGER 2u           // set by the host on every launch in 256-thread workgroups
// trajectory export: the NO3-PID's e / ie / dcv of every interval go straight to the call's trace record while the PID runs
// (slot _FIRST for the first interval of the call, the plain slots for the last one run), so that nothing has to be carried
// across the integration for it.  Off (b.trace == NULL, the default) this is one untaken scalar branch per interval.
struct SbrTraceRec {
    const SbrBuf& b;
    const double* meta_lds;       // the lane's parked meta word
    int64_t env;                  // index of the lane's env in the handle
    SBR_DEV void pid(int iv, double e, double ie, double dcv) const {
        if (__builtin_expect(b.trace != nullptr, 0)) {
            const int64_t steps = (int64_t)((int)(*meta_lds) >> SbrMeta::kStepsShift);
            if (env < b.n_trace && steps < b.trace_cap) {
                double* rec = b.trace + (steps * SBR_NTRACE) * b.n_trace + env;
                if (iv == 0) {
                    rec[SBR_TR_E_EC_FIRST * b.n_trace] = e; rec[SBR_TR_IE_EC_FIRST * b.n_trace] = ie; rec[SBR_TR_DCV_EC_FIRST * b.n_trace] = dcv;
                }
                rec[SBR_TR_E_EC * b.n_trace] = e; rec[SBR_TR_IE_EC * b.n_trace] = ie; rec[SBR_TR_DCV_EC * b.n_trace] = dcv;
            }
        }
    }
};

// WAVES = 2 (scheme 1, launches with more wavefronts than the chip has SIMDs): the register budget of two resident waves per SIMD
// (256).  The scheme-1 step loops need more than that with everything the call carries across them (the one-wave build: 264; 322
// before round 12, which stopped carrying constants and addresses across); this build parks that - 13
// controller values per interval, 7 of the call, 19 around the idle phase of the done call - in the lane's LDS slots (64 KiB per
// workgroup, two workgroups per CU) and forms the row addresses of its stores again afterwards instead of keeping them.
// Same arithmetic, same bits.  Measured (profiles/r05_ab_two_waves.log): 65 536 envs 12.8 against 12.2 us per call (one wave per
// SIMD either way: the host keeps WAVES = 1 there), 131 072 envs 20.1 against 23.3, 262 144 envs 36.1 against 44.5.
template <typename OutT, typename ActT, int BLK, bool OCI, int SCH, int WAVES = 1>
__global__ __launch_bounds__(BLK, BLK == 256 && WAVES == 2 ? 2 : 1) void k_step(double* __restrict__ bx, double* __restrict__ bctrl, int64_t bn,
                                                      const ActT* __restrict__ action, uint32_t flags, OutT* __restrict__ obs,
                                                      OutT* __restrict__ state, OutT* __restrict__ reward,
                                                      uint8_t* __restrict__ done, SbrPar p, SbrBuf b0) {
    SbrBuf b = b0;
    b.x = bx; b.ctrl = bctrl; b.n = bn;
    // wave-major: wave w owns park[w][slot][64], 20 slots x 512 B = 10 KiB; the region is reused for the output
    // transpose (64 float64 observation rows take 9216 B, float32 observation + state rows together 8448 B)
    constexpr bool PARK = WAVES == 2;
    constexpr bool AGAIN = !PARK && SCH == 1;    // the one-wave scheme-1 builds read constants and pointers again behind the step loops (sbr_kernarg_again)
    constexpr int NSLOT = PARK ? SBR_NPARK_2W : SBR_NPARK;
    // the upper bounds of the parking region: static LDS is limited to 64 KiB per workgroup, and the two-waves build only pays while
    // TWO of its workgroups fit the 160 KiB of a CU - one more __shared__ word would silently halve the residency
    static_assert(sizeof(double) * NSLOT * BLK <= 65536, "k_step's parking region exceeds the 64 KiB static LDS limit");
    static_assert(!PARK || 2 * sizeof(double) * NSLOT * BLK <= 160 * 1024, "two workgroups of the two-waves build must fit a CU's 160 KiB of LDS");
    __shared__ __attribute__((aligned(16))) double park[NSLOT * BLK];
    uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * BLK;
    if (i0 + l >= b.n) return;
#ifdef SBR_STAMPS
    if (reinterpret_cast<uintptr_t>(b.stamps) == 1) return;   // diagnostic build: the launch period of an EMPTY k_step = the boundary
#endif
    double* wave_lds = park + (l >> 6) * (NSLOT * 64);
    double* my = wave_lds + (l & 63u);        // slot j of this lane: my[j * 64]
    double x[SBR_NX];
    SbrCtl c;
    SBR_STAMP(0, false);
    const uint32_t warm_token = sbr_warm_kernarg_issue();
    // Staggered entry (SBR_KF_STAGGER, large batches): every other workgroup of an XCD (workgroup g runs on XCD g % 8, so bit 3
    // of the index alternates inside one) waits ~0.65 us before its loads.  With one wave per SIMD every wave of the chip
    // otherwise loads at the same moment and stores at the same moment; half a microsecond of skew inside each XCD takes the
    // two bursts apart (measured: profiles/r04_notes.md, "staggered entry").
    if ((flags & SBR_KF_STAGGER) != 0u && ((blockIdx.x >> 3) & 1u) != 0u) __builtin_amdgcn_s_sleep(25);   // x 64 cycles
    // every load below has an address that depends on nothing loaded: ONE memory round trip (the ring used to be read
    // in logical order, whose rows depend on t: a second, dependent round trip)
    load_x(b, i0, l, x);
    const double meta0 = CTRL(R_META);
    c.t = CTRL(R_T); c.ie_do = CTRL(R_IE_DO); c.ie_ec = CTRL(R_IE_EC); c.ec_last = CTRL(R_EC_LAST);
    c.ec_prev = c.ec_last; c.u_do = 0.0; c.u_ec = 0.0;
    c.n_new = 0; c.st_new = 0; c.span = 0.0; c.rows = 9; c.plans = 0;
    if ((flags & SBR_KF_NEED_M2) != 0u) { c.so_m2 = CTRL(R_SO_M2); c.sno_m2 = CTRL(R_SNO_M2); }
    const ActT* act = action + i0 * 2;
    const double a0 = (double)act[2 * l], a1 = (double)act[2 * l + 1];           // one 8- or 16-byte load per lane
    c.kla_last = CTRL(R_KLA_LAST);
    const double w8_0 = CTRL(R_W8), ret0 = CTRL(R_RET);
    sbr_warm_kernarg_wait(warm_token);
    my[SBR_PK_RET * 64] = ret0; my[SBR_PK_META * 64] = meta0; my[SBR_PK_W8 * 64] = w8_0;
    // (The compiler sinks the action load into the `not done` branch below - one global_load behind the branch in the ISA.
    // Pinning it into the batch above was measured SLOWER, profiles/r04_ab_kernarg_warm_and_pinned_loads.log: left alone.)
    SbrX6LdsT<PARK> x6{my + SBR_PK_X6 * 64};
    if (OCI) my[SBR_PK_KSUM * 64] = CTRL(R_KSUM);          // only this reward keeps the running sum of Kla
    x6.put(x);
    // the ring slot of the oldest entry = where this call's first Kla goes; the three entries behind it are the ones that leave
    // the reward's window with this call's appends (SbrHistInc): loads whose address depends on t, issued now, needed after the
    // integration
    const int kb = ring_k(p, c.t) % SBR_KLA_HIST;
    double lv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) lv[j] = CTRL(R_RING0 + ring_wrap(kb + 1 + j));
    const double kla_before = c.kla_last;
    SBR_STAMP(1, true);                       // every load has returned, the parked values are in LDS
    double t_obs = p.t_cycle, r = 0.0;
    bool dn = true;
    double xa6[SBR_NXD];
    if (((int)meta0 & SbrMeta::kDone) == 0) {   // not done: a finished env waits for sbr_reset (the reference leaves resetting to the caller)
        double qw = 0.0;
        SbrRewardParts rp;
        const double v0 = x[0], si0 = x[1], xi0 = x[3];
        // So[-1], Sno[-1]: the plant's own values after an ordinary step (meta's m1i bit); the first call after a reset, an import
        // or a rollout fetches the rows (a second, dependent load: once per episode)
        c.so_m1 = x[8]; c.sno_m1 = x[9];
        const bool m1_rows = ((int)meta0 & SbrMeta::kM1i) == 0;
        if (SBR_RARE_IF(AGAIN, __builtin_amdgcn_ballot_w64(m1_rows) != 0ull)) {
            if (m1_rows) { c.so_m1 = CTRL(R_SO_M1); c.sno_m1 = CTRL(R_SNO_M1); }
        }
        if ((flags & SBR_KF_NEED_M2) == 0u) { c.so_m2 = c.so_m1; c.sno_m2 = c.sno_m1; }
        SBR_STAMP(2, false);
        const SbrTraceRec tr{b, my + SBR_PK_META * 64, i0 + l};
        if constexpr (PARK) {
            x6.park(PK_CALL_LV0, lv[0]); x6.park(PK_CALL_LV1, lv[1]); x6.park(PK_CALL_LV2, lv[2]);
            x6.park(PK_CALL_KLA_BEFORE, kla_before); x6.park(PK_CALL_V0, v0); x6.park(PK_CALL_SI0, si0); x6.park(PK_CALL_XI0, xi0);
        }
        sbr_run_intervals<SCH>(SbrParAgain<AGAIN>().again(p), c, x, a0, a1, x6, tr, SbrParAgain<AGAIN>());
        double kla_before_r = kla_before, v0_r = v0, si0_r = si0, xi0_r = xi0;
        if constexpr (PARK || AGAIN) asm volatile("" : "+v"(l) : : "memory");  // the row addresses of the stores are formed again from here (not kept across the integration)
        const SbrPar& pe = SbrParAgain<AGAIN>().again(p);
        if constexpr (AGAIN) {                    // ... from the handle's pointers as the argument segment holds them
            const auto& ka = *(const SbrStepLead<OutT, ActT>*)sbr_kernarg_again();
            b.x = ka.bx; b.ctrl = ka.bctrl; b.n = ka.bn;
        }
        if constexpr (PARK) {
            lv[0] = x6.unpark(PK_CALL_LV0); lv[1] = x6.unpark(PK_CALL_LV1); lv[2] = x6.unpark(PK_CALL_LV2);
            kla_before_r = x6.unpark(PK_CALL_KLA_BEFORE); v0_r = x6.unpark(PK_CALL_V0); si0_r = x6.unpark(PK_CALL_SI0);
            xi0_r = x6.unpark(PK_CALL_XI0);
        }
        SBR_STAMP(3, false);                  // PIDs + RK4 done
        SbrHistInc hs{my[SBR_PK_W8 * 64], kla_before_r, {lv[0], lv[1], lv[2]}, 0.0, false};
        if constexpr (!PARK) x6.get(xa6);
        double ksum = OCI ? my[SBR_PK_KSUM * 64] : 0.0;
        r = sbr_finish_step<OCI, SCH, SbrHistInc, true, SbrX6LdsT<PARK>, AGAIN>(pe, c, hs, x, xa6, t_obs, dn, qw, ksum, rp, &x6);
        if constexpr (PARK) x6.get(xa6);              // after the terminal phases, which leave their pre-settle values in the slots
        SBR_STAMP(4, false);                  // reward (and, on the done call, the terminal phases) done
        // everything that reads the three ring entries loaded before the integration comes BEFORE the first store: the memory
        // counter retires in order, so a wait for one of those (long finished) loads placed after the plant stores would wait
        // for the stores' acknowledgements too
        double w8_new, last_new;
        hs.roll(c, w8_new, last_new);
        asm volatile("" : "+v"(w8_new), "+v"(last_new) : : "memory");     // ... and the scheduler is held to that order
        SBR_STAMP(8, false);                  // window rolled: everything that waits for a load is done
        if (OCI) CTRL(R_KSUM) = ksum;
        // plant: V, Si and Xi only change with carbon dosing or in the terminal phases - skip their stores otherwise
        // (wave-uniform test: no lane of the wave changed them)
        const bool inert_moved = (x[0] != v0_r) || (x[1] != si0_r) || (x[3] != xi0_r);
        if (__builtin_amdgcn_ballot_w64(inert_moved) != 0ull) {
            store_x(b, i0, l, x);
        } else {
#pragma unroll
            for (int j = 0; j < SBR_NX; ++j) if (j != 0 && j != 1 && j != 3) st_out(&XROW(j), x[j]);
        }
        SBR_STAMP(9, false);                  // plant stores issued
        // So[-1], Sno[-1] stay implicit unless this was the done call (the terminal phases have moved x away from them)
        store_ctl(b, i0, l, c, false);
        if (SBR_RARE_IF(AGAIN, __builtin_amdgcn_ballot_w64(dn) != 0ull)) {
            if (dn) { CTRL(R_SO_M1) = c.so_m1; CTRL(R_SNO_M1) = c.sno_m1; }
        }
        // the Kla ring is addressed by the interval count: envs reset together share it, so the slot is normally
        // wave-uniform (scalar row arithmetic); a wave whose lanes disagree (masked resets, injected states) takes the
        // per-lane form.  A second (phase-boundary call) and a third append (the idle phase of the done call) are rare.
        const int kb_u = __builtin_amdgcn_readfirstlane(kb);
        const bool ring_uniform = __builtin_amdgcn_ballot_w64(kb != kb_u) == 0ull;
        const bool idle_pushed = hs.idle_pushed;
        const double app0 = c.n_new > 0 ? c.knew[0] : hs.idle;            // the appended values in order: knew[0], knew[1], idle
        const int n_app = c.n_new + (idle_pushed ? 1 : 0);
        if (SBR_USUAL_IF(AGAIN, ring_uniform)) {
            if (n_app > 0) st_out(&CTRL(R_RING0 + kb_u), app0);
        } else {
            if (n_app > 0) CTRL(R_RING0 + kb) = app0;
        }
        if (SBR_RARE_IF(AGAIN, __builtin_amdgcn_ballot_w64(n_app > 1) != 0ull)) {
            const double app1 = c.n_new > 1 ? c.knew[1] : hs.idle;
            if (n_app > 1) CTRL(R_RING0 + ring_wrap(kb + 1)) = app1;
            if (n_app > 2) CTRL(R_RING0 + ring_wrap(kb + 2)) = hs.idle;
        }
        st_out(&CTRL(R_KLA_LAST), last_new); st_out(&CTRL(R_W8), w8_new);
        if (SBR_RARE_IF(AGAIN, dn && pe.terminal)) CTRL(R_QW) = qw;
        const SbrMeta m = SbrMeta::unpack(my[SBR_PK_META * 64]);
        const int steps = m.steps;
        st_out(&CTRL(R_RET), my[SBR_PK_RET * 64] + r);
        // the m1i bit ("So[-1] / Sno[-1] are x[8] / x[9]") is claimed only by a call that RAN an interval: a call with
        // n_new == 0 (t injected as NaN) writes nothing to the memories, so it leaves them where they were - rows stay rows
        const bool m1i_new = dn ? false : (c.n_new > 0 ? true : !m1_rows);
        st_out(&CTRL(R_META), SbrMeta::pack({SbrMeta::next_steps(steps), m.status | c.st_new, dn, idle_pushed, m1i_new, c.plans & 0xff}));
        SBR_STAMP(10, false);                 // controller stores issued
        if (SBR_RARE_IF(AGAIN, b.trace != nullptr && i0 + l < b.n_trace && (int64_t)steps < b.trace_cap)) {     // trajectory export, off by default
            double* rec = b.trace + ((int64_t)steps * SBR_NTRACE) * b.n_trace + (i0 + l);
            rec[0] = c.t;
#pragma unroll
            for (int j = 0; j < SBR_NX; ++j) rec[(int64_t)(SBR_TR_X0 + j) * b.n_trace] = x[j];
            rec[SBR_TR_KLA * b.n_trace] = c.knew[c.n_new > 1 ? 1 : 0]; rec[SBR_TR_EC * b.n_trace] = c.ec_last;
            rec[SBR_TR_REWARD * b.n_trace] = r; rec[SBR_TR_DONE * b.n_trace] = dn ? 1.0 : 0.0;
            rec[SBR_TR_U_DO * b.n_trace] = c.u_do; rec[SBR_TR_U_EC * b.n_trace] = c.u_ec;
            const double ae2 = rp.ae * pe.inv_ae_max, ec2 = rp.ec * pe.inv_ec_max;
            rec[SBR_TR_R_EQI * b.n_trace] = rp.eqi2; rec[SBR_TR_R_OCI * b.n_trace] = ae2 + ec2;
            rec[SBR_TR_R_AE * b.n_trace] = ae2; rec[SBR_TR_R_EC * b.n_trace] = ec2;
            rec[SBR_TR_N_IV * b.n_trace] = (double)c.n_new; rec[SBR_TR_KLA_FIRST * b.n_trace] = c.knew[0];
            rec[SBR_TR_EC_FIRST * b.n_trace] = c.n_new > 1 ? c.ec_prev : c.ec_last;
            rec[SBR_TR_PLAN * b.n_trace] = (double)(c.plans & 0xff); rec[SBR_TR_PLAN_FIRST * b.n_trace] = (double)((c.plans >> 8) & 0xff);
        }
    } else {
        x6.get(xa6);
    }
    SBR_STAMP(5, false);                      // state stores issued
    if constexpr (AGAIN) {                        // behind the join of the two branches: wave-uniform again (see sbr_kernarg_again)
        const auto& ka = *(const SbrStepLead<OutT, ActT>*)sbr_kernarg_again();
        obs = ka.obs; state = ka.state; reward = ka.reward; done = ka.done;
    }
    if (reward) st_out(&(reward + i0)[l], (OutT)r);
    if (done) st_out(&(done + i0)[l], (uint8_t)(dn ? 1 : 0));
    SBR_STAMP(11, false);                     // reward / done stores issued
    const bool wide = __builtin_amdgcn_ballot_w64(true) == ~0ull;      // all 64 lanes of the wave hold an env
    char* stage = reinterpret_cast<char*>(wave_lds);
    // both row sets fit the wave's staging region together when they are float32 (64 x (72 + 60) = 8448 of the region's 10240 bytes: 20 slots x 512)
    constexpr bool kBoth = 64 * (SBR_NOBS + SBR_NSTATE) * (int)sizeof(OutT) <= NSLOT * 64 * (int)sizeof(double);
    if (SBR_USUAL_IF(AGAIN, kBoth && obs && state)) {
        OutT o[SBR_NOBS], sv[SBR_NSTATE];
        sbr_write_obs<OutT>(o, 1, t_obs, x, xa6, x);
        sbr_write_state<OutT>(sv, 1, t_obs, x);
#ifdef SBR_STAMPS
        asm volatile("" : "+v"(o[0]), "+v"(o[17]), "+v"(sv[14]) : : "memory");
#endif
        SBR_STAMP(12, false);                 // output values formed
        store_rows2<OutT, SBR_NOBS, SBR_NSTATE, AGAIN>(obs + i0 * SBR_NOBS, state + i0 * SBR_NSTATE, l, stage, wide, o, sv);
    } else {
        if (obs) {
            OutT o[SBR_NOBS];
            sbr_write_obs<OutT>(o, 1, t_obs, x, xa6, x);
            store_rows<OutT, SBR_NOBS>(obs + i0 * SBR_NOBS, l, stage, wide, o);
        }
        if (state) {
            OutT sv[SBR_NSTATE];
            sbr_write_state<OutT>(sv, 1, t_obs, x);
            store_rows<OutT, SBR_NSTATE>(state + i0 * SBR_NSTATE, l, stage, wide, sv);
        }
    }
    SBR_STAMP(6, false);                      // output stores issued
    SBR_STAMP(7, true);                       // every store acknowledged
}

// ------------------------------------------------------------------------------------------- per-cycle env (SBR-v2)
// SbrEnv2.reset (gym_SBR_env2.py:69-129): influent draw (scenario 0 by default, :104) and the 3-element observation built
// from the sums of start state and influent.  CARRY keeps each env's current state as the start state (x0_new, :152).
template <typename OutT, bool CARRY>
__global__ __launch_bounds__(SBR_RESET_BLOCK) void k_cycle_reset(SbrPar p, SbrBuf b, const double* __restrict__ tables,
                                                                uint64_t seed, const int32_t* __restrict__ scenario,
                                                                const double* __restrict__ rnd, const double* __restrict__ influent,
                                                                const uint8_t* __restrict__ mask, OutT* __restrict__ obs) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const bool need_tables = (influent == nullptr);
    if (need_tables) {
        stage_tables(lds, tables);
        __syncthreads();
    }
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SBR_RESET_BLOCK, i = i0 + l;
    if (i >= b.n) return;
    if (mask != nullptr && mask[i] == 0) return;
    double ld[SBR_NX], x0[SBR_NX];
    const uint64_t gid = (uint64_t)(b.first_env_id + i);
    influent_lane(lds, need_tables, pick_scenario(p, scenario, 0 /* :104 */, seed, gid, i), rnd, influent, seed, gid, i, ld);
    if (CARRY) load_x(b, i0, l, x0);
    else {
#pragma unroll
        for (int j = 0; j < SBR_NX; ++j) x0[j] = p.x0[j];
        store_x(b, i0, l, x0);
    }
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) INFL(j) = ld[j];
    CTRL(R_T) = 0.0; CTRL(R_RET) = 0.0; CTRL(R_QW) = 0.0;
    CTRL(R_META) = SbrMeta::pack({0, sbr_status_bits(p, x0), true});       // inert for sbr_step: this handle runs whole cycles
    if (obs) {
        const double cod = (x0[1] + ld[1]) + (x0[2] + ld[2]) + (x0[3] + ld[3]) + (x0[4] + ld[4]) + (x0[5] + ld[5]) +
                           (x0[6] + ld[6]) + (x0[7] + ld[7]);
        obs[i * 3 + 0] = (OutT)(x0[0] + ld[0]); obs[i * 3 + 1] = (OutT)((cod - 5145) / 10); obs[i * 3 + 2] = (OutT)((x0[10] + ld[10]) / 30);
    }
}

// the scenario draw of cfg.random_scenario, for tests and callers that want to know it
__global__ __launch_bounds__(SBR_BLOCK) void k_scenarios(SbrBuf b, uint64_t seed, int32_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * SBR_BLOCK + threadIdx.x;
    if (i < b.n) out[i] = sbr_scenario_draw(seed, (uint64_t)(b.first_env_id + i));
}

// ------------------------------------------------------------------------------------------- stats
// {sum, min, max, count} of a per-env vector: butterfly over the 64 lanes of each wave (DPP/swizzle via
// __shfl_xor), then one atomic per wave.
SBR_DEV double atomic_min_f64(double* addr, double v) {
    unsigned long long* a = reinterpret_cast<unsigned long long*>(addr);
    unsigned long long old = *a, assumed;
    do {
        assumed = old;
        if (__longlong_as_double((long long)assumed) <= v) break;
        old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(v));
    } while (assumed != old);
    return __longlong_as_double((long long)old);
}
SBR_DEV double atomic_max_f64(double* addr, double v) {
    unsigned long long* a = reinterpret_cast<unsigned long long*>(addr);
    unsigned long long old = *a, assumed;
    do {
        assumed = old;
        if (__longlong_as_double((long long)assumed) >= v) break;
        old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(v));
    } while (assumed != old);
    return __longlong_as_double((long long)old);
}

__global__ __launch_bounds__(SBR_BLOCK) void k_stats_init(double* out4) {
    if (threadIdx.x == 0) { out4[0] = 0.0; out4[1] = INFINITY; out4[2] = -INFINITY; out4[3] = 0.0; }
}

__global__ __launch_bounds__(SBR_BLOCK) void k_stats(const double* __restrict__ v, int64_t n, double* out4) {
    double s = 0.0, mn = INFINITY, mx = -INFINITY, cnt = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * SBR_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SBR_BLOCK) {
        const double a = v[i];
        s += a; mn = fmin(mn, a); mx = fmax(mx, a); cnt += 1.0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off, 64);
        mn = fmin(mn, __shfl_xor(mn, off, 64));
        mx = fmax(mx, __shfl_xor(mx, off, 64));
        cnt += __shfl_xor(cnt, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && cnt > 0.0) {      // lane 0 of EVERY wave of the workgroup publishes its wave's partials
        atomicAdd(out4 + 0, s);
        atomic_min_f64(out4 + 1, mn);
        atomic_max_f64(out4 + 2, mx);
        atomicAdd(out4 + 3, cnt);
    }
}

// ------------------------------------------------------------------------------------------- helpers
__global__ __launch_bounds__(SBR_BLOCK) void k_fill(double* __restrict__ dst, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * SBR_BLOCK + threadIdx.x;
    if (i < n) dst[i] = v;
}

__global__ __launch_bounds__(SBR_BLOCK) void k_rhs(SbrPar p, int32_t kind, int64_t n, const double* __restrict__ x,
                                                  const double* __restrict__ kla, const double* __restrict__ ec,
                                                  const double* __restrict__ loading, double* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * SBR_BLOCK + threadIdx.x;
    if (i >= n) return;
    double xv[SBR_NX], ld[SBR_NX], d[SBR_NX];
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) { xv[j] = x[i * SBR_NX + j]; ld[j] = loading ? loading[i * SBR_NX + j] : 0.0; }
    if (kind == 0) sbr_rhs<0>(p, xv, kla[i], ec[i], ld, d);
    else if (kind == 1) sbr_rhs<1>(p, xv, kla[i], 0.0, ld, d);
    else sbr_rhs<2>(p, xv, kla[i], 0.0, ld, d);
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) dx[i * SBR_NX + j] = d[j];
}

// RK4 nodes of one integration span and the right-hand side at each node (sbr_eval_substeps; trajectory export only).
// kind 0: a control interval (reaction_dxdt with Kla and EC held) - substep by substep with the dosing code path, whose flow
// terms are exact no-ops at ec == 0 (sbr_rk4), so the nodes are those sbr_step passes through, to rounding (V, Si, Xi and the
// charge balance are closed per substep here, per interval there); kind 1: the fill phase (filling_dxdt, loading vector);
// kind 2: the idle phase (idle_dxdt); kind 3: settle + draw applied to x0 first (Sim_Settling_Drawing), then the idle phase -
// node 0 is then the reactor after the draw.
__global__ __launch_bounds__(SBR_BLOCK) void k_substeps(SbrPar p, int32_t kind, int64_t n, int32_t n_sub, const double* __restrict__ x0,
                                                       const double* __restrict__ kla, const double* __restrict__ ec,
                                                       const double* __restrict__ loading, const double* __restrict__ hstep,
                                                       double* __restrict__ xs, double* __restrict__ dxs) {
    const int64_t i = (int64_t)blockIdx.x * SBR_BLOCK + threadIdx.x;
    if (i >= n) return;
    double x[SBR_NX], ld[SBR_NX], d[SBR_NX];
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) { x[j] = x0[i * SBR_NX + j]; ld[j] = (kind == 1) ? loading[i * SBR_NX + j] : 0.0; }
    if (kind == 3) {
        double sx[10], sx_eff;
        const double xf = sbr_settle(p, x, p.t_settle * p.t_cycle, sx);
        (void)sbr_draw(p, x, sx, xf, sx_eff);
    }
    const double h = hstep[i], k = kla[i], e = (kind == 0) ? ec[i] : 0.0;
    for (int s = 0; s <= n_sub; ++s) {
        if (kind == 0) sbr_rhs<0>(p, x, k, e, ld, d);
        else if (kind == 1) sbr_rhs<1>(p, x, k, 0.0, ld, d);
        else sbr_rhs<2>(p, x, k, 0.0, ld, d);
        const int64_t o = (i * ((int64_t)n_sub + 1) + s) * SBR_NX;
#pragma unroll
        for (int j = 0; j < SBR_NX; ++j) { xs[o + j] = x[j]; dxs[o + j] = d[j]; }
        if (s < n_sub) {
            if (kind == 0) sbr_rk4<1>(p, x, h, 1, k, e, ld);
            else if (kind == 1) sbr_rk4<2>(p, x, h, 1, k, ld[0], ld);
            else sbr_rk4<0>(p, x, h, 1, k, 0.0, ld);
        }
    }
}

__global__ __launch_bounds__(SBR_BLOCK) void k_normals(SbrBuf b, uint64_t seed, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * SBR_BLOCK + threadIdx.x;
    if (i >= b.n) return;
    for (uint32_t k = 0; k < SBR_NSAMP / 2; ++k) {
        double z0, z1;
        sbr_normal_pair(seed, (uint64_t)(b.first_env_id + i), k, z0, z1);
        out[i * SBR_NSAMP + 2 * k] = z0;
        out[i * SBR_NSAMP + 2 * k + 1] = z1;
    }
}

// Influent FUTURES without a reset (sbr_draw_influent): one lane per draw, the tables staged as the resets stage them, nothing of
// the handle read but its first env id.  Lane t = (r * N + i) * per_env + s is draw d = first_draw + r * per_env + s of env i: the
// reset's mix under the stream words 0 + 256 d (the normals) and 2 + 256 d (the scenario, where the caller names none), so d = 0 is
// the reset's own draw.  The row of fourteen is what sbr_cycle_reset takes as an env's influent.
__global__ __launch_bounds__(SBR_RESET_BLOCK) void k_draw_influent(SbrBuf b, const double* __restrict__ tables, uint64_t seed,
                                                                  uint32_t per_env, uint32_t first_draw, uint32_t n_draws,
                                                                  const int32_t* __restrict__ scenario, double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    stage_tables(lds, tables);
    __syncthreads();
    const uint32_t t = blockIdx.x * (uint32_t)SBR_RESET_BLOCK + threadIdx.x;      // n_draws < 2^31 (checked by the host)
    if (t >= n_draws) return;
    const uint32_t pair = t / per_env, s = t - pair * per_env, n = (uint32_t)b.n;   // pair = r * N + i
    const uint32_t r = pair / n;
    const int64_t i = (int64_t)(pair - r * n);
    const uint32_t word = 256u * (first_draw + r * per_env + s);                    // d < 2^24 (checked by the host)
    const uint64_t gid = (uint64_t)(b.first_env_id + i);
    double ld[SBR_NX];
    influent_lane(lds, true, scenario ? scenario[i] : sbr_scenario_draw(seed, gid, 2u + word), nullptr, nullptr, seed, gid, i, ld, word);
    double* mine = out + (int64_t)t * SBR_NX;
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) mine[j] = ld[j];
}

// =========================================================================================== host / C ABI
static thread_local std::string g_create_err;      // creation errors are reported per calling thread (sbr_last_error(NULL))

int fail(sbr_env* e, int code, const std::string& msg) {
    if (e) e->err = msg; else g_create_err = msg;
    return code;
}

// smallest double s with (int)(s / dt) >= rows, i.e. whose IEEE quotient by dt reaches rows: start at rows*dt and step
// through the neighbouring doubles (the quotient is monotonic in s; a handful of steps at most)
static double rows_threshold(double dt, int rows) {
    double s = (double)rows * dt;
    for (int it = 0; it < 64 && (int)(s / dt) < rows; ++it) s = std::nextafter(s, INFINITY);
    for (int it = 0; it < 64; ++it) {
        const double below = std::nextafter(s, 0.0);
        if ((int)(below / dt) < rows) break;
        s = below;
    }
    return s;
}

void derive_params(const sbr_config& c, SbrPar& p) {
    p.muH = c.muH; p.Ks = c.Ks; p.Koh = c.Koh; p.Kno = c.Kno; p.bH = c.bH; p.eta_g = c.eta_g; p.eta_h = c.eta_h;
    p.kh = c.kh; p.Kx = c.Kx; p.muA = c.muA; p.Knh = c.Knh; p.bA = c.bA; p.Koa = c.Koa; p.ka = c.ka;
    const double Yh = c.Yh, Ya = c.Ya, ixb = c.ixb, ixp = c.ixp, fp = c.fp;
    p.n2_12 = -1 / Yh; p.n4_45 = 1 - ixp; p.n7_45 = ixp;
    p.n8_1 = -(1 - Yh) / Yh; p.n8_3 = -(4.57 - Ya) / Ya;
    p.n9_2 = -((1 - Yh) / (2.86 * Yh)); p.n9_3 = 1 / Ya;
    p.n10_12 = -ixb; p.n10_3 = -ixb - 1 / Ya;
    p.n12_45 = ixb - fp * ixp;
    p.n13_1 = -ixb / 14; p.n13_2 = (1 - Yh) / (14 * 2.86 * Yh) - ixb / 14; p.n13_3 = -ixb / 14 - 1 / (7 * Ya);
    p.n13_6 = 1.0 / 14;
    p.WV = c.WV; p.IV = c.IV; p.dt = c.dt; p.t_delta = c.t_delta; p.t_cycle = c.t_cycle;
    p.T_fill = c.T_fill; p.T3_0 = c.T3_0; p.T3_end = c.T3_end; p.T4_end = c.T4_end; p.T5_end = c.T5_end;
    p.t_settle = c.t_settle; p.t_draw = c.t_draw;
    p.qin = c.WV - c.IV; p.load0 = p.qin / c.T_fill;
    p.So_sat = c.So_sat; p.Kla_min = c.Kla_min; p.Kla_max = c.Kla_max;
    p.Kc_DO = c.Kc_DO; p.KcI_DO = c.Kc_DO / c.tauI_DO; p.KcD_DO = c.Kc_DO * c.tauD_DO;
    p.EC_min = c.EC_min; p.EC_max = c.EC_max;
    p.Kc_EC = c.Kc_EC; p.KcI_EC = c.Kc_EC / c.tauI_EC; p.KcD_EC = c.Kc_EC * c.tauD_EC; p.EC_conc = c.EC_conc;
    p.act_DO_max = c.act_DO_max; p.act_EC_max = c.act_EC_max;
    p.biomass_setpoint = c.biomass_setpoint; p.Qeff = c.Qeff; p.settler_area = c.settler_area;
    p.settler_vmax = c.settler_vmax;
    memcpy(p.x0, c.x0, sizeof p.x0);
    p.f1a = c.kh / c.muH; p.f1b = c.Ks * (c.kh / c.muH);
    p.f2a = 1.0 / c.kh; p.f2b = c.Koh / c.kh;
    p.f4a = 1.0 / c.muA; p.f4b = c.Knh / c.muA;
    p.f3a = 1.0 / (c.Koh * c.eta_g); p.f3b = c.Kno / (c.Koh * c.eta_g);
    p.KohEtag = c.Koh * c.eta_g; p.etah_g = c.eta_h / c.eta_g;
    p.bA_bH = c.bA / c.bH; p.n4_45b = p.n4_45 * c.bH; p.n12_45b = p.n12_45 * c.bH; p.n7_45b = p.n7_45 * c.bH;
    p.n9_23 = p.n9_2 / p.n9_3; p.inv_n9_3 = 1.0 / p.n9_3;
    for (int k = 0; k < 8; ++k) p.t_ph[k] = c.t_cycle * c.t_ratio[k];
    p.cyc_Kc = c.cyc_Kc; p.cyc_KcI = c.cyc_Kc / c.cyc_tauI; p.cyc_KcD = c.cyc_Kc * c.cyc_tauD; p.cyc_dt = c.cyc_dt;
    p.substeps = c.substeps; p.terminal = c.terminal; p.scheme = c.scheme;
    p.inv_Koh = 1.0 / c.Koh; p.inv_Koa = 1.0 / c.Koa;
    p.fill_rows = (int)((c.T_fill - 0) / c.dt);      // int((t_end - t_start)/dt) = 252, :1588
    p.reward_kind = c.reward_kind;
    p.random_scenario = c.random_scenario;
    p.inv_dt = 1.0 / c.dt; p.inv_t_delta = 1.0 / c.t_delta; p.inv_substeps = 1.0 / (double)c.substeps;
    p.inv_cyc_dt = 1.0 / c.cyc_dt; p.h_fill = c.T_fill / (double)p.fill_rows;
    {   // module_reward_EQIOCI.py:72, :80 - Kla = 240 and EC = 0.0005 over eleven rows of its own t_delta = 0.002/24, So_sat = 8
        const double td = 0.002 / 24;
        p.inv_ae_max = 1.0 / (1.32 * (240 * 11) * td * (8 / ((td * 11) * 1.8 * 1000)));
        p.inv_ec_max = 1.0 / (c.EC_conc * (0.0005 * 11) * td / ((td * 11) * 1000));
    }
    p.rows10_min = rows_threshold(c.dt, 10); p.rows9_min = rows_threshold(c.dt, 9);
    {   // SBR-v2 phase schedule, with the reference's own operations (SBR_model_FB.py:30-258: t_start = t_end + t_delta,
        // t_end = t_start + t_phs; sub_phases_FB.py:183-184: n2 = int((t_end - t_start)/(t_delta*10)), numpy.linspace's step)
        const double t_delta = 0.002 / 24;                         // gym_SBR_env2.py:34
        double t_start = 0.0, t_end = 0.0 + p.t_ph[0];
        int slot = 0;
        for (int ph = 0; ph < 8; ++ph) {
            if (ph > 0) { t_start = t_end + t_delta; t_end = t_start + p.t_ph[ph]; }
            if (ph == 5) { p.cyc_tset = t_end - t_start; continue; }      // settle
            if (ph == 6) continue;                                         // draw
            int n2 = (int)((t_end - t_start) / (t_delta * 10));
            n2 = n2 < 2 ? 2 : (n2 > 100000 ? 100000 : n2);                 // every wave terminates
            p.cyc_t0[slot] = t_start; p.cyc_t1[slot] = t_end; p.cyc_n2[slot] = n2;
            p.cyc_step[slot] = (t_end - t_start) / (double)(n2 - 1);
            p.cyc_inv_ntd[slot] = 1.0 / ((double)(n2 - 1) * t_delta);      // module_reward.py: .../(len(Kla) * t_delta)
            p.cyc_inv_n[slot] = 1.0 / (double)(n2 - 1);
            ++slot;
        }
        p.inv_t_ph0 = 1.0 / p.t_ph[0];
        p.sosat_k = c.So_sat / (1.8 * 1000);
        p.inv_T_fill = 1.0 / c.T_fill;
    }
}

// the reset kernels of output type T, indexed by CARRY: k_reset in workgroups of BLK threads, k_cycle_reset (same arguments)
template <typename T> using ResetFn = decltype(&k_reset<T, false>);
template <typename T, int BLK> constexpr ResetFn<T> kReset[2] = {k_reset<T, false, BLK>, k_reset<T, true, BLK>};
template <typename T> constexpr ResetFn<T> kCycleReset[2] = {k_cycle_reset<T, false>, k_cycle_reset<T, true>};
template <typename T> using ResetModelsFn = decltype(&k_reset_models<T, false>);
template <typename T, int BLK> constexpr ResetModelsFn<T> kResetModels[2] = {k_reset_models<T, false, BLK>, k_reset_models<T, true, BLK>};

// What sbr_create has to say about a config; empty if it is valid.  Every check is evaluated and the LAST failing one is reported.
std::string config_error(const sbr_config& c) {
    std::string bad;
    if (c.substeps < 1 || c.substeps > 10000) bad = "substeps out of range";
    if (c.scheme < 0 || c.scheme > 1) bad = "scheme must be 0 (RK4 x substeps) or 1 (adaptive Butcher-5)";
    if (c.reserved_ != 0) bad = "reserved_ must be 0 (a caller that leaves it uninitialised could not be told from one using a later meaning)";
    if (!(c.Koa > 0 && c.Koa < 1e300)) bad = "Koa must be positive";
    if (c.reward_kind < 0 || c.reward_kind > 2) bad = "reward_kind must be 0 (EQI/OCI), 1 (G2ANET) or 2 (operating cost)";
    if (!(c.dt > 0) || !(c.t_delta > 0)) bad = "dt and t_delta must be positive";
    else {
        const int rows = (int)(c.t_delta / c.dt + 0.5);
        if (rows != 10) bad = "t_delta must be 10*dt (the reward's Kla look-back is 9 intervals)";
    }
    if (!(c.T_fill > 0) || (int)(c.T_fill / c.dt) < 1) bad = "T_fill/dt must be >= 1";
    // every reaction phase must be longer than one control interval, so that a call runs at most two intervals
    // (the reference's schedule: phases of 46, 190, 171 and 1 intervals; the last phase is open-ended)
    if (!(c.T3_0 - c.T_fill > c.t_delta) || !(c.T3_end - c.T3_0 > c.t_delta) || !(c.T4_end - c.T3_end > c.t_delta))
        bad = "phases 2, 3 and 4 must each be longer than t_delta";
    if (!(c.tauI_DO != 0) || !(c.tauI_EC != 0) || !(c.cyc_tauI != 0) || !(c.cyc_dt > 0)) bad = "tauI must be non-zero, cyc_dt positive";
    // the rate constants that are folded into the Monod denominators (sbr_rates) must be positive and finite
    if (!(c.muH > 0 && c.muH < 1e300) || !(c.muA > 0 && c.muA < 1e300) || !(c.kh > 0 && c.kh < 1e300) ||
        !(c.eta_g > 0 && c.eta_g < 1e300) || !(c.bH > 0 && c.bH < 1e300) || !(c.Ya > 0 && c.Ya < 1e300) ||
        !(c.Koh > 0 && c.Koh < 1e300))
        bad = "muH, muA, kh, eta_g, Koh, bH and Ya must be positive";
    // the dosing integrator expands 1/s, s = V/V0, to third order in s - 1 <= EC_max t_delta / V (sbr_rk4_dose): 7e-7 with
    // the reference's EC_max; refuse configurations in which the truncation (s - 1)^4 would reach 1e-16
    if (!(c.IV > 0) || !(c.WV > 0) || !(c.EC_max * c.t_delta <= 1e-4 * (c.IV < c.WV ? c.IV : c.WV)))
        bad = "EC_max * t_delta must be below 1e-4 of the reactor volume (IV, WV > 0)";
    for (int k = 0; k < 8; ++k) if (!(c.t_ratio[k] > 0)) bad = "t_ratio entries must be positive";
    return bad;
}

extern "C" {

const char* sbr_version(void) { return "sbr_amd 0.6.0 (gfx950, fp64; scheme 1 = adaptive Butcher-5, scheme 0 = RK4)"; }
int sbr_abi_version(void) { return SBR_ABI_VERSION; }

int sbr_default_config(sbr_config* c) {
    if (!c) return SBR_ERR_INVALID;
    memset(c, 0, sizeof *c);
    // SURVEY.md Appendix A; values asserted against tests/golden/constants.npz by tests/test_capi_cpu.py
    c->Ya = 0.24; c->Yh = 0.67; c->fp = 0.08; c->ixb = 0.08; c->ixp = 0.06;
    c->muH = 4.0; c->Ks = 10.0; c->Koh = 0.2; c->Kno = 0.5; c->bH = 0.3; c->eta_g = 0.8; c->eta_h = 0.8;
    c->kh = 3.0; c->Kx = 0.1; c->muA = 0.5; c->Knh = 1.0; c->bA = 0.05; c->Koa = 0.4; c->ka = 0.05;
    c->WV = 1.32; c->IV = 0.6161484733495801; c->dt = 0.002 / 24; c->t_delta = c->dt * 10; c->t_cycle = 12.0 / 24;
    c->T_fill = 0.021; c->T3_0 = 0.06416666666666668; c->T3_end = 0.2516666666666667;
    c->T4_end = 0.4085000000000001; c->T5_end = 0.40933333333333344;
    c->t_settle = 8.3 / 100; c->t_draw = 2.1 / 100;
    c->So_sat = 8.000000000006622; c->Kla_min = 0; c->Kla_max = 240; c->Kc_DO = 100; c->tauI_DO = 20; c->tauD_DO = 0;
    c->EC_min = 0; c->EC_max = 0.0005; c->Kc_EC = 100; c->tauI_EC = 20; c->tauD_EC = 0; c->EC_conc = 1200000 * 4.0;
    c->act_DO_max = 8; c->act_EC_max = 15;
    c->biomass_setpoint = 2700; c->Qeff = 0.66; c->settler_area = (1.25 / 2) * (1.25 / 2); c->settler_vmax = 474;
    static const double tr[8] = {4.2 / 100, 8.3 / 100, 37.5 / 100, 31.2 / 100, 2.1 / 100, 8.3 / 100, 2.1 / 100, 6.3 / 100};
    memcpy(c->t_ratio, tr, sizeof tr);
    c->cyc_Kc = 5.0; c->cyc_tauI = 0.00035; c->cyc_tauD = 0.005; c->cyc_dt = 0.02 / 24;      // gym_SBR_env2.py:48
    static const double x0[SBR_NX] = {0.6161484733495801, 30, 0.571098000538576, 1440.01157895393, 31.254221999137,
                                      2599.2714348941, 168.915006750837, 551.901552960823, 2.16607843793004,
                                      13.3791460027604, 0.00562880208518134, 0.35996687629947, 1.86916737961228,
                                      3.790463057094611};
    memcpy(c->x0, x0, sizeof x0);
    c->substeps = 10; c->out_f64 = 0; c->terminal = 1; c->reward_kind = 0; c->act_f64 = 0; c->random_scenario = 0;
    c->scheme = 1; c->reserved_ = 0;
    return SBR_OK;
}

int sbr_rows_thresholds(const sbr_config* cfg, double* out2) {
    if (!out2) return SBR_ERR_INVALID;
    sbr_config c;
    if (cfg) c = *cfg; else sbr_default_config(&c);
    if (!(c.dt > 0)) return SBR_ERR_INVALID;
    out2[0] = rows_threshold(c.dt, 9); out2[1] = rows_threshold(c.dt, 10);
    return SBR_OK;
}

int sbr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int sbr_create(int64_t n_envs, int device_id, int64_t first_env_id, const sbr_config* cfg, sbr_env** out) {
    if (!out) return fail(nullptr, SBR_ERR_INVALID, "sbr_create: out is NULL");
    *out = nullptr;
    if (n_envs <= 0) return fail(nullptr, SBR_ERR_INVALID, "sbr_create: n_envs must be > 0");
    int ndev = sbr_device_count();
    if (ndev <= 0)
        return fail(nullptr, SBR_ERR_NO_DEVICE, "sbr_create: no HIP device visible - this library has no CPU path");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, SBR_ERR_INVALID, "sbr_create: bad device_id");
    sbr_config c;
    if (cfg) c = *cfg; else sbr_default_config(&c);
    const std::string bad = config_error(c);
    if (!bad.empty()) return fail(nullptr, SBR_ERR_INVALID, "sbr_create: " + bad);
    // the handle is this function's until the last line: every early return below destroys it with whatever it holds by then,
    // and reports to the calling thread (HIP_TRY(nullptr, ...), sbr_last_error(NULL))
    struct Destroy { void operator()(sbr_env* p) const { sbr_destroy(p); } };
    std::unique_ptr<sbr_env, Destroy> e(new (std::nothrow) sbr_env());
    if (!e) return fail(nullptr, SBR_ERR_ALLOC, "sbr_create: out of host memory");
    e->n = n_envs; e->device = device_id; e->first_env_id = first_env_id; e->cfg = c;
    derive_params(c, e->par);
    DeviceGuard guard(device_id);
    HIP_TRY(nullptr, guard.status);
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_id));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
        return fail(nullptr, SBR_ERR_NO_DEVICE, std::string("sbr_create: device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    e->one_wave_envs = (int64_t)prop.multiProcessorCount * 4 * 64;
    const size_t nb = (size_t)n_envs * sizeof(double);
    HIP_TRY(nullptr, hipMalloc(&e->buf.x, SBR_NX * nb));
    HIP_TRY(nullptr, hipMalloc(&e->buf.ctrl, R_NROWS * nb));
    HIP_TRY(nullptr, hipMalloc(&e->buf.infl, SBR_NX * nb));
    HIP_TRY(nullptr, hipMalloc(&e->tables, 2 * kTableDoubles * sizeof(double)));
    HIP_TRY(nullptr, hipMemset(e->buf.x, 0, SBR_NX * nb));
    HIP_TRY(nullptr, hipMemset(e->buf.ctrl, 0, R_NROWS * nb));
    HIP_TRY(nullptr, hipMemset(e->buf.infl, 0, SBR_NX * nb));
    // an env is unusable until its first reset: mark everything done so that step() is a no-op until then; filled on the
    // device, no host staging buffer
    hipLaunchKernelGGL(k_fill, grid_for(n_envs), dim3(SBR_BLOCK), 0, nullptr, e->buf.ctrl + (size_t)R_META * n_envs, n_envs,
                       SbrMeta::pack({0, 0, true}));
    HIP_TRY(nullptr, hipGetLastError());
    HIP_TRY(nullptr, hipDeviceSynchronize());
    HIP_TRY(nullptr, hipEventCreate(&e->ev0));
    HIP_TRY(nullptr, hipEventCreate(&e->ev1));
    const int lds_bytes = kLdsTableDoubles * (int)sizeof(double);      // 84 KiB of dynamic LDS: above the 64 KiB default
    for (const int carry : {0, 1}) {
        const void* fns[10] = {(const void*)kReset<float, SBR_RESET_BLOCK>[carry], (const void*)kReset<double, SBR_RESET_BLOCK>[carry],
                               (const void*)kReset<float, 512>[carry], (const void*)kReset<double, 512>[carry],
                               (const void*)kCycleReset<float>[carry], (const void*)kCycleReset<double>[carry],
                               (const void*)kResetModels<float, SBR_RESET_BLOCK>[carry], (const void*)kResetModels<double, SBR_RESET_BLOCK>[carry],
                               (const void*)kResetModels<float, 512>[carry], (const void*)kResetModels<double, 512>[carry]};
        for (const void* fn : fns) HIP_TRY(nullptr, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    }
    HIP_TRY(nullptr, hipFuncSetAttribute((const void*)k_draw_influent, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    e->buf.n = n_envs; e->buf.first_env_id = first_env_id;
    *out = e.release();
    return SBR_OK;
}

int sbr_destroy(sbr_env* e) {
    if (!e) return SBR_OK;
    DeviceGuard guard(e->device);
    if (e->buf.x) (void)hipFree(e->buf.x);
    if (e->buf.ctrl) (void)hipFree(e->buf.ctrl);
    if (e->buf.infl) (void)hipFree(e->buf.infl);
    if (e->tables) (void)hipFree(e->tables);
    if (e->models) (void)hipFree(e->models);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    delete e;
    return SBR_OK;
}

const char* sbr_last_error(const sbr_env* e) { return e ? e->err.c_str() : g_create_err.c_str(); }

int sbr_query(const sbr_env* e, int32_t what, int64_t* out) {
    if (!e || !out) return SBR_ERR_INVALID;
    switch (what) {
        case SBR_Q_ONE_WAVE_ENVS: *out = e->one_wave_envs; break;
        case SBR_Q_STEP_SMALL_BATCH_ENVS: *out = SBR_SMALL_BATCH; break;
        case SBR_Q_STEP_BLOCK: *out = step_block(e); break;
        case SBR_Q_STEP_WAVES: *out = step_waves(e); break;
        case SBR_Q_STEP_TWO_WAVES_ABOVE_ENVS: *out = step_two_waves_above(e); break;
        case SBR_Q_FUSED_ONE_WAVE_MAX_ENVS: *out = fused_one_wave_max(e); break;
        case SBR_Q_ROLLOUT_WAVES: *out = fused_waves(e); break;
        case SBR_Q_RESET_BLOCK: *out = reset_block(e); break;
        case SBR_Q_SCHEME: *out = e->cfg.scheme; break;
        default: return SBR_ERR_INVALID;
    }
    return SBR_OK;
}
int64_t sbr_num_envs(const sbr_env* e) { return e ? e->n : 0; }

int sbr_set_influent_tables(sbr_env* e, const double* means, const double* stds) {
    if (!e || !means || !stds) return fail(e, SBR_ERR_INVALID, "sbr_set_influent_tables: NULL argument");
    ON_DEVICE(e);
    HIP_TRY(e, hipMemcpy(e->tables, means, kTableDoubles * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(e, hipMemcpy(e->tables + kTableDoubles, stds, kTableDoubles * sizeof(double), hipMemcpyHostToDevice));
    e->have_tables = true;
    return SBR_OK;
}

// k_reset and k_cycle_reset take the same arguments and stage the same tables; `who` is the entry point named in the message
static int reset_impl(sbr_env* e, const char* who, bool cycle, bool carry, uint64_t seed, const int32_t* scenario,
                      const double* rnd, const double* influent, const uint8_t* mask, void* obs, void* stream) {
    if (!e) return SBR_ERR_INVALID;
    if (!influent && !e->have_tables)
        return fail(e, SBR_ERR_INVALID, std::string(who) + ": no influent given and sbr_set_influent_tables was never called");
    return launched(e, [&] {
        const size_t lds = influent ? 0 : kLdsTableDoubles * sizeof(double);
        const int blk = cycle ? SBR_RESET_BLOCK : reset_block(e);
        dispatch(e, [&](auto c) {
            using T = typename decltype(c)::OutT;
            const ResetFn<T> fn = (cycle ? kCycleReset<T> : blk == 512 ? kReset<T, 512> : kReset<T, SBR_RESET_BLOCK>)[carry];
            hipLaunchKernelGGL(fn, dim3((unsigned)((e->n + blk - 1) / blk)), dim3(blk), lds, (hipStream_t)stream, e->par, e->buf,
                               e->tables, seed, scenario, rnd, influent, mask, (T*)obs);
        });
    });
}

int sbr_reset(sbr_env* e, uint64_t seed, const int32_t* scenario, const double* rnd, const double* influent,
              const uint8_t* mask, void* obs, void* stream) {
    return reset_impl(e, "sbr_reset", false, false, seed, scenario, rnd, influent, mask, obs, stream);
}

int sbr_reset_carry(sbr_env* e, uint64_t seed, const int32_t* scenario, const double* rnd, const double* influent,
                    const uint8_t* mask, void* obs, void* stream) {
    return reset_impl(e, "sbr_reset", false, true, seed, scenario, rnd, influent, mask, obs, stream);
}

int sbr_reset_models(sbr_env* e, int64_t envs_per_model, int32_t carry_over, uint64_t seed, const int32_t* scenario, const double* rnd,
                     const double* influent, const uint8_t* mask, void* obs, void* stream) {
    std::string bad;                  // every check is evaluated, the LAST failing one is reported - before anything is touched
    if (e && !influent && !e->have_tables) bad = "no influent given and sbr_set_influent_tables was never called";
    const std::string mb = models_error(e, envs_per_model);
    if (!mb.empty()) bad = mb;
    if (!e) bad = "NULL env";
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_reset_models: " + bad);
    return launched(e, [&] {
        const size_t lds = influent ? 0 : kLdsTableDoubles * sizeof(double);
        const int blk = reset_block(e);
        dispatch(e, [&](auto c) {
            using T = typename decltype(c)::OutT;
            const ResetModelsFn<T> fn = (blk == 512 ? kResetModels<T, 512> : kResetModels<T, SBR_RESET_BLOCK>)[carry_over != 0];
            hipLaunchKernelGGL(fn, dim3((unsigned)((e->n + blk - 1) / blk)), dim3(blk), lds, (hipStream_t)stream,
                               (const SbrPar*)e->models, (uint32_t)e->n_models, envs_per_model, e->buf, e->tables, seed, scenario, rnd,
                               influent, mask, (T*)obs);
        });
    });
}

int sbr_cycle_reset(sbr_env* e, uint64_t seed, const int32_t* scenario, const double* rnd, const double* influent,
                    const uint8_t* mask, int32_t carry_over, void* obs, void* stream) {
    return reset_impl(e, "sbr_cycle_reset", true, carry_over != 0, seed, scenario, rnd, influent, mask, obs, stream);
}

int sbr_draw_influent(sbr_env* e, uint64_t seed, int32_t rows, int32_t per_env, int32_t first_draw, const int32_t* scenario,
                      double* out, void* stream) {
    std::string bad;                  // every check is evaluated, the LAST failing one is reported - before anything is touched
    if (e && !scenario && !e->cfg.random_scenario)
        bad = "NULL scenario without cfg.random_scenario: SBROS-v1 and SBR-v2 fix different scenarios, name one";
    if (e && !e->have_tables) bad = "sbr_set_influent_tables was never called";
    if (rows >= 1 && per_env >= 1 && first_draw >= 0) {
        const int64_t draws = rows * (int64_t)per_env;
        if (e && (draws >= (int64_t)1 << 31 || e->n * draws >= (int64_t)1 << 31)) bad = "num_envs * rows * per_env must stay below 2^31 draws";
        if (first_draw + draws > (int64_t)1 << 24) bad = "first_draw + rows * per_env must be <= 2^24 (the draw is 24 bits of the Philox stream word)";
    }
    if (first_draw < 0) bad = "first_draw must be >= 0";
    if (rows < 1 || per_env < 1) bad = "rows and per_env must be >= 1";
    if (!out) bad = "NULL out";
    if (!e) bad = "NULL env";
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_draw_influent: " + bad);
    const int64_t n_draws = e->n * rows * (int64_t)per_env;
    return launched(e, [&] {
        hipLaunchKernelGGL(k_draw_influent, dim3((unsigned)((n_draws + SBR_RESET_BLOCK - 1) / SBR_RESET_BLOCK)), dim3(SBR_RESET_BLOCK),
                           kLdsTableDoubles * sizeof(double), (hipStream_t)stream, e->buf, e->tables, seed, (uint32_t)per_env,
                           (uint32_t)first_draw, (uint32_t)n_draws, scenario, out);
    });
}

int sbr_set_trace(sbr_env* e, double* buf, int64_t n_envs, int64_t capacity, int32_t record_width) {
    if (!e || (buf && (n_envs <= 0 || n_envs > e->n || capacity <= 0)))
        return fail(e, SBR_ERR_INVALID, "sbr_set_trace: need 0 < n_envs <= N and capacity > 0");
    if (buf && record_width != SBR_NTRACE)
        return fail(e, SBR_ERR_INVALID, "sbr_set_trace: record_width " + std::to_string(record_width) + " != SBR_NTRACE " +
                                            std::to_string(SBR_NTRACE) + " of this library (caller built against another header?)");
    e->buf.trace = buf; e->buf.n_trace = buf ? n_envs : 0; e->buf.trace_cap = buf ? capacity : 0;
    return SBR_OK;
}

int sbr_step(sbr_env* e, const void* action, void* obs, void* state, void* reward, uint8_t* done, void* stream) {
    if (!e || !action) return fail(e, SBR_ERR_INVALID, "sbr_step: NULL env or action");
    return launched(e, [&] {
        const int blk = step_block(e);
        const uint32_t flags = ((e->par.KcD_DO != 0.0 || e->par.KcD_EC != 0.0 || e->buf.trace != nullptr) ? SBR_KF_NEED_M2 : 0u) |
                               (blk == 256 ? SBR_KF_STAGGER : 0u);
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using OutT = typename C::OutT;
            using ActT = typename C::ActT;
            // scheme 0 has no two-waves build (step_waves is 1 for it)
            auto fn = k_step<OutT, ActT, 64, C::OCI, C::SCH>;
            if (blk == 256)
                fn = step_waves(e) == 2 ? k_step<OutT, ActT, 256, C::OCI, C::SCH, C::SCH == 1 ? 2 : 1> : k_step<OutT, ActT, 256, C::OCI, C::SCH>;
            hipLaunchKernelGGL(fn, dim3((unsigned)((e->n + blk - 1) / blk)), dim3(blk), 0, (hipStream_t)stream, e->buf.x, e->buf.ctrl,
                               e->buf.n, (const ActT*)action, flags, (OutT*)obs, (OutT*)state, (OutT*)reward, done, e->par, e->buf);
        });
    });
}

int sbr_reduce_stats(sbr_env* e, const double* values, int64_t n, double* out4, void* stream) {
    if (!e || !values || !out4 || n < 0) return fail(e, SBR_ERR_INVALID, "sbr_reduce_stats: bad argument");
    return launched(e, [&] {
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(k_stats_init, dim3(1), dim3(SBR_BLOCK), 0, st, out4);
        if (n > 0) {
            int64_t blocks = (n + SBR_BLOCK - 1) / SBR_BLOCK;
            if (blocks > 2048) blocks = 2048;      // grid-stride beyond 8 waves per CU
            hipLaunchKernelGGL(k_stats, dim3((unsigned)blocks), dim3(SBR_BLOCK), 0, st, values, n, out4);
        }
    });
}

int sbr_get_state(sbr_env* e, double* x, double* ctrl, void* stream) {
    if (!e) return SBR_ERR_INVALID;
    ON_DEVICE(e);
    const size_t nb = (size_t)e->n * sizeof(double);
    if (x) HIP_TRY(e, hipMemcpyAsync(x, e->buf.x, SBR_NX * nb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (ctrl) {
        hipLaunchKernelGGL(k_export, grid_for(e->n), dim3(SBR_BLOCK), 0, (hipStream_t)stream, e->par, e->buf, ctrl, -1);
        HIP_TRY(e, hipGetLastError());
    }
    return SBR_OK;
}

int sbr_set_state(sbr_env* e, const double* x, const double* ctrl, void* stream) {
    if (!e) return SBR_ERR_INVALID;
    ON_DEVICE(e);
    const size_t nb = (size_t)e->n * sizeof(double);
    if (x) {
        // a plant without controller rows: So[-1] / Sno[-1] of envs that hold them implicitly (x[8], x[9] of the OLD plant)
        // are written out first, so that replacing the plant does not replace the controllers' memories with it
        if (!ctrl) {
            hipLaunchKernelGGL(k_m1_explicit, grid_for(e->n), dim3(SBR_BLOCK), 0, (hipStream_t)stream, e->buf);
            HIP_TRY(e, hipGetLastError());
        }
        HIP_TRY(e, hipMemcpyAsync(e->buf.x, x, SBR_NX * nb, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    if (ctrl) {
        hipLaunchKernelGGL(k_import, grid_for(e->n), dim3(SBR_BLOCK), 0, (hipStream_t)stream, e->par, e->buf, ctrl);
        HIP_TRY(e, hipGetLastError());
    }
    return SBR_OK;
}

int sbr_get_ctrl_row(sbr_env* e, int32_t row, double* out, void* stream) {
    if (!e || !out || row < 0 || row >= SBR_NCTRL) return fail(e, SBR_ERR_INVALID, "sbr_get_ctrl_row: bad argument");
    ON_DEVICE(e);
    if (row == SBR_C_RETURN) {           // stored as is: a plain device-to-device copy
        HIP_TRY(e, hipMemcpyAsync(out, e->buf.ctrl + (size_t)R_RET * e->n, (size_t)e->n * sizeof(double),
                                  hipMemcpyDeviceToDevice, (hipStream_t)stream));
    } else {
        hipLaunchKernelGGL(k_export, grid_for(e->n), dim3(SBR_BLOCK), 0, (hipStream_t)stream, e->par, e->buf, out, (int)row);
        HIP_TRY(e, hipGetLastError());
    }
    return SBR_OK;
}

int sbr_get_influent(sbr_env* e, double* out, void* stream) {
    if (!e || !out) return fail(e, SBR_ERR_INVALID, "sbr_get_influent: NULL argument");
    ON_DEVICE(e);
    HIP_TRY(e, hipMemcpyAsync(out, e->buf.infl, SBR_NX * (size_t)e->n * sizeof(double), hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
    return SBR_OK;
}

int sbr_eval_rhs(sbr_env* e, int32_t kind, int64_t n, const double* x, const double* kla, const double* ec,
                 const double* loading, double* dx, void* stream) {
    if (!e || !x || !kla || !ec || !dx || kind < 0 || kind > 2 || (kind == 1 && !loading))
        return fail(e, SBR_ERR_INVALID, "sbr_eval_rhs: bad argument");
    return launched(e, [&] {
        if (n > 0)
            hipLaunchKernelGGL(k_rhs, grid_for(n), dim3(SBR_BLOCK), 0, (hipStream_t)stream, e->par, kind, n, x, kla, ec,
                               loading, dx);
    });
}

int sbr_eval_substeps(sbr_env* e, int32_t kind, int64_t n, int32_t n_sub, const double* x0, const double* kla, const double* ec,
                      const double* loading, const double* h, double* xs, double* dxs, void* stream) {
    if (!e || !x0 || !kla || !h || !xs || !dxs || n < 0 || n_sub < 1 || n_sub > (1 << 20) || kind < 0 || kind > 3 ||
        (kind == 0 && !ec) || (kind == 1 && !loading))
        return fail(e, SBR_ERR_INVALID, "sbr_eval_substeps: bad argument");
    return launched(e, [&] {
        if (n > 0)
            hipLaunchKernelGGL(k_substeps, grid_for(n), dim3(SBR_BLOCK), 0, (hipStream_t)stream, e->par, kind, n, n_sub, x0, kla, ec,
                               loading, h, xs, dxs);
    });
}

int sbr_draw_normals(sbr_env* e, uint64_t seed, double* out, void* stream) {
    if (!e || !out) return fail(e, SBR_ERR_INVALID, "sbr_draw_normals: NULL argument");
    return launched(e, [&] { hipLaunchKernelGGL(k_normals, grid_for(e->n), dim3(SBR_BLOCK), 0, (hipStream_t)stream, e->buf, seed, out); });
}

int sbr_draw_scenarios(sbr_env* e, uint64_t seed, int32_t* out, void* stream) {
    if (!e || !out) return fail(e, SBR_ERR_INVALID, "sbr_draw_scenarios: NULL argument");
    return launched(e, [&] { hipLaunchKernelGGL(k_scenarios, grid_for(e->n), dim3(SBR_BLOCK), 0, (hipStream_t)stream, e->buf, seed, out); });
}

#ifdef SBR_STAMPS
int sbr_set_stamps(sbr_env* e, unsigned long long* buf) { if (!e) return SBR_ERR_INVALID; e->buf.stamps = buf; return SBR_OK; }
#endif

int sbr_synchronize(sbr_env* e, void* stream) {
    if (!e) return SBR_ERR_INVALID;
    ON_DEVICE(e);
    HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
    return SBR_OK;
}

int sbr_timer_start(sbr_env* e, void* stream) {
    if (!e) return SBR_ERR_INVALID;
    ON_DEVICE(e);
    HIP_TRY(e, hipEventRecord(e->ev0, (hipStream_t)stream));
    return SBR_OK;
}

int sbr_timer_stop(sbr_env* e, void* stream, float* elapsed_ms) {
    if (!e || !elapsed_ms) return SBR_ERR_INVALID;
    ON_DEVICE(e);
    HIP_TRY(e, hipEventRecord(e->ev1, (hipStream_t)stream));
    HIP_TRY(e, hipEventSynchronize(e->ev1));
    HIP_TRY(e, hipEventElapsedTime(elapsed_ms, e->ev0, e->ev1));
    return SBR_OK;
}

}  // extern "C"
