// sbr_cycle_models.hip - the per-cycle lookahead under UNCERTAIN PLANT KINETICS: futures over models, and the handle's model table.
//   k_cycle_lookahead_models   k_cycle_lookahead_scenarios with the FUTURE on the grid's y axis and the constants of future s read
//              from model s % n_models of a table the handle owns (sbr_set_models) and not from the handle's own SbrPar; the
//              influent futures optional (sbr_cycle_lookahead_models; mean / worst come from k_scenario_stats of
//              sbr_cycle_scenarios.hip through launch_scenario_stats, the winners from k_branch_best of sbr_tape.hip through
//              launch_branch_best)
//   sbr_check_model, sbr_set_models, sbr_num_models   which configs may stand in such a table, and the table itself
#include <cstddef>
#include <vector>

#include "sbr_host.h"

// One lane per (env, candidate) PAIR q = env * fanout + candidate along x, one FUTURE s = blockIdx.y per row of workgroups; the
// branch of the ABI is j = q * n_scen + s.  A cycle is k_cycle's body word for word under the constants of model s % n_models and
// ld[1..13] = entries 1..13 of influent[c][env * n_scen + s] - or, with influent NULL, of the env's stored influent
// (k_cycle_lookahead's rule): the bits of sbr_cycle_reset(carry_over = 1, influent = that row) followed by sbr_cycle_step on an env
// holding the branch's state, on a handle created with that model's config.
// WHY THE FUTURE IS A GRID AXIS.  Every constant of the model is wave-uniform in k_cycle and read with scalar loads.  With the
// future in the lane index (k_cycle_lookahead_scenarios' layout) a model per future would be a model per LANE: some 190 doubles in
// vector registers or behind per-lane loads.  With the future in blockIdx.y the whole workgroup integrates ONE plant: the model's
// address is table + blockIdx.y % n_models, formed from kernel arguments and blockIdx alone - scalar registers, constant address
// space - and the cycle reads its constants exactly as the sibling kernels read theirs, through another pointer.
// ADDRESSING.  Along x this is k_cycle_lookahead: the plant (e0, el), the tape row q itself (q0, l) - no division by n_scen.  The
// influent row env * n_scen + s: base the row of the workgroup's first env in this future, (e0 * n_scen + s), offset el * n_scen
// rows (el <= 256, n_scen <= 65535: 32 bits; widened to 64 before it is scaled by the row of fourteen doubles).  Every output is
// written at j = q * n_scen + s < 2^31: strided by n_scen across the lanes, a handful of stores per cycle of milliseconds.
// REGISTERS: every measure of k_cycle_lookahead (the comment there) - the lane index through an empty asm per
// cycle, the constants through a pointer re-made per cycle at an offset of zero the compiler cannot see through (here the model's
// address and not the kernel-argument segment's; the asm sits at the top of the loop, a wave-uniform path, so the offset is a
// scalar), the sum and the status bits parked in LDS, no fetch ahead, the end rows stored inside the last cycle.
template <typename ActT, int SCH>
SBR_DEV void sbr_cycle_models_branch(const SbrPar* __restrict__ table, uint32_t n_models, SbrBuf b, int32_t n_cycles, uint32_t fanout,
                                     uint32_t n_scen, uint32_t n_pairs, const ActT* __restrict__ actions,
                                     const double* __restrict__ influent, double* __restrict__ returns, double* __restrict__ rewards_out,
                                     double* __restrict__ obs_end, double* __restrict__ diag_end, uint8_t* __restrict__ status_out) {
    __shared__ double park_acc[SBR_BLOCK];                   // each lane its own slot: no barrier anywhere
    __shared__ int park_st[SBR_BLOCK];
    const uint32_t l = threadIdx.x;
    const uint32_t q0u = blockIdx.x * (uint32_t)SBR_BLOCK;   // n_pairs * n_scen < 2^31 (checked by the host): 32 bits hold every index
    const uint32_t s = blockIdx.y;                           // the future: wave-uniform, < n_scen by the grid
    if (q0u + l >= n_pairs) return;
    double acc = 0.0;
    if (n_cycles > 0) {               // no cycle: nothing of the state, the tape, the futures or the table is loaded
        const SbrConstBytes model = (SbrConstBytes)(table + s % n_models);   // wave-uniform: one scalar division per launch
        const uint32_t e0u = q0u / fanout;                       // wave-uniform
        const int64_t e0 = (int64_t)e0u, q0 = (int64_t)q0u;
        const int64_t n_branch = (int64_t)n_pairs * n_scen, infl_stride = (int64_t)(n_pairs / fanout) * n_scen * SBR_NX;
        double x[SBR_NX];
        load_x(b, e0, cycle_env_of(q0u + l, fanout, e0u), x);
        park_acc[l] = 0.0;
        park_st[l] = sbr_status_bits(*(const SbrPar*)model, x);  // a later cycle starts where the one before it ended
        const ActT* row = actions + q0 * 3;                      // the workgroup's part of the row in force (wave-uniform)
        const double* fut = influent ? influent + (e0 * (int64_t)n_scen + s) * SBR_NX : nullptr;
        for (int32_t c = 0; c < n_cycles; ++c) {
            const bool last = c + 1 == n_cycles;                 // wave-uniform
            uint32_t lc = l, z = 0;
            asm volatile("" : "+v"(lc), "+s"(z) : : "memory");
            lc &= SBR_BLOCK - 1u;
            const SbrPar& pc = *(const SbrPar*)(model + z);
            ActT a0, a1, a2;
            cycle_row_load(row, lc, a0, a1, a2);
            row += (int64_t)n_pairs * 3;
            double ld[SBR_NX], o3[3];
            const uint32_t el = cycle_env_of(q0u + lc, fanout, e0u);
            if (fut) {                // wave-uniform: the caller's future, one lane address for the thirteen loads
                const double* mine = fut + (uint64_t)(el * n_scen) * SBR_NX;
#pragma unroll
                for (int q = 1; q < SBR_NX; ++q) ld[q] = mine[q];
                fut += infl_stride;
            } else {                  // the env's stored influent, as k_cycle_lookahead reads it
#pragma unroll
                for (int q = 1; q < SBR_NX; ++q) ld[q] = (b.infl + ((int64_t)q * b.n + e0))[el];
            }
            ld[0] = (pc.WV - x[0]) * pc.inv_t_ph0;               // as in k_cycle
            const uint32_t j = (q0u + lc) * n_scen + s;          // the branch, where its outputs go
            const double r = sbr_cycle_env<SCH>(pc, x, ld, (double)a0, (double)a1, (double)a2, o3,
                                               diag_end && last ? diag_end + (uint64_t)j * SBR_NCYC_DIAG : nullptr, 1);
            park_acc[lc] = park_acc[lc] + r;
            park_st[lc] |= sbr_status_bits(pc, x);
            if (rewards_out) (rewards_out + (int64_t)c * n_branch)[j] = r;
            if (obs_end && last) {
                double* mine = obs_end + (uint64_t)j * SBR_NCYC_OBS;
                mine[0] = o3[0]; mine[1] = o3[1]; mine[2] = o3[2];
            }
        }
        acc = park_acc[l];
        if (status_out) status_out[(q0u + l) * n_scen + s] = (uint8_t)park_st[l];
    }
    if (returns) returns[(q0u + l) * n_scen + s] = acc;
}
#define SBR_CYCLE_MODELS_PARAMS(ActT)                                                                                              \
    const SbrPar* __restrict__ table, uint32_t n_models, SbrBuf b, int32_t n_cycles, uint32_t fanout, uint32_t n_scen,           \
        uint32_t n_pairs, const ActT* __restrict__ actions, const double* __restrict__ influent, double* __restrict__ returns,   \
        double* __restrict__ rewards_out, double* __restrict__ obs_end, double* __restrict__ diag_end, uint8_t* __restrict__ status_out
// the kernel and its two-waves specialisations: SBR_CYCLE_KERNEL (sbr_host.h).  The table comes first here and the constants are
// read through it, so there is no first parameter to assert.
SBR_CYCLE_KERNEL(k_cycle_lookahead_models, sbr_cycle_models_branch, SBR_CYCLE_MODELS_PARAMS, table, n_models, b, n_cycles, fanout, n_scen,
                 n_pairs, actions, influent, returns, rewards_out, obs_end, diag_end, status_out)

// ---------------------------------------------------------------------------------------------- which configs are models
// sbr_config in declaration order, cut into the MODEL FIELDS - kinetics, stoichiometry, oxygen saturation: what a model of the
// table may change - and everything else, which picks a template build, a loop count or a schedule the handle has fixed.
#define SBR_CFG_FIELD(f) {#f, offsetof(sbr_config, f), sizeof(sbr_config::f)}
struct SbrCfgField { const char* name; size_t off, size; };
static constexpr SbrCfgField kModelFields[] = {
    SBR_CFG_FIELD(Ya), SBR_CFG_FIELD(Yh), SBR_CFG_FIELD(fp), SBR_CFG_FIELD(ixb), SBR_CFG_FIELD(ixp), SBR_CFG_FIELD(muH),
    SBR_CFG_FIELD(Ks), SBR_CFG_FIELD(Koh), SBR_CFG_FIELD(Kno), SBR_CFG_FIELD(bH), SBR_CFG_FIELD(eta_g), SBR_CFG_FIELD(eta_h),
    SBR_CFG_FIELD(kh), SBR_CFG_FIELD(Kx), SBR_CFG_FIELD(muA), SBR_CFG_FIELD(Knh), SBR_CFG_FIELD(bA), SBR_CFG_FIELD(Koa),
    SBR_CFG_FIELD(ka), SBR_CFG_FIELD(So_sat)};
static constexpr SbrCfgField kFixedFields[] = {
    SBR_CFG_FIELD(WV), SBR_CFG_FIELD(IV), SBR_CFG_FIELD(dt), SBR_CFG_FIELD(t_delta), SBR_CFG_FIELD(t_cycle), SBR_CFG_FIELD(T_fill),
    SBR_CFG_FIELD(T3_0), SBR_CFG_FIELD(T3_end), SBR_CFG_FIELD(T4_end), SBR_CFG_FIELD(T5_end), SBR_CFG_FIELD(t_settle),
    SBR_CFG_FIELD(t_draw), SBR_CFG_FIELD(Kla_min), SBR_CFG_FIELD(Kla_max), SBR_CFG_FIELD(Kc_DO), SBR_CFG_FIELD(tauI_DO),
    SBR_CFG_FIELD(tauD_DO), SBR_CFG_FIELD(EC_min), SBR_CFG_FIELD(EC_max), SBR_CFG_FIELD(Kc_EC), SBR_CFG_FIELD(tauI_EC),
    SBR_CFG_FIELD(tauD_EC), SBR_CFG_FIELD(EC_conc), SBR_CFG_FIELD(act_DO_max), SBR_CFG_FIELD(act_EC_max),
    SBR_CFG_FIELD(biomass_setpoint), SBR_CFG_FIELD(Qeff), SBR_CFG_FIELD(settler_area), SBR_CFG_FIELD(settler_vmax),
    SBR_CFG_FIELD(t_ratio), SBR_CFG_FIELD(cyc_Kc), SBR_CFG_FIELD(cyc_tauI), SBR_CFG_FIELD(cyc_tauD), SBR_CFG_FIELD(cyc_dt),
    SBR_CFG_FIELD(x0), SBR_CFG_FIELD(substeps), SBR_CFG_FIELD(out_f64), SBR_CFG_FIELD(terminal), SBR_CFG_FIELD(reward_kind),
    SBR_CFG_FIELD(act_f64), SBR_CFG_FIELD(random_scenario), SBR_CFG_FIELD(scheme), SBR_CFG_FIELD(reserved_)};
constexpr size_t cfg_bytes(const SbrCfgField* f, size_t n) { return n == 0 ? 0 : f[0].size + cfg_bytes(f + 1, n - 1); }
// the two lists cover the struct: a field added to sbr_config has to be put into one of them
static_assert(cfg_bytes(kModelFields, sizeof kModelFields / sizeof *kModelFields) +
                      cfg_bytes(kFixedFields, sizeof kFixedFields / sizeof *kFixedFields) == sizeof(sbr_config),
              "kModelFields and kFixedFields name every field of sbr_config");

// What keeps `m` out of a model table over `base`; empty if it may stand there.  The first field (in the order of the struct) in
// which m differs from base outside the model fields, by its bytes; for a config that differs in model fields only, config_error.
static std::string model_error(const sbr_config& base, const sbr_config& m) {
    for (const SbrCfgField& f : kFixedFields) {
        const char *u = (const char*)&base + f.off, *v = (const char*)&m + f.off;
        if (memcmp(u, v, f.size) == 0) continue;
        std::string name = f.name;
        if (f.size > sizeof(double))                             // t_ratio, x0: name the entry
            for (size_t k = 0; k < f.size / sizeof(double); ++k)
                if (memcmp(u + k * sizeof(double), v + k * sizeof(double), sizeof(double)) != 0) {
                    name += "[" + std::to_string(k) + "]";
                    break;
                }
        return name + " differs from the base config: a model may change Ya, Yh, fp, ixb, ixp, the fourteen rate constants muH .. ka and "
                      "So_sat, and nothing else";
    }
    return config_error(m);
}

// The rule of sbr_reset_models / sbr_collect_policy_models on this handle.  With more than one model a wave must never hold two:
// the population rule of policy_error - blocks of a multiple of 256 envs, counted from a first env id that is one.
std::string models_error(const sbr_env* e, int64_t envs_per_model) {
    std::string bad;
    if (!e) return bad;
    if (e->n_models > 1) {
        if (e->first_env_id < 0 || e->first_env_id % SBR_BLOCK != 0)
            bad = "with more than one model the handle's first_env_id must be a non-negative multiple of 256";
        if (envs_per_model < SBR_BLOCK || envs_per_model % SBR_BLOCK != 0)
            bad = "with more than one model envs_per_model must be a positive multiple of 256";
    }
    if (e->n_models < 1) bad = "no model table: call sbr_set_models first";
    return bad;
}

extern "C" {

int sbr_check_model(const sbr_config* base, const sbr_config* model) {
    if (!model) return fail(nullptr, SBR_ERR_INVALID, "sbr_check_model: NULL model");
    sbr_config b;
    if (base) b = *base; else sbr_default_config(&b);
    const std::string bad = model_error(b, *model);
    if (!bad.empty()) return fail(nullptr, SBR_ERR_INVALID, "sbr_check_model: " + bad);
    return SBR_OK;
}

int sbr_set_models(sbr_env* e, int32_t n_models, const sbr_config* models) {
    std::string bad;                  // every check is evaluated, the LAST failing one is reported - before anything is touched
    if (e && models)
        for (int32_t m = 0; m < n_models; ++m) {
            const std::string why = model_error(e->cfg, models[m]);
            if (!why.empty()) bad = "models[" + std::to_string(m) + "]: " + why;
        }
    if (!models && n_models > 0) bad = "NULL models with n_models > 0";
    if (n_models < 0) bad = "n_models must be >= 0";
    if (!e) bad = "NULL env";
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_set_models: " + bad);
    ON_DEVICE(e);
    SbrPar* table = nullptr;
    if (n_models > 0) {
        std::vector<SbrPar> host((size_t)n_models);
        memset((void*)host.data(), 0, host.size() * sizeof(SbrPar));
        for (int32_t m = 0; m < n_models; ++m) derive_params(models[m], host[(size_t)m]);
        HIP_TRY(e, hipMalloc(&table, host.size() * sizeof(SbrPar)));
        const hipError_t copied = hipMemcpy(table, host.data(), host.size() * sizeof(SbrPar), hipMemcpyHostToDevice);
        if (copied != hipSuccess) {
            (void)hipFree(table);
            return hip_fail(e, copied, "hipMemcpy(model table)");
        }
    }
    if (e->models) {                  // a launch that reads the old table may still be in flight on any stream
        const hipError_t idle = hipDeviceSynchronize();
        if (idle != hipSuccess) {
            if (table) (void)hipFree(table);
            return hip_fail(e, idle, "hipDeviceSynchronize()");
        }
        (void)hipFree(e->models);
    }
    e->models = table; e->n_models = n_models;
    return SBR_OK;
}

int64_t sbr_num_models(const sbr_env* e) {
    if (!e) return fail(nullptr, SBR_ERR_INVALID, "sbr_num_models: NULL env");
    return e->n_models;
}

int sbr_cycle_lookahead_models(sbr_env* e, int32_t n_cycles, int32_t fanout, int32_t n_scen, const void* actions,
                               const double* influent, double* returns, double* rewards_out, double* mean_out, double* worst_out,
                               int32_t* best_index, double* best_value, double* obs_end, double* diag_end, uint8_t* status_out,
                               void* stream) {
    const std::string bad = cycle_lookahead_error(e, n_cycles, fanout, &n_scen, 65535, actions, false, influent, true, returns, true, mean_out,
                                                  worst_out, best_index, best_value, obs_end || diag_end || status_out);
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_cycle_lookahead_models: " + bad);
    const int64_t pairs = e->n * (int64_t)fanout;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused_models<C::SCH>(e, pairs, n_scen, stream, [](auto w) { return k_cycle_lookahead_models<A, C::SCH, decltype(w)::value>; },
                                        n_cycles, (uint32_t)fanout, (uint32_t)n_scen, (uint32_t)pairs, (const A*)actions, influent, returns,
                                        rewards_out, obs_end, diag_end, status_out);
        });
        launch_stats_and_best(e, fanout, n_scen, returns, mean_out, worst_out, best_index, best_value, stream);
    });
}

}  // extern "C"
