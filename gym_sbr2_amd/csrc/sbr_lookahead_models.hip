// sbr_lookahead_models.hip - the step-level read-only lookahead under UNCERTAIN PLANT KINETICS, and its entry points.
//   k_models_lookahead_tape      k_lookahead_tape with the MODEL on the grid's y axis: branch (env, candidate, model) plays the
//              candidate's tape under the constants of model blockIdx.y of the table the handle owns (sbr_set_models,
//              sbr_cycle_models.hip) and not under the handle's own SbrPar (sbr_lookahead_actions_models)
//   k_models_lookahead_sampled   the same over tapes sampled in the lane (k_lookahead_sampled); a candidate is keyed by (seed,
//              global env id, k, row) and NOT by the model: all models of a candidate play one tape
//              (sbr_lookahead_sampled_models)
// Mean / worst come from k_scenario_stats of sbr_cycle_scenarios.hip through launch_scenario_stats, the winners from
// k_branch_best of sbr_tape.hip through launch_branch_best: no reduction kernel here.  A unit of its own: its 24 builds compile
// next to the parents' units instead of behind them.
#include "sbr_host.h"

// One lane per (env, candidate) PAIR q = env * fanout + candidate along x, one MODEL m = blockIdx.y per row of workgroups; the
// branch of the ABI is j = q * n_models + m.  The body is k_lookahead_tape's word for word (REPEATED and not shared, DESIGN.md
// sections 3.6 and 3.8) with `p` taken from the table: branch j returns the bits k_lookahead_tape returns for pair q on a handle
// created with model m's config that holds the env's state.
// WHY THE MODEL IS A GRID AXIS (k_cycle_lookahead_models' argument).  Every constant of the plant is wave-uniform in the parent
// and read with scalar loads.  With the model in the lane index it would be a model per LANE: some 190 doubles in vector registers
// or behind per-lane loads.  With the model in blockIdx.y the whole workgroup integrates ONE plant, at table + blockIdx.y -
// kernel arguments and blockIdx alone, scalar registers, constant address space.
// ADDRESSING.  Along x this is the parent: the env's rows (e0, el), the tape (q0, l).  Outputs go to j = q * n_models + m < 2^31
// (checked by the host): strided by n_models across the lanes - returns once per launch, rewards_out once per call.
// REGISTERS: the model's pointer is re-made at the top of every call at an offset of zero the compiler cannot
// see through (an empty asm on a scalar, on a wave-uniform path), so that constants are scalar loads inside the call and not
// registers held across the call loop.  The call then works on a COPY of the model and not through a reference to it: the copy
// is taken apart into the scalar loads of the fields the call reads, and every build issues exactly its parent build's vector
// loads; through a reference each build issued one more (two under the operating-cost reward), in the prologue, among the
// rows of the env's plant - loads the parent's build does not issue.  load_record reads only fields every model shares (T_fill, inv_t_delta).
template <typename ActT, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_models_lookahead_tape(const SbrPar* __restrict__ table, uint32_t n_models, SbrBuf b,
                                                                    int32_t n_steps, int32_t hold, uint32_t fanout, uint32_t n_pairs,
                                                                    const ActT* __restrict__ actions, double* __restrict__ returns,
                                                                    double* __restrict__ rewards_out) {
    const uint32_t l = threadIdx.x;
    const uint32_t q0u = blockIdx.x * (uint32_t)SBR_BLOCK;   // n_pairs * n_models < 2^31 (checked by the host): 32 bits hold every index
    if (q0u + l >= n_pairs) return;
    const uint32_t j = (q0u + l) * n_models + blockIdx.y;    // the branch, where its outputs go
    if (n_steps == 0) {               // no call: nothing of the state, the tape or the table is loaded
        if (returns) returns[j] = 0.0;
        return;
    }
    const SbrConstBytes model = (SbrConstBytes)(table + blockIdx.y);     // wave-uniform; blockIdx.y < n_models by the grid
    const int64_t q0 = (int64_t)q0u, n_branch = (int64_t)n_pairs * n_models;
    const uint32_t e0u = q0u / fanout;                       // wave-uniform: one scalar division per launch
    const uint32_t el = ((q0u + l) / fanout - e0u) & 511u;   // see k_lookahead_tape: el <= 256, the mask keeps row offsets in 32 bits
    const int64_t e0 = (int64_t)e0u;
    double x[SBR_NX], xa6[SBR_NXD];
    SbrX6Reg x6;                      // x6 and the ten Kla values stay in registers: see k_rollout
    SbrRewardParts rp;
    load_x(b, e0, el, x);
    SbrRecord rec;
    load_record<OCI>(*(const SbrPar*)model, b, e0, el, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    bool done = rec.meta.done;
    const ActT* row = actions + q0 * 2;            // the workgroup's part of the row in force (wave-uniform)
    ActT a0, a1;
    tape_load(row, l, a0, a1);
    int32_t left = hold;                           // calls the row in force still covers, this one included
    double acc = 0.0;
    for (int32_t s = 0; s < n_steps; ++s) {
        uint32_t z = 0;
        asm volatile("" : "+s"(z));                // wave-uniform: the call loop's own top
        const SbrPar p = *(const SbrPar*)(model + z);     // by value: see REGISTERS
        ActT n0 = a0, n1 = a1;
        if (--left == 0 && s + 1 < n_steps) {      // the next call starts a row (wave-uniform): issue its load now
            row += (int64_t)n_pairs * 2; left = hold;
            tape_load(row, l, n0, n1);
        }
        double r = 0.0;
        if (!done) {
            double t_obs;
            bool dn;
            sbr_run_intervals<SCH>(p, c, x, (double)a0, (double)a1, x6, SbrNoTrace{});
            x6.get(xa6);
            SbrHistReg hs{rec.hist};
            r = sbr_finish_step<OCI, SCH, SbrHistReg, false>(p, c, hs, x, xa6, t_obs, dn, rec.qw, rec.ksum, rp);
            acc += r;
            if (dn) done = true;
        }
        if (rewards_out) (rewards_out + (int64_t)s * n_branch)[j] = r;
        a0 = n0; a1 = n1;
    }
    if (returns) returns[j] = acc;
}

// k_lookahead_sampled's body word for word under the constants of model blockIdx.y.  The candidate is drawn per (gid, k, row) as
// there, in every row of workgroups alike - COMMON RANDOM NUMBERS: two models of a candidate differ by the plant and not by what
// they drew.  actions_out [rows][n_pairs][2] is stored by the blockIdx.y == 0 row of workgroups alone.
template <typename ActT, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_models_lookahead_sampled(const SbrPar* __restrict__ table, uint32_t n_models, SbrBuf b,
                                                                       int32_t n_steps, int32_t hold, uint32_t fanout, uint32_t n_pairs,
                                                                       const ActT* __restrict__ nominal, sbr_sampler sm,
                                                                       double* __restrict__ returns, double* __restrict__ rewards_out,
                                                                       ActT* __restrict__ actions_out) {
    const uint32_t l = threadIdx.x;
    const uint32_t q0u = blockIdx.x * (uint32_t)SBR_BLOCK;   // n_pairs * n_models < 2^31 (checked by the host): 32 bits hold every index
    if (q0u + l >= n_pairs) return;
    const uint32_t j = (q0u + l) * n_models + blockIdx.y;    // the branch, where its outputs go
    if (n_steps == 0) {               // no call: nothing of the state, the tape or the table is loaded
        if (returns) returns[j] = 0.0;
        return;
    }
    const SbrConstBytes model = (SbrConstBytes)(table + blockIdx.y);     // wave-uniform; blockIdx.y < n_models by the grid
    const int64_t q0 = (int64_t)q0u, n_branch = (int64_t)n_pairs * n_models;
    const uint32_t e0u = q0u / fanout;                       // the (e0, el) addressing of the env's rows: see k_lookahead_tape
    const uint32_t eu = (q0u + l) / fanout;
    const uint32_t el = (eu - e0u) & 511u;
    const uint32_t k = q0u + l - eu * fanout;                // the lane's candidate
    const int64_t e0 = (int64_t)e0u;
    const uint64_t gid = (uint64_t)(b.first_env_id + e0) + el;
    double x[SBR_NX], xa6[SBR_NXD];
    SbrX6Reg x6;                      // x6 and the ten Kla values stay in registers: see k_rollout
    SbrRewardParts rp;
    load_x(b, e0, el, x);
    SbrRecord rec;
    load_record<OCI>(*(const SbrPar*)model, b, e0, el, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    bool done = rec.meta.done;
    typedef typename SbrAct2<ActT>::type Act2;
    const ActT* row = nominal + e0 * 2;            // the workgroup's part of the nominal row in force (wave-uniform)
    ActT* out = actions_out && blockIdx.y == 0 ? actions_out + q0 * 2 : nullptr;      // ... and of the row of candidates it is drawn into
    ActT m0, m1, a0 = 0, a1 = 0;
    tape_load(row, el, m0, m1);
    uint32_t r = 0;                                // the launch-relative row that comes into force next
    bool draw = true;                              // this call starts a row (wave-uniform)
    int32_t left = hold;                           // calls the row in force still covers, this one included
    double acc = 0.0;
    for (int32_t s = 0; s < n_steps; ++s) {
        uint32_t z = 0;
        asm volatile("" : "+s"(z));                // wave-uniform: the call loop's own top
        const SbrPar p = *(const SbrPar*)(model + z);     // by value: see REGISTERS
        if (draw) {                                // the row comes into force: its candidate, from the pair loaded a call ago
            sbr_tape_sample<ActT>(sm, gid, k, r, m0, m1, a0, a1);
            if (out) { Act2 v; v.x = a0; v.y = a1; *reinterpret_cast<Act2*>(out + 2 * l) = v; out += (int64_t)n_pairs * 2; }
            ++r;
        }
        draw = --left == 0 && s + 1 < n_steps;     // the next call starts a row: issue its load now
        if (draw) {
            row += b.n * 2; left = hold;
            tape_load(row, el, m0, m1);
        }
        double rw = 0.0;
        if (!done) {
            double t_obs;
            bool dn;
            sbr_run_intervals<SCH>(p, c, x, (double)a0, (double)a1, x6, SbrNoTrace{});
            x6.get(xa6);
            SbrHistReg hs{rec.hist};
            rw = sbr_finish_step<OCI, SCH, SbrHistReg, false>(p, c, hs, x, xa6, t_obs, dn, rec.qw, rec.ksum, rp);
            acc += rw;
            if (dn) done = true;
        }
        if (rewards_out) (rewards_out + (int64_t)s * n_branch)[j] = rw;
    }
    if (returns) returns[j] = acc;
}

// ------------------------------------------------------------------------------------------- host
// What the two entry points add to their parents' refusals (lookahead_error, lookahead_sampled_error: shared through sbr_host.h,
// given no best_* - here the winner is reduced from the means).  Like the checks around them they overwrite `bad` where they fail:
// of all the checks of an entry point the LAST failing one is reported.  models_outputs_error goes in front of the parent's
// checks, models_table_error behind them.
static void models_outputs_error(std::string& bad, const sbr_env* e, int32_t fanout, const double* returns, const double* mean_out,
                                 const double* worst_out, const int32_t* best_index, const double* best_value) {
    if ((best_index || best_value) && !mean_out) bad = "best_index / best_value are reduced from mean_out: give mean_out with them";
    if ((mean_out || worst_out) && !returns) bad = "mean_out / worst_out are reduced from returns: give returns with them";
    if (e && fanout >= 1 && e->n_models >= 1 && e->n * (int64_t)fanout < (int64_t)1 << 31 &&
        e->n * (int64_t)fanout * e->n_models >= (int64_t)1 << 31)
        bad = "num_envs * fanout * n_models must stay below 2^31 branches";
}
static void models_table_error(std::string& bad, const sbr_env* e) {
    if (e && e->n_models > 65535) bad = "the table must hold <= 65535 models (the models are the grid's y axis)";
    if (e && e->n_models < 1) bad = "no model table: call sbr_set_models first";
    if (!e) bad = "NULL env";
}

extern "C" {

int sbr_lookahead_actions_models(sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* actions, double* returns,
                                 double* rewards_out, double* mean_out, double* worst_out, int32_t* best_index, double* best_value,
                                 void* stream) {
    std::string bad;                  // every check is evaluated, the LAST failing one is reported - before anything is touched
    models_outputs_error(bad, e, fanout, returns, mean_out, worst_out, best_index, best_value);
    const std::string pb = lookahead_error(e, n_steps, hold, fanout, actions, returns, nullptr, nullptr);
    if (!pb.empty()) bad = pb;
    models_table_error(bad, e);
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_lookahead_actions_models: " + bad);
    const int64_t pairs = e->n * (int64_t)fanout;
    const int32_t n_models = (int32_t)e->n_models;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused_models<C::SCH>(e, pairs, n_models, stream,
                                        [](auto w) { return k_models_lookahead_tape<A, C::OCI, C::SCH, decltype(w)::value>; }, n_steps,
                                        hold, (uint32_t)fanout, (uint32_t)pairs, (const A*)actions, returns, rewards_out);
        });
        launch_scenario_stats(returns, pairs, n_models, mean_out, worst_out, stream);
        launch_branch_best(e, fanout, mean_out, best_index, best_value, stream);
    });
}

int sbr_lookahead_sampled_models(sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* nominal,
                                 const sbr_sampler* sampler, double* returns, double* rewards_out, double* mean_out, double* worst_out,
                                 int32_t* best_index, double* best_value, void* actions_out, void* stream) {
    std::string bad;                  // every check is evaluated, the LAST failing one is reported - before anything is touched
    models_outputs_error(bad, e, fanout, returns, mean_out, worst_out, best_index, best_value);
    const std::string pb = lookahead_sampled_error(e, n_steps, hold, fanout, nominal, sampler, returns, nullptr, nullptr);
    if (!pb.empty()) bad = pb;
    models_table_error(bad, e);
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_lookahead_sampled_models: " + bad);
    const int64_t pairs = e->n * (int64_t)fanout;
    const int32_t n_models = (int32_t)e->n_models;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused_models<C::SCH>(e, pairs, n_models, stream,
                                        [](auto w) { return k_models_lookahead_sampled<A, C::OCI, C::SCH, decltype(w)::value>; }, n_steps,
                                        hold, (uint32_t)fanout, (uint32_t)pairs, (const A*)nominal, *sampler, returns, rewards_out,
                                        (A*)actions_out);
        });
        launch_scenario_stats(returns, pairs, n_models, mean_out, worst_out, stream);
        launch_branch_best(e, fanout, mean_out, best_index, best_value, stream);
    });
}

}  // extern "C"
