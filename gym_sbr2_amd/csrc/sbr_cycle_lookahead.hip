// sbr_cycle_lookahead.hip - the per-cycle env SBR-v2 as a read-only fan-out, and its entry point.
//   k_cycle_lookahead   k_cycle over `fanout` candidate tapes of n_cycles whole cycles per env, each played from the env's current
//              state and stored influent, nothing of the handle written (sbr_cycle_lookahead; the winners come from k_branch_best
//              of sbr_tape.hip through launch_branch_best)
//   cycle_lookahead_error   the one argument check of the three cycle lookaheads (this unit, sbr_cycle_scenarios.hip,
//              sbr_cycle_models.hip); their kernel wrapper and reduce tail are sbr_host.h's
#include "sbr_host.h"

// The env's stored influent, addressed like its plant: (i0, l) = (first env of the workgroup, the lane's env minus it).
SBR_DEV void load_influent(const SbrBuf& b, int64_t i0, uint32_t l, double (&ld)[SBR_NX]) {
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) ld[j] = INFL(j);
}

// k_cycle as a READ-ONLY fan-out over whole cycles (sbr_cycle_lookahead).  One lane per BRANCH j = env * fanout + candidate.  A
// cycle is k_cycle's body word for word - the influent row, ld[0] from the branch's own volume, sbr_cycle_env - so cycle 0 of
// branch j returns the bits sbr_cycle_step returns for an env holding a copy of that state, and cycle c > 0 the bits of
// sbr_cycle_reset(carry_over = 1, influent = the env's own) followed by sbr_cycle_step: that reset keeps x (the state after the
// aerated idle), stores the influent it was given and touches nothing else the step reads.
// What is NOT here, and why that changes no returned bit: store_x, the R_RET / R_T / R_META rows and the influent store of the
// reset - they only feed the handle, and the next cycle of a branch reads its x from registers.
// Addressing is sbr_lookahead_tape's (sbr_tape.hip): (e0, el) for the env's rows, (j0, l) for the tape and every output.
// REGISTERS.  The yardstick is k_cycle's build of the same scheme and waves (tests/test_cycle_lookahead_cpu.py), and a loop
// around a whole cycle is where the compiler hoists: written plainly the one-wave build took 314 registers against k_cycle's 278
// and the two-waves build 240 B of scratch against 92 - the 64-bit lane addresses of the thirteen influent rows, the status
// thresholds, every product of two constants, all computed once in front of the loop and then live through every Butcher-5 step
// loop of every phase.  What keeps a cycle of this loop as cheap as k_cycle (DESIGN.md 3.9 has each step's numbers):
//  * the lane index is passed through an empty asm at the top of every cycle, so lane addresses are formed where they are used;
//  * the constants are read through the kernel-argument segment at an offset of zero the compiler cannot see through (SbrPar is
//    the FIRST argument, as in every kernel launch_fused launches): a scalar load of a constant is then part of the cycle, as
//    it is in k_cycle, and not a register held across the loop;
//  * the influent is read again at the top of every cycle: only the fill phase reads ld[1..13], thirteen L2 hits per 528
//    intervals against 26 registers; el is divided out again with it;
//  * the running sum and the status bits wait in LDS (each lane its own slot) while a cycle is integrated;
//  * the end rows leave inside the last cycle (wave-uniform test): behind the loop they would be loop-carried registers;
//  * the row of cycle c + 1 is NOT fetched ahead of cycle c as the tape kernels fetch theirs: three or six more registers held
//    through the cycle (five in the scheme-0 build, which put it above k_cycle's 225) to hide one load in front of some
//    milliseconds.
// The body is a device function and not the kernel because one build carries an attribute of its own (SBR_CYCLE_KERNEL); p and b by value,
// as in sbr_lookahead_tape.
template <typename ActT, int SCH>
SBR_DEV void sbr_cycle_lookahead_branch(SbrPar p, SbrBuf b, int32_t n_cycles, uint32_t fanout, uint32_t n_branch,
                                        const ActT* __restrict__ actions, double* __restrict__ returns, double* __restrict__ rewards_out,
                                        double* __restrict__ obs_end, double* __restrict__ diag_end, uint8_t* __restrict__ status_out) {
    __shared__ double park_acc[SBR_BLOCK];                   // each lane its own slot: no barrier anywhere
    __shared__ int park_st[SBR_BLOCK];
    const uint32_t l = threadIdx.x;
    const uint32_t j0u = blockIdx.x * (uint32_t)SBR_BLOCK;   // n_branch < 2^31 (checked by the host): 32 bits hold every branch index
    if (j0u + l >= n_branch) return;
    const int64_t j0 = (int64_t)j0u;
    double acc = 0.0;
    if (n_cycles > 0) {               // no cycle: nothing of the state is loaded
        const uint32_t e0u = j0u / fanout;                       // wave-uniform: one scalar division per launch
        const int64_t e0 = (int64_t)e0u;
        double x[SBR_NX];
        load_x(b, e0, cycle_env_of(j0u + l, fanout, e0u), x);
        park_acc[l] = 0.0;
        park_st[l] = sbr_status_bits(p, x);                      // a later cycle starts where the one before it ended
        const ActT* row = actions + j0 * 3;                      // the workgroup's part of the row in force (wave-uniform)
        for (int32_t c = 0; c < n_cycles; ++c) {
            const bool last = c + 1 == n_cycles;                 // wave-uniform
            uint32_t lc = l, z = 0;
            asm volatile("" : "+v"(lc), "+s"(z) : : "memory");
            lc &= SBR_BLOCK - 1u;
            const SbrPar& pc = *(const SbrPar*)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + z);
            ActT a0, a1, a2;
            cycle_row_load(row, lc, a0, a1, a2);
            row += (int64_t)n_branch * 3;
            double ld[SBR_NX], o3[3];
            load_influent(b, e0, cycle_env_of(j0u + lc, fanout, e0u), ld);
            ld[0] = (pc.WV - x[0]) * pc.inv_t_ph0;               // as in k_cycle
            const double r = sbr_cycle_env<SCH>(pc, x, ld, (double)a0, (double)a1, (double)a2, o3,
                                               diag_end && last ? diag_end + j0 * SBR_NCYC_DIAG + lc * (uint32_t)SBR_NCYC_DIAG : nullptr, 1);
            park_acc[lc] = park_acc[lc] + r;
            park_st[lc] |= sbr_status_bits(pc, x);
            if (rewards_out) (rewards_out + ((int64_t)c * n_branch + j0))[lc] = r;
            if (obs_end && last) {
                double* mine = obs_end + j0 * SBR_NCYC_OBS + lc * (uint32_t)SBR_NCYC_OBS;
                mine[0] = o3[0]; mine[1] = o3[1]; mine[2] = o3[2];
            }
        }
        acc = park_acc[l];
        if (status_out) (status_out + j0)[l] = (uint8_t)park_st[l];
    }
    if (returns) (returns + j0)[l] = acc;
}
#define SBR_CYCLE_LOOKAHEAD_PARAMS(ActT)                                                                                          \
    SbrPar p, SbrBuf b, int32_t n_cycles, uint32_t fanout, uint32_t n_branch, const ActT* __restrict__ actions,                  \
        double* __restrict__ returns, double* __restrict__ rewards_out, double* __restrict__ obs_end, double* __restrict__ diag_end, \
        uint8_t* __restrict__ status_out
// the kernel, its two-waves specialisations and why they exist, and the assert on its first parameter: sbr_host.h
SBR_CYCLE_KERNEL_PAR_FIRST(k_cycle_lookahead, sbr_cycle_lookahead_branch, SBR_CYCLE_LOOKAHEAD_PARAMS, p, b, n_cycles, fanout, n_branch,
                           actions, returns, rewards_out, obs_end, diag_end, status_out)

// What the three cycle lookaheads have to say about their arguments; empty if they are valid.  Every check is evaluated and the
// LAST failing one is reported - all of them before anything is touched - so the order of this list is the precedence between
// simultaneous faults, for all three: a NULL env last, a missing table just before it.  What varies between the entry points:
//   n_scen         NULL where a branch is (env, candidate) and there are no futures (sbr_cycle_lookahead); max_scen its upper
//                  bound, 0 for none (65535 where the futures are the grid's y axis: sbr_cycle_lookahead_models)
//   need_influent  the futures' influent is the only one there is (sbr_cycle_lookahead_scenarios)
//   need_table     the futures run under the handle's model table (sbr_cycle_lookahead_models)
//   best_of_means  the winners are reduced from mean_out and not from returns (both entry points with futures)
//   end_rows       obs_end, diag_end or status_out was asked for
std::string cycle_lookahead_error(const sbr_env* e, int32_t n_cycles, int32_t fanout, const int32_t* n_scen, int32_t max_scen,
                                  const void* actions, bool need_influent, const void* influent, bool need_table, const double* returns,
                                  bool best_of_means, const double* mean_out, const double* worst_out, const int32_t* best_index,
                                  const double* best_value, bool end_rows) {
    std::string bad;
    if (!best_of_means) best_error(bad, returns, best_index, best_value);
    else if ((best_index || best_value) && !mean_out) bad = "best_index / best_value are reduced from mean_out: give mean_out with them";
    if ((mean_out || worst_out) && !returns) bad = "mean_out / worst_out are reduced from returns: give returns with them";
    if (n_cycles == 0 && end_rows) bad = "n_cycles = 0 has no last cycle for obs_end, diag_end or status_out";
    if (need_influent && !influent && n_cycles > 0) bad = "NULL influent with n_cycles > 0";
    if (!actions && n_cycles > 0) bad = "NULL actions with n_cycles > 0";
    if (e && n_scen && fanout >= 1 && *n_scen >= 1 && e->n * (int64_t)fanout < (int64_t)1 << 31 &&
        e->n * (int64_t)fanout * *n_scen >= (int64_t)1 << 31)
        bad = "num_envs * fanout * n_scen must stay below 2^31 branches";
    fanout_error(bad, e, fanout, nullptr);
    if (n_scen && max_scen && *n_scen > max_scen) bad = "n_scen must be <= " + std::to_string(max_scen) + " (the futures are the grid's y axis)";
    if (n_scen && *n_scen < 1) bad = "n_scen must be >= 1";
    if (n_cycles < 0) bad = "n_cycles must be >= 0";
    if (need_table && e && e->n_models < 1) bad = "no model table: call sbr_set_models first";
    if (!e) bad = "NULL env";
    return bad;
}

extern "C" {

int sbr_cycle_lookahead(sbr_env* e, int32_t n_cycles, int32_t fanout, const void* actions, double* returns, double* rewards_out,
                        int32_t* best_index, double* best_return, double* obs_end, double* diag_end, uint8_t* status_out,
                        void* stream) {
    const std::string bad = cycle_lookahead_error(e, n_cycles, fanout, nullptr, 0, actions, false, nullptr, false, returns, false, nullptr,
                                                  nullptr, best_index, best_return, obs_end || diag_end || status_out);
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_cycle_lookahead: " + bad);
    const int64_t nb = e->n * (int64_t)fanout;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused<C::SCH>(e, nb, stream, [](auto w) { return k_cycle_lookahead<A, C::SCH, decltype(w)::value>; }, n_cycles,
                                 (uint32_t)fanout, (uint32_t)nb, (const A*)actions, returns, rewards_out, obs_end, diag_end, status_out);
        });
        launch_branch_best(e, fanout, returns, best_index, best_return, stream);
    });
}

}  // extern "C"
