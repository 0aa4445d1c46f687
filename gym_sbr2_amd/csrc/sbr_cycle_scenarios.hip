// sbr_cycle_scenarios.hip - the per-cycle lookahead under UNCERTAIN influent, and its entry point.
//   k_cycle_lookahead_scenarios   k_cycle_lookahead over `fanout` candidate tapes x `n_scen` influent futures per env: every
//              candidate of an env is played against the SAME n_scen futures (common random numbers), the futures come from the
//              caller (sbr_draw_influent draws them), nothing of the handle written (sbr_cycle_lookahead_scenarios; the winners
//              come from k_branch_best of sbr_tape.hip through launch_branch_best)
//   k_scenario_stats              mean and worst case of each candidate's n_scen returns
#include "sbr_host.h"

// k_cycle_lookahead (sbr_cycle_lookahead.hip) with the influent of every cycle taken from the caller's futures and not from
// the handle.  One lane per BRANCH j = (env * fanout + candidate) * n_scen + future.  A cycle is k_cycle's body word for word,
// with ld[1..13] = entries 1..13 of influent[c][env * n_scen + future]: the bits of sbr_cycle_reset(carry_over = 1, influent =
// that row) followed by sbr_cycle_step on an env holding the branch's state.  The env's STORED influent is never read.
// ADDRESSING.  Three rows per lane, each a wave-uniform base plus a lane offset:
//  * the plant: (e0, el) as in k_cycle_lookahead, an env now holding fanout * n_scen consecutive branches (el <= 255);
//  * the action row (j0 + l) / n_scen, the tape not being expanded over the futures: base a0 = j0 / n_scen, offset <= 255;
//  * the influent row env * n_scen + future.  It is NOT monotone in l - the next candidate of an env starts again at future 0 -
//    so the base is the row of the workgroup's first ENV, e0 * n_scen, and the offset (env - e0) * n_scen + future.  With
//    n_scen > 256 that offset exceeds what a workgroup has lanes (up to 254 + 2 n_scen), so it takes no mask and is widened to 64
//    bits before it is scaled: a row is fourteen adjacent doubles, so the thirteen loads share ONE lane address, formed at the
//    top of the cycle and dead behind the loads.
// Every output is B wide and addressed by (j0, l).
// REGISTERS: every measure of k_cycle_lookahead (the comment there) - the lane index through an empty asm
// per cycle, the constants through the kernel-argument segment, the sum and the status bits parked in LDS, no fetch ahead, the
// end rows stored inside the last cycle.  The body is written out again and not shared with k_cycle_lookahead's: that kernel's
// instruction text is pinned, and its three rows are one.
template <typename ActT, int SCH>
SBR_DEV void sbr_cycle_scenarios_branch(SbrPar p, SbrBuf b, int32_t n_cycles, uint32_t fanout, uint32_t n_scen, uint32_t n_branch,
                                        const ActT* __restrict__ actions, const double* __restrict__ influent,
                                        double* __restrict__ returns, double* __restrict__ rewards_out, double* __restrict__ obs_end,
                                        double* __restrict__ diag_end, uint8_t* __restrict__ status_out) {
    __shared__ double park_acc[SBR_BLOCK];                   // each lane its own slot: no barrier anywhere
    __shared__ int park_st[SBR_BLOCK];
    const uint32_t l = threadIdx.x;
    const uint32_t j0u = blockIdx.x * (uint32_t)SBR_BLOCK;   // n_branch < 2^31 (checked by the host): 32 bits hold every branch index
    if (j0u + l >= n_branch) return;
    const int64_t j0 = (int64_t)j0u;
    double acc = 0.0;
    if (n_cycles > 0) {               // no cycle: nothing of the state, the tape or the futures is loaded
        const uint32_t per_env = fanout * n_scen;                // < 2^31 with n_branch
        const uint32_t e0u = j0u / per_env, a0u = j0u / n_scen;  // wave-uniform: two scalar divisions per launch
        const int64_t e0 = (int64_t)e0u;
        const int64_t act_stride = (int64_t)(n_branch / n_scen) * 3, infl_stride = (int64_t)(n_branch / fanout) * SBR_NX;
        double x[SBR_NX];
        load_x(b, e0, cycle_env_of(j0u + l, per_env, e0u), x);
        park_acc[l] = 0.0;
        park_st[l] = sbr_status_bits(p, x);                      // a later cycle starts where the one before it ended
        const ActT* row = actions + (int64_t)a0u * 3;            // the workgroup's part of the rows in force (wave-uniform)
        const double* fut = influent + e0 * (int64_t)n_scen * SBR_NX;
        for (int32_t c = 0; c < n_cycles; ++c) {
            const bool last = c + 1 == n_cycles;                 // wave-uniform
            uint32_t lc = l, z = 0;
            asm volatile("" : "+v"(lc), "+s"(z) : : "memory");
            lc &= SBR_BLOCK - 1u;
            const SbrPar& pc = *(const SbrPar*)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + z);
            const uint32_t j = j0u + lc, a = j / n_scen;         // a: the branch's (env, candidate) pair, the row of its tape
            ActT a0, a1, a2;
            cycle_row_load(row, a - a0u, a0, a1, a2);
            row += act_stride;
            double ld[SBR_NX], o3[3];
            {   // the future: row (env - e0) * n_scen + (j - a * n_scen) behind the workgroup's base, loaded where it is used
                const double* mine = fut + (uint64_t)((j / per_env - e0u) * n_scen + (j - a * n_scen)) * SBR_NX;
#pragma unroll
                for (int q = 1; q < SBR_NX; ++q) ld[q] = mine[q];
            }
            fut += infl_stride;
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
#define SBR_CYCLE_SCENARIOS_PARAMS(ActT)                                                                                          \
    SbrPar p, SbrBuf b, int32_t n_cycles, uint32_t fanout, uint32_t n_scen, uint32_t n_branch, const ActT* __restrict__ actions, \
        const double* __restrict__ influent, double* __restrict__ returns, double* __restrict__ rewards_out,                     \
        double* __restrict__ obs_end, double* __restrict__ diag_end, uint8_t* __restrict__ status_out
// the kernel, its two-waves specialisations and the assert on its first parameter: SBR_CYCLE_KERNEL_PAR_FIRST (sbr_host.h)
SBR_CYCLE_KERNEL_PAR_FIRST(k_cycle_lookahead_scenarios, sbr_cycle_scenarios_branch, SBR_CYCLE_SCENARIOS_PARAMS, p, b, n_cycles, fanout,
                           n_scen, n_branch, actions, influent, returns, rewards_out, obs_end, diag_end, status_out)

// Mean and worst case of each (env, candidate) pair's n_scen returns, behind the lookahead on the same stream: one lane per pair,
// the futures walked in order.  mean = ((..(0.0 + r_0) + r_1 ..) + r_{S-1}) / S, one IEEE division, a NaN propagating through the
// sum; worst = the smallest return, NaN as soon as one of them is.
__global__ __launch_bounds__(SBR_BLOCK) void k_scenario_stats(const double* __restrict__ returns, int64_t n_pairs, uint32_t n_scen,
                                                             double* __restrict__ mean_out, double* __restrict__ worst_out) {
    const int64_t m = (int64_t)blockIdx.x * SBR_BLOCK + threadIdx.x;
    if (m >= n_pairs) return;
    const double* mine = returns + m * (int64_t)n_scen;
    double sum = 0.0, worst = mine[0];
    for (uint32_t s = 0; s < n_scen; ++s) {
        const double r = mine[s];
        sum = sum + r;
        if (worst == worst && !(r >= worst)) worst = r;      // a smaller return, or the first NaN - which then stays
    }
    if (mean_out) mean_out[m] = sum / (double)n_scen;
    if (worst_out) worst_out[m] = worst;
}

// k_scenario_stats for every caller, this unit's entry point and the other units' alike (launch_stats_and_best, sbr_host.h): a
// kernel is named in one unit only.  Nothing is launched when neither output was asked for.
void launch_scenario_stats(const double* returns, int64_t n_pairs, int32_t n_scen, double* mean_out, double* worst_out, void* stream) {
    if (mean_out || worst_out)
        hipLaunchKernelGGL(k_scenario_stats, grid_for(n_pairs), dim3(SBR_BLOCK), 0, (hipStream_t)stream, returns, n_pairs,
                           (uint32_t)n_scen, mean_out, worst_out);
}

extern "C" {

int sbr_cycle_lookahead_scenarios(sbr_env* e, int32_t n_cycles, int32_t fanout, int32_t n_scen, const void* actions,
                                  const double* influent, double* returns, double* rewards_out, double* mean_out, double* worst_out,
                                  int32_t* best_index, double* best_value, double* obs_end, double* diag_end, uint8_t* status_out,
                                  void* stream) {
    const std::string bad = cycle_lookahead_error(e, n_cycles, fanout, &n_scen, 0, actions, true, influent, false, returns, true, mean_out,
                                                  worst_out, best_index, best_value, obs_end || diag_end || status_out);
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_cycle_lookahead_scenarios: " + bad);
    const int64_t nb = e->n * (int64_t)fanout * n_scen;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused<C::SCH>(e, nb, stream, [](auto w) { return k_cycle_lookahead_scenarios<A, C::SCH, decltype(w)::value>; },
                                 n_cycles, (uint32_t)fanout, (uint32_t)n_scen, (uint32_t)nb, (const A*)actions, influent, returns,
                                 rewards_out, obs_end, diag_end, status_out);
        });
        launch_stats_and_best(e, fanout, n_scen, returns, mean_out, worst_out, best_index, best_value, stream);
    });
}

}  // extern "C"
