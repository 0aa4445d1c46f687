// sbr_sampled.hip - the lookahead over tapes SAMPLED on the device, the MPPI update of the nominal tape, and their entry points.
//   k_lookahead_sampled, k_lookahead_sampled_end   the fan-out over tapes each branch samples around a nominal tape in its own
//              lane; _end also reports where each branch ended (sbr_lookahead_sampled, _end)
//   k_mppi_update    the softmax-weighted update of that tape with the candidates drawn again: no candidate tensor anywhere
#include "sbr_host.h"

// k_lookahead_tape over SAMPLED tapes (sbr_lookahead_sampled): branch j = env * fanout + k plays candidate k of its env, drawn in
// the lane that integrates it (sbr_tape_sample) around the env's row of the nominal tape [rows][N][2] - no candidate tensor is
// read.  The loop body, the (e0, el) addressing of the env's rows and the n_steps = 0 path are k_lookahead_tape's; what differs:
//  * the row a lane loads is its ENV's pair of the nominal tape, addressed like the env's state rows: the workgroup's base
//    (e0, wave-uniform) plus el; the fanout neighbouring lanes of an env share one fetch.  As there, the fetch of the next row is
//    issued before the current call is integrated (tape_load);
//  * the perturbation is drawn when a row comes into force - at the top of the row's first call, from the pair that was loaded
//    under the call before; one Philox block and one Box-Muller per branch and row, not per call, and one place in the code;
//  * actions_out [rows][B][2]: the candidate as it is integrated, stored where it is drawn.  A done branch draws and stores its
//    rows too: the sample depends on nothing of the state, and sbr_mppi_update averages every row of every candidate.
// Fed actions_out, k_lookahead_tape runs the same arithmetic on the same values: same bits in returns and rewards_out.
template <typename ActT, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_lookahead_sampled(SbrPar p, SbrBuf b, int32_t n_steps, int32_t hold, uint32_t fanout,
                                                                uint32_t n_branch, const ActT* __restrict__ nominal, sbr_sampler sm,
                                                                double* __restrict__ returns, double* __restrict__ rewards_out,
                                                                ActT* __restrict__ actions_out) {
    const uint32_t l = threadIdx.x;
    const uint32_t j0u = blockIdx.x * (uint32_t)SBR_BLOCK;   // n_branch < 2^31 (checked by the host): 32 bits hold every branch index
    if (j0u + l >= n_branch) return;
    const int64_t j0 = (int64_t)j0u;
    if (n_steps == 0) {               // no call: nothing of the state or the tape is loaded
        if (returns) (returns + j0)[l] = 0.0;
        return;
    }
    const uint32_t e0u = j0u / fanout;                       // wave-uniform: one scalar division per launch
    const uint32_t eu = (j0u + l) / fanout;
    const uint32_t el = (eu - e0u) & 511u;                   // see k_lookahead_tape: el <= 256, the mask keeps row offsets in 32 bits
    const uint32_t k = j0u + l - eu * fanout;                // the lane's candidate
    const int64_t e0 = (int64_t)e0u;
    const uint64_t gid = (uint64_t)(b.first_env_id + e0) + el;
    double x[SBR_NX], xa6[SBR_NXD];
    SbrX6Reg x6;                      // x6 and the ten Kla values stay in registers: see k_rollout
    SbrRewardParts rp;
    load_x(b, e0, el, x);
    SbrRecord rec;
    load_record<OCI>(p, b, e0, el, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    bool done = rec.meta.done;
    typedef typename SbrAct2<ActT>::type Act2;
    const ActT* row = nominal + e0 * 2;            // the workgroup's part of the nominal row in force (wave-uniform)
    ActT* out = actions_out ? actions_out + j0 * 2 : nullptr;      // ... and of the row of candidates it is drawn into
    ActT m0, m1, a0 = 0, a1 = 0;
    tape_load(row, el, m0, m1);
    uint32_t r = 0;                                // the launch-relative row that comes into force next
    bool draw = true;                              // this call starts a row (wave-uniform)
    int32_t left = hold;                           // calls the row in force still covers, this one included
    double acc = 0.0;
    for (int32_t s = 0; s < n_steps; ++s) {
        if (draw) {                                // the row comes into force: its candidate, from the pair loaded a call ago
            sbr_tape_sample<ActT>(sm, gid, k, r, m0, m1, a0, a1);
            if (out) { Act2 v; v.x = a0; v.y = a1; *reinterpret_cast<Act2*>(out + 2 * l) = v; out += (int64_t)n_branch * 2; }
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
        if (rewards_out) (rewards_out + ((int64_t)s * n_branch + j0))[l] = rw;
    }
    if (returns) (returns + j0)[l] = acc;
}

// k_lookahead_sampled that also reports where each branch ended.  Its body is k_lookahead_sampled's REPEATED, and not one body
// under two kernels like sbr_lookahead_tape: merged that way one of the 24 builds (float32 tape, operating-cost reward, scheme 0)
// spilled four more scalar registers and grew by 24 instructions (profiles/r14_fused_isa.txt).
template <typename ActT, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_lookahead_sampled_end(SbrPar p, SbrBuf b, int32_t n_steps, int32_t hold, uint32_t fanout,
                                                                    uint32_t n_branch, const ActT* __restrict__ nominal, sbr_sampler sm,
                                                                    double* __restrict__ returns, double* __restrict__ rewards_out,
                                                                    ActT* __restrict__ actions_out, float* __restrict__ obs_end,
                                                                    float* __restrict__ state_end, uint8_t* __restrict__ done_end) {
    const uint32_t l = threadIdx.x;
    const uint32_t j0u = blockIdx.x * (uint32_t)SBR_BLOCK;   // n_branch < 2^31 (checked by the host): 32 bits hold every branch index
    if (j0u + l >= n_branch) return;
    const int64_t j0 = (int64_t)j0u;
    const uint32_t e0u = j0u / fanout;                       // the (e0, el) addressing of the env's rows: see k_lookahead_tape
    const uint32_t eu = (j0u + l) / fanout;
    const uint32_t el = (eu - e0u) & 511u;
    const uint32_t k = j0u + l - eu * fanout;                // the lane's candidate
    const int64_t e0 = (int64_t)e0u;
    const uint64_t gid = (uint64_t)(b.first_env_id + e0) + el;
    double x[SBR_NX], xa6[SBR_NXD];
    SbrX6Reg x6;
    SbrRewardParts rp;
    load_x(b, e0, el, x);
    SbrRecord rec;
    load_record<OCI>(p, b, e0, el, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    bool done = rec.meta.done;
    typedef typename SbrAct2<ActT>::type Act2;
    const ActT* row = nominal + e0 * 2;
    ActT* out = actions_out ? actions_out + j0 * 2 : nullptr;
    ActT m0, m1, a0 = 0, a1 = 0;
    tape_load(row, el, m0, m1);
    uint32_t r = 0;                                // the launch-relative row that comes into force next
    bool draw = true;
    int32_t left = hold;
    double acc = 0.0;
    for (int32_t s = 0; s < n_steps; ++s) {
        if (draw) {
            sbr_tape_sample<ActT>(sm, gid, k, r, m0, m1, a0, a1);
            if (out) { Act2 v; v.x = a0; v.y = a1; *reinterpret_cast<Act2*>(out + 2 * l) = v; out += (int64_t)n_branch * 2; }
            ++r;
        }
        draw = --left == 0 && s + 1 < n_steps;
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
        if (rewards_out) (rewards_out + ((int64_t)s * n_branch + j0))[l] = rw;
    }
    if (returns) (returns + j0)[l] = acc;
    sbr_store_branch_end(j0, l, done, c.t, x, x6, obs_end, state_end, done_end);
}

// The MPPI update of the nominal tape (sbr_mppi_update): one wavefront per env, four per workgroup, the shape of k_branch_best.
// Lanes stride over the candidates; the maximum and the sums are closed by a 64-lane xor butterfly.  A lane adds its candidates
// in ascending k and the butterfly adds pairs (commutative, so every lane ends with the same bits): the order of every sum is
// fixed by (k, lane) alone and an env's output by its global id, its returns and the arguments.  The candidates are not read from
// anywhere: sbr_tape_sample draws them again.  Rows are produced in ascending OUTPUT order; output row r needs nominal row
// min(r + shift, rows - 1) >= r, which the wave reads before it writes row r and which no earlier iteration wrote - so
// nominal_out may be nominal itself (the two are deliberately not __restrict__).
SBR_DEV double sbr_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
template <typename ActT>
__global__ __launch_bounds__(SBR_BLOCK) void k_mppi_update(SbrBuf b, int32_t rows, uint32_t fanout, const ActT* nominal, sbr_sampler sm,
                                                          const double* __restrict__ returns, double inv, int32_t shift,
                                                          ActT* nominal_out, double* __restrict__ weights_out) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t i = (int64_t)blockIdx.x * (SBR_BLOCK / 64) + (threadIdx.x >> 6);     // wave-uniform
    if (i >= b.n) return;
    const uint64_t gid = (uint64_t)(b.first_env_id + i);
    const double* mine = returns + i * (int64_t)fanout;
    double m = -INFINITY;
    for (uint32_t k = lane; k < fanout; k += 64u) {
        const double v = mine[k];
        m = fmax(m, v != v ? -INFINITY : v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    const bool weighted = m - m == 0.0;            // m finite; otherwise the tape is passed through and the weights are 0
    double S = 0.0;
    if (weighted) {
        for (uint32_t k = lane; k < fanout; k += 64u) {
            const double v = mine[k];
            S += exp(((v != v ? -INFINITY : v) - m) * inv);
        }
        S = sbr_wave_sum(S);                       // >= 1: the maximum itself has weight exp(0)
    }
    if (weights_out)
        for (uint32_t k = lane; k < fanout; k += 64u) {
            const double v = mine[k];
            (weights_out + i * (int64_t)fanout)[k] = weighted ? exp(((v != v ? -INFINITY : v) - m) * inv) / S : 0.0;
        }
    int32_t have = -1;                             // the nominal row u was formed from
    ActT u0 = 0, u1 = 0;
    for (int32_t r = 0; r < rows; ++r) {
        const int32_t src = (int64_t)r + shift < rows - 1 ? r + shift : rows - 1;
        if (src != have) {
            have = src;
            const ActT* pair = nominal + ((int64_t)src * b.n + i) * 2;
            const ActT m0 = pair[0], m1 = pair[1];
            u0 = m0; u1 = m1;
            if (weighted) {
                double s0 = 0.0, s1 = 0.0;
                for (uint32_t k = lane; k < fanout; k += 64u) {
                    const double v = mine[k];
                    const double w = exp(((v != v ? -INFINITY : v) - m) * inv);
                    ActT a0, a1;
                    sbr_tape_sample<ActT>(sm, gid, k, (uint32_t)src, m0, m1, a0, a1);
                    s0 += w * (double)a0; s1 += w * (double)a1;
                }
                u0 = (ActT)(sbr_wave_sum(s0) / S); u1 = (ActT)(sbr_wave_sum(s1) / S);
            }
        }
        if (lane == 0) {
            ActT* o = nominal_out + ((int64_t)r * b.n + i) * 2;
            o[0] = u0; o[1] = u1;
        }
    }
}

// ------------------------------------------------------------------------------------------- host
// What sbr_lookahead_sampled and sbr_mppi_update have to say about a sampler and a fan-out; empty if they are valid.
static std::string sampler_error(const sbr_env* e, const sbr_sampler* sm, int32_t fanout) {
    std::string bad;
    fanout_error(bad, e, fanout, "candidate");
    if (!sm) return "NULL sampler";
    for (int c = 0; c < 2; ++c) {
        if (!(sm->sigma[c] >= 0) || !std::isfinite(sm->sigma[c])) bad = "sampler.sigma must be >= 0 and finite";
        if (!std::isfinite(sm->lo[c]) || !std::isfinite(sm->hi[c]) || !(sm->lo[c] <= sm->hi[c])) bad = "sampler.lo and hi must be finite with lo <= hi";
    }
    if (sm->reserved_ != 0) bad = "sampler.reserved_ must be 0";
    return bad;
}
// The same for sbr_lookahead_sampled and sbr_lookahead_sampled_end: the LAST failing check is reported.
std::string lookahead_sampled_error(const sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* nominal,
                                    const sbr_sampler* sampler, const double* returns, const int32_t* best_index,
                                    const double* best_return) {
    std::string bad;
    best_error(bad, returns, best_index, best_return);
    if (!nominal && n_steps > 0) bad = "NULL nominal with n_steps > 0";
    const std::string sb = sampler_error(e, sampler, fanout);
    if (!sb.empty()) bad = sb;
    if (hold < 1) bad = "hold must be >= 1";
    if (n_steps < 0) bad = "n_steps must be >= 0";
    if (!e) bad = "NULL env";
    return bad;
}

extern "C" {

int sbr_lookahead_sampled(sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* nominal, const sbr_sampler* sampler,
                          double* returns, double* rewards_out, int32_t* best_index, double* best_return, void* actions_out,
                          void* stream) {
    const std::string bad = lookahead_sampled_error(e, n_steps, hold, fanout, nominal, sampler, returns, best_index, best_return);
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_lookahead_sampled: " + bad);
    const int64_t nb = e->n * (int64_t)fanout;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused<C::SCH>(e, nb, stream, [](auto w) { return k_lookahead_sampled<A, C::OCI, C::SCH, decltype(w)::value>; },
                                 n_steps, hold, (uint32_t)fanout, (uint32_t)nb, (const A*)nominal, *sampler, returns, rewards_out,
                                 (A*)actions_out);
        });
        launch_branch_best(e, fanout, returns, best_index, best_return, stream);
    });
}

int sbr_lookahead_sampled_end(sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* nominal,
                              const sbr_sampler* sampler, double* returns, double* rewards_out, int32_t* best_index,
                              double* best_return, void* actions_out, float* obs_end, float* state_end, uint8_t* done_end,
                              void* stream) {
    std::string bad = end_error(n_steps, obs_end, state_end, done_end);
    const std::string pb = lookahead_sampled_error(e, n_steps, hold, fanout, nominal, sampler, returns, best_index, best_return);
    if (!pb.empty()) bad = pb;
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_lookahead_sampled_end: " + bad);
    const int64_t nb = e->n * (int64_t)fanout;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused<C::SCH>(e, nb, stream, [](auto w) { return k_lookahead_sampled_end<A, C::OCI, C::SCH, decltype(w)::value>; },
                                 n_steps, hold, (uint32_t)fanout, (uint32_t)nb, (const A*)nominal, *sampler, returns, rewards_out,
                                 (A*)actions_out, obs_end, state_end, done_end);
        });
        launch_branch_best(e, fanout, returns, best_index, best_return, stream);
    });
}

int sbr_mppi_update(sbr_env* e, int32_t rows, int32_t fanout, const void* nominal, const sbr_sampler* sampler, const double* returns,
                    double temperature, int32_t shift, void* nominal_out, double* weights_out, void* stream) {
    std::string bad;
    if (shift < 0) bad = "shift must be >= 0";
    const double inv = 1.0 / temperature;          // formed once, here: the kernel multiplies by it
    if (!(temperature > 0) || !std::isfinite(temperature) || !std::isfinite(inv)) bad = "temperature must be > 0, finite, with a finite 1/temperature";
    if (!nominal || !returns || !nominal_out) bad = "NULL nominal, returns or nominal_out";
    const std::string sb = sampler_error(e, sampler, fanout);
    if (!sb.empty()) bad = sb;
    if (rows < 1) bad = "rows must be >= 1";
    if (!e) bad = "NULL env";
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_mppi_update: " + bad);
    return launched(e, [&] {
        either(e->cfg.act_f64, [&](auto a64) {
            using A = std::conditional_t<decltype(a64)::value, double, float>;
            hipLaunchKernelGGL(k_mppi_update<A>, dim3((unsigned)((e->n + SBR_BLOCK / 64 - 1) / (SBR_BLOCK / 64))), dim3(SBR_BLOCK), 0,
                               (hipStream_t)stream, e->buf, rows, (uint32_t)fanout, (const A*)nominal, *sampler, returns, inv, shift,
                               (A*)nominal_out, weights_out);
        });
    });
}

}  // extern "C"
