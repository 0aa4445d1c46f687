// sbr_tape.hip - the fused kernels under the CALLER's action tape, and their entry points.
//   k_rollout_tape   k_rollout under the caller's actions: a tape [rows][N][2], each row held for `hold` calls (sbr_rollout_actions)
//   k_lookahead_tape, k_lookahead_tape_end   the tape kernel as a read-only fan-out: K tapes per env from its current state,
//              nothing of the handle written; _end also reports where each branch ended (sbr_lookahead_actions, _end)
//   k_branch_best    the per-env winner of the K returns, one wavefront per env (sbr_branch_best; the sampled and the policy
//              lookaheads launch it through launch_branch_best)
#include "sbr_host.h"

// k_rollout under the CALLER's actions (sbr_rollout_actions): the same calls in the same order - sbr_run_intervals,
// sbr_finish_step with the register history, sbr_terminal once after the loop - so an env fed the actions k_rollout sampled ends
// with the same bits.  Only the action source differs: row r of the tape [rows][N][2] is in force for calls r*hold .. r*hold +
// hold - 1 of THIS launch.  A lane reads its pair of a row with one 8- or 16-byte load (the wave's 64 pairs are contiguous), and
// the row of call s + 1 is fetched BEFORE call s is integrated: the load's latency passes under the call's arithmetic and not in
// front of every call.  rewards_out [n_steps][N]: one 512-byte segment per wave and call, 0.0 for a call the env skipped.
// A kernel of its own and not a template parameter of k_rollout: tests/test_isa_cpu.py addresses k_rollout by its mangled name.
template <typename ActT, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_rollout_tape(SbrPar p, SbrBuf b, int32_t n_steps, int32_t hold,
                                                           const ActT* __restrict__ actions, double* __restrict__ returns,
                                                           double* __restrict__ rewards_out) {
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SBR_BLOCK, i = i0 + l;
    if (i >= b.n) return;
    if (n_steps == 0) {               // no call: the handle is left as it is (also its plan row)
        if (returns) returns[i] = 0.0;
        return;
    }
    double x[SBR_NX], xa6[SBR_NXD];
    SbrX6Reg x6;                      // x6 and the ten Kla values stay in registers, the terminal phases run after the loop: see k_rollout
    SbrRewardParts rp;
    load_x(b, i0, l, x);
    SbrRecord rec;
    load_record<OCI>(p, b, i0, l, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    SbrMeta& m = rec.meta;
    const ActT* row = actions + i0 * 2;            // the workgroup's part of the row in force (wave-uniform)
    ActT a0, a1;
    tape_load(row, l, a0, a1);
    int32_t left = hold;                           // calls the row in force still covers, this one included
    double acc = 0.0;
    bool terminal_due = false;
    for (int32_t s = 0; s < n_steps; ++s) {
        ActT n0 = a0, n1 = a1;
        if (--left == 0 && s + 1 < n_steps) {      // the next call starts a row (wave-uniform): issue its load now
            row += b.n * 2; left = hold;
            tape_load(row, l, n0, n1);
        }
        double r = 0.0;
        if (!m.done) {
            double t_obs;
            bool dn;
            sbr_run_intervals<SCH>(p, c, x, (double)a0, (double)a1, x6, SbrNoTrace{});
            x6.get(xa6);
            SbrHistReg hs{rec.hist};
            r = sbr_finish_step<OCI, SCH, SbrHistReg, false>(p, c, hs, x, xa6, t_obs, dn, rec.qw, rec.ksum, rp);
            acc += r; rec.ret += r; m.status |= c.st_new;
            m.steps = SbrMeta::next_steps(m.steps);
            if (dn) { m.done = true; terminal_due = !OCI && p.terminal; }
        }
        if (rewards_out) (rewards_out + ((int64_t)s * b.n + i0))[l] = r;
        a0 = n0; a1 = n1;
    }
    if (terminal_due) {
        SbrHistReg hs{rec.hist};
        rec.qw = sbr_terminal<SCH>(p, c, hs, x);
    }
    m.plan = 0;                       // a rollout reports no plan
    store_x(b, i0, l, x);
    store_record<OCI>(p, b, i0, l, rec);
    if (returns) returns[i] = acc;
}

// k_rollout_tape as a READ-ONLY fan-out (sbr_lookahead_actions, sbr_lookahead_actions_end): `fanout` tapes per env, each played
// from the env's CURRENT plant and controller record, and nothing of the handle written.  One lane per BRANCH j = env * fanout +
// candidate; the loop body is the tape kernel's - sbr_run_intervals, sbr_finish_step with the register history, a done branch
// skips - so branch j returns the bits k_rollout_tape returns for an env holding a copy of that state and fed column j of the
// tape.
// What is NOT here, and why that changes no returned bit:
//  * store_x / store_record: the branch's end state is discarded;
//  * sbr_terminal: settle, draw and idle after the done call move only x and Qw, which nothing reads afterwards (a finished branch
//    skips every later call); the end-of-cycle reward of the OCI builds is formed inside sbr_finish_step and stays;
//  * the return row, the call count, the status bits and the plan: they only feed the record's stores.
// Addressing.  fanout neighbouring lanes read the SAME env, a workgroup spans at most 256 / fanout + 2 envs.  The env of a lane is
// formed once, as (e0, el): e0 = env of the workgroup's first branch (wave-uniform), el = the lane's env minus e0 (< 258, 32
// bits).  load_x / load_record take that pair where the other kernels pass (i0, l): every row stays a scalar base plus one
// 32-bit lane offset, and lanes of one env coalesce into one fetch of its 8 bytes.  The tape and the outputs
// are B = N * fanout wide and addressed by (j0, l) like the tape kernel's.
// END: the build that also reports where each branch ended (sbr_store_branch_end), k_lookahead_tape_end.  It has no n_steps = 0
// path: the host refuses that (the handle already holds the state).  Two kernels over the one body and not a run-time test: the
// tests address each by its mangled name and pin its registers and its store count, and a caller that wants no end state pays
// nothing for one.  p and b by value: through references every build came out 80 - 190 instructions longer.
template <bool END, typename ActT, bool OCI, int SCH>
SBR_DEV void sbr_lookahead_tape(SbrPar p, SbrBuf b, int32_t n_steps, int32_t hold, uint32_t fanout, uint32_t n_branch,
                                const ActT* __restrict__ actions, double* __restrict__ returns, double* __restrict__ rewards_out,
                                float* __restrict__ obs_end, float* __restrict__ state_end, uint8_t* __restrict__ done_end) {
    const uint32_t l = threadIdx.x;
    const uint32_t j0u = blockIdx.x * (uint32_t)SBR_BLOCK;   // n_branch < 2^31 (checked by the host): 32 bits hold every branch index
    if (j0u + l >= n_branch) return;
    const int64_t j0 = (int64_t)j0u;
    if constexpr (!END) {
        if (n_steps == 0) {           // no call: nothing of the state is loaded
            if (returns) (returns + j0)[l] = 0.0;
            return;
        }
    }
    const uint32_t e0u = j0u / fanout;                       // wave-uniform: one scalar division per launch
    // el <= l / fanout + 1 <= 256.  The mask changes no value; it tells the backend that el * 8 fits 32 bits, which is what lets
    // a row access be `global_load v, v_off, s[base]` - without it every row's address was formed per lane in 64 bits
    const uint32_t el = ((j0u + l) / fanout - e0u) & 511u;
    const int64_t e0 = (int64_t)e0u;
    double x[SBR_NX], xa6[SBR_NXD];
    SbrX6Reg x6;                      // x6 and the ten Kla values stay in registers: see k_rollout
    SbrRewardParts rp;
    load_x(b, e0, el, x);
    SbrRecord rec;
    load_record<OCI>(p, b, e0, el, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    bool done = rec.meta.done;
    const ActT* row = actions + j0 * 2;            // the workgroup's part of the row in force (wave-uniform)
    ActT a0, a1;
    tape_load(row, l, a0, a1);
    int32_t left = hold;                           // calls the row in force still covers, this one included
    double acc = 0.0;
    for (int32_t s = 0; s < n_steps; ++s) {
        ActT n0 = a0, n1 = a1;
        if (--left == 0 && s + 1 < n_steps) {      // the next call starts a row (wave-uniform): issue its load now
            row += (int64_t)n_branch * 2; left = hold;
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
        if (rewards_out) (rewards_out + ((int64_t)s * n_branch + j0))[l] = r;
        a0 = n0; a1 = n1;
    }
    if (returns) (returns + j0)[l] = acc;
    if constexpr (END) sbr_store_branch_end(j0, l, done, c.t, x, x6, obs_end, state_end, done_end);
}
template <typename ActT, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_lookahead_tape(SbrPar p, SbrBuf b, int32_t n_steps, int32_t hold, uint32_t fanout,
                                                             uint32_t n_branch, const ActT* __restrict__ actions,
                                                             double* __restrict__ returns, double* __restrict__ rewards_out) {
    sbr_lookahead_tape<false, ActT, OCI, SCH>(p, b, n_steps, hold, fanout, n_branch, actions, returns, rewards_out, nullptr, nullptr, nullptr);
}
template <typename ActT, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_lookahead_tape_end(SbrPar p, SbrBuf b, int32_t n_steps, int32_t hold, uint32_t fanout,
                                                                 uint32_t n_branch, const ActT* __restrict__ actions,
                                                                 double* __restrict__ returns, double* __restrict__ rewards_out,
                                                                 float* __restrict__ obs_end, float* __restrict__ state_end,
                                                                 uint8_t* __restrict__ done_end) {
    sbr_lookahead_tape<true, ActT, OCI, SCH>(p, b, n_steps, hold, fanout, n_branch, actions, returns, rewards_out, obs_end, state_end, done_end);
}

// The winner of each env's `fanout` branch returns (sbr_lookahead_actions, launched behind k_lookahead_tape on the same stream):
// one wavefront per env.  Rule (include/sbr_amd.h): the largest return wins, a NaN return compares as -inf, ties go to the lowest
// candidate; best_return is the winner's return as it stands in `returns` (NaN only if all are NaN or -inf ties with one at a
// lower index).  Lanes stride over the candidates, then a 64-lane xor butterfly under the same rule, then lane 0 stores: one path
// for every fanout.
struct SbrBest {
    double key, val;      // key: the return with NaN replaced by -inf; val: the return itself
    uint32_t k;
    SBR_DEV void take(double key2, double val2, uint32_t k2) {
        if (key2 > key || (key2 == key && k2 < k)) { key = key2; val = val2; k = k2; }
    }
};
__global__ __launch_bounds__(SBR_BLOCK) void k_branch_best(const double* __restrict__ returns, int64_t n, uint32_t fanout,
                                                          int32_t* __restrict__ best_index, double* __restrict__ best_return) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t i = (int64_t)blockIdx.x * (SBR_BLOCK / 64) + (threadIdx.x >> 6);     // wave-uniform
    if (i >= n) return;
    const double* mine = returns + i * (int64_t)fanout;
    SbrBest bst{-INFINITY, NAN, 0xffffffffu};      // a lane without a candidate loses every comparison (lane 0 always has k = 0)
    for (uint32_t k = lane; k < fanout; k += 64u) {
        const double v = mine[k];
        bst.take(v != v ? -INFINITY : v, v, k);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        bst.take(__shfl_xor(bst.key, off, 64), __shfl_xor(bst.val, off, 64), (uint32_t)__shfl_xor((int)bst.k, off, 64));
    if (lane == 0) {
        if (best_index) best_index[i] = (int32_t)bst.k;
        if (best_return) best_return[i] = bst.val;
    }
}

// ------------------------------------------------------------------------------------------- host
// The refusals every entry point with a fan-out shares.  Like the checks around them they overwrite `bad` where they fail: of all
// the checks of an entry point the LAST failing one is reported.  word: what the upper 24 bits of the Philox stream word carry
// where something is drawn per branch ("candidate", "branch"); NULL where nothing is, and the fan-out has no such limit.
void fanout_error(std::string& bad, const sbr_env* e, int32_t fanout, const char* word) {
    if (fanout < 1) bad = "fanout must be >= 1";
    else if (word && fanout > (1 << 24)) bad = std::string("fanout must be <= 2^24 (the ") + word + " is 24 bits of the Philox stream word)";
    else if (e && e->n * (int64_t)fanout >= (int64_t)1 << 31) bad = "num_envs * fanout must stay below 2^31 branches";
}
void best_error(std::string& bad, const double* returns, const int32_t* best_index, const double* best_return) {
    if ((best_index || best_return) && !returns) bad = "best_index / best_return are reduced from returns: give returns with them";
}
// What sbr_lookahead_actions and sbr_lookahead_actions_end have to say about the arguments they share; empty if they are valid.
// Every check is evaluated, the LAST failing one is reported - all of them before anything is touched.
std::string lookahead_error(const sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* actions, const double* returns,
                            const int32_t* best_index, const double* best_return) {
    std::string bad;
    best_error(bad, returns, best_index, best_return);
    if (!actions && n_steps > 0) bad = "NULL actions with n_steps > 0";
    fanout_error(bad, e, fanout, nullptr);
    if (hold < 1) bad = "hold must be >= 1";
    if (n_steps < 0) bad = "n_steps must be >= 0";
    if (!e) bad = "NULL env";
    return bad;
}
// What the two _end entry points add to their parents' refusals; empty if the arguments are valid.
std::string end_error(int32_t n_steps, const void* obs_end, const void* state_end, const void* done_end) {
    if (n_steps == 0) return "n_steps = 0 has no end state to report that the handle does not already hold";
    if (!obs_end && !state_end && !done_end) return "obs_end, state_end and done_end are all NULL: call the entry point without _end";
    return "";
}
// k_branch_best behind a lookahead kernel on the same stream, where the caller wants a winner, or on its own (sbr_branch_best):
// one wavefront per env
void launch_branch_best(const sbr_env* e, int32_t fanout, const double* values, int32_t* best_index, double* best_value,
                               void* stream) {
    if (!best_index && !best_value) return;
    hipLaunchKernelGGL(k_branch_best, dim3((unsigned)((e->n + SBR_BLOCK / 64 - 1) / (SBR_BLOCK / 64))), dim3(SBR_BLOCK), 0,
                       (hipStream_t)stream, values, e->n, (uint32_t)fanout, best_index, best_value);
}

extern "C" {

int sbr_rollout_actions(sbr_env* e, int32_t n_steps, int32_t hold, const void* actions, double* returns, double* rewards_out,
                        void* stream) {
    if (!e || n_steps < 0 || hold < 1 || (!actions && n_steps > 0))
        return fail(e, SBR_ERR_INVALID, "sbr_rollout_actions: need n_steps >= 0, hold >= 1 and an action tape");
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused<C::SCH>(e, e->n, stream, [](auto w) { return k_rollout_tape<A, C::OCI, C::SCH, decltype(w)::value>; }, n_steps,
                                 hold, (const A*)actions, returns, rewards_out);
        });
    });
}

int sbr_lookahead_actions(sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* actions, double* returns,
                          double* rewards_out, int32_t* best_index, double* best_return, void* stream) {
    const std::string bad = lookahead_error(e, n_steps, hold, fanout, actions, returns, best_index, best_return);
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_lookahead_actions: " + bad);
    const int64_t nb = e->n * (int64_t)fanout;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused<C::SCH>(e, nb, stream, [](auto w) { return k_lookahead_tape<A, C::OCI, C::SCH, decltype(w)::value>; }, n_steps,
                                 hold, (uint32_t)fanout, (uint32_t)nb, (const A*)actions, returns, rewards_out);
        });
        launch_branch_best(e, fanout, returns, best_index, best_return, stream);
    });
}

int sbr_lookahead_actions_end(sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* actions, double* returns,
                              double* rewards_out, int32_t* best_index, double* best_return, float* obs_end, float* state_end,
                              uint8_t* done_end, void* stream) {
    std::string bad = end_error(n_steps, obs_end, state_end, done_end);
    const std::string pb = lookahead_error(e, n_steps, hold, fanout, actions, returns, best_index, best_return);
    if (!pb.empty()) bad = pb;
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_lookahead_actions_end: " + bad);
    const int64_t nb = e->n * (int64_t)fanout;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using A = typename C::ActT;
            launch_fused<C::SCH>(e, nb, stream, [](auto w) { return k_lookahead_tape_end<A, C::OCI, C::SCH, decltype(w)::value>; },
                                 n_steps, hold, (uint32_t)fanout, (uint32_t)nb, (const A*)actions, returns, rewards_out, obs_end, state_end,
                                 done_end);
        });
        launch_branch_best(e, fanout, returns, best_index, best_return, stream);
    });
}

int sbr_branch_best(sbr_env* e, int32_t fanout, const double* values, int32_t* best_index, double* best_value, void* stream) {
    std::string bad;
    if (!best_index && !best_value) bad = "best_index and best_value are both NULL";
    if (!values) bad = "NULL values";
    fanout_error(bad, e, fanout, nullptr);
    if (!e) bad = "NULL env";
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_branch_best: " + bad);
    return launched(e, [&] { launch_branch_best(e, fanout, values, best_index, best_value, stream); });
}

}  // extern "C"
