// sbr_policy_lookahead.hip - the closed-loop lookahead under the caller's MLP, and its entry point.
//   k_lookahead_policy   the policy kernel as a read-only fan-out: K closed-loop rollouts of the caller's MLP per env, each branch
//              with exploration noise of its own, the handle and the observation untouched (sbr_lookahead_policy)
#include "sbr_policy.h"

// exploration noise of BRANCH k of a closed-loop lookahead (sbr_lookahead_policy): sbr_policy_noise's construction with k in the
// upper 24 bits of the stream word, as sbr_tape_sample carries its candidate in stream 4.  k = 0 is sbr_policy_noise's block: the
// same operations in the same order, so under -ffp-contract=off the same bits.  A function of its own: sbr_policy_noise and the
// kernel that calls it stay as they are.
SBR_DEV void sbr_branch_noise(uint64_t seed, uint64_t env_id, uint32_t k, uint32_t call, double& z0, double& z1) {
    uint32_t c[4] = {call, 3u + 256u * k, (uint32_t)env_id, (uint32_t)(env_id >> 32)};
    sbr_philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u1 = sbr_u53(c[0], c[1]), u2 = sbr_u53(c[2], c[3]);
    const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586476925286766559 * u2;
    double sn, cs;
    sincos(ang, &sn, &cs);
    z0 = rad * cs; z1 = rad * sn;
}
// k_rollout_policy as a READ-ONLY fan-out (sbr_lookahead_policy): `fanout` closed-loop rollouts of the caller's policy per env,
// each from the env's CURRENT plant, controller record and observation row, nothing of the handle and nothing of obs written.
// One lane per BRANCH j = env * fanout + k.  The loop is k_rollout_policy's, REPEATED and not shared (DESIGN.md section 3.6:
// shared through device functions it moved registers, spills or scratch of both kernels' builds, profiles/r14_fused_isa.txt) -
// sbr_write_obs<float> before a decision with s > 0, sbr_mlp<H>,
// sbr_run_intervals, sbr_finish_step with the register history - so without noise every branch returns the bits
// k_rollout_policy returns for an env holding a copy of that state, and fed its own actions_out k_lookahead_tape returns the
// same bits.  What is NOT here, for the reasons given at k_lookahead_tape: store_x / store_record, sbr_terminal, the return row,
// the status bits and the plan.  The call count stays: it is the counter word of the noise.
//  * Addressing: the env's rows - plant, record and the 18 observation values - by (e0, el) as in k_lookahead_tape, the mask on
//    el included; the fanout lanes of an env share one fetch of each value.  The outputs are B wide and addressed by (j0, l).
//  * Noise: sbr_branch_noise, branch k of the env; keep_mean = 1 leaves branch 0 of every env at the policy's mean (the value is
//    not touched, rather than 0 added to it: -0 stays -0).
//  * Population: the policy of a wave is its first lane's (readfirstlane below).
//  * End outputs: sbr_store_branch_end behind the loop, each behind its wave-uniform NULL test.
// n_steps = 0 (the host refuses it together with an end output): zeros in returns, nothing loaded.
template <int H, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_lookahead_policy(SbrPar p, SbrBuf b, int32_t n_steps, int32_t hold, uint32_t fanout,
                                                               uint32_t n_branch, const float* __restrict__ params, SbrPolicyDev pl,
                                                               int32_t keep_mean, const float* __restrict__ obs,
                                                               double* __restrict__ returns, double* __restrict__ rewards_out,
                                                               float* __restrict__ actions_out, float* __restrict__ obs_end,
                                                               float* __restrict__ state_end, uint8_t* __restrict__ done_end) {
    const uint32_t l = threadIdx.x;
    const uint32_t j0u = blockIdx.x * (uint32_t)SBR_BLOCK;   // n_branch < 2^31 (checked by the host): 32 bits hold every branch index
    if (j0u + l >= n_branch) return;
    const int64_t j0 = (int64_t)j0u;
    if (n_steps == 0) {               // no call: nothing of the state, the observation or the net is loaded
        if (returns) (returns + j0)[l] = 0.0;
        return;
    }
    const uint32_t e0u = j0u / fanout;                       // the (e0, el) addressing of the env's rows: see k_lookahead_tape
    const uint32_t eu = (j0u + l) / fanout;
    const uint32_t el = (eu - e0u) & 511u;
    const uint32_t k = j0u + l - eu * fanout;                // the lane's branch of its env
    const int64_t e0 = (int64_t)e0u;
    const uint64_t gid = (uint64_t)(b.first_env_id + e0) + el;
    // the wave's policy block.  A population is cut at global ids that are multiples of 256 and the handle's first id is one
    // (checked by the host), so a policy boundary falls at a local env index that is a multiple of 256, i.e. at branch index
    // (multiple of 256) * fanout - a multiple of the workgroup size.  No workgroup of 256 branches, and so no wave, straddles
    // two policies: the policy of the wave's first lane is the policy of all of them, whatever the fanout
    const float* __restrict__ w = params;
    if (pl.n_policies > 1) {
        const uint32_t pol = __builtin_amdgcn_readfirstlane((uint32_t)(gid / (uint64_t)pl.envs_per_policy));
        w = params + (int64_t)pol * pl.stride;
    }
    const bool noisy = pl.noise != 0 && !(keep_mean != 0 && k == 0);
    double x[SBR_NX], xa6[SBR_NXD];
    SbrX6Reg x6;                      // x6 and the ten Kla values stay in registers: see k_rollout
    SbrRewardParts rp;
    load_x(b, e0, el, x);
    SbrRecord rec;
    load_record<OCI>(p, b, e0, el, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    bool done = rec.meta.done;
    int32_t steps = rec.meta.steps;                // the branch's calls since reset: the counter word of its noise
    float o[SBR_NOBS];
    const float* __restrict__ env_obs = obs + e0 * SBR_NOBS + el * (uint32_t)SBR_NOBS;
#pragma unroll
    for (int q = 0; q < SBR_NOBS; ++q) o[q] = env_obs[q];
    float a0 = 0.0f, a1 = 0.0f;
    int32_t left = 1;                              // calls until the next decision, this one included
    double acc = 0.0;
    for (int32_t s = 0; s < n_steps; ++s) {
        if (--left == 0) {                         // a decision call (wave-uniform): s % hold == 0
            left = hold;
            if (__builtin_amdgcn_ballot_w64(!done) != 0ull) {
                if (s > 0) {
                    x6.get(xa6);
                    sbr_write_obs<float>(o, 1, c.t, x, xa6, x);
                }
                float y[2];
                sbr_mlp<H>(pl, w, o, y);
                if (pl.squash != 0) { y[0] = tanhf(y[0]); y[1] = tanhf(y[1]); }
                a0 = __builtin_fmaf(pl.scale[0], y[0], pl.bias[0]);
                a1 = __builtin_fmaf(pl.scale[1], y[1], pl.bias[1]);
                if (pl.noise != 0) {
                    double z0, z1;
                    sbr_branch_noise(pl.seed, gid, k, (uint32_t)steps, z0, z1);
                    if (noisy) {
                        a0 = (float)((double)a0 + (double)pl.std[0] * z0);
                        a1 = (float)((double)a1 + (double)pl.std[1] * z1);
                    }
                }
            }
            if (done) { a0 = 0.0f; a1 = 0.0f; }
            if (actions_out) {
                const int64_t row = (int64_t)(s / hold);
                sbr_act2_f32 v; v.x = a0; v.y = a1;
                *reinterpret_cast<sbr_act2_f32*>(actions_out + (row * n_branch + j0) * 2 + 2 * l) = v;
            }
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
            steps = SbrMeta::next_steps(steps);
            if (dn) done = true;
        }
        if (rewards_out) (rewards_out + ((int64_t)s * n_branch + j0))[l] = r;
    }
    if (returns) (returns + j0)[l] = acc;
    sbr_store_branch_end(j0, l, done, c.t, x, x6, obs_end, state_end, done_end);
}

extern "C" {

int sbr_lookahead_policy(sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const sbr_policy* policy, int32_t keep_mean,
                         const float* obs, double* returns, double* rewards_out, int32_t* best_index, double* best_return,
                         float* actions_out, float* obs_end, float* state_end, uint8_t* done_end, void* stream) {
    // Every check is evaluated, the LAST failing one is reported - all of them before anything is touched.
    std::string bad;
    if (!e) bad = "NULL env";
    if (n_steps < 0) bad = "n_steps must be >= 0";
    else if (n_steps == 0 && (obs_end || state_end || done_end))
        bad = "n_steps = 0 has no end state to report that the handle does not already hold";
    if (hold < 1) bad = "hold must be >= 1";
    fanout_error(bad, e, fanout, "branch");
    if (keep_mean != 0 && keep_mean != 1) bad = "keep_mean must be 0 or 1";
    best_error(bad, returns, best_index, best_return);
    if (!obs) bad = "NULL obs";
    const std::string pb = policy_error(e, policy);
    if (!pb.empty()) bad = pb;
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_lookahead_policy: " + bad);
    const SbrPolicyDev pl = policy_dev(policy);
    const bool wide = policy->n_hidden > 0 && policy->width == 64;     // without a hidden layer the width does not matter
    const int64_t nb = e->n * (int64_t)fanout;
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            either(wide, [&](auto w64) {
                constexpr int H = decltype(w64)::value ? 64 : 32;
                launch_fused<C::SCH>(e, nb, stream, [](auto w) { return k_lookahead_policy<H, C::OCI, C::SCH, decltype(w)::value>; },
                                     n_steps, hold, (uint32_t)fanout, (uint32_t)nb, policy->params, pl, keep_mean, obs, returns, rewards_out,
                                     actions_out, obs_end, state_end, done_end);
            });
        });
        launch_branch_best(e, fanout, returns, best_index, best_return, stream);
    });
}

}  // extern "C"
