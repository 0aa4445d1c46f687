// sbr_policy.hip - the fused rollout in CLOSED loop under the caller's MLP, and its entry point.
//   k_rollout_policy     the tape kernel in closed loop: the caller's MLP maps the env's observation to the action, in the lane of
//              the plant (sbr_rollout_policy)
// The read-only fan-out of this kernel, k_lookahead_policy, is a unit of its own (sbr_policy_lookahead.hip): the two kernels'
// 24 builds are most of the library's compile time, and apart they compile side by side.
#include "sbr_policy.h"

// k_rollout_tape in CLOSED loop (sbr_rollout_policy): the action of a decision call is the caller's MLP applied to the env's
// observation, evaluated in the lane that holds the plant.  The loop body is the tape kernel's - sbr_run_intervals,
// sbr_finish_step with the register history, sbr_terminal once after the loop - so an env fed this kernel's own actions_out as a
// tape ends with the same bits.
// The net and the exploration noise of a decision (sbr_policy_noise): sbr_policy.h.
// obs [N][18] float32, in and out: on entry the observation in force, on exit the current one of every env that is not done
// (a done env's row is left alone).  In between the observation is never stored: before a decision it is formed in registers
// from the plant, the interval's start values (x6) and the running time, exactly as k_step forms the row it returns.
// actions_out [ceil(n_steps/hold)][N][2]: the decisions as float32 - the values that are cast to double and integrated -
// 0 for a decision an env skipped because its episode had ended.
template <int H, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_rollout_policy(SbrPar p, SbrBuf b, int32_t n_steps, int32_t hold,
                                                             const float* __restrict__ params, SbrPolicyDev pl,
                                                             float* __restrict__ obs, double* __restrict__ returns,
                                                             float* __restrict__ actions_out, double* __restrict__ rewards_out) {
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SBR_BLOCK, i = i0 + l;
    if (i >= b.n) return;
    if (n_steps == 0) {               // no call: the handle and obs are left as they are
        if (returns) returns[i] = 0.0;
        return;
    }
    const uint64_t gid = (uint64_t)(b.first_env_id + i);
    // the wave's policy block: a population is cut at multiples of the workgroup size (checked by the host), so the policy of
    // the wave's first lane is the policy of all of them
    const float* __restrict__ w = params;
    if (pl.n_policies > 1) {
        const uint32_t pol = __builtin_amdgcn_readfirstlane((uint32_t)(gid / (uint64_t)pl.envs_per_policy));
        w = params + (int64_t)pol * pl.stride;
    }
    double x[SBR_NX], xa6[SBR_NXD];
    SbrX6Reg x6;                      // x6 and the ten Kla values stay in registers, the terminal phases run after the loop: see k_rollout
    SbrRewardParts rp;
    load_x(b, i0, l, x);
    SbrRecord rec;
    load_record<OCI>(p, b, i0, l, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    SbrMeta& m = rec.meta;
    float o[SBR_NOBS];
    float* __restrict__ my_obs = obs + i * SBR_NOBS;
#pragma unroll
    for (int k = 0; k < SBR_NOBS; ++k) o[k] = my_obs[k];
    float a0 = 0.0f, a1 = 0.0f;
    int32_t left = 1;                              // calls until the next decision, this one included
    double acc = 0.0;
    bool terminal_due = false;
    for (int32_t s = 0; s < n_steps; ++s) {
        if (--left == 0) {                         // a decision call (wave-uniform): s % hold == 0
            left = hold;
            if (__builtin_amdgcn_ballot_w64(!m.done) != 0ull) {
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
                    sbr_policy_noise(pl.seed, gid, (uint32_t)m.steps, z0, z1);
                    a0 = (float)((double)a0 + (double)pl.std[0] * z0);
                    a1 = (float)((double)a1 + (double)pl.std[1] * z1);
                }
            }
            if (m.done) { a0 = 0.0f; a1 = 0.0f; }
            if (actions_out) {
                const int64_t row = (int64_t)(s / hold);
                sbr_act2_f32 v; v.x = a0; v.y = a1;
                *reinterpret_cast<sbr_act2_f32*>(actions_out + (row * b.n + i0) * 2 + 2 * l) = v;
            }
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
    }
    if (!m.done) {                    // ran every call of the launch: its observation for the next one
        x6.get(xa6);
        sbr_write_obs<float>(o, 1, c.t, x, xa6, x);
#pragma unroll
        for (int k = 0; k < SBR_NOBS; ++k) my_obs[k] = o[k];
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

// ------------------------------------------------------------------------------------------- host
extern "C" {

int64_t sbr_policy_param_count(int32_t n_hidden, int32_t width) {
    const int64_t h = width;
    if (n_hidden == 0) return SBR_NOBS * 2 + 2;
    if (n_hidden < 0 || n_hidden > 2 || (width != 32 && width != 64)) return -1;
    return (SBR_NOBS * h + h) + (n_hidden == 2 ? h * h + h : 0) + (h * 2 + 2);
}

}  // extern "C"

// What sbr_rollout_policy and sbr_lookahead_policy have to say about a policy; empty if it is valid.  Every check is evaluated,
// the LAST failing one is reported.
std::string policy_error(const sbr_env* e, const sbr_policy* policy) {
    if (!policy) return "NULL policy";
    std::string bad;
    const sbr_policy& q = *policy;
    if (!q.params) bad = "NULL params";
    if (q.n_hidden < 0 || q.n_hidden > 2) bad = "n_hidden must be 0, 1 or 2";
    else if (q.n_hidden > 0 && q.width != 32 && q.width != 64) bad = "width must be 32 or 64";
    if (q.activation != 0 && q.activation != 1) bad = "activation must be 0 (tanh) or 1 (relu)";
    if (q.squash != 0 && q.squash != 1) bad = "squash must be 0 (none) or 1 (tanh)";
    for (int k = 0; k < 2; ++k)
        if (!(q.noise_std[k] >= 0.0f) || !std::isfinite(q.noise_std[k])) bad = "noise_std must be finite and >= 0";
    if (q.n_policies < 1) bad = "n_policies must be >= 1";
    else if (q.n_policies > 1) {
        // a wave reads ONE policy block through the scalar data path: the population is cut at workgroup boundaries
        if (q.envs_per_policy < SBR_BLOCK || q.envs_per_policy % SBR_BLOCK != 0)
            bad = "with n_policies > 1 envs_per_policy must be a positive multiple of 256";
        else if (e && e->buf.first_env_id % SBR_BLOCK != 0)
            bad = "with n_policies > 1 the handle's first_env_id must be a multiple of 256";
        else if (e && (e->buf.first_env_id < 0 || q.envs_per_policy > INT64_MAX / q.n_policies ||
                       e->buf.first_env_id + e->n > q.n_policies * q.envs_per_policy))
            bad = "the handle's envs reach past n_policies * envs_per_policy";
    }
    return bad;
}
// a validated sbr_policy as the kernels take it
SbrPolicyDev policy_dev(const sbr_policy* policy) {
    SbrPolicyDev pl{};
    pl.n_hidden = policy->n_hidden; pl.activation = policy->activation; pl.squash = policy->squash;
    pl.noise = (policy->noise_std[0] != 0.0f || policy->noise_std[1] != 0.0f) ? 1 : 0;
    pl.n_policies = policy->n_policies; pl.envs_per_policy = policy->envs_per_policy;
    pl.stride = sbr_policy_param_count(policy->n_hidden, policy->width);
    for (int k = 0; k < 2; ++k) { pl.scale[k] = policy->act_scale[k]; pl.bias[k] = policy->act_bias[k]; pl.std[k] = policy->noise_std[k]; }
    pl.seed = policy->noise_seed;
    return pl;
}

extern "C" {

int sbr_rollout_policy(sbr_env* e, int32_t n_steps, int32_t hold, const sbr_policy* policy, float* obs, double* returns,
                       float* actions_out, double* rewards_out, void* stream) {
    // What the call has to say about its arguments; empty if they are valid.  Every check is evaluated, the LAST failing one is
    // reported - all of them before anything is touched.
    std::string bad;
    if (!e) bad = "NULL env";
    if (n_steps < 0) bad = "n_steps must be >= 0";
    if (hold < 1) bad = "hold must be >= 1";
    if (!obs) bad = "NULL obs";
    const std::string pb = policy_error(e, policy);
    if (!pb.empty()) bad = pb;
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_rollout_policy: " + bad);
    const SbrPolicyDev pl = policy_dev(policy);
    const bool wide = policy->n_hidden > 0 && policy->width == 64;     // without a hidden layer the width does not matter
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            either(wide, [&](auto w64) {
                constexpr int H = decltype(w64)::value ? 64 : 32;
                launch_fused<C::SCH>(e, e->n, stream, [](auto w) { return k_rollout_policy<H, C::OCI, C::SCH, decltype(w)::value>; },
                                     n_steps, hold, policy->params, pl, obs, returns, actions_out, rewards_out);
            });
        });
    });
}

}  // extern "C"
