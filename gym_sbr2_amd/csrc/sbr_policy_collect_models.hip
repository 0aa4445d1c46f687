// sbr_policy_collect_models.hip - the fused policy collector over DOMAIN-RANDOMISED envs, and its entry point.
//   k_models_collect_policy   k_collect_policy with every constant read from the env's own plant model - model
//              (global id / envs_per_model) % n_models of the table the handle owns (sbr_set_models, sbr_cycle_models.hip) - and not
//              from the handle's own SbrPar; both per-decision outputs optional, so that it is the models form of k_rollout_policy
//              as well (sbr_collect_policy_models)
// A unit of its own, as k_collect_policy is: its 12 builds compile next to the other policy units' instead of behind them.
#include "sbr_policy.h"

// k_collect_policy's body word for word (REPEATED and not shared, DESIGN.md sections 3.6 and 3.8), with `p` taken from the table.
// WHY PER WAVE.  Every constant of the plant is wave-uniform in the parent and read with scalar loads.  A model per LANE would be
// some 190 doubles in vector registers or behind per-lane loads; a model per WAVE is another base address for the same scalar
// loads.  The wave's model is sbr_wave_model's: the index formed once, behind a readfirstlane, from the wave's global env ids -
// the rule of the policy block of a population.
// REGISTERS.  The parent reads its constants from the kernel-argument segment wherever it needs them.  Here
// they sit behind a pointer, and a pointer the compiler can see through invites it to load a constant once in front of the call
// loop and keep it in scalar registers across it.  So the pointer is re-made at the top of every call at an offset of zero the
// compiler cannot see through (an empty asm on a scalar, on a wave-uniform path), and once more behind the loop: constants are
// scalar loads where they are used, not registers held across the step loops.
template <int H, bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_models_collect_policy(const SbrPar* __restrict__ table, uint32_t n_models, SbrBuf b,
                                                                    int64_t envs_per_model, int32_t n_steps, int32_t hold,
                                                                    const float* __restrict__ params, SbrPolicyDev pl,
                                                                    float* __restrict__ obs, double* __restrict__ returns,
                                                                    float* __restrict__ actions_out, double* __restrict__ rewards_out,
                                                                    float* __restrict__ obs_out, uint8_t* __restrict__ flags_out) {
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SBR_BLOCK, i = i0 + l;
    if (i >= b.n) return;
    if (n_steps == 0) {               // no call: the handle, obs and the per-decision outputs are left as they are
        if (returns) returns[i] = 0.0;
        return;
    }
    const uint64_t gid = (uint64_t)(b.first_env_id + i);
    // the wave's plant, and the wave's policy block (see k_rollout_policy)
    const SbrConstBytes model = sbr_wave_model(table, n_models, envs_per_model, gid);
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
    load_record<OCI>(*(const SbrPar*)model, b, i0, l, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    SbrMeta& m = rec.meta;
    float o[SBR_NOBS];
    float* __restrict__ my_obs = obs + i * SBR_NOBS;
#pragma unroll
    for (int k = 0; k < SBR_NOBS; ++k) o[k] = my_obs[k];
    float a0 = 0.0f, a1 = 0.0f;
    int32_t left = 1;                              // calls until the next decision, this one included
    uint32_t flags = 0;                            // SBR_DF_* of the decision in force
    double acc = 0.0;
    bool terminal_due = false;
    for (int32_t s = 0; s < n_steps; ++s) {
        uint32_t z = 0;
        asm volatile("" : "+s"(z));                // wave-uniform: the call loop's own top
        const SbrPar& p = *(const SbrPar*)(model + z);
        if (--left == 0) {                         // a decision call (wave-uniform): s % hold == 0
            left = hold;
            const int64_t row = (int64_t)(s / hold);
            const bool any = __builtin_amdgcn_ballot_w64(!m.done) != 0ull;
            if (any && s > 0) {
                x6.get(xa6);
                sbr_write_obs<float>(o, 1, c.t, x, xa6, x);
            }
            if (obs_out) {                         // the row the net is applied to, before the net is entered
                float* mine = obs_out + (row * b.n + i0) * SBR_NOBS + l * (uint32_t)SBR_NOBS;
#pragma unroll
                for (int k = 0; k < SBR_NOBS; ++k) mine[k] = m.done ? 0.0f : o[k];
            }
            if (any) {
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
            flags = m.done ? 0u : (uint32_t)SBR_DF_TAKEN;
            if (actions_out) {
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
            if (dn) { m.done = true; terminal_due = !OCI && p.terminal; flags |= (uint32_t)SBR_DF_ENDED; }
        }
        if (rewards_out) (rewards_out + ((int64_t)s * b.n + i0))[l] = r;
        if (flags_out && (left == 1 || s == n_steps - 1))      // the decision's last call, or the launch's (wave-uniform)
            (flags_out + ((int64_t)(s / hold) * b.n + i0))[l] = (uint8_t)flags;
    }
    uint32_t z = 0;
    asm volatile("" : "+s"(z));                    // behind the join of the loop: wave-uniform again
    const SbrPar& pe = *(const SbrPar*)(model + z);
    if (!m.done) {                    // ran every call of the launch: its observation for the next one
        x6.get(xa6);
        sbr_write_obs<float>(o, 1, c.t, x, xa6, x);
#pragma unroll
        for (int k = 0; k < SBR_NOBS; ++k) my_obs[k] = o[k];
    }
    if (terminal_due) {
        SbrHistReg hs{rec.hist};
        rec.qw = sbr_terminal<SCH>(pe, c, hs, x);
    }
    m.plan = 0;                       // a rollout reports no plan
    store_x(b, i0, l, x);
    store_record<OCI>(pe, b, i0, l, rec);
    if (returns) returns[i] = acc;
}

extern "C" {

int sbr_collect_policy_models(sbr_env* e, int64_t envs_per_model, int32_t n_steps, int32_t hold, const sbr_policy* policy, float* obs,
                              double* returns, float* actions_out, double* rewards_out, float* obs_out, uint8_t* flags_out,
                              void* stream) {
    // sbr_rollout_policy's checks and the rule's.  Every check is evaluated, the LAST failing one is reported - all of them before
    // anything is touched.
    std::string bad;
    if (!e) bad = "NULL env";
    if (n_steps < 0) bad = "n_steps must be >= 0";
    if (hold < 1) bad = "hold must be >= 1";
    if (!obs) bad = "NULL obs";
    const std::string pb = policy_error(e, policy);
    if (!pb.empty()) bad = pb;
    const std::string mb = models_error(e, envs_per_model);
    if (!mb.empty()) bad = mb;
    if (!bad.empty()) return fail(e, SBR_ERR_INVALID, "sbr_collect_policy_models: " + bad);
    const SbrPolicyDev pl = policy_dev(policy);
    const bool wide = policy->n_hidden > 0 && policy->width == 64;     // without a hidden layer the width does not matter
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            either(wide, [&](auto w64) {
                constexpr int H = decltype(w64)::value ? 64 : 32;
                launch_fused_models<C::SCH>(e, e->n, 1, stream,
                                            [](auto w) { return k_models_collect_policy<H, C::OCI, C::SCH, decltype(w)::value>; },
                                            (int64_t)envs_per_model, n_steps, hold, policy->params, pl, obs, returns, actions_out,
                                            rewards_out, obs_out, flags_out);
            });
        });
    });
}

}  // extern "C"
