// sbr_rollout.hip - the fused kernels that draw or take their actions per env themselves, and their entry points.
//   k_rollout  n_steps fused step()s with an on-device Philox policy, plant state stays in VGPRs (sbr_rollout)
//   k_cycle    the per-cycle env SBR-v2: one launch = one whole 12 h cycle, 528 control intervals (sbr_cycle_step; its reset,
//              k_cycle_reset, shares the influent code of k_reset and lives in sbr_core.hip)
#include "sbr_host.h"

// ------------------------------------------------------------------------------------------- rollout
// WAVES: resident waves per SIMD the register budget is cut for.  Scheme 1 keeps more state live (five 9-vectors and the step
// constants of the Butcher-5 steps): capped at 256 registers for two waves per SIMD it spills ~170 B per lane to scratch, which
// pays only where two waves ARE resident - launches above 98 304 envs; up to there the uncapped build runs (measured, round 5:
// 65 536 envs 6.6 against 7.3 us per call, 131 072 envs 11.6 against 10.8).
template <bool OCI, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_rollout(SbrPar p, SbrBuf b, int32_t n_steps, uint64_t policy_seed,
                                                      double* __restrict__ returns, float* __restrict__ actions_out) {
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SBR_BLOCK, i = i0 + l;
    if (i >= b.n) return;
    const uint64_t gid = (uint64_t)(b.first_env_id + i);
    double x[SBR_NX], xa6[SBR_NXD];
    // x6 and the ten Kla values stay in registers.  With the terminal phases INSIDE the loop over the calls the kernel needed
    // 268 VGPRs and, capped at 256 for two waves per SIMD, spilled six loop invariants to 52 B of scratch per lane; parking x6 or
    // the history in LDS removed the spill and was 1 - 2 % slower.  Running settle / draw / idle once AFTER the loop (a finished
    // lane skips every later call, so nothing changes in between) gives 243 VGPRs, no scratch and 2 - 3 % less time per call
    // (profiles/r03_ab_rollout_scratch.log, r03_ab_rollout_terminal_after_loop.log).
    SbrX6Reg x6;
    SbrRewardParts rp;
    load_x(b, i0, l, x);
    SbrRecord rec;
    load_record<OCI>(p, b, i0, l, x[8], x[9], rec);
    SbrCtl& c = rec.c;
    SbrMeta& m = rec.meta;
    double acc = 0.0;
    bool terminal_due = false;        // the done call happened in this launch: its settle / draw / idle run once, after the loop
    for (int32_t s = 0; s < n_steps; ++s) {
        float a0, a1;
        sbr_policy_action(p, policy_seed, gid, (uint32_t)m.steps, a0, a1);
        if (actions_out) reinterpret_cast<float2*>(actions_out)[(int64_t)s * b.n + i] = make_float2(a0, a1);
        if (m.done) continue;
        double t_obs;
        bool dn;
        sbr_run_intervals<SCH>(p, c, x, (double)a0, (double)a1, x6, SbrNoTrace{});
        x6.get(xa6);
        SbrHistReg hs{rec.hist};
        const double r = sbr_finish_step<OCI, SCH, SbrHistReg, false>(p, c, hs, x, xa6, t_obs, dn, rec.qw, rec.ksum, rp);
        acc += r; rec.ret += r; m.status |= c.st_new;
        m.steps = SbrMeta::next_steps(m.steps);
        if (dn) { m.done = true; terminal_due = !OCI && p.terminal; }
    }
    if (terminal_due) {               // a finished lane skipped every later call, so c, x and hist are as the done call left them
        SbrHistReg hs{rec.hist};
        rec.qw = sbr_terminal<SCH>(p, c, hs, x);
    }
    m.plan = 0;                       // a rollout reports no plan
    store_x(b, i0, l, x);
    store_record<OCI>(p, b, i0, l, rec);
    if (returns) returns[i] = acc;
}

// SbrEnv2.step: one whole 12 h cycle per env (528 control intervals; scheme 1: adaptive Butcher-5 steps on all but the 24 fill
// intervals, scheme 0: x 10 RK4 substeps) in one launch.
template <typename OutT, typename ActT, int SCH, int WAVES>
__global__ __launch_bounds__(SBR_BLOCK, WAVES) void k_cycle(SbrPar p, SbrBuf b, const ActT* __restrict__ action, OutT* __restrict__ obs,
                                                    OutT* __restrict__ reward, double* __restrict__ diag) {
    const uint32_t l = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * SBR_BLOCK, i = i0 + l;
    if (i >= b.n) return;
    double x[SBR_NX], ld[SBR_NX], o3[3];
    load_x(b, i0, l, x);
#pragma unroll
    for (int j = 0; j < SBR_NX; ++j) ld[j] = INFL(j);
    ld[0] = (p.WV - x[0]) * p.inv_t_ph0;                              // Qin / (t_cycle * t_ratio[0]), gym_SBR_env2.py:144 (host reciprocal: 1 ulp)
    const int st0 = sbr_status_bits(p, x);
    const double r = sbr_cycle_env<SCH>(p, x, ld, (double)action[3 * i], (double)action[3 * i + 1], (double)action[3 * i + 2], o3,
                                   diag ? diag + i * SBR_NCYC_DIAG : nullptr, 1);
    store_x(b, i0, l, x);
    CTRL(R_RET) = CTRL(R_RET) + r; CTRL(R_T) = p.t_cycle;
    CTRL(R_META) = SbrMeta::pack({1, st0 | sbr_status_bits(p, x), true});
    if (obs) { obs[i * 3 + 0] = (OutT)o3[0]; obs[i * 3 + 1] = (OutT)o3[1]; obs[i * 3 + 2] = (OutT)o3[2]; }
    if (reward) reward[i] = (OutT)r;
}

extern "C" {

int sbr_cycle_step(sbr_env* e, const void* action, void* obs, void* reward, double* diag, void* stream) {
    if (!e || !action) return fail(e, SBR_ERR_INVALID, "sbr_cycle_step: NULL env or action");
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            using T = typename C::OutT;
            using A = typename C::ActT;
            launch_fused<C::SCH>(e, e->n, stream, [](auto w) { return k_cycle<T, A, C::SCH, decltype(w)::value>; }, (const A*)action,
                                 (T*)obs, (T*)reward, diag);
        });
    });
}

int sbr_rollout(sbr_env* e, int32_t n_steps, uint64_t policy_seed, double* returns, float* actions_out, void* stream) {
    if (!e || n_steps < 0) return fail(e, SBR_ERR_INVALID, "sbr_rollout: bad argument");
    return launched(e, [&] {
        dispatch(e, [&](auto c) {
            using C = decltype(c);
            launch_fused<C::SCH>(e, e->n, stream, [](auto w) { return k_rollout<C::OCI, C::SCH, decltype(w)::value>; }, n_steps,
                                 policy_seed, returns, actions_out);
        });
    });
}

}  // extern "C"
