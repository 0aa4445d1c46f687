// sbr_policy.h - what the three units of the policy family share (sbr_policy.hip, sbr_policy_lookahead.hip,
// sbr_policy_collect.hip): the caller's MLP as the kernels evaluate it, the noise of a decision, and the host's checks of an
// sbr_policy.
#pragma once
#include "sbr_host.h"

// The net: float32, one lane per env, activations in VGPR arrays whose every index is a compile-time constant (H is a template
// parameter: a run-time width would put the arrays in scratch); n_hidden and the activation are wave-uniform branches.  The
// arithmetic is fixed by the source: acc = b[j], then acc = fmaf(W[j][k], h[k], acc) for k ascending.  SBR_MLP_UNITS output
// units are advanced together, because one fmaf chain alone is bound by the latency of the FMA.
// The weights are wave-uniform: `w` is formed from kernel arguments and a readfirstlane only, so the loads are scalar loads
// (s_load_dwordxN) and the weight enters v_fmac_f32 as its SGPR operand - no VGPR is spent on a weight.
#define SBR_MLP_UNITS 8
struct SbrPolicyDev {                 // sbr_policy without its pointer, validated by the host
    int32_t n_hidden, activation, squash, noise;
    int64_t n_policies, envs_per_policy, stride;     // stride: floats per policy block
    float scale[2], bias[2], std[2];
    uint64_t seed;
};
// a loop whose index is a compile-time constant in every iteration, by construction (a `#pragma unroll` the optimiser may decline
// for a body this large, and ONE rolled loop over an activation array sends the whole array to scratch)
template <int I, int N, typename F>
SBR_DEV void sbr_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sbr_static_for<I + 1, N>(f);
    }
}
template <int IN, int OUT, int U>
SBR_DEV void sbr_mlp_layer(const float* __restrict__ w, const float (&h)[IN], float (&y)[OUT]) {
    static_assert(OUT % U == 0, "the output units are advanced in groups of U");
    const float* __restrict__ bias = w + OUT * IN;
    sbr_static_for<0, OUT / U>([&](auto jg) {
        constexpr int j0 = decltype(jg)::value * U;
        float acc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) acc[u] = bias[j0 + u];
        sbr_static_for<0, IN>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                acc[u] = __builtin_fmaf(w[(j0 + u) * IN + k], h[k], acc[u]);
                // each chain stays a scalar v_fmac_f32 fed from an SGPR: paired into v_pk_fma_f32 the two weights of a pair,
                // which are a row apart in memory, first have to be moved into adjacent SGPRs - two s_mov_b32 per packed FMA
                asm("" : "+v"(acc[u]));
            }
        });
#pragma unroll
        for (int u = 0; u < U; ++u) y[j0 + u] = acc[u];
    });
}
template <int H>
SBR_DEV void sbr_mlp_act(int32_t activation, float (&h)[H]) {
    if (activation == 0) {
        sbr_static_for<0, H>([&](auto jc) { h[decltype(jc)::value] = tanhf(h[decltype(jc)::value]); });
    } else {
        sbr_static_for<0, H>([&](auto jc) { h[decltype(jc)::value] = h[decltype(jc)::value] > 0.0f ? h[decltype(jc)::value] : 0.0f; });
    }
}
// the two pre-squash outputs of the net for the observation o
template <int H>
SBR_DEV void sbr_mlp(const SbrPolicyDev& pl, const float* __restrict__ w, const float (&o)[SBR_NOBS], float (&y)[2]) {
    if (pl.n_hidden == 0) {
        sbr_mlp_layer<SBR_NOBS, 2, 2>(w, o, y);
        return;
    }
    float h[H];
    sbr_mlp_layer<SBR_NOBS, H, SBR_MLP_UNITS>(w, o, h);
    sbr_mlp_act<H>(pl.activation, h);
    w += SBR_NOBS * H + H;
    if (pl.n_hidden == 2) {
        float g[H];
        sbr_mlp_layer<H, H, SBR_MLP_UNITS>(w, h, g);
        sbr_mlp_act<H>(pl.activation, g);
#pragma unroll
        for (int j = 0; j < H; ++j) h[j] = g[j];
        w += H * H + H;
    }
    sbr_mlp_layer<H, 2, 2>(w, h, y);
}
// exploration noise of a decision (k_rollout_policy, k_collect_policy): one Box-Muller pair of Philox stream 3, subsequence =
// global env id, counter = the env's calls since reset (sbr_normal_pair's construction; streams 0 - 2 are the influent, the
// random policy and the scenario draw)
SBR_DEV void sbr_policy_noise(uint64_t seed, uint64_t env_id, uint32_t call, double& z0, double& z1) {
    uint32_t c[4] = {call, 3u, (uint32_t)env_id, (uint32_t)(env_id >> 32)};
    sbr_philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u1 = sbr_u53(c[0], c[1]), u2 = sbr_u53(c[2], c[3]);
    const double rad = sqrt(-2.0 * log(u1)), ang = 6.283185307179586476925286766559 * u2;
    double sn, cs;
    sincos(ang, &sn, &cs);
    z0 = rad * cs; z1 = rad * sn;
}

// What sbr_rollout_policy, sbr_collect_policy and sbr_lookahead_policy have to say about a policy (empty if it is valid), and a validated sbr_policy
// as the kernels take it: defined in sbr_policy.hip.
SBR_INTERNAL std::string policy_error(const sbr_env* e, const sbr_policy* policy);
SBR_INTERNAL SbrPolicyDev policy_dev(const sbr_policy* policy);
