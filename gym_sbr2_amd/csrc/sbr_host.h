// sbr_host.h - the host side every translation unit of libsbr_amd.so shares: the handle, error reporting, the frame of an
// entry point, the launch shapes and the one place that turns run-time choices into template arguments.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <type_traits>

#include "sbr_kernels.h"

#define SBR_INTERNAL __attribute__((visibility("hidden")))     // shared between the units, not part of the C ABI

struct sbr_env {
    int64_t n = 0;
    int device = 0;
    int64_t first_env_id = 0;
    sbr_config cfg;
    SbrPar par;
    SbrBuf buf{};
    double* tables = nullptr;     // [2][8][14][48] on the device
    int64_t one_wave_envs = 65536; // lanes of one wave per SIMD on this device: CUs x 4 SIMDs x 64 (MI355X: 256 CUs)
    bool have_tables = false;
    SbrPar* models = nullptr;     // [n_models] on the device: the plant models of sbr_set_models (sbr_cycle_models.hip), or none
    int64_t n_models = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
};

// A config folded into the constants the kernels read, and what sbr_create has to say about a config (empty if it is valid):
// defined in sbr_core.hip, shared with sbr_set_models / sbr_check_model (sbr_cycle_models.hip).
SBR_INTERNAL void derive_params(const sbr_config& c, SbrPar& p);
SBR_INTERNAL std::string config_error(const sbr_config& c);

// Defined once, in sbr_core.hip, next to the calling thread's error text it writes when there is no handle (sbr_last_error(NULL)):
// a copy per unit would each keep a text of its own.
SBR_INTERNAL int fail(sbr_env* e, int code, const std::string& msg);
// A failed HIP call.  Only sbr_create passes no handle (the one it is building is not the caller's yet), and only there does
// running out of device memory have a code of its own.
static inline int hip_fail(sbr_env* e, hipError_t s, const char* call) {
    return fail(e, !e && s == hipErrorOutOfMemory ? SBR_ERR_ALLOC : SBR_ERR_HIP, std::string(call) + ": " + hipGetErrorString(s));
}
#define HIP_TRY(e, call)                                          \
    do {                                                          \
        hipError_t _s = (call);                                   \
        if (_s != hipSuccess) return hip_fail(e, _s, #call);      \
    } while (0)

static inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + SBR_BLOCK - 1) / SBR_BLOCK)); }

// Entry points run on the handle's device and leave the caller's current device as they found it (a process may drive
// several GPUs, and torch tracks the current device itself).
struct DeviceGuard {
    int prev = -1;
    hipError_t status = hipSuccess;
    explicit DeviceGuard(int device) {
        int cur = -1;
        status = hipGetDevice(&cur);
        if (status == hipSuccess && cur != device) { status = hipSetDevice(device); prev = cur; }
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define ON_DEVICE(e)                      \
    DeviceGuard _guard((e)->device);      \
    HIP_TRY(e, _guard.status)
// The frame of an entry point that only launches kernels, behind its own argument check: launch() runs on the handle's device
// and the launch status is collected once behind it.  (Entry points that copy or wait check each call where it is made:
// ON_DEVICE, then HIP_TRY per call.)
template <typename Launch> static int launched(sbr_env* e, Launch&& launch) {
    ON_DEVICE(e);
    launch();
    HIP_TRY(e, hipGetLastError());
    return SBR_OK;
}

// Launch shapes.  Each decision is taken once, here: the launch sites and sbr_query both read these functions.
#define SBR_SMALL_BATCH 49152       // up to this many envs k_step runs in 64-thread workgroups (measured: profiles/r02_ab_block.log)
static inline int step_block(const sbr_env* e) { return e->n <= SBR_SMALL_BATCH ? 64 : 256; }
// A launch with more wavefronts than the device has SIMDs (MI355X: 1024 SIMDs x 64 lanes = 65536 envs; a partitioned device has
// fewer) runs the two-waves-per-SIMD build of the scheme-1 k_step.
static inline int64_t step_two_waves_above(const sbr_env* e) { return e->one_wave_envs > SBR_SMALL_BATCH ? e->one_wave_envs : SBR_SMALL_BATCH; }
static inline int step_waves(const sbr_env* e) { return e->cfg.scheme == 1 && e->n > step_two_waves_above(e) ? 2 : 1; }
// up to 1.5 waves per SIMD (MI355X: 98304 envs) the fused scheme-1 kernels (k_rollout, k_cycle) run their uncapped-register build
static inline int64_t fused_one_wave_max(const sbr_env* e) { return e->one_wave_envs + e->one_wave_envs / 2; }
static inline int fused_waves(const sbr_env* e) { return e->cfg.scheme == 1 && e->n <= fused_one_wave_max(e) ? 1 : 2; }
// the same decision for a launch of `lanes` lanes that are not the handle's envs (sbr_lookahead_actions: one lane per branch)
static inline int fused_waves_for(const sbr_env* e, int64_t lanes) { return e->cfg.scheme == 1 && lanes <= fused_one_wave_max(e) ? 1 : 2; }
// more waves than SIMDs: k_reset in 512-thread workgroups, two waves per SIMD
static inline int reset_block(const sbr_env* e) { return e->n > e->one_wave_envs ? 512 : SBR_RESET_BLOCK; }

// The handle's run-time choices as template arguments.  This is the only place that turns one into the other: f is called with
// a Choice that names the output and action types, whether the reward is the operating cost (reward_kind 2) and the scheme.
// A launch site names its kernel once, with the members of the Choice it needs.  Which WAVES builds of a kernel exist stays
// with the launch site: a kernel is instantiated wherever its name is spelled, taken or not.
template <typename OutT_, typename ActT_, bool OCI_, int SCH_>
struct Choice {
    using OutT = OutT_;
    using ActT = ActT_;
    static constexpr bool OCI = OCI_;
    static constexpr int SCH = SCH_;
};
template <typename F> static void either(bool c, F&& f) { if (c) f(std::true_type{}); else f(std::false_type{}); }
template <typename F> static void dispatch(const sbr_env* e, F&& f) {
    either(e->cfg.out_f64, [&](auto o64) { either(e->cfg.act_f64, [&](auto a64) {
        either(e->cfg.reward_kind == 2, [&](auto oci) { either(e->cfg.scheme == 1, [&](auto b5) {
            f(Choice<std::conditional_t<decltype(o64)::value, double, float>, std::conditional_t<decltype(a64)::value, double, float>,
                     decltype(oci)::value, decltype(b5)::value ? 1 : 0>{});
        }); });
    }); });
}

// the fused kernels (k_cycle, k_rollout and the kernels behind it): scheme 0 has no one-wave build (fused_waves is 2 for it)
template <int SCH> constexpr int kFusedOneWave = SCH == 1 ? 1 : 2;
// The launch of a fused kernel over `lanes` lanes: the handle's envs, or the branches of a lookahead - the register budget goes by
// the lanes of THE launch.  kernel(w) names the build for decltype(w)::value waves per SIMD; e->par and e->buf lead its arguments.
// That order is relied on: k_cycle_lookahead and k_cycle_lookahead_scenarios read SbrPar a second time at offset 0 of their
// kernel-argument segment (sbr_cycle_lookahead.hip, sbr_cycle_scenarios.hip: each asserts the first parameter of its builds).
template <int SCH, typename Kernel, typename... Args>
static void launch_fused(const sbr_env* e, int64_t lanes, void* stream, Kernel&& kernel, Args... args) {
    const auto fn = fused_waves_for(e, lanes) == 1 ? kernel(std::integral_constant<int, kFusedOneWave<SCH>>{})
                                                   : kernel(std::integral_constant<int, 2>{});
    hipLaunchKernelGGL(fn, grid_for(lanes), dim3(SBR_BLOCK), 0, (hipStream_t)stream, e->par, e->buf, args...);
}

// launch_fused on a two-dimensional grid, for the kernels that read their constants from the handle's model table and not from
// e->par (k_cycle_lookahead_models, sbr_cycle_models.hip; with rows_y = 1 k_models_collect_policy,
// sbr_policy_collect_models.hip): lanes_x lanes along x, rows_y <= 65535 rows along y, the register budget by their product.
// e->models, e->n_models and e->buf lead the arguments.
template <int SCH, typename Kernel, typename... Args>
static void launch_fused_models(const sbr_env* e, int64_t lanes_x, int32_t rows_y, void* stream, Kernel&& kernel, Args... args) {
    const auto fn = fused_waves_for(e, lanes_x * rows_y) == 1 ? kernel(std::integral_constant<int, kFusedOneWave<SCH>>{})
                                                              : kernel(std::integral_constant<int, 2>{});
    hipLaunchKernelGGL(fn, dim3(grid_for(lanes_x).x, (unsigned)rows_y), dim3(SBR_BLOCK), 0, (hipStream_t)stream,
                       (const SbrPar*)e->models, (uint32_t)e->n_models, e->buf, args...);
}

// What sbr_reset_models and sbr_collect_policy_models have to say about the rule "env g is plant (g / envs_per_model) % n_models"
// on this handle (empty if it can be applied; the last failing check is reported; a NULL handle is the caller's to report):
// defined in sbr_cycle_models.hip, next to the table.
SBR_INTERNAL std::string models_error(const sbr_env* e, int64_t envs_per_model);

// the type of a kernel's first parameter, for the units that assert the order launch_fused relies on
template <typename F> struct SbrFirstParam;
template <typename A, typename... R> struct SbrFirstParam<void (*)(A, R...)> { using type = A; };

// The kernel around a cycle lookahead's branch body (sbr_cycle_lookahead.hip, sbr_cycle_scenarios.hip, sbr_cycle_models.hip):
// K<ActT, SCH, WAVES> calls BRANCH<ActT, SCH>.  PARAMS(ActT) is the parameter list both share, the rest of the arguments its names.
// The two-waves build of scheme 1 is an explicit specialisation per tape type.  Two waves per SIMD leave a wave 256 registers;
// such a build, like k_cycle's, wants more and spills the rest to scratch.  How many of the 256 it ends up naming is the
// allocator's business: an even count of ordinary registers plus those that hold spilled scalars in their lanes - 252 + 3 = 255 in
// k_cycle, 254 + 2 = 256 in k_cycle_lookahead, with fewer scalars spilled.  amdgpu_num_vgpr(127) asks for 2 x 127 = 254 of the
// unified file (vector + accumulation registers): k_cycle_lookahead then takes 254 registers and 68 B of scratch per lane against
// k_cycle's 255 and 92 B (without the attribute: 256 registers), so that it needs no more than k_cycle of either.  An attribute
// takes no template argument, hence specialisations and not a condition on WAVES.
#define SBR_CYCLE_KERNEL(K, BRANCH, PARAMS, ...)                                                                              \
    template <typename ActT, int SCH, int WAVES>                                                                              \
    __global__ __launch_bounds__(SBR_BLOCK, WAVES) void K(PARAMS(ActT)) {                                                     \
        BRANCH<ActT, SCH>(__VA_ARGS__);                                                                                       \
    }                                                                                                                         \
    template <>                                                                                                               \
    __global__ __launch_bounds__(SBR_BLOCK, 2) __attribute__((amdgpu_num_vgpr(127))) void K<float, 1, 2>(PARAMS(float)) {     \
        BRANCH<float, 1>(__VA_ARGS__);                                                                                        \
    }                                                                                                                         \
    template <>                                                                                                               \
    __global__ __launch_bounds__(SBR_BLOCK, 2) __attribute__((amdgpu_num_vgpr(127))) void K<double, 1, 2>(PARAMS(double)) {   \
        BRANCH<double, 1>(__VA_ARGS__);                                                                                       \
    }
// SBR_CYCLE_KERNEL for a branch that reads the constants a second time at offset 0 of the kernel-argument segment: every build -
// the specialisations are written out on their own - takes SbrPar by value as its FIRST parameter.  (That the host fills it from
// e->par is launch_fused's.)
#define SBR_TAKES_PAR_FIRST(K, ...) std::is_same_v<SbrFirstParam<decltype(&K<__VA_ARGS__>)>::type, SbrPar>
#define SBR_CYCLE_KERNEL_PAR_FIRST(K, BRANCH, PARAMS, ...)                                                   \
    SBR_CYCLE_KERNEL(K, BRANCH, PARAMS, __VA_ARGS__)                                                         \
    static_assert(SBR_TAKES_PAR_FIRST(K, float, 1, 1) && SBR_TAKES_PAR_FIRST(K, double, 1, 1) &&             \
                      SBR_TAKES_PAR_FIRST(K, float, 1, 2) && SBR_TAKES_PAR_FIRST(K, double, 1, 2) &&         \
                      SBR_TAKES_PAR_FIRST(K, float, 0, 2) && SBR_TAKES_PAR_FIRST(K, double, 0, 2),           \
                  #K " reads SbrPar at offset 0 of its kernel-argument segment");

// Argument checks that several families share, and the one kernel two of them launch without owning it: defined in
// sbr_tape.hip, which owns k_branch_best.
SBR_INTERNAL void fanout_error(std::string& bad, const sbr_env* e, int32_t fanout, const char* word);
SBR_INTERNAL void best_error(std::string& bad, const double* returns, const int32_t* best_index, const double* best_return);
SBR_INTERNAL std::string end_error(int32_t n_steps, const void* obs_end, const void* state_end, const void* done_end);
SBR_INTERNAL void launch_branch_best(const sbr_env* e, int32_t fanout, const double* values, int32_t* best_index, double* best_value,
                                     void* stream);
// What sbr_lookahead_actions / sbr_lookahead_sampled (and their _end forms) have to say about the arguments they share, for the
// models forms of the two (sbr_lookahead_models.hip): defined in sbr_tape.hip and in sbr_sampled.hip, next to the entry points.
SBR_INTERNAL std::string lookahead_error(const sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* actions,
                                         const double* returns, const int32_t* best_index, const double* best_return);
SBR_INTERNAL std::string lookahead_sampled_error(const sbr_env* e, int32_t n_steps, int32_t hold, int32_t fanout, const void* nominal,
                                                 const sbr_sampler* sampler, const double* returns, const int32_t* best_index,
                                                 const double* best_return);
// What sbr_cycle_lookahead, sbr_cycle_lookahead_scenarios and sbr_cycle_lookahead_models have to say about their arguments (empty
// if they are valid): defined in sbr_cycle_lookahead.hip, which has the ordered list and what each argument switches.
SBR_INTERNAL std::string cycle_lookahead_error(const sbr_env* e, int32_t n_cycles, int32_t fanout, const int32_t* n_scen,
                                               int32_t max_scen, const void* actions, bool need_influent, const void* influent,
                                               bool need_table, const double* returns, bool best_of_means, const double* mean_out,
                                               const double* worst_out, const int32_t* best_index, const double* best_value,
                                               bool end_rows);
// k_scenario_stats for a caller outside its unit (sbr_cycle_scenarios.hip owns it): mean and worst of each pair's n_scen returns
SBR_INTERNAL void launch_scenario_stats(const double* returns, int64_t n_pairs, int32_t n_scen, double* mean_out, double* worst_out,
                                        void* stream);
// The reduce tail of a lookahead over futures, behind its kernel on the same stream: mean and worst of each pair's returns where
// either was asked for, then the winners among an env's means where they were.
static inline void launch_stats_and_best(const sbr_env* e, int32_t fanout, int32_t n_scen, const double* returns, double* mean_out,
                                         double* worst_out, int32_t* best_index, double* best_value, void* stream) {
    launch_scenario_stats(returns, e->n * (int64_t)fanout, n_scen, mean_out, worst_out, stream);
    launch_branch_best(e, fanout, mean_out, best_index, best_value, stream);
}
