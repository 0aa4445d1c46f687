// sbr_amd.hip (build.SRC) - the library as ONE translation unit, for a tool that takes a single file.  The library itself is built
// from these units apart, side by side (build.SOURCES, build.compile_library()).
#include "sbr_core.hip"
#include "sbr_rollout.hip"
#include "sbr_tape.hip"
#include "sbr_sampled.hip"
#include "sbr_policy.hip"
#include "sbr_policy_lookahead.hip"
#include "sbr_policy_collect.hip"
#include "sbr_policy_collect_models.hip"
#include "sbr_cycle_lookahead.hip"
#include "sbr_cycle_scenarios.hip"
#include "sbr_cycle_models.hip"
#include "sbr_lookahead_models.hip"
