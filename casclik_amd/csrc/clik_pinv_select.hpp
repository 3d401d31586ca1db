// Which pseudo-inverse kernel serves a batch: the inputs of the choice (PinvPolicy, the shape predicates, the batch
// limits), the ONE function that makes it (pinv_select) and the launch arguments that carry the policy to the kernel
// objects compiled at run time.  No kernels here: the library's host code (clik_api.hip) includes it as well as the
// launchers (clik_pinv_kernels.hpp).
#pragma once
#include "clik_device.hpp"

namespace clik {

// value-specialised lane kernel (pinv_solve_static_values_kernel): single-mode skills, and the config-3 family
// (whose lane evaluation, solo_tick, beats the one-wave-per-mode kernel once the numbers are compiled in: 5.19 / 5.26 /
// 5.44 us against 5.87 / 5.89 / 5.98 us at 20480 / 24576 / 32768 instances); other skills with up to
// CLIK_VALUE_LANE_MAX_SETS SetConstraints as an experiment switch (plan-driven sequential modes: 0-6 % over mp2)
#ifndef CLIK_VALUE_LANE_MAX_SETS
#define CLIK_VALUE_LANE_MAX_SETS 0
#endif
// ... at every batch size: without an image in LDS or registers the kernel fits two waves per SIMD with no spill,
// and the rows a lane loads / stores itself cost nothing measurable - config 3: 6.18 against 7.19 us at 65536
// instances, 10.2 against 13.3 us at 131072, 67.7 against 87.2 us at 1 M (CLIK_VALUE_LANE_MAX_BATCH caps it)
#ifndef CLIK_VALUE_LANE_MAX_BATCH
#define CLIK_VALUE_LANE_MAX_BATCH (1ll << 40)
#endif

constexpr int TEAM = 4;                     // lanes per instance = one DPP quad

// ---- batch limits ----------------------------------------------------------------------------------------------
// batches up to this many instances leave SIMDs idle (1024 SIMDs x 64 lanes / 2 waves per block)
constexpr long long kModeParallelMaxBatch = 32768;
// the team kernel runs four lanes per instance: up to 16384 instances its waves have a SIMD each; beyond,
// two of them share a SIMD's fp64 pipe and the tick doubles (measured: 5.1 us at 16384, 9.2 us at 32768 against
// 6.0 us of the two-wave kernel, profiles/r2_lanes_head_to_head.md)
constexpr long long kTeamMaxBatch = 16384;
// the value-specialised team TICK addresses its rows with 24-bit row numbers (its rollout does not)
constexpr long long kTeamValuesMaxBatch = 1ll << 24;
// from this many instances on every SIMD has several waves queued and the two-waves-per-SIMD build of the
// lane-per-instance kernel wins (pinv_solve_static_occ2_kernel)
constexpr long long kOcc2MinBatch = 524288;
constexpr long long kValueLaneMaxBatch = CLIK_VALUE_LANE_MAX_BATCH;

// ---- shape predicates ------------------------------------------------------------------------------------------
constexpr int shape_n_sets(const ShapeDesc& sd)
{
    int k = 0;
    for (int q = 0; q < sd.n_tasks; ++q) k += sd.cls[q] == CLIK_CLS_SET;
    return k;
}

// ---- the config-3 family: [joint-limit set on every state; task with m <= n state-dependent rows; joint-space task] -----
// Both modes of such a skill need only shifted copies of ONE Gram matrix Gm = J J' (J: the m x n Jacobian of the
// second constraint) - see clik_pinv_team.hpp for the algebra and the four-lanes-per-instance kernel built on it.
constexpr bool shape_team_ok(const ShapeDesc& sd)
{
    if (sd.qp || sd.n_tasks != 3 || sd.n_x != 0 || sd.standard || sd.conv_last || !sd.multidim) return false;
    if (sd.cls[0] != CLIK_CLS_SET || sd.cls[1] != CLIK_CLS_EQ || sd.cls[2] != CLIK_CLS_EQ) return false;
    if ((sd.ext[0] | sd.ext[1] | sd.ext[2]) & ~1) return false;      // (gains / bounds given as expressions)
    // the set covers every state variable exactly once (then  lam I + Jset'Jset = (1+lam) I)
    if (!shape_unit(sd, 0) || sd.m[0] != sd.n || sd.n < 2) return false;
    for (int c = 0; c < sd.n; ++c)
        if (shape_unit_row(sd, 0, c) < 0) return false;
    if (sd.const_j[1] || sd.m[1] > sd.n || sd.m[1] < 1) return false;
    if (!shape_unit(sd, 2)) return false;
    return true;
}

// The skills the value-specialised lane-per-instance kernel serves: single-mode skills without virtual variables (skills
// with SetConstraints keep the one-wave-per-mode kernels at small batches, the config-3 family its four lanes per
// instance) ...
constexpr bool shape_value_lane_ok(const ShapeDesc& sd)
{
    return sd.n_x == 0 && !sd.qp && (shape_n_sets(sd) <= CLIK_VALUE_LANE_MAX_SETS || shape_team_ok(sd));
}
// ... and those whose small batches run four lanes per instance with the sin / cos evaluations split over the quad
// (pinv_solve_static_values_quad_kernel).
constexpr bool shape_quad_front_ok(const ShapeDesc& sd)
{
    return shape_value_lane_ok(sd) && !shape_team_ok(sd) && sd.uses_fk != 0 && sd.n >= 3 && sd.n <= 2 * TEAM;
}

// ---- the choice ------------------------------------------------------------------------------------------------
// CLIK_LANES: unset / empty / 0 = the library's choice, 4 = the config-3 family's four lanes per instance at every batch
// size, anything else = one lane per instance
enum class PinvLanes : int { choice, lane, team };

// A handle's switches: clik_pinv_create reads the environment once, clik_pinv_attach_value_kernel sets values_attached.
struct PinvPolicy {
    bool mode_waves;              // CLIK_MODE_PARALLEL != 0: one wave per mode (mp2 / mp4) at small batches
    PinvLanes lanes;              // CLIK_LANES: the four-lanes-per-instance kernels of the config-3 family
    bool large_batch;             // CLIK_LARGE_BATCH != 0: the two-waves-per-SIMD lane kernel from kOcc2MinBatch on
    bool aot_large_batch_build;   // the handle runs the ahead-of-time table, the only build with that kernel
    bool values_attached;         // a value-specialised library is attached
    bool quad_front;              // CLIK_QUAD_FRONT != 0: four lanes per instance for small single-mode batches
};

// the kernel variants of a shape-specialised skill (the "v" ones have the skill's numbers compiled in)
enum class PinvVariant : int { team4, team4v, quadv, lanev, mp2, mp4, lane, lane_occ2 };
// ... the labels clik_pinv_kernel_variant reports (bench.py and the tests read them)
constexpr const char* kPinvVariantName[] = {"team4", "team4v", "quadv", "lanev", "mp2", "mp4", "lane", "lane/occ2"};

constexpr bool pinv_value_variant(PinvVariant v)
{
    return v == PinvVariant::team4v || v == PinvVariant::quadv || v == PinvVariant::lanev;
}

enum class PinvOp : int { tick, rollout };

// The kernel that serves a tick or a rollout of B instances.  The label, the library's choice between the
// value-specialised and the image-reading kernel objects, and every launcher read it.  A rollout has no quad,
// one-wave-per-mode or large-batch kernel, and its value-specialised team kernel has no 24-bit row limit.
constexpr PinvVariant pinv_select(const ShapeDesc& sd, const PinvPolicy& p, long long B, PinvOp op)
{
    const bool team = shape_team_ok(sd) &&
                      (p.lanes == PinvLanes::team || (p.lanes == PinvLanes::choice && B <= kTeamMaxBatch));
    if (p.values_attached) {
        if (team && (op == PinvOp::rollout || B <= kTeamValuesMaxBatch)) return PinvVariant::team4v;
        if (shape_value_lane_ok(sd) && B <= kValueLaneMaxBatch) {
            if (op == PinvOp::tick && shape_quad_front_ok(sd) && B <= kTeamMaxBatch && p.quad_front)
                return PinvVariant::quadv;
            return PinvVariant::lanev;
        }
    }
    if (team) return PinvVariant::team4;
    if (op == PinvOp::rollout) return PinvVariant::lane;
    const int ns = shape_n_sets(sd);
    if ((ns == 1 || ns == 2) && sd.n_x == 0 && p.mode_waves && B <= kModeParallelMaxBatch / ((1 << ns) / 2))
        return ns == 1 ? PinvVariant::mp2 : PinvVariant::mp4;
    if (p.aot_large_batch_build && p.large_batch && B >= kOcc2MinBatch) return PinvVariant::lane_occ2;
    return PinvVariant::lane;
}

// common launcher signature of the kernel table; the library passes it to the objects compiled at run time too
struct LaunchArgs {
    const DevSkill* dS;        // dynamic kernels
    const void*     dImg;      // static kernels: device copy of the skill image
    const WarmArgs* warm;
    int nq, nx, ny;
    PinvPolicy policy;
    double* roll_x;            // rollout of a skill with virtual variables: their state (in/out) and last rates
    double* roll_dx;
    int roll_stages;           // rollout: controller evaluations per tick (0 / 1 explicit Euler, 4 Runge-Kutta)
    const double* t_inst;      // solve: one time-slot record per instance ([B][2 * n_tslots], device) or null
    const RollRec* roll_rec;   // recording / per-tick-target rollout (host copy, read by the launcher) or null
};

}  // namespace clik
