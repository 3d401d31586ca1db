// Time slots on the device: the table of time terms the rollouts and the per-instance-time ticks read, filled from a
// vector of times by the skill's own time-only sub-expressions as generated code (casclik_amd/codegen.py,
// emit_time_slots: `struct TimeSlots`), where the host otherwise walks the expression trees once per time stamp
// (lowering.py, SkillDescriptor.time_terms).
//
// A header and a translation unit of its own (jit.py, _TIME_TEMPLATE): no header that holds another kernel names this
// one, so no other kernel's code depends on it.  The includer supplies sincos_joint (clik_device.hpp).
#pragma once
#include <hip/hip_runtime.h>

namespace clik {

// One lane per table row, nothing shared between lanes (no LDS, no cross-lane traffic): 256 threads are one wave per
// SIMD of a compute unit; a rollout's table (a few hundred to a few thousand rows) is a handful of blocks either way.
constexpr int kTimeBlock = 256;

// out [n_times * stages][2 * TS::n_tslots]: row r belongs to tick r / stages, stage r % stages (stages 1 or 4), and
// holds the slots' values, then their time derivatives, at the stage time t, t + dt/2, t + dt/2, t + dt - each ONE
// rounded add (dt/2 is exact), which is the host's `times + 0.5 * dt` / `times + dt` bit for bit.  Each lane stores its
// row of 2 * n_tslots consecutive doubles (measured against the tick it feeds: profiles/time_on_device.md).
template <class TS>
__global__ void __launch_bounds__(kTimeBlock)
time_terms_kernel(const double* __restrict__ times, long long n_times, int stages, double dt, double* __restrict__ out)
{
    constexpr int W = 2 * TS::n_tslots;
    const long long r = (long long)blockIdx.x * kTimeBlock + threadIdx.x;
    if (r >= n_times * stages) return;
    const long long tick = stages == 4 ? (r >> 2) : r;
    const int stage = stages == 4 ? (int)(r & 3) : 0;
    double t = times[tick];
    if (stage == 1 || stage == 2) t = t + 0.5 * dt;
    if (stage == 3) t = t + dt;
    double tv[W > 0 ? W : 1];
    TS::eval(t, tv);
    double* row = out + r * W;
#pragma unroll
    for (int k = 0; k < W; ++k) row[k] = tv[k];
}

template <class TS>
hipError_t launch_time_terms(const double* times, long long n_times, int stages, double dt, double* out,
                             hipStream_t stream)
{
    const long long rows = n_times * (long long)stages;
    if (rows <= 0 || TS::n_tslots == 0) return hipSuccess;
    const long long blocks = (rows + kTimeBlock - 1) / kTimeBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(time_terms_kernel<TS>, dim3((unsigned)blocks), dim3(kTimeBlock), 0, stream, times, n_times, stages,
                       dt, out);
    return hipGetLastError();
}

}  // namespace clik
