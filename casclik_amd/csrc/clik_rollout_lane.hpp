// What the lane-per-instance, image-in-LDS rollouts of both controllers share, each part once: a wave's place in the batch,
// the rows into LDS and out of it, the clamp that reports the step, the hook a rollout may carry through its ticks, the
// waves-per-block chooser, and on the host the launch above 64 KB of dynamic LDS and the scratch query.  Included by the
// recording rollouts' two headers and by nothing else, so only the on-demand translation units see it (casclik_amd/jit.py):
// the plain rollouts keep their own text (clik_pinv_kernels.hpp, clik_pinv_team.hpp, clik_qp_static.hpp) and compile from it
// unchanged.  What is NOT here - clamp and Euler step, the Runge-Kutta bookkeeping, the per-tick target feed - stays written
// out in each controller's lane body: moved into helpers, the recording kernels' code was no longer the same instruction for
// instruction (tools/isa_compare.py), and those kernels are held to that.
#pragma once
#include "clik_pinv_kernels.hpp"
namespace clik {

// A wave's place in the batch, WV waves per block: every wave owns 64 instances.  All waves of a block meet the same
// barriers, so a wave past the end of the batch (idle; WV > 1 only) works on the first rows again and stores nothing.
template <int WV>
struct WavePlace {
    int lane, wave;
    long long b0;               // first instance of the wave's rows
    int rows_valid, rows_store; // rows to load (> 0), rows to store
    bool valid, idle;
    __device__ __forceinline__ explicit WavePlace(const long long B)
    {
        if constexpr (WV == 1) {
            lane = threadIdx.x;
            wave = 0;
            idle = false;
            b0 = (long long)blockIdx.x * WAVE;
        } else {
            lane = threadIdx.x & (WAVE - 1);
            wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
            const long long b_own = ((long long)blockIdx.x * WV + wave) * WAVE;
            idle = b_own >= B;
            b0 = idle ? 0 : b_own;
        }
        const long long left = B - b0;                  // (> 0)
        rows_valid = left < WAVE ? (int)left : WAVE;
        rows_store = idle ? 0 : rows_valid;
        valid = !idle && lane < rows_valid;
    }
};

// doubles of a wave's own LDS region: zs (N slots) ys (n_y slots) (Runge-Kutta: z0s, kss, N slots each), then `extra`
template <const ShapeDesc& SD, bool RK>
constexpr int lane_wave_doubles(const int extra)
{
    return (SD.n + (SD.n_y > 0 ? SD.n_y : 0) + (RK ? 2 * SD.n : 0)) * WAVE + extra;
}

// The wave's q / x / y rows on their way into LDS: all loads in flight first (one memory round trip), then the copies.
template <int NQ, int NX, int NY>
struct StagedRows {
    double qv[NQ], xv[NX > 0 ? NX : 1], yv[NY > 0 ? NY : 1];
    template <int WV>
    __device__ __forceinline__ void load(const double* q, const double* x, const double* y, const WavePlace<WV>& w)
    {
        stage_load<NQ>(q + w.b0 * NQ, NQ, w.rows_valid, w.lane, qv);
        if constexpr (NX > 0) stage_load<NX>(x + w.b0 * NX, NX, w.rows_valid, w.lane, xv);
        if constexpr (NY > 0) stage_load<NY>(y + w.b0 * NY, NY, w.rows_valid, w.lane, yv);
    }
    __device__ __forceinline__ void to_lds(double* zs, double* xs, double* ys, const int lane) const
    {
        rows_to_lds<NQ>(qv, zs, lane);
        if constexpr (NX > 0) rows_to_lds<NX>(xv, xs, lane);
        if constexpr (NY > 0) rows_to_lds<NY>(yv, ys, lane);
    }
};

// The lanes' values v = [robot (NQ); virtual (NX)] out through the wave's state slots, coalesced: once for the state,
// once more for the velocity.  also(): what else goes to LDS between the two barriers (the QP's slack).
template <int NQ, int NX, int WV, class ALSO>
__device__ __forceinline__ void rows_out(const double (&v)[NQ + NX], double* gq, double* gx, const WavePlace<WV>& w,
                                         double* zs, double* xs, ALSO&& also)
{
    __syncthreads();
    state_to_lds<NQ, NX>(v, zs, xs, w.lane);
    also();
    __syncthreads();
    rows_from_lds<NQ>(gq + w.b0 * NQ, w.rows_store, zs, w.lane);
    if constexpr (NX > 0) rows_from_lds<NX>(gx + w.b0 * NX, w.rows_store, xs, w.lane);
}
template <int NQ, int NX, int WV>
__device__ __forceinline__ void rows_out(const double (&v)[NQ + NX], double* gq, double* gx, const WavePlace<WV>& w,
                                         double* zs, double* xs)
{
    rows_out<NQ, NX>(v, gq, gx, w, zs, xs, []() {});
}

// clamp(+-max_speed) on the robot variables; returns the largest step a robot variable would take (the caller decides whether to take it)
template <int N, int NQ>
__device__ __forceinline__ double clamp_step_size(double (&v)[N], const double max_speed, const double dt)
{
    double step = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        double d = v[j];
        if (j < NQ && max_speed > 0.0) d = fmax(fmin(d, max_speed), -max_speed);
        v[j] = d;
        if (j < NQ) step = fmax(step, fabs(d) * dt);
    }
    return step;
}

// What a rollout may carry through its ticks beside the record: start(base, lane, valid, inst) before the first barrier,
// with the base of its own LDS_DOUBLES behind the wave's region; tick(S, tk, z, ys, lane, tick, n_ticks, valid) at the top
// of a tick, with the record the tick acts on (Runge-Kutta: the first stage's); finish(valid, n_ticks, inst) after the
// loop.  This one is nothing, at compile time: the recording rollouts.
struct NoTickHook {
    static constexpr bool ACTIVE = false;
    static constexpr int LDS_DOUBLES = 0;
    template <class... A>
    __device__ __forceinline__ void start(const A&...) {}
    template <class... A>
    __device__ __forceinline__ void tick(const A&...) {}
    template <class... A>
    __device__ __forceinline__ void finish(const A&...) {}
};

// waves per block, 1 to 4, of a kernel whose block of wv waves takes BYTES(wv) of LDS: what puts most waves on a compute
// unit (four SIMDs, one wave each: the kernels hold the whole register file), the fewest waves per block among equals;
// 0: not even one wave fits under `cap`
template <size_t (*BYTES)(int)>
constexpr int waves_per_block(const size_t cap)
{
    int best = 0, best_cu = 0;
    for (int wv = 1; wv <= 4; ++wv) {
        const size_t bytes = BYTES(wv);
        if (bytes > cap) continue;
        int cu = (int)(cap / bytes) * wv;
        cu = cu > 4 ? 4 : cu;
        if (cu > best_cu) {
            best_cu = cu;
            best = wv;
        }
    }
    return best;
}

// launch with `shmem` bytes of dynamic LDS: above 64 KB the kernel's limit is raised first
template <class... P, class... A>
inline hipError_t launch_with_lds(void (*kernel)(P...), const unsigned grid, const unsigned block, const size_t shmem,
                                  hipStream_t stream, const A&... args)
{
    if (shmem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), shmem, stream, args...);
    return hipGetLastError();
}

// bytes of scratch per lane as the loaded code object states them (-1: no device to ask)
inline long long kernel_scratch_bytes(const void* kernel)
{
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, kernel) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return (long long)fa.localSizeBytes;
}

}  // namespace clik
