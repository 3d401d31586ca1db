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
// A hook with FEEDS is also called at the end of a tick, behind the tick's record and the reload of a per-tick target with
// its barrier: fed(v, bad_hi, yrow) with the velocity the tick was integrated with (after the clamp; Runge-Kutta: the
// combined rate), the NaN bits of an instance the record shows as NaN (QP: infeasible so far) and the lane's own target
// row in LDS.
struct NoTickHook {
    static constexpr bool ACTIVE = false;
    static constexpr bool FEEDS = false;
    static constexpr int LDS_DOUBLES = 0;
    template <class... A>
    __device__ __forceinline__ void start(const A&...) {}
    template <class... A>
    __device__ __forceinline__ void tick(const A&...) {}
    template <class... A>
    __device__ __forceinline__ void fed(const A&...) {}
    template <class... A>
    __device__ __forceinline__ void finish(const A&...) {}
};

// The velocity feedback of the on-device loops (include/clik.h: the rule), compiled in as CLIK_CONVERGE_GROUP is:
// -DCLIK_VELOCITY_FEEDBACK={f_0,...,f_{N-1}}, one entry per state (robot variables, then virtual ones): f_j >= 0 names the
// entry of the instance's input_var row that the next tick reads the velocity of state j in, -1 none.  Without the flag
// there is no map, every use below is behind `if constexpr`, and the units compile to the code they had.
#ifdef CLIK_VELOCITY_FEEDBACK
inline constexpr int kVelFeedbackMap[] = CLIK_VELOCITY_FEEDBACK;
constexpr int kVelFeedbackN = (int)(sizeof(kVelFeedbackMap) / sizeof(kVelFeedbackMap[0]));
#else
inline constexpr int kVelFeedbackMap[1] = {-1};
constexpr int kVelFeedbackN = 0;
#endif

constexpr size_t kLaneLdsCap = 160u * 1024u;        // LDS of one compute unit (gfx950): what a block of a lane rollout may take

// what a unit's info query says about the map: k = 0 its length (0: compiled without), k = 1 + j entry j (-1 beyond it)
inline long long velocity_feedback_info(const int k)
{
    if (k == 0) return kVelFeedbackN;
    return (k >= 1 && k <= kVelFeedbackN) ? kVelFeedbackMap[k - 1] : -1;
}

// the fed entries of the lane's own target row: every lane writes its own row and nobody else's, so no barrier
template <const ShapeDesc& SD>
__device__ __forceinline__ void velocity_feed(const double (&v)[SD.n], const unsigned bad_hi, double* yrow)
{
    static_assert(kVelFeedbackN == SD.n, "CLIK_VELOCITY_FEEDBACK has one entry per robot and virtual variable");
    if constexpr (kVelFeedbackN == SD.n) {
        static_for<0, SD.n>([&](auto jc) __attribute__((always_inline)) {
            constexpr int j = decltype(jc)::value;
            constexpr int k = kVelFeedbackMap[j];
            static_assert(k >= -1 && k < (SD.n_y > 0 ? SD.n_y : 0), "CLIK_VELOCITY_FEEDBACK: an entry outside input_var");
            if constexpr (k >= 0) yrow[k] = nan_or(v[j], bad_hi);
        });
    }
}

// the feedback as a hook of the lane-per-instance rollouts
template <const ShapeDesc& SD>
struct VelocityFeedbackHook : NoTickHook {
    static constexpr bool FEEDS = true;
    __device__ __forceinline__ void fed(const double (&v)[SD.n], const unsigned bad_hi, double* yrow)
    {
        velocity_feed<SD>(v, bad_hi, yrow);
    }
};

// two hooks as one: A (made from the constructor's arguments) with its LDS first, then B
template <class A, class B>
struct ComposeHook {
    static constexpr bool ACTIVE = A::ACTIVE || B::ACTIVE;
    static constexpr bool FEEDS = A::FEEDS || B::FEEDS;
    static constexpr int LDS_DOUBLES = A::LDS_DOUBLES + B::LDS_DOUBLES;
    A a;
    B b;
    template <class... P>
    __device__ __forceinline__ explicit ComposeHook(const P&... p) : a{p...}, b{} {}
    __device__ __forceinline__ void start(double* base, const int lane, const bool valid, const long long inst)
    {
        a.start(base, lane, valid, inst);
        b.start(base + A::LDS_DOUBLES, lane, valid, inst);
    }
    template <class... P>
    __device__ __forceinline__ void tick(const P&... p)
    {
        if constexpr (A::ACTIVE) a.tick(p...);
        if constexpr (B::ACTIVE) b.tick(p...);
    }
    template <class V>
    __device__ __forceinline__ void fed(const V& v, const unsigned bad_hi, double* yrow)
    {
        if constexpr (A::FEEDS) a.fed(v, bad_hi, yrow);
        if constexpr (B::FEEDS) b.fed(v, bad_hi, yrow);
    }
    __device__ __forceinline__ void finish(const bool valid, const int n_ticks, const long long inst)
    {
        a.finish(valid, n_ticks, inst);
        b.finish(valid, n_ticks, inst);
    }
};

// the hook a lane rollout carries: H itself in a unit without the feedback, H and the feedback with it
template <const ShapeDesc& SD, class H>
using FedHook = std::conditional_t<(kVelFeedbackN > 0), ComposeHook<H, VelocityFeedbackHook<SD>>, H>;

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
