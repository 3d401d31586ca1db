// Rollouts that record their trajectory and read one target per tick (clik_qp_rollout_batch_rec, include/clik.h; RollRec in
// clik_device.hpp): the loops of clik_qp_static.hpp again, with one RollRec - records and per-tick targets - and their
// launchers.  A header of its own, included by the on-demand translation units only (casclik_amd/jit.py): the compiler's code
// for a kernel depends on what else its translation unit declares - with these templates declared next to them, the rollouts
// that record nothing fused their multiply-adds in another order, and their results are pinned to the tick kernels' (the
// smoke test: q after one tick to 1e-12).
// The lane-per-instance loop (qp_rollout_static_body) is the one text of the recording rollout and, with a hook that folds
// every tick's state (clik_rollout_lane.hpp: NoTickHook), of the rollout that summarises its constraint values.
#pragma once
#include "clik_qp_static.hpp"
#include "clik_rollout_lane.hpp"
namespace clik {

// One record of a QP rollout (RollRec): what a launch ending at this tick returns - the state, the clamped velocity and
// the slack with the NaN of an infeasible instance, the worst status so far.  The lane stores its own rows with plain
// stores, nothing waits for them.
template <int NQ, int NX, int NS, int NSA>
__device__ __forceinline__ void qp_record(const RollRec& ra, const long long row, const double (&z)[NQ + NX],
                                          const double (&v)[NQ + NX], const double (&sl)[NSA], const int worst)
{
    const unsigned bad = (worst == 2) ? 0x7ff80000u : 0u;
    if (ra.q != nullptr) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) ra.q[row * NQ + j] = z[j];
    }
    if (ra.dq != nullptr) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) ra.dq[row * NQ + j] = nan_or(v[j], bad);
    }
    if constexpr (NX > 0) {
        if (ra.x != nullptr) {
#pragma unroll
            for (int j = 0; j < NX; ++j) ra.x[row * NX + j] = z[NQ + j];
        }
        if (ra.dx != nullptr) {
#pragma unroll
            for (int j = 0; j < NX; ++j) ra.dx[row * NX + j] = nan_or(v[NQ + j], bad);
        }
    }
    if constexpr (NS > 0) {
        if (ra.slack != nullptr) {
#pragma unroll
            for (int k = 0; k < NS; ++k) ra.slack[row * NS + k] = nan_or(sl[k], bad);
        }
    }
    if (ra.flag != nullptr) ra.flag[row] = worst;
}

// ... and its on-device rollout (see qp_rollout_static_kernel): state, working set and Runge-Kutta bookkeeping in
// registers from tick to tick, rows loaded once and stored once by the lane itself
// ra: records of the trajectory and one target row per tick (RollRec, clik_device.hpp).
// (a body and a kernel that calls it, here and below, not one function: the compiler's code for the loop differs between
// the two forms, and these kernels' code is held to what it was)
template <const ShapeDesc& SD, class IMGV, bool RK>
__device__ __forceinline__ void qp_rollout_static_box_values_body(
    double* __restrict__ q, const double* __restrict__ y, double* __restrict__ dq, double* __restrict__ slack_out,
    int32_t* __restrict__ status_out, const long long B, const double* __restrict__ tterms, const int n_ticks,
    const double dt, const double max_speed, double* __restrict__ x, double* __restrict__ dx, const RollRec ra)
{
    using LY = QpLayout<SD>;
    static_assert(LY::BOX, "box family only");
    constexpr int N = SD.n, NX = SD.n_x, NQ = N - NX, NS = LY::NS;
    constexpr QpImg<SD> kValues = IMGV::value;
    constexpr int stages = RK ? 4 : 1;
    const int lane = threadIdx.x;
    const long long inst = (long long)blockIdx.x * WAVE + lane;
    const bool valid = inst < B;
    const long long row = valid ? inst : B - 1;
    const int nts = kValues.img.n_tslots;
    double z[N];
#pragma unroll
    for (int j = 0; j < NQ; ++j) z[j] = q[row * NQ + j];
    if constexpr (NX > 0) {
#pragma unroll
        for (int j = 0; j < NX; ++j) z[NQ + j] = x[row * NX + j];
    }
    const double* ysl = SD.n_y > 0 ? y + row * SD.n_y : nullptr;
    double v[N], sl[LY::NSA];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = 0.0;
#pragma unroll
    for (int k = 0; k < LY::NSA; ++k) sl[k] = 0.0;
    int32_t hot = 0;
    int worst = 0;
    // per-tick target (RollRec): the row lives in registers, and the NEXT tick's is requested at the top of a tick
    RecClock clk;
    [[maybe_unused]] double ycur[SD.n_y > 0 ? SD.n_y : 1], ynext[SD.n_y > 0 ? SD.n_y : 1];
    clk.start(ra);
    if constexpr (SD.n_y > 0) {
#pragma unroll
        for (int k = 0; k < SD.n_y; ++k) ycur[k] = ynext[k] = ysl[k];
        ysl = ycur;
    }
#pragma unroll 1
    for (int tick = 0; tick < n_ticks; ++tick) {
        if constexpr (SD.n_y > 0) {
            if (ra.y_stride != 0) {
                const double* yn = next_rows(y, ra, tick, n_ticks) + row * SD.n_y;
#pragma unroll
                for (int k = 0; k < SD.n_y; ++k) ynext[k] = yn[k];
            }
        }
        double z0[N], ks[N];
        bool okl = true;
        if constexpr (RK) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                z0[j] = z[j];
                ks[j] = 0.0;
            }
        }
#pragma unroll 1
        for (int stg = 0; stg < stages; ++stg) {
            const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + ((size_t)tick * stages + stg) * 2 * nts);
            double priv[LY::SLOTS];
            // (one copy of the tick with a run-time `use_hot`: two copies with the flag a literal in each - as the launched and the
            // resident kernels have - measured 85 instructions MORE per tick here, 3.78 against 3.72 us, round 6: the register
            // allocator's doing)
            const int st = qp_tick_static<SD, 1>(&kValues.img, &kValues.tail, tk, z, ysl, lane, valid, priv, v, sl, &hot,
                                                 (tick | stg) > 0);
            worst = st > worst ? st : worst;
            okl = okl & (st != 2);              // an infeasible tick (stage) leaves the state where it was
            if constexpr (!RK) {
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double d = v[j];
                    if (j < NQ && max_speed > 0.0) d = fmax(fmin(d, max_speed), -max_speed);
                    v[j] = d;
                    z[j] = okl ? fma(d, dt, z[j]) : z[j];
                }
            } else {
                const double wgt = (stg == 0 || stg == 3) ? 1.0 : 2.0;
                const double cnext = (stg == 2) ? dt : 0.5 * dt;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double d = okl ? v[j] : 0.0;
                    if (j < NQ && max_speed > 0.0) d = fmax(fmin(d, max_speed), -max_speed);
                    ks[j] = fma(wgt, d, ks[j]);
                    z[j] = fma(d, cnext, z0[j]);
                }
            }
        }
        if constexpr (RK) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double d = ks[j] * (1.0 / 6.0);
                v[j] = okl ? d : v[j];
                z[j] = okl ? fma(d, dt, z0[j]) : z0[j];
            }
        }
        if (clk.due(ra)) {
            if (valid) qp_record<NQ, NX, NS, LY::NSA>(ra, clk.r * B + inst, z, v, sl, worst);
            ++clk.r;
        }
        if constexpr (SD.n_y > 0) {
#pragma unroll
            for (int k = 0; k < SD.n_y; ++k) ycur[k] = ynext[k];
        }
    }
    if (valid) {
        const unsigned bad = (worst == 2) ? 0x7ff80000u : 0u;      // (nan_or: the NaN of an infeasible instance, as bits)
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            q[inst * NQ + j] = z[j];
            dq[inst * NQ + j] = nan_or(v[j], bad);
        }
        if constexpr (NX > 0) {
#pragma unroll
            for (int j = 0; j < NX; ++j) {
                x[inst * NX + j] = z[NQ + j];
                dx[inst * NX + j] = nan_or(v[NQ + j], bad);
            }
        }
        if constexpr (NS > 0) {
            if (slack_out != nullptr) {
#pragma unroll
                for (int k = 0; k < NS; ++k) slack_out[inst * NS + k] = nan_or(sl[k], bad);
            }
        }
        if (status_out != nullptr) status_out[inst] = worst;
    }
}

// ... recording its trajectory / reading one target per tick (RollRec, clik_device.hpp)
template <const ShapeDesc& SD, class IMGV, bool RK>
__global__ __launch_bounds__(WAVE) void qp_rollout_static_box_values_rec_kernel(
    double* __restrict__ q, const double* __restrict__ y, double* __restrict__ dq, double* __restrict__ slack_out,
    int32_t* __restrict__ status_out, const long long B, const double* __restrict__ tterms, const int n_ticks,
    const double dt, const double max_speed, double* __restrict__ x, double* __restrict__ dx, const RollRec rec)
{
    qp_rollout_static_box_values_body<SD, IMGV, RK>(q, y, dq, slack_out, status_out, B, tterms, n_ticks, dt, max_speed, x, dx, rec);
}

// n_ticks of (QP tick -> clamp(+-max_speed) -> explicit Euler q += dq dt) in one launch: the host
// loop of the notebooks (ur5_moe2016_example2.ipynb:537-545) for the QP controller.  The working
// set stays in a register from tick to tick (hot start), the skill image and the targets in LDS.
// q is updated in place; dq / slack receive the last tick, status the worst status met.
// RK: classical Runge-Kutta with the controller as the right-hand side (integration_methods.py:17-23; four QP
// solves per tick, the working set hot-started from stage to stage, tterms holds four records per tick) instead of
// explicit Euler; a tick with an infeasible stage leaves the state where it was.
// ra: records of the trajectory and one target row per tick (RollRec, clik_device.hpp).
// LDS: [QP image | the tick's slots (QpLayout) | Runge-Kutta: z0s, kss (N slots each) | the hook's doubles]
// hook: see NoTickHook (clik_rollout_lane.hpp).
template <const ShapeDesc& SD, bool RK, class HOOK>
__device__ __forceinline__ void qp_rollout_static_body(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, double* __restrict__ slack_out, int32_t* __restrict__ status_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed,
    double* __restrict__ x, double* __restrict__ dx, const RollRec ra, HOOK& hook)
{
    // x / dx: virtual variables, integrated like the robot variables and never clamped (null without them)
    extern __shared__ double lds[];
    using LY = QpLayout<SD>;
    constexpr int N = SD.n;
    constexpr int NX = SD.n_x, NQ = N - NX;
    constexpr int NS = LY::NS;
    constexpr int NY = SD.n_y > 0 ? SD.n_y : 0;
    const WavePlace<1> w(B);
    const int lane = w.lane;
    const long long b0 = w.b0;
    const int rows_valid = w.rows_valid;
    const bool valid = w.valid;
    double* slots = lds + LY::IMG_DOUBLES;
    double* zs = slots + LY::O_Z * WAVE;
    double* ys = slots + LY::O_Y * WAVE;
    typedef double d2 __attribute__((ext_vector_type(2)));
    {
        d2 img[LY::IMG_CHUNKS];
        const d2* src = (const d2*)img_g;
#pragma unroll
        for (int k = 0; k < LY::IMG_CHUNKS; ++k) img[k] = src[k * WAVE + lane];
        double qv[NQ], xv[NX > 0 ? NX : 1], yv[NY > 0 ? NY : 1];
        stage_load<NQ>(q + b0 * NQ, NQ, rows_valid, lane, qv);
        if constexpr (NX > 0) stage_load<NX>(x + b0 * NX, NX, rows_valid, lane, xv);
        if constexpr (NY > 0) stage_load<NY>(y + b0 * NY, NY, rows_valid, lane, yv);
        d2* dst = (d2*)lds;
#pragma unroll
        for (int k = 0; k < LY::IMG_CHUNKS; ++k) dst[k * WAVE + lane] = img[k];
        rows_to_lds<NQ>(qv, zs, lane);
        if constexpr (NX > 0) rows_to_lds<NX>(xv, zs + NQ * WAVE, lane);
        if constexpr (NY > 0) rows_to_lds<NY>(yv, ys, lane);
    }
    hook.start(slots + (LY::SLOTS + (RK ? 2 * N : 0)) * WAVE, lane, valid, b0 + lane);
    __syncthreads();
    const Img<SD>* __restrict__ S = (const Img<SD>*)lds;
    const QpTail* __restrict__ T = (const QpTail*)((const char*)lds + LY::TAIL_OFF);
    const int nts = S->n_tslots;
    const double* ysl = ys + lane * NY;
    double* xs = zs + NQ * WAVE;
    double z[N];
    state_from_lds<NQ, NX>(zs, xs, lane, z);
    double v[N], sl[LY::NSA];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = 0.0;
#pragma unroll
    for (int k = 0; k < LY::NSA; ++k) sl[k] = 0.0;
    int32_t hot = 0;
    int worst = 0;
    RecClock clk;
    [[maybe_unused]] double ynext[NY > 0 ? NY : 1];
    clk.start(ra);
    // per-tick target: the NEXT tick's block is requested at the top of a tick (coalesced, as the first one was) and
    // replaces this tick's in LDS at its end, where the tick's record is stored too (see pinv_rollout_static_kernel)
    auto request_rows = [&](const int tick) __attribute__((always_inline)) {
        if constexpr (NY > 0) {
            if (ra.y_stride != 0)
                stage_load<NY>(next_rows(y, ra, tick, n_ticks) + b0 * NY, NY, rows_valid, lane, ynext);
        }
    };
    auto end_of_tick = [&]() __attribute__((always_inline)) {
        if (clk.due(ra)) {
            if (valid) qp_record<NQ, NX, NS, LY::NSA>(ra, clk.r * B + b0 + lane, z, v, sl, worst);
            ++clk.r;
        }
        if constexpr (NY > 0) {
            if (ra.y_stride != 0) {
                rows_to_lds<NY>(ynext, ys, lane);
                __syncthreads();
            }
        }
        // (velocity feedback: behind the record and the reload, and what the record holds - NaN once infeasible)
        if constexpr (HOOK::FEEDS) hook.fed(v, (worst == 2) ? 0x7ff80000u : 0u, ys + lane * NY);
    };
    if constexpr (!RK) {
#pragma unroll 1
        for (int tick = 0; tick < n_ticks; ++tick) {
            request_rows(tick);
            asm volatile("" ::: "memory");      // (keeps the image reads inside the loop, see pinv_rollout_static_kernel)
            const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + (size_t)tick * 2 * nts);
            hook.tick(S, tk, z, ysl, lane, tick, n_ticks, valid);
            const int st = qp_tick_static<SD>(S, T, tk, z, ysl, lane, valid, slots, v, sl, &hot, tick > 0);
            worst = st > worst ? st : worst;
            const bool okl = st != 2;           // an infeasible tick leaves the state where it is
#pragma unroll
            for (int j = 0; j < N; ++j) {
                double d = v[j];
                if (j < NQ && max_speed > 0.0) d = fmax(fmin(d, max_speed), -max_speed);
                v[j] = d;
                z[j] = okl ? fma(d, dt, z[j]) : z[j];
            }
            end_of_tick();
        }
    } else {
        double* z0s = slots + LY::SLOTS * WAVE;      // [N][64] state at the start of the tick, [N][64] sum of w_i k_i
        double* kss = z0s + N * WAVE;
#pragma unroll 1
        for (int tick = 0; tick < n_ticks; ++tick) {
            request_rows(tick);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                z0s[j * WAVE + lane] = z[j];
                kss[j * WAVE + lane] = 0.0;
            }
            if constexpr (HOOK::ACTIVE) {
                // the tick's first stage: its time, the state before the tick
                asm volatile("" ::: "memory");
                const TickArgs& tk0 = *reinterpret_cast<const TickArgs*>(tterms + (size_t)tick * 4 * 2 * nts);
                hook.tick(S, tk0, z, ysl, lane, tick, n_ticks, valid);
            }
            bool okl = true;
#pragma unroll 1
            for (int stg = 0; stg < 4; ++stg) {
                asm volatile("" ::: "memory");
                const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + ((size_t)tick * 4 + stg) * 2 * nts);
                const int st = qp_tick_static<SD>(S, T, tk, z, ysl, lane, valid, slots, v, sl, &hot, (tick | stg) > 0);
                worst = st > worst ? st : worst;
                okl = okl & (st != 2);
                const double wgt = (stg == 0 || stg == 3) ? 1.0 : 2.0;
                const double cnext = (stg == 2) ? dt : 0.5 * dt;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double d = okl ? v[j] : 0.0;
                    if (j < NQ && max_speed > 0.0) d = fmax(fmin(d, max_speed), -max_speed);
                    kss[j * WAVE + lane] = fma(wgt, d, kss[j * WAVE + lane]);
                    z[j] = fma(d, cnext, z0s[j * WAVE + lane]);
                }
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const double d = kss[j * WAVE + lane] * (1.0 / 6.0);
                v[j] = okl ? d : v[j];
                z[j] = okl ? fma(d, dt, z0s[j * WAVE + lane]) : z0s[j * WAVE + lane];
            }
            end_of_tick();
        }
    }
    hook.finish(valid, n_ticks, b0 + lane);
    const unsigned bad = (worst == 2) ? 0x7ff80000u : 0u;      // (nan_or: the NaN of an infeasible instance, as bits)
    rows_out<NQ, NX>(z, q, x, w, zs, xs);
    double vb[N];
#pragma unroll
    for (int j = 0; j < N; ++j) vb[j] = nan_or(v[j], bad);
    rows_out<NQ, NX>(vb, dq, dx, w, zs, xs, [&]() __attribute__((always_inline)) {
        if constexpr (NS > 0) {
            double* so = slots + LY::O_SL * WAVE;
            if (slack_out != nullptr) {
#pragma unroll
                for (int k = 0; k < NS; ++k) so[lane * NS + k] = nan_or(sl[k], bad);
            }
        }
    });
    if constexpr (NS > 0) {
        if (slack_out != nullptr) rows_from_lds<NS>(slack_out + b0 * NS, rows_valid, slots + LY::O_SL * WAVE, lane);
    }
    if (status_out != nullptr && valid) status_out[b0 + lane] = worst;
}

// ... recording its trajectory / reading one target per tick (RollRec, clik_device.hpp)
template <const ShapeDesc& SD, bool RK>
__global__ __launch_bounds__(WAVE) void qp_rollout_static_rec_kernel(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, double* __restrict__ slack_out, int32_t* __restrict__ status_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed,
    double* __restrict__ x, double* __restrict__ dx, const RollRec rec)
{
    FedHook<SD, NoTickHook> none;
    qp_rollout_static_body<SD, RK>(img_g, q, y, dq, slack_out, status_out, B, tterms, n_ticks, dt, max_speed, x, dx, rec, none);
}

// The recording / per-tick-target instantiations of the two rollouts (clik_qp_rollout_batch_rec): in translation units
// of their own (casclik_amd/jit.py: clik_jit_qp_rollout_rec / clik_jit_qp_value_rollout_rec)
template <const ShapeDesc& SD>
inline hipError_t launch_qp_rollout_static_rec(const void* d_img, const double* d_tterms, int n_ticks, double dt,
                                               double max_speed, long long B, double* q, const double* y, double* dq,
                                               double* slack, int32_t* status, double* x, double* dx,
                                               hipStream_t stream, int stages, const RollRec* rec)
{
    if (rec == nullptr || (SD.n_x != 0 && (x == nullptr || dx == nullptr))) return hipErrorInvalidValue;
    const RollRec rr = *rec;
    const unsigned grid = (unsigned)((B + WAVE - 1) / WAVE);
    if (stages == 4) {
        constexpr size_t shmem = QpLayout<SD>::LDS_BYTES + (size_t)2 * SD.n * WAVE * sizeof(double);
        static_assert(shmem <= kLdsBytesPerCu, "Runge-Kutta QP rollout needs more LDS than a CU has");
        if (shmem > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)qp_rollout_static_rec_kernel<SD, true>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((qp_rollout_static_rec_kernel<SD, true>), dim3(grid), dim3(WAVE), shmem, stream, d_img, q, y,
                           dq, slack, status, B, d_tterms, n_ticks, dt, max_speed, x, dx, rr);
        return hipGetLastError();
    }
    constexpr size_t shmem = QpLayout<SD>::LDS_BYTES;
    if (shmem > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)qp_rollout_static_rec_kernel<SD, false>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((qp_rollout_static_rec_kernel<SD, false>), dim3(grid), dim3(WAVE), shmem, stream, d_img, q, y, dq,
                       slack, status, B, d_tterms, n_ticks, dt, max_speed, x, dx, rr);
    return hipGetLastError();
}

// hipErrorNotSupported outside the box family (the caller then uses the image-reading recording rollout)
template <const ShapeDesc& SD, class IMGV>
inline hipError_t launch_qp_rollout_static_values_rec(const double* d_tterms, int n_ticks, double dt, double max_speed,
                                                      long long B, double* q, const double* y, double* dq, double* slack,
                                                      int32_t* status, double* x, double* dx, hipStream_t stream,
                                                      int stages, const RollRec* rec)
{
    if constexpr (QpLayout<SD>::BOX && kVelFeedbackN == 0) {       // (the lane kernels alone carry the velocity feedback)
        if (rec == nullptr || (SD.n_x != 0 && (x == nullptr || dx == nullptr))) return hipErrorInvalidValue;
        const RollRec rr = *rec;
        const unsigned grid = (unsigned)((B + WAVE - 1) / WAVE);
        if (stages == 4)
            hipLaunchKernelGGL((qp_rollout_static_box_values_rec_kernel<SD, IMGV, true>), dim3(grid), dim3(WAVE), 0,
                               stream, q, y, dq, slack, status, B, d_tterms, n_ticks, dt, max_speed, x, dx, rr);
        else
            hipLaunchKernelGGL((qp_rollout_static_box_values_rec_kernel<SD, IMGV, false>), dim3(grid), dim3(WAVE), 0,
                               stream, q, y, dq, slack, status, B, d_tterms, n_ticks, dt, max_speed, x, dx, rr);
        return hipGetLastError();
    } else {
        return hipErrorNotSupported;
    }
}

// what a caller may ask about the lane kernels of a recording unit (clik_jit_rec_info, in the units built with the
// velocity feedback): 0 / 1 bytes of scratch per lane of the Euler / Runge-Kutta kernel as the loaded code object states
// them (-1: no device to ask), 2 / 3 LDS bytes of an Euler / Runge-Kutta block, 4 both fit the LDS of a CU, 5 + k the
// compiled-in feedback map (velocity_feedback_info(k))
template <const ShapeDesc& SD>
inline long long rollout_rec_info(int what)
{
    constexpr size_t euler = QpLayout<SD>::LDS_BYTES, rk = euler + (size_t)2 * SD.n * WAVE * sizeof(double);
    if (what == 0) return kernel_scratch_bytes((const void*)qp_rollout_static_rec_kernel<SD, false>);
    if (what == 1) return kernel_scratch_bytes((const void*)qp_rollout_static_rec_kernel<SD, true>);
    return what == 2 ? (long long)euler : what == 3 ? (long long)rk : what == 4 ? (rk <= kLaneLdsCap ? 1 : 0)
         : what >= 5 ? velocity_feedback_info(what - 5) : -1;
}

}  // namespace clik
