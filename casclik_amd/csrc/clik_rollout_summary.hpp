// Rollouts that summarise their constraint values while they run (clik_*_rollout_batch_sum, include/clik.h): the
// lane-per-instance, image-reading rollouts of clik_pinv_rec.hpp / clik_qp_rec.hpp written out once more, with the fold of
// clik_summary.hpp at the top of every tick.  Record r of the summary is what tick r acts on - the tick's time, the state it
// starts from, the target it reads; with Runge-Kutta the tick's first stage - so the trajectory [n_ticks][B][.] is never
// stored and never read back: [B][M_tot] comes out.
//
// One lane owns one instance and meets its ticks in order, so the reduction rides along in that lane: no chunks, no work
// tensor, no second kernel, and the same bits on every call and in every batch by construction.  The running doubles live
// in the wave's LDS region, one column per lane (slots as SummaryLayout); after the last tick the lane writes its own
// [M_tot] outputs.  What decides the speed at large batches is how many waves a compute unit holds, and that is decided by
// LDS: the PseudoInverseController's kernels therefore run blocks of several waves that share ONE copy of the skill image
// (as constraint_summary_kernel does), read the image from LDS in place in both integration methods, and keep the running
// int32 in the registers that this frees (RollSumAccHybrid) - four waves per compute unit for the headline skill's Euler
// loop, where one wave per block with everything in LDS held two (profiles/rollout_summary.md).  The ReactiveQPController's
// kernels keep one wave per block and all running values in LDS (SummaryAcc<., ., true>): their tick's work area is the
// larger part of the block.
//
// A header and a translation unit of its own (jit.py, _ROLLSUM_TEMPLATE / _QP_ROLLSUM_TEMPLATE; CLIK_ROLLSUM_QP selects the
// QP controller's loop).  The unit includes, ahead of this header, the recording rollouts' header of its controller
// (clik_pinv_rec.hpp / clik_qp_rec.hpp: lane_record / qp_record, RollRec) and clik_summary.hpp (summary_task, SummaryAcc,
// SummaryLayout, SummarySetSlots, SummaryOut) - read-only, nothing of theirs is copied here - and this header includes
// nothing itself: every kernel header stays named by its own units only, and no header that holds another kernel names
// this one.
#pragma once

namespace clik {

// what the summary of a launch reads and writes beside the rollout's own arguments (device pointers; tol and
// o.settled_at may be null together)
struct RollSumArgs {
    const double* tol;          // [MT]
    SummaryOut o;               // [B][MT] each
};

// The lane's running values with the doubles in the wave's LDS region (one column per lane, as SummaryAcc<., ., true>) and
// the int32 in registers: the form of the kernels that read the image from LDS in place and so have the registers, where
// the 256 bytes of LDS per int32 slot decide how many waves a compute unit holds.  summary_task takes any class with these
// four accessors.
template <int ND, int NI>
struct RollSumAccHybrid {
    int32_t i[NI > 0 ? NI : 1];
    double* ld;                 // the lane's element of slot 0; slot k at ld[k * WAVE]
    template <int K>
    __device__ __forceinline__ double getd() const { return ld[K * WAVE]; }
    template <int K>
    __device__ __forceinline__ void setd(const double v) { ld[K * WAVE] = v; }
    template <int K>
    __device__ __forceinline__ int32_t geti() const { return i[K]; }
    template <int K>
    __device__ __forceinline__ void seti(const int32_t v) { i[K] = v; }
};
template <int ND, int NI>
__device__ __forceinline__ void rollsum_bind(SummaryAcc<ND, NI, true>& a, double* vals, const int lane)
{
    a.ld = vals + lane;
    a.li = (int32_t*)(vals + ND * WAVE) + lane;
}
template <int ND, int NI>
__device__ __forceinline__ void rollsum_bind(RollSumAccHybrid<ND, NI>& a, double* vals, const int lane)
{
    a.ld = vals + lane;
}

// LDS a wave of a summarising rollout keeps behind the rollout's own: [tol (MT, even) | running doubles (ND slots) | running
// int32 (NI slots; HYBRID: none, they live in registers)], slot = one value per lane
template <const ShapeDesc& SD, bool HYBRID>
struct RollSumLayout {
    using LY = SummaryLayout<SD>;
    static constexpr int ACC_DOUBLES = LY::ND * WAVE + (HYBRID ? 0 : LY::NI * (WAVE / 2));
    static constexpr int DOUBLES = LY::TOL_DOUBLES + ACC_DOUBLES;
    using Acc = std::conditional_t<HYBRID, RollSumAccHybrid<LY::ND, LY::NI>, SummaryAcc<LY::ND, LY::NI, true>>;
};

// the lane's running values at `base` (the wave's region, see RollSumLayout), initialised; the tolerances copied in
// (visible after the caller's next barrier)
template <const ShapeDesc& SD, class ACC>
__device__ __forceinline__ void rollsum_start(double* base, const double* __restrict__ tol_g, const int lane, ACC& acc,
                                              unsigned (&bad)[SummaryLayout<SD>::BW])
{
    using LY = SummaryLayout<SD>;
    constexpr int MT = LY::MT, MS = LY::MS;
    for (int k = lane; k < MT; k += WAVE) base[k] = tol_g != nullptr ? tol_g[k] : 0.0;
    rollsum_bind(acc, base + LY::TOL_DOUBLES, lane);
    static_for<0, MT>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        acc.template setd<i>(-1.0);                     // (below every |e|: record 0 sets abs_max_at)
        acc.template setd<MT + i>(0.0);
        acc.template seti<i>(0);
        acc.template seti<MT + i>(-1);
    });
    static_for<0, MS>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        acc.template setd<2 * MT + i>(0.0);
        acc.template seti<2 * MT + i>(0);
    });
#pragma unroll
    for (int k = 0; k < LY::BW; ++k) bad[k] = 0u;
}

// record `tick` of the lane's instance: the constraints at (tk, z, ys) as the constraint-summary kernel evaluates them,
// folded task by task.  S: the image in LDS.  last_row: where the lane's `last` values go ([MT], written at the last tick).
template <const ShapeDesc& SD, class ACC>
__device__ __forceinline__ void rollsum_fold(const Img<SD>* __restrict__ S, const TickArgs& tk, const double (&z)[SD.n],
                                             const double* ys, const double* tol, const int lane, const int tick,
                                             ACC& acc,
                                             unsigned (&bad)[SummaryLayout<SD>::BW], const bool last, const bool valid,
                                             double* __restrict__ last_row)
{
    constexpr int N = SD.n;
    Kin<N> K;
    if constexpr (SD.uses_fk != 0) {
        forward_kinematics_s<SD>(S, z, K);
        if constexpr (SD.quat_src != 0) orientation_feature_s<SD>(S, ys, lane, K);
    }
    // (row i of `last` at last_row[i]: the stride between rows that summary_task takes is 1 here)
    summary_task<SD, 0>(S, tk, K, z, ys, tol, lane, tick, acc, bad, last, valid, last_row, 1LL);
    // (the tick's arithmetic stays behind the summary's: one of the two is live at a time)
    __builtin_amdgcn_sched_barrier(0);
}

// after the last tick: the lane's [MT] outputs.  A row that was non-finite at any record: NaN by bits in the float outputs.
template <const ShapeDesc& SD, class ACC>
__device__ __forceinline__ void rollsum_finish(const ACC& acc,
                                               const unsigned (&bad)[SummaryLayout<SD>::BW], const int n_ticks,
                                               const long long inst, const SummaryOut& o)
{
    using LY = SummaryLayout<SD>;
    constexpr int MT = LY::MT;
    constexpr SummarySetSlots<SD> slots{};
    const size_t out0 = (size_t)inst * MT;
    const double rn = (double)n_ticks;
    static_for<0, MT>([&](auto ic) __attribute__((always_inline)) {
        constexpr int row = decltype(ic)::value;
        constexpr int slot = slots.v[row];
        const bool is_bad = ((bad[row / 32] >> (row % 32)) & 1u) != 0u;
        const unsigned bad_hi = is_bad ? 0x7ff80000u : 0u;
        o.abs_max[out0 + row] = nan_or(acc.template getd<row>(), bad_hi);
        o.abs_max_at[out0 + row] = acc.template geti<row>();
        if (is_bad) o.last[out0 + row] = nan_or(0.0, bad_hi);         // (behind the lane's own store of the last tick)
        o.rms[out0 + row] = nan_or(sqrt(acc.template getd<MT + row>() / rn), bad_hi);
        if constexpr (slot >= 0) {
            o.viol_max[out0 + row] = nan_or(acc.template getd<2 * MT + slot>(), bad_hi);
            o.viol_count[out0 + row] = acc.template geti<2 * MT + slot>();
        } else {
            o.viol_max[out0 + row] = nan_or(0.0, bad_hi);
            o.viol_count[out0 + row] = 0;
        }
        if (o.settled_at != nullptr) o.settled_at[out0 + row] = acc.template geti<MT + row>() + 1;
    });
}

#ifndef CLIK_ROLLSUM_QP
// ---- PseudoInverseController ------------------------------------------------------------------------------------------
// A block is WV waves that share ONE copy of the skill image; every wave owns 64 instances and a region of its own.
// LDS: [skill image | wave 0: zs (N slots) ys (n_y slots) (Runge-Kutta: z0s, kss, N slots each) RollSumLayout | wave 1 ...]
template <const ShapeDesc& SD, bool RK>
constexpr int pinv_rollsum_wave_doubles()
{
    constexpr int NY = SD.n_y > 0 ? SD.n_y : 0;
    return (SD.n + NY + (RK ? 2 * SD.n : 0)) * WAVE + RollSumLayout<SD, true>::DOUBLES;
}
template <const ShapeDesc& SD, bool RK>
constexpr size_t pinv_rollsum_lds_bytes(int wv)
{
    return ((size_t)StaticLayout<SD>::IMG_DOUBLES + (size_t)wv * pinv_rollsum_wave_doubles<SD, RK>()) * sizeof(double);
}
// waves per block: what puts most waves on a compute unit (four SIMDs, one wave each: the kernels hold the whole register
// file), the fewest waves per block among equals; 0: not even one wave fits
template <const ShapeDesc& SD, bool RK>
constexpr int pinv_rollsum_waves()
{
    int best = 0, best_cu = 0;
    for (int wv = 1; wv <= 4; ++wv) {
        const size_t bytes = pinv_rollsum_lds_bytes<SD, RK>(wv);
        if (bytes > kSummaryLdsCap) continue;
        int cu = (int)(kSummaryLdsCap / bytes) * wv;
        cu = cu > 4 ? 4 : cu;
        if (cu > best_cu) {
            best_cu = cu;
            best = wv;
        }
    }
    return best;
}

// pinv_rollout_static_body (clik_pinv_rec.hpp) with one RollRec, and the summary of every tick's own state before the
// tick's solve.  The image is read from LDS in place by both integration methods (the running int32 take the registers
// the Euler loop's copy of the image has there).  Every wave of a block walks the same ticks, so all of them meet every
// barrier; a wave past the end of the batch works on the first rows again and stores nothing.
template <const ShapeDesc& SD, bool RK, int WV>
__global__ __launch_bounds__(WV * WAVE) CLIK_ROLL_ATTR void pinv_rollout_static_sum_kernel(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, int32_t* __restrict__ mode_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed,
    double* __restrict__ x, double* __restrict__ dx, const RollRec ra, const RollSumArgs sa)
{
    extern __shared__ double lds[];
    using SL = SummaryLayout<SD>;
    constexpr int N = SD.n;
    constexpr int NX = SD.n_x, NQ = N - NX;
    constexpr int NY = SD.n_y > 0 ? SD.n_y : 0;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
    const long long b_own = ((long long)blockIdx.x * WV + wave) * WAVE;
    const bool idle = b_own >= B;
    const long long b0 = idle ? 0 : b_own;
    const long long left = B - b0;                      // (> 0)
    const int rows_valid = left < WAVE ? (int)left : WAVE;
    const int rows_store = idle ? 0 : rows_valid;
    const bool valid = !idle && lane < rows_valid;
    double* zs = lds + StaticLayout<SD>::IMG_DOUBLES + wave * pinv_rollsum_wave_doubles<SD, RK>();
    double* xs = zs + NQ * WAVE;
    double* ys = zs + N * WAVE;
    double* z0s = ys + NY * WAVE;           // (Runge-Kutta) [N][64] state at the start of the tick, then sum of w_i k_i
    double* kss = z0s + N * WAVE;
    double* sum_base = ys + (NY + (RK ? 2 * N : 0)) * WAVE;
    typedef double d2 __attribute__((ext_vector_type(2)));
    {
        const d2* src = (const d2*)img_g;
        d2* dst = (d2*)lds;
        for (int k = wave; k < StaticLayout<SD>::IMG_CHUNKS; k += WV) dst[k * WAVE + lane] = src[k * WAVE + lane];
        double qv[NQ], xv[NX > 0 ? NX : 1], yv[NY > 0 ? NY : 1];
        stage_load<NQ>(q + b0 * NQ, NQ, rows_valid, lane, qv);
        if constexpr (NX > 0) stage_load<NX>(x + b0 * NX, NX, rows_valid, lane, xv);
        if constexpr (NY > 0) stage_load<NY>(y + b0 * NY, NY, rows_valid, lane, yv);
        rows_to_lds<NQ>(qv, zs, lane);
        if constexpr (NX > 0) rows_to_lds<NX>(xv, xs, lane);
        if constexpr (NY > 0) rows_to_lds<NY>(yv, ys, lane);
    }
    typename RollSumLayout<SD, true>::Acc acc;
    unsigned bad[SL::BW];
    rollsum_start<SD>(sum_base, sa.tol, lane, acc, bad);
    const double* tol = sum_base;
    double* last_row = sa.o.last + (valid ? (size_t)(b0 + lane) * SL::MT : 0);
    __syncthreads();
    const Img<SD>* __restrict__ S = (const Img<SD>*)lds;
    const int nts = S->n_tslots;
    const double* ysl = ys + lane * NY;
    double z[N];
    state_from_lds<NQ, NX>(zs, xs, lane, z);
    double vout[N];
    int acc_mode = -1;
#pragma unroll
    for (int j = 0; j < N; ++j) vout[j] = 0.0;
    RecClock clk;
    [[maybe_unused]] double ynext[NY > 0 ? NY : 1];
    clk.start(ra);
    auto request_rows = [&](const int tick) __attribute__((always_inline)) {
        if constexpr (NY > 0) {
            if (ra.y_stride != 0)
                stage_load<NY>(next_rows(y, ra, tick, n_ticks) + b0 * NY, NY, rows_valid, lane, ynext);
        }
    };
    auto end_of_tick = [&]() __attribute__((always_inline)) {
        if (clk.due(ra)) {
            if (valid) lane_record<NQ, NX>(ra, clk.r * B + b0 + lane, z, vout, acc_mode);
            ++clk.r;
        }
        if constexpr (NY > 0) {
            if (ra.y_stride != 0) {
                rows_to_lds<NY>(ynext, ys, lane);
                __syncthreads();
            }
        }
    };
    if constexpr (!RK) {
#pragma unroll 1
        for (int tick = 0; tick < n_ticks; ++tick) {
            request_rows(tick);
            asm volatile("" ::: "memory");      // (keeps the image reads inside the loop, see pinv_rollout_static_body)
            const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + (size_t)tick * 2 * nts);
            rollsum_fold<SD>(S, tk, z, ysl, tol, lane, tick, acc, bad, tick == n_ticks - 1, valid, last_row);
            pinv_tick_static<SD>(S, tk, z, ysl, lane, valid, vout, acc_mode);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                double d = vout[j];
                if (j < NQ && max_speed > 0.0) d = fmax(fmin(d, max_speed), -max_speed);
                vout[j] = d;
                z[j] = fma(d, dt, z[j]);
            }
            end_of_tick();
        }
    } else {
#pragma unroll 1
        for (int tick = 0; tick < n_ticks; ++tick) {
            request_rows(tick);
            int mode0 = -1;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                z0s[j * WAVE + lane] = z[j];
                kss[j * WAVE + lane] = 0.0;
            }
            {
                // the tick's first stage: its time, the state before the tick
                asm volatile("" ::: "memory");
                const TickArgs& tk0 = *reinterpret_cast<const TickArgs*>(tterms + (size_t)tick * 4 * 2 * nts);
                rollsum_fold<SD>(S, tk0, z, ysl, tol, lane, tick, acc, bad, tick == n_ticks - 1, valid, last_row);
            }
#pragma unroll 1
            for (int st = 0; st < 4; ++st) {
                asm volatile("" ::: "memory");
                const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + ((size_t)tick * 4 + st) * 2 * nts);
                pinv_tick_static<SD>(S, tk, z, ysl, lane, valid, vout, acc_mode);
                const double wgt = (st == 0 || st == 3) ? 1.0 : 2.0;
                const double cnext = (st == 2) ? dt : 0.5 * dt;          // offset of the next stage's state
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double d = vout[j];
                    if (j < NQ && max_speed > 0.0) d = fmax(fmin(d, max_speed), -max_speed);
                    kss[j * WAVE + lane] = fma(wgt, d, kss[j * WAVE + lane]);
                    z[j] = fma(d, cnext, z0s[j * WAVE + lane]);
                }
                mode0 = (st == 0) ? acc_mode : mode0;
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
                vout[j] = kss[j * WAVE + lane] * (1.0 / 6.0);
                z[j] = fma(vout[j], dt, z0s[j * WAVE + lane]);
            }
            acc_mode = mode0;       // (the mode of the first stage)
            end_of_tick();
        }
    }
    if (valid) rollsum_finish<SD>(acc, bad, n_ticks, b0 + lane, sa.o);
    __syncthreads();
    state_to_lds<NQ, NX>(z, zs, xs, lane);
    __syncthreads();
    rows_from_lds<NQ>(q + b0 * NQ, rows_store, zs, lane);
    if constexpr (NX > 0) rows_from_lds<NX>(x + b0 * NX, rows_store, xs, lane);
    __syncthreads();
    state_to_lds<NQ, NX>(vout, zs, xs, lane);
    __syncthreads();
    rows_from_lds<NQ>(dq + b0 * NQ, rows_store, zs, lane);
    if constexpr (NX > 0) rows_from_lds<NX>(dx + b0 * NX, rows_store, xs, lane);
    if (mode_out != nullptr && valid) mode_out[b0 + lane] = acc_mode;
}

template <const ShapeDesc& SD>
constexpr bool rollsum_fits()
{
    return pinv_rollsum_waves<SD, false>() > 0 && pinv_rollsum_waves<SD, true>() > 0;
}
template <const ShapeDesc& SD>
constexpr int rollsum_waves(bool rk)
{
    return rk ? pinv_rollsum_waves<SD, true>() : pinv_rollsum_waves<SD, false>();
}
template <const ShapeDesc& SD>
constexpr size_t rollsum_lds_bytes(bool rk)
{
    // (a shape that does not fit: the figure of one wave, for the refusal)
    constexpr int we = pinv_rollsum_waves<SD, false>(), wr = pinv_rollsum_waves<SD, true>();
    return rk ? pinv_rollsum_lds_bytes<SD, true>(wr > 0 ? wr : 1) : pinv_rollsum_lds_bytes<SD, false>(we > 0 ? we : 1);
}
template <const ShapeDesc& SD, bool RK>
inline const void* rollsum_kernel_ptr()
{
    return (const void*)pinv_rollout_static_sum_kernel<SD, RK, pinv_rollsum_waves<SD, RK>()>;
}

// the lane kernel at every batch size (the team and value-specialised kernels have no summarising form)
template <const ShapeDesc& SD>
inline hipError_t launch_rollout_static_sum(const LaunchArgs& a, const double* d_tterms, int n_ticks, double dt,
                                            double max_speed, long long B, double* q, const double* y, double* dq,
                                            int32_t* mode, hipStream_t stream, const RollSumArgs& sa)
{
    if constexpr (!rollsum_fits<SD>()) {
        return hipErrorInvalidValue;        // (refused at attach time with the figure: jit.attach_rollsum)
    } else {
        if (a.roll_rec == nullptr || n_ticks < 1 || B < 1) return hipErrorInvalidValue;
        if (SD.n_x != 0 && (a.roll_x == nullptr || a.roll_dx == nullptr)) return hipErrorInvalidValue;
        const RollRec rr = *a.roll_rec;
        const bool rk = a.roll_stages == 4;
        const long long per_block = (long long)rollsum_waves<SD>(rk) * WAVE;
        const unsigned grid = (unsigned)((B + per_block - 1) / per_block);
        const size_t shmem = rollsum_lds_bytes<SD>(rk);
        const void* fn = rk ? rollsum_kernel_ptr<SD, true>() : rollsum_kernel_ptr<SD, false>();
        if (shmem > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
            if (e != hipSuccess) return e;
        }
        if (rk) {
            constexpr int WV = pinv_rollsum_waves<SD, true>();
            hipLaunchKernelGGL((pinv_rollout_static_sum_kernel<SD, true, WV>), dim3(grid), dim3(WV * WAVE), shmem, stream,
                               a.dImg, q, y, dq, mode, B, d_tterms, n_ticks, dt, max_speed, a.roll_x, a.roll_dx, rr, sa);
        } else {
            constexpr int WV = pinv_rollsum_waves<SD, false>();
            hipLaunchKernelGGL((pinv_rollout_static_sum_kernel<SD, false, WV>), dim3(grid), dim3(WV * WAVE), shmem, stream,
                               a.dImg, q, y, dq, mode, B, d_tterms, n_ticks, dt, max_speed, a.roll_x, a.roll_dx, rr, sa);
        }
        return hipGetLastError();
    }
}

#else
// ---- ReactiveQPController ---------------------------------------------------------------------------------------------
// LDS: [QP image | the tick's slots (QpLayout) | Runge-Kutta: z0s, kss (N slots each) | RollSumLayout]
template <const ShapeDesc& SD, bool RK>
constexpr size_t qp_rollsum_lds_bytes()
{
    return QpLayout<SD>::LDS_BYTES + ((size_t)(RK ? 2 * SD.n : 0) * WAVE + (size_t)RollSumLayout<SD, false>::DOUBLES) * sizeof(double);
}

// qp_rollout_static_body (clik_qp_rec.hpp) with one RollRec, and the summary of every tick's own state before the tick's
// solve.  An infeasible tick leaves the state where it was: the next record is that same state.
template <const ShapeDesc& SD, bool RK>
__global__ __launch_bounds__(WAVE) void qp_rollout_static_sum_kernel(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, double* __restrict__ slack_out, int32_t* __restrict__ status_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed,
    double* __restrict__ x, double* __restrict__ dx, const RollRec ra, const RollSumArgs sa)
{
    extern __shared__ double lds[];
    using LY = QpLayout<SD>;
    using SL = SummaryLayout<SD>;
    constexpr int N = SD.n;
    constexpr int NX = SD.n_x, NQ = N - NX;
    constexpr int NS = LY::NS;
    constexpr int NY = SD.n_y > 0 ? SD.n_y : 0;
    const int lane = threadIdx.x;
    const long long b0 = (long long)blockIdx.x * WAVE;
    const long long left = B - b0;
    const int rows_valid = left < WAVE ? (int)left : WAVE;
    const bool valid = lane < rows_valid;
    double* slots = lds + LY::IMG_DOUBLES;
    double* zs = slots + LY::O_Z * WAVE;
    double* ys = slots + LY::O_Y * WAVE;
    double* z0s = slots + LY::SLOTS * WAVE;      // (Runge-Kutta) [N][64] state at the start of the tick, then sum of w_i k_i
    double* kss = z0s + N * WAVE;
    double* sum_base = slots + (LY::SLOTS + (RK ? 2 * N : 0)) * WAVE;
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
    typename RollSumLayout<SD, false>::Acc acc;
    unsigned bad[SL::BW];
    rollsum_start<SD>(sum_base, sa.tol, lane, acc, bad);
    const double* tol = sum_base;
    double* last_row = sa.o.last + (valid ? (size_t)(b0 + lane) * SL::MT : 0);
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
    };
    if constexpr (!RK) {
#pragma unroll 1
        for (int tick = 0; tick < n_ticks; ++tick) {
            request_rows(tick);
            asm volatile("" ::: "memory");      // (keeps the image reads inside the loop, see pinv_rollout_static_body)
            const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + (size_t)tick * 2 * nts);
            rollsum_fold<SD>(S, tk, z, ysl, tol, lane, tick, acc, bad, tick == n_ticks - 1, valid, last_row);
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
#pragma unroll 1
        for (int tick = 0; tick < n_ticks; ++tick) {
            request_rows(tick);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                z0s[j * WAVE + lane] = z[j];
                kss[j * WAVE + lane] = 0.0;
            }
            {
                // the tick's first stage: its time, the state before the tick
                asm volatile("" ::: "memory");
                const TickArgs& tk0 = *reinterpret_cast<const TickArgs*>(tterms + (size_t)tick * 4 * 2 * nts);
                rollsum_fold<SD>(S, tk0, z, ysl, tol, lane, tick, acc, bad, tick == n_ticks - 1, valid, last_row);
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
    if (valid) rollsum_finish<SD>(acc, bad, n_ticks, b0 + lane, sa.o);
    const unsigned nan_hi = (worst == 2) ? 0x7ff80000u : 0u;      // (nan_or: the NaN of an infeasible instance, as bits)
    __syncthreads();
    state_to_lds<NQ, NX>(z, zs, xs, lane);
    __syncthreads();
    rows_from_lds<NQ>(q + b0 * NQ, rows_valid, zs, lane);
    if constexpr (NX > 0) rows_from_lds<NX>(x + b0 * NX, rows_valid, xs, lane);
    __syncthreads();
    {
        double vb[N];
#pragma unroll
        for (int j = 0; j < N; ++j) vb[j] = nan_or(v[j], nan_hi);
        state_to_lds<NQ, NX>(vb, zs, xs, lane);
    }
    if constexpr (NS > 0) {
        double* so = slots + LY::O_SL * WAVE;
        if (slack_out != nullptr) {
#pragma unroll
            for (int k = 0; k < NS; ++k) so[lane * NS + k] = nan_or(sl[k], nan_hi);
        }
    }
    __syncthreads();
    rows_from_lds<NQ>(dq + b0 * NQ, rows_valid, zs, lane);
    if constexpr (NX > 0) rows_from_lds<NX>(dx + b0 * NX, rows_valid, xs, lane);
    if constexpr (NS > 0) {
        if (slack_out != nullptr) rows_from_lds<NS>(slack_out + b0 * NS, rows_valid, slots + LY::O_SL * WAVE, lane);
    }
    if (status_out != nullptr && valid) status_out[b0 + lane] = worst;
}

template <const ShapeDesc& SD>
constexpr bool rollsum_fits()
{
    return qp_rollsum_lds_bytes<SD, true>() <= kSummaryLdsCap;
}
template <const ShapeDesc& SD>
constexpr size_t rollsum_lds_bytes(bool rk)
{
    return rk ? qp_rollsum_lds_bytes<SD, true>() : qp_rollsum_lds_bytes<SD, false>();
}
template <const ShapeDesc& SD>
constexpr int rollsum_waves(bool) { return 1; }
template <const ShapeDesc& SD, bool RK>
inline const void* rollsum_kernel_ptr()
{
    return (const void*)qp_rollout_static_sum_kernel<SD, RK>;
}

template <const ShapeDesc& SD>
inline hipError_t launch_qp_rollout_static_sum(const void* d_img, const double* d_tterms, int n_ticks, double dt,
                                               double max_speed, long long B, double* q, const double* y, double* dq,
                                               double* slack, int32_t* status, double* x, double* dx,
                                               hipStream_t stream, int stages, const RollRec* rec, const RollSumArgs& sa)
{
    if constexpr (!rollsum_fits<SD>()) {
        return hipErrorInvalidValue;        // (refused at attach time with the figure: jit.attach_qp_rollsum)
    } else {
        if (rec == nullptr || n_ticks < 1 || B < 1) return hipErrorInvalidValue;
        if (SD.n_x != 0 && (x == nullptr || dx == nullptr)) return hipErrorInvalidValue;
        const RollRec rr = *rec;
        const unsigned grid = (unsigned)((B + WAVE - 1) / WAVE);
        const bool rk = stages == 4;
        const size_t shmem = rollsum_lds_bytes<SD>(rk);
        const void* fn = rk ? rollsum_kernel_ptr<SD, true>() : rollsum_kernel_ptr<SD, false>();
        if (shmem > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
            if (e != hipSuccess) return e;
        }
        if (rk)
            hipLaunchKernelGGL((qp_rollout_static_sum_kernel<SD, true>), dim3(grid), dim3(WAVE), shmem, stream, d_img, q, y,
                               dq, slack, status, B, d_tterms, n_ticks, dt, max_speed, x, dx, rr, sa);
        else
            hipLaunchKernelGGL((qp_rollout_static_sum_kernel<SD, false>), dim3(grid), dim3(WAVE), shmem, stream, d_img, q, y,
                               dq, slack, status, B, d_tterms, n_ticks, dt, max_speed, x, dx, rr, sa);
        return hipGetLastError();
    }
}
#endif

// what a caller may ask about the instantiation (clik_jit_rollsum_info): 0 rows, 1 SetConstraint rows, 2 LDS bytes of a
// Runge-Kutta block, 3 fits the LDS of a CU, 4 LDS bytes of an Euler block, 5 / 6 bytes of scratch per lane of the Euler /
// Runge-Kutta kernel as the loaded code object states them (-1: no device to ask), 7 / 8 waves of an Euler / Runge-Kutta
// block
template <const ShapeDesc& SD>
inline long long rollsum_info(int what)
{
    using LY = SummaryLayout<SD>;
    if (what == 5 || what == 6) {
        if constexpr (!rollsum_fits<SD>()) {
            return -1;
        } else {
            hipFuncAttributes fa;
            const void* fn = what == 6 ? rollsum_kernel_ptr<SD, true>() : rollsum_kernel_ptr<SD, false>();
            if (hipFuncGetAttributes(&fa, fn) != hipSuccess) {
                (void)hipGetLastError();
                return -1;
            }
            return (long long)fa.localSizeBytes;
        }
    }
    return what == 0 ? LY::MT : what == 1 ? LY::MS : what == 2 ? (long long)rollsum_lds_bytes<SD>(true)
         : what == 3 ? (rollsum_fits<SD>() ? 1 : 0) : what == 4 ? (long long)rollsum_lds_bytes<SD>(false)
         : what == 7 ? rollsum_waves<SD>(false) : what == 8 ? rollsum_waves<SD>(true) : -1;
}

}  // namespace clik
