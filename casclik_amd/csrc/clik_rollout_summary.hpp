// Rollouts that summarise their constraint values while they run (clik_*_rollout_batch_sum, include/clik.h): the
// lane-per-instance, image-reading rollouts of clik_pinv_rec.hpp / clik_qp_rec.hpp - their loops, not copies of them - with
// the fold of clik_summary.hpp hooked in at the top of every tick (RollSumHook).  Record r of the summary is what tick r acts on - the tick's time, the state it
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

// The summary as the hook of a lane-per-instance rollout (NoTickHook, clik_rollout_lane.hpp): the lane's running values,
// started before the rollout's first barrier, folded at the top of every tick, written out after the loop.
template <const ShapeDesc& SD, bool HYBRID>
struct RollSumHook {
    using SL = SummaryLayout<SD>;
    static constexpr bool ACTIVE = true;
    static constexpr bool FEEDS = false;
    static constexpr int LDS_DOUBLES = RollSumLayout<SD, HYBRID>::DOUBLES;
    const RollSumArgs& sa;
    typename RollSumLayout<SD, HYBRID>::Acc acc;
    unsigned bad[SL::BW];
    const double* tol;          // [MT] in LDS
    double* last_row;           // where the lane's `last` values go
    __device__ __forceinline__ void start(double* base, const int lane, const bool valid, const long long inst)
    {
        rollsum_start<SD>(base, sa.tol, lane, acc, bad);
        tol = base;
        last_row = sa.o.last + (valid ? (size_t)inst * SL::MT : 0);
    }
    __device__ __forceinline__ void tick(const Img<SD>* __restrict__ S, const TickArgs& tk, const double (&z)[SD.n],
                                         const double* ys, const int lane, const int tick, const int n_ticks,
                                         const bool valid)
    {
        rollsum_fold<SD>(S, tk, z, ys, tol, lane, tick, acc, bad, tick == n_ticks - 1, valid, last_row);
    }
    __device__ __forceinline__ void finish(const bool valid, const int n_ticks, const long long inst)
    {
        if (valid) rollsum_finish<SD>(acc, bad, n_ticks, inst, sa.o);
    }
};

#ifndef CLIK_ROLLSUM_QP
// ---- PseudoInverseController ------------------------------------------------------------------------------------------
// A block is WV waves that share ONE copy of the skill image; every wave owns 64 instances and a region of its own.
// LDS: [skill image | wave 0: zs (N slots) ys (n_y slots) (Runge-Kutta: z0s, kss, N slots each) RollSumLayout | wave 1 ...]
template <const ShapeDesc& SD, bool RK>
constexpr size_t pinv_rollsum_lds_bytes(int wv)
{
    return ((size_t)StaticLayout<SD>::IMG_DOUBLES
            + (size_t)wv * lane_wave_doubles<SD, RK>(RollSumLayout<SD, true>::DOUBLES)) * sizeof(double);
}
template <const ShapeDesc& SD, bool RK>
constexpr int pinv_rollsum_waves()
{
    return waves_per_block<pinv_rollsum_lds_bytes<SD, RK>>(kSummaryLdsCap);
}

// pinv_rollout_static_body (clik_pinv_rec.hpp) with the summary of every tick's own state before the tick's solve.  The
// image is read from LDS in place by both integration methods (the running int32 take the registers the Euler loop's copy
// of the image has in the recording rollout).
template <const ShapeDesc& SD, bool RK, int WV>
__global__ __launch_bounds__(WV * WAVE) CLIK_ROLL_ATTR void pinv_rollout_static_sum_kernel(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, int32_t* __restrict__ mode_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed,
    double* __restrict__ x, double* __restrict__ dx, const RollRec ra, const RollSumArgs sa)
{
    FedHook<SD, RollSumHook<SD, true>> hook{sa};
    pinv_rollout_static_body<SD, RK, WV, false>(img_g, q, y, dq, mode_out, B, tterms, n_ticks, dt, max_speed, x, dx, ra, hook);
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
        const unsigned wv = (unsigned)rollsum_waves<SD>(rk);
        const unsigned grid = (unsigned)((B + wv * WAVE - 1) / (wv * WAVE));
        return launch_with_lds(rk ? pinv_rollout_static_sum_kernel<SD, true, pinv_rollsum_waves<SD, true>()>
                                  : pinv_rollout_static_sum_kernel<SD, false, pinv_rollsum_waves<SD, false>()>,
                               grid, wv * WAVE, rollsum_lds_bytes<SD>(rk), stream, a.dImg, q, y, dq, mode, B, d_tterms,
                               n_ticks, dt, max_speed, a.roll_x, a.roll_dx, rr, sa);
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

// qp_rollout_static_body (clik_qp_rec.hpp) with the summary of every tick's own state before the tick's solve.  An
// infeasible tick leaves the state where it was: the next record is that same state.
template <const ShapeDesc& SD, bool RK>
__global__ __launch_bounds__(WAVE) void qp_rollout_static_sum_kernel(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, double* __restrict__ slack_out, int32_t* __restrict__ status_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed,
    double* __restrict__ x, double* __restrict__ dx, const RollRec ra, const RollSumArgs sa)
{
    FedHook<SD, RollSumHook<SD, false>> hook{sa};
    qp_rollout_static_body<SD, RK>(img_g, q, y, dq, slack_out, status_out, B, tterms, n_ticks, dt, max_speed, x, dx, ra, hook);
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
        return launch_with_lds(rk ? qp_rollout_static_sum_kernel<SD, true> : qp_rollout_static_sum_kernel<SD, false>, grid,
                               WAVE, rollsum_lds_bytes<SD>(rk), stream, d_img, q, y, dq, slack, status, B, d_tterms, n_ticks,
                               dt, max_speed, x, dx, rr, sa);
    }
}
#endif

// what a caller may ask about the instantiation (clik_jit_rollsum_info): 0 rows, 1 SetConstraint rows, 2 LDS bytes of a
// Runge-Kutta block, 3 fits the LDS of a CU, 4 LDS bytes of an Euler block, 5 / 6 bytes of scratch per lane of the Euler /
// Runge-Kutta kernel as the loaded code object states them (-1: no device to ask), 7 / 8 waves of an Euler / Runge-Kutta
// block, 9 + k the compiled-in velocity feedback map (velocity_feedback_info(k), clik_rollout_lane.hpp)
template <const ShapeDesc& SD>
inline long long rollsum_info(int what)
{
    using LY = SummaryLayout<SD>;
    if (what >= 9) return velocity_feedback_info(what - 9);
    if (what == 5 || what == 6) {
        if constexpr (!rollsum_fits<SD>()) {
            return -1;
        } else {
            return kernel_scratch_bytes(what == 6 ? rollsum_kernel_ptr<SD, true>() : rollsum_kernel_ptr<SD, false>());
        }
    }
    return what == 0 ? LY::MT : what == 1 ? LY::MS : what == 2 ? (long long)rollsum_lds_bytes<SD>(true)
         : what == 3 ? (rollsum_fits<SD>() ? 1 : 0) : what == 4 ? (long long)rollsum_lds_bytes<SD>(false)
         : what == 7 ? rollsum_waves<SD>(false) : what == 8 ? rollsum_waves<SD>(true) : -1;
}

}  // namespace clik
