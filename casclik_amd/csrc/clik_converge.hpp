// Rollouts that run until each instance has converged (clik_*_converge_batch, include/clik.h): closed-loop inverse
// kinematics for a batch in one launch.  The lane-per-instance, image-in-LDS Euler loop of the recording rollouts with
// the time and the target frozen - every tick reads ONE TickArgs record and the target rows the launch came with - and a
// stop test at the top of every tick.  A lane that has stopped keeps its state; a wave leaves the loop as soon as a
// ballot shows none of its lanes active, so a launch costs every wave the ticks of its own slowest instance and no more.
//
// The stop rule of instance b, r = 0, 1, ... (clik.h has it in full): evaluate every constraint at (t, z_r, y); dist_i
// is |e_i|, on a SetConstraint row the distance outside [lo_i, hi_i] (the bounds as summary_task takes them).  A
// non-finite e_i stops with CLIK_CONVERGE_NONFINITE; dist_i <= tol_i on every row with CLIK_CONVERGE_OK (tol_i = +inf:
// the row cannot block); r == max_ticks with CLIK_CONVERGE_MAX_TICKS.  Otherwise tick r is solved: an infeasible QP stops
// with CLIK_CONVERGE_INFEASIBLE, a step of at most min_step (> 0) with CLIK_CONVERGE_STALLED - the state as it was - and
// any other is integrated.  `ticks` is r at the stop: the ticks that were integrated.
//
// Nothing in the loop is shared between waves: no per-tick table, no record, no per-tick target, hence no barrier.  The
// waves of a block leave at different ticks and meet again at the barriers behind the loop.  The lane's control state
// (active, ticks, status) and its dist values live in registers; LDS holds the skill image, the wave's state and target
// rows and the [MT] tolerances, nothing else - so the block is smaller than the summarising rollout's and the waves per
// block are worked out again from that.
//
// A header and translation units of its own (jit.py, _CONVERGE_TEMPLATE / _QP_CONVERGE_TEMPLATE; CLIK_CONVERGE_QP
// selects the QP controller's loop).  The units include, ahead of this header, what the summarising rollouts' units
// include - clik_pinv_rec.hpp / clik_qp_rec.hpp and clik_summary.hpp, read-only - and this header includes nothing
// itself.
#pragma once

namespace clik {

// status of an instance (include/clik.h: CLIK_CONVERGE_*)
constexpr int kConvOk = 0, kConvMaxTicks = 1, kConvStalled = 2, kConvInfeasible = 3, kConvNonFinite = 4, kConvCancelled = 5;

// The group rule (include/clik.h), compiled in: the lanes [g G, (g + 1) G) of a wave are one group - the seeds of one
// target of a multi-seed launch -, and a lane that is still active behind the stop test of tick r stops there with
// kConvCancelled once a lane of its group has stopped with kConvOk.  G divides 64 and the host asks for B % G == 0, so a
// group never spans two waves and is valid as a whole or not at all.  G == 1: the kernels as they are without the rule.
#ifndef CLIK_CONVERGE_GROUP
#define CLIK_CONVERGE_GROUP 1
#endif
constexpr int kConvGroup = CLIK_CONVERGE_GROUP;
static_assert(kConvGroup == 1 || kConvGroup == 2 || kConvGroup == 4 || kConvGroup == 8 || kConvGroup == 16 ||
              kConvGroup == 32 || kConvGroup == 64, "CLIK_CONVERGE_GROUP is one of 1, 2, 4, 8, 16, 32, 64");

// what a launch reads and writes beside the state (device pointers)
struct ConvergeArgs {
    const double* tol;          // [MT]
    int32_t* ticks;             // [B]
    int32_t* status;            // [B]
    double* residual;           // [B][MT]
    int max_ticks;
    double dt, max_speed, min_step;
};

// task TI of the lane's instance at its present state: dist of every row into `dist` where the lane is active (a
// stopped lane keeps what it had), `met` cleared by a row outside its tolerance, `nonfin` set by a non-finite e.  One
// task's e is live at a time.  (Only e is read: the Jacobian the evaluation shares products with is dead here, so e may
// differ from the constraint-value kernel's in the last place - far inside every tolerance a caller can ask for.)
template <const ShapeDesc& SD, int TI>
__device__ __forceinline__ void converge_task(const Img<SD>* __restrict__ S, const TickArgs& tk, const Kin<SD.n>& K,
                                              const double (&z)[SD.n], const double* ys, const double* tol, const int lane,
                                              const bool active, double (&dist)[SummaryLayout<SD>::MT > 0 ? SummaryLayout<SD>::MT : 1],
                                              bool& met, unsigned& nonfin)
{
    if constexpr (TI < SD.n_tasks) {
        constexpr int N = SD.n, M = SD.m[TI];
        constexpr int m0 = summary_row_base(SD, TI);
        constexpr bool SET = SD.cls[TI] == CLIK_CLS_SET;
        double e[M], J[M][N], Jt[M];
        task_eval_s<SD, TI>(S, tk, K, z, ys, lane, e, J, Jt);
        [[maybe_unused]] double lo[M], hi[M];
        if constexpr (SET) {
            constexpr int bits = shape_attr_bits(SD, TI);
            constexpr int an = shape_attr_off(SD, TI, 16);
            [[maybe_unused]] double at[an > 0 ? an : 1];
            if constexpr ((bits & (CLIK_ATTR_SET_MIN | CLIK_ATTR_SET_MAX)) != 0)
                ExternAttr<TI>::template eval<N>(z, ys, tk.tv, K, at);
            constexpr int olo = shape_attr_off(SD, TI, CLIK_ATTR_SET_MIN);
            constexpr int ohi = shape_attr_off(SD, TI, CLIK_ATTR_SET_MAX);
            static_for<0, M>([&](auto kc) __attribute__((always_inline)) {
                constexpr int k = decltype(kc)::value;
                if constexpr ((bits & CLIK_ATTR_SET_MIN) != 0) lo[k] = at[olo + k];
                else lo[k] = S->tasks[TI].set_min[k];
                if constexpr ((bits & CLIK_ATTR_SET_MAX) != 0) hi[k] = at[ohi + k];
                else hi[k] = S->tasks[TI].set_max[k];
            });
        }
        static_for<0, M>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value;
            constexpr int row = m0 + i;
            const double ev = e[i];
            double d = fabs(ev);
            if constexpr (SET) d = fmax(fmax(lo[i] - ev, ev - hi[i]), 0.0);
            met = met & (d <= tol[row]);
            nonfin |= summary_nonfinite(ev);
            dist[row] = active ? d : dist[row];
        });
        __builtin_amdgcn_sched_barrier(0);
        converge_task<SD, TI + 1>(S, tk, K, z, ys, tol, lane, active, dist, met, nonfin);
    }
}

// the stop test of tick r (steps 1 - 4 of the rule): the constraints at the lane's state, then `active`, `status` and
// `ticks` of a lane that stops here.  The solve's arithmetic stays behind it: one of the two is live at a time.
template <const ShapeDesc& SD>
__device__ __forceinline__ void converge_test(const Img<SD>* __restrict__ S, const TickArgs& tk, const double (&z)[SD.n],
                                              const double* ys, const double* tol, const int lane, const int r,
                                              const int max_ticks,
                                              double (&dist)[SummaryLayout<SD>::MT > 0 ? SummaryLayout<SD>::MT : 1],
                                              bool& active, int& status, int& ticks)
{
    constexpr int N = SD.n;
    bool met = true;
    unsigned nonfin = 0u;
    {
        Kin<N> K;
        if constexpr (SD.uses_fk != 0) {
            forward_kinematics_s<SD>(S, z, K);
            if constexpr (SD.quat_src != 0) orientation_feature_s<SD>(S, ys, lane, K);
        }
        converge_task<SD, 0>(S, tk, K, z, ys, tol, lane, active, dist, met, nonfin);
    }
    const int st = nonfin != 0u ? kConvNonFinite : met ? kConvOk : r == max_ticks ? kConvMaxTicks : -1;
    if (active && st >= 0) {
        active = false;
        status = st;
        ticks = r;
    }
    __builtin_amdgcn_sched_barrier(0);
}

// the group rule of tick r, right behind its stop test: one ballot of the lanes that have stopped with kConvOk (a lane
// past the end of the batch starts stopped with that status and is no winner: `valid`), the lane's own group cut out of
// it.  A lane the test itself stopped at r is not active and keeps its status; a cancelled lane keeps its state and the
// dist values of this test.  Called by all 64 lanes (the loops around it branch on ballots only).
template <int G>
__device__ __forceinline__ void converge_group(const bool valid, const int lane, const int r, bool& active, int& status,
                                               int& ticks)
{
    if constexpr (G > 1) {
        constexpr unsigned long long mask = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
        const unsigned long long won = __ballot(valid && !active && status == kConvOk);
        if (active && ((won >> (lane & ~(G - 1))) & mask) != 0ull) {
            active = false;
            status = kConvCancelled;
            ticks = r;
        }
    }
}

// the lane's [MT] residuals, after the loop (NaN by bits for an instance that stopped on a non-finite value)
template <const ShapeDesc& SD>
__device__ __forceinline__ void converge_store(const ConvergeArgs& ca, const long long inst, const int ticks,
                                               const int status, const unsigned nan_hi,
                                               const double (&dist)[SummaryLayout<SD>::MT > 0 ? SummaryLayout<SD>::MT : 1])
{
    constexpr int MT = SummaryLayout<SD>::MT;
    ca.ticks[inst] = ticks;
    ca.status[inst] = status;
#pragma unroll
    for (int i = 0; i < MT; ++i) ca.residual[(size_t)inst * MT + i] = nan_or(dist[i], nan_hi);
}

#ifndef CLIK_CONVERGE_QP
// ---- PseudoInverseController ------------------------------------------------------------------------------------------
// A block is WV waves that share ONE copy of the skill image and of the tolerances; every wave owns 64 instances.
// LDS: [skill image | tol (MT, even) | wave 0: zs (N slots) ys (n_y slots) | wave 1 ...], slot = 64 doubles
template <const ShapeDesc& SD>
constexpr size_t pinv_converge_lds_bytes(int wv)
{
    return ((size_t)StaticLayout<SD>::IMG_DOUBLES + SummaryLayout<SD>::TOL_DOUBLES
            + (size_t)wv * lane_wave_doubles<SD, false>(0)) * sizeof(double);
}
template <const ShapeDesc& SD>
constexpr int pinv_converge_waves()
{
    return waves_per_block<pinv_converge_lds_bytes<SD>>(kSummaryLdsCap);
}

template <const ShapeDesc& SD, int WV>
__global__ __launch_bounds__(WV * WAVE) CLIK_ROLL_ATTR void pinv_converge_static_kernel(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, int32_t* __restrict__ mode_out, const long long B, const TickArgs tk,
    double* __restrict__ x, double* __restrict__ dx, const ConvergeArgs ca)
{
    extern __shared__ double lds[];
    using SL = SummaryLayout<SD>;
    constexpr int N = SD.n;
    constexpr int NX = SD.n_x, NQ = N - NX;
    constexpr int NY = SD.n_y > 0 ? SD.n_y : 0;
    constexpr int MT = SL::MT;
    const WavePlace<WV> w(B);       // (a wave past the end of the batch loads the first rows, never enters the loop, stores nothing)
    const int lane = w.lane;
    const long long b0 = w.b0;
    const bool valid = w.valid;
    double* tols = lds + StaticLayout<SD>::IMG_DOUBLES;
    double* zs = tols + SL::TOL_DOUBLES + w.wave * lane_wave_doubles<SD, false>(0);
    double* xs = zs + NQ * WAVE;
    double* ys = zs + N * WAVE;
    typedef double d2 __attribute__((ext_vector_type(2)));
    {
        const d2* src = (const d2*)img_g;
        d2* dst = (d2*)lds;
        for (int k = w.wave; k < StaticLayout<SD>::IMG_CHUNKS; k += WV) dst[k * WAVE + lane] = src[k * WAVE + lane];
        for (int k = threadIdx.x; k < MT; k += WV * WAVE) tols[k] = ca.tol[k];
        StagedRows<NQ, NX, NY> rows;
        rows.load(q, x, y, w);
        rows.to_lds(zs, xs, ys, lane);
    }
    __syncthreads();
    const Img<SD>* __restrict__ S = (const Img<SD>*)lds;
    const double* ysl = ys + lane * NY;
    double z[N];
    state_from_lds<NQ, NX>(zs, xs, lane, z);
    double vout[N], dist[MT > 0 ? MT : 1];
    int acc_mode = -1;
#pragma unroll
    for (int j = 0; j < N; ++j) vout[j] = 0.0;
#pragma unroll
    for (int i = 0; i < (MT > 0 ? MT : 1); ++i) dist[i] = 0.0;
    bool active = valid;
    int ticks = 0, status = kConvOk;
    // (r <= max_ticks by the test's own step 4: the loop ends whatever the data)
#pragma unroll 1
    for (int r = 0; __ballot(active) != 0ull; ++r) {
        asm volatile("" ::: "memory");      // (keeps the image reads inside the loop, see pinv_rollout_static_body)
        converge_test<SD>(S, tk, z, ysl, tols, lane, r, ca.max_ticks, dist, active, status, ticks);
        converge_group<kConvGroup>(valid, lane, r, active, status, ticks);
        if (__ballot(active) == 0ull) break;
        double vt[N];
        int mt = -1;
        pinv_tick_static<SD>(S, tk, z, ysl, lane, active, vt, mt);
        const double step = clamp_step_size<N, NQ>(vt, ca.max_speed, ca.dt);
        if (active && ca.min_step > 0.0 && step <= ca.min_step) {
            active = false;
            status = kConvStalled;
            ticks = r;
        }
        if (active) {
            acc_mode = mt;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                vout[j] = vt[j];
                z[j] = fma(vt[j], ca.dt, z[j]);
            }
            // (velocity feedback: a tick that was integrated, and no other, feeds the next; a stopped lane keeps its row)
            if constexpr (kVelFeedbackN > 0) velocity_feed<SD>(vt, 0u, ys + lane * NY);
        }
    }
    const unsigned nan_hi = (status == kConvNonFinite) ? 0x7ff80000u : 0u;
    if (valid) converge_store<SD>(ca, b0 + lane, ticks, status, nan_hi, dist);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        z[j] = nan_or(z[j], nan_hi);
        vout[j] = nan_or(vout[j], nan_hi);
    }
    rows_out<NQ, NX>(z, q, x, w, zs, xs);
    rows_out<NQ, NX>(vout, dq, dx, w, zs, xs);
    if (mode_out != nullptr && valid) mode_out[b0 + lane] = acc_mode;
}

template <const ShapeDesc& SD>
constexpr bool converge_fits() { return pinv_converge_waves<SD>() > 0; }
template <const ShapeDesc& SD>
constexpr int converge_waves() { return pinv_converge_waves<SD>(); }
template <const ShapeDesc& SD>
constexpr size_t converge_lds_bytes()
{
    // (a shape that does not fit: the figure of one wave, for the refusal)
    constexpr int wv = pinv_converge_waves<SD>();
    return pinv_converge_lds_bytes<SD>(wv > 0 ? wv : 1);
}
template <const ShapeDesc& SD>
inline const void* converge_kernel_ptr()
{
    return (const void*)pinv_converge_static_kernel<SD, (pinv_converge_waves<SD>() > 0 ? pinv_converge_waves<SD>() : 1)>;
}

template <const ShapeDesc& SD>
inline hipError_t launch_converge_static(const LaunchArgs& a, const TickArgs& tk, long long B, double* q, const double* y,
                                         double* dq, int32_t* mode, hipStream_t stream, const ConvergeArgs& ca)
{
    if constexpr (!converge_fits<SD>()) {
        return hipErrorInvalidValue;        // (refused at attach time with the figure: jit._converge_entry)
    } else {
        if (B < 1 || ca.max_ticks < 0 || ca.tol == nullptr || ca.ticks == nullptr || ca.status == nullptr ||
            ca.residual == nullptr)
            return hipErrorInvalidValue;
        if constexpr (kConvGroup > 1) {
            if (B % kConvGroup != 0) return hipErrorInvalidValue;       // (a group is whole: the host checks it first)
        }
        if (SD.n_x != 0 && (a.roll_x == nullptr || a.roll_dx == nullptr)) return hipErrorInvalidValue;
        constexpr int WV = pinv_converge_waves<SD>();
        const long long per_block = (long long)WV * WAVE;
        const long long blocks = (B + per_block - 1) / per_block;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
        return launch_with_lds(pinv_converge_static_kernel<SD, WV>, (unsigned)blocks, WV * WAVE, converge_lds_bytes<SD>(),
                               stream, a.dImg, q, y, dq, mode, B, tk, a.roll_x, a.roll_dx, ca);
    }
}

#else
// ---- ReactiveQPController ---------------------------------------------------------------------------------------------
// One wave per block: the tick's work area is the larger part of it.
// LDS: [QP image | the tick's slots (QpLayout) | tol (MT, even)]
template <const ShapeDesc& SD>
constexpr size_t qp_converge_lds_bytes()
{
    return QpLayout<SD>::LDS_BYTES + (size_t)SummaryLayout<SD>::TOL_DOUBLES * sizeof(double);
}

// `valid && active` goes into qp_tick_static: all three of its solvers start a lane that is not valid as done, so a
// stopped lane takes part in no further active-set pass and cannot hold the wave in one; its working-set word stays too.
template <const ShapeDesc& SD>
__global__ __launch_bounds__(WAVE) void qp_converge_static_kernel(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, double* __restrict__ slack_out, int32_t* __restrict__ status_out, const long long B,
    const TickArgs tk, double* __restrict__ x, double* __restrict__ dx, const ConvergeArgs ca)
{
    extern __shared__ double lds[];
    using LY = QpLayout<SD>;
    using SL = SummaryLayout<SD>;
    constexpr int N = SD.n;
    constexpr int NX = SD.n_x, NQ = N - NX;
    constexpr int NS = LY::NS;
    constexpr int NY = SD.n_y > 0 ? SD.n_y : 0;
    constexpr int MT = SL::MT;
    const WavePlace<1> w(B);
    const int lane = w.lane;
    const long long b0 = w.b0;
    const bool valid = w.valid;
    double* slots = lds + LY::IMG_DOUBLES;
    double* zs = slots + LY::O_Z * WAVE;
    double* ys = slots + LY::O_Y * WAVE;
    double* tols = slots + LY::SLOTS * WAVE;
    typedef double d2 __attribute__((ext_vector_type(2)));
    {
        d2 img[LY::IMG_CHUNKS];
        const d2* src = (const d2*)img_g;
#pragma unroll
        for (int k = 0; k < LY::IMG_CHUNKS; ++k) img[k] = src[k * WAVE + lane];
        StagedRows<NQ, NX, NY> rows;
        rows.load(q, x, y, w);
        d2* dst = (d2*)lds;
#pragma unroll
        for (int k = 0; k < LY::IMG_CHUNKS; ++k) dst[k * WAVE + lane] = img[k];
        for (int k = lane; k < MT; k += WAVE) tols[k] = ca.tol[k];
        rows.to_lds(zs, zs + NQ * WAVE, ys, lane);
    }
    __syncthreads();
    const Img<SD>* __restrict__ S = (const Img<SD>*)lds;
    const QpTail* __restrict__ T = (const QpTail*)((const char*)lds + LY::TAIL_OFF);
    const double* ysl = ys + lane * NY;
    double* xs = zs + NQ * WAVE;
    double z[N];
    state_from_lds<NQ, NX>(zs, xs, lane, z);
    double v[N], sl[LY::NSA], dist[MT > 0 ? MT : 1];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = 0.0;
#pragma unroll
    for (int k = 0; k < LY::NSA; ++k) sl[k] = 0.0;
#pragma unroll
    for (int i = 0; i < (MT > 0 ? MT : 1); ++i) dist[i] = 0.0;
    int32_t hot = 0;
    int worst = 0;
    bool active = valid;
    int ticks = 0, status = kConvOk;
    // (r <= max_ticks by the test's own step 4: the loop ends whatever the data)
#pragma unroll 1
    for (int r = 0; __ballot(active) != 0ull; ++r) {
        asm volatile("" ::: "memory");      // (keeps the image reads inside the loop, see pinv_rollout_static_body)
        converge_test<SD>(S, tk, z, ysl, tols, lane, r, ca.max_ticks, dist, active, status, ticks);
        converge_group<kConvGroup>(valid, lane, r, active, status, ticks);
        if (__ballot(active) == 0ull) break;
        double vt[N], st_sl[LY::NSA];
        const int st = qp_tick_static<SD>(S, T, tk, z, ysl, lane, active, slots, vt, st_sl, &hot, r > 0);
        const double step = clamp_step_size<N, NQ>(vt, ca.max_speed, ca.dt);
        if (active) {
            worst = st > worst ? st : worst;
            if (st == 2) {                  // an infeasible tick: the state stays where it is
                active = false;
                status = kConvInfeasible;
                ticks = r;
            } else if (ca.min_step > 0.0 && step <= ca.min_step) {
                active = false;
                status = kConvStalled;
                ticks = r;
            }
        }
        if (active) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                v[j] = vt[j];
                z[j] = fma(vt[j], ca.dt, z[j]);
            }
            // (velocity feedback: a tick that was integrated, and no other, feeds the next; a stopped lane keeps its row)
            if constexpr (kVelFeedbackN > 0) velocity_feed<SD>(vt, 0u, ys + lane * NY);
#pragma unroll
            for (int k = 0; k < LY::NSA; ++k) sl[k] = st_sl[k];
        }
    }
    const unsigned nan_hi = (status == kConvNonFinite) ? 0x7ff80000u : 0u;
    if (valid) converge_store<SD>(ca, b0 + lane, ticks, status, nan_hi, dist);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        z[j] = nan_or(z[j], nan_hi);
        v[j] = nan_or(v[j], nan_hi);
    }
    rows_out<NQ, NX>(z, q, x, w, zs, xs);
    rows_out<NQ, NX>(v, dq, dx, w, zs, xs, [&]() __attribute__((always_inline)) {
        if constexpr (NS > 0) {
            double* so = slots + LY::O_SL * WAVE;
            if (slack_out != nullptr) {
#pragma unroll
                for (int k = 0; k < NS; ++k) so[lane * NS + k] = nan_or(sl[k], nan_hi);
            }
        }
    });
    if constexpr (NS > 0) {
        if (slack_out != nullptr) rows_from_lds<NS>(slack_out + b0 * NS, w.rows_store, slots + LY::O_SL * WAVE, lane);
    }
    if (status_out != nullptr && valid) status_out[b0 + lane] = worst;
}

template <const ShapeDesc& SD>
constexpr bool converge_fits() { return qp_converge_lds_bytes<SD>() <= kSummaryLdsCap; }
template <const ShapeDesc& SD>
constexpr int converge_waves() { return 1; }
template <const ShapeDesc& SD>
constexpr size_t converge_lds_bytes() { return qp_converge_lds_bytes<SD>(); }
template <const ShapeDesc& SD>
inline const void* converge_kernel_ptr() { return (const void*)qp_converge_static_kernel<SD>; }

template <const ShapeDesc& SD>
inline hipError_t launch_qp_converge_static(const void* d_img, const TickArgs& tk, long long B, double* q, const double* y,
                                            double* dq, double* slack, int32_t* status, double* x, double* dx,
                                            hipStream_t stream, const ConvergeArgs& ca)
{
    if constexpr (!converge_fits<SD>()) {
        return hipErrorInvalidValue;        // (refused at attach time with the figure: jit._converge_entry)
    } else {
        if (B < 1 || ca.max_ticks < 0 || ca.tol == nullptr || ca.ticks == nullptr || ca.status == nullptr ||
            ca.residual == nullptr)
            return hipErrorInvalidValue;
        if constexpr (kConvGroup > 1) {
            if (B % kConvGroup != 0) return hipErrorInvalidValue;       // (a group is whole: the host checks it first)
        }
        if (SD.n_x != 0 && (x == nullptr || dx == nullptr)) return hipErrorInvalidValue;
        const long long blocks = (B + WAVE - 1) / WAVE;
        if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
        return launch_with_lds(qp_converge_static_kernel<SD>, (unsigned)blocks, WAVE, converge_lds_bytes<SD>(), stream,
                               d_img, q, y, dq, slack, status, B, tk, x, dx, ca);
    }
}
#endif

// what a caller may ask about the instantiation (clik_jit_converge_info): 0 rows, 1 SetConstraint rows, 2 LDS bytes of a
// block, 3 fits the LDS of a CU, 4 waves of a block, 5 bytes of scratch per lane as the loaded code object states them
// (-1: no device to ask), 6 the group size the unit was compiled with (CLIK_CONVERGE_GROUP), 7 + k the compiled-in
// velocity feedback map (velocity_feedback_info(k), clik_rollout_lane.hpp)
template <const ShapeDesc& SD>
inline long long converge_info(int what)
{
    using LY = SummaryLayout<SD>;
    if (what >= 7) return velocity_feedback_info(what - 7);
    if (what == 5) {
        if constexpr (!converge_fits<SD>()) {
            return -1;
        } else {
            return kernel_scratch_bytes(converge_kernel_ptr<SD>());
        }
    }
    return what == 0 ? LY::MT : what == 1 ? LY::MS : what == 2 ? (long long)converge_lds_bytes<SD>()
         : what == 3 ? (converge_fits<SD>() ? 1 : 0) : what == 4 ? converge_waves<SD>() : what == 6 ? kConvGroup : -1;
}

}  // namespace clik
