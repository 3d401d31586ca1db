// Rollouts that record their trajectory and read one target per tick (clik_pinv_rollout_batch_rec, include/clik.h; RollRec in
// clik_device.hpp): the loops of clik_pinv_team.hpp and clik_pinv_kernels.hpp again, with one RollRec - records and per-tick
// targets - and their launchers.  A header of its own, included by the on-demand translation units only (casclik_amd/jit.py):
// the compiler's code for a kernel depends on what else its translation unit declares - with these templates declared next
// to them, the rollouts that record nothing fused their multiply-adds in another order, and their results are pinned to the
// tick kernels' (the smoke test: q after one tick to 1e-12).
// The lane-per-instance loop (pinv_rollout_static_body) is the one text of the recording rollout and, with a hook that
// folds every tick's state (clik_rollout_lane.hpp: NoTickHook), of the rollout that summarises its constraint values.
#pragma once
#include "clik_pinv_kernels.hpp"
#include "clik_rollout_lane.hpp"
namespace clik {

// One record of a team rollout (RollRec): plain stores, nothing waits for them.  The state is replicated over the quad;
// lane r stores elements 2r and 2r + 1 of both rows, so that all 64 lanes of the wave issue stores
// (CLIK_REC_QUAD_SPLIT=0: lane 0 stores the whole rows, as the final stores do - measured in profiles/rollout_record.md).
#ifndef CLIK_REC_QUAD_SPLIT
#define CLIK_REC_QUAD_SPLIT 1
#endif
template <int N>
__device__ __forceinline__ void team_record(const RollRec& ra, const long long row, const int r, const double (&z)[N],
                                            const double (&v)[N], const int mode)
{
#if CLIK_REC_QUAD_SPLIT
    double z0 = z[N - 1], z1 = z[N - 1], v0 = v[N - 1], v1 = v[N - 1];
    static_for<0, TEAM>([&](auto kc) __attribute__((always_inline)) {
        constexpr int k = decltype(kc)::value;
        if constexpr (2 * k < N) {
            z0 = (r == k) ? z[2 * k] : z0;
            v0 = (r == k) ? v[2 * k] : v0;
        }
        if constexpr (2 * k + 1 < N) {
            z1 = (r == k) ? z[2 * k + 1] : z1;
            v1 = (r == k) ? v[2 * k + 1] : v1;
        }
    });
    static_assert(N <= 2 * TEAM, "a quad stores two elements per lane");
    if (2 * r < N) {
        if (ra.q != nullptr) ra.q[row * N + 2 * r] = z0;
        if (ra.dq != nullptr) ra.dq[row * N + 2 * r] = v0;
    }
    if (2 * r + 1 < N) {
        if (ra.q != nullptr) ra.q[row * N + 2 * r + 1] = z1;
        if (ra.dq != nullptr) ra.dq[row * N + 2 * r + 1] = v1;
    }
    if (r == TEAM - 1 && ra.flag != nullptr) ra.flag[row] = mode;
#else
    if (r == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            if (ra.q != nullptr) ra.q[row * N + j] = z[j];
            if (ra.dq != nullptr) ra.dq[row * N + j] = v[j];
        }
        if (ra.flag != nullptr) ra.flag[row] = mode;
    }
#endif
}

// n_ticks of (tick -> clamp(+-max_speed) -> integrate) in one launch with four lanes per instance: the host loop
// of the notebooks (ur5_moe2016_example2.ipynb:537-545) without the per-tick launch and HBM round trip, the state
// in registers (replicated over the quad).  stages = 1: explicit Euler; 4: classical Runge-Kutta with the
// controller as the right-hand side (see pinv_rollout_static_kernel).  q is updated in place; dq / mode receive
// the last tick (Runge-Kutta: the combined rate and the mode of the first stage).
// ra: records of the trajectory and one target row per tick (RollRec, clik_device.hpp).
template <const ShapeDesc& SD, class IMGV, int STAGES>
__device__ __forceinline__ void pinv_rollout_static_team_body(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, int32_t* __restrict__ mode_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed, const RollRec ra)
{
    static_assert(STAGES == 1 || STAGES == 4, "explicit Euler or classical Runge-Kutta");
    constexpr int stages = STAGES;
    static_assert(shape_team_ok(SD), "shape outside the team kernel's family");
    constexpr bool VALUES = !std::is_void<IMGV>::value;
    extern __shared__ double lds[];
    constexpr int N = SD.n, NY = SD.n_y > 0 ? SD.n_y : 0;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = tid & (TEAM - 1);
    const int inst = tid >> 2;
    const long long b0 = (long long)blockIdx.x * TEAM_INST;
    const bool valid = b0 + inst < B;
    const long long binst = valid ? (b0 + inst) : (B - 1);
    double* ys = lds + (VALUES ? 0 : StaticLayout<SD>::IMG_DOUBLES);        // [64][NY] (image-reading build only)
    double z[N], ydir[NY > 0 ? NY : 1];
#pragma unroll
    for (int j = 0; j < N; ++j) z[j] = q[binst * N + j];
    if constexpr (NY > 0) {
#pragma unroll
        for (int k = 0; k < NY; ++k) ydir[k] = y[binst * NY + k];
    }
    if constexpr (!VALUES) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        constexpr int CH = StaticLayout<SD>::IMG_CHUNKS;
        const d2* src = (const d2*)img_g;
        d2* dst = (d2*)lds;
        const int lane = tid & (WAVE - 1);
        for (int ck = wave; ck < CH; ck += TEAM_WAVES) dst[ck * WAVE + lane] = src[ck * WAVE + lane];
        if constexpr (NY > 0) {
            // (run-time input indices: the rows of the image-reading build live in LDS; the quad writes the same values)
#pragma unroll
            for (int k = 0; k < NY; ++k) ys[inst * NY + k] = ydir[k];
        }
        __syncthreads();
    }
    constexpr Img<SD> Sval = []() constexpr { if constexpr (VALUES) return IMGV::value; else return Img<SD>{}; }();
    const Img<SD>* __restrict__ Slds = VALUES ? &Sval : (const Img<SD>*)lds;
    const double* ysl = VALUES ? ydir : ys + inst * NY;
    RoleConsts rc;
    if constexpr (VALUES) rc = role_consts_loaded<IMGV>(r);
    else rc = role_consts_computed(r, Slds->lam);
    const SinCosK sck = sincos_consts();        // (once per launch)
    const int nts = Slds->n_tslots;
    double vout[N];
    int acc_mode = -1;
#pragma unroll
    for (int j = 0; j < N; ++j) vout[j] = 0.0;
    // (no clamp = a bound no finite velocity reaches: the same two instructions, no test per element)
    const double vmax = max_speed > 0.0 ? max_speed : 1.7976931348623157e308;
    // the accepted candidate in every lane of the quad: mode 0 lives in lane 0, mode 1 in lane 3 - lane 0's value is
    // broadcast, and only quads that rejected mode 0 (a uniform decision inside a quad) fetch lane 3's on top
    auto accepted = [&](const double (&v)[N], const bool ok0, double (&d)[N]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < N; ++j) d[j] = quad_perm_f64<0x00>(v[j]);
        if (__builtin_amdgcn_ballot_w64(!ok0) != 0ull) {
            if (!ok0) {
#pragma unroll
                for (int j = 0; j < N; ++j) d[j] = quad_perm_f64<0xFF>(v[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < N; ++j) d[j] = fmax(fmin(d[j], vmax), -vmax);
    };
    auto sincos_args = [&](const double (&zz)[N], double& a0, double& a1) __attribute__((always_inline)) {
        // lane r's two sin / cos arguments out of the replicated state (register selects)
        a0 = zz[N - 1];
        a1 = zz[N - 1];
        static_for<0, TEAM>([&](auto kc) __attribute__((always_inline)) {
            constexpr int k = decltype(kc)::value;
            if constexpr (2 * k < N) a0 = (r == k) ? zz[2 * k] : a0;
            if constexpr (2 * k + 1 < N) a1 = (r == k) ? zz[2 * k + 1] : a1;
        });
    };
    RecClock clk;
    [[maybe_unused]] double ynext[NY > 0 ? NY : 1];
    clk.start(ra);
    if constexpr (NY > 0) {
#pragma unroll
        for (int k = 0; k < NY; ++k) ynext[k] = ydir[k];
    }
#pragma unroll 1
    for (int tick = 0; tick < n_ticks; ++tick) {
        if constexpr (NY > 0) {
            // per-tick target: the NEXT tick's row is requested here, a whole tick before it is used
            if (ra.y_stride != 0) {
                const double* yn = next_rows(y, ra, tick, n_ticks) + binst * NY;
#pragma unroll
                for (int k = 0; k < NY; ++k) ynext[k] = yn[k];
            }
        }
        if constexpr (STAGES == 1) {
            // explicit Euler (the notebooks' loop, ur5_moe2016_example2.ipynb:537-545): nothing of the Runge-Kutta
            // staging - no saved state, no stage sums, no weights
            asm volatile("" ::: "memory");      // (keeps the image reads inside the loop, see pinv_rollout_static_kernel)
            const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + (size_t)tick * 2 * nts);
            double a0, a1;
            sincos_args(z, a0, a1);
            double v[N];
            bool in_tc;
            team_tick<SD>(Slds, tk, z, ysl, a0, a1, r, inst, rc, sck, v, in_tc);
            const bool ok0 = __builtin_amdgcn_mov_dpp((int)in_tc, QUAD_LANE0, 0xf, 0xf, true) != 0;
            accepted(v, ok0, vout);
#pragma unroll
            for (int j = 0; j < N; ++j) z[j] = fma(vout[j], dt, z[j]);
            acc_mode = ok0 ? 0 : 1;
        } else {
        double z0[N], ks[N];
        int mode0 = -1;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            z0[j] = z[j];
            ks[j] = 0.0;
        }
#pragma unroll 1
        for (int st = 0; st < stages; ++st) {
            asm volatile("" ::: "memory");
            const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + ((size_t)tick * stages + st) * 2 * nts);
            double a0, a1;
            sincos_args(z, a0, a1);
            double v[N], d[N];
            bool in_tc;
            team_tick<SD>(Slds, tk, z, ysl, a0, a1, r, inst, rc, sck, v, in_tc);
            const bool ok0 = __builtin_amdgcn_mov_dpp((int)in_tc, QUAD_LANE0, 0xf, 0xf, true) != 0;
            accepted(v, ok0, d);
            const double wgt = (st == 0 || st == 3) ? 1.0 : 2.0;
            const double cnext = (st == 2) ? dt : 0.5 * dt;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                ks[j] = fma(wgt, d[j], ks[j]);
                z[j] = fma(d[j], cnext, z0[j]);
            }
            mode0 = (st == 0) ? (ok0 ? 0 : 1) : mode0;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            vout[j] = ks[j] * (1.0 / 6.0);
            z[j] = fma(vout[j], dt, z0[j]);
        }
        acc_mode = mode0;
        }
        if (clk.due(ra)) {
            if (valid) team_record<N>(ra, clk.r * B + b0 + inst, r, z, vout, acc_mode);
            ++clk.r;
        }
        if constexpr (NY > 0) {
#pragma unroll
            for (int k = 0; k < NY; ++k) {
                ydir[k] = ynext[k];
                if constexpr (!VALUES) ys[inst * NY + k] = ynext[k];
            }
        }
    }
    if (r == 0 && valid) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            q[(b0 + inst) * N + j] = z[j];
            dq[(b0 + inst) * N + j] = vout[j];
        }
        if (mode_out != nullptr) mode_out[b0 + inst] = acc_mode;
    }
}

// (a body and a kernel that calls it, here and below, not one function: the compiler's code for the loop differs between
// the two forms, and these kernels' code is held to what it was)
template <const ShapeDesc& SD, class IMGV = void, int STAGES = 1>
__global__ __launch_bounds__(TEAM_WAVES * WAVE) void pinv_rollout_static_team_rec_kernel(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, int32_t* __restrict__ mode_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed, const RollRec rec)
{
    pinv_rollout_static_team_body<SD, IMGV, STAGES>(img_g, q, y, dq, mode_out, B, tterms, n_ticks, dt, max_speed, rec);
}

// One record of a lane-per-instance rollout (RollRec): the lane stores its own rows with plain stores, nothing waits
// for them.  z / v hold the NQ robot variables, then the NX virtual ones.
template <int NQ, int NX>
__device__ __forceinline__ void lane_record(const RollRec& ra, const long long row, const double (&z)[NQ + NX],
                                            const double (&v)[NQ + NX], const int flag)
{
    if (ra.q != nullptr) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) ra.q[row * NQ + j] = z[j];
    }
    if (ra.dq != nullptr) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) ra.dq[row * NQ + j] = v[j];
    }
    if constexpr (NX > 0) {
        if (ra.x != nullptr) {
#pragma unroll
            for (int j = 0; j < NX; ++j) ra.x[row * NX + j] = z[NQ + j];
        }
        if (ra.dx != nullptr) {
#pragma unroll
            for (int j = 0; j < NX; ++j) ra.dx[row * NX + j] = v[NQ + j];
        }
    }
    if (ra.flag != nullptr) ra.flag[row] = flag;
}

// (one wave per SIMD, stated: the register copy of the skill image lives across the tick loop, and without the
// statement the allocator parks a few of its values in scratch although the wave could use all 512 registers)
#ifndef CLIK_ROLL_ATTR
#define CLIK_ROLL_ATTR __attribute__((amdgpu_waves_per_eu(1, 1)))
#endif
// RK: classical Runge-Kutta (four controller evaluations per tick) instead of explicit Euler.  Two
// instantiations, because the Runge-Kutta bookkeeping (start state and weighted sum of the stage velocities, kept
// in LDS) would otherwise sit in the Euler loop's registers and push the widest stacks into scratch.
// ra: records of the trajectory and one target row per tick (RollRec, clik_device.hpp).
// WV: waves per block; they share ONE copy of the skill image, and every wave has a region of its own behind it:
//   LDS: [skill image | wave 0: zs (N slots) ys (n_y slots) (Runge-Kutta: z0s, kss, N slots each) the hook's doubles | wave 1 ...]
// REGIMG: the Euler loop reads the image from a register copy; otherwise from LDS in place, as the Runge-Kutta loop always
// does (with the register copy the widest stacks spill there).
// hook: see NoTickHook (clik_rollout_lane.hpp).
template <const ShapeDesc& SD, bool RK, int WV, bool REGIMG, class HOOK>
__device__ __forceinline__ void pinv_rollout_static_body(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, int32_t* __restrict__ mode_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed,
    double* __restrict__ x, double* __restrict__ dx, const RollRec ra, HOOK& hook)
{
    // x / dx: virtual variables (path parameters, cart_on_track_1D...ipynb cells 56-60): integrated like the
    // robot variables, never clamped; unused (null) in skills without them.
    // Euler: the notebooks' loop.  Runge-Kutta: the controller as the right-hand side
    // (integration_methods.py:17-23): k1..k4 at t, t + dt/2, t + dt/2, t + dt, each stage clamped; tterms then
    // holds four time-slot records per tick.
    extern __shared__ double lds[];
    constexpr int N = SD.n;
    constexpr int NX = SD.n_x, NQ = N - NX;
    constexpr int NY = SD.n_y > 0 ? SD.n_y : 0;
    const WavePlace<WV> w(B);
    const int lane = w.lane;
    const long long b0 = w.b0;
    const int rows_valid = w.rows_valid;
    const bool valid = w.valid;
    double* zs = lds + StaticLayout<SD>::IMG_DOUBLES;
    if constexpr (WV > 1) zs += w.wave * lane_wave_doubles<SD, RK>(HOOK::LDS_DOUBLES);
    double* xs = zs + NQ * WAVE;
    double* ys = zs + N * WAVE;
    const Img<SD>* __restrict__ S = (const Img<SD>*)lds;
    if constexpr (WV == 1) {
        load_image<SD>(img_g, lds, lane);
    } else {
        // (the waves of a block share ONE copy of the image and load it together)
        typedef double d2 __attribute__((ext_vector_type(2)));
        const d2* src = (const d2*)img_g;
        d2* dst = (d2*)lds;
        for (int k = w.wave; k < StaticLayout<SD>::IMG_CHUNKS; k += WV) dst[k * WAVE + lane] = src[k * WAVE + lane];
    }
    {
        StagedRows<NQ, NX, NY> rows;
        rows.load(q, x, y, w);
        rows.to_lds(zs, xs, ys, lane);
    }
    hook.start(ys + (NY + (RK ? 2 * N : 0)) * WAVE, lane, valid, b0 + lane);
    __syncthreads();
    const int nts = S->n_tslots;
    const double* ysl = ys + lane * NY;
    double z[N];
    state_from_lds<NQ, NX>(zs, xs, lane, z);
    [[maybe_unused]] Img<SD> Sreg;
    if constexpr (REGIMG) {
        Sreg = *S;                                   // register copy, see pinv_solve_static_kernel
        __builtin_amdgcn_sched_barrier(0);
    }
    double vout[N];
    int acc_mode = -1;
#pragma unroll
    for (int j = 0; j < N; ++j) vout[j] = 0.0;
    RecClock clk;
    [[maybe_unused]] double ynext[NY > 0 ? NY : 1];
    clk.start(ra);
    // per-tick target: the NEXT tick's block is requested at the top of a tick (coalesced, as the first one was) ...
    auto request_rows = [&](const int tick) __attribute__((always_inline)) {
        if constexpr (NY > 0) {
            if (ra.y_stride != 0)
                stage_load<NY>(next_rows(y, ra, tick, n_ticks) + b0 * NY, NY, rows_valid, lane, ynext);
        }
    };
    // ... and replaces this tick's in LDS at its end, where the tick's record is stored too: every lane its own rows,
    // plain stores, nothing waits for them
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
        // (velocity feedback: behind the record and the reload, or the next record's rows would overwrite the fed entries)
        if constexpr (HOOK::FEEDS) hook.fed(vout, 0u, ys + lane * NY);
    };
    if constexpr (!RK) {
        const Img<SD>* __restrict__ Se = REGIMG ? &Sreg : S;       // (what the Euler tick reads)
#pragma unroll 1
        for (int tick = 0; tick < n_ticks; ++tick) {
            request_rows(tick);
            // the skill image is loop invariant: without this fence its LDS reads are all hoisted out of the
            // tick loop and the live constants spill (2.8 KB of scratch per lane)
            asm volatile("" ::: "memory");
            // time terms are read in place ([values | derivatives], 2*nts doubles per tick, never past them)
            const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + (size_t)tick * 2 * nts);
            hook.tick(S, tk, z, ysl, lane, tick, n_ticks, valid);
            pinv_tick_static<SD>(Se, tk, z, ysl, lane, valid, vout, acc_mode);
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
        double* z0s = ys + NY * WAVE;       // [N][64] state at the start of the tick, then [N][64] sum of w_i k_i
        double* kss = z0s + N * WAVE;
#pragma unroll 1
        for (int tick = 0; tick < n_ticks; ++tick) {
            request_rows(tick);
            int mode0 = -1;
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
#pragma unroll 1
            for (int st = 0; st < 4; ++st) {
                asm volatile("" ::: "memory");
                const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + ((size_t)tick * 4 + st) * 2 * nts);
                // (the image is read from LDS in place: with the register copy of the Euler loop the widest stacks
                // spill here)
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
    hook.finish(valid, n_ticks, b0 + lane);
    rows_out<NQ, NX>(z, q, x, w, zs, xs);
    rows_out<NQ, NX>(vout, dq, dx, w, zs, xs);
    if (mode_out != nullptr && valid) mode_out[b0 + lane] = acc_mode;
}

// ... recording its trajectory / reading one target per tick (RollRec, clik_device.hpp)
template <const ShapeDesc& SD, bool RK>
__global__ __launch_bounds__(WAVE) CLIK_ROLL_ATTR void pinv_rollout_static_rec_kernel(
    const void* __restrict__ img_g, double* __restrict__ q, const double* __restrict__ y,
    double* __restrict__ dq, int32_t* __restrict__ mode_out, const long long B,
    const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed,
    double* __restrict__ x, double* __restrict__ dx, const RollRec rec)
{
    FedHook<SD, NoTickHook> none;
    pinv_rollout_static_body<SD, RK, 1, true>(img_g, q, y, dq, mode_out, B, tterms, n_ticks, dt, max_speed, x, dx, rec, none);
}

// ... and its on-device rollout (see pinv_rollout_static_kernel): state in registers from tick to tick, the rows
// loaded once and stored once by the lane itself, no LDS (the Runge-Kutta bookkeeping lives in registers here: without
// the image there is room)
// ra: records of the trajectory and one target row per tick (RollRec, clik_device.hpp).
template <const ShapeDesc& SD, class IMGV, bool RK>
__device__ __forceinline__ void pinv_rollout_static_values_body(
    double* __restrict__ q, const double* __restrict__ y, double* __restrict__ dq, int32_t* __restrict__ mode_out,
    const long long B, const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed,
    const RollRec ra)
{
    static_assert(SD.n_x == 0, "value-specialised lane kernel: robot variables only");
    constexpr int N = SD.n;
    constexpr Img<SD> Sval = IMGV::value;
    constexpr int stages = RK ? 4 : 1;
    const int lane = threadIdx.x;
    const long long inst = (long long)blockIdx.x * WAVE + lane;
    const bool valid = inst < B;
    const long long row = valid ? inst : B - 1;
    const int nts = Sval.n_tslots;
    double z[N];
#pragma unroll
    for (int j = 0; j < N; ++j) z[j] = q[row * N + j];
    const double* ys = SD.n_y > 0 ? y + row * SD.n_y : nullptr;
    double vout[N];
    int acc_mode = -1;
#pragma unroll
    for (int j = 0; j < N; ++j) vout[j] = 0.0;
    // per-tick target (RollRec): the row lives in registers, and the NEXT tick's is requested at the top of a tick
    RecClock clk;
    [[maybe_unused]] double ycur[SD.n_y > 0 ? SD.n_y : 1], ynext[SD.n_y > 0 ? SD.n_y : 1];
    clk.start(ra);
    if constexpr (SD.n_y > 0) {
#pragma unroll
        for (int k = 0; k < SD.n_y; ++k) ycur[k] = ynext[k] = ys[k];
        ys = ycur;
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
        if constexpr (!RK) {
            const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + (size_t)tick * 2 * nts);
            pinv_tick_static<SD>(&Sval, tk, z, ys, lane, valid, vout, acc_mode);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                double d = vout[j];
                if (max_speed > 0.0) d = fmax(fmin(d, max_speed), -max_speed);
                vout[j] = d;
                z[j] = fma(d, dt, z[j]);
            }
        } else {
            double z0[N], ks[N];
            int mode0 = -1;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                z0[j] = z[j];
                ks[j] = 0.0;
            }
#pragma unroll 1
            for (int st = 0; st < stages; ++st) {
                const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tterms + ((size_t)tick * stages + st) * 2 * nts);
                pinv_tick_static<SD>(&Sval, tk, z, ys, lane, valid, vout, acc_mode);
                const double wgt = (st == 0 || st == 3) ? 1.0 : 2.0;
                const double cnext = (st == 2) ? dt : 0.5 * dt;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    double d = vout[j];
                    if (max_speed > 0.0) d = fmax(fmin(d, max_speed), -max_speed);
                    ks[j] = fma(wgt, d, ks[j]);
                    z[j] = fma(d, cnext, z0[j]);
                }
                mode0 = (st == 0) ? acc_mode : mode0;
            }
#pragma unroll
            for (int j = 0; j < N; ++j) {
                vout[j] = ks[j] * (1.0 / 6.0);
                z[j] = fma(vout[j], dt, z0[j]);
            }
            acc_mode = mode0;
        }
        if (clk.due(ra)) {
            if (valid) lane_record<N, 0>(ra, clk.r * B + inst, z, vout, acc_mode);
            ++clk.r;
        }
        if constexpr (SD.n_y > 0) {
#pragma unroll
            for (int k = 0; k < SD.n_y; ++k) ycur[k] = ynext[k];
        }
    }
    if (valid) {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            q[inst * N + j] = z[j];
            dq[inst * N + j] = vout[j];
        }
        if (mode_out != nullptr) mode_out[inst] = acc_mode;
    }
}

template <const ShapeDesc& SD, class IMGV, bool RK>
__global__ __launch_bounds__(WAVE) CLIK_OCC_ATTR void pinv_rollout_static_values_rec_kernel(
    double* __restrict__ q, const double* __restrict__ y, double* __restrict__ dq, int32_t* __restrict__ mode_out,
    const long long B, const double* __restrict__ tterms, const int n_ticks, const double dt, const double max_speed, const RollRec rec)
{
    pinv_rollout_static_values_body<SD, IMGV, RK>(q, y, dq, mode_out, B, tterms, n_ticks, dt, max_speed, rec);
}

// The recording / per-tick-target instantiations of the rollouts above (a.roll_rec, clik_pinv_rollout_batch_rec).  They
// live in translation units of their own (casclik_amd/jit.py: clik_jit_rollout_rec / clik_jit_value_rollout_rec), so the
// objects that serve ordinary rollouts do not carry them.
template <const ShapeDesc& SD, class IMGV>
inline hipError_t launch_rollout_values_rec(const LaunchArgs& a, const double* d_tterms, int n_ticks, double dt,
                                            double max_speed, long long B, double* q, const double* y, double* dq,
                                            int32_t* mode, hipStream_t stream)
{
    if constexpr (kVelFeedbackN > 0) return hipErrorNotSupported;       // (the lane kernels alone carry the feedback)
    if (a.roll_rec == nullptr) return hipErrorInvalidValue;
    const RollRec rr = *a.roll_rec;
    const bool rk = a.roll_stages == 4;
    switch (pinv_select(SD, a.policy, B, PinvOp::rollout)) {
    case PinvVariant::team4v:
        if constexpr (shape_team_ok(SD)) {
            const unsigned grid = (unsigned)((B + TEAM_INST - 1) / TEAM_INST);
            return launch_with_lds(rk ? pinv_rollout_static_team_rec_kernel<SD, IMGV, 4>
                                      : pinv_rollout_static_team_rec_kernel<SD, IMGV, 1>,
                                   grid, TEAM_WAVES * WAVE, team_rollout_lds_bytes<SD>(true), stream, nullptr, q, y, dq, mode,
                                   B, d_tterms, n_ticks, dt, max_speed, rr);
        }
        break;
    case PinvVariant::lanev:
        if constexpr (shape_value_lane_ok(SD)) {
            const unsigned grid = (unsigned)((B + WAVE - 1) / WAVE);
            return launch_with_lds(rk ? pinv_rollout_static_values_rec_kernel<SD, IMGV, true>
                                      : pinv_rollout_static_values_rec_kernel<SD, IMGV, false>,
                                   grid, WAVE, 0, stream, q, y, dq, mode, B, d_tterms, n_ticks, dt, max_speed, rr);
        }
        break;
    default:
        break;
    }
    return hipErrorNotSupported;
}

template <const ShapeDesc& SD>
inline hipError_t launch_rollout_static_rec(const LaunchArgs& a, const double* d_tterms, int n_ticks, double dt,
                                            double max_speed, long long B, double* q, const double* y, double* dq,
                                            int32_t* mode, hipStream_t stream)
{
    if (a.roll_rec == nullptr) return hipErrorInvalidValue;
    const RollRec rr = *a.roll_rec;
    const bool rk = a.roll_stages == 4;
    const unsigned grid = (unsigned)((B + WAVE - 1) / WAVE);
    // (a unit with the velocity feedback compiled in runs the lane kernel at every batch size: the team kernel has none)
    if constexpr (shape_team_ok(SD) && kVelFeedbackN == 0) {
        PinvPolicy p = a.policy;
        p.values_attached = false;  // (see launch_solve_static)
        if (pinv_select(SD, p, B, PinvOp::rollout) == PinvVariant::team4)
            return launch_with_lds(rk ? pinv_rollout_static_team_rec_kernel<SD, void, 4>
                                      : pinv_rollout_static_team_rec_kernel<SD, void, 1>,
                                   grid, TEAM_WAVES * WAVE, team_rollout_lds_bytes<SD>(), stream, a.dImg, q, y, dq, mode, B,
                                   d_tterms, n_ticks, dt, max_speed, rr);
    }
    const size_t shmem = static_lds_bytes<SD>(a.ny) + (rk ? (size_t)2 * SD.n * WAVE * sizeof(double) : 0);
    return launch_with_lds(rk ? pinv_rollout_static_rec_kernel<SD, true> : pinv_rollout_static_rec_kernel<SD, false>, grid,
                           WAVE, shmem, stream, a.dImg, q, y, dq, mode, B, d_tterms, n_ticks, dt, max_speed, a.roll_x,
                           a.roll_dx, rr);
}

// what a caller may ask about the lane kernels of a recording unit (clik_jit_rec_info, in the units built with the
// velocity feedback): 0 / 1 bytes of scratch per lane of the Euler / Runge-Kutta kernel as the loaded code object states
// them (-1: no device to ask), 2 / 3 LDS bytes of an Euler / Runge-Kutta block, 4 both fit the LDS of a CU, 5 + k the
// compiled-in feedback map (velocity_feedback_info(k))
template <const ShapeDesc& SD>
inline long long rollout_rec_info(int what)
{
    const size_t euler = static_lds_bytes<SD>(SD.n_y > 0 ? SD.n_y : 0), rk = euler + (size_t)2 * SD.n * WAVE * sizeof(double);
    if (what == 0) return kernel_scratch_bytes((const void*)pinv_rollout_static_rec_kernel<SD, false>);
    if (what == 1) return kernel_scratch_bytes((const void*)pinv_rollout_static_rec_kernel<SD, true>);
    return what == 2 ? (long long)euler : what == 3 ? (long long)rk : what == 4 ? (rk <= kLaneLdsCap ? 1 : 0)
         : what >= 5 ? velocity_feedback_info(what - 5) : -1;
}

}  // namespace clik
