// Constraint values on the device: e, J = d e / d (q, x) and d e / d t of every constraint of a skill at a whole
// trajectory of states - what the notebooks of the reference get from `cnstr.eval(t, q)` once per simulated tick - from
// the task evaluation the tick kernels run and discard (task_eval_s, clik_pinv_static.hpp): affine row table, norm_2
// groups and generated code (ExternTask<TI>) alike, the Velocity*Constraints included.
//
// A header and a translation unit of its own (jit.py, _MONITOR_TEMPLATE): it includes the shape-specialised headers
// read-only, and no header that holds another kernel names this one, so no other kernel's code depends on it.  Both
// controllers use it: the QP skill image begins with the Img<SD> this kernel reads (QpImg<SD> = Img<SD> + QpTail).
#pragma once
#include "clik_pinv_kernels.hpp"

namespace clik {

// Four waves per block, one per SIMD of a compute unit; a wave works on its own 64 rows and shares only the skill image
// with the other three.
constexpr int kMonitorWaves = 4;
constexpr int kMonitorBlock = kMonitorWaves * WAVE;
constexpr size_t kMonitorLdsCap = 160u * 1024u;        // LDS of one CU (gfx950)

// first output row of task ti / all rows of the skill (M_tot): the constraints' rows in skill order
constexpr int monitor_row_base(const ShapeDesc& sd, int ti)
{
    int r = 0;
    for (int i = 0; i < ti; ++i) r += sd.m[i];
    return r;
}
constexpr int monitor_rows(const ShapeDesc& sd) { return monitor_row_base(sd, sd.n_tasks); }

// LDS: [skill image | wave 0: zs (N slots) ys (n_y slots) | wave 1 ... ], slot = 64 doubles - per wave what the
// lane-per-instance kernels stage (StaticLayout<SD>), the image once per block.  The wave's region is reused for its
// [64][M_tot] block of e (then of e_t) on the way out, so it holds M_tot slots where that is more.
template <const ShapeDesc& SD>
struct MonitorLayout {
    static constexpr int N = SD.n, NX = SD.n_x, NQ = SD.n - SD.n_x, NY = SD.n_y;
    static constexpr int M_TOT = monitor_rows(SD);
#ifdef CLIK_MONITOR_LANE_STORES     // (measuring switch: every lane stores its own e / e_t rows, no staging)
    static constexpr int WAVE_SLOTS = N + NY;
#else
    static constexpr int WAVE_SLOTS = N + NY > M_TOT ? N + NY : M_TOT;
#endif
    static constexpr int WAVE_DOUBLES = WAVE_SLOTS * WAVE;
    static constexpr size_t LDS_BYTES =
        ((size_t)StaticLayout<SD>::IMG_DOUBLES + (size_t)kMonitorWaves * WAVE_DOUBLES) * sizeof(double);
};

// what a launch reads and writes (device pointers)
struct MonitorArgs {
    const void* img;            // skill image (Img<SD> first)
    const double* q;            // [R][B][n_q]
    const double* x;            // [R][B][n_x] or null (n_x == 0)
    const double* y;            // input_var rows of record r at y + r * y_stride: [B][n_y]
    long long y_stride;         // doubles between the records' input rows; 0: one [B][n_y] block for all records
    const double* tt;           // time-term table: row (r, b) reads 2 * n_tslots doubles at tt + r * tt_rec_stride +
    long long tt_rec_stride;    //   b * tt_inst_stride (0 / 0: one stamp; 2 nts / 0: one per record; 0 / 2 nts: one per
    long long tt_inst_stride;   //   instance); null for a skill without time slots
    long long B;                // instances per record
    unsigned blocks_per_rec;    // ceil(B / kMonitorBlock)
    double* e;                  // [R * B][M_tot]            (each may be null)
    double* J;                  // [R * B][M_tot][N]
    double* et;                 // [R * B][M_tot]
};

// task TI of the lane's row: evaluated, its J stored, and only then the next one - one task's J[M][N] is live at a
// time; e and e_t are kept (M_tot registers each) for the staged store at the end.  `valid` masks the stores of the
// lanes past the end of the record (their inputs are clamped copies of rows of the record).  One instantiation serves
// every combination of outputs, so e is the same bits with and without J (an e-only instantiation, in which J is dead
// code, measured no faster: profiles/constraint_values.md).
template <const ShapeDesc& SD, int TI>
__device__ __forceinline__ void monitor_task(const Img<SD>* __restrict__ S, const TickArgs& tk, const Kin<SD.n>& K,
                                             const double (&z)[SD.n], const double* ys, const int lane, const bool valid,
                                             double (&e_all)[monitor_rows(SD)], double (&et_all)[monitor_rows(SD)],
                                             double* __restrict__ J_row)
{
    if constexpr (TI < SD.n_tasks) {
        constexpr int N = SD.n;
        constexpr int M = SD.m[TI];
        constexpr int m0 = monitor_row_base(SD, TI);
        double e[M], J[M][N], Jt[M];
        task_eval_s<SD, TI>(S, tk, K, z, ys, lane, e, J, Jt);
#pragma unroll
        for (int i = 0; i < M; ++i) e_all[m0 + i] = e[i];
#pragma unroll
        for (int i = 0; i < M; ++i) et_all[m0 + i] = Jt[i];
        if (valid && J_row != nullptr) {
#pragma unroll
            for (int i = 0; i < M; ++i)
#pragma unroll
                for (int j = 0; j < N; ++j) J_row[(m0 + i) * N + j] = J[i][j];
        }
        // (the next task's arithmetic stays behind this one's: interleaved, the tasks of the headline skill need more
        // registers than two waves per SIMD have)
        __builtin_amdgcn_sched_barrier(0);
        monitor_task<SD, TI + 1>(S, tk, K, z, ys, lane, valid, e_all, et_all, J_row);
    }
}

// the wave's [64][M_tot] block of e or e_t: through its LDS region and out as whole lines (rows_from_lds), as the tick
// kernels store their velocities; every wave of the block calls this (barriers)
template <int MT>
__device__ __forceinline__ void monitor_rows_out(double* __restrict__ g, const double (&v)[MT], const int rows_valid,
                                                 const bool valid, double* region, const int lane)
{
#ifdef CLIK_MONITOR_LANE_STORES
    if (g != nullptr && valid) {
#pragma unroll
        for (int i = 0; i < MT; ++i) g[lane * MT + i] = v[i];
    }
#else
    __syncthreads();            // (the region's last readers are done)
    if (g != nullptr) {
#pragma unroll
        for (int i = 0; i < MT; ++i) region[lane * MT + i] = v[i];
    }
    __syncthreads();
    if (g != nullptr) rows_from_lds<MT>(g, rows_valid, region, lane);
#endif
}

// One lane per (record, instance) row.  A block belongs to ONE record (blockIdx.x / blocks_per_rec) and to 256
// consecutive instances of it, so the state, input and time-term rows of a wave are contiguous whatever the strides
// are, and no lane divides.  The state and input rows come in coalesced through the lane kernels' helpers (stage_load ->
// rows_to_lds), e and e_t go out the same way; every lane stores its own rows of J (profiles/constraint_values.md).
// A wave past the end of its record (the last block of a record only) works on the record's first rows again and
// stores nothing, so that every wave of a block meets every barrier.
template <const ShapeDesc& SD>
__global__ __launch_bounds__(kMonitorBlock) void constraint_values_kernel(const MonitorArgs a)
{
    extern __shared__ double lds[];
    using LY = MonitorLayout<SD>;
    constexpr int N = LY::N, NX = LY::NX, NQ = LY::NQ, NY = LY::NY, MT = LY::M_TOT;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const long long rec = (long long)(blockIdx.x / a.blocks_per_rec);
    const long long b_own = (long long)(blockIdx.x % a.blocks_per_rec) * kMonitorBlock + (long long)wave * WAVE;
    const bool idle = b_own >= a.B;
    const long long b0 = idle ? 0 : b_own;
    const long long left = a.B - b0;                    // (> 0)
    const int rows_load = left < WAVE ? (int)left : WAVE;
    const int rows_valid = idle ? 0 : rows_load;        // rows this wave stores
    const bool valid = lane < rows_valid;
    const long long row0 = rec * a.B + b0;              // first (record, instance) row of the wave

    double* zs = lds + StaticLayout<SD>::IMG_DOUBLES + wave * LY::WAVE_DOUBLES;    // [64][NQ] robot_var, [64][NX] virtual_var
    double* xs = zs + NQ * WAVE;
    double* ysl = zs + N * WAVE;
    // the image once per block, chunk k by wave k % 4; the wave's state and input rows in the same round trip
    typedef double d2 __attribute__((ext_vector_type(2)));
    {
        const d2* src = (const d2*)a.img;
        d2* dst = (d2*)lds;
        for (int k = wave; k < StaticLayout<SD>::IMG_CHUNKS; k += kMonitorWaves) dst[k * WAVE + lane] = src[k * WAVE + lane];
    }
    {
        double qv[NQ], xv[NX > 0 ? NX : 1], yv[NY > 0 ? NY : 1];
        stage_load<NQ>(a.q + row0 * NQ, NQ, rows_load, lane, qv);
        if constexpr (NX > 0) stage_load<NX>(a.x + row0 * NX, NX, rows_load, lane, xv);
        if constexpr (NY > 0) stage_load<NY>(a.y + rec * a.y_stride + b0 * NY, NY, rows_load, lane, yv);
        // (tail: the clamped loads filled the rows past rows_load with copies of the last element - finite values
        // whose results are never stored)
        rows_to_lds<NQ>(qv, zs, lane);
        if constexpr (NX > 0) rows_to_lds<NX>(xv, xs, lane);
        if constexpr (NY > 0) rows_to_lds<NY>(yv, ysl, lane);
    }
    __syncthreads();

    const Img<SD>* __restrict__ S = (const Img<SD>*)lds;
    double z[N];
    state_from_lds<NQ, NX>(zs, xs, lane, z);
    const double* ys = ysl + lane * NY;
    // the lane's time-slot record, read in place where the rows use it (as the per-instance-time tick kernels do); a
    // skill without time slots has no table and reads none: the reference then names memory that exists
    const long long inst = b0 + (lane < rows_load ? lane : rows_load - 1);
    const double* tt = a.tt != nullptr ? a.tt + rec * a.tt_rec_stride + inst * a.tt_inst_stride : lds;
    const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tt);

    Kin<N> K;
    if constexpr (SD.uses_fk != 0) {
        forward_kinematics_s<SD>(S, z, K);
        if constexpr (SD.quat_src != 0) orientation_feature_s<SD>(S, ys, lane, K);
    }
    double e_all[MT], et_all[MT];
    monitor_task<SD, 0>(S, tk, K, z, ys, lane, valid, e_all, et_all,
                              a.J != nullptr ? a.J + (row0 + lane) * (long long)(MT * N) : nullptr);
    monitor_rows_out<MT>(a.e != nullptr ? a.e + row0 * MT : nullptr, e_all, rows_valid, valid, zs, lane);
    monitor_rows_out<MT>(a.et != nullptr ? a.et + row0 * MT : nullptr, et_all, rows_valid, valid, zs, lane);
}

// R records of B instances each; see MonitorArgs for the pointers (blocks_per_rec is filled in here)
template <const ShapeDesc& SD>
hipError_t launch_constraint_values(MonitorArgs a, long long n_rec, hipStream_t stream)
{
    using LY = MonitorLayout<SD>;
    static_assert(LY::LDS_BYTES <= kMonitorLdsCap, "constraint_values_kernel needs more LDS than a CU has");
    if (n_rec <= 0 || a.B <= 0) return hipSuccess;
    const long long per_rec = (a.B + kMonitorBlock - 1) / kMonitorBlock;
    if (per_rec > 0x7fffffffLL || n_rec > 0x7fffffffLL / per_rec) return hipErrorInvalidValue;
    a.blocks_per_rec = (unsigned)per_rec;
    if (LY::LDS_BYTES > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)constraint_values_kernel<SD>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)LY::LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((constraint_values_kernel<SD>), dim3((unsigned)(per_rec * n_rec)), dim3(kMonitorBlock), LY::LDS_BYTES,
                       stream, a);
    return hipGetLastError();
}

}  // namespace clik
