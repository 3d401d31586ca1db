// Constraint summaries on the device: per instance and per constraint row, what a whole trajectory of states did to the
// task error e - its largest magnitude and where, its last value, its rms, how far and how often a SetConstraint was
// left, and from which record on it stayed within a tolerance - reduced over the record axis INSIDE the kernel that
// evaluates the constraints (task_eval_s, clik_pinv_static.hpp), so e [R][B][M_tot] never reaches memory.
//
// A header and a translation unit of its own (jit.py, _SUMMARY_TEMPLATE): it includes the shape-specialised headers
// read-only, and no header that holds another kernel names this one.  Both controllers use it: the QP skill image begins
// with the Img<SD> this kernel reads.
//
// Two phases.  One lane owns one instance and walks the records of one CHUNK of the record axis (summary_chunk_length: a
// function of R and B alone), its running values in registers; it leaves one partial per (chunk, row) in a work tensor.
// A small second kernel combines the partials of an instance in chunk order.  No atomics, no dependence on the device or
// on the other instances of the batch: the same bits on every call.
#pragma once
#include "clik_pinv_kernels.hpp"

namespace clik {

constexpr size_t kSummaryLdsCap = 160u * 1024u;        // LDS of one CU (gfx950)
// chunking of the record axis: enough blocks of 256 instances to put four waves on every SIMD of the largest part, and no
// chunk shorter than 8 records (a partial costs about as much memory as five records of e)
constexpr long long kSummaryTargetBlocks = 1024;
constexpr long long kSummaryMinChunk = 8;
constexpr long long kSummaryGroup = 256;               // instances per block of the register form
// running values of a lane, in dwords, up to which they stay in registers (two waves per SIMD with what the task
// evaluation needs); wider skills keep them in the wave's LDS region, one wave per block
constexpr int kSummaryRegDwords = 256;

constexpr long long summary_chunk_length(long long n_rec, long long B)
{
    const long long groups = B > 0 ? (B + kSummaryGroup - 1) / kSummaryGroup : 1;
    const long long want = groups < kSummaryTargetBlocks ? kSummaryTargetBlocks / groups : 1;      // chunks wanted
    const long long c = (n_rec + want - 1) / want;
    return c > kSummaryMinChunk ? c : kSummaryMinChunk;
}

constexpr int summary_row_base(const ShapeDesc& sd, int ti)
{
    int r = 0;
    for (int i = 0; i < ti; ++i) r += sd.m[i];
    return r;
}
constexpr int summary_rows(const ShapeDesc& sd) { return summary_row_base(sd, sd.n_tasks); }
// rows of SetConstraints before task ti / in all: their violation slots (the VelocitySetConstraints bound a velocity, not
// e: "other class")
constexpr int summary_set_base(const ShapeDesc& sd, int ti)
{
    int r = 0;
    for (int i = 0; i < ti; ++i)
        if (sd.cls[i] == CLIK_CLS_SET) r += sd.m[i];
    return r;
}
constexpr int summary_set_rows(const ShapeDesc& sd) { return summary_set_base(sd, sd.n_tasks); }

// Slots of a lane's running values and of a partial in the work tensor.  Doubles: [abs_max (MT) | sum of squares (MT) |
// viol_max (MS)]; int32: [abs_max_at (MT) | last unsettled record (MT) | viol_count (MS) | non-finite bits (BW words)].
// LDS: [skill image | tol (MT) | wave 0: zs (N slots) ys (n_y slots) (running values) | wave 1 ... ], slot = 64 doubles.
template <const ShapeDesc& SD>
struct SummaryLayout {
    static constexpr int N = SD.n, NX = SD.n_x, NQ = SD.n - SD.n_x, NY = SD.n_y;
    static constexpr int MT = summary_rows(SD), MS = summary_set_rows(SD);
    static constexpr int BW = (MT + 31) / 32;
    static constexpr int ND = 2 * MT + MS;
    static constexpr int NI = 2 * MT + MS;              // (+ BW words of bits, always in registers)
    static constexpr bool IN_LDS = 2 * ND + NI > kSummaryRegDwords;
    static constexpr int WAVES = IN_LDS ? 1 : 4;
    static constexpr int BLOCK = WAVES * WAVE;
    static constexpr int TOL_DOUBLES = (MT + 1) & ~1;
    static constexpr int ACC_DOUBLES = IN_LDS ? ND * WAVE + NI * (WAVE / 2) : 0;
    static constexpr int WAVE_DOUBLES = (N + NY) * WAVE + ACC_DOUBLES;
    static constexpr size_t LDS_BYTES =
        ((size_t)StaticLayout<SD>::IMG_DOUBLES + TOL_DOUBLES + (size_t)WAVES * WAVE_DOUBLES) * sizeof(double);
    static constexpr bool FITS = LDS_BYTES <= kSummaryLdsCap;
};

// doubles / int32 of the work tensor of a launch (the partials of every chunk, then `last` [MT][B])
template <const ShapeDesc& SD>
constexpr size_t summary_work_bytes(long long n_chunks, long long B)
{
    using LY = SummaryLayout<SD>;
    return ((size_t)n_chunks * LY::ND + LY::MT) * (size_t)B * sizeof(double)
           + (size_t)n_chunks * (LY::NI + LY::BW) * (size_t)B * sizeof(int32_t);
}

// what a launch reads and writes (device pointers)
struct SummaryArgs {
    const void* img;            // skill image (Img<SD> first)
    const double* q;            // [R][B][n_q]
    const double* x;            // [R][B][n_x] or null (n_x == 0)
    const double* y;            // input_var rows of record r at y + r * y_stride: [B][n_y]
    long long y_stride;         // 0: one [B][n_y] block for all records
    const double* tt;           // time-term table, row (r, b) at tt + r * tt_rec_stride + b * tt_inst_stride; null: no slots
    long long tt_rec_stride;
    long long tt_inst_stride;
    long long B;                // instances per record
    long long R;                // records
    long long chunk;            // records per chunk
    unsigned groups;            // blocks per chunk: ceil(B / BLOCK)
    const double* tol;          // [MT] or null (no settled_at)
    double* work_d;             // [n_chunks][ND][B], then last [MT][B]
    int32_t* work_i;            // [n_chunks][NI + BW][B]
};

// the lane's running values: registers (every index a constant expression) or its column of the wave's LDS region
template <int ND, int NI, bool IN_LDS>
struct SummaryAcc {
    double d[IN_LDS ? 1 : ND];
    int32_t i[IN_LDS ? 1 : NI];
    double* ld;                 // (IN_LDS) the lane's element of slot 0; slot k at ld[k * WAVE]
    int32_t* li;
    template <int K>
    __device__ __forceinline__ double getd() const
    {
        if constexpr (IN_LDS) return ld[K * WAVE];
        else return d[K];
    }
    template <int K>
    __device__ __forceinline__ void setd(const double v)
    {
        if constexpr (IN_LDS) ld[K * WAVE] = v;
        else d[K] = v;
    }
    template <int K>
    __device__ __forceinline__ int32_t geti() const
    {
        if constexpr (IN_LDS) return li[K * WAVE];
        else return i[K];
    }
    template <int K>
    __device__ __forceinline__ void seti(const int32_t v)
    {
        if constexpr (IN_LDS) li[K * WAVE] = v;
        else i[K] = v;
    }
};

// non-finite as BITS of a word the compiler knows nothing about: device code is built with -fno-honor-nans, under which
// a floating-point test for NaN folds away - and so does a test of the exponent bits of a value it knows to be the
// result of arithmetic (it becomes a class test that leaves NaN out); pin_arrived makes the high word opaque
__device__ __forceinline__ unsigned summary_nonfinite(const double v)
{
    unsigned hi = (unsigned)__double2hiint(v);
    pin_arrived(hi);
    return (hi & 0x7ff00000u) == 0x7ff00000u ? 1u : 0u;
}

// task TI of the lane's instance at record `rec`: evaluated as the constraint-value kernel evaluates it, then folded into
// the running values, and only then the next task - one task's e is live at a time.  `last`: this is record R - 1.
template <const ShapeDesc& SD, int TI, class ACC>
__device__ __forceinline__ void summary_task(const Img<SD>* __restrict__ S, const TickArgs& tk, const Kin<SD.n>& K,
                                             const double (&z)[SD.n], const double* ys, const double* tol, const int lane,
                                             const int rec, ACC& acc, unsigned (&bad)[SummaryLayout<SD>::BW],
                                             const bool last, const bool valid, double* __restrict__ last_out,
                                             const long long B)
{
    if constexpr (TI < SD.n_tasks) {
        using LY = SummaryLayout<SD>;
        constexpr int N = SD.n, M = SD.m[TI], MT = LY::MT;
        constexpr int m0 = summary_row_base(SD, TI);
        constexpr bool SET = SD.cls[TI] == CLIK_CLS_SET;
        constexpr int s0 = summary_set_base(SD, TI);
        double e[M], J[M][N], Jt[M];
        task_eval_s<SD, TI>(S, tk, K, z, ys, lane, e, J, Jt);
        // J and d e / d t stay ALIVE (an empty statement reads them): with them dead the compiler contracts the products
        // that e shares with its Jacobian differently, and e then differs from the constraint-value kernel's by a unit in
        // the last place - the summary must be the reduction of exactly those values
#pragma unroll
        for (int i = 0; i < M; ++i) {
            asm volatile("" ::"v"(Jt[i]));
#pragma unroll
            for (int j = 0; j < N; ++j) asm volatile("" ::"v"(J[i][j]));
        }
        // the set bounds as the tick kernels take them (task_consts): image values, or the task's slice of the
        // attributes evaluated at this record's (t, q, x, y)
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
            const double a = fabs(ev);
            if (a > acc.template getd<row>()) {           // (strictly: the first record of equal maxima stays)
                acc.template setd<row>(a);
                acc.template seti<row>(rec);
            }
            acc.template setd<MT + row>(fma(ev, ev, acc.template getd<MT + row>()));
            double dist = a;
            if constexpr (SET) {
                const double v = fmax(fmax(lo[i] - ev, ev - hi[i]), 0.0);
                acc.template setd<2 * MT + s0 + i>(fmax(acc.template getd<2 * MT + s0 + i>(), v));
                acc.template seti<2 * MT + s0 + i>(acc.template geti<2 * MT + s0 + i>() + (v > 0.0 ? 1 : 0));
                dist = v;
            }
            if (dist > tol[row]) acc.template seti<MT + row>(rec);
            bad[row / 32] |= summary_nonfinite(ev) << (row % 32);
            if (last && valid) last_out[(long long)row * B] = ev;
        });
        // (the next task's arithmetic stays behind this one's, as in the constraint-value kernel)
        __builtin_amdgcn_sched_barrier(0);
        summary_task<SD, TI + 1>(S, tk, K, z, ys, tol, lane, rec, acc, bad, last, valid, last_out, B);
    }
}

// Phase one.  A block belongs to ONE chunk of records (blockIdx.x / groups) and to BLOCK consecutive instances; a wave
// works on its own 64 instances and shares only the skill image and the tolerances with the others.  Record by record
// the wave's state and input rows come in coalesced (stage_load -> rows_to_lds), the next record's while this one is
// evaluated.  Every wave of a block walks the same records, so all of them meet every barrier; a wave past the end of
// the batch works on the first rows again and stores nothing.
template <const ShapeDesc& SD>
__global__ __launch_bounds__(SummaryLayout<SD>::BLOCK) void constraint_summary_kernel(const SummaryArgs a)
{
    extern __shared__ double lds[];
    using LY = SummaryLayout<SD>;
    constexpr int N = LY::N, NX = LY::NX, NQ = LY::NQ, NY = LY::NY, MT = LY::MT, MS = LY::MS;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const long long chunk = (long long)(blockIdx.x / a.groups);
    const long long b_own = (long long)(blockIdx.x % a.groups) * LY::BLOCK + (long long)wave * WAVE;
    const bool idle = b_own >= a.B;
    const long long b0 = idle ? 0 : b_own;
    const long long left = a.B - b0;                    // (> 0)
    const int rows_load = left < WAVE ? (int)left : WAVE;
    const bool valid = !idle && lane < rows_load;
    const long long r0 = chunk * a.chunk;
    const long long r1 = r0 + a.chunk < a.R ? r0 + a.chunk : a.R;       // (r0 < R: the launch makes no empty chunk)

    double* tol = lds + StaticLayout<SD>::IMG_DOUBLES;
    double* zs = tol + LY::TOL_DOUBLES + wave * LY::WAVE_DOUBLES;       // [64][NQ] robot_var, [64][NX] virtual_var
    double* xs = zs + NQ * WAVE;
    double* ysl = zs + N * WAVE;
    typedef double d2 __attribute__((ext_vector_type(2)));
    {
        const d2* src = (const d2*)a.img;
        d2* dst = (d2*)lds;
        for (int k = wave; k < StaticLayout<SD>::IMG_CHUNKS; k += LY::WAVES) dst[k * WAVE + lane] = src[k * WAVE + lane];
        for (int k = threadIdx.x; k < MT; k += LY::BLOCK) tol[k] = a.tol != nullptr ? a.tol[k] : 0.0;
    }
    SummaryAcc<LY::ND, LY::NI, LY::IN_LDS> acc;
    acc.ld = ysl + NY * WAVE + lane;
    acc.li = (int32_t*)(ysl + NY * WAVE + LY::ND * WAVE) + lane;
    static_for<0, MT>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        acc.template setd<i>(-1.0);                     // (below every |e|: the chunk's first record sets abs_max_at)
        acc.template setd<MT + i>(0.0);
        acc.template seti<i>((int32_t)r0);
        acc.template seti<MT + i>(-1);
    });
    static_for<0, MS>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = decltype(ic)::value;
        acc.template setd<2 * MT + i>(0.0);
        acc.template seti<2 * MT + i>(0);
    });
    unsigned bad[LY::BW];
#pragma unroll
    for (int k = 0; k < LY::BW; ++k) bad[k] = 0u;

    const Img<SD>* __restrict__ S = (const Img<SD>*)lds;
    const long long inst = b0 + (lane < rows_load ? lane : rows_load - 1);
    double* last_out = a.work_d + ((size_t)((a.R + a.chunk - 1) / a.chunk) * LY::ND) * (size_t)a.B + (valid ? b0 + lane : 0);
    double qv[NQ], xv[NX > 0 ? NX : 1], yv[NY > 0 ? NY : 1];
    auto request = [&](const long long rec) __attribute__((always_inline)) {
        const long long row0 = rec * a.B + b0;
        stage_load<NQ>(a.q + row0 * NQ, NQ, rows_load, lane, qv);
        if constexpr (NX > 0) stage_load<NX>(a.x + row0 * NX, NX, rows_load, lane, xv);
        if constexpr (NY > 0) {
            if (rec == r0 || a.y_stride != 0) stage_load<NY>(a.y + rec * a.y_stride + b0 * NY, NY, rows_load, lane, yv);
        }
    };
    request(r0);
#pragma unroll 1
    for (long long rec = r0; rec < r1; ++rec) {
        __syncthreads();            // (the previous record's readers are done; the first time: nothing to wait for)
        rows_to_lds<NQ>(qv, zs, lane);
        if constexpr (NX > 0) rows_to_lds<NX>(xv, xs, lane);
        if constexpr (NY > 0) rows_to_lds<NY>(yv, ysl, lane);
        __syncthreads();            // (also: the image and the tolerances are in place)
        if (rec + 1 < r1) request(rec + 1);
        double z[N];
        state_from_lds<NQ, NX>(zs, xs, lane, z);
        const double* ys = ysl + lane * NY;
        // the lane's time-slot record, read in place where the rows use it; a skill without time slots reads none
        const double* tt = a.tt != nullptr ? a.tt + rec * a.tt_rec_stride + inst * a.tt_inst_stride : lds;
        const TickArgs& tk = *reinterpret_cast<const TickArgs*>(tt);
        Kin<N> K;
        if constexpr (SD.uses_fk != 0) {
            forward_kinematics_s<SD>(S, z, K);
            if constexpr (SD.quat_src != 0) orientation_feature_s<SD>(S, ys, lane, K);
        }
        summary_task<SD, 0>(S, tk, K, z, ys, tol, lane, (int)rec, acc, bad, rec == a.R - 1, valid, last_out, a.B);
    }
    if (valid) {
        // the chunk's partial: slot by slot, the wave's 64 instances side by side (whole lines)
        double* wd = a.work_d + (size_t)chunk * LY::ND * (size_t)a.B + (b0 + lane);
        int32_t* wi = a.work_i + (size_t)chunk * (LY::NI + LY::BW) * (size_t)a.B + (b0 + lane);
        static_for<0, LY::ND>([&](auto kc) __attribute__((always_inline)) {
            constexpr int k = decltype(kc)::value;
            wd[(size_t)k * a.B] = acc.template getd<k>();
        });
        static_for<0, LY::NI>([&](auto kc) __attribute__((always_inline)) {
            constexpr int k = decltype(kc)::value;
            wi[(size_t)k * a.B] = acc.template geti<k>();
        });
#pragma unroll
        for (int k = 0; k < LY::BW; ++k) wi[(size_t)(LY::NI + k) * a.B] = (int32_t)bad[k];
    }
}

// what phase two writes: [B][MT] each (settled_at may be null)
struct SummaryOut {
    double* abs_max;
    int32_t* abs_max_at;
    double* last;
    double* rms;
    double* viol_max;
    int32_t* viol_count;
    int32_t* settled_at;
};

// violation slot of every row (-1: not a SetConstraint's), for the run-time row index of phase two
template <const ShapeDesc& SD>
struct SummarySetSlots {
    int v[summary_rows(SD) > 0 ? summary_rows(SD) : 1];
    constexpr SummarySetSlots() : v{}
    {
        for (int ti = 0; ti < SD.n_tasks; ++ti)
            for (int i = 0; i < SD.m[ti]; ++i)
                v[summary_row_base(SD, ti) + i] = SD.cls[ti] == CLIK_CLS_SET ? summary_set_base(SD, ti) + i : -1;
    }
};

// Phase two: one thread per (row, instance), the instances side by side, so the partials are read as whole lines.  In
// chunk order: abs_max / viol_max the maximum (the lowest record among equal maxima: chunks hold ascending records and
// only a strictly larger value replaces), the sums of squares added, the counts added, settled_at from the last chunk
// that holds an unsettled record.  A row that was non-finite at any record: NaN by bits (nan_or) in the float outputs.
template <const ShapeDesc& SD>
__global__ __launch_bounds__(256) void constraint_summary_combine_kernel(const SummaryArgs a, const SummaryOut o,
                                                                         const long long n_chunks)
{
    using LY = SummaryLayout<SD>;
    constexpr int MT = LY::MT;
    constexpr SummarySetSlots<SD> slots{};
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)MT * a.B) return;
    const int row = (int)(idx / a.B);
    const long long b = idx - (long long)row * a.B;
    const int slot = slots.v[row];
    double amax = -1.0, ssq = 0.0, vmax = 0.0;
    int32_t at = 0, vcount = 0, uns = -1;
    unsigned bad = 0u;
    for (long long k = 0; k < n_chunks; ++k) {
        const double* wd = a.work_d + (size_t)k * LY::ND * (size_t)a.B + b;
        const int32_t* wi = a.work_i + (size_t)k * (LY::NI + LY::BW) * (size_t)a.B + b;
        const double pa = wd[(size_t)row * a.B];
        if (pa > amax) {
            amax = pa;
            at = wi[(size_t)row * a.B];
        }
        ssq += wd[(size_t)(MT + row) * a.B];
        const int32_t pu = wi[(size_t)(MT + row) * a.B];
        uns = pu > uns ? pu : uns;
        if (slot >= 0) {
            vmax = fmax(vmax, wd[(size_t)(2 * MT + slot) * a.B]);
            vcount += wi[(size_t)(2 * MT + slot) * a.B];
        }
        bad |= ((unsigned)wi[(size_t)(LY::NI + row / 32) * a.B] >> (row % 32)) & 1u;
    }
    const unsigned bad_hi = bad != 0u ? 0x7ff80000u : 0u;
    const double last = a.work_d[(size_t)n_chunks * LY::ND * (size_t)a.B + (size_t)row * a.B + b];
    const size_t out = (size_t)b * MT + row;
    o.abs_max[out] = nan_or(amax, bad_hi);
    o.abs_max_at[out] = at;
    o.last[out] = nan_or(last, bad_hi);
    o.rms[out] = nan_or(sqrt(ssq / (double)a.R), bad_hi);
    o.viol_max[out] = nan_or(vmax, bad_hi);
    o.viol_count[out] = vcount;
    if (o.settled_at != nullptr) o.settled_at[out] = uns + 1;
}

// what a caller may ask about the instantiation (clik_jit_summary_info): 0 rows, 1 SetConstraint rows, 2 LDS bytes of a
// block, 3 fits the LDS of a CU, 4 running values in LDS
template <const ShapeDesc& SD>
constexpr long long summary_info(int what)
{
    using LY = SummaryLayout<SD>;
    return what == 0 ? LY::MT : what == 1 ? LY::MS : what == 2 ? (long long)LY::LDS_BYTES : what == 3 ? (LY::FITS ? 1 : 0)
         : what == 4 ? (LY::IN_LDS ? 1 : 0) : -1;
}

// R records of B instances each; `work` holds summary_work_bytes<SD>(ceil(R / chunk), B) bytes (checked)
template <const ShapeDesc& SD>
hipError_t launch_constraint_summary(SummaryArgs a, void* work, size_t work_bytes, const SummaryOut o, hipStream_t stream)
{
    using LY = SummaryLayout<SD>;
    if constexpr (!LY::FITS) {
        return hipErrorInvalidValue;        // (refused at attach time with the figure: jit.attach_summary)
    } else {
        if (a.R <= 0 || a.B <= 0) return hipSuccess;
        if (a.R > 0x7fffffffLL) return hipErrorInvalidValue;
        a.chunk = summary_chunk_length(a.R, a.B);
        const long long n_chunks = (a.R + a.chunk - 1) / a.chunk;
        const long long groups = (a.B + LY::BLOCK - 1) / LY::BLOCK;
        if (groups > 0x7fffffffLL || n_chunks > 0x7fffffffLL / groups) return hipErrorInvalidValue;
        if (work == nullptr || work_bytes < summary_work_bytes<SD>(n_chunks, a.B)) return hipErrorInvalidValue;
        a.groups = (unsigned)groups;
        a.work_d = (double*)work;
        a.work_i = (int32_t*)(a.work_d + ((size_t)n_chunks * LY::ND + LY::MT) * (size_t)a.B);
        if (LY::LDS_BYTES > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void*)constraint_summary_kernel<SD>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)LY::LDS_BYTES);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL((constraint_summary_kernel<SD>), dim3((unsigned)(groups * n_chunks)), dim3(LY::BLOCK),
                           LY::LDS_BYTES, stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        const long long threads = (long long)LY::MT * a.B;
        if (threads > 0x7fffffffLL * 256LL) return hipErrorInvalidValue;
        hipLaunchKernelGGL((constraint_summary_combine_kernel<SD>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                           stream, a, o, n_chunks);
        return hipGetLastError();
    }
}

}  // namespace clik
