// A user function on the device: the outputs of a `cs.Function` - a tool path, a tool frame, a manipulability curve,
// whatever the notebooks of the reference compute once per simulated tick with a compiled CasADi Function - at every
// row of a batch [B] or of a recorded trajectory [R][B] in one launch, from the expression's own generated code
// (casclik_amd/codegen.py, emit_function: `struct BatchFn`).
//
// A header and a translation unit of its own (jit.py, _FUNCTION_TEMPLATE): it includes clik_pinv_kernels.hpp read-only
// for the staging helpers (stage_load, rows_to_lds, rows_from_lds) and sincos_joint, and no header that holds another
// kernel names this one, so no other kernel's code depends on it.  There is no skill, no image and no handle: the
// generated library's entry point is the interface.
#pragma once
#include "clik_pinv_kernels.hpp"

namespace clik {

// Four waves per block, one per SIMD of a compute unit; a wave works on its own 64 rows.
constexpr int kFunctionWaves = 4;
constexpr int kFunctionBlock = kFunctionWaves * WAVE;
constexpr size_t kFunctionLdsCap = 160u * 1024u;        // LDS of one CU (gfx950)

// LDS: [wave 0: S slots | wave 1 ... ], slot = 64 doubles.  On the way in the wave's region holds the [64][w] blocks of
// ALL inputs side by side (input k at slot in_off[k]: they are in flight together); on the way out it is reused for
// one output's [64][w] block after the other.  S = max(sum of input widths, widest output), at least 1.
template <class FN>
struct FunctionLayout {
    static constexpr int widest_out()
    {
        int m = 1;
        for (int k = 0; k < FN::n_out; ++k) m = FN::out_w[k] > m ? FN::out_w[k] : m;
        return m;
    }
    static constexpr int WAVE_SLOTS = FN::n_x > widest_out() ? FN::n_x : widest_out();
    static constexpr int WAVE_DOUBLES = WAVE_SLOTS * WAVE;
    static constexpr size_t LDS_BYTES = (size_t)kFunctionWaves * WAVE_DOUBLES * sizeof(double);
};

// What a launch reads and writes (device pointers).  Row (r, b) of input k is the in_w[k] doubles at
// in[k] + r * rec_stride[k] + b * inst_stride[k]: strides 0 / 0 one value for all rows, w / 0 one per record, 0 / w one per
// instance, B w / w the full trajectory.  Output k is dense: [R * B][out_w[k]].
template <int NI, int NO>
struct FunctionArgs {
    const double* in[NI];
    long long rec_stride[NI];
    long long inst_stride[NI];
    double* out[NO];
    long long B;                // instances per record
    unsigned blocks_per_rec;    // ceil(B / kFunctionBlock)
};

template <int W>
__device__ __forceinline__ double (&function_slice(double* p))[W]
{
    return *reinterpret_cast<double (*)[W]>(p);
}

// input K and the ones after it: the dense ones (inst_stride == width: the wave's 64 rows are one contiguous block) are
// loaded coalesced into `sv`, the others are read where they are used (function_gather)
template <class FN, int K>
__device__ __forceinline__ void function_stage_load(const FunctionArgs<FN::n_in, FN::n_out>& a, const long long rec,
                                                    const long long b0, const int rows_load, const int lane,
                                                    double (&sv)[FN::n_x])
{
    if constexpr (K < FN::n_in) {
        constexpr int W = FN::in_w[K], OFF = FN::in_off[K];
        if (a.inst_stride[K] == W)
            stage_load<W>(a.in[K] + rec * a.rec_stride[K] + b0 * W, W, rows_load, lane, function_slice<W>(sv + OFF));
        function_stage_load<FN, K + 1>(a, rec, b0, rows_load, lane, sv);
    }
}
template <class FN, int K>
__device__ __forceinline__ void function_stage_store(const FunctionArgs<FN::n_in, FN::n_out>& a, double* region,
                                                     const int lane, double (&sv)[FN::n_x])
{
    if constexpr (K < FN::n_in) {
        constexpr int W = FN::in_w[K], OFF = FN::in_off[K];
        if (a.inst_stride[K] == W) rows_to_lds<W>(function_slice<W>(sv + OFF), region + OFF * WAVE, lane);
        function_stage_store<FN, K + 1>(a, region, lane, sv);
    }
}
// the lane's rows: staged ones from LDS, a shared or per-record one from its one address for the whole block (uniform:
// the compiler reads it once per wave), anything else per lane (`inst` is clamped to the record)
template <class FN, int K>
__device__ __forceinline__ void function_gather(const FunctionArgs<FN::n_in, FN::n_out>& a, const double* region,
                                                const long long rec, const long long inst, const int lane,
                                                double (&x)[FN::n_x])
{
    if constexpr (K < FN::n_in) {
        constexpr int W = FN::in_w[K], OFF = FN::in_off[K];
        if (a.inst_stride[K] == W) {
#pragma unroll
            for (int i = 0; i < W; ++i) x[OFF + i] = region[OFF * WAVE + lane * W + i];
        } else if (a.inst_stride[K] == 0) {
            const double* __restrict__ p = a.in[K] + rec * a.rec_stride[K];
#pragma unroll
            for (int i = 0; i < W; ++i) x[OFF + i] = p[i];
        } else {
            const double* __restrict__ p = a.in[K] + rec * a.rec_stride[K] + inst * a.inst_stride[K];
#pragma unroll
            for (int i = 0; i < W; ++i) x[OFF + i] = p[i];
        }
        function_gather<FN, K + 1>(a, region, rec, inst, lane, x);
    }
}

// output K and the ones after it, one after the other: the wave's [64][W] block through its LDS region and out as whole
// lines (rows_from_lds), as the tick kernels store their velocities; every wave of the block takes part (barriers).  A
// one-column output is whole lines as the lanes hold it.
template <class FN, int K>
__device__ __forceinline__ void function_rows_out(const FunctionArgs<FN::n_in, FN::n_out>& a, const double (&y)[FN::n_y],
                                                  const long long row0, const int rows_valid, double* region,
                                                  const int lane)
{
    if constexpr (K < FN::n_out) {
        constexpr int W = FN::out_w[K], OFF = FN::out_off[K];
        if constexpr (W == 1) {
            if (lane < rows_valid) a.out[K][row0 + lane] = y[OFF];
        } else {
            __syncthreads();            // (the region's last readers are done)
#pragma unroll
            for (int i = 0; i < W; ++i) region[lane * W + i] = y[OFF + i];
            __syncthreads();
            rows_from_lds<W>(a.out[K] + row0 * W, rows_valid, region, lane);
        }
        function_rows_out<FN, K + 1>(a, y, row0, rows_valid, region, lane);
    }
}

// One lane per (record, instance) row.  A block belongs to ONE record (blockIdx.x / blocks_per_rec) and to 256
// consecutive instances of it, so no lane divides and the per-record inputs are uniform over the block.  A wave past
// the end of its record (the last block of a record only) works on the record's first rows again and stores nothing,
// so that every wave of a block meets every barrier.  The lanes of a wave's tail compute on filler whose results are
// never stored: for a staged input stage_load clamps the ELEMENT index, so such a lane's row in LDS is the block's last
// element repeated (or straddles the last row), for an input read per lane it is the record's last row - finite where
// the input is, either way.
template <class FN>
__global__ __launch_bounds__(kFunctionBlock) void function_batch_kernel(const FunctionArgs<FN::n_in, FN::n_out> a)
{
    extern __shared__ double lds[];
    using LY = FunctionLayout<FN>;
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const long long rec = (long long)(blockIdx.x / a.blocks_per_rec);
    const long long b_own = (long long)(blockIdx.x % a.blocks_per_rec) * kFunctionBlock + (long long)wave * WAVE;
    const bool idle = b_own >= a.B;
    const long long b0 = idle ? 0 : b_own;
    const long long left = a.B - b0;                    // (> 0)
    const int rows_load = left < WAVE ? (int)left : WAVE;
    const int rows_valid = idle ? 0 : rows_load;        // rows this wave stores
    const long long row0 = rec * a.B + b0;              // first (record, instance) row of the wave
    double* region = lds + wave * LY::WAVE_DOUBLES;

    double x[FN::n_x], y[FN::n_y];
    {
        // every dense input in flight before the first LDS write: one memory round trip
        double sv[FN::n_x];
        function_stage_load<FN, 0>(a, rec, b0, rows_load, lane, sv);
        function_stage_store<FN, 0>(a, region, lane, sv);
    }
    __syncthreads();
    function_gather<FN, 0>(a, region, rec, b0 + (lane < rows_load ? lane : rows_load - 1), lane, x);
    FN::eval(x, y);
    function_rows_out<FN, 0>(a, y, row0, rows_valid, region, lane);
}

// R records of B instances each; `in`, `rec_stride`, `inst_stride` (n_in entries) and `out` (n_out entries) are HOST
// arrays of device pointers / strides in doubles (see FunctionArgs)
template <class FN>
hipError_t launch_function_batch(long long n_rec, long long B, const double* const* in, const long long* rec_stride,
                                 const long long* inst_stride, double* const* out, hipStream_t stream)
{
    using LY = FunctionLayout<FN>;
    static_assert(LY::LDS_BYTES <= kFunctionLdsCap, "function_batch_kernel needs more LDS than a CU has");
    if (n_rec < 0 || B < 0 || in == nullptr || rec_stride == nullptr || inst_stride == nullptr || out == nullptr)
        return hipErrorInvalidValue;
    if (n_rec == 0 || B == 0) return hipSuccess;
    FunctionArgs<FN::n_in, FN::n_out> a;
    for (int k = 0; k < FN::n_in; ++k) {
        if (in[k] == nullptr || rec_stride[k] < 0 || inst_stride[k] < 0) return hipErrorInvalidValue;
        a.in[k] = in[k];
        a.rec_stride[k] = rec_stride[k];
        a.inst_stride[k] = inst_stride[k];
    }
    for (int k = 0; k < FN::n_out; ++k) {
        if (out[k] == nullptr) return hipErrorInvalidValue;
        a.out[k] = out[k];
    }
    const long long per_rec = (B + kFunctionBlock - 1) / kFunctionBlock;
    if (per_rec > 0x7fffffffLL || n_rec > 0x7fffffffLL / per_rec) return hipErrorInvalidValue;
    a.B = B;
    a.blocks_per_rec = (unsigned)per_rec;
    if (LY::LDS_BYTES > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)function_batch_kernel<FN>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)LY::LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((function_batch_kernel<FN>), dim3((unsigned)(per_rec * n_rec)), dim3(kFunctionBlock), LY::LDS_BYTES,
                       stream, a);
    return hipGetLastError();
}

// what the generated library tells its loader: 0 n_in, 1 n_out, 2 in_w[k], 3 out_w[k], 4 LDS bytes of a block; -1
// otherwise
template <class FN>
int function_info(int what, int k)
{
    switch (what) {
    case 0: return FN::n_in;
    case 1: return FN::n_out;
    case 2: return k >= 0 && k < FN::n_in ? FN::in_w[k] : -1;
    case 3: return k >= 0 && k < FN::n_out ? FN::out_w[k] : -1;
    case 4: return (int)FunctionLayout<FN>::LDS_BYTES;
    default: return -1;
    }
}

// bytes of scratch (private segment) per lane of the compiled kernel, or -1 when the runtime cannot say (no device)
template <class FN>
int function_scratch_bytes()
{
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, (const void*)function_batch_kernel<FN>) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return (int)attr.localSizeBytes;
}

}  // namespace clik
