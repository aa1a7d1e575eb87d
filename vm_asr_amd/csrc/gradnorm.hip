// gradnorm.hip — global L2 norm, clip coefficient and non-finite flag of one optimiser's gradients, gfx950.
//
// Reference: the reference trains under a GradScaler (trainer/trainer.py:106-107, 428-438), whose step() leaves weights and Adam moments
// alone when a gradient holds an inf or a NaN; torch.nn.utils.clip_grad_norm_ gives the coefficient's formula.  Here both are one stream
// over the gradient views (grad_sync.FlatGrads) that ends in a few device floats the guarded AdamW launch (csrc/adamw.hip) reads: no host
// read anywhere, so the pair sits in the captured optimiser graph.
//
// Two launches, no float atomics, every sum in a fixed order -> the values are bit-identical from call to call on the same data:
//   pass 1  one workgroup per 4096-element chunk of a segment (the chunk table of adamw.hip: (segment, chunk) pairs built by the host).
//           Each thread accumulates x*x of its 16 (17) elements in fp64, the 64 lanes of a wave add up in a 6-level butterfly, the four
//           wave sums in a 2-level tree through LDS behind ONE barrier: one fp64 partial per chunk, plus one flag "some ELEMENT of this chunk is inf / NaN" (exponent all ones: decided per element,
//           not from the sum).  fp64, not fp32: the square of a gradient element leaves fp32's range below 1e-19 (subnormal: a
//           one-element segment of 1e-20 would lose its norm's last 3 digits) and above 1e19, the norm itself does not; the pass is a
//           4 B/element stream, the convert + fp64 fma per element hide behind it.
//   finish  one workgroup: thread t adds the partials t, t + 256, ... , the 256 sums add up in the same way, thread 0 writes
//           state[0] = norm (rounded to fp32 once), [1] = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0), [2] = found_inf,
//           [3] += found_inf (a float: exact up to 2^24 flagged calls), [4] = 1 - found_inf (what the step counters advance by).
//           An inf element makes the norm inf and the coefficient 0: meaningless then, and unused — the step is not taken.
#include "common.h"

namespace vmasr {
namespace {

constexpr int kNormChunk = 4096;   // elements per workgroup: vmasr_adamw_chunk(), the two chunk tables are built alike

__device__ __forceinline__ void sq_acc(const float x, double &s, unsigned &bad) {
    s = fma((double)x, (double)x, s);
    bad |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;      // inf or NaN
}

// sum of `a` over the 256 threads in a fixed order (every thread gets it), OR of `bad` over them: a butterfly over the 64 lanes of each
// wave (every lane ends with the same bits: a + b == b + a), then the four wave sums through LDS — the OR's barrier is the only one
__device__ __forceinline__ double block_sum_or(double a, const unsigned bad, int &any_bad) {
    __shared__ double wsum[4];
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) a += __shfl_xor(a, d);
    if ((threadIdx.x & (kWave - 1)) == 0) wsum[threadIdx.x / kWave] = a;
    any_bad = __syncthreads_or((int)bad);
    return (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const vmasr_grad_segment *__restrict__ segs, const int2 *__restrict__ chunks,
                                                                double *__restrict__ part, unsigned *__restrict__ flags) {
    const int2 ck = chunks[blockIdx.x];                       // (segment, chunk index within the segment)
    const vmasr_grad_segment sg = segs[ck.x];
    const long base = (long)ck.y * kNormChunk;
    const long n = sg.n - base < kNormChunk ? sg.n - base : kNormChunk;
    const float *g = sg.ptr + base;
    double s = 0.0;
    unsigned bad = 0;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {        // gradient views start anywhere in the flat buffer: per chunk, wave-uniform
        const long n4 = n / 4;
        for (long i = threadIdx.x; i < n4; i += 256) {
            const float4 G = reinterpret_cast<const float4 *>(g)[i];
            sq_acc(G.x, s, bad); sq_acc(G.y, s, bad); sq_acc(G.z, s, bad); sq_acc(G.w, s, bad);
        }
        for (long i = n4 * 4 + threadIdx.x; i < n; i += 256) sq_acc(g[i], s, bad);
    } else {
        for (long i = threadIdx.x; i < n; i += 256) sq_acc(g[i], s, bad);
    }
    int any_bad;
    const double total = block_sum_or(s, bad, any_bad);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = total;
        flags[blockIdx.x] = any_bad ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const double *__restrict__ part, const unsigned *__restrict__ flags,
                                                               const int nchunks, const float max_norm, float *__restrict__ state) {
    double a = 0.0;
    unsigned bad = 0;
    for (int i = threadIdx.x; i < nchunks; i += 256) {
        a += part[i];
        bad |= flags[i];
    }
    int any_bad;
    const double total = block_sum_or(a, bad, any_bad);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        float coef = 1.f;
        if (max_norm > 0.f) {
            const float c = max_norm / (norm + 1e-6f);      // torch.nn.utils.clip_grad_norm_
            coef = c < 1.f ? c : 1.f;                       // (a NaN norm gives 1: found_inf is set then, nothing is applied)
        }
        state[0] = norm;
        state[1] = coef;
        state[2] = any_bad ? 1.f : 0.f;
        if (any_bad) state[3] += 1.f;                       // running count, never reset here
        state[4] = any_bad ? 0.f : 1.f;
    }
}

}  // namespace
}  // namespace vmasr

using namespace vmasr;

VMASR_EXPORT size_t vmasr_grad_norm_workspace(int32_t nchunks) {
    return nchunks > 0 ? (size_t)nchunks * (sizeof(double) + sizeof(unsigned)) : 0;      // the partials, then the flags
}

VMASR_EXPORT int vmasr_grad_norm(const vmasr_grad_segment *segments, const int32_t *chunks, int32_t nchunks, int64_t total_elems,
                                 float max_norm, float *state, void *workspace, size_t ws_bytes, vmasr_stream_t stream) {
    VMASR_REQUIRE(segments && chunks && state && workspace, VMASR_EINVAL, "grad_norm: null argument");
    VMASR_REQUIRE(nchunks > 0 && total_elems > 0, VMASR_EINVAL, "grad_norm: no elements");
    VMASR_REQUIRE(max_norm == max_norm, VMASR_EINVAL, "grad_norm: max_norm is NaN");
    VMASR_REQUIRE(ws_bytes >= vmasr_grad_norm_workspace(nchunks), VMASR_EINVAL, "grad_norm: workspace too small (%zu < %zu bytes)", ws_bytes,
                  vmasr_grad_norm_workspace(nchunks));
    VMASR_REQUIRE(aligned_to(workspace, 8) && aligned_to(state, 4), VMASR_EINVAL, "grad_norm: workspace not 8-byte / state not 4-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *part = static_cast<double *>(workspace);
    unsigned *flags = reinterpret_cast<unsigned *>(part + nchunks);
    VMASR_LAUNCH(VMASR_K_GRAD_NORM, 4.0 * (double)total_elems, grad_norm_partial_kernel, dim3(nchunks), dim3(256), 0, st, segments,
                 reinterpret_cast<const int2 *>(chunks), part, flags);
    VMASR_LAUNCH(VMASR_K_GRAD_NORM, 12.0 * (double)nchunks, grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, part, flags, nchunks, max_norm,
                 state);
    return check_launch("grad_norm");
}
