// resample.hip — polyphase FIR resampling (scipy.signal.resample_poly, padtype "constant") of a batch of rows, for gfx950.
//
// Replaces the CPU stage the reference runs per clip (data_loader/data_loaders.py:340,472-478, trainer/inferencer.py:270):
//
//     y[b, m] = sum_q x[b, q] * h[half_len + m*down - q*up]          x zero outside [0, n_in), h index inside [0, 2*half_len]
//
// with h = up * firwin(2*half_len + 1, 1/max(up, down), kaiser 5.0) designed on the host (vm_asr_amd/resample.py).
//
// One thread per output sample, grid (output tiles, B).  Output m reads the inputs q0, q0 + 1, ... with q0 = ceil((m*down -
// half_len) / up) and the taps k0, k0 - up, ... >= 0 with k0 = half_len + m*down - q0*up: 2*half_len/up + 1 terms, about 20 when
// upsampling and 20*down/up when downsampling, summed in fp32 with fmaf in that order.
//
// Staging (chosen by the launcher from the ratio, never from the data):
//   * the tile's input window, ((tile - 1)*down + 2*half_len) / up + 1 floats starting at the first sample its first output
//     reads, goes to LDS with the zero padding applied while it is filled; the tile shrinks 256 -> 128 -> 64 until the window
//     fits kMaxWin.  The tile's base m0*down - half_len is 64-bit (n_out*down passes 2^31 for minutes of audio at awkward
//     ratios); what a thread adds to it is 32-bit, which the launcher checks.  A ratio whose window does not fit even 64
//     outputs (down >> up) reads x from global memory with 64-bit indices throughout.
//   * h goes to LDS when it has at most kMaxTaps taps (small integer ratios: 61..121 taps; 147/160: 3201); a larger h
//     (3200/823: 64 001 taps; 47999/48000: 960 001) is read through L2.
#include "common.h"

namespace vmasr {
namespace {

constexpr int kTile = 256;        // outputs (= threads) per workgroup, halved down to kMinTile while the window does not fit
constexpr int kMinTile = 64;
constexpr int kMaxWin = 6144;     // floats of x one workgroup stages (24 KB)
constexpr int kMaxTaps = 8192;    // taps of h one workgroup stages (32 KB); window + taps stay inside the 64 KB default limit

__host__ __device__ __forceinline__ int64_t ceil_div64(int64_t a, int64_t b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }
__device__ __forceinline__ int ceil_div32(int a, int b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

// floats of x the outputs [m0, m0 + tile) read, from the first sample output m0 reads (any m0)
int64_t window_floats(int tile, int up, int down, int half_len) {
    return ((int64_t)(tile - 1) * down + 2 * (int64_t)half_len) / up + 1;
}

template <bool XLDS, bool HLDS>
__global__ __launch_bounds__(kTile) void resample_poly_kernel(const float *__restrict__ x, const float *__restrict__ h,
                                                              float *__restrict__ y, const int64_t n_in, const int64_t n_out,
                                                              const int up, const int down, const int half_len, const int win) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sx = reinterpret_cast<float *>(smem);
    float *sh = sx + (XLDS ? (win + 3) / 4 * 4 : 0);
    const int tid = threadIdx.x, tile = blockDim.x;
    const int64_t m0 = (int64_t)blockIdx.x * tile;
    const float *xb = x + (size_t)blockIdx.y * n_in;
    float *yb = y + (size_t)blockIdx.y * n_out;
    const int64_t a = m0 * down - half_len;       // output m0 + t reads the inputs q >= ceil((a + t*down) / up)
    const int64_t q_lo = ceil_div64(a, up);       // workgroup-uniform
    if constexpr (XLDS) {
        for (int i = tid; i < win; i += tile) {
            const int64_t q = q_lo + i;
            sx[i] = (q >= 0 && q < n_in) ? xb[q] : 0.f;
        }
    }
    if constexpr (HLDS) {
        for (int i = tid; i <= 2 * half_len; i += tile) sh[i] = h[i];
    }
    if constexpr (XLDS || HLDS) __syncthreads();
    const int64_t m = m0 + tid;
    if (m >= n_out) return;
    const float *hp = HLDS ? sh : h;
    float acc = 0.f;
    if constexpr (XLDS) {
        // relative to the window: a + t*down = q_lo*up + d with d = t*down - (q_lo*up - a) > -up, a 32-bit number (launcher)
        const int d = tid * down - (int)(q_lo * up - a);
        int i = ceil_div32(d, up);                // q0 - q_lo, in [0, win)
        for (int k = 2 * half_len + d - i * up; k >= 0; k -= up, ++i) acc = fmaf(sx[i], hp[k], acc);
    } else {
        const int64_t t = a + (int64_t)tid * down;
        int64_t q = ceil_div64(t, up);
        int64_t k = 2 * (int64_t)half_len + t - q * up;
        if (q < 0) { k += q * up; q = 0; }        // the zero padding in front: skip to x[0]
        for (; k >= 0 && q < n_in; k -= up, ++q) acc = fmaf(xb[q], hp[k], acc);
    }
    yb[m] = acc;
}

}  // namespace
}  // namespace vmasr

using namespace vmasr;

VMASR_EXPORT int vmasr_resample_poly(const float *x, const float *h, float *y, int32_t B, int64_t n_in, int64_t n_out, int32_t up,
                                     int32_t down, int32_t half_len, vmasr_stream_t stream) {
    VMASR_REQUIRE(x && h && y, VMASR_EINVAL, "resample_poly: null tensor");
    VMASR_REQUIRE(B > 0 && n_in > 0 && up > 0 && down > 0, VMASR_EINVAL,
                  "resample_poly: non-positive B, n_in, up or down (got %d, %lld, %d, %d)", B, (long long)n_in, up, down);
    VMASR_REQUIRE(half_len >= 0, VMASR_EINVAL, "resample_poly: half_len < 0 (got %d)", half_len);
    int g = up, r = down;
    while (r) { const int t = g % r; g = r; r = t; }
    VMASR_REQUIRE(g == 1, VMASR_EINVAL, "resample_poly: up / down = %d / %d is not in lowest terms (gcd %d)", up, down, g);
    // the index arithmetic stays inside int64: n_in*up + (kTile + 1)*down + 2*half_len < 2^62
    VMASR_REQUIRE(n_in <= (INT64_MAX >> 2) / (up > down ? up : down) && half_len <= (1 << 30), VMASR_EINVAL,
                  "resample_poly: n_in * max(up, down) or half_len too large for the 64-bit index arithmetic");
    VMASR_REQUIRE(n_out == ceil_div64(n_in * up, down), VMASR_EINVAL, "resample_poly: n_out must be ceil(n_in*up/down) = %lld (got %lld)",
                  (long long)ceil_div64(n_in * up, down), (long long)n_out);
    VMASR_REQUIRE(B <= 65535, VMASR_EINVAL, "resample_poly: B > 65535 rows in one call (got %d)", B);
    int tile = kTile;
    while (tile > kMinTile && window_floats(tile, up, down, half_len) > kMaxWin) tile /= 2;
    const int64_t win = window_floats(tile, up, down, half_len);
    // staged x: the window fits and a thread's offsets from the tile base are 32-bit: |t*down - r| + 2*half_len + up < 2^31
    const bool xlds = win <= kMaxWin && (int64_t)tile * down + 2 * (int64_t)half_len + 2 * (int64_t)up < INT32_MAX;
    if (!xlds) tile = kTile;
    const bool hlds = 2 * (int64_t)half_len + 1 <= kMaxTaps;
    const int64_t tiles = (n_out + tile - 1) / tile;
    VMASR_REQUIRE(tiles <= INT32_MAX, VMASR_EINVAL, "resample_poly: n_out too large for one launch (%lld tiles)", (long long)tiles);
    const size_t sm = (xlds ? (size_t)((win + 3) / 4 * 4) * 4 : 0) + (hlds ? (size_t)(2 * half_len + 1) * 4 : 0);
    const double bytes = 4.0 * ((double)B * ((double)n_in + (double)n_out) + 2.0 * half_len + 1.0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)tiles, (unsigned)B), block(tile);
    const int w = xlds ? (int)win : 0;
#define VMASR_RS_LAUNCH(XL, HL) \
    VMASR_LAUNCH(VMASR_K_RESAMPLE, bytes, (resample_poly_kernel<XL, HL>), grid, block, sm, st, x, h, y, n_in, n_out, up, down, half_len, w)
    if (xlds && hlds) VMASR_RS_LAUNCH(true, true);
    else if (xlds) VMASR_RS_LAUNCH(true, false);
    else if (hlds) VMASR_RS_LAUNCH(false, true);
    else VMASR_RS_LAUNCH(false, false);
#undef VMASR_RS_LAUNCH
    return check_launch("resample_poly");
}
