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
//
// Also here: vmasr_degrade_batch, the same per-output code for a batch of clips at per-clip ratios (down pass, up pass + align, the
// staging chosen per workgroup from the clip's descriptor), and vmasr_resample_design, the filter above designed on the device.
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

// The outputs [m0, m0 + tile) of one row, one per thread (every thread of the workgroup calls it; XLDS / HLDS as above).  Output m
// is stored for m < n_store: the sum for m < n_out, zero beyond (n_store == n_out in resample_poly; degrade_batch's up pass
// stores the row trimmed or zero-filled to the clip's length: align_waveform).
template <bool XLDS, bool HLDS>
__device__ __forceinline__ void resample_tile(const float *__restrict__ xb, const float *__restrict__ h, float *__restrict__ yb,
                                              const int64_t n_in, const int64_t n_out, const int64_t n_store, const int up,
                                              const int down, const int half_len, const int win, const int64_t m0, const int tile) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sx = reinterpret_cast<float *>(smem);
    float *sh = sx + (XLDS ? (win + 3) / 4 * 4 : 0);
    const int tid = threadIdx.x;
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
    if (m >= n_store) return;
    const float *hp = HLDS ? sh : h;
    float acc = 0.f;
    if (m >= n_out) {
        // past the end of the resampled row: zero
    } else if constexpr (XLDS) {
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

template <bool XLDS, bool HLDS>
__global__ __launch_bounds__(kTile) void resample_poly_kernel(const float *__restrict__ x, const float *__restrict__ h,
                                                              float *__restrict__ y, const int64_t n_in, const int64_t n_out,
                                                              const int up, const int down, const int half_len, const int win) {
    const int tile = blockDim.x;
    resample_tile<XLDS, HLDS>(x + (size_t)blockIdx.y * n_in, h, y + (size_t)blockIdx.y * n_out, n_in, n_out, n_out, up, down, half_len,
                              win, (int64_t)blockIdx.x * tile, tile);
}

// ---- degrade_batch: B clips, each down to its own rate and up again, in two launches ------------------------------------------------
// grid (tiles of the longest row, B), kTile outputs per workgroup.  Every workgroup reads its clip's descriptor (a uniform load) and
// takes that clip's staging choice, the same for all its threads: batch_plan below, which the launcher evaluates too (for the
// dynamic LDS size of the launch, the largest any clip needs).  The tile is not shrunk here: a window too large for kTile outputs
// (down/up > 20) reads x from global memory.  An output's terms and their order do not depend on the staging or on the tile, so
// a row is bit-identical to resample_poly's.
struct BatchPlan { bool xlds, hlds; int win; };

__host__ __device__ __forceinline__ BatchPlan batch_plan(int up, int down, int half_len) {
    const int64_t win = ((int64_t)(kTile - 1) * down + 2 * (int64_t)half_len) / up + 1;
    BatchPlan p;
    p.xlds = win <= kMaxWin && (int64_t)kTile * down + 2 * (int64_t)half_len + 2 * (int64_t)up < INT32_MAX;
    p.hlds = 2 * (int64_t)half_len + 1 <= kMaxTaps;
    p.win = p.xlds ? (int)win : 0;
    return p;
}

size_t batch_plan_lds(int up, int down, int half_len) {
    const BatchPlan p = batch_plan(up, down, half_len);
    return (size_t)((p.win + 3) / 4 * 4) * 4 + (p.hlds ? (size_t)(2 * half_len + 1) * 4 : 0);
}

// UP false: x[b] (T) -> the clip's intermediate (n_mid) by up/down.  UP true: the intermediate -> y[b, :T] by down/up, trimmed or
// zero-filled to T; a clip with up == down is copied from x[b].
template <bool UP>
__global__ __launch_bounds__(kTile) void degrade_pass_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                             const vmasr_degrade_item *__restrict__ items, float *__restrict__ mid,
                                                             const int64_t T) {
    const vmasr_degrade_item it = items[blockIdx.y];
    const int64_t m0 = (int64_t)blockIdx.x * kTile;
    const float *xb = x + (size_t)blockIdx.y * T;
    if (it.up == it.down) {
        const int64_t m = m0 + threadIdx.x;
        if (UP && m < T) y[(size_t)blockIdx.y * T + m] = xb[m];
        return;
    }
    float *mb = mid + it.mid_off;
    const int up = UP ? it.down : it.up, down = UP ? it.up : it.down, half_len = UP ? it.half_len_up : it.half_len;
    const int64_t n_in = UP ? it.n_mid : T;
    const int64_t n_out = UP ? ceil_div64(it.n_mid * up, down) : it.n_mid, n_store = UP ? T : it.n_mid;
    if (m0 >= n_store) return;                    // workgroup-uniform: the grid is sized for the longest row of the batch
    const float *src = UP ? mb : xb, *h = UP ? it.h_up : it.h_down;
    float *dst = UP ? y + (size_t)blockIdx.y * T : mb;
    const BatchPlan p = batch_plan(up, down, half_len);
#define VMASR_DG_TILE(XL, HL) resample_tile<XL, HL>(src, h, dst, n_in, n_out, n_store, up, down, half_len, p.win, m0, kTile)
    if (p.xlds && p.hlds) VMASR_DG_TILE(true, true);
    else if (p.xlds) VMASR_DG_TILE(true, false);
    else if (p.hlds) VMASR_DG_TILE(false, true);
    else VMASR_DG_TILE(false, false);
#undef VMASR_DG_TILE
}

// ---- filter design on the device ---------------------------------------------------------------------------------------------------
// h = up * firwin(2*half_len + 1, fc, kaiser 5.0), fc = 1/max(up, down), as vm_asr_amd/resample.py:_design states it: everything in
// float64, one rounding to fp32 at the store.  Stage 1 writes the taps before normalisation to the workspace and one partial sum per
// workgroup; stage 2 adds the partial sums (every workgroup the same way) and stores h = raw / sum * up.  Which thread adds which tap
// depends on the tap count alone and every sum is a fixed tree: no atomics, the same bits in every run.
constexpr int kDesignThreads = 256;
constexpr int kDesignBlocks = 1024;   // at most; the partial sums of stage 1
constexpr int kI0Terms = 24;          // (6.25^k / k!^2 < 1e-30 beyond: x <= 5)

// Modified Bessel function I0 on [0, 5]: the power series sum_k (x^2/4)^k / k!^2 in nested form, 1 + t/1 (1 + t/4 (1 + t/9 (...))).
// All terms are positive and each step's rounding is damped by the factors that follow: relative error of a few 1e-16.
__device__ __forceinline__ double bessel_i0(double x) {
    const double t = 0.25 * x * x;
    double s = 1.0;
#pragma unroll
    for (int k = kI0Terms; k >= 1; --k) s = 1.0 + s * (t / (double)(k * k));
    return s;
}

__device__ __forceinline__ double block_sum(double v, double *sm) {   // fixed tree over kDesignThreads values; every thread gets it
    sm[threadIdx.x] = v;
    __syncthreads();
    for (int s = kDesignThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
        __syncthreads();
    }
    const double r = sm[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(kDesignThreads) void design_taps_kernel(double *__restrict__ raw, double *__restrict__ part,
                                                                     const int64_t n, const int half_len, const double fc) {
    __shared__ double sm[kDesignThreads];
    const double i0b = bessel_i0(5.0);
    double local = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * kDesignThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDesignThreads) {
        const double m = (double)(i - half_len), xs = fc * m, r = m / (double)half_len;
        const double sinc = (m == 0.0) ? 1.0 : sinpi(xs) / (M_PI * xs);
        const double v = fc * sinc * (bessel_i0(5.0 * sqrt(fmax(1.0 - r * r, 0.0))) / i0b);
        raw[i] = v;
        local += v;
    }
    const double s = block_sum(local, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kDesignThreads) void design_scale_kernel(const double *__restrict__ raw, const double *__restrict__ part,
                                                                      float *__restrict__ h, const int64_t n, const double up) {
    __shared__ double sm[kDesignThreads];
    double local = 0.0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += kDesignThreads) local += part[i];
    const double total = block_sum(local, sm);
    for (int64_t i = (int64_t)blockIdx.x * kDesignThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDesignThreads)
        h[i] = (float)(raw[i] / total * up);
}

int design_blocks(int64_t n) {
    const int64_t b = (n + kDesignThreads - 1) / kDesignThreads;
    return (int)(b < kDesignBlocks ? b : kDesignBlocks);
}

int gcd32(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
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
    const int g = gcd32(up, down);
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

VMASR_EXPORT size_t vmasr_resample_design_workspace(int32_t half_len) {
    if (half_len < 1 || half_len > (1 << 30)) return 0;
    return (size_t)(2 * (int64_t)half_len + 1 + kDesignBlocks) * sizeof(double);
}

VMASR_EXPORT int vmasr_resample_design(float *h, int32_t up, int32_t down, int32_t half_len, void *ws, size_t ws_bytes,
                                       vmasr_stream_t stream) {
    VMASR_REQUIRE(h && ws, VMASR_EINVAL, "resample_design: null tensor");
    VMASR_REQUIRE(up > 0 && down > 0, VMASR_EINVAL, "resample_design: non-positive up or down (got %d, %d)", up, down);
    VMASR_REQUIRE(gcd32(up, down) == 1, VMASR_EINVAL, "resample_design: up / down = %d / %d is not in lowest terms (gcd %d)", up, down,
                  gcd32(up, down));
    VMASR_REQUIRE(half_len >= 1 && half_len <= (1 << 30), VMASR_EINVAL, "resample_design: half_len outside [1, 2^30] (got %d)", half_len);
    VMASR_REQUIRE(ws_bytes >= vmasr_resample_design_workspace(half_len) && aligned_to(ws, sizeof(double)), VMASR_EINVAL,
                  "resample_design: workspace too small or not 8-byte aligned (%zu bytes, need %zu)", ws_bytes,
                  vmasr_resample_design_workspace(half_len));
    const int64_t n = 2 * (int64_t)half_len + 1;
    double *raw = static_cast<double *>(ws), *part = raw + n;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)design_blocks(n)), block(kDesignThreads);
    VMASR_LAUNCH(VMASR_K_RESAMPLE_DESIGN, 8.0 * (double)n, design_taps_kernel, grid, block, 0, st, raw, part, n, half_len,
                 1.0 / (double)(up > down ? up : down));
    VMASR_LAUNCH(VMASR_K_RESAMPLE_DESIGN, 12.0 * (double)n, design_scale_kernel, grid, block, 0, st, raw, part, h, n, (double)up);
    return check_launch("resample_design");
}

// floats of the workspace a clip's intermediate takes (16-byte granules; none for a clip that is copied)
static int64_t degrade_mid_floats(const vmasr_degrade_item &it) { return it.up == it.down ? 0 : (it.n_mid + 3) / 4 * 4; }

VMASR_EXPORT size_t vmasr_degrade_batch_workspace(const vmasr_degrade_item *items, int32_t B) {
    if (!items || B <= 0) return 0;
    int64_t floats = 0;
    for (int b = 0; b < B; ++b) {
        if (items[b].n_mid < 0 || items[b].n_mid > (INT64_MAX >> 4) - floats) return 0;
        floats += degrade_mid_floats(items[b]);
    }
    return (size_t)floats * sizeof(float);
}

VMASR_EXPORT int vmasr_degrade_batch(const float *x, float *y, const vmasr_degrade_item *items, const vmasr_degrade_item *items_dev,
                                     int32_t B, int64_t T, void *ws, size_t ws_bytes, vmasr_stream_t stream) {
    VMASR_REQUIRE(x && y && items && items_dev, VMASR_EINVAL, "degrade_batch: null tensor or descriptor table");
    VMASR_REQUIRE(B > 0 && T > 0, VMASR_EINVAL, "degrade_batch: non-positive B or T (got %d, %lld)", B, (long long)T);
    VMASR_REQUIRE(B <= 65535, VMASR_EINVAL, "degrade_batch: B > 65535 clips in one call (got %d)", B);
    int64_t end = 0, rows = 0;             // end of the intermediates laid out so far (floats); the longest intermediate
    size_t lds[2] = {0, 0};
    for (int b = 0; b < B; ++b) {
        const vmasr_degrade_item &it = items[b];
        VMASR_REQUIRE(it.up > 0 && it.down > 0, VMASR_EINVAL, "degrade_batch: clip %d: non-positive up or down (got %d, %d)", b, it.up, it.down);
        VMASR_REQUIRE(gcd32(it.up, it.down) == 1, VMASR_EINVAL, "degrade_batch: clip %d: up / down = %d / %d is not in lowest terms", b,
                      it.up, it.down);
        const int big = it.up > it.down ? it.up : it.down;
        VMASR_REQUIRE(T <= (INT64_MAX >> 3) / big / big, VMASR_EINVAL, "degrade_batch: clip %d: T * max(up, down)^2 too large for the 64-bit index arithmetic", b);
        VMASR_REQUIRE(it.n_mid == ceil_div64(T * it.up, it.down), VMASR_EINVAL, "degrade_batch: clip %d: n_mid must be ceil(T*up/down) = %lld (got %lld)",
                      b, (long long)ceil_div64(T * it.up, it.down), (long long)it.n_mid);
        if (it.up == it.down) continue;    // copied: no taps, no intermediate
        VMASR_REQUIRE(it.h_down && it.h_up, VMASR_EINVAL, "degrade_batch: clip %d: null taps", b);
        VMASR_REQUIRE(it.half_len >= 0 && it.half_len_up >= 0 && it.half_len <= (1 << 30) && it.half_len_up <= (1 << 30), VMASR_EINVAL,
                      "degrade_batch: clip %d: half_len outside [0, 2^30] (got %d, %d)", b, it.half_len, it.half_len_up);
        VMASR_REQUIRE(it.mid_off >= end && it.mid_off % 4 == 0 && (size_t)(it.mid_off + it.n_mid) <= ws_bytes / sizeof(float), VMASR_EINVAL,
                      "degrade_batch: clip %d: intermediate [%lld, %lld) overlaps the previous clip's, is not 16-byte aligned or lies outside "
                      "the workspace (%zu bytes; vmasr_degrade_batch_workspace)", b, (long long)it.mid_off, (long long)(it.mid_off + it.n_mid), ws_bytes);
        end = it.mid_off + it.n_mid;
        if (it.n_mid > rows) rows = it.n_mid;
        const size_t l0 = batch_plan_lds(it.up, it.down, it.half_len), l1 = batch_plan_lds(it.down, it.up, it.half_len_up);
        if (l0 > lds[0]) lds[0] = l0;
        if (l1 > lds[1]) lds[1] = l1;
    }
    VMASR_REQUIRE(end == 0 || (ws && aligned_to(ws, 16)), VMASR_EINVAL, "degrade_batch: null or misaligned workspace");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 block(kTile), grid_up((unsigned)((T + kTile - 1) / kTile), (unsigned)B);
    VMASR_REQUIRE((rows + kTile - 1) / kTile <= INT32_MAX, VMASR_EINVAL, "degrade_batch: T too large for one launch");
    float *mid = static_cast<float *>(ws);
    const double bytes = 4.0 * (double)B * (double)T + 4.0 * (double)end;
    if (end > 0) {                         // (every clip copied: the down pass has nothing to do)
        const dim3 grid_down((unsigned)((rows + kTile - 1) / kTile), (unsigned)B);
        VMASR_LAUNCH(VMASR_K_DEGRADE_BATCH, bytes, degrade_pass_kernel<false>, grid_down, block, lds[0], st, x, y, items_dev, mid, T);
    }
    VMASR_LAUNCH(VMASR_K_DEGRADE_BATCH, bytes, degrade_pass_kernel<true>, grid_up, block, lds[1], st, x, y, items_dev, mid, T);
    return check_launch("degrade_batch");
}
