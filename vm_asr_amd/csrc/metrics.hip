// metrics.hip — SNR, LSD, LSD-HF, LSD-LF of a batch in two launches, for gfx950.
//
// Replaces the composition in vm_asr_amd/metric.py (model/metric.py:5-67 of the reference: six 2048-point STFTs written to
// HBM, ~30 elementwise / reduction launches, one host read per clip for the band edge) on the per-step path.
//
// metrics_frames_kernel: one workgroup owns kMF consecutive frames of one clip.  Per frame the windowed OUTPUT frame and the
//   windowed TARGET frame are the real and imaginary parts of one complex radix-2 Stockham FFT in LDS and are separated by
//   Hermitian symmetry (the split stft_like_kernel uses for two frames of one signal).  d = log10 max(|X|^2, 1e-8) -
//   log10 max(|Y|^2, 1e-8) is squared and summed over all bins, over [hf, F) and over [0, hf) — three direct sums — and the
//   workgroup writes sqrt(mean) of each plus the SNR partial sums (sum tgt^2, sum (out - tgt)^2) of the frame's own `hop`
//   samples: 5 floats per frame.  No spectrum reaches HBM.
// metrics_finish_kernel: one workgroup per clip: mean over frames and the SNR in fp64 -> per_clip (B, 4) fp32; workgroup 0
//   also forms the batch means (fp64, clip order) and adds them to the 5-double accumulator.
// Every sum runs in a fixed order (DPP wave sums, then waves in order, then frames in order; no atomics): two calls agree bit
// for bit.
//
// out == tgt gives LSD = LSD-HF = LSD-LF = 0 EXACTLY, by construction of the transform: with equal real and imaginary parts
// the input is invariant under the swap S(x, y) = (y, x), and Z[n - f] = S(Z[f]) then holds bit for bit after every pass
// because (a) the twiddle table is built mirror-symmetric, tw[n/2 - m] = (-tw[m].x, tw[m].y), and (b) the butterfly is
// evaluated without fused multiply-add contraction, so that the products of the mirrored butterfly are the same rounded
// numbers with the sign flipped.  Z[n - f] = S(Z[f]) makes the two separated spectra identical, hence d == 0.
#include "common.h"

namespace vmasr {
namespace {

constexpr int kMF = 2;        // frames per workgroup: the twiddle / window tables (3 n / 2 sincospi) are built once for both
constexpr int kThreads = 256;
constexpr int kVals = 5;      // per frame: lsd, lsd_hf, lsd_lf, sum tgt^2, sum (out - tgt)^2

struct MetSmem {
    float2 *a, *b;  // ping-pong, n each
    float2 *tw;     // n/2: exp(-2 pi i m / n)
    float *win;     // n: periodic hann
};

__device__ __forceinline__ MetSmem met_carve(char *smem, int n) {
    MetSmem s;
    s.a = reinterpret_cast<float2 *>(smem);
    s.b = s.a + n;
    s.tw = s.b + n;
    s.win = reinterpret_cast<float *>(s.tw + n / 2);
    return s;
}

size_t met_smem_bytes(int n) { return (size_t)n * 8 * 2 + (size_t)n / 2 * 8 + (size_t)n * 4; }   // 48 KB at n = 2048

__device__ __forceinline__ void met_tables(const MetSmem &s, int n) {
    // first quadrant from sincospi, second quadrant mirrored from it (see the header: exact swap symmetry)
    for (int m = threadIdx.x; m <= n / 4; m += blockDim.x) {
        float sn, cs;
        sincospif(2.f * (float)m / (float)n, &sn, &cs);
        if (m == 0) { cs = 1.f; sn = 0.f; }
        if (m == n / 4) { cs = 0.f; sn = 1.f; }
        s.tw[m] = make_float2(cs, -sn);
        if (m > 0 && m < n / 4) s.tw[n / 2 - m] = make_float2(-cs, -sn);
    }
    for (int i = threadIdx.x; i < n; i += blockDim.x) s.win[i] = 0.5f - 0.5f * cospif(2.f * (float)i / (float)n);
}

// Stockham radix-2, forward, natural order in/out (stft.hip: block_fft), butterflies without FMA contraction.
__device__ __forceinline__ float2 *met_fft(float2 *src, float2 *dst, const float2 *tw, int n) {
#pragma clang fp contract(off)
    for (int ns = 1; ns < n; ns <<= 1) {
        const int tstride = n / (2 * ns);
        for (int j = threadIdx.x; j < n / 2; j += blockDim.x) {
            const int k = j & (ns - 1);
            const float2 w = tw[k * tstride];
            const float2 p = src[j], q = src[j + n / 2];
            const float wqx = w.x * q.x - w.y * q.y;
            const float wqy = w.x * q.y + w.y * q.x;
            const int j0 = ((j - k) << 1) + k;
            dst[j0] = make_float2(p.x + wqx, p.y + wqy);
            dst[j0 + ns] = make_float2(p.x - wqx, p.y - wqy);
        }
        __syncthreads();
        float2 *t = src; src = dst; dst = t;
    }
    return src;
}

__device__ __forceinline__ int met_reflect(int i, int T) {
    while (i < 0 || i >= T) {      // T > n/2 >= 32 (checked by the launcher)
        if (i < 0) i = -i;
        if (i >= T) i = 2 * (T - 1) - i;
    }
    return i;
}

// sums of kVals values over the workgroup, fixed order: DPP wave sums, then the waves in order.  Result in thread 0.
__device__ __forceinline__ void met_block_sum(float (&v)[kVals], float (*red)[kVals]) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < kVals; ++c) {
        const float t = wave_sum(v[c]);
        if (lane == 0) red[wave][c] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < kVals; ++c) {
            float t = red[0][c];
            for (int w = 1; w < kThreads / kWave; ++w) t += red[w][c];
            v[c] = t;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void metrics_frames_kernel(const float *__restrict__ out, const float *__restrict__ tgt,
                                                                  const int64_t *__restrict__ hf, float *__restrict__ part,
                                                                  const int T, const int n, const int hop, const int M) {
#pragma clang fp contract(off)     // |X|^2 and |Y|^2 from one instruction pattern (see the header); the explicit fmaf below stay
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float red[kThreads / kWave][kVals];
    const MetSmem s = met_carve(smem, n);
    const int F = n / 2 + 1, pad = n / 2;
    // neighbouring frame groups read overlapping samples: keep them on one XCD (stft.hip)
    const int lin = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y);
    const int b = lin / gridDim.x, m0 = (lin % gridDim.x) * kMF;
    const float *x = out + (size_t)b * T, *y = tgt + (size_t)b * T;
    const int64_t h64 = hf[b];
    const int h = h64 < 0 ? 0 : (h64 > F ? F : (int)h64);     // bins [0, h) are LF, [h, F) HF; an empty band divides 0 by 0
    met_tables(s, n);
    __syncthreads();
    for (int m = m0; m < m0 + kMF && m < M; ++m) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int t = met_reflect(m * hop + i - pad, T);
            const float w = s.win[i];
            s.a[i] = make_float2(w * x[t], w * y[t]);
        }
        __syncthreads();
        const float2 *z = met_fft(s.a, s.b, s.tw, n);
        float v[kVals] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int f = threadIdx.x; f < F; f += blockDim.x) {
            const float2 zf = z[f], zc = z[(n - f) & (n - 1)];
            // X = (Z[f] + conj Z[n-f]) / 2 ; Y = (Z[f] - conj Z[n-f]) / (2i)
            const float xr = 0.5f * (zf.x + zc.x), xi = 0.5f * (zf.y - zc.y);
            const float yr = 0.5f * (zf.y + zc.y), yi = 0.5f * (zc.x - zf.x);
            const float px = xr * xr + xi * xi, py = yr * yr + yi * yi;
            const float d = log10f(fmaxf(px, 1e-8f)) - log10f(fmaxf(py, 1e-8f));
            const float d2 = d * d;
            v[0] += d2;
            if (f >= h) v[1] += d2; else v[2] += d2;
        }
        // SNR partial sums of this frame's own hop samples: the M frames tile [0, M hop), which covers [0, T)
        for (int j = threadIdx.x; j < hop; j += blockDim.x) {
            const long t = (long)m * hop + j;
            if (t < T) {
                const float tv = y[t], dv = x[t] - tv;
                v[3] = fmaf(tv, tv, v[3]);
                v[4] = fmaf(dv, dv, v[4]);
            }
        }
        met_block_sum(v, red);     // (its barriers also separate this frame's reads of z from the next frame's fill)
        if (threadIdx.x == 0) {
            float *o = part + ((size_t)b * M + m) * kVals;
            o[0] = sqrtf(v[0] / (float)F);
            o[1] = sqrtf(v[1] / (float)(F - h));
            o[2] = sqrtf(v[2] / (float)h);
            o[3] = v[3];
            o[4] = v[4];
        }
    }
}

// The four values of clip b, computed by the whole workgroup (fixed order), valid in thread 0.
__device__ __forceinline__ void met_clip_values(const float *__restrict__ part, int b, int M, double (*red)[kVals],
                                                float (&res)[4]) {
    double acc[kVals] = {0., 0., 0., 0., 0.};
    const float *p = part + (size_t)b * M * kVals;
    for (int m = threadIdx.x; m < M; m += blockDim.x)
#pragma unroll
        for (int c = 0; c < kVals; ++c) acc[c] += (double)p[(size_t)m * kVals + c];
#pragma unroll
    for (int c = 0; c < kVals; ++c) red[threadIdx.x][c] = acc[c];
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st)
#pragma unroll
            for (int c = 0; c < kVals; ++c) red[threadIdx.x][c] += red[threadIdx.x + st][c];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double nt = sqrt(red[0][3]), nd = fmax(sqrt(red[0][4]), 1e-8);
        res[0] = (float)(20.0 * log10(nt / nd));
        for (int c = 0; c < 3; ++c) res[1 + c] = (float)(red[0][c] / (double)M);
    }
    __syncthreads();
}

__global__ __launch_bounds__(kThreads) void metrics_finish_kernel(const float *__restrict__ part, float *__restrict__ per_clip,
                                                                  double *__restrict__ acc, const int B, const int M) {
    __shared__ double red[kThreads][kVals];
    float res[4];
    met_clip_values(part, blockIdx.x, M, red, res);
    if (threadIdx.x == 0)
        for (int c = 0; c < 4; ++c) per_clip[(size_t)blockIdx.x * 4 + c] = res[c];
    if (acc == nullptr || blockIdx.x != 0) return;
    // workgroup 0: the batch means.  It recomputes the other clips' values itself (same code, same order: the same
    // fp32 numbers their own workgroups write) instead of waiting for them — no inter-workgroup ordering, no atomics.
    double sum[4] = {0., 0., 0., 0.};
    for (int b = 0; b < B; ++b) {
        if (b > 0) met_clip_values(part, b, M, red, res);
        if (threadIdx.x == 0)
            for (int c = 0; c < 4; ++c) sum[c] += (double)res[c];
    }
    if (threadIdx.x == 0) {
        for (int c = 0; c < 4; ++c) acc[c] += sum[c] / (double)B;
        acc[4] += 1.0;
    }
}

}  // namespace
}  // namespace vmasr

using namespace vmasr;

VMASR_EXPORT size_t vmasr_metrics_workspace(int32_t B, int32_t T, int32_t n_fft, int32_t hop) {
    if (B <= 0 || T <= 0 || n_fft <= 0 || hop <= 0) return 0;
    return (size_t)B * (size_t)(1 + T / hop) * kVals * sizeof(float);
}

VMASR_EXPORT int vmasr_metrics(const float *out, const float *tgt, const int64_t *hf, float *per_clip, double *acc, int32_t B,
                               int32_t T, int32_t n_fft, int32_t hop, void *ws, size_t ws_bytes, vmasr_stream_t stream) {
    VMASR_REQUIRE(n_fft >= 64 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0, VMASR_EINVAL,
                  "metrics: n_fft must be a power of two in [64, 2048] (got %d)", n_fft);
    VMASR_REQUIRE(hop > 0, VMASR_EINVAL, "metrics: need hop > 0");
    VMASR_REQUIRE(out && tgt && hf && per_clip, VMASR_EINVAL, "metrics: null tensor");
    VMASR_REQUIRE(B > 0 && B <= 65535 && T > n_fft / 2, VMASR_EINVAL,
                  "metrics: need 0 < B <= 65535 and T > n_fft/2 (reflect padding)");
    VMASR_REQUIRE(ws && ws_bytes >= vmasr_metrics_workspace(B, T, n_fft, hop), VMASR_ENOSPACE, "metrics: workspace too small");
    const int M = 1 + T / hop;
    const size_t sm = met_smem_bytes(n_fft);     // <= 48 KB, plus 80 B static: inside the default dynamic-LDS limit
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *part = static_cast<float *>(ws);
    const double pbytes = (double)B * M * kVals * 4.0;
    VMASR_LAUNCH(VMASR_K_METRICS, 2.0 * B * T * 4.0 + pbytes, metrics_frames_kernel, dim3((M + kMF - 1) / kMF, B), dim3(kThreads),
                 sm, st, out, tgt, hf, part, T, n_fft, hop, M);
    VMASR_LAUNCH(VMASR_K_METRICS, pbytes + B * 16.0, metrics_finish_kernel, dim3(B), dim3(kThreads), 0, st,
                 static_cast<const float *>(part), per_clip, acc, B, M);
    return check_launch("metrics");
}
