// dconv1d.hip — the scale discriminator's dense tail: stride-1, groups-1 1-D convolutions (8h -> 8h k 5 + GELU, 8h -> 1 k 3), forward
// and both gradients.
//
// Reference: model/discriminator.py:239-258 — the last two layers of a ScaleDiscriminator,
//   y[b, o, t]  = bias[o] + sum_{c < Cin} sum_{j < k} w[o, c, j] x[b, c, t + j - pad]           (x zero outside [0, L)),  T = L + 2 pad - k + 1
//   dx[b, c, p] = sum_o sum_j w[o, c, j] g[b, o, p - j + pad]                                   g = gy GELU'(pre)  (or gy without the activation)
//   dw[o, c, j] = sum_{b, t} g[b, o, t] x[b, c, t + j - pad]        db[o] = sum_{b, t} g[b, o, t]
// on channel-first fp32 maps (B, C, L).  The maps are short (<= 120 positions at the workload) and the channels many (1024), so these
// are GEMMs of M = 1024, K = 5120 over a few hundred columns: the parallelism comes from splitting K, not from output tiles.
//
// Arithmetic: v_mfma_f32_16x16x4_f32 — exact fp32 products, fp32 accumulation; operand layout and conventions as in gconv1d.hip
// (A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15], D[m = 4 (lane >> 4) + r][n = lane & 15] in register r; zero operands
// past an edge; the 4 k of an MFMA on 4 consecutive taps, k rounded up with zero weights; the window of a channel chunk staged in LDS
// once and walked by tap offset, no im2col).
//
//   fwd   : block = (64 output channels: 16 per wave) x (16 NT positions of one batch row, NT = 2 / 4 / 8 by the map's length) x (one
//           slab of the input channels).  K walks (channel, tap) in chunks of 16 channels.  One slab: the epilogue adds the bias, writes
//           pre (kept for the backward) and y = GELU(pre), or y alone.  S > 1 slabs (few output tiles): every slab writes its partial to
//           a workspace and a second launch adds the S partials IN SLAB ORDER and applies the same epilogue.
//   dgrad : at stride 1 the same GEMM with the roles of the channels swapped and the taps reversed: dx = conv(g, w'[c, o, j] =
//           w[o, c, k - 1 - j], pad' = k - 1 - pad).  The SAME kernel: only the staging differs (the weight chunk is written to LDS
//           transposed and reversed; g = gy GELU'(pre) is formed while the gradient window is staged: no g tensor reaches memory).
//   wgrad : M = o (64 per block, 16 per wave), N = 32 input channels x the k taps (one accumulator tile per tap: no padded taps),
//           K = (b, t) in units of 32 positions of one batch row.  Enough (o, c) tiles: one workgroup owns the whole K of its tile and
//           writes dw itself.  Few tiles: the units are cut into S slabs, partials in the workspace, added in slab order by a second
//           launch.  db rides along: the workgroups of channel tile 0 sum their staged gradient rows per output channel.
// No float atomics anywhere: every result is bit-identical from call to call.
#include <algorithm>

#include "common.h"

namespace vmasr {
namespace {

typedef float dc_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kDcKMax = 8;                                // most taps
constexpr int kDcMR = 64;                                 // M tile: output (fwd, wgrad) / input (dgrad) channels per block, 16 per wave
constexpr int kDcCC = 16;                                 // K chunk: channels per LDS stage (fwd, dgrad)
constexpr int kDcTN = 128;                                // largest position tile (NT = 8); 64 and 32 for shorter maps
constexpr int kDcRSMax = 132;                             // fwd: largest LDS row of one M row's weights (dc_row_stride(kDcKMax))
constexpr int kDcXWMax = kDcTN + kDcKMax - 1;             // fwd: staged positions per channel
constexpr int kDcBlocks = 512;                            // workgroups a launch aims for (sets the slab counts): 2 per CU
constexpr int kDcSMax = 64;                               // fwd / dgrad: most K slabs
constexpr int kDcTK = 32;                                 // wgrad: positions per K unit
constexpr int kDcWC = 32;                                 // wgrad: input channels per block (2 tiles of 16)
constexpr int kDcGS = kDcTK + 4;                          // wgrad: LDS row of one output channel's gradient (36: conflict-free A reads)
constexpr int kDcXS = 44;                                 // wgrad: LDS row of one input channel (>= 32 + 7; 44: conflict-free B reads)

// M = channels of the result, Kc = channels summed over; Ls / Lo = length of the staged source map / of the result
struct DcGeom {
    int B, M, Kc, Ls, Lo, k, kp, pad, rs, cps, S;
};

struct DcWGeom {
    int B, Cin, Cout, L, T, k, pad, nT, ups, S, nct;
};

__device__ __forceinline__ dc_f32x4 dc_mma(float a, float b, dc_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// grid (ceil(Lo / 16 NT) * S, ceil(M / 64), B).  DG = false: src = x, w (M, Kc, k).  DG = true: src = gy, spre = pre or NULL, w (Kc, M, k).
// part != NULL: the slab's partial (S, B, M, Lo) instead of the epilogue.
template <int NT, bool DG>
__global__ __launch_bounds__(256) void dconv1d_gemm_kernel(const float *__restrict__ src, const float *__restrict__ spre, const float *__restrict__ w,
                                                           const float *__restrict__ bias, float *__restrict__ y, float *__restrict__ pre,
                                                           float *__restrict__ part, const DcGeom g, const int act) {
    constexpr int TN = 16 * NT;
    __shared__ float ws[kDcMR * kDcRSMax];
    __shared__ float xs[kDcCC * (TN + kDcKMax - 1)];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 15, lk = lane >> 4;
    const int sp = blockIdx.x % g.S, t0 = (blockIdx.x / g.S) * TN, m0 = blockIdx.y * kDcMR, b = blockIdx.z;
    const int mrows = min(kDcMR, g.M - m0), xw = TN + g.kp - 1, p0 = t0 - g.pad;
    const int chunks = (g.Kc + kDcCC - 1) / kDcCC, ch0 = sp * g.cps, ch1 = min(chunks, ch0 + g.cps);
    const float *sb = src + (size_t)b * g.Kc * g.Ls;
    const float *pb = (DG && spre) ? spre + (size_t)b * g.Kc * g.Ls : nullptr;
    dc_f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = dc_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = ch0; ch < ch1; ++ch) {
        const int c0 = ch * kDcCC, cc = min(kDcCC, g.Kc - c0);
        __syncthreads();
        if (!DG) {                                       // w[m0 + m][c0 .. c0 + cc)[0 .. k) is one contiguous run per row
            const int wn = cc * g.k;
            for (int i = tid; i < kDcMR * wn; i += 256) {    // rows past the last channel: zero weights
                const int m = i / wn, r = i - m * wn;
                ws[m * g.rs + r] = m < mrows ? w[((size_t)(m0 + m) * g.Kc + c0) * g.k + r] : 0.f;
            }
        } else {                                         // w[c0 + o][m0 .. m0 + mrows)[0 .. k) is one contiguous run per o; taps reversed
            const int wn = kDcMR * g.k;
            for (int i = tid; i < cc * wn; i += 256) {
                const int o = i / wn, r = i - o * wn, m = r / g.k, j = r - m * g.k;
                ws[m * g.rs + o * g.k + (g.k - 1 - j)] = m < mrows ? w[((size_t)(c0 + o) * g.M + m0) * g.k + r] : 0.f;
            }
        }
        for (int i = tid; i < cc * xw; i += 256) {       // the whole window, zero outside the map: the padded taps read it too
            const int c = i / xw, q = i - c * xw, p = p0 + q;
            float v = 0.f;
            if (p >= 0 && p < g.Ls) {
                const size_t off = (size_t)(c0 + c) * g.Ls + p;
                v = sb[off];
                if (DG && pb) v *= gelu_grad_f(pb[off]);
            }
            xs[c * xw + q] = v;
        }
        __syncthreads();
        if (wave * 16 < mrows) {                         // (a wave whose 16 rows are all past the edge has nothing to add)
            for (int c = 0; c < cc; ++c) {
                const float *xr = xs + c * xw + ln + lk;
                const float *wr = ws + (wave * 16 + ln) * g.rs + c * g.k + lk;
                for (int j0 = 0; j0 < g.kp; j0 += 4) {
                    const float av = j0 + lk < g.k ? wr[j0] : 0.f;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) acc[nt] = dc_mma(av, xr[nt * 16 + j0], acc[nt]);
                }
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int t = t0 + nt * 16 + ln;
        if (t >= g.Lo) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = wave * 16 + lk * 4 + r;
            if (m >= mrows) continue;
            const size_t off = ((size_t)b * g.M + m0 + m) * g.Lo + t;
            if (part) {
                part[(size_t)sp * g.B * g.M * g.Lo + off] = acc[nt][r];
                continue;
            }
            const float v = acc[nt][r] + (bias ? bias[m0 + m] : 0.f);
            if (act) { pre[off] = v; y[off] = gelu_f(v); }
            else y[off] = v;
        }
    }
}

// y[i] = epilogue(sum over the S partials in slab order): + bias, pre and GELU as the one-slab epilogue does
__global__ __launch_bounds__(256) void dconv1d_reduce_kernel(const float *__restrict__ part, const float *__restrict__ bias, float *__restrict__ y,
                                                             float *__restrict__ pre, const size_t n, const int M, const int Lo, const int S,
                                                             const int act) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = 0.f;
    for (int sp = 0; sp < S; ++sp) v += part[(size_t)sp * n + i];
    if (bias) v += bias[(i / Lo) % M];
    if (act) { pre[i] = v; y[i] = gelu_f(v); }
    else y[i] = v;
}

// grid (ceil(Cout / 64) * nct, S), nct = ceil(Cin / 32) (1 when only db is wanted); slab sp owns the K units [sp ups, (sp + 1) ups) of
// the B * nT units (b, 32 outputs).  out_w (S, Cout, Cin, k) / out_b (S, Cout): the workspace, or dw / db themselves when S == 1.
__global__ __launch_bounds__(256) void dconv1d_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ gy, const float *__restrict__ pre,
                                                            float *__restrict__ out_w, float *__restrict__ out_b, const DcWGeom g) {
    __shared__ float gs[kDcMR * kDcGS];
    __shared__ float xs[kDcWC * kDcXS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 15, lk = lane >> 4;
    const int ctile = blockIdx.x % g.nct, o0 = (blockIdx.x / g.nct) * kDcMR, c0 = ctile * kDcWC, sp = blockIdx.y;
    const int mrows = min(kDcMR, g.Cout - o0), cc = min(kDcWC, g.Cin - c0), xw = kDcTK + g.k - 1;
    const int total = g.B * g.nT, u0 = sp * g.ups, u1 = min(total, u0 + g.ups);
    dc_f32x4 acc[2][kDcKMax];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int j = 0; j < kDcKMax; ++j) acc[ct][j] = dc_f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int u = u0; u < u1; ++u) {
        const int b = u / g.nT, t0 = (u - b * g.nT) * kDcTK, p0 = t0 - g.pad;
        __syncthreads();
        for (int i = tid; i < kDcMR * kDcTK; i += 256) {
            const int m = i / kDcTK, tt = i - m * kDcTK, t = t0 + tt;
            float v = 0.f;
            if (m < mrows && t < g.T) {
                const size_t off = ((size_t)b * g.Cout + o0 + m) * g.T + t;
                v = gy[off];
                if (pre) v *= gelu_grad_f(pre[off]);
            }
            gs[m * kDcGS + tt] = v;
        }
        if (out_w)
            for (int i = tid; i < kDcWC * xw; i += 256) {
                const int c = i / xw, q = i - c * xw, p = p0 + q;
                xs[c * kDcXS + q] = (c < cc && p >= 0 && p < g.L) ? x[((size_t)b * g.Cin + c0 + c) * g.L + p] : 0.f;
            }
        __syncthreads();
        if (ctile == 0 && out_b && tid < mrows) {         // the bias gradient: one thread per output channel, a fixed order
            float s = 0.f;
            for (int tt = 0; tt < kDcTK; ++tt) s += gs[tid * kDcGS + tt];
            bsum += s;
        }
        if (out_w && wave * 16 < mrows) {
#pragma unroll 2
            for (int tt = 0; tt < kDcTK; tt += 4) {
                const float av = gs[(wave * 16 + ln) * kDcGS + tt + lk];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    if (ct * 16 >= cc) continue;
                    const float *xr = xs + (ct * 16 + ln) * kDcXS + tt + lk;
#pragma unroll
                    for (int j = 0; j < kDcKMax; ++j)
                        if (j < g.k) acc[ct][j] = dc_mma(av, xr[j], acc[ct][j]);
                }
            }
        }
    }
    if (out_w && wave * 16 < mrows) {
        float *ow = out_w + (size_t)sp * g.Cout * g.Cin * g.k;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int c = ct * 16 + ln;
            if (c >= cc) continue;
#pragma unroll
            for (int j = 0; j < kDcKMax; ++j) {
                if (j >= g.k) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = wave * 16 + lk * 4 + r;
                    if (m < mrows) ow[((size_t)(o0 + m) * g.Cin + c0 + c) * g.k + j] = acc[ct][j][r];
                }
            }
        }
    }
    if (ctile == 0 && out_b && tid < mrows) out_b[(size_t)sp * g.Cout + o0 + tid] = bsum;
}

// dw[i] = sum over the S partials in slab order; db likewise.  Either output may be NULL.
__global__ __launch_bounds__(256) void dconv1d_wgrad_reduce_kernel(const float *__restrict__ part_w, const float *__restrict__ part_b,
                                                                   float *__restrict__ dw, float *__restrict__ db, const size_t nw, const int nb,
                                                                   const int S) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nw) {
        if (!dw) return;
        float s = 0.f;
        for (int sp = 0; sp < S; ++sp) s += part_w[(size_t)sp * nw + i];
        dw[i] = s;
    } else if (i < nw + nb && db) {
        const size_t o = i - nw;
        float s = 0.f;
        for (int sp = 0; sp < S; ++sp) s += part_b[(size_t)sp * nb + o];
        db[o] = s;
    }
}

// ---- host side: ONE predicate for the queries and the launchers -------------------------------------------------------------------
bool dc_shape_ok(int Cin, int Cout, int groups, int k, int stride) {
    return groups == 1 && stride == 1 && k >= 1 && k <= kDcKMax && Cin >= 1 && Cout >= 1 && Cin <= 65536 && Cout <= 65536;
}

bool dc_launch_ok(int Cin, int Cout, int groups, int k, int stride, int pad, int B, int64_t L) {
    if (!(dc_shape_ok(Cin, Cout, groups, k, stride) && pad >= 0 && pad < k && B > 0 && B <= 65535 && L > 0 && L <= (int64_t(1) << 28) &&
          L + 2 * pad >= k))
        return false;
    // the weight gradient counts its K units (b, 32 outputs) in 32-bit: u0 + ups <= 2 * B * ceil(T / 32) must fit
    const int64_t T = L + 2 * pad - k + 1;
    return (int64_t)B * ((T + kDcTK - 1) / kDcTK) <= (int64_t(1) << 30);
}

int dc_row_stride(int k) { return (kDcCC * k + 27) / 32 * 32 + 4; }      // >= 16 k + 3 (the padded taps stay inside the row), = 4 mod 32

int dc_nt(int Lo) { return Lo <= 32 ? 2 : Lo <= 64 ? 4 : 8; }

// the forward's (dgrad = false) or the input gradient's GEMM: tile choice and K slabs
DcGeom dc_geom(int Cin, int Cout, int k, int pad, int B, int64_t L, bool dgrad) {
    const int T = (int)(L + 2 * pad - k + 1);
    DcGeom g{};
    g.B = B; g.k = k; g.kp = (k + 3) / 4 * 4; g.rs = dc_row_stride(k);
    if (!dgrad) { g.M = Cout; g.Kc = Cin; g.Ls = (int)L; g.Lo = T; g.pad = pad; }
    else { g.M = Cin; g.Kc = Cout; g.Ls = T; g.Lo = (int)L; g.pad = k - 1 - pad; }
    const int TN = 16 * dc_nt(g.Lo);
    const int64_t tiles = (int64_t)((g.Lo + TN - 1) / TN) * ((g.M + kDcMR - 1) / kDcMR) * B;
    const int chunks = (g.Kc + kDcCC - 1) / kDcCC;
    const int64_t want = std::min<int64_t>(std::min<int64_t>(chunks, kDcSMax), std::max<int64_t>(1, (kDcBlocks + tiles - 1) / tiles));
    g.cps = (int)((chunks + want - 1) / want);
    g.S = (chunks + g.cps - 1) / g.cps;                 // no empty slab
    return g;
}

size_t dc_gemm_ws_floats(const DcGeom &g) { return g.S > 1 ? (size_t)g.S * g.B * g.M * g.Lo : 0; }

DcWGeom dc_wgeom(int Cin, int Cout, int k, int pad, int B, int64_t L, bool want_dw) {
    DcWGeom g{};
    g.B = B; g.Cin = Cin; g.Cout = Cout; g.L = (int)L; g.T = (int)(L + 2 * pad - k + 1); g.k = k; g.pad = pad;
    g.nT = (g.T + kDcTK - 1) / kDcTK;
    const int nct = (Cin + kDcWC - 1) / kDcWC;
    g.nct = want_dw ? nct : 1;                          // db alone: the workgroups of channel tile 0, the SAME slabs (the same sums)
    const int64_t blocks = (int64_t)((Cout + kDcMR - 1) / kDcMR) * nct, total = (int64_t)B * g.nT;
    const int64_t want = std::min<int64_t>(std::max<int64_t>(1, (kDcBlocks + blocks - 1) / blocks), std::min<int64_t>(total, 1024));
    g.ups = (int)((total + want - 1) / want);
    g.S = (int)((total + g.ups - 1) / g.ups);           // no empty slab
    return g;
}

size_t dc_wgrad_ws_floats(const DcWGeom &g) { return g.S > 1 ? (size_t)g.S * ((size_t)g.Cout * g.Cin * g.k + (size_t)g.Cout) : 0; }

template <bool DG>
void dc_launch_gemm(int kid, double bytes, const DcGeom &g, hipStream_t st, const float *src, const float *spre, const float *w, const float *bias,
                    float *y, float *pre, float *part, int act) {
    const int nt = dc_nt(g.Lo), TN = 16 * nt;
    const dim3 grid((unsigned)((g.Lo + TN - 1) / TN) * (unsigned)g.S, (unsigned)((g.M + kDcMR - 1) / kDcMR), (unsigned)g.B);
    switch (nt) {
        case 2: VMASR_LAUNCH(kid, bytes, (dconv1d_gemm_kernel<2, DG>), grid, dim3(256), 0, st, src, spre, w, bias, y, pre, part, g, act); break;
        case 4: VMASR_LAUNCH(kid, bytes, (dconv1d_gemm_kernel<4, DG>), grid, dim3(256), 0, st, src, spre, w, bias, y, pre, part, g, act); break;
        default: VMASR_LAUNCH(kid, bytes, (dconv1d_gemm_kernel<8, DG>), grid, dim3(256), 0, st, src, spre, w, bias, y, pre, part, g, act); break;
    }
    if (part) {
        const size_t n = (size_t)g.B * g.M * g.Lo;
        VMASR_LAUNCH(VMASR_K_DCONV1D_REDUCE, 4.0 * ((double)g.S + (act ? 2.0 : 1.0)) * (double)n, dconv1d_reduce_kernel,
                     dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, bias, y, pre, n, g.M, g.Lo, g.S, act);
    }
}

}  // namespace
}  // namespace vmasr

using namespace vmasr;

VMASR_EXPORT int32_t vmasr_dconv1d_pos_tile(void) { return kDcTN; }
VMASR_EXPORT int32_t vmasr_dconv1d_m_tile(void) { return kDcMR; }
VMASR_EXPORT int32_t vmasr_dconv1d_k_chunk(void) { return kDcCC; }
VMASR_EXPORT int32_t vmasr_dconv1d_max_taps(void) { return kDcKMax; }

VMASR_EXPORT int vmasr_dconv1d_supported(int32_t Cin, int32_t Cout, int32_t groups, int32_t k, int32_t stride) {
    return dc_shape_ok(Cin, Cout, groups, k, stride) ? 1 : 0;
}

VMASR_EXPORT int vmasr_dconv1d_supported_launch(int32_t Cin, int32_t Cout, int32_t groups, int32_t k, int32_t stride, int32_t pad, int32_t B,
                                                int64_t L) {
    return dc_launch_ok(Cin, Cout, groups, k, stride, pad, B, L) ? 1 : 0;
}

VMASR_EXPORT int32_t vmasr_dconv1d_fwd_slabs(int32_t Cin, int32_t Cout, int32_t groups, int32_t k, int32_t stride, int32_t pad, int32_t B,
                                             int64_t L) {
    return dc_launch_ok(Cin, Cout, groups, k, stride, pad, B, L) ? dc_geom(Cin, Cout, k, pad, B, L, false).S : 0;
}

VMASR_EXPORT size_t vmasr_dconv1d_fwd_workspace(int32_t Cin, int32_t Cout, int32_t groups, int32_t k, int32_t stride, int32_t pad, int32_t B,
                                                int64_t L) {
    if (!dc_launch_ok(Cin, Cout, groups, k, stride, pad, B, L)) return 0;
    return dc_gemm_ws_floats(dc_geom(Cin, Cout, k, pad, B, L, false)) * sizeof(float);
}

VMASR_EXPORT size_t vmasr_dconv1d_dgrad_workspace(int32_t Cin, int32_t Cout, int32_t groups, int32_t k, int32_t stride, int32_t pad, int32_t B,
                                                  int64_t L) {
    if (!dc_launch_ok(Cin, Cout, groups, k, stride, pad, B, L)) return 0;
    return dc_gemm_ws_floats(dc_geom(Cin, Cout, k, pad, B, L, true)) * sizeof(float);
}

VMASR_EXPORT size_t vmasr_dconv1d_wgrad_workspace(int32_t Cin, int32_t Cout, int32_t groups, int32_t k, int32_t stride, int32_t pad, int32_t B,
                                                  int64_t L) {
    if (!dc_launch_ok(Cin, Cout, groups, k, stride, pad, B, L)) return 0;
    return dc_wgrad_ws_floats(dc_wgeom(Cin, Cout, k, pad, B, L, true)) * sizeof(float);
}

#define VMASR_DC_CHECK(what)                                                                                                              \
    VMASR_REQUIRE(dc_launch_ok(Cin, Cout, groups, k, stride, pad, B, L), VMASR_EINVAL,                                                      \
                  what ": unsupported shape (Cin=%d Cout=%d groups=%d k=%d stride=%d pad=%d B=%d L=%lld): needs groups 1, stride 1, "        \
                       "1 <= k <= 8, 1 <= Cin, Cout <= 65536, 0 <= pad < k, 1 <= B <= 65535, max(1, k - 2 pad) <= L <= 2^28, "               \
                       "B * ceil(T / 32) <= 2^30",                                                                                           \
                  Cin, Cout, groups, k, stride, pad, B, (long long)L)

#define VMASR_DC_WS(what, need)                                                                                                            \
    VMASR_REQUIRE((need) == 0 || (ws && ws_bytes >= (need) && aligned_to(ws, 4)), VMASR_EINVAL,                                              \
                  what ": workspace missing, too small or unaligned (%zu bytes, need %zu)", ws_bytes, (size_t)(need))

VMASR_EXPORT int vmasr_dconv1d_fwd(const float *x, const float *w, const float *bias, float *y, float *pre, void *ws, size_t ws_bytes, int32_t B,
                                   int32_t Cin, int32_t Cout, int32_t groups, int64_t L, int32_t k, int32_t stride, int32_t pad, int32_t act,
                                   vmasr_stream_t stream) {
    VMASR_REQUIRE(x && w && y && (pre || !act), VMASR_EINVAL, "dconv1d_fwd: null tensor (x, w, y; pre with the activation)");
    VMASR_DC_CHECK("dconv1d_fwd");
    const DcGeom g = dc_geom(Cin, Cout, k, pad, B, L, false);
    const size_t need = dc_gemm_ws_floats(g) * sizeof(float);
    VMASR_DC_WS("dconv1d_fwd", need);
    const double bytes = 4.0 * ((double)B * Cin * L + (double)Cout * Cin * k + (double)B * Cout * g.Lo * (act ? 2.0 : 1.0));
    dc_launch_gemm<false>(VMASR_K_DCONV1D_FWD, bytes, g, static_cast<hipStream_t>(stream), x, nullptr, w, bias, y, pre,
                          need ? static_cast<float *>(ws) : nullptr, act);
    return check_launch("dconv1d_fwd");
}

VMASR_EXPORT int vmasr_dconv1d_dgrad(const float *gy, const float *pre, const float *w, float *dx, void *ws, size_t ws_bytes, int32_t B,
                                     int32_t Cin, int32_t Cout, int32_t groups, int64_t L, int32_t k, int32_t stride, int32_t pad,
                                     vmasr_stream_t stream) {
    VMASR_REQUIRE(gy && w && dx, VMASR_EINVAL, "dconv1d_dgrad: null tensor (gy, w, dx)");
    VMASR_DC_CHECK("dconv1d_dgrad");
    const DcGeom g = dc_geom(Cin, Cout, k, pad, B, L, true);
    const size_t need = dc_gemm_ws_floats(g) * sizeof(float);
    VMASR_DC_WS("dconv1d_dgrad", need);
    const double bytes = 4.0 * ((double)B * Cin * L + (double)Cout * Cin * k + (double)B * Cout * g.Ls * (pre ? 2.0 : 1.0));
    dc_launch_gemm<true>(VMASR_K_DCONV1D_DGRAD, bytes, g, static_cast<hipStream_t>(stream), gy, pre, w, nullptr, dx, nullptr,
                         need ? static_cast<float *>(ws) : nullptr, 0);
    return check_launch("dconv1d_dgrad");
}

VMASR_EXPORT int vmasr_dconv1d_wgrad(const float *x, const float *gy, const float *pre, float *dw, float *db, void *ws, size_t ws_bytes, int32_t B,
                                     int32_t Cin, int32_t Cout, int32_t groups, int64_t L, int32_t k, int32_t stride, int32_t pad,
                                     vmasr_stream_t stream) {
    VMASR_REQUIRE(x && gy && (dw || db), VMASR_EINVAL, "dconv1d_wgrad: null tensor (x, gy; dw or db)");
    VMASR_DC_CHECK("dconv1d_wgrad");
    const DcWGeom g = dc_wgeom(Cin, Cout, k, pad, B, L, dw != nullptr);
    const size_t nw = (size_t)Cout * Cin * k;
    const size_t need = g.S > 1 ? (size_t)g.S * (nw + (size_t)Cout) * sizeof(float) : 0;
    VMASR_DC_WS("dconv1d_wgrad", need);
    float *part_w = static_cast<float *>(ws), *part_b = need ? part_w + (size_t)g.S * nw : nullptr;
    const dim3 grid((unsigned)((Cout + kDcMR - 1) / kDcMR) * (unsigned)g.nct, (unsigned)g.S);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double bytes = 4.0 * ((double)B * Cin * L + (double)B * Cout * g.T * (pre ? 2.0 : 1.0) + (double)g.S * nw);
    if (need == 0) {
        VMASR_LAUNCH(VMASR_K_DCONV1D_WGRAD, bytes, dconv1d_wgrad_kernel, grid, dim3(256), 0, st, x, gy, pre, dw, db, g);
    } else {
        VMASR_LAUNCH(VMASR_K_DCONV1D_WGRAD, bytes, dconv1d_wgrad_kernel, grid, dim3(256), 0, st, x, gy, pre, dw ? part_w : nullptr,
                     db ? part_b : nullptr, g);
        const size_t n = nw + (size_t)Cout;
        VMASR_LAUNCH(VMASR_K_DCONV1D_WGRAD_REDUCE, 4.0 * ((double)g.S + 1.0) * (double)n, dconv1d_wgrad_reduce_kernel,
                     dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part_w, part_b, dw, db, nw, (int)Cout, g.S);
    }
    return check_launch("dconv1d_wgrad");
}
