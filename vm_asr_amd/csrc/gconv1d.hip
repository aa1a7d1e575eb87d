// gconv1d.hip — the scale discriminator's strided grouped 1-D convolutions (k 41, stride 4, groups 4 / 16), forward and both gradients.
//
// Reference: model/discriminator.py:189-238 — five of the eight layers of a ScaleDiscriminator are
//   y[b, g Co + o, t] = bias + sum_{c < Ci} sum_{j < 41} w[g Co + o, c, j] x[b, g Ci + c, 4 t + j - pad]        (x zero outside [0, L))
// on channel-first fp32 maps (B, C, L), each followed by an exact GELU.  Per group this is a GEMM with M = Co, N = positions and
// K = 41 Ci whose B operand is a sliding window of x: a tile of 128 outputs reads 4 * 127 + 41 input positions of a channel, every one of
// them ~10 times, so the window is staged in LDS once per channel chunk and the 41 taps are walked as LDS offsets (no im2col).
//
// Arithmetic: v_mfma_f32_16x16x4_f32 — exact fp32 products, fp32 accumulation, the numerics of an fp32 FMA loop.  One element per lane
// and operand: A[m = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15], D[m = 4 (lane >> 4) + r][n = lane & 15] in register r.
// Rows / columns past the problem's edge are zero operands (A side) or unwritten results, so every per-group (Ci, Co) pair runs, down
// to (1, 2); the small pairs simply waste most of a tile.
//
//   fwd   : block = (128 outputs) x (16 MT output channels of one group) x (one batch row); K walks (channel, tap) with the 4 k of an
//           MFMA on 4 consecutive taps (41 -> 44, the 3 extra taps have zero weights): B = xs[c][4 n + j], 64 consecutive LDS words.
//           Epilogue: + bias -> pre (kept for the backward), GELU -> y; or + bias -> y alone.
//   dgrad : by residue classes of the stride.  With p + pad = 4 q + r:  dx[c, p] = sum_o sum_i w[o, c, r + 4 i] g[o, q - i]  (i < 11):
//           per residue a GEMM with M = input channel, N = q, K = (o, i); wave r of a block owns residue r.  g = gy GELU'(pre) is formed
//           while the gradient tile is staged.
//   wgrad : dw[o, c, j] = sum_{b, t} g[b, o, t] x[b, c, 4 t + j - pad]: M = o, N = j (41 -> 48), K = (b, t).  The (b, t) range is cut
//           into S slabs, every slab writes its own partial to a workspace and a second launch adds the S partials IN SLAB ORDER: no float
//           atomics anywhere, so dw and db are bit-identical from run to run (VMASR_DETERMINISTIC needs no second path).
//           db rides along: the workgroups of channel chunk 0 sum their staged gradient tile per output channel.
#include <algorithm>

#include "common.h"

namespace vmasr {
namespace {

typedef float gc_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGcK = 41, kGcS = 4, kGcKP = 44;            // taps, stride, taps rounded up to the MFMA's 4 k
constexpr int kGcCC = 4;                                  // input channels per LDS stage (fwd, wgrad)
constexpr int kGcTN = 128;                                // fwd: outputs per block (4 waves x 2 tiles of 16)
constexpr int kGcWL = (kGcTN - 1) * kGcS + kGcKP;         // fwd: staged input positions per channel
constexpr int kGcRS = kGcCC * kGcK;                       // fwd: LDS row of one output channel's weights (164 = 4 mod 32)
constexpr int kGcQN = 64;                                 // dgrad: q positions per block (4 tiles of 16 per wave)
constexpr int kGcOC = 4;                                  // dgrad: output channels per LDS stage
constexpr int kGcGW = kGcQN + 12;                         // dgrad: staged gradient positions per output channel
constexpr int kGcTK = 64;                                 // wgrad: outputs per K unit
constexpr int kGcGS = kGcTK + 4;                          // wgrad: LDS row of one output channel's gradient (68 = 4 mod 64: no conflicts)
constexpr int kGcXW = (kGcTK - 1) * kGcS + 48;            // wgrad: staged input positions per channel
constexpr int kGcWgradBlocks = 2048;                      // wgrad: workgroups a launch aims for (sets the slab count)

struct GcGeom {
    int B, Cin, Cout, G, Ci, Co, L, T, pad;
};

__device__ __forceinline__ gc_f32x4 gc_mma(float a, float b, gc_f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// grid (ceil(T / 128), G * ceil(Co / 16 MT), B)
template <int MT>
__global__ __launch_bounds__(256) void gconv1d_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                          float *__restrict__ y, float *__restrict__ pre, const GcGeom g, const int act) {
    constexpr int MR = 16 * MT;
    __shared__ float ws[MR * kGcRS + 8];
    __shared__ float xs[kGcCC * kGcWL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 15, lk = lane >> 4;
    const int mtiles = (g.Co + MR - 1) / MR;
    const int grp = blockIdx.y / mtiles, o0 = (blockIdx.y % mtiles) * MR, b = blockIdx.z, t0 = blockIdx.x * kGcTN;
    const int mrows = min(MR, g.Co - o0);
    const int p0 = t0 * kGcS - g.pad;
    const float *xg = x + ((size_t)b * g.Cin + (size_t)grp * g.Ci) * g.L;
    const float *wg = w + ((size_t)grp * g.Co + o0) * g.Ci * kGcK;
    gc_f32x4 acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt][0] = acc[mt][1] = gc_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < g.Ci; c0 += kGcCC) {
        const int cc = min(kGcCC, g.Ci - c0), wn = cc * kGcK;
        __syncthreads();
        for (int i = tid; i < MR * wn; i += 256) {       // rows past the group's last output channel: zero weights
            const int m = i / wn, r = i - m * wn;
            ws[m * kGcRS + r] = m < mrows ? wg[((size_t)m * g.Ci + c0) * kGcK + r] : 0.f;
        }
        for (int i = tid; i < cc * kGcWL; i += 256) {    // the whole window, zero outside [0, L): the 3 padded taps read it too
            const int c = i / kGcWL, p = p0 + (i - c * kGcWL);
            xs[i] = (p >= 0 && p < g.L) ? xg[(size_t)(c0 + c) * g.L + p] : 0.f;
        }
        __syncthreads();
        for (int c = 0; c < cc; ++c) {
            const float *xr = xs + c * kGcWL + (wave * 32 + ln) * kGcS + lk;
            const float *wr = ws + ln * kGcRS + c * kGcK + lk;
#pragma unroll
            for (int j0 = 0; j0 < kGcKP; j0 += 4) {
                const bool tap = j0 + lk < kGcK;
                const float b0 = xr[j0], b1 = xr[16 * kGcS + j0];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const float av = tap ? wr[mt * 16 * kGcRS + j0] : 0.f;
                    acc[mt][0] = gc_mma(av, b0, acc[mt][0]);
                    acc[mt][1] = gc_mma(av, b1, acc[mt][1]);
                }
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int t = t0 + wave * 32 + nt * 16 + ln;
        if (t >= g.T) continue;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mt * 16 + lk * 4 + r;
                if (m >= mrows) continue;
                const int oc = grp * g.Co + o0 + m;
                const float v = acc[mt][nt][r] + (bias ? bias[oc] : 0.f);
                const size_t off = ((size_t)b * g.Cout + oc) * g.T + t;
                if (act) { pre[off] = v; y[off] = gelu_f(v); }
                else y[off] = v;
            }
    }
}

// grid (ceil(nq / 64), G * ceil(Ci / 16 MT), B), nq = ceil((L + pad) / 4); wave r = residue r of p + pad
template <int MT>
__global__ __launch_bounds__(256) void gconv1d_dgrad_kernel(const float *__restrict__ gy, const float *__restrict__ pre, const float *__restrict__ w,
                                                            float *__restrict__ dx, const GcGeom g) {
    constexpr int MR = 16 * MT;
    __shared__ float ws[kGcOC * MR * kGcK + 8];
    __shared__ float gs[kGcOC * kGcGW];
    const int tid = threadIdx.x, lane = tid & 63, res = tid >> 6, ln = lane & 15, lk = lane >> 4;
    const int ctiles = (g.Ci + MR - 1) / MR;
    const int grp = blockIdx.y / ctiles, c0 = (blockIdx.y % ctiles) * MR, b = blockIdx.z, q0 = blockIdx.x * kGcQN;
    const int crows = min(MR, g.Ci - c0);
    const int tb = q0 - 11;                               // first staged output position (i = 0 .. 11 behind q)
    gc_f32x4 acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = gc_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int oc0 = 0; oc0 < g.Co; oc0 += kGcOC) {
        const int occ = min(kGcOC, g.Co - oc0);
        __syncthreads();
        for (int i = tid; i < occ * MR * kGcK; i += 256) {      // w[o][c0 .. c0 + crows)[0 .. 41) is one contiguous run per o
            const int o = i / (MR * kGcK), r = i - o * (MR * kGcK);
            ws[i] = r < crows * kGcK ? w[(((size_t)grp * g.Co + oc0 + o) * g.Ci + c0) * kGcK + r] : 0.f;
        }
        for (int i = tid; i < occ * kGcGW; i += 256) {
            const int o = i / kGcGW, t = tb + (i - o * kGcGW);
            float v = 0.f;
            if (t >= 0 && t < g.T) {
                const size_t off = ((size_t)b * g.Cout + (size_t)grp * g.Co + oc0 + o) * g.T + t;
                v = gy[off];
                if (pre) v *= gelu_grad_f(pre[off]);
            }
            gs[i] = v;
        }
        __syncthreads();
        for (int o = 0; o < occ; ++o) {
#pragma unroll
            for (int ks = 0; ks < 3; ++ks) {
                const int i = ks * 4 + lk, j = res + 4 * i;
                const bool tap = j < kGcK;
                float av[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) av[mt] = tap ? ws[(o * MR + mt * 16 + ln) * kGcK + j] : 0.f;
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const float bv = gs[o * kGcGW + nt * 16 + ln + 11 - i];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = gc_mma(av[mt], bv, acc[mt][nt]);
                }
            }
        }
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int p = (q0 + nt * 16 + ln) * kGcS + res - g.pad;
        if (p < 0 || p >= g.L) continue;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = mt * 16 + lk * 4 + r;
                if (m < crows) dx[((size_t)b * g.Cin + (size_t)grp * g.Ci + c0 + m) * g.L + p] = acc[mt][nt][r];
            }
    }
}

// grid (G * ceil(Co / 16 MT) * ceil(Ci / 4), S); wave = input channel of the chunk; slab sp owns the K units [sp ups, (sp + 1) ups)
// of the B * nT units (b, 64 outputs).  part_w (S, Cout, Ci, 41), part_b (S, Cout).
template <int MT>
__global__ __launch_bounds__(256) void gconv1d_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ gy, const float *__restrict__ pre,
                                                            float *__restrict__ part_w, float *__restrict__ part_b, const GcGeom g, const int nT,
                                                            const int ups) {
    constexpr int MR = 16 * MT;
    __shared__ float gs[MR * kGcGS];
    __shared__ float xs[kGcCC * kGcXW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 15, lk = lane >> 4;
    const int mtiles = (g.Co + MR - 1) / MR, cchunks = (g.Ci + kGcCC - 1) / kGcCC;
    const int cchunk = blockIdx.x % cchunks, mtile = (blockIdx.x / cchunks) % mtiles, grp = blockIdx.x / (cchunks * mtiles);
    const int o0 = mtile * MR, c0 = cchunk * kGcCC, sp = blockIdx.y;
    const int mrows = min(MR, g.Co - o0), cc = min(kGcCC, g.Ci - c0);
    const int total = g.B * nT, u0 = sp * ups, u1 = min(total, u0 + ups);
    gc_f32x4 acc[MT][3];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt][0] = acc[mt][1] = acc[mt][2] = gc_f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    for (int u = u0; u < u1; ++u) {
        const int b = u / nT, t0 = (u - b * nT) * kGcTK, p0 = t0 * kGcS - g.pad;
        __syncthreads();
        for (int i = tid; i < MR * kGcTK; i += 256) {
            const int m = i / kGcTK, tt = i - m * kGcTK, t = t0 + tt;
            float v = 0.f;
            if (m < mrows && t < g.T) {
                const size_t off = ((size_t)b * g.Cout + (size_t)grp * g.Co + o0 + m) * g.T + t;
                v = gy[off];
                if (pre) v *= gelu_grad_f(pre[off]);
            }
            gs[m * kGcGS + tt] = v;
        }
        for (int i = tid; i < kGcCC * kGcXW; i += 256) {
            const int c = i / kGcXW, p = p0 + (i - c * kGcXW);
            xs[i] = (c < cc && p >= 0 && p < g.L) ? x[((size_t)b * g.Cin + (size_t)grp * g.Ci + c0 + c) * g.L + p] : 0.f;
        }
        __syncthreads();
        if (cchunk == 0 && tid < mrows) {                 // the bias gradient: one thread per output channel, a fixed order
            float s = 0.f;
            for (int tt = 0; tt < kGcTK; ++tt) s += gs[tid * kGcGS + tt];
            bsum += s;
        }
#pragma unroll 4
        for (int tt = 0; tt < kGcTK; tt += 4) {
            float av[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) av[mt] = gs[(mt * 16 + ln) * kGcGS + tt + lk];
#pragma unroll
            for (int jt = 0; jt < 3; ++jt) {
                const float bv = xs[wave * kGcXW + (tt + lk) * kGcS + jt * 16 + ln];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt][jt] = gc_mma(av[mt], bv, acc[mt][jt]);
            }
        }
    }
    if (wave < cc) {
#pragma unroll
        for (int jt = 0; jt < 3; ++jt) {
            const int j = jt * 16 + ln;
            if (j >= kGcK) continue;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = mt * 16 + lk * 4 + r;
                    if (m < mrows)
                        part_w[(((size_t)sp * g.Cout + (size_t)grp * g.Co + o0 + m) * g.Ci + c0 + wave) * kGcK + j] = acc[mt][jt][r];
                }
        }
    }
    if (cchunk == 0 && tid < mrows) part_b[(size_t)sp * g.Cout + (size_t)grp * g.Co + o0 + tid] = bsum;
}

// dw[i] = sum over the S partials in slab order; db likewise.  Either output may be NULL.
__global__ __launch_bounds__(256) void gconv1d_wgrad_reduce_kernel(const float *__restrict__ part_w, const float *__restrict__ part_b,
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

// ---- host side: ONE predicate for the query and the launchers ---------------------------------------------------------------------
bool gc_shape_ok(int Cin, int Cout, int groups, int k, int stride) {
    return groups > 0 && Cin > 0 && Cout > 0 && Cin % groups == 0 && Cout % groups == 0 && k == kGcK && stride == kGcS && Cin <= 65536 &&
           Cout <= 65536 && groups <= 4096;            // (grid.y = groups * channel tiles <= 65535)
}

bool gc_launch_ok(int Cin, int Cout, int groups, int k, int stride, int pad, int B, int64_t L) {
    if (!(gc_shape_ok(Cin, Cout, groups, k, stride) && pad >= 0 && pad < k && B > 0 && B <= 65535 && L > 0 && L <= (int64_t(1) << 28) &&
          L + 2 * pad >= k))
        return false;
    // the weight gradient counts its K units (b, 64 outputs) in 32-bit: u0 + ups <= 2 * B * ceil(T / 64) must fit
    const int64_t T = (L + 2 * pad - kGcK) / kGcS + 1;
    return (int64_t)B * ((T + kGcTK - 1) / kGcTK) <= (int64_t(1) << 30);
}

int gc_mt(int rows) { return rows <= 16 ? 1 : rows <= 32 ? 2 : 4; }

GcGeom gc_geom(int Cin, int Cout, int groups, int pad, int B, int64_t L) {
    GcGeom g{};
    g.B = B; g.Cin = Cin; g.Cout = Cout; g.G = groups; g.Ci = Cin / groups; g.Co = Cout / groups; g.L = (int)L; g.pad = pad;
    g.T = (int)((L + 2 * pad - kGcK) / kGcS + 1);
    return g;
}

struct GcSplit {
    int nT, ups, S;
    unsigned blocks;
};

GcSplit gc_split(const GcGeom &g) {
    const int MR = 16 * gc_mt(g.Co);
    GcSplit s{};
    s.blocks = (unsigned)g.G * (unsigned)((g.Co + MR - 1) / MR) * (unsigned)((g.Ci + kGcCC - 1) / kGcCC);
    s.nT = (g.T + kGcTK - 1) / kGcTK;
    const int64_t total = (int64_t)g.B * s.nT;
    int64_t want = std::min<int64_t>(std::max<int64_t>(1, (kGcWgradBlocks + s.blocks - 1) / s.blocks), std::min<int64_t>(total, 1024));
    s.ups = (int)((total + want - 1) / want);
    s.S = (int)((total + s.ups - 1) / s.ups);          // no empty slab
    return s;
}

size_t gc_ws_floats(const GcGeom &g, const GcSplit &s) { return (size_t)s.S * ((size_t)g.Cout * g.Ci * kGcK + (size_t)g.Cout); }

}  // namespace
}  // namespace vmasr

using namespace vmasr;

VMASR_EXPORT int vmasr_gconv1d_supported(int32_t Cin, int32_t Cout, int32_t groups, int32_t k, int32_t stride) {
    return gc_shape_ok(Cin, Cout, groups, k, stride) ? 1 : 0;
}

VMASR_EXPORT int vmasr_gconv1d_supported_launch(int32_t Cin, int32_t Cout, int32_t groups, int32_t k, int32_t stride, int32_t pad, int32_t B,
                                                int64_t L) {
    return gc_launch_ok(Cin, Cout, groups, k, stride, pad, B, L) ? 1 : 0;
}

VMASR_EXPORT size_t vmasr_gconv1d_wgrad_workspace(int32_t Cin, int32_t Cout, int32_t groups, int32_t k, int32_t stride, int32_t pad, int32_t B,
                                                  int64_t L) {
    if (!gc_launch_ok(Cin, Cout, groups, k, stride, pad, B, L)) return 0;
    const GcGeom g = gc_geom(Cin, Cout, groups, pad, B, L);
    return gc_ws_floats(g, gc_split(g)) * sizeof(float);
}

#define VMASR_GC_CHECK(what)                                                                                                            \
    VMASR_REQUIRE(gc_launch_ok(Cin, Cout, groups, k, stride, pad, B, L), VMASR_EINVAL,                                                    \
                  what ": unsupported shape (Cin=%d Cout=%d groups=%d k=%d stride=%d pad=%d B=%d L=%lld): needs k 41, stride 4, groups "   \
                       "dividing both channel counts, 0 <= pad < k, B <= 65535, k - 2 pad <= L <= 2^28, B * ceil(T / 64) <= 2^30",                                   \
                  Cin, Cout, groups, k, stride, pad, B, (long long)L)

VMASR_EXPORT int vmasr_gconv1d_fwd(const float *x, const float *w, const float *bias, float *y, float *pre, int32_t B, int32_t Cin, int32_t Cout,
                                   int32_t groups, int64_t L, int32_t k, int32_t stride, int32_t pad, int32_t act, vmasr_stream_t stream) {
    VMASR_REQUIRE(x && w && y && (pre || !act), VMASR_EINVAL, "gconv1d_fwd: null tensor (x, w, y; pre with the activation)");
    VMASR_GC_CHECK("gconv1d_fwd");
    const GcGeom g = gc_geom(Cin, Cout, groups, pad, B, L);
    const int mt = gc_mt(g.Co), MR = 16 * mt;
    const dim3 grid((unsigned)((g.T + kGcTN - 1) / kGcTN), (unsigned)(g.G * ((g.Co + MR - 1) / MR)), (unsigned)B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double bytes = 4.0 * ((double)B * Cin * L + (double)Cout * g.Ci * kGcK + (double)B * Cout * g.T * (act ? 2.0 : 1.0));
    switch (mt) {
        case 1: VMASR_LAUNCH(VMASR_K_GCONV1D_FWD, bytes, gconv1d_fwd_kernel<1>, grid, dim3(256), 0, st, x, w, bias, y, pre, g, act); break;
        case 2: VMASR_LAUNCH(VMASR_K_GCONV1D_FWD, bytes, gconv1d_fwd_kernel<2>, grid, dim3(256), 0, st, x, w, bias, y, pre, g, act); break;
        default: VMASR_LAUNCH(VMASR_K_GCONV1D_FWD, bytes, gconv1d_fwd_kernel<4>, grid, dim3(256), 0, st, x, w, bias, y, pre, g, act); break;
    }
    return check_launch("gconv1d_fwd");
}

VMASR_EXPORT int vmasr_gconv1d_dgrad(const float *gy, const float *pre, const float *w, float *dx, int32_t B, int32_t Cin, int32_t Cout,
                                     int32_t groups, int64_t L, int32_t k, int32_t stride, int32_t pad, vmasr_stream_t stream) {
    VMASR_REQUIRE(gy && w && dx, VMASR_EINVAL, "gconv1d_dgrad: null tensor (gy, w, dx)");
    VMASR_GC_CHECK("gconv1d_dgrad");
    const GcGeom g = gc_geom(Cin, Cout, groups, pad, B, L);
    const int mt = gc_mt(g.Ci), MR = 16 * mt;
    const int64_t nq = (L + pad + kGcS - 1) / kGcS;
    const dim3 grid((unsigned)((nq + kGcQN - 1) / kGcQN), (unsigned)(g.G * ((g.Ci + MR - 1) / MR)), (unsigned)B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double bytes = 4.0 * ((double)B * Cin * L + (double)Cout * g.Ci * kGcK + (double)B * Cout * g.T * (pre ? 2.0 : 1.0));
    switch (mt) {
        case 1: VMASR_LAUNCH(VMASR_K_GCONV1D_DGRAD, bytes, gconv1d_dgrad_kernel<1>, grid, dim3(256), 0, st, gy, pre, w, dx, g); break;
        case 2: VMASR_LAUNCH(VMASR_K_GCONV1D_DGRAD, bytes, gconv1d_dgrad_kernel<2>, grid, dim3(256), 0, st, gy, pre, w, dx, g); break;
        default: VMASR_LAUNCH(VMASR_K_GCONV1D_DGRAD, bytes, gconv1d_dgrad_kernel<4>, grid, dim3(256), 0, st, gy, pre, w, dx, g); break;
    }
    return check_launch("gconv1d_dgrad");
}

VMASR_EXPORT int vmasr_gconv1d_wgrad(const float *x, const float *gy, const float *pre, float *dw, float *db, void *ws, size_t ws_bytes, int32_t B,
                                     int32_t Cin, int32_t Cout, int32_t groups, int64_t L, int32_t k, int32_t stride, int32_t pad,
                                     vmasr_stream_t stream) {
    VMASR_REQUIRE(x && gy && ws && (dw || db), VMASR_EINVAL, "gconv1d_wgrad: null tensor (x, gy, ws; dw or db)");
    VMASR_GC_CHECK("gconv1d_wgrad");
    const GcGeom g = gc_geom(Cin, Cout, groups, pad, B, L);
    const GcSplit s = gc_split(g);
    const size_t need = gc_ws_floats(g, s) * sizeof(float);
    VMASR_REQUIRE(ws_bytes >= need && aligned_to(ws, 4), VMASR_EINVAL, "gconv1d_wgrad: workspace too small or unaligned (%zu bytes, need %zu)",
                  ws_bytes, need);
    const size_t nw = (size_t)Cout * g.Ci * kGcK;
    float *part_w = static_cast<float *>(ws), *part_b = part_w + (size_t)s.S * nw;
    const dim3 grid(s.blocks, (unsigned)s.S);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double bytes = 4.0 * ((double)B * Cin * L + (double)B * Cout * g.T * (pre ? 2.0 : 1.0) + (double)s.S * nw);
    switch (gc_mt(g.Co)) {
        case 1: VMASR_LAUNCH(VMASR_K_GCONV1D_WGRAD, bytes, gconv1d_wgrad_kernel<1>, grid, dim3(256), 0, st, x, gy, pre, part_w, part_b, g, s.nT, s.ups); break;
        case 2: VMASR_LAUNCH(VMASR_K_GCONV1D_WGRAD, bytes, gconv1d_wgrad_kernel<2>, grid, dim3(256), 0, st, x, gy, pre, part_w, part_b, g, s.nT, s.ups); break;
        default: VMASR_LAUNCH(VMASR_K_GCONV1D_WGRAD, bytes, gconv1d_wgrad_kernel<4>, grid, dim3(256), 0, st, x, gy, pre, part_w, part_b, g, s.nT, s.ups); break;
    }
    const size_t n = nw + (size_t)Cout;
    VMASR_LAUNCH(VMASR_K_GCONV1D_WGRAD_REDUCE, 4.0 * ((double)s.S + 1.0) * (double)n, gconv1d_wgrad_reduce_kernel, dim3((unsigned)((n + 255) / 256)),
                 dim3(256), 0, st, part_w, part_b, dw, db, nw, (int)Cout, s.S);
    return check_launch("gconv1d_wgrad");
}
