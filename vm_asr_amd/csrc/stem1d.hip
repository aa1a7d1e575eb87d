// stem1d.hip — the scale discriminator's stem: Conv1d(1, Cout, k, stride 1) + bias + GELU as one pass over the output map, and its
// backward without a stored pre-activation.
//
// Reference: model/discriminator.py:181-188 — convs.0 of a ScaleDiscriminator is
//   y[b, o, t] = GELU(bias[o] + sum_{j < k} w[o, j] x[b, t + j - pad])                                          (x zero outside [0, L))
// on a one-channel signal: 15 multiply-adds per output of the LARGEST map of the discriminator (B x Cout x L at the waveform rate).
// The layer is memory traffic and nothing else, so every kernel here touches the map once: the forward writes y only, the backward
// reads gy only and rebuilds pre = conv + bias in registers from the row of x (Cout times smaller than the map) and the taps.
//
// Shape of all three kernels: a time tile of kStTT = 1024 positions per workgroup pass, 4 per lane at lane + 64 i of the wave's 256,
// so every global load / store of the map is one full wave on 256 contiguous bytes, whatever the row's alignment (T is odd at the
// second scale).  The window of x (tile + k - 1 halo) is staged in LDS as float4 xq[wave][q] = x[256 wave + q + 64 (0..3)]: tap j of
// all four positions of a lane is ONE conflict-free ds_read_b128 at q = lane + j.  Taps are staged per channel group and read as
// broadcasts.  Plain fp32 FMAs in a fixed order, no float atomics: results are bit-identical from call to call.
//
//   fwd    : block = (tile, 16 channels, b); acc[16][4] over the taps, + bias, GELU, store.
//   bwd dw : block = (CG channels, slab of (b, tile) units).  g = gy GELU'(pre); dw[c][j] += g x[t + j - pad] in per-lane accumulators
//            that live across the whole slab; one wave / workgroup sum at the end -> part[slab][o][k + 1] (the last entry is db);
//            a second launch adds the slabs in a fixed order.
//   bwd dx : block = (256 g positions -> 256 - (k - 1) complete dx positions, b), ALL channels inside the block, a quarter per wave in a
//            fixed order: D_j[t] = sum_o w[o, j] g[o, t] per lane and tap, no exchange inside the channel loop; then
//            dx[p] = sum_j sum_waves D_j[p + pad - j] through double-buffered LDS rows, once per tile.  Neighbouring tiles recompute
//            the k - 1 halo positions (the short tile keeps small batches on every CU: 1024-position tiles left half the chip idle).
//
// The generator's pass (vmasr_stem1d_fm_fwd / _fm_bwd) folds the feature-matching term of this map, coef sum |y - y_real|, into the same
// two passes: the forward also reads its tile of y_real and leaves one fp64 partial per workgroup (the caller adds them: a fixed order);
// the dx kernel rebuilds y beside pre and adds coef * gterm * sgn(y - y_real) to gy before GELU'.  No sign tensor, no difference tensor.
// The forward and the dx kernel form pre with ONE device function (st_pre), so the y rebuilt there is the forward's y bit for bit: a
// position where y == y_real has sign 0 in the backward exactly when its |y - y_real| is 0 in the forward.
#include <algorithm>

#include "common.h"

namespace vmasr {
namespace {

constexpr int kStTT = 1024;                 // time tile (4 waves x 64 lanes x 4 positions)
constexpr int kStKMax = 32;                 // largest k
constexpr int kStQ = 64 + kStKMax;          // float4 entries of a wave's staged window
constexpr int kStCG = 16;                   // fwd: channels per block
constexpr int kStXT = 256;                  // bwd dx: gradient positions per block (every wave works on all of them)
constexpr int kStXC = 32;                   // bwd dx: channels per weight stage (8 sub-chunks of 4, two per wave)
constexpr int kStBlocks = 2048;             // bwd dw: workgroups a launch aims for (sets the slab count)
constexpr int kStSlabMax = 256;

struct StGeom {
    int B, Cout, k, pad, act, L, T;
};

// xq[wave][q].c = x[w0 + 256 wave + q + 64 c] for `nwin` waves' worth of positions, where that index lies in the block's window
// [0, 256 nwin + k - 1) and in [0, L), else 0
__device__ __forceinline__ void st_stage_x(float4 *xq, const float *__restrict__ xrow, const int w0, const int L, const int k, const int nwin) {
    float *xf = reinterpret_cast<float *>(xq);
    for (int i = threadIdx.x; i < nwin * kStQ * 4; i += 256) {
        const int c = i & 3, e = i >> 2, wv = e / kStQ, q = e - wv * kStQ;
        const int win = wv * 256 + q + 64 * c, p = w0 + win;
        xf[i] = (win < 256 * nwin + k - 1 && p >= 0 && p < L) ? xrow[p] : 0.f;
    }
}

// THE stem arithmetic, defined once: pre = st_pre(acc, bias) with acc[c][i] = sum_{j < k} w_c[j] x[t_i + j - pad] from st_taps, for NC
// channels at a lane's four positions — a zero-start chain of one fmaf per tap, taps ascending, then the bias in one rounded add.
// tap(j, c) is w_c[j] (from the kernel's LDS image).
__device__ __forceinline__ float st_pre(const float acc, const float bv) { return acc + bv; }

template <int NC, class Tap>
__device__ __forceinline__ void st_taps(float (&pre)[NC][4], const float4 *xr, const int k, const Tap tap) {
#pragma unroll
    for (int c = 0; c < NC; ++c) pre[c][0] = pre[c][1] = pre[c][2] = pre[c][3] = 0.f;
    for (int j = 0; j < k; ++j) {
        const float4 xv = xr[j];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float wv = tap(j, c);
            pre[c][0] = fmaf(wv, xv.x, pre[c][0]);
            pre[c][1] = fmaf(wv, xv.y, pre[c][1]);
            pre[c][2] = fmaf(wv, xv.z, pre[c][2]);
            pre[c][3] = fmaf(wv, xv.w, pre[c][3]);
        }
    }
}

// y = GELU(pre) as the ROUNDED fp32 value the forward stores: the empty asm keeps the compiler from contracting gelu_f's last product into
// a following y - y_real (an fma would see the unrounded product: |y - y| != 0, and a sign where the forward's y ties with y_real)
__device__ __forceinline__ float st_gelu_rounded(const float pre) {
    float y = gelu_f(pre);
    asm volatile("" : "+v"(y));
    return y;
}

// grid (ceil(T / 1024), ceil(Cout / 16), B).  FM: also partials[block] = sum over the block's tile of |y - y_real| (fp64; every block
// writes its own slot, blocks in (b, channel group, tile) order)
template <bool FM>
__global__ __launch_bounds__(256) void stem1d_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                         float *__restrict__ y, const float *__restrict__ y_real,
                                                         double *__restrict__ partials, const StGeom g) {
    __shared__ float4 xq[4 * kStQ];
    __shared__ __attribute__((aligned(16))) float ws[kStKMax * kStCG];
    __shared__ float bs[kStCG];
    __shared__ double wsum[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = blockIdx.x * kStTT, o0 = blockIdx.y * kStCG, b = blockIdx.z;
    const int nch = min(kStCG, g.Cout - o0);
    st_stage_x(xq, x + (size_t)b * g.L, t0 - g.pad, g.L, g.k, 4);
    for (int i = tid; i < g.k * kStCG; i += 256) {          // ws[j][c]; channels past the last: zero taps
        const int j = i / kStCG, c = i - j * kStCG;
        ws[i] = c < nch ? w[(size_t)(o0 + c) * g.k + j] : 0.f;
    }
    if (tid < kStCG) bs[tid] = (bias && tid < nch) ? bias[o0 + tid] : 0.f;
    __syncthreads();
    float acc[kStCG][4];
    st_taps(acc, xq + wave * kStQ + lane, g.k, [&](const int j, const int c) { return ws[j * kStCG + c]; });
    const int tl = t0 + wave * 256 + lane;
    double l1 = 0.0;
#pragma unroll
    for (int c = 0; c < kStCG; ++c) {
        if (c < nch) {
            const size_t row = ((size_t)b * g.Cout + o0 + c) * g.T;
            float *yr = y + row;
            const float bv = bs[c];
            float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = tl + 64 * i;
                const float v = st_pre(acc[c][i], bv);
                if (t < g.T) {
                    if constexpr (FM) {
                        const float rv = y_real[row + t], yv = st_gelu_rounded(v);
                        yr[t] = yv;
                        d[i] = fabsf(yv - rv);
                    } else {
                        yr[t] = g.act ? gelu_f(v) : v;
                    }
                }
            }
            if constexpr (FM) l1 += (double)((d[0] + d[1]) + (d[2] + d[3]));
        }
    }
    if constexpr (FM) {                                     // workgroup sum: wave shuffle, then the four waves in order
        for (int off = 32; off > 0; off >>= 1) l1 += __shfl_down(l1, off, 64);
        if (lane == 0) wsum[wave] = l1;
        __syncthreads();
        if (tid == 0) partials[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
}

// grid (ceil(Cout / CG), S); slab sp owns the units [sp ups, (sp + 1) ups) of the B * nT units (b, tile).  part (S, Cout, k + 1).
template <int KP, int CG>
__global__ __launch_bounds__(256) void stem1d_bwd_w_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ w,
                                                           const float *__restrict__ bias, float *__restrict__ part, const StGeom g, const int nT,
                                                           const long long ups) {
    constexpr int NV = CG * (KP + 1);
    __shared__ float4 xq[4 * kStQ];
    __shared__ __attribute__((aligned(16))) float ws[KP * CG];
    __shared__ float red[4][NV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = blockIdx.x * CG, sp = blockIdx.y;
    const int nch = min(CG, g.Cout - o0);
    for (int i = tid; i < KP * CG; i += 256) {              // ws[j][c]; zero past the last tap / channel
        const int j = i / CG, c = i - j * CG;
        ws[i] = (j < g.k && c < nch) ? w[(size_t)(o0 + c) * g.k + j] : 0.f;
    }
    float bv[CG], dwacc[CG][KP], dbacc[CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) {
        bv[c] = (bias && c < nch) ? bias[o0 + c] : 0.f;
        dbacc[c] = 0.f;
#pragma unroll
        for (int j = 0; j < KP; ++j) dwacc[c][j] = 0.f;
    }
    const float4 *xr = xq + wave * kStQ + lane;
    const long long total = (long long)g.B * nT, u0 = (long long)sp * ups, u1 = min(total, u0 + ups);
    for (long long u = u0; u < u1; ++u) {
        const int b = (int)(u / nT), t0 = (int)(u - (long long)b * nT) * kStTT;
        __syncthreads();                                    // the previous unit's window reads are done
        st_stage_x(xq, x + (size_t)b * g.L, t0 - g.pad, g.L, g.k, 4);
        float gv[CG][4];
        const int tl = t0 + wave * 256 + lane;
#pragma unroll
        for (int c = 0; c < CG; ++c) {
            const float *gr = gy + ((size_t)b * g.Cout + o0 + (c < nch ? c : 0)) * g.T;
#pragma unroll
            for (int i = 0; i < 4; ++i) gv[c][i] = (c < nch && tl + 64 * i < g.T) ? gr[tl + 64 * i] : 0.f;
        }
        __syncthreads();
        if (g.act) {
            float pre[CG][4];
#pragma unroll
            for (int c = 0; c < CG; ++c) pre[c][0] = pre[c][1] = pre[c][2] = pre[c][3] = bv[c];
            for (int j = 0; j < g.k; ++j) {
                const float4 xv = xr[j];
#pragma unroll
                for (int c = 0; c < CG; ++c) {
                    const float wv = ws[j * CG + c];
                    pre[c][0] = fmaf(wv, xv.x, pre[c][0]);
                    pre[c][1] = fmaf(wv, xv.y, pre[c][1]);
                    pre[c][2] = fmaf(wv, xv.z, pre[c][2]);
                    pre[c][3] = fmaf(wv, xv.w, pre[c][3]);
                }
            }
#pragma unroll
            for (int c = 0; c < CG; ++c)
#pragma unroll
                for (int i = 0; i < 4; ++i) gv[c][i] *= gelu_grad_f(pre[c][i]);
        }
#pragma unroll
        for (int j = 0; j < KP; ++j) {                      // taps past k read zeros (or real samples) and are never written out
            const float4 xv = xr[j];
#pragma unroll
            for (int c = 0; c < CG; ++c)
                dwacc[c][j] = fmaf(gv[c][3], xv.w, fmaf(gv[c][2], xv.z, fmaf(gv[c][1], xv.y, fmaf(gv[c][0], xv.x, dwacc[c][j]))));
        }
#pragma unroll
        for (int c = 0; c < CG; ++c) dbacc[c] += (gv[c][0] + gv[c][1]) + (gv[c][2] + gv[c][3]);
    }
#pragma unroll
    for (int c = 0; c < CG; ++c) {
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const float s = wave_sum(dwacc[c][j]);
            if (lane == 0) red[wave][c * (KP + 1) + j] = s;
        }
        const float s = wave_sum(dbacc[c]);
        if (lane == 0) red[wave][c * (KP + 1) + KP] = s;
    }
    __syncthreads();
    if (tid < NV) {
        const int c = tid / (KP + 1), j = tid - c * (KP + 1);
        if (c < nch && (j < g.k || j == KP))
            part[((size_t)sp * g.Cout + o0 + c) * (g.k + 1) + (j == KP ? g.k : j)] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    }
}

// dw[o][j] / db[o] = sum over the S slabs: 16 slices of consecutive slabs per output, then the 16 slice sums in order.  n = Cout (k + 1).
__global__ __launch_bounds__(256) void stem1d_bwd_reduce_kernel(const float *__restrict__ part, float *__restrict__ dw, float *__restrict__ db,
                                                                const size_t n, const int k, const int S) {
    __shared__ float red[16][16];
    const int col = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const size_t idx = (size_t)blockIdx.x * 16 + col;
    const int per = (S + 15) / 16, s0 = sl * per, s1 = min(S, s0 + per);
    float s = 0.f;
    if (idx < n)
        for (int sp = s0; sp < s1; ++sp) s += part[(size_t)sp * n + idx];
    red[sl][col] = s;
    __syncthreads();
    if (sl == 0 && idx < n) {
        float t = red[0][col];
#pragma unroll
        for (int q = 1; q < 16; ++q) t += red[q][col];
        const size_t o = idx / (size_t)(k + 1);
        const int j = (int)(idx - o * (size_t)(k + 1));
        if (j < k) {
            if (dw) dw[o * k + j] = t;
        } else if (db) {
            db[o] = t;
        }
    }
}

// grid (ceil(L / (256 - (k - 1))), B).  All four waves work on the SAME 256 gradient positions (4 per lane) and share the channels:
// wave v takes the sub-chunks of 4 channels with index v mod 4, in ascending order; the four partial D_j are added in wave order.
// FM (act on): the gradient of the map is gy + kc sgn(y - y_real) with y = GELU(pre) rebuilt beside pre, kc = coef * gterm[0] (gterm: the
// loss term's upstream gradient on the device; NULL: no loss gradient) and sgn(0) = 0; gy may be NULL (zeros).
template <int KP, bool FM>
__global__ __launch_bounds__(256) void stem1d_bwd_x_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ w,
                                                           const float *__restrict__ bias, const float *__restrict__ y_real,
                                                           const float *__restrict__ gterm, const float coef, float *__restrict__ dx,
                                                           const StGeom g) {
    __shared__ float4 xq[kStQ];
    __shared__ float4 ws4[(kStXC / 4) * KP];                // ws4[sub-chunk][j] = the tap j of its 4 channels
    __shared__ float bs[kStXC];
    __shared__ float buf[2][4][kStXT + kStKMax];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, TO = kStXT - (g.k - 1);
    const int p0 = blockIdx.x * TO, tg0 = p0 + g.pad - (g.k - 1);   // first dx position, first gradient position of the tile
    buf[tid >> 7][(tid >> 5) & 3][kStXT + (tid & 31)] = 0.f;        // the rows' tails: read by lanes whose result is not stored
    st_stage_x(xq, x + (size_t)b * g.L, tg0 - g.pad, g.L, g.k, 1);
    float D[KP][4];
#pragma unroll
    for (int j = 0; j < KP; ++j) D[j][0] = D[j][1] = D[j][2] = D[j][3] = 0.f;
    const float4 *xr = xq + lane;
    const int tl = tg0 + lane;
    float *wsf = reinterpret_cast<float *>(ws4);
    const float kc = (FM && gterm) ? coef * gterm[0] : 0.f;
    for (int oc0 = 0; oc0 < g.Cout; oc0 += kStXC) {
        __syncthreads();
        for (int i = tid; i < kStXC * KP; i += 256) {       // i = (sub * KP + j) * 4 + c
            const int c = i & 3, e = i >> 2, sub = e / KP, j = e - sub * KP, o = oc0 + sub * 4 + c;
            wsf[i] = (o < g.Cout && j < g.k) ? w[(size_t)o * g.k + j] : 0.f;
        }
        if (tid < kStXC) bs[tid] = (bias && oc0 + tid < g.Cout) ? bias[oc0 + tid] : 0.f;
        __syncthreads();
        const int nsub = min(kStXC / 4, (g.Cout - oc0 + 3) / 4);
        for (int sub = wave; sub < nsub; sub += 4) {
            float gv[4][4], rv[4][4];
            unsigned inm = 0;                               // bit 4 c + i: (channel c, position i) lies in the map
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int o = oc0 + sub * 4 + c;
                const bool och = o < g.Cout;
                const size_t row = ((size_t)b * g.Cout + (och ? o : 0)) * g.T;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int t = tl + 64 * i;
                    const bool in = och && t >= 0 && t < g.T;
                    gv[c][i] = (in && (!FM || gy)) ? gy[row + t] : 0.f;
                    if constexpr (FM) {
                        rv[c][i] = in ? y_real[row + t] : 0.f;
                        inm |= (unsigned)in << (4 * c + i);
                    }
                }
            }
            const float4 *wr = ws4 + sub * KP;
            if (g.act) {
                float pre[4][4];
                st_taps(pre, xr, g.k, [&](const int j, const int c) { return wsf[(sub * KP + j) * 4 + c]; });
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        pre[c][i] = st_pre(pre[c][i], bs[sub * 4 + c]);
                        if constexpr (FM) {                 // outside the map y = GELU(pre) of padding: no sign there
                            const float yv = st_gelu_rounded(pre[c][i]);
                            const float sg = ((inm >> (4 * c + i)) & 1u) ? (float)((yv > rv[c][i]) - (yv < rv[c][i])) : 0.f;
                            gv[c][i] = fmaf(kc, sg, gv[c][i]);
                        }
                        gv[c][i] *= gelu_grad_f(pre[c][i]);
                    }
            }
#pragma unroll
            for (int j = 0; j < KP; ++j) {                  // zero taps past k
                const float4 w4 = wr[j];
                const float wv[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int i = 0; i < 4; ++i) D[j][i] = fmaf(wv[c], gv[c][i], D[j][i]);
            }
        }
    }
    // dx[p0 + v] = sum_j sum_waves D_j[v + (k - 1) - j], taps ascending, waves ascending; wave v finishes the positions 64 v + lane.
    // The buffers alternate, so one barrier per tap is enough.
    float dxa = 0.f;
    const int v = tid;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        if (j < g.k) {
            float(*bf)[kStXT + kStKMax] = buf[j & 1];
#pragma unroll
            for (int i = 0; i < 4; ++i) bf[wave][lane + 64 * i] = D[j][i];
            __syncthreads();
            const int idx = v + (g.k - 1) - j;
            dxa += ((bf[0][idx] + bf[1][idx]) + bf[2][idx]) + bf[3][idx];
        }
    }
    if (v < TO && p0 + v < g.L) dx[(size_t)b * g.L + p0 + v] = dxa;
}

// ---- host side: ONE predicate for the queries and the launchers ---------------------------------------------------------------------
bool st_shape_ok(int Cout, int k, int stride, int pad) {
    return stride == 1 && k >= 1 && k <= kStKMax && pad >= 0 && pad < k && Cout >= 1 && Cout <= 65536;   // (grid.y = ceil(Cout / 16))
}

bool st_launch_ok(int Cout, int k, int stride, int pad, int B, int64_t L) {
    return st_shape_ok(Cout, k, stride, pad) && B >= 1 && B <= 65535 && L >= 1 && L >= k - 2 * pad && L <= (int64_t(1) << 28);
}

StGeom st_geom(int Cout, int k, int pad, int B, int64_t L, int act) {
    StGeom g{};
    g.B = B; g.Cout = Cout; g.k = k; g.pad = pad; g.act = act ? 1 : 0; g.L = (int)L; g.T = (int)(L + 2 * pad - k + 1);
    return g;
}

int st_cg(int k) { return k <= 16 ? 4 : 2; }               // bwd dw: channels per block (64 tap accumulators per lane either way)

struct StSplit {
    int nT, S;
    long long ups;
    unsigned groups;
};

StSplit st_split(const StGeom &g) {
    StSplit s{};
    const int cg = st_cg(g.k);
    s.groups = (unsigned)((g.Cout + cg - 1) / cg);
    s.nT = (g.T + kStTT - 1) / kStTT;
    const long long total = (long long)g.B * s.nT;
    const long long want = std::min<long long>(std::max<long long>(1, (kStBlocks + s.groups - 1) / s.groups), std::min<long long>(total, kStSlabMax));
    s.ups = (total + want - 1) / want;
    s.S = (int)((total + s.ups - 1) / s.ups);              // no empty slab
    return s;
}

size_t st_ws_floats(const StGeom &g, const StSplit &s) { return (size_t)s.S * (size_t)g.Cout * (size_t)(g.k + 1); }

dim3 st_fwd_grid(const StGeom &g) { return dim3((unsigned)((g.T + kStTT - 1) / kStTT), (unsigned)((g.Cout + kStCG - 1) / kStCG), (unsigned)g.B); }

size_t st_fm_partials(const StGeom &g) {                   // one fp64 slot per workgroup of the forward
    const dim3 grid = st_fwd_grid(g);
    return (size_t)grid.x * grid.y * grid.z;
}

double st_map_bytes(const StGeom &g) { return 4.0 * (double)g.B * g.Cout * g.T; }
double st_small_bytes(const StGeom &g) { return 4.0 * ((double)g.B * g.L + (double)g.Cout * (g.k + 1)); }

// the forward and the dx launch, plain (FM false: the last operands unused) and with the feature-matching term
template <bool FM>
void st_launch_fwd(const float *x, const float *w, const float *bias, float *y, const float *y_real, double *partials, const StGeom &g,
                   hipStream_t st) {
    const dim3 grid = st_fwd_grid(g);
    const double bytes = st_small_bytes(g) + (FM ? 2.0 : 1.0) * st_map_bytes(g) + (FM ? 8.0 * (double)st_fm_partials(g) : 0.0);
    VMASR_LAUNCH(VMASR_K_STEM1D_FWD, bytes, stem1d_fwd_kernel<FM>, grid, dim3(256), 0, st, x, w, bias, y, y_real, partials, g);
}

template <bool FM>
void st_launch_dx(const float *gy, const float *x, const float *w, const float *bias, const float *y_real, const float *gterm, const float coef,
                  float *dx, const StGeom &g, hipStream_t st) {
    const dim3 grid((unsigned)((g.L + (kStXT - g.k)) / (kStXT - (g.k - 1))), (unsigned)g.B);
    const double bytes = ((gy ? 1.0 : 0.0) + (FM ? 1.0 : 0.0)) * st_map_bytes(g) + st_small_bytes(g) + 4.0 * g.B * g.L;
    if (g.k <= 16) VMASR_LAUNCH(VMASR_K_STEM1D_BWD, bytes, (stem1d_bwd_x_kernel<16, FM>), grid, dim3(256), 0, st, gy, x, w, bias, y_real, gterm, coef, dx, g);
    else VMASR_LAUNCH(VMASR_K_STEM1D_BWD, bytes, (stem1d_bwd_x_kernel<32, FM>), grid, dim3(256), 0, st, gy, x, w, bias, y_real, gterm, coef, dx, g);
}

}  // namespace
}  // namespace vmasr

using namespace vmasr;

VMASR_EXPORT int32_t vmasr_stem1d_time_tile(void) { return kStTT; }
VMASR_EXPORT int32_t vmasr_stem1d_channel_group(void) { return kStCG; }

VMASR_EXPORT int vmasr_stem1d_supported(int32_t Cout, int32_t k, int32_t stride, int32_t pad) { return st_shape_ok(Cout, k, stride, pad) ? 1 : 0; }

VMASR_EXPORT int vmasr_stem1d_supported_launch(int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t B, int64_t L) {
    return st_launch_ok(Cout, k, stride, pad, B, L) ? 1 : 0;
}

VMASR_EXPORT size_t vmasr_stem1d_bwd_workspace(int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t B, int64_t L) {
    if (!st_launch_ok(Cout, k, stride, pad, B, L)) return 0;
    const StGeom g = st_geom(Cout, k, pad, B, L, 1);
    return st_ws_floats(g, st_split(g)) * sizeof(float);
}

#define VMASR_ST_CHECK(what)                                                                                                          \
    VMASR_REQUIRE(st_launch_ok(Cout, k, stride, pad, B, L), VMASR_EINVAL,                                                               \
                  what ": unsupported shape (Cout=%d k=%d stride=%d pad=%d B=%d L=%lld): needs stride 1, 1 <= k <= 32, 0 <= pad < k, "   \
                       "1 <= Cout <= 65536, 1 <= B <= 65535, max(1, k - 2 pad) <= L <= 2^28",                                           \
                  Cout, k, stride, pad, B, (long long)L)

VMASR_EXPORT int vmasr_stem1d_fwd(const float *x, const float *w, const float *bias, float *y, int32_t B, int32_t Cout, int64_t L, int32_t k,
                                  int32_t stride, int32_t pad, int32_t act, vmasr_stream_t stream) {
    VMASR_REQUIRE(x && w && y, VMASR_EINVAL, "stem1d_fwd: null tensor (x, w, y)");
    VMASR_ST_CHECK("stem1d_fwd");
    st_launch_fwd<false>(x, w, bias, y, nullptr, nullptr, st_geom(Cout, k, pad, B, L, act), static_cast<hipStream_t>(stream));
    return check_launch("stem1d_fwd");
}

VMASR_EXPORT int vmasr_stem1d_bwd(const float *gy, const float *x, const float *w, const float *bias, float *dx, float *dw, float *db, void *ws,
                                  size_t ws_bytes, int32_t B, int32_t Cout, int64_t L, int32_t k, int32_t stride, int32_t pad, int32_t act,
                                  vmasr_stream_t stream) {
    VMASR_REQUIRE(gy && x && w && (dx || dw || db), VMASR_EINVAL, "stem1d_bwd: null tensor (gy, x, w; one of dx, dw, db)");
    VMASR_ST_CHECK("stem1d_bwd");
    const StGeom g = st_geom(Cout, k, pad, B, L, act);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double map = st_map_bytes(g), small = st_small_bytes(g);
    StSplit s{};
    if (dw || db) {
        s = st_split(g);
        const size_t need = st_ws_floats(g, s) * sizeof(float);
        VMASR_REQUIRE(ws && ws_bytes >= need && aligned_to(ws, 4), VMASR_EINVAL,
                      "stem1d_bwd: workspace missing, too small or unaligned (%zu bytes, need %zu)", ws_bytes, need);
    }
    if (dx) st_launch_dx<false>(gy, x, w, bias, nullptr, nullptr, 0.f, dx, g, st);
    if (dw || db) {
        float *part = static_cast<float *>(ws);
        const dim3 grid(s.groups, (unsigned)s.S);
        const size_t n = (size_t)Cout * (size_t)(k + 1);
        const double bytes = map + small + 4.0 * (double)s.S * (double)n;
        const auto narrow = stem1d_bwd_w_kernel<16, 4>, wide = stem1d_bwd_w_kernel<32, 2>;
        if (k <= 16) VMASR_LAUNCH(VMASR_K_STEM1D_BWD, bytes, narrow, grid, dim3(256), 0, st, gy, x, w, bias, part, g, s.nT, s.ups);
        else VMASR_LAUNCH(VMASR_K_STEM1D_BWD, bytes, wide, grid, dim3(256), 0, st, gy, x, w, bias, part, g, s.nT, s.ups);
        VMASR_LAUNCH(VMASR_K_STEM1D_BWD_REDUCE, 4.0 * ((double)s.S + 1.0) * (double)n, stem1d_bwd_reduce_kernel, dim3((unsigned)((n + 15) / 16)),
                     dim3(256), 0, st, part, dw, db, n, (int)k, s.S);
    }
    return check_launch("stem1d_bwd");
}

// ---- the generator's pass: the stem with its feature-matching term (GELU always on) --------------------------------------------------
VMASR_EXPORT int vmasr_stem1d_fm_supported_launch(int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t B, int64_t L) {
    return st_launch_ok(Cout, k, stride, pad, B, L) ? 1 : 0;
}

VMASR_EXPORT size_t vmasr_stem1d_fm_workspace(int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t B, int64_t L) {
    if (!st_launch_ok(Cout, k, stride, pad, B, L)) return 0;
    return st_fm_partials(st_geom(Cout, k, pad, B, L, 1)) * sizeof(double);
}

VMASR_EXPORT int vmasr_stem1d_fm_fwd(const float *x, const float *w, const float *bias, const float *y_real, float *y, double *partials,
                                     size_t ws_bytes, int32_t B, int32_t Cout, int64_t L, int32_t k, int32_t stride, int32_t pad,
                                     vmasr_stream_t stream) {
    VMASR_REQUIRE(x && w && y_real && y, VMASR_EINVAL, "stem1d_fm_fwd: null tensor (x, w, y_real, y)");
    VMASR_ST_CHECK("stem1d_fm_fwd");
    const StGeom g = st_geom(Cout, k, pad, B, L, 1);
    const size_t need = st_fm_partials(g) * sizeof(double);
    VMASR_REQUIRE(partials && ws_bytes >= need && aligned_to(partials, 8), VMASR_EINVAL,
                  "stem1d_fm_fwd: workspace missing, too small or unaligned (%zu bytes, need %zu)", ws_bytes, need);
    st_launch_fwd<true>(x, w, bias, y, y_real, partials, g, static_cast<hipStream_t>(stream));
    return check_launch("stem1d_fm_fwd");
}

VMASR_EXPORT int vmasr_stem1d_fm_bwd(const float *gy, const float *x, const float *w, const float *bias, const float *y_real, const float *gterm,
                                     float coef, float *dx, int32_t B, int32_t Cout, int64_t L, int32_t k, int32_t stride, int32_t pad,
                                     vmasr_stream_t stream) {
    VMASR_REQUIRE(x && w && y_real && dx && (gy || gterm), VMASR_EINVAL, "stem1d_fm_bwd: null tensor (x, w, y_real, dx; one of gy, gterm)");
    VMASR_ST_CHECK("stem1d_fm_bwd");
    st_launch_dx<true>(gy, x, w, bias, y_real, gterm, coef, dx, st_geom(Cout, k, pad, B, L, 1), static_cast<hipStream_t>(stream));
    return check_launch("stem1d_fm_bwd");
}
