// gmlp.hip — the GATED Mlp branch of a VSSBlock (MODEL.VSSM.GMLP) as ONE kernel on the gfx950 matrix cores:
//
//     [u ; z] = fc1(LayerNorm(x))   (fc1: d -> 2 * hidden; u = the first `hidden` rows of fc1.weight, z = the second)
//     y = x + s * fc2(u * GELU(z))                         model/vmamba.py:512-538 (gMlp), :1815 / :1832-1837 (VSSBlock),
//                                                          timm DropPath (s = per-sample keep mask / keep)
//
// for the residual stream x (rows, d) fp32 or bf16, d in {8, 16, 32, 64}, hidden = 4 d: W1 is (8 d, d), W2 is (d, 4 d).
// The scheme is mlp.hip's (a wave owns 32 rows; both products transposed on v_mfma_f32_32x32x16_bf16; helpers in mlp_tile.h).
// Per hidden tile t the wave forms TWO accumulator tiles — rows 32 t.. (u) and rows 4 d + 32 t.. (z) of W1 against the same
// operand xn^T.  Both have the same layout (hidden unit on the register, data row on the lane), so the gate u * GELU(z) is a
// lane-local product of corresponding registers; it is taken in fp32 on the un-rounded fc1 outputs, rounded ONCE to bf16 and fed
// to fc2 as its B operand straight from the registers, exactly as GELU(h) is in mlp.hip.  Epilogue, hidden-split workgroups for
// d = 64 and the ordered LDS accumulation of deterministic mode: as in mlp.hip.
//
// Backward (recompute, nothing saved but x): the same wave re-runs LayerNorm, u and z, and forms
//     dact^T = W2^T . (s gy)^T,   du = dact * GELU(z),   dz = dact * u * GELU'(z),   dxn^T = W1u^T . du^T + W1z^T . dz^T
// (two MFMA contributions per hidden tile, from the u and the z columns of w1t (d, 8 d)).  It writes dxn (bf16) and the operands
// of the two weight-gradient GEMMs: gpre = [du | dz] (rows, 8 d), act_aug = [u * GELU(z) | 1 0..] (rows, 4 d + 8), xn_aug, s gy
// (host: vm_asr_amd/gmlp.py -> vmasr_layer_norm_bwd_res and wgrad.weight_grad_finished, as for the Mlp).
#include "mlp_tile.h"

namespace vmasr {
namespace {

struct GMlpArgs {
    const void *x;                  // (rows, D) fp32 or bf16 (the residual stream's dtype: TX)
    const float *gamma, *beta;      // (D)
    const bf16_t *w1;               // (8D, D)   fc1.weight: rows 0 .. 4D-1 = u, 4D .. 8D-1 = z
    const float *b1;                // (8D)
    const bf16_t *w2;               // (D, 4D)   fc2.weight
    const float *b2;                // (D)
    const float *scale;             // per-sample residual scale (DropPath) or null
    void *y;                        // (rows, D) TX
    long rows;
    int rows_per_sample;
    float eps;
    // backward only
    const void *gy;                 // (rows, D) TX
    const bf16_t *w1t;              // (D, 8D)   fc1.weight^T
    const bf16_t *w2t;              // (4D, D)   fc2.weight^T
    bf16_t *dxn;                    // (rows, D)
    bf16_t *xn_aug;                 // (rows, D + 8):  xn | 1 0 0 0 0 0 0 0
    bf16_t *gys;                    // (rows, D):      s * gy
    bf16_t *act_aug;                // (rows, 4D + 8): u * GELU(z) | 1 0 ...
    bf16_t *gpre;                   // (rows, 8D):     du | dz
    float *mean, *rstd;             // (rows)
    unsigned *det = nullptr;        // deterministic mode (common.h): the hidden-split waves add their partial tiles to LDS in wave order
};

template <int D, typename TX, int HS>
__global__ __launch_bounds__(256) void gmlp_fwd_kernel(const GMlpArgs a) {
    constexpr int KS = (D + 15) / 16, HD = 4 * D, HT = HD / 32, OT = (D + 31) / 32;
    constexpr int TPW = HS > 1 ? 1 : 4;                          // row tiles per workgroup
    static_assert(HS == 1 || HS == 4, "a workgroup is four waves: four row tiles, or one row tile split over the hidden tiles");
    __shared__ float s_out[HS > 1 ? OT * 32 * 32 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int split = HS > 1 ? wave : 0;
    const bf16_t *w1z = a.w1 + (size_t)HD * D;
    for (long tile = (long)blockIdx.x * TPW + (HS > 1 ? 0 : wave); tile * 32 < a.rows; tile += (long)gridDim.x * TPW) {
        const long row = tile * 32 + r;
        const bool ok = row < a.rows;
        const TX *xr = static_cast<const TX *>(a.x) + row * D;
        float xv[KS][8];
        load_row<D, KS, TX>(xr, ok, h, xv);
        float mean, rstd;
        row_stats<D, KS>(xv, h, a.eps, mean, rstd);
        bf16x8 xn[KS];
        normalise<D, KS>(xv, h, mean, rstd, a.gamma, a.beta, xn);

        f32x16 out[OT];
#pragma unroll
        for (int u = 0; u < OT; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) out[u][i] = 0.f;
        if constexpr (HS > 1) {
            for (int i = threadIdx.x; i < OT * 32 * 32; i += 64 * HS) s_out[i] = 0.f;
            __syncthreads();
        }
#pragma unroll 1
        for (int t = split; t < HT; t += HS) {
            const f32x16 uacc = hidden_tile<D, KS>(a.w1, t, r, h, xn);
            const f32x16 zacc = hidden_tile<D, KS>(w1z, t, r, h, xn);
            bf16x8 act[2];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int hid0 = 32 * t + 8 * g + 4 * h;
                const float4 bu = *reinterpret_cast<const float4 *>(a.b1 + hid0);
                const float4 bz = *reinterpret_cast<const float4 *>(a.b1 + HD + hid0);
                const float bbu[4] = {bu.x, bu.y, bu.z, bu.w}, bbz[4] = {bz.x, bz.y, bz.z, bz.w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float uv = uacc[4 * g + c] + bbu[c], zv = zacc[4 * g + c] + bbz[c];
                    act[g >> 1][4 * (g & 1) + c] = (bf16_t)(uv * (0.5f * zv * (1.f + erff(zv * kRsqrt2))));
                }
            }
#pragma unroll
            for (int u = 0; u < OT; ++u) {
                const int o = 32 * u + r;
                const bf16_t *wr = a.w2 + (size_t)o * HD;
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2)
                    out[u] = mfma_bf16(perm_frag(wr, 32 * t + 16 * s2 + 4 * h, o < D), act[s2], out[u]);
            }
        }
        const float sc = a.scale ? a.scale[ok ? row / a.rows_per_sample : 0] : 1.f;
        if constexpr (HS > 1) {
            VMASR_DET_WAVE_ORDER(a.det, HS, lds_accumulate<OT>(s_out, out, r, h));
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < OT; ++u)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (HS > 1 && (4 * u + g) % HS != split) continue;            // the 4-feature groups go round the waves
                const int o0 = 32 * u + 8 * g + 4 * h;
                if (ok && o0 < D) {
                    float xq[4], acc[4];
                    load4x<TX>(xr + o0, xq);
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = HS > 1 ? s_out[(o0 + c) * 32 + r] : out[u][4 * g + c];
                    const float4 bq = *reinterpret_cast<const float4 *>(a.b2 + o0);
                    store4x<TX>(static_cast<TX *>(a.y) + row * D + o0, fmaf(sc, acc[0] + bq.x, xq[0]), fmaf(sc, acc[1] + bq.y, xq[1]),
                                fmaf(sc, acc[2] + bq.z, xq[2]), fmaf(sc, acc[3] + bq.w, xq[3]));
                }
            }
        if constexpr (HS > 1) __syncthreads();                               // s_out is reused by the next row tile
    }
}

template <int D, typename TX, int HS>
__global__ __launch_bounds__(256) void gmlp_bwd_kernel(const GMlpArgs a) {
    constexpr int KS = (D + 15) / 16, HD = 4 * D, HT = HD / 32, OT = (D + 31) / 32;
    constexpr int TPW = HS > 1 ? 1 : 4;
    static_assert(HS == 1 || HS == 4, "a workgroup is four waves");
    __shared__ float s_out[HS > 1 ? OT * 32 * 32 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int split = HS > 1 ? wave : 0;
    const bf16_t *w1z = a.w1 + (size_t)HD * D;
    for (long tile = (long)blockIdx.x * TPW + (HS > 1 ? 0 : wave); tile * 32 < a.rows; tile += (long)gridDim.x * TPW) {
        const long row = tile * 32 + r;
        const bool ok = row < a.rows;
        float xv[KS][8];
        load_row<D, KS, TX>(static_cast<const TX *>(a.x) + row * D, ok, h, xv);
        float mean, rstd;
        row_stats<D, KS>(xv, h, a.eps, mean, rstd);
        bf16x8 xn[KS];
        normalise<D, KS>(xv, h, mean, rstd, a.gamma, a.beta, xn);
        load_row<D, KS, TX>(static_cast<const TX *>(a.gy) + row * D, ok, h, xv);      // xv <- gy
        const float sc = a.scale ? a.scale[ok ? row / a.rows_per_sample : 0] : 1.f;
        bf16x8 gyf[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int j = 0; j < 8; ++j) gyf[s][j] = (bf16_t)(sc * xv[s][j]);
            const int f0 = 16 * s + 8 * h;
            if (ok && f0 < D && split == 0) {
                *reinterpret_cast<bf16x8 *>(a.xn_aug + row * (D + 8) + f0) = xn[s];
                *reinterpret_cast<bf16x8 *>(a.gys + row * D + f0) = gyf[s];
            }
        }
        if (ok && h == 0 && split == 0) {
            bf16x8 one = zero8();
            one[0] = (bf16_t)1.f;
            *reinterpret_cast<bf16x8 *>(a.xn_aug + row * (D + 8) + D) = one;
            *reinterpret_cast<bf16x8 *>(a.act_aug + row * (HD + 8) + HD) = one;
            a.mean[row] = mean;
            a.rstd[row] = rstd;
        }

        f32x16 dx[OT];
#pragma unroll
        for (int u = 0; u < OT; ++u)
#pragma unroll
            for (int i = 0; i < 16; ++i) dx[u][i] = 0.f;
        if constexpr (HS > 1) {
            for (int i = threadIdx.x; i < OT * 32 * 32; i += 64 * HS) s_out[i] = 0.f;
            __syncthreads();
        }
#pragma unroll 1
        for (int t = split; t < HT; t += HS) {
            const f32x16 uacc = hidden_tile<D, KS>(a.w1, t, r, h, xn);
            const f32x16 zacc = hidden_tile<D, KS>(w1z, t, r, h, xn);
            const f32x16 dacc = hidden_tile<D, KS>(a.w2t, t, r, h, gyf);   // dact^T = W2^T[32 t .., :] . (s gy)^T
            bf16x8 gu[2], gz[2];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int hid0 = 32 * t + 8 * g + 4 * h;
                const float4 bu = *reinterpret_cast<const float4 *>(a.b1 + hid0);
                const float4 bz = *reinterpret_cast<const float4 *>(a.b1 + HD + hid0);
                const float bbu[4] = {bu.x, bu.y, bu.z, bu.w}, bbz[4] = {bz.x, bz.y, bz.z, bz.w};
                float av[4], duv[4], dzv[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float uv = uacc[4 * g + c] + bbu[c], zv = zacc[4 * g + c] + bbz[c];
                    const float cdf = 0.5f * (1.f + erff(zv * kRsqrt2));
                    const float pdf = kInvSqrt2Pi * __expf(-0.5f * zv * zv);
                    const float gel = zv * cdf, da = dacc[4 * g + c];
                    av[c] = uv * gel;
                    duv[c] = da * gel;
                    dzv[c] = da * uv * fmaf(zv, pdf, cdf);
                    gu[g >> 1][4 * (g & 1) + c] = (bf16_t)duv[c];
                    gz[g >> 1][4 * (g & 1) + c] = (bf16_t)dzv[c];
                }
                if (ok) {
                    store_bf16x4(a.act_aug + row * (HD + 8) + hid0, av[0], av[1], av[2], av[3]);
                    store_bf16x4(a.gpre + row * (2 * HD) + hid0, duv[0], duv[1], duv[2], duv[3]);
                    store_bf16x4(a.gpre + row * (2 * HD) + HD + hid0, dzv[0], dzv[1], dzv[2], dzv[3]);
                }
            }
#pragma unroll
            for (int u = 0; u < OT; ++u) {
                const int f = 32 * u + r;
                const bf16_t *wr = a.w1t + (size_t)f * (2 * HD);
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    dx[u] = mfma_bf16(perm_frag(wr, 32 * t + 16 * s2 + 4 * h, f < D), gu[s2], dx[u]);
                    dx[u] = mfma_bf16(perm_frag(wr, HD + 32 * t + 16 * s2 + 4 * h, f < D), gz[s2], dx[u]);
                }
            }
        }
        if constexpr (HS > 1) {
            VMASR_DET_WAVE_ORDER(a.det, HS, lds_accumulate<OT>(s_out, dx, r, h));
            __syncthreads();
        }
#pragma unroll
        for (int u = 0; u < OT; ++u)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (HS > 1 && (4 * u + g) % HS != split) continue;
                const int f0 = 32 * u + 8 * g + 4 * h;
                if (ok && f0 < D) {
                    float acc[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = HS > 1 ? s_out[(f0 + c) * 32 + r] : dx[u][4 * g + c];
                    store_bf16x4(a.dxn + row * D + f0, acc[0], acc[1], acc[2], acc[3]);
                }
            }
        if constexpr (HS > 1) __syncthreads();
    }
}

bool supported_d(int d) { return d == 8 || d == 16 || d == 32 || d == 64; }

template <bool BWD, typename TX>
int launch(const GMlpArgs &a, int d, hipStream_t st) {
    const double sx = sizeof(TX);
    // bytes: forward x in + y out; backward x, gy in + dxn, xn, gys (2 B) + act (2 B x 4 d) + gpre (2 B x 8 d) out
    const double bytes = (double)a.rows * d * (BWD ? 2 * sx + 2.0 * 3 + 2.0 * 12 : 2 * sx);
    // waves per row tile: 1 while the rows alone fill the chip (d <= 32), hidden-split below that — as for the Mlp
#define VMASR_GMLP_CASE(DD, HS)                                                                                         \
    case DD: {                                                                                                          \
        const dim3 grid(grid_for(a.rows, HS > 1 ? 1 : 4)), block(256);                                                  \
        if (BWD) VMASR_LAUNCH(VMASR_K_GMLP_BWD, bytes, (gmlp_bwd_kernel<DD, TX, HS>), grid, block, 0, st, a);          \
        else VMASR_LAUNCH(VMASR_K_GMLP_FWD, bytes, (gmlp_fwd_kernel<DD, TX, HS>), grid, block, 0, st, a);              \
    } break;
    switch (d) {
        VMASR_GMLP_CASE(8, 1) VMASR_GMLP_CASE(16, 1) VMASR_GMLP_CASE(32, 1) VMASR_GMLP_CASE(64, 4)
        default: set_error("gmlp: unsupported width %d", d); return VMASR_EINVAL;
    }
#undef VMASR_GMLP_CASE
    return check_launch(BWD ? "gmlp_bwd" : "gmlp_fwd");
}

}  // namespace
}  // namespace vmasr

using namespace vmasr;

VMASR_EXPORT int vmasr_gmlp_supported(int32_t d, int32_t hidden) { return supported_d(d) && hidden == 4 * d; }

VMASR_EXPORT int vmasr_gmlp_fwd(const void *x, const float *gamma, const float *beta, float eps, const void *w1, const float *b1,
                                const void *w2, const float *b2, const float *scale, int32_t rows_per_sample, void *y,
                                int64_t rows, int32_t d, int32_t x_dtype, vmasr_stream_t stream) {
    VMASR_REQUIRE(x_dtype == VMASR_F32 || x_dtype == VMASR_BF16, VMASR_EINVAL, "gmlp_fwd: x must be fp32 or bf16");
    VMASR_REQUIRE(x && gamma && beta && w1 && b1 && w2 && b2 && y, VMASR_EINVAL, "gmlp_fwd: null tensor");
    VMASR_REQUIRE(supported_d(d) && rows > 0, VMASR_EINVAL, "gmlp_fwd: need d in {8,16,32,64} (got %d) and rows > 0", d);
    VMASR_REQUIRE(!scale || rows_per_sample > 0, VMASR_EINVAL, "gmlp_fwd: rows_per_sample must be positive with a scale vector");
    VMASR_REQUIRE(aligned_to(x, 16) && aligned_to(y, 16) && aligned_to(w1, 16) && aligned_to(w2, 16) && aligned_to(b1, 16) &&
                      aligned_to(b2, 16), VMASR_EINVAL, "gmlp_fwd: tensors must be 16-byte aligned");
    GMlpArgs a{};
    a.det = det_ticket(VMASR_K_GMLP_FWD);
    a.x = x; a.gamma = gamma; a.beta = beta; a.eps = eps;
    a.w1 = static_cast<const bf16_t *>(w1); a.b1 = b1; a.w2 = static_cast<const bf16_t *>(w2); a.b2 = b2;
    a.scale = scale; a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; a.y = y; a.rows = rows;
    return x_dtype == VMASR_F32 ? launch<false, float>(a, d, static_cast<hipStream_t>(stream))
                                : launch<false, bf16_t>(a, d, static_cast<hipStream_t>(stream));
}

VMASR_EXPORT int vmasr_gmlp_bwd(const void *x, const void *gy, const float *gamma, const float *beta, float eps, const void *w1,
                                const void *w1t, const float *b1, const void *w2t, const float *scale, int32_t rows_per_sample,
                                void *dxn, void *xn_aug, void *gys, void *act_aug, void *gpre, float *mean, float *rstd,
                                int64_t rows, int32_t d, int32_t x_dtype, vmasr_stream_t stream) {
    VMASR_REQUIRE(x_dtype == VMASR_F32 || x_dtype == VMASR_BF16, VMASR_EINVAL, "gmlp_bwd: x / gy must be fp32 or bf16");
    VMASR_REQUIRE(x && gy && gamma && beta && w1 && w1t && b1 && w2t && dxn && xn_aug && gys && act_aug && gpre && mean && rstd,
                  VMASR_EINVAL, "gmlp_bwd: null tensor");
    VMASR_REQUIRE(supported_d(d) && rows > 0, VMASR_EINVAL, "gmlp_bwd: need d in {8,16,32,64} (got %d) and rows > 0", d);
    VMASR_REQUIRE(!scale || rows_per_sample > 0, VMASR_EINVAL, "gmlp_bwd: rows_per_sample must be positive with a scale vector");
    VMASR_REQUIRE(aligned_to(x, 16) && aligned_to(gy, 16) && aligned_to(w1, 16) && aligned_to(w1t, 16) && aligned_to(w2t, 16) &&
                      aligned_to(b1, 16) && aligned_to(dxn, 16) && aligned_to(xn_aug, 16) && aligned_to(gys, 16) &&
                      aligned_to(act_aug, 16) && aligned_to(gpre, 16), VMASR_EINVAL, "gmlp_bwd: tensors must be 16-byte aligned");
    GMlpArgs a{};
    a.det = det_ticket(VMASR_K_GMLP_BWD);
    a.x = x; a.gy = gy; a.gamma = gamma; a.beta = beta; a.eps = eps;
    a.w1 = static_cast<const bf16_t *>(w1); a.w1t = static_cast<const bf16_t *>(w1t); a.b1 = b1;
    a.w2t = static_cast<const bf16_t *>(w2t);
    a.scale = scale; a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; a.rows = rows;
    a.dxn = static_cast<bf16_t *>(dxn); a.xn_aug = static_cast<bf16_t *>(xn_aug); a.gys = static_cast<bf16_t *>(gys);
    a.act_aug = static_cast<bf16_t *>(act_aug); a.gpre = static_cast<bf16_t *>(gpre); a.mean = mean; a.rstd = rstd;
    return x_dtype == VMASR_F32 ? launch<true, float>(a, d, static_cast<hipStream_t>(stream))
                                : launch<true, bf16_t>(a, d, static_cast<hipStream_t>(stream));
}
