// mlp_tile.h — the device helpers of the wave-owns-32-rows transposed-MFMA scheme (v_mfma_f32_32x32x16_bf16), shared by the
// VSS-block kernels of mlp.hip (Mlp plain and gated, in_proj, out_proj).  The scheme itself is described at the top of
// mlp.hip; every function here is per-lane, needs no LDS and no barrier (lds_accumulate excepted: the hidden-split epilogue).
#pragma once
#include "common.h"

namespace vmasr {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ f32x16 mfma_bf16(const bf16x8 a, const bf16x8 b, const f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (bf16_t)0.f;
    return z;
}

// The lane's row of x in operand order: element j of k-step s is feature 16 s + 8 h + j (0 beyond D / past the end).
template <typename TX>
__device__ __forceinline__ void load4x(const TX *__restrict__ p, float (&v)[4]) {
    if constexpr (sizeof(TX) == 4) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        const bf16x4 q = *reinterpret_cast<const bf16x4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)q[j];
    }
}

template <typename TX>
__device__ __forceinline__ void store4x(TX *__restrict__ p, const float v0, const float v1, const float v2, const float v3) {
    if constexpr (sizeof(TX) == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(v0, v1, v2, v3);
    } else {
        bf16x4 q;
        q[0] = (bf16_t)v0; q[1] = (bf16_t)v1; q[2] = (bf16_t)v2; q[3] = (bf16_t)v3;
        *reinterpret_cast<bf16x4 *>(p) = q;
    }
}

template <int D, int KS, typename TX>
__device__ __forceinline__ void load_row(const TX *__restrict__ p, const bool ok, const int h, float (&v)[KS][8]) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int f0 = 16 * s + 8 * h;
        if (ok && f0 < D) {
            if constexpr (sizeof(TX) == 4) {
                const float4 q0 = *reinterpret_cast<const float4 *>(p + f0), q1 = *reinterpret_cast<const float4 *>(p + f0 + 4);
                v[s][0] = q0.x; v[s][1] = q0.y; v[s][2] = q0.z; v[s][3] = q0.w;
                v[s][4] = q1.x; v[s][5] = q1.y; v[s][6] = q1.z; v[s][7] = q1.w;
            } else {
                const bf16x8 q = *reinterpret_cast<const bf16x8 *>(p + f0);
#pragma unroll
                for (int j = 0; j < 8; ++j) v[s][j] = (float)q[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[s][j] = 0.f;
        }
    }
}

// two-pass LayerNorm statistics of the row shared by lanes l and l ^ 32
template <int D, int KS>
__device__ __forceinline__ void row_stats(const float (&v)[KS][8], const int h, const float eps, float &mean, float &rstd) {
    float s1 = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int j = 0; j < 8; ++j) s1 += v[s][j];
    s1 += __shfl_xor(s1, 32);
    mean = s1 * (1.f / D);
    float s2 = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
        if (16 * s + 8 * h < D) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float c = v[s][j] - mean;
                s2 = fmaf(c, c, s2);
            }
        }
    s2 += __shfl_xor(s2, 32);
    rstd = rsqrtf(s2 * (1.f / D) + eps);
}

template <int D, int KS>
__device__ __forceinline__ void normalise(const float (&v)[KS][8], const int h, const float mean, const float rstd,
                                          const float *__restrict__ gamma, const float *__restrict__ beta, bf16x8 (&xn)[KS]) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int f0 = 16 * s + 8 * h;
        if (f0 < D) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xn[s][j] = (bf16_t)fmaf((v[s][j] - mean) * rstd, gamma[f0 + j], beta[f0 + j]);
        } else {
            xn[s] = zero8();
        }
    }
}

// H^T tile t (32 hidden units x 32 rows) = W1[32 t .. 32 t + 31, :] . xn^T
template <int D, int KS>
__device__ __forceinline__ f32x16 hidden_tile(const bf16_t *__restrict__ w1, const int t, const int r, const int h,
                                              const bf16x8 (&xn)[KS]) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const bf16_t *wr = w1 + (size_t)(32 * t + r) * D;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int f0 = 16 * s + 8 * h;
        const bf16x8 a = f0 < D ? *reinterpret_cast<const bf16x8 *>(wr + f0) : zero8();
        acc = mfma_bf16(a, xn[s], acc);
    }
    return acc;
}

// fragment of a row-major (n_rows, ld) bf16 matrix W for the PERMUTED k order of an accumulator tile used as operand:
// element j <-> column c0 + 8 (j >> 2) + (j & 3), c0 = 32 t + 16 s2 + 4 h  (two 8-byte loads); zero row when !valid
__device__ __forceinline__ bf16x8 perm_frag(const bf16_t *__restrict__ row_ptr, const int c0, const bool valid) {
    bf16x8 w = zero8();
    if (valid) {
        const bf16x4 lo = *reinterpret_cast<const bf16x4 *>(row_ptr + c0), hi = *reinterpret_cast<const bf16x4 *>(row_ptr + c0 + 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) { w[j] = lo[j]; w[4 + j] = hi[j]; }
    }
    return w;
}

constexpr float kRsqrt2 = 0.70710678118654752f, kInvSqrt2Pi = 0.3989422804014327f;

// Hidden-split workgroups (HS > 1: the deep stages have 1 024 .. 4 096 rows, i.e. 32 .. 128 row tiles — one wave per tile
// would leave the chip empty and walk 8 .. 16 hidden tiles serially): the HS waves of a workgroup share ONE row tile and
// each takes every HS-th hidden tile; their partial output tiles (feature x row, fp32) are summed in LDS with ds_add_f32
// and the epilogue is spread over the waves by 4-feature groups.   s_out[feature * 32 + row]
template <int OT>
__device__ __forceinline__ void lds_accumulate(float *s_out, const f32x16 (&acc)[OT], const int r, const int h) {
#pragma unroll
    for (int u = 0; u < OT; ++u)
#pragma unroll
        for (int i = 0; i < 16; ++i) atomicAdd(s_out + (32 * u + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r, acc[u][i]);
}

__device__ __forceinline__ void store_bf16x4(bf16_t *p, const float v0, const float v1, const float v2, const float v3) {
    bf16x4 q;
    q[0] = (bf16_t)v0; q[1] = (bf16_t)v1; q[2] = (bf16_t)v2; q[3] = (bf16_t)v3;
    *reinterpret_cast<bf16x4 *>(p) = q;
}

inline int grid_for(long rows, int tiles_per_wg) {
    const long tiles = ((rows + 31) / 32 + tiles_per_wg - 1) / tiles_per_wg;
    return (int)(tiles < 2048 ? (tiles < 1 ? 1 : tiles) : 2048);
}

}  // namespace
}  // namespace vmasr
