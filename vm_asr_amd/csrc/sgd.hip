// sgd.hip — the SGD (momentum / Nesterov) step of all parameters of one optimiser as ONE launch, gfx950.
//
// Reference: torch.optim.SGD as the reference configures it (utils/optimizer.py:32-39: momentum from the yaml, nesterov=True,
// dampening 0, coupled weight decay, 1-D parameters and biases without decay).  The sibling of adamw.hip: the same chunk table
// ((item, chunk) pairs, vmasr_adamw_chunk() elements per workgroup), the same float4 body / scalar tail / misaligned path, the same
// bf16 shadow and transposed-shadow stores from the value just written.  The update is a pure stream — read p, g, buf, write p, buf:
// 20 B per parameter (+ 2 ... 4 B of shadows) — so there is no LDS and every lane moves 16 B per load.
//
// Arithmetic (fp32, torch's SGD with dampening = 0, maximize = False):
//     g' = clip * g + wd * p;  buf = mu * buf + g';  d = nesterov ? g' + mu * buf : buf;  p -= lr * d
// lr is read from DEVICE memory at run time (the schedule keeps working under graph replay); mu and nesterov are launch arguments.
// torch's first step sets buf = g' where no buffer exists; a zero buffer gives the same floats (mu * 0 + g' = g'), which is what the
// host wrapper (vm_asr_amd/fused_sgd.py) creates, so the kernel has no first-step case.  No float atomics: bit-identical run to run.
//
// GUARD (vmasr_sgd_step_guarded): the same body behind the gradient guard's device floats (csrc/gradnorm.hip), read as adamw.hip
// reads them: clip = state[1] multiplies every gradient element as it is read (the gradient buffer is not modified), and when state[2]
// (found_inf) is set every workgroup returns before its first store: p, buf and the shadows stay bit-identical.  SGD keeps no step
// counter, so nothing else is launched.
#include "common.h"

namespace vmasr {
namespace {

constexpr int kSgdChunk = 4096;   // elements per workgroup (256 threads x 4 float4): vmasr_adamw_chunk(), checked by the launcher

template <bool GUARD>
__global__ __launch_bounds__(256) void sgd_kernel(const vmasr_sgd_item *__restrict__ items, const int2 *__restrict__ chunks,
                                                  const float *__restrict__ lr_p, const float mu, const int nesterov,
                                                  const float *__restrict__ guard) {
    float clip = 1.f;
    if constexpr (GUARD) {
        if (guard[2] != 0.f) return;                          // a non-finite gradient somewhere: the step is not taken (uniform over the grid)
        clip = guard[1];
    }
    const int2 ck = chunks[blockIdx.x];                       // (item, chunk index within the item)
    const vmasr_sgd_item it = items[ck.x];
    const long base = (long)ck.y * kSgdChunk;
    const long n = it.n - base < kSgdChunk ? it.n - base : kSgdChunk;
    const float lr = lr_p[0], wd = it.weight_decay;
    float *p = it.p + base, *b = it.buf + base;
    const float *g = it.g + base;
    bf16_t *lp = it.lp ? static_cast<bf16_t *>(it.lp) + base : nullptr;
    bf16_t *lpt = static_cast<bf16_t *>(it.lpt);            // transposed shadow (2-D weights): scattered 2-byte stores, few MB in all
    const int rows = it.rows, cols = it.cols;
    auto put_t = [&](const long i, const float P) {        // i: index within this chunk
        const long gi = base + i;
        const int r = (int)(gi / cols), c = (int)(gi - (long)r * cols);
        lpt[(size_t)c * rows + r] = (bf16_t)P;
    };
    auto upd = [&](float &pp, float gg, float &bb) {
        if constexpr (GUARD) gg *= clip;
        gg = fmaf(wd, pp, gg);
        bb = fmaf(mu, bb, gg);
        pp -= lr * (nesterov ? fmaf(mu, bb, gg) : bb);
    };
    if (it.vec) {   // p, g, buf 16-byte aligned (bf16 shadow: 8); n % 4 != 0 goes through the tail below
        const long n4 = n / 4;
        for (long i = threadIdx.x; i < n4; i += 256) {
            float4 P = reinterpret_cast<float4 *>(p)[i], B = reinterpret_cast<float4 *>(b)[i];
            const float4 G = reinterpret_cast<const float4 *>(g)[i];
            upd(P.x, G.x, B.x); upd(P.y, G.y, B.y); upd(P.z, G.z, B.z); upd(P.w, G.w, B.w);
            reinterpret_cast<float4 *>(p)[i] = P;
            reinterpret_cast<float4 *>(b)[i] = B;
            if (lp) {
                union { uint2 raw; bf16_t b[4]; } o;
                o.b[0] = (bf16_t)P.x; o.b[1] = (bf16_t)P.y; o.b[2] = (bf16_t)P.z; o.b[3] = (bf16_t)P.w;
                reinterpret_cast<uint2 *>(lp)[i] = o.raw;
            }
            if (lpt) { put_t(4 * i, P.x); put_t(4 * i + 1, P.y); put_t(4 * i + 2, P.z); put_t(4 * i + 3, P.w); }
        }
        for (long i = n4 * 4 + threadIdx.x; i < n; i += 256) {
            float P = p[i], B = b[i];
            upd(P, g[i], B);
            p[i] = P; b[i] = B;
            if (lp) lp[i] = (bf16_t)P;
            if (lpt) put_t(i, P);
        }
    } else {
        for (long i = threadIdx.x; i < n; i += 256) {
            float P = p[i], B = b[i];
            upd(P, g[i], B);
            p[i] = P; b[i] = B;
            if (lp) lp[i] = (bf16_t)P;
            if (lpt) put_t(i, P);
        }
    }
}

}  // namespace
}  // namespace vmasr

using namespace vmasr;

template <bool GUARD>
static int sgd_launch(const vmasr_sgd_item *items, const int32_t *chunks, int32_t nchunks, int64_t total_elems, const float *lr,
                      float momentum, int32_t nesterov, const float *guard, vmasr_stream_t stream) {
    VMASR_REQUIRE(items && chunks && lr && (!GUARD || guard), VMASR_EINVAL, "sgd_step: null argument");
    VMASR_REQUIRE(nchunks > 0, VMASR_EINVAL, "sgd_step: nchunks must be positive (got %d)", nchunks);
    VMASR_REQUIRE(momentum >= 0.f && momentum < 1.f, VMASR_EINVAL, "sgd_step: momentum outside [0, 1) (got %g)", (double)momentum);
    VMASR_REQUIRE(vmasr_adamw_chunk() == kSgdChunk, VMASR_EINVAL, "sgd_step: the chunk size differs from vmasr_adamw_chunk()");
    hipStream_t st = static_cast<hipStream_t>(stream);
    VMASR_LAUNCH(VMASR_K_SGD, 20.0 * (double)total_elems, sgd_kernel<GUARD>, dim3(nchunks), dim3(256), 0, st, items,
                 reinterpret_cast<const int2 *>(chunks), lr, momentum, nesterov != 0 ? 1 : 0, guard);
    return check_launch("sgd_step");
}

VMASR_EXPORT int vmasr_sgd_step(const vmasr_sgd_item *items, const int32_t *chunks, int32_t nchunks, int64_t total_elems, const float *lr,
                                float momentum, int32_t nesterov, vmasr_stream_t stream) {
    return sgd_launch<false>(items, chunks, nchunks, total_elems, lr, momentum, nesterov, nullptr, stream);
}

VMASR_EXPORT int vmasr_sgd_step_guarded(const vmasr_sgd_item *items, const int32_t *chunks, int32_t nchunks, int64_t total_elems,
                                        const float *lr, float momentum, int32_t nesterov, const float *state, vmasr_stream_t stream) {
    return sgd_launch<true>(items, chunks, nchunks, total_elems, lr, momentum, nesterov, state, stream);
}
