// Fused global-norm clip + AdamW over the FLAT fp32 parameter / gradient arena (gfx950, HBM-bound).
//
// Replaces, per optimizer step, `torch.nn.utils.clip_grad_norm_(params, max_grad_norm)` (TF:trainer.py:1780-1782) followed by
// `torch.optim.AdamW.step` (HF Trainer with optim="adamw_torch" / "adamw_torch_fused", TF:trainer_optimizer.py:201-208) over the
// two weight-decay groups: ~10 elementwise torch passes x ~230 tensors become TWO launches.
//
//   A  aw_sumsq : one in-order sweep over g: per-block partial sums of g^2 (grid-strided 8192-float tiles, fixed order)
//   B  aw_apply : every block reduces the partials in the same fixed order (global norm, clip coefficient), then updates one
//                 work item (<= 4096 contiguous floats of one tensor) in torch's order of operations:
//                   g = grad * coef
//                   p = p * (1 - lr wd)
//                   m = m + (1 - b1) (g - m)                            (torch: exp_avg.lerp_(g, 1 - b1))
//                   v = b2 v + (1 - b2) g g
//                   p = p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
//                 Work items run in DESCENDING arena order: the tail of g that A streamed last is still in the 256 MiB
//                 Infinity Cache when B starts.
//
// HBM traffic: g twice + p, m, v read and written = 32 N bytes (N = arena floats); g cannot be consumed in one pass because
// the clip coefficient needs the norm of ALL gradients first.  Plain float4 loads / stores: every tensor starts on a 64-float
// boundary and every work item covers a multiple of 4 floats, so there are no scalar tails.  `grads` is read only.
//
// No float atomics: all data-parallel ranks compute bit-identical updates from bit-identical all-reduced gradients, and two
// runs of the same step are bitwise equal.
#include "common.h"
#include "desta_hip.h"

namespace {

constexpr int NT = 256;
constexpr int SUMSQ_V4 = 8;                       // float4 loads in flight per thread in A
constexpr int TILE_V4 = NT * SUMSQ_V4;            // float4 per tile of A (8192 floats)
constexpr int MAX_PARTIALS = 1024;                // blocks of A (4 per CU): the partials B re-reads are <= 4 KB
constexpr int ITEM_V4 = 4;                        // float4 per thread and stream in B (16 float4 = 64 VGPRs in flight)
constexpr int ITEM = NT * 4 * ITEM_V4;            // floats per work item of B
static_assert(ITEM == DESTA_ADAMW_ITEM_FLOATS, "work-item size of the ABI");

__host__ __device__ inline int n_partials(int64_t numel) {
    const int64_t tiles = (numel / 4 + TILE_V4 - 1) / TILE_V4;
    return (int)(tiles < MAX_PARTIALS ? (tiles > 0 ? tiles : 1) : MAX_PARTIALS);
}

// ------------------------------------------------------------------------------------------------ A: sum of squares
// block b sums tiles b, b + nb, b + 2 nb, ...: the grid sweeps the arena in order, so its last 256 MiB are what the
// Infinity Cache holds when B starts at the end of the arena
__global__ __launch_bounds__(NT) void aw_sumsq(const float4* __restrict__ g, int64_t n4, float* __restrict__ partial) {
    __shared__ float red[NT / 64];
    const int nb = gridDim.x;
    float s = 0.f;
    for (int64_t t = blockIdx.x; t * TILE_V4 < n4; t += nb) {
        const int64_t base = t * TILE_V4 + threadIdx.x;
        float4 x[SUMSQ_V4];
#pragma unroll
        for (int j = 0; j < SUMSQ_V4; ++j) {
            const int64_t i = base + (int64_t)j * NT;
            x[j] = i < n4 ? g[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < SUMSQ_V4; ++j) s += (x[j].x * x[j].x + x[j].y * x[j].y) + (x[j].z * x[j].z + x[j].w * x[j].w);
    }
    s = block_sum<NT>(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------ B: norm + update
struct Hyper {
    float lr, omb1, b2, omb2, eps, step_size, sqrt_bc2, max_norm;
};

// rounding points of torch's CPU single-tensor AdamW: every op rounds on its own, except lerp (ATen's vectorised lerp is one fmadd)
__device__ __forceinline__ void adamw_one(float gr, float& p, float& m, float& v, float coef, float decay, const Hyper& h) {
    const float g = __fmul_rn(gr, coef);                                             // clip: grad.mul_(coef)
    p = __fmul_rn(p, decay);                                                         // param.mul_(1 - lr wd)
    m = fmaf(h.omb1, g - m, m);                                                      // exp_avg.lerp_(g, 1 - b1)
    v = __fadd_rn(__fmul_rn(v, h.b2), __fmul_rn(__fmul_rn(h.omb2, g), g));           // exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
    const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), h.sqrt_bc2), h.eps);           // (sqrt(v) / sqrt(bc2)).add_(eps)
    p = __fsub_rn(p, __fmul_rn(h.step_size, __fdiv_rn(m, denom)));                   // param.addcdiv_(m, denom, -lr / bc1)
}

__global__ __launch_bounds__(NT) void aw_apply(const int64_t* __restrict__ items, const float* __restrict__ item_wd, int n_items,
                                               const float* __restrict__ g, float* __restrict__ p, float* __restrict__ m,
                                               float* __restrict__ v, int64_t numel, float* __restrict__ ws, int npart, Hyper h) {
    __shared__ float red[NT / 64];
    const int it = n_items - 1 - (int)blockIdx.x;                          // descending arena order
    const int64_t off = items[2 * it + 0];
    const int64_t cnt = items[2 * it + 1];
    // a malformed item touches nothing (n4 = 0); the block still takes part in the reduction below
    const bool ok = off >= 0 && !(off & 3) && cnt >= 0 && cnt <= ITEM && !(cnt & 3) && off + cnt <= numel;
    const int n4 = ok ? (int)(cnt >> 2) : 0;
    const float4* g4 = (const float4*)(g + off);
    float4* p4 = (float4*)(p + off);
    float4* m4 = (float4*)(m + off);
    float4* v4 = (float4*)(v + off);
    // the item's loads go out first: the partial-sum reduction runs while they are in flight
    float4 gv[ITEM_V4], pv[ITEM_V4], mv[ITEM_V4], vv[ITEM_V4];
#pragma unroll
    for (int j = 0; j < ITEM_V4; ++j) {
        const int i = j * NT + threadIdx.x;
        if (i < n4) { gv[j] = g4[i]; pv[j] = p4[i]; mv[j] = m4[i]; vv[j] = v4[i]; }
    }
    const float* partial = ws + 8;
    float s = 0.f;
    for (int i = threadIdx.x; i < npart; i += NT) s += partial[i];          // same partition + order in every block
    s = block_sum<NT>(s, red);
    const float gn = sqrtf(s);
    const float coef = h.max_norm > 0.f ? fminf(h.max_norm / (gn + 1e-6f), 1.0f) : 1.0f;
    if (blockIdx.x == 0 && threadIdx.x == 0) { ws[0] = gn; ws[1] = coef; }
    const float decay = ok ? (float)(1.0 - (double)h.lr * (double)item_wd[it]) : 1.0f;
#pragma unroll
    for (int j = 0; j < ITEM_V4; ++j) {
        const int i = j * NT + threadIdx.x;
        if (i < n4) {
            adamw_one(gv[j].x, pv[j].x, mv[j].x, vv[j].x, coef, decay, h);
            adamw_one(gv[j].y, pv[j].y, mv[j].y, vv[j].y, coef, decay, h);
            adamw_one(gv[j].z, pv[j].z, mv[j].z, vv[j].z, coef, decay, h);
            adamw_one(gv[j].w, pv[j].w, mv[j].w, vv[j].w, coef, decay, h);
            p4[i] = pv[j]; m4[i] = mv[j]; v4[i] = vv[j];
        }
    }
}

}  // namespace

extern "C" size_t desta_adamw_workspace_floats(const desta_adamw_plan* pl) {
    return pl ? 8 + (size_t)n_partials(pl->numel) : 0;
}

extern "C" int desta_clip_adamw_step(const desta_adamw_plan* pl, float* params, const float* grads, float* exp_avg,
                                     float* exp_avg_sq, float* workspace, float lr, double beta1, double beta2, float eps,
                                     float bc1, float bc2, float max_grad_norm, void* stream) {
    DESTA_CHECK_ARG(pl && params && grads && exp_avg && exp_avg_sq && workspace, "adamw: null argument");
    DESTA_CHECK_ARG(pl->numel > 0 && pl->numel % 4 == 0, "adamw: arena of %lld floats (must be a positive multiple of 4)",
                    (long long)pl->numel);
    DESTA_CHECK_ARG(pl->n_items > 0 && pl->items && pl->item_wd, "adamw: plan without work items");
    DESTA_CHECK_ARG(bc1 > 0.f && bc2 > 0.f, "adamw: bias corrections must be > 0 (bc1 %g, bc2 %g)", (double)bc1, (double)bc2);
    Hyper h;
    h.lr = lr;
    h.omb1 = (float)(1.0 - beta1);                  // 1 - beta in double, then fp32: what torch's scalar arguments are
    h.b2 = (float)beta2;
    h.omb2 = (float)(1.0 - beta2);
    h.eps = eps;
    h.step_size = (float)((double)lr / (double)bc1);
    h.sqrt_bc2 = (float)sqrt((double)bc2);
    h.max_norm = max_grad_norm;
    const int npart = n_partials(pl->numel);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(aw_sumsq, dim3(npart), dim3(NT), 0, st, (const float4*)grads, pl->numel / 4, workspace + 8);
    hipLaunchKernelGGL(aw_apply, dim3(pl->n_items), dim3(NT), 0, st, pl->items, pl->item_wd, pl->n_items, grads, params, exp_avg,
                       exp_avg_sq, pl->numel, workspace, npart, h);
    DESTA_CHECK_LAUNCH("clip_adamw_step");
    return DESTA_OK;
}
