// Row-wise normalisation / activation / layout kernels of the DeSTA2.5 step (gfx950, all HBM-bound:
// 16-B per-lane accesses, one wave per row, fp32 statistics, everything else fused into the GEMM
// epilogues).  Reference call sites (TF: = transformers 5.15):
//   LayerNorm fwd/bwd ... TF:models/whisper/modeling_whisper.py:392,402 (pre-LN, eps 1e-5),
//                         TF:models/bert/modeling_bert.py:296,350 (post-LN, eps 1e-12),
//                         modeling_desta25.py:166 (proj.0)
//   RMSNorm fwd/bwd ..... TF:models/llama/modeling_llama.py:53-67
//   RoPE (+ q/k norm) ... TF:models/llama/modeling_llama.py:126-160, TF:models/qwen3/modeling_qwen3.py:237-257
//   SwiGLU .............. TF:models/llama/modeling_llama.py:163-176
//   GELU' ............... autograd of F.gelu (erf form)
#include "common.h"
#include "desta_hip.h"

namespace {

constexpr int RPB = 4;  // rows per block = waves per block

__device__ __forceinline__ void load8(const void* base, long idx, int is_f32, float* v) {
    if (is_f32) {
        const float4 a = *(const float4*)((const float*)base + idx);
        const float4 b = *(const float4*)((const float*)base + idx + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const u16x8 a = *(const u16x8*)((const bf16_t*)base + idx);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = bf2f(a[e]);
    }
}
__device__ __forceinline__ void store8_bf16(bf16_t* base, long idx, const float* v) {
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e]);
    *(u16x8*)(base + idx) = o;
}
__device__ __forceinline__ void store8_f32(float* base, long idx, const float* v) {
    *(float4*)(base + idx) = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)(base + idx + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// ------------------------------------------------------------------------------------ LayerNorm
template <int MAXV>
__global__ __launch_bounds__(256) void layernorm_fwd_k(const void* __restrict__ x, int x_f32, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float eps, int rows, int cols,
                                                       bf16_t* __restrict__ y16, float* __restrict__ y32,
                                                       float* __restrict__ stats) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * RPB + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[MAXV][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < cols) {
            load8(x, (long)row * cols + c, x_f32, v[i]);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[i][e];
        }
    }
    const float mean = wave_sum(s) / (float)cols;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < cols) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; q += d * d; }
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)cols + eps);
    if (stats && lane == 0) { stats[2 * row] = mean; stats[2 * row + 1] = rstd; }
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < cols) {
            float g[8], b[8], o[8];
            load8(gamma, c, 1, g);
            load8(beta, c, 1, b);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (v[i][e] - mean) * rstd * g[e] + b[e];
            if (y16) store8_bf16(y16, (long)row * cols + c, o);
            if (y32) store8_f32(y32, (long)row * cols + c, o);
        }
    }
}

// dx and per-block partial dgamma/dbeta.  part: [gridDim.x][2][cols]
template <int MAXV>
__global__ __launch_bounds__(256) void layernorm_bwd_k(const void* __restrict__ dy, int dy_f32, const void* __restrict__ x,
                                                       int x_f32, const float* __restrict__ gamma,
                                                       const float* __restrict__ stats, int rows, int cols,
                                                       float* __restrict__ dx32, bf16_t* __restrict__ dx16,
                                                       float* __restrict__ part) {
    __shared__ float comb[RPB][64 * 8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float dg[MAXV][8], db[MAXV][8];
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) { dg[i][e] = 0.f; db[i][e] = 0.f; }
    for (int row = blockIdx.x * RPB + wave; row < rows; row += gridDim.x * RPB) {
        const float mean = stats[2 * row], rstd = stats[2 * row + 1];
        float xh[MAXV][8], gy[MAXV][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * 8;
            if (c < cols) {
                float xv[8], dyv[8], g[8];
                load8(x, (long)row * cols + c, x_f32, xv);
                load8(dy, (long)row * cols + c, dy_f32, dyv);
                load8(gamma, c, 1, g);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    xh[i][e] = (xv[e] - mean) * rstd;
                    gy[i][e] = dyv[e] * g[e];
                    s1 += gy[i][e];
                    s2 += gy[i][e] * xh[i][e];
                    dg[i][e] += dyv[e] * xh[i][e];
                    db[i][e] += dyv[e];
                }
            }
        }
        s1 = wave_sum(s1) / (float)cols;
        s2 = wave_sum(s2) / (float)cols;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * 8;
            if (c < cols) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = rstd * (gy[i][e] - s1 - xh[i][e] * s2);
                if (dx32) store8_f32(dx32, (long)row * cols + c, o);
                if (dx16) store8_bf16(dx16, (long)row * cols + c, o);
            }
        }
    }
    if (!part) return;
    // combine the block's 4 waves (fixed order) and write the partial rows
    for (int which = 0; which < 2; ++which) {
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            if (i * 512 < cols) {
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 8; ++e) comb[wave][lane * 8 + e] = which ? db[i][e] : dg[i][e];
                __syncthreads();
                for (int j = threadIdx.x; j < 512; j += 256) {
                    const int c = i * 512 + j;
                    if (c < cols)
                        part[((long)blockIdx.x * 2 + which) * cols + c] = (comb[0][j] + comb[1][j]) + (comb[2][j] + comb[3][j]);
                }
            }
        }
    }
}

// out[which][c] (+)= sum_b part[b][which][c];  also used for column sums (bias gradients).  64 columns per block, the
// partial rows are split over the block's 4 waves (4 independent accumulators each) and combined in fixed order.
__global__ __launch_bounds__(1024) void reduce_partials_k(const float* __restrict__ part, int nblk, int width,
                                                          float* __restrict__ out0, float* __restrict__ out1, int cols,
                                                          int accumulate) {
    // 16 wave groups x 4 independent accumulators: the partial rows are a chain of dependent loads per accumulator (256 rows:
    // 4 rounds instead of the 16 that a 4-group block needs)
    __shared__ float comb[16][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (c < width) {
        int b = grp;
        for (; b + 48 < nblk; b += 64) {
            a0 += part[(long)b * width + c];
            a1 += part[(long)(b + 16) * width + c];
            a2 += part[(long)(b + 32) * width + c];
            a3 += part[(long)(b + 48) * width + c];
        }
        for (; b < nblk; b += 16) a0 += part[(long)b * width + c];
    }
    comb[grp][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (grp == 0 && c < width) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < 16; g += 4) s += (comb[g][lane] + comb[g + 1][lane]) + (comb[g + 2][lane] + comb[g + 3][lane]);
        float* o = (c < cols) ? out0 + c : out1 + (c - cols);
        *o = accumulate ? *o + s : s;
    }
}

// column sums of a bf16 [rows, cols] matrix -> per-block partials [gridDim.y][cols]; V columns per thread (8 = 16-B loads)
template <int V>
__global__ __launch_bounds__(256) void colsum_partial_k(const bf16_t* __restrict__ x, int rows, int cols, long ld,
                                                        float* __restrict__ part) {
    typedef __attribute__((ext_vector_type(V))) unsigned short vec_t;
    const int c = (blockIdx.x * 256 + threadIdx.x) * V;
    if (c >= cols) return;
    const int r0 = blockIdx.y, nr = gridDim.y;
    float s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f;
#pragma unroll 8
    for (int r = r0; r < rows; r += nr) {
        const vec_t v = *(const vec_t*)(x + (long)r * ld + c);
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] += bf2f(v[e]);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) part[(long)r0 * cols + c + e] = s[e];
}
// row splits: enough blocks to fill the chip on tall matrices (the [48000, 2560] d(K|V) of the cross-attention ran at
// 1.5 TB/s with 64 splits x 3 column blocks), at least ~8 rows per split: the 2048-row bias gradients of the Q-Former are
// latency-bound chains of row loads (32 rows per split = 8 dependent rounds of 4 loads: 17.8 us for 5 MB; 8 rows = one round)
static int colsum_splits(int rows, int cols) {
    const int xb = (cols / 4 + 255) / 256;
    int nr = (2048 + xb - 1) / xb;
    if (nr > rows / 8) nr = rows / 8;
    if (nr > 512) nr = 512;
    if (nr < 1) nr = 1;
    return nr;
}

// ------------------------------------------------------------------------------------ RMSNorm
template <int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_fwd_k(const bf16_t* __restrict__ x, const float* __restrict__ w, float eps,
                                                     int rows, int cols, bf16_t* __restrict__ y, float* __restrict__ rstd_out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * RPB + (threadIdx.x >> 6);
    if (row >= rows) return;
    float v[MAXV][8];
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < cols) {
            load8(x, (long)row * cols + c, 0, v[i]);
#pragma unroll
            for (int e = 0; e < 8; ++e) q += v[i][e] * v[i][e];
        }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)cols + eps);
    if (rstd_out && lane == 0) rstd_out[row] = rstd;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < cols) {
            float g[8], o[8];
            load8(w, c, 1, g);
            // HF: weight * (x * rstd).to(bf16)  -> round the normalised value first
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = g[e] * bf2f(f2bf(v[i][e] * rstd));
            store8_bf16(y, (long)row * cols + c, o);
        }
    }
}

// dx = [dres +] rstd * (w*dy - xhat * mean(w*dy*xhat))
template <int MAXV>
__global__ __launch_bounds__(256) void rmsnorm_bwd_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                     const float* __restrict__ w, const float* __restrict__ rstd_in,
                                                     const bf16_t* __restrict__ dres, int rows, int cols,
                                                     bf16_t* __restrict__ dx) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * RPB + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float rstd = rstd_in[row];
    // every load of the row is issued up front and kept as raw bf16 (12 registers per 8 columns instead of 16 floats + a
    // second, dependent residual load after the reduction): a one-row wave exposes ONE memory latency and three waves fit a SIMD
    u16x8 xr[MAXV], dyr[MAXV], rres[MAXV];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < cols) {
            xr[i] = *(const u16x8*)(x + (long)row * cols + c);
            dyr[i] = *(const u16x8*)(dy + (long)row * cols + c);
            if (dres) rres[i] = *(const u16x8*)(dres + (long)row * cols + c);
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < cols) {
            float g[8];
            load8(w, c, 1, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) s += (bf2f(dyr[i][e]) * g[e]) * (bf2f(xr[i][e]) * rstd);
        }
    }
    s = wave_sum(s) / (float)cols;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) asm volatile("" : "+v"(xr[i]), "+v"(dyr[i]));        // opaque: convert again below instead of keeping 16 floats per vector alive
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * 8;
        if (c < cols) {
            float g[8], o[8];
            load8(w, c, 1, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = rstd * (bf2f(dyr[i][e]) * g[e] - (bf2f(xr[i][e]) * rstd) * s);
            if (dres) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] += bf2f(rres[i][e]);
            }
            store8_bf16(dx, (long)row * cols + c, o);
        }
    }
}

// ------------------------------------------------------------------------------------ RoPE (+ per-head q/k RMSNorm)
// buf: [rows, ld] bf16; heads [0, n_heads) of width HD starting at column 0 are rotated in place.
// G = HD/16 lanes own one head: lane j holds elements 8j..8j+7 of both halves.
// NORM: 0 = plain rope; 1 = fwd (rmsnorm with weight then rope); 2 = bwd of (1) given saved pre-norm x.
// KV-cache append (generate()): with kv.dst the grid also covers the V heads that follow K in `buf`; rotated K heads and
// plain V heads of row (b, s) are ALSO written to kv.dst + b*bs + (slot0 + s)*rs + (head - n_q)*HD (the K|V slab).
// BIAS (Qwen2 / Qwen2.5, TF:models/qwen2/modeling_qwen2.py attention: q_proj, k_proj, v_proj = nn.Linear(bias=True)): the
// projection GEMM stays bias-free on every path and leaves bf16(x W^T); the kernel that rotates adds the fp32 bias
// [(n_q + 2 n_kv) * HD] to the row, rotates q and k in fp32 and rounds once, and rounds v as bf16(v + b).  So a BIAS grid always
// covers the n_kv V heads, cache or not, which the bias-free forms touch only to copy them into a cache.
// No q/k-norm (no model has both), no backward (d(pre-bias) = d(post-bias), the bias itself is frozen).  With a zero bias the
// q|k bits are the bias-free ones: x + 0 = x (an input of -0 would come out as +0; a GEMM output is not -0).
struct RopeKV { bf16_t* dst; long bs, rs; int slot0; int n_v; };
// Thread -> (head group, lane j of its G = HD/16) -> (row, head) over rows x all_heads heads.  Lanes past the end keep row 0,
// head 0 with active = false: a head is G adjacent lanes, and the norm and the FP8 amax shuffle over the whole group.
struct RopeLane { int j, row, head; bool active; };
template <int HD>
__device__ __forceinline__ RopeLane rope_lane(int rows, int n_heads, int n_v) {
    constexpr int G = HD / 16;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long grp = gid / G;
    RopeLane t;
    t.j = (int)(gid % G);
    const int all_heads = n_heads + n_v;
    t.active = grp < (long)rows * all_heads;
    t.row = t.active ? (int)(grp / all_heads) : 0;
    t.head = t.active ? (int)(grp % all_heads) : 0;
    return t;
}
// position_ids: arange(S) for every row in training (H7); generate() passes a per-sequence shift
// (-left_pad for the prompt, cache_length - left_pad for a decode step) as HF derives them from the mask
// sm_batch > 0: the token grid is stored position-major (row = s * batch + b), else batch-major (row = b * S + s)
__device__ __forceinline__ int rope_pos(int row, int S, int sm_batch, const int* pos_shift) {
    const int spos = sm_batch ? row / sm_batch : row % S, bidx = sm_batch ? row % sm_batch : row / S;
    return pos_shift ? max(0, spos + pos_shift[bidx]) : spos;
}
// Where K or V head `head` of batch-major row (b, s) goes in a cache laid out [batch: bs][slot: rs][n_kv K heads | n_kv V heads] with
// W elements per head: the K|V slab (W = HD) and the FP8 cache's scales (W = 1).
template <int W, typename T>
__device__ __forceinline__ T* rope_slot(T* dst, long bs, long rs, int slot0, int row, int S, int head, int n_q) {
    return dst + (long)(row / S) * bs + (long)(slot0 + row % S) * rs + (long)(head - n_q) * W;
}
// Lane j's 2 x 8 elements of the head at p, forward: load, BIAS: add bias[0..HD) in fp32, NORM == 1: RMSNorm with weight w
// (rounded to bf16 twice as HF does), then the rotation at position pos, or rotate == false (a V head): pass through.  Every
// lane of a head group has to get here: the norm's sum is a shuffle over the group.
template <int HD, int NORM, bool BIAS>
__device__ __forceinline__ void rope_head(const bf16_t* p, int j, bool rotate, int pos, const float* __restrict__ cs, const float* __restrict__ w,
                                          float eps, const float* __restrict__ bias, float (&oa)[8], float (&ob)[8]) {
    constexpr int G = HD / 16, H2 = HD / 2;
    float a[8], b[8];
    load8(p, 8 * j, 0, a);
    load8(p, H2 + 8 * j, 0, b);
    if constexpr (BIAS) {
        float ba[8], bb[8];
        load8(bias, 8 * j, 1, ba);
        load8(bias, H2 + 8 * j, 1, bb);
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] += ba[e]; b[e] += bb[e]; }
    }
    if (!rotate) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { oa[e] = a[e]; ob[e] = b[e]; }
        return;
    }
    float c[8], s[8];
    load8(cs, ((long)pos * 2) * H2 + 8 * j, 1, c);
    load8(cs, ((long)pos * 2 + 1) * H2 + 8 * j, 1, s);
    // The sums of two products are spelled as fmaf(x, y, u * v): under -ffp-contract=fast the compiler is free to fuse either
    // product of "x * y + u * v", and which one it takes varies with the code around it, so the kernels that inline this
    // would not round alike.  These are the forms the kernels were compiled to before the rotation became one function.
    if constexpr (NORM == 1) {
        float q = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) q += fmaf(a[e], a[e], b[e] * b[e]);
#pragma unroll
        for (int o = 1; o < G; o <<= 1) q += __shfl_xor(q, o, 64);
        const float rstd = rsqrtf(q / (float)HD + eps);
        float wa[8], wb[8];
        load8(w, 8 * j, 1, wa);
        load8(w, H2 + 8 * j, 1, wb);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            a[e] = bf2f(f2bf(wa[e] * bf2f(f2bf(a[e] * rstd))));
            b[e] = bf2f(f2bf(wb[e] * bf2f(f2bf(b[e] * rstd))));
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { oa[e] = fmaf(a[e], c[e], -(b[e] * s[e])); ob[e] = fmaf(b[e], c[e], a[e] * s[e]); }
}
// n_heads = n_q + n_kv rotated heads, then the V heads: kv.n_v of them (0 without a cache), BIAS: always n_kv = n_heads - n_q.
// kv.dst == nullptr: in place only (training / eval forward).  BIAS is instantiated for NORM == 0, BWD == false only.
template <int HD, int NORM, bool BWD, bool BIAS>
__global__ __launch_bounds__(256) void rope_k(bf16_t* __restrict__ buf, long ld, int rows, int S, int n_heads, int n_q,
                                              const float* __restrict__ cs, const float* __restrict__ wq,
                                              const float* __restrict__ wk, float eps, const bf16_t* __restrict__ pre,
                                              long ld_pre, const int* __restrict__ pos_shift, RopeKV kv, int sm_batch,
                                              const float* __restrict__ bias) {
    constexpr int G = HD / 16, H2 = HD / 2;
    const RopeLane t = rope_lane<HD>(rows, n_heads, BIAS ? n_heads - n_q : kv.n_v);
    const int j = t.j, row = t.row, head = t.head;
    if constexpr (BIAS) {
        if (!t.active) return;                                           // no whole-wave op follows
    } else if (!BWD && head >= n_heads) {                                // V head: copy into the cache (no whole-wave op follows)
        const bf16_t* src = buf + (long)row * ld + (long)head * HD;
        bf16_t* d = rope_slot<HD>(kv.dst, kv.bs, kv.rs, kv.slot0, row, S, head, n_q);
        *(u16x8*)(d + 8 * j) = *(const u16x8*)(src + 8 * j);
        *(u16x8*)(d + H2 + 8 * j) = *(const u16x8*)(src + H2 + 8 * j);
        return;
    }
    const int pos = rope_pos(row, S, sm_batch, pos_shift);
    bf16_t* p = buf + (long)row * ld + (long)head * HD;
    if (!BWD) {
        float oa[8], ob[8];
        rope_head<HD, NORM, BIAS>(p, j, !BIAS || head < n_heads, pos, cs, head < n_q ? wq : wk, eps, BIAS ? bias + (long)head * HD : nullptr, oa, ob);
        if (t.active) {
            store8_bf16(p, 8 * j, oa); store8_bf16(p, H2 + 8 * j, ob);
            if (kv.dst && head >= n_q) {                                 // cache rows are batch-major (the entry points pass sm_batch = 0)
                bf16_t* d = rope_slot<HD>(kv.dst, kv.bs, kv.rs, kv.slot0, row, S, head, n_q);
                store8_bf16(d, 8 * j, oa); store8_bf16(d, H2 + 8 * j, ob);
            }
        }
    } else {
        float a[8], b[8], c[8], s[8];
        load8(p, 8 * j, 0, a);
        load8(p, H2 + 8 * j, 0, b);
        load8(cs, ((long)pos * 2) * H2 + 8 * j, 1, c);
        load8(cs, ((long)pos * 2 + 1) * H2 + 8 * j, 1, s);
        float ga[8], gb[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { ga[e] = a[e] * c[e] + b[e] * s[e]; gb[e] = b[e] * c[e] - a[e] * s[e]; }
        if (NORM == 2) {
            const float* w = head < n_q ? wq : wk;
            const bf16_t* pp = pre + (long)row * ld_pre + (long)head * HD;
            float xa[8], xb[8], wa[8], wb[8];
            load8(pp, 8 * j, 0, xa);
            load8(pp, H2 + 8 * j, 0, xb);
            load8(w, 8 * j, 1, wa);
            load8(w, H2 + 8 * j, 1, wb);
            float q = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) q += xa[e] * xa[e] + xb[e] * xb[e];
#pragma unroll
            for (int o = 1; o < G; o <<= 1) q += __shfl_xor(q, o, 64);
            const float rstd = rsqrtf(q / (float)HD + eps);
            float t = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                ga[e] *= wa[e]; gb[e] *= wb[e];
                xa[e] *= rstd; xb[e] *= rstd;
                t += ga[e] * xa[e] + gb[e] * xb[e];
            }
#pragma unroll
            for (int o = 1; o < G; o <<= 1) t += __shfl_xor(t, o, 64);
            t /= (float)HD;
#pragma unroll
            for (int e = 0; e < 8; ++e) { ga[e] = rstd * (ga[e] - xa[e] * t); gb[e] = rstd * (gb[e] - xb[e] * t); }
        }
        if (t.active) { store8_bf16(p, 8 * j, ga); store8_bf16(p, H2 + 8 * j, gb); }
    }
}

// ------------------------------------------------------------------------------------ SwiGLU / GELU'
// gu: [rows, 2*I] (gate | up); act: [rows, I]
__global__ __launch_bounds__(256) void swiglu_fwd_k(const bf16_t* __restrict__ gu, bf16_t* __restrict__ act, long rows, int I) {
    const long n8 = rows * (I / 8);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        const long r = i / (I / 8);
        const int c = (int)(i % (I / 8)) * 8;
        float g[8], u[8], o[8];
        load8(gu, r * 2 * I + c, 0, g);
        load8(gu, r * 2 * I + I + c, 0, u);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float sg = g[e] / (1.0f + __expf(-g[e]));
            o[e] = bf2f(f2bf(sg)) * u[e];                  // HF rounds silu(gate) to bf16 before the product
        }
        store8_bf16(act, r * I + c, o);
    }
}
__global__ __launch_bounds__(256) void swiglu_bwd_k(const bf16_t* __restrict__ gu, const bf16_t* __restrict__ dact,
                                                    bf16_t* __restrict__ dgu, long rows, int I) {
    const long n8 = rows * (I / 8);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        const long r = i / (I / 8);
        const int c = (int)(i % (I / 8)) * 8;
        float g[8], u[8], d[8], dg[8], du[8];
        load8(gu, r * 2 * I + c, 0, g);
        load8(gu, r * 2 * I + I + c, 0, u);
        load8(dact, r * I + c, 0, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float sig = 1.0f / (1.0f + __expf(-g[e]));
            const float sg = g[e] * sig;
            du[e] = d[e] * sg;
            dg[e] = d[e] * u[e] * (sig * (1.0f + g[e] * (1.0f - sig)));
        }
        store8_bf16(dgu, r * 2 * I + c, dg);
        store8_bf16(dgu, r * 2 * I + I + c, du);
    }
}
__global__ __launch_bounds__(256) void gelu_bwd_k(const bf16_t* __restrict__ pre, const bf16_t* __restrict__ dact,
                                                  bf16_t* __restrict__ dpre, long n8) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        float x[8], d[8], o[8];
        load8(pre, i * 8, 0, x);
        load8(dact, i * 8, 0, d);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = d[e] * gelu_erf_grad(x[e]);
        store8_bf16(dpre, i * 8, o);
    }
}

// ------------------------------------------------------------------------------------ casts / transposes / adds
__global__ __launch_bounds__(256) void cast_f32_bf16_k(const float* __restrict__ x, bf16_t* __restrict__ y, long n8) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
        float v[8];
        load8(x, i * 8, 1, v);
        store8_bf16(y, i * 8, v);
    }
}
__global__ __launch_bounds__(256) void add_f32_k(float* __restrict__ y, const float* __restrict__ x, long n4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 a = ((float4*)y)[i];
        const float4 b = ((const float4*)x)[i];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        ((float4*)y)[i] = a;
    }
}
// out[c][r] = in[r][c]; out has ld_out >= rows columns, tail [rows, ld_out) zero filled. 64x64 tiles via LDS.
template <bool IN_F32>
__global__ __launch_bounds__(256) void transpose_k(const void* __restrict__ in, long ld_in, int rows, int cols,
                                                   bf16_t* __restrict__ out, long ld_out) {
    __shared__ bf16_t tile[64][66];
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = r0 + i, c = c0 + tx;
        bf16_t v = 0;
        if (r < rows && c < cols) v = IN_F32 ? f2bf(((const float*)in)[(long)r * ld_in + c]) : ((const bf16_t*)in)[(long)r * ld_in + c];
        tile[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < ld_out) out[(long)c * ld_out + r] = tile[tx][i];
    }
}

// Same contract, 16-byte global accesses on both sides (cols, ld_in, ld_out multiples of 8, 16-B aligned pointers):
// a thread moves 2 x 8 elements in and 2 x 8 out instead of 16 + 16 two-byte accesses (the [48000, 2560] d(K|V)
// transpose of the cross-attention ran at 2.6 TB/s on the scalar kernel).
template <bool IN_F32>
__global__ __launch_bounds__(256) void transpose_vec_k(const void* __restrict__ in, long ld_in, int rows, int cols,
                                                       bf16_t* __restrict__ out, long ld_out) {
    __shared__ __attribute__((aligned(16))) bf16_t tile[64][72];          // tile[c][r], 144-B rows
    const int r0 = blockIdx.y * 64, c0 = blockIdx.x * 64;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = i * 256 + threadIdx.x;
        const int r = idx >> 3, ch = idx & 7, c = c0 + ch * 8;
        u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (r0 + r < rows && c < cols) {
            if (IN_F32) {
                const float4 a = *(const float4*)((const float*)in + (long)(r0 + r) * ld_in + c);
                const float4 b = *(const float4*)((const float*)in + (long)(r0 + r) * ld_in + c + 4);
                v[0] = f2bf(a.x); v[1] = f2bf(a.y); v[2] = f2bf(a.z); v[3] = f2bf(a.w);
                v[4] = f2bf(b.x); v[5] = f2bf(b.y); v[6] = f2bf(b.z); v[7] = f2bf(b.w);
            } else {
                v = *(const u16x8*)((const bf16_t*)in + (long)(r0 + r) * ld_in + c);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) tile[ch * 8 + e][r] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = i * 256 + threadIdx.x;
        const int c = idx >> 3, rc = idx & 7;
        if (c0 + c < cols && r0 + rc * 8 < ld_out)
            *(u16x8*)(out + (long)(c0 + c) * ld_out + r0 + rc * 8) = *(const u16x8*)&tile[c][rc * 8];
    }
}

// mel [B, C, T] f32 -> rows [B, T+2, Cp] bf16 with zero rows at t=0 and t=T+1 and zero channels >= C
__global__ __launch_bounds__(256) void mel_rows_k(const float* __restrict__ mel, int B, int Cn, int T, int Cp,
                                                  bf16_t* __restrict__ out) {
    __shared__ float tile[64][65];
    const int b = blockIdx.z, t0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int c = c0 + i, t = t0 + tx;
        tile[i][tx] = (c < Cn && t < T) ? mel[((long)b * Cn + c) * T + t] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int t = t0 + i, c = c0 + tx;
        if (t < T && c < Cp) out[((long)b * (T + 2) + t + 1) * Cp + c] = f2bf(tile[tx][i]);
    }
}

__global__ __launch_bounds__(256) void dropout_bf16_k(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int rows, int cols,
                                                      long ld, unsigned thresh, float scale, unsigned slo, unsigned shi) {
    const long n4 = (long)rows * (cols / 4);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const long r = i / (cols / 4);
        const int c = (int)(i % (cols / 4)) * 4;
        const u16x4 v = *(const u16x4*)(x + r * ld + c);
        u16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            o[e] = desta_keep(slo, shi, (unsigned long)(r * cols + c + e), thresh) ? f2bf(bf2f(v[e]) * scale) : (bf16_t)0;
        *(u16x4*)(y + r * ld + c) = o;
    }
}
__global__ __launch_bounds__(256) void dropout_mask_k(unsigned slo, unsigned shi, long n, unsigned thresh, uint8_t* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        out[i] = desta_keep(slo, shi, (unsigned long)i, thresh) ? 1 : 0;
}

// greedy decoding: out[r] = argmax_c x[r][c] (first maximum, like torch.argmax).  Keys order by value, then by
// SMALLER index: (monotone float bits << 32) | ~index.  Stage 1: ARGMAX_SPLIT blocks per row reduce a column slice
// each to one key in the workspace; stage 2: one wave per row reduces the slice keys.
constexpr int ARGMAX_SPLIT = 64;
__device__ __forceinline__ unsigned long argmax_key(float v, int idx) {
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;                                       // -0 maps onto +0 (they compare equal in torch)
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);                     // monotone map of float order onto unsigned
    return ((unsigned long)b << 32) | (unsigned)(~(unsigned)idx);
}
__global__ __launch_bounds__(256) void argmax_part_k(const bf16_t* __restrict__ x, long ld, int cols, unsigned long* __restrict__ ws) {
    __shared__ unsigned long red[4];
    const bf16_t* row = x + (long)blockIdx.y * ld;
    const int per = (cols + ARGMAX_SPLIT - 1) / ARGMAX_SPLIT;
    const int c0 = blockIdx.x * per, c1 = min(cols, c0 + per);
    unsigned long best = 0;                                              // below every real key (NaN-free logits)
    for (int c = c0 + threadIdx.x; c < c1; c += 256) {
        const unsigned long k = argmax_key(bf2f(row[c]), c);
        best = k > best ? k : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long ok = __shfl_xor(best, o, 64);
        best = ok > best ? ok : best;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = red[w] > best ? red[w] : best;
        ws[(long)blockIdx.y * ARGMAX_SPLIT + blockIdx.x] = best;
    }
}
__global__ __launch_bounds__(64) void argmax_final_k(const unsigned long* __restrict__ ws, long* __restrict__ out) {
    unsigned long best = ws[(long)blockIdx.x * ARGMAX_SPLIT + threadIdx.x];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long ok = __shfl_xor(best, o, 64);
        best = ok > best ? ok : best;
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (long)(unsigned)(~(unsigned)(best & 0xffffffffu));
}

// ------------------------------------------------------------------------------------ temperature + top-p sampling
// One 1024-thread block per row.  p_j = softmax(logit_j / T).  TopPLogitsWarper keeps token i iff the mass of all
// tokens that are not more probable than i exceeds 1 - top_p (ascending cumulative sum, TF:generation/logits_process.py);
// logits are bf16, so "not more probable" is a comparison of 16-bit keys and the boundary is found by a 16-step binary
// search over the key space (each step one pass over the row: L2-resident, 256 KiB for a 128k vocabulary).  Tokens that
// TIE with the boundary logit are all kept (torch.sort leaves their order unspecified).  The sample is drawn by
// inverting the prefix sum of the kept masses in index order with one counter-based uniform per (seed, step, row).
// A -inf logit (desta_mask_tokens_bf16) is never kept; a row without a finite logit keeps nothing and yields token 0.
__device__ __forceinline__ unsigned bf16_key(bf16_t b) {
    if (b == 0x8000u) b = 0u;                                      // -0 maps onto +0: one key for equal logits
    return (b & 0x8000u) ? (unsigned)(~b & 0xffffu) : (unsigned)(b | 0x8000u);
}
constexpr unsigned BF16_KEY_NINF = 0x007fu;                        // bf16_key(-inf): a suppressed token, never kept (mass 0)
__device__ __forceinline__ float block_sum_1024(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += red[i];
    return t;
}
__global__ __launch_bounds__(1024) void sample_top_p_k(const bf16_t* __restrict__ x, long ld, int cols, float inv_temp, float top_p,
                                                       unsigned seed_lo, unsigned seed_hi, unsigned step, int width, long* __restrict__ out,
                                                       unsigned char* __restrict__ keep_mask) {
    __shared__ float red[16];
    __shared__ float part[1024];
    __shared__ int pick;
    const bf16_t* row = x + (long)blockIdx.x * ld;
    const int tid = threadIdx.x;
    float mx = -INFINITY;
    for (int c = tid; c < cols; c += 1024) mx = fmaxf(mx, bf2f(row[c]));
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, red[i]);
    float z = 0.f;
    for (int c = tid; c < cols; c += 1024) z += __expf((bf2f(row[c]) - mx) * inv_temp);
    z = block_sum_1024(z, red);
    unsigned kstar = 0;                                            // keep every token (top_p >= 1)
    if (top_p < 1.0f) {
        const float cut = (1.0f - top_p) * z;
        unsigned lo = 0, hi = 65535;                               // smallest key k with F(k) = sum_{key_j <= k} e_j > cut
        while (lo < hi) {
            const unsigned mid = (lo + hi) >> 1;
            float f = 0.f;
            for (int c = tid; c < cols; c += 1024) {
                const bf16_t b = row[c];
                if (bf16_key(b) <= mid) f += __expf((bf2f(b) - mx) * inv_temp);
            }
            f = block_sum_1024(f, red);
            if (f > cut) hi = mid; else lo = mid + 1;
        }
        kstar = lo;
    }
    // kept mass per thread over a CONTIGUOUS index chunk (so the prefix sum runs in index order)
    const int chunk = (cols + 1023) / 1024, c0 = tid * chunk, c1 = min(cols, c0 + chunk);
    float mine = 0.f;
    for (int c = c0; c < c1; ++c) {
        const bf16_t b = row[c];
        const bool keep = bf16_key(b) >= kstar && bf16_key(b) != BF16_KEY_NINF;
        if (keep) mine += __expf((bf2f(b) - mx) * inv_temp);
        if (keep_mask) keep_mask[(long)blockIdx.x * cols + c] = keep ? 1 : 0;
    }
    part[tid] = mine;
    if (tid == 0) pick = -1;
    __syncthreads();
    if (tid == 0) {                                                // 1024-entry serial scan by one lane: ~2 us, fixed order
        float tot = 0.f;
        for (int i = 0; i < 1024; ++i) tot += part[i];
        // row r = blockIdx.x is row j = r % width of sequence b = r / width (width 1, the one-row entry point: b = r, j = 0): the
        // draw of emitted position step + j (a uint32 sum: it wraps) of sequence b, so the counter row is b, not r.  One lane
        // divides, once; a (batch, width) grid without the division cost the row loops above 2.4 % (MI355X, 8 and 64 rows)
        const unsigned b = blockIdx.x / (unsigned)width, j = blockIdx.x - b * (unsigned)width;
        const unsigned u = desta_rng32(seed_lo, seed_hi, ((unsigned long)(step + j) << 32) | b);
        const float target = (float)(u >> 8) * (1.0f / 16777216.0f) * tot;
        float run = 0.f;
        int t = 0;
        for (; t < 1023; ++t) {
            if (run + part[t] > target) break;
            run += part[t];
        }
        // skip empty tails (rounding may leave target == tot): walk back to the last thread that holds mass
        while (t > 0 && part[t] == 0.f) --t;
        pick = t;
        red[0] = target - run;
    }
    __syncthreads();
    if (tid == pick) {
        float rem = red[0], run = 0.f;
        int tok = -1, last = -1;
        for (int c = c0; c < c1; ++c) {
            const bf16_t b = row[c];
            if (bf16_key(b) >= kstar && bf16_key(b) != BF16_KEY_NINF) {
                last = c;
                run += __expf((bf2f(b) - mx) * inv_temp);
                if (run > rem) { tok = c; break; }
            }
        }
        out[blockIdx.x] = tok >= 0 ? tok : (last >= 0 ? last : 0);   // nothing kept in the chunk (no finite logit in the row): token 0
    }
}

int nblocks(long n, int per = 256, int cap = 8192) {
    long b = (n + per - 1) / per;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

#define LN_DISPATCH(KERNEL, cols, ...)                                                         \
    do {                                                                                       \
        if ((cols) <= 512) hipLaunchKernelGGL((KERNEL<1>), __VA_ARGS__);                       \
        else if ((cols) <= 1024) hipLaunchKernelGGL((KERNEL<2>), __VA_ARGS__);                 \
        else if ((cols) <= 2048) hipLaunchKernelGGL((KERNEL<4>), __VA_ARGS__);                 \
        else if ((cols) <= 4096) hipLaunchKernelGGL((KERNEL<8>), __VA_ARGS__);                 \
        else hipLaunchKernelGGL((KERNEL<16>), __VA_ARGS__);                                    \
    } while (0)

extern "C" int desta_layernorm_fwd(const void* x, int x_f32, const float* gamma, const float* beta, float eps, int rows,
                                   int cols, void* y_bf16, float* y_f32, float* stats, void* stream) {
    DESTA_CHECK_ARG(x && gamma && beta && (y_bf16 || y_f32), "layernorm_fwd: null argument");
    DESTA_CHECK_ARG(rows > 0 && cols > 0 && cols % 8 == 0 && cols <= 8192, "layernorm_fwd: cols=%d must be a multiple of 8, <= 8192", cols);
    dim3 grid((rows + RPB - 1) / RPB);
    LN_DISPATCH(layernorm_fwd_k, cols, grid, dim3(256), 0, (hipStream_t)stream, x, x_f32, gamma, beta, eps, rows, cols,
                (bf16_t*)y_bf16, y_f32, stats);
    DESTA_CHECK_LAUNCH("layernorm_fwd");
    return DESTA_OK;
}

extern "C" size_t desta_layernorm_bwd_workspace_floats(int rows, int cols) {
    int nb = (rows + RPB - 1) / RPB;
    if (nb > 512) nb = 512;                                    // two blocks per CU (128 left half the chip idle: 19.5 us per call, 0.15 of the HBM rate)
    return (size_t)nb * 2 * cols;
}

extern "C" int desta_layernorm_bwd(const void* dy, int dy_f32, const void* x, int x_f32, const float* gamma,
                                   const float* stats, int rows, int cols, float* dx_f32, void* dx_bf16, float* dgamma,
                                   float* dbeta, int accumulate, float* workspace, void* stream) {
    DESTA_CHECK_ARG(dy && x && gamma && stats && (dx_f32 || dx_bf16), "layernorm_bwd: null argument");
    DESTA_CHECK_ARG(rows > 0 && cols % 8 == 0 && cols <= 4096, "layernorm_bwd: cols=%d must be a multiple of 8, <= 4096", cols);
    DESTA_CHECK_ARG(!dgamma || (dbeta && workspace), "layernorm_bwd: dgamma needs dbeta and workspace");
    int nb = (rows + RPB - 1) / RPB;
    if (nb > 512) nb = 512;                                    // two blocks per CU (128 left half the chip idle: 19.5 us per call, 0.15 of the HBM rate)
    float* part = dgamma ? workspace : nullptr;
    if (cols <= 512) hipLaunchKernelGGL((layernorm_bwd_k<1>), dim3(nb), dim3(256), 0, (hipStream_t)stream, dy, dy_f32, x, x_f32, gamma, stats, rows, cols, dx_f32, (bf16_t*)dx_bf16, part);
    else if (cols <= 1024) hipLaunchKernelGGL((layernorm_bwd_k<2>), dim3(nb), dim3(256), 0, (hipStream_t)stream, dy, dy_f32, x, x_f32, gamma, stats, rows, cols, dx_f32, (bf16_t*)dx_bf16, part);
    else if (cols <= 2048) hipLaunchKernelGGL((layernorm_bwd_k<4>), dim3(nb), dim3(256), 0, (hipStream_t)stream, dy, dy_f32, x, x_f32, gamma, stats, rows, cols, dx_f32, (bf16_t*)dx_bf16, part);
    else hipLaunchKernelGGL((layernorm_bwd_k<8>), dim3(nb), dim3(256), 0, (hipStream_t)stream, dy, dy_f32, x, x_f32, gamma, stats, rows, cols, dx_f32, (bf16_t*)dx_bf16, part);   // ORCA's LayerNorms over the LLM width (4096): 256 live floats per lane, off the hot path
    if (dgamma)
        hipLaunchKernelGGL(reduce_partials_k, dim3((2 * cols + 63) / 64), dim3(1024), 0, (hipStream_t)stream,
                           (const float*)part, nb, 2 * cols, dgamma, dbeta, cols, accumulate);
    DESTA_CHECK_LAUNCH("layernorm_bwd");
    return DESTA_OK;
}

extern "C" size_t desta_colsum_workspace_floats(int rows, int cols) { return (size_t)colsum_splits(rows, cols) * cols; }

extern "C" int desta_colsum_bf16(const void* x, int rows, int cols, int64_t ld, float* out, int accumulate,
                                 float* workspace, void* stream) {
    DESTA_CHECK_ARG(x && out && workspace, "colsum: null argument");
    DESTA_CHECK_ARG(rows > 0 && cols > 0 && cols % 4 == 0 && ld % 4 == 0, "colsum: cols/ld must be multiples of 4");
    const int nr = colsum_splits(rows, cols);
    if (cols % 8 == 0 && ld % 8 == 0 && ((uintptr_t)x % 16) == 0)
        hipLaunchKernelGGL(colsum_partial_k<8>, dim3((cols / 8 + 255) / 256, nr), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, rows, cols, (long)ld, workspace);
    else
        hipLaunchKernelGGL(colsum_partial_k<4>, dim3((cols / 4 + 255) / 256, nr), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, rows, cols, (long)ld, workspace);
    hipLaunchKernelGGL(reduce_partials_k, dim3((cols + 63) / 64), dim3(1024), 0, (hipStream_t)stream,
                       (const float*)workspace, nr, cols, out, out, cols, accumulate);
    DESTA_CHECK_LAUNCH("colsum");
    return DESTA_OK;
}

extern "C" int desta_rmsnorm_fwd(const void* x, const float* weight, float eps, int rows, int cols, void* y,
                                 float* rstd, void* stream) {
    DESTA_CHECK_ARG(x && weight && y, "rmsnorm_fwd: null argument");
    DESTA_CHECK_ARG(rows > 0 && cols % 8 == 0 && cols <= 8192, "rmsnorm_fwd: cols=%d must be a multiple of 8, <= 8192", cols);
    dim3 grid((rows + RPB - 1) / RPB);
    LN_DISPATCH(rmsnorm_fwd_k, cols, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, weight, eps, rows, cols,
                (bf16_t*)y, rstd);
    DESTA_CHECK_LAUNCH("rmsnorm_fwd");
    return DESTA_OK;
}

extern "C" int desta_rmsnorm_bwd(const void* dy, const void* x, const float* weight, const float* rstd,
                                 const void* dres, int rows, int cols, void* dx, void* stream) {
    DESTA_CHECK_ARG(dy && x && weight && rstd && dx, "rmsnorm_bwd: null argument");
    DESTA_CHECK_ARG(rows > 0 && cols % 8 == 0 && cols <= 8192, "rmsnorm_bwd: cols=%d must be a multiple of 8, <= 8192", cols);
    dim3 grid((rows + RPB - 1) / RPB);
    LN_DISPATCH(rmsnorm_bwd_k, cols, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dy, (const bf16_t*)x, weight,
                rstd, (const bf16_t*)dres, rows, cols, (bf16_t*)dx);
    DESTA_CHECK_LAUNCH("rmsnorm_bwd");
    return DESTA_OK;
}

namespace {
// RoPE + QUANTISING KV-cache append (the opt-in FP8 cache of generate()): rope_k<128, NORM, false, BIAS> with the cache written as
// OCP e4m3 bytes + one power-of-two fp32 scale per (row, slot, K-or-V head), the rule of desta_quantize_rows_e4m3 with "row"
// = one head's 128 values.  q and k are rotated in place with the bits rope_k leaves; what is quantised is the bf16 value the
// bf16 cache would hold (BIAS: after the bias, k: after the rotation).  A head is 8 adjacent lanes, so its amax is three xor
// shuffles.
struct RopeKV8 { uint8_t* dst; float* scale; long bs, rs, sbs, srs; int slot0; int n_v; };
template <int NORM, bool BIAS>
__global__ __launch_bounds__(256) void rope_kv8_k(bf16_t* __restrict__ buf, long ld, int rows, int S, int n_heads, int n_q,
                                                  const float* __restrict__ cs, const float* __restrict__ wq,
                                                  const float* __restrict__ wk, float eps, const int* __restrict__ pos_shift, RopeKV8 kv,
                                                  const float* __restrict__ bias) {
    constexpr int HD = 128, G = HD / 16, H2 = HD / 2;
    const RopeLane t = rope_lane<HD>(rows, n_heads, kv.n_v);
    const int j = t.j, row = t.row, head = t.head;
    bf16_t* p = buf + (long)row * ld + (long)head * HD;
    u16x8 ca, cb;                                                        // the bf16 bits a bf16 cache would hold
    if (!BIAS && head >= n_heads) {                                      // bias-free V head: as stored
        ca = *(const u16x8*)(p + 8 * j);
        cb = *(const u16x8*)(p + H2 + 8 * j);
    } else {
        const int pos = rope_pos(row, S, 0, pos_shift);
        float oa[8], ob[8];
        rope_head<HD, NORM, BIAS>(p, j, !BIAS || head < n_heads, pos, cs, head < n_q ? wq : wk, eps, BIAS ? bias + (long)head * HD : nullptr, oa, ob);
#pragma unroll
        for (int e = 0; e < 8; ++e) { ca[e] = f2bf(oa[e]); cb[e] = f2bf(ob[e]); }
        if (t.active) { *(u16x8*)(p + 8 * j) = ca; *(u16x8*)(p + H2 + 8 * j) = cb; }
    }
    unsigned amax = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) amax = max(amax, max((unsigned)(ca[e] & 0x7fff), (unsigned)(cb[e] & 0x7fff)));
#pragma unroll
    for (int o = 1; o < G; o <<= 1) amax = max(amax, (unsigned)__shfl_xor((int)amax, o, 64));
    if (!t.active || head < n_q) return;
    const int ex = amax ? e4m3_row_exponent(amax) : 0;
    uint8_t* d = rope_slot<HD>(kv.dst, kv.bs, kv.rs, kv.slot0, row, S, head, n_q);
    unsigned w[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const u16x8& v = h ? cb : ca;
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = ldexpf(bf2f(v[e]), -ex);
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
        w[2 * h] = (unsigned)lo; w[2 * h + 1] = (unsigned)hi;
    }
    *(uint2*)(d + 8 * j) = make_uint2(w[0], w[1]);
    *(uint2*)(d + H2 + 8 * j) = make_uint2(w[2], w[3]);
    if (j == 0) *rope_slot<1>(kv.scale, kv.sbs, kv.srs, kv.slot0, row, S, head, n_q) = pow2f(ex);
}

// One call of any of the six rotary entry points: the arguments all of them take, then what only some do.
struct RopeCall {
    void* buf; int64_t ld; int rows, seq, n_q, n_kv, hd;
    const float *cos_sin, *wq, *wk; float eps;
    const int32_t* pos_shift; void* stream;
    const void* pre = nullptr; int64_t ld_pre = 0; int backward = 0, sm_batch = 0;       // desta_rope, desta_rope_bias
    bool has_bias = false; const float* bias = nullptr;                                  // the _bias forms
    bool has_cache = false; void* cache = nullptr; int64_t kbs = 0, krs = 0; int slot0 = 0;    // the _kv_append forms
    bool e4m3 = false; float* scale = nullptr; int64_t sbs = 0, srs = 0;                 // the _e4m3 forms
};
}  // namespace

// The one argument check: every condition is a fact about memory the kernels touch (or a combination no kernel exists for), so
// a form is held to it exactly when its kernel makes that access.  A cache or a bias makes the grid cover the V heads.
static int rope_check(const char* who, const RopeCall& c) {
    const bool covers_v = c.has_cache || c.has_bias;
    DESTA_CHECK_ARG(c.buf && c.cos_sin && (!c.has_bias || c.bias), "%s: null argument", who);
    DESTA_CHECK_ARG(!c.has_bias || (!c.wq && !c.wk), "%s: a q|k|v bias together with q/k-norm weights is not supported", who);
    DESTA_CHECK_ARG(c.hd == 128 || (c.hd == 64 && !c.e4m3), "%s: head_dim %d unsupported (%s)", who, c.hd, c.e4m3 ? "128" : "64 or 128");
    DESTA_CHECK_ARG(!c.wq == !c.wk, "%s: q_norm and k_norm come together", who);
    DESTA_CHECK_ARG(!(c.wq && c.backward) || c.pre, "%s: backward with q/k norm needs the saved pre-norm q/k", who);
    DESTA_CHECK_ARG(c.sm_batch >= 0 && (c.sm_batch == 0 || c.rows % c.sm_batch == 0), "%s: rows must be a multiple of s_major_batch", who);
    DESTA_CHECK_ARG(c.rows > 0 && c.seq > 0 && (!covers_v || (c.n_q > 0 && c.n_kv > 0)), "%s: bad shape", who);
    DESTA_CHECK_ARG(c.ld % 8 == 0 && (!covers_v || c.ld >= (int64_t)(c.n_q + 2 * c.n_kv) * c.hd),
                    "%s: ld %lld is not a multiple of 8%s", who, (long long)c.ld, covers_v ? " that holds q|k|v" : "");
    if (c.has_cache) {                                                   // slot (row / seq, slot0 + row % seq) of a batch-major grid
        DESTA_CHECK_ARG(c.rows % c.seq == 0, "%s: rows must be a multiple of seq", who);
        DESTA_CHECK_ARG(c.cache && c.krs % 8 == 0 && c.kbs % 8 == 0 && c.slot0 >= 0 && c.krs >= 2L * c.n_kv * c.hd && c.kbs >= 0 &&
                        (!c.e4m3 || (c.scale && c.srs >= 2L * c.n_kv && c.sbs >= 0)), "%s: bad cache argument", who);
    }
    DESTA_CHECK_ARG((uintptr_t)c.buf % 16 == 0 && (uintptr_t)c.cos_sin % 16 == 0 && (uintptr_t)c.bias % 16 == 0 && (uintptr_t)c.cache % 16 == 0 &&
                    (uintptr_t)c.scale % 4 == 0, "%s: buffers must be 16-byte aligned", who);
    return DESTA_OK;
}

static int rope_launch(const char* who, const RopeCall& c) {             // rope_k: in place, or into the bf16 cache
    const RopeKV kv = {(bf16_t*)c.cache, (long)c.kbs, (long)c.krs, c.slot0, c.has_cache || c.has_bias ? c.n_kv : 0};
    const int nh = c.n_q + c.n_kv;
    const long nthreads = (long)c.rows * (nh + kv.n_v) * (c.hd / 16);
    const dim3 grid((unsigned)((nthreads + 255) / 256));
#define ROPE_GO(HD, NORM, BWD, BIAS)                                                                                                         \
    hipLaunchKernelGGL((rope_k<HD, NORM, BWD, BIAS>), grid, dim3(256), 0, (hipStream_t)c.stream, (bf16_t*)c.buf, (long)c.ld, c.rows, c.seq, nh, \
                       c.n_q, c.cos_sin, c.wq, c.wk, c.eps, (const bf16_t*)c.pre, (long)c.ld_pre, c.pos_shift, kv, c.sm_batch, c.bias)
#define ROPE_HD(NORM, BWD, BIAS) do { if (c.hd == 128) ROPE_GO(128, NORM, BWD, BIAS); else ROPE_GO(64, NORM, BWD, BIAS); } while (0)
    if (c.has_bias) ROPE_HD(0, false, true);
    else if (!c.backward) { if (c.wq) ROPE_HD(1, false, false); else ROPE_HD(0, false, false); }
    else { if (c.wq) ROPE_HD(2, true, false); else ROPE_HD(0, true, false); }
#undef ROPE_HD
#undef ROPE_GO
    DESTA_CHECK_LAUNCH(who);
    return DESTA_OK;
}

static int rope_kv8_launch(const char* who, const RopeCall& c) {         // rope_kv8_k: into the FP8 cache
    const RopeKV8 kv = {(uint8_t*)c.cache, c.scale, (long)c.kbs, (long)c.krs, (long)c.sbs, (long)c.srs, c.slot0, c.n_kv};
    const int nh = c.n_q + c.n_kv;
    const long nthreads = (long)c.rows * (nh + c.n_kv) * 8;
    const dim3 grid((unsigned)((nthreads + 255) / 256));
#define ROPE8_GO(NORM, BIAS)                                                                                                            \
    hipLaunchKernelGGL((rope_kv8_k<NORM, BIAS>), grid, dim3(256), 0, (hipStream_t)c.stream, (bf16_t*)c.buf, (long)c.ld, c.rows, c.seq, nh, \
                       c.n_q, c.cos_sin, c.wq, c.wk, c.eps, c.pos_shift, kv, c.bias)
    if (c.has_bias) ROPE8_GO(0, true);
    else if (c.wq) ROPE8_GO(1, false);
    else ROPE8_GO(0, false);
#undef ROPE8_GO
    DESTA_CHECK_LAUNCH(who);
    return DESTA_OK;
}

static int rope_run(const char* who, const RopeCall& c) {
    const int rc = rope_check(who, c);
    return rc != DESTA_OK ? rc : c.e4m3 ? rope_kv8_launch(who, c) : rope_launch(who, c);
}

// The six exports (include/desta_hip.h): each fills a RopeCall.  The _bias forms take qkv_bias where the plain ones take eps.
#define ROPE_COMMON(EPS) {buf, ld, rows, seq, n_q_heads, n_kv_heads, head_dim, cos_sin, q_norm_w, k_norm_w, EPS, pos_shift, stream}
extern "C" int desta_rope(void* buf, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                          const float* cos_sin, const float* q_norm_w, const float* k_norm_w, float eps,
                          const void* pre_norm, int64_t ld_pre, int backward, const int32_t* pos_shift, int s_major_batch,
                          void* stream) {
    RopeCall c = ROPE_COMMON(eps);
    c.pre = pre_norm; c.ld_pre = ld_pre; c.backward = backward; c.sm_batch = s_major_batch;
    return rope_run("rope", c);
}
extern "C" int desta_rope_bias(void* buf, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                               const float* cos_sin, const float* q_norm_w, const float* k_norm_w, const float* qkv_bias,
                               const int32_t* pos_shift, int s_major_batch, void* stream) {
    RopeCall c = ROPE_COMMON(0.f);
    c.sm_batch = s_major_batch; c.has_bias = true; c.bias = qkv_bias;
    return rope_run("rope_bias", c);
}
extern "C" int desta_rope_kv_append(void* buf, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                                    const float* cos_sin, const float* q_norm_w, const float* k_norm_w, float eps,
                                    const int32_t* pos_shift, void* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride,
                                    int slot0, void* stream) {
    RopeCall c = ROPE_COMMON(eps);
    c.has_cache = true; c.cache = kv_cache; c.kbs = kv_batch_stride; c.krs = kv_row_stride; c.slot0 = slot0;
    return rope_run("rope_kv_append", c);
}
extern "C" int desta_rope_kv_append_bias(void* buf, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                                         const float* cos_sin, const float* q_norm_w, const float* k_norm_w, const float* qkv_bias,
                                         const int32_t* pos_shift, void* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride,
                                         int slot0, void* stream) {
    RopeCall c = ROPE_COMMON(0.f);
    c.has_cache = true; c.cache = kv_cache; c.kbs = kv_batch_stride; c.krs = kv_row_stride; c.slot0 = slot0;
    c.has_bias = true; c.bias = qkv_bias;
    return rope_run("rope_kv_append_bias", c);
}
extern "C" int desta_rope_kv_append_e4m3(void* buf, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                                         const float* cos_sin, const float* q_norm_w, const float* k_norm_w, float eps,
                                         const int32_t* pos_shift, uint8_t* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride,
                                         float* kv_scale, int64_t scale_batch_stride, int64_t scale_row_stride, int slot0, void* stream) {
    RopeCall c = ROPE_COMMON(eps);
    c.has_cache = true; c.cache = kv_cache; c.kbs = kv_batch_stride; c.krs = kv_row_stride; c.slot0 = slot0;
    c.e4m3 = true; c.scale = kv_scale; c.sbs = scale_batch_stride; c.srs = scale_row_stride;
    return rope_run("rope_kv_append_e4m3", c);
}
extern "C" int desta_rope_kv_append_e4m3_bias(void* buf, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                                              const float* cos_sin, const float* q_norm_w, const float* k_norm_w, const float* qkv_bias,
                                              const int32_t* pos_shift, uint8_t* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride,
                                              float* kv_scale, int64_t scale_batch_stride, int64_t scale_row_stride, int slot0, void* stream) {
    RopeCall c = ROPE_COMMON(0.f);
    c.has_cache = true; c.cache = kv_cache; c.kbs = kv_batch_stride; c.krs = kv_row_stride; c.slot0 = slot0;
    c.e4m3 = true; c.scale = kv_scale; c.sbs = scale_batch_stride; c.srs = scale_row_stride;
    c.has_bias = true; c.bias = qkv_bias;
    return rope_run("rope_kv_append_e4m3_bias", c);
}
#undef ROPE_COMMON

extern "C" int desta_swiglu_fwd(const void* gate_up, void* act, int64_t rows, int inter, void* stream) {
    DESTA_CHECK_ARG(gate_up && act && rows > 0 && inter % 8 == 0, "swiglu_fwd: bad argument");
    hipLaunchKernelGGL(swiglu_fwd_k, dim3(nblocks(rows * (inter / 8))), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)gate_up, (bf16_t*)act, (long)rows, inter);
    DESTA_CHECK_LAUNCH("swiglu_fwd");
    return DESTA_OK;
}
extern "C" int desta_swiglu_bwd(const void* gate_up, const void* dact, void* dgate_up, int64_t rows, int inter, void* stream) {
    DESTA_CHECK_ARG(gate_up && dact && dgate_up && rows > 0 && inter % 8 == 0, "swiglu_bwd: bad argument");
    hipLaunchKernelGGL(swiglu_bwd_k, dim3(nblocks(rows * (inter / 8))), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)gate_up, (const bf16_t*)dact, (bf16_t*)dgate_up, (long)rows, inter);
    DESTA_CHECK_LAUNCH("swiglu_bwd");
    return DESTA_OK;
}
extern "C" int desta_gelu_bwd(const void* preact, const void* dact, void* dpre, int64_t n, void* stream) {
    DESTA_CHECK_ARG(preact && dact && dpre && n > 0 && n % 8 == 0, "gelu_bwd: n must be a positive multiple of 8");
    hipLaunchKernelGGL(gelu_bwd_k, dim3(nblocks(n / 8)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)preact,
                       (const bf16_t*)dact, (bf16_t*)dpre, (long)(n / 8));
    DESTA_CHECK_LAUNCH("gelu_bwd");
    return DESTA_OK;
}
extern "C" int desta_cast_f32_bf16(const float* x, void* y, int64_t n, void* stream) {
    DESTA_CHECK_ARG(x && y && n > 0 && n % 8 == 0, "cast: n must be a positive multiple of 8");
    hipLaunchKernelGGL(cast_f32_bf16_k, dim3(nblocks(n / 8)), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)y, (long)(n / 8));
    DESTA_CHECK_LAUNCH("cast_f32_bf16");
    return DESTA_OK;
}
extern "C" int desta_add_f32(float* y, const float* x, int64_t n, void* stream) {
    DESTA_CHECK_ARG(x && y && n > 0 && n % 4 == 0, "add_f32: n must be a positive multiple of 4");
    hipLaunchKernelGGL(add_f32_k, dim3(nblocks(n / 4)), dim3(256), 0, (hipStream_t)stream, y, x, (long)(n / 4));
    DESTA_CHECK_LAUNCH("add_f32");
    return DESTA_OK;
}
extern "C" int desta_transpose_to_bf16(const void* in, int in_f32, int64_t ld_in, int rows, int cols, void* out,
                                       int64_t ld_out, void* stream) {
    DESTA_CHECK_ARG(in && out && rows > 0 && cols > 0 && ld_out >= rows, "transpose: bad argument");
    dim3 grid((cols + 63) / 64, (unsigned)((ld_out + 63) / 64));
    const bool vec = cols % 8 == 0 && ld_in % 8 == 0 && ld_out % 8 == 0 && ((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0;
    if (vec && in_f32) hipLaunchKernelGGL((transpose_vec_k<true>), grid, dim3(256), 0, (hipStream_t)stream, in, (long)ld_in, rows, cols, (bf16_t*)out, (long)ld_out);
    else if (vec) hipLaunchKernelGGL((transpose_vec_k<false>), grid, dim3(256), 0, (hipStream_t)stream, in, (long)ld_in, rows, cols, (bf16_t*)out, (long)ld_out);
    else if (in_f32) hipLaunchKernelGGL((transpose_k<true>), grid, dim3(256), 0, (hipStream_t)stream, in, (long)ld_in, rows, cols, (bf16_t*)out, (long)ld_out);
    else hipLaunchKernelGGL((transpose_k<false>), grid, dim3(256), 0, (hipStream_t)stream, in, (long)ld_in, rows, cols, (bf16_t*)out, (long)ld_out);
    DESTA_CHECK_LAUNCH("transpose");
    return DESTA_OK;
}
extern "C" int desta_mel_to_rows(const float* mel, int batch, int n_mels, int frames, int c_pad, void* out, void* stream) {
    DESTA_CHECK_ARG(mel && out && batch > 0 && n_mels > 0 && frames > 0 && c_pad >= n_mels, "mel_to_rows: bad argument");
    dim3 grid((frames + 63) / 64, (c_pad + 63) / 64, batch);
    hipLaunchKernelGGL(mel_rows_k, grid, dim3(256), 0, (hipStream_t)stream, mel, batch, n_mels, frames, c_pad, (bf16_t*)out);
    DESTA_CHECK_LAUNCH("mel_to_rows");
    return DESTA_OK;
}

extern "C" int desta_dropout_bf16(const void* x, void* y, int rows, int cols, int64_t ld, float p, uint64_t seed, void* stream) {
    DESTA_CHECK_ARG(x && y && rows > 0 && cols > 0 && cols % 4 == 0 && ld % 4 == 0 && p >= 0.f && p < 1.f, "dropout: bad argument");
    hipLaunchKernelGGL(dropout_bf16_k, dim3(nblocks((long)rows * (cols / 4))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (bf16_t*)y, rows, cols, (long)ld, p > 0.f ? desta_drop_thresh(p) : 0u, 1.0f / (1.0f - p), (unsigned)seed,
                       (unsigned)(seed >> 32));
    DESTA_CHECK_LAUNCH("dropout_bf16");
    return DESTA_OK;
}
extern "C" int desta_dropout_mask_u8(uint64_t seed, int64_t n, float p, uint8_t* out, void* stream) {
    DESTA_CHECK_ARG(out && n > 0 && p >= 0.f && p < 1.f, "dropout_mask: bad argument");
    hipLaunchKernelGGL(dropout_mask_k, dim3(nblocks(n)), dim3(256), 0, (hipStream_t)stream, (unsigned)seed, (unsigned)(seed >> 32),
                       (long)n, p > 0.f ? desta_drop_thresh(p) : 0u, out);
    DESTA_CHECK_LAUNCH("dropout_mask");
    return DESTA_OK;
}

// logits[r, ids[i]] = -inf for every row: the SuppressTokens / SuppressTokensAtBegin logits processors of Whisper's generate
// (TF:generation/logits_process.py SuppressTokensLogitsProcessor) in front of the argmax
namespace {
__global__ __launch_bounds__(256) void mask_tokens_k(bf16_t* __restrict__ x, long ld, int rows, const int* __restrict__ ids, int n, int cols) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)rows * n) return;
    const int r = (int)(i / n), c = ids[i % n];
    if (c >= 0 && c < cols) x[(long)r * ld + c] = (bf16_t)0xff80;      // bf16 -inf
}
}  // namespace
extern "C" int desta_mask_tokens_bf16(void* logits, int64_t ld, int rows, int cols, const int32_t* ids, int n, void* stream) {
    DESTA_CHECK_ARG(logits && ids && rows > 0 && n > 0 && cols > 0 && ld >= cols, "mask_tokens: bad argument");
    hipLaunchKernelGGL(mask_tokens_k, dim3((unsigned)(((long)rows * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)logits, (long)ld, rows, ids, n, cols);
    DESTA_CHECK_LAUNCH("mask_tokens");
    return DESTA_OK;
}

extern "C" size_t desta_argmax_workspace_bytes(int rows) { return (size_t)(rows > 0 ? rows : 0) * ARGMAX_SPLIT * sizeof(unsigned long); }
extern "C" int desta_argmax_bf16(const void* x, int64_t ld, int rows, int cols, int64_t* out, void* workspace, void* stream) {
    DESTA_CHECK_ARG(x && out && workspace && rows > 0 && cols > 0, "argmax: bad argument");
    static_assert(ARGMAX_SPLIT == 64, "final stage is one 64-lane wave");
    hipLaunchKernelGGL(argmax_part_k, dim3(ARGMAX_SPLIT, rows), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (long)ld, cols,
                       (unsigned long*)workspace);
    hipLaunchKernelGGL(argmax_final_k, dim3(rows), dim3(64), 0, (hipStream_t)stream, (const unsigned long*)workspace, (long*)out);
    DESTA_CHECK_LAUNCH("argmax_bf16");
    return DESTA_OK;
}

static int sample_top_p_launch(const void* logits, int64_t ld, int batch, int width, int cols, float temperature, float top_p, uint64_t seed,
                               uint32_t step0, int64_t* out, uint8_t* keep_mask, void* stream) {
    DESTA_CHECK_ARG(logits && out && batch > 0 && cols > 0, "sample_top_p: bad argument");
    DESTA_CHECK_ARG(width >= 1 && width <= 8, "sample_top_p: width %d out of range (1..8)", width);
    DESTA_CHECK_ARG(temperature > 0.f && top_p > 0.f && top_p <= 1.f, "sample_top_p: need temperature > 0 and 0 < top_p <= 1");
    hipLaunchKernelGGL(sample_top_p_k, dim3(batch * width), dim3(1024), 0, (hipStream_t)stream, (const bf16_t*)logits, (long)ld, cols,
                       1.0f / temperature, top_p, (unsigned)seed, (unsigned)(seed >> 32), step0, width, (long*)out, keep_mask);
    DESTA_CHECK_LAUNCH("sample_top_p");
    return DESTA_OK;
}

extern "C" int desta_sample_top_p_bf16(const void* logits, int64_t ld, int rows, int cols, float temperature, float top_p,
                                       uint64_t seed, uint32_t step, int64_t* out, uint8_t* keep_mask, void* stream) {
    return sample_top_p_launch(logits, ld, rows, 1, cols, temperature, top_p, seed, step, out, keep_mask, stream);
}

extern "C" int desta_sample_top_p_rows_bf16(const void* logits, int64_t ld, int batch, int width, int cols, float temperature, float top_p,
                                            uint64_t seed, uint32_t step0, int64_t* out, uint8_t* keep_mask, void* stream) {
    return sample_top_p_launch(logits, ld, batch, width, cols, temperature, top_p, seed, step0, out, keep_mask, stream);
}
