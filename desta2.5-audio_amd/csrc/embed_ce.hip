// Embedding gather + audio splice, fused shifted cross-entropy (forward + dlogits), and the
// connector's tap mix — the glue ops of DeSTA25AudioModel around the three transformer stacks (gfx950).
//   embed/splice ... modeling_desta25.py:1009-1041 (`embed_tokens(input_ids)` then the slice-assign of
//                    cat(audio_features, transcription_embeddings) at each start position)
//   CE ............. TF:loss/loss_utils.py:49-71 (`ForCausalLMLoss`: fp32 upcast of the bf16 logits,
//                    labels shifted left by one, mean over labels != -100) and its autograd backward
//   token logprobs . the same fp32 log-softmax, kept per target row and with the logits left intact (scoring: ranking answer
//                    options by log-likelihood); compact_labels + 1 of desta_target_rows is its label vector (row i predicts it)
//   tap mix ........ modeling_desta25.py:600-604 (softmax(layer_weights) weighted sum over the 4 taps)
#include "common.h"
#include "desta_hip.h"

namespace {

// out[r] = src[r] >= 0 ? table[src[r]] : audio[-(src[r]+1)]     (rows of h bf16, h % 8 == 0)
__global__ __launch_bounds__(256) void embed_gather_k(const bf16_t* __restrict__ table, const bf16_t* __restrict__ audio,
                                                      const int* __restrict__ src, int rows, int h,
                                                      bf16_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int s = src[row];
    const bf16_t* in = s >= 0 ? table + (long)s * h : audio + (long)(-(s + 1)) * h;
    for (int c = lane * 8; c < h; c += 512) *(u16x8*)(out + (long)row * h + c) = *(const u16x8*)(in + c);
}

__global__ __launch_bounds__(256) void gather_rows_k(const bf16_t* __restrict__ in, const int* __restrict__ idx, int rows,
                                                     int h, bf16_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const bf16_t* src = in + (long)idx[row] * h;
    for (int c = lane * 8; c < h; c += 512) *(u16x8*)(out + (long)row * h + c) = *(const u16x8*)(src + c);
}

// out[idx[i]] = in[i]: rows of a compact [rows, h] matrix back into their places (the inverse of gather_rows)
__global__ __launch_bounds__(256) void scatter_rows_k(const bf16_t* __restrict__ in, const int* __restrict__ idx, int rows,
                                                      int h, bf16_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    bf16_t* dst = out + (long)idx[row] * h;
    for (int c = lane * 8; c < h; c += 512) *(u16x8*)(dst + c) = *(const u16x8*)(in + (long)row * h + c);
}

// Rows of the [B*S] token grid whose SHIFTED label is a real target (ForCausalLMLoss: row (b,s) predicts labels[b,s+1]):
// idx[0..n) = those rows in order, lab[0] = -100, lab[1 + i] = target of compact row i, lab[1 + n] = -100, count = n.
// One block; fixed-order scan (deterministic).  lab is laid out so that `desta_causal_lm_loss(batch = 1, seq = n + 1)`
// on a compact [n + 1, V] logits buffer reproduces the full-grid loss and gradients of exactly these rows.
__global__ __launch_bounds__(1024) void target_rows_k(const long* __restrict__ labels, int B, int S, int* __restrict__ idx,
                                                      long* __restrict__ lab, int* __restrict__ count, int s_major) {
    __shared__ int part[1024];
    const int M = B * S, tid = threadIdx.x;
    const int per = (M + 1023) / 1024, m0 = tid * per, m1 = min(M, m0 + per);
    __shared__ int first[1024];
    int n = 0, f = S;                                           // f: first POSITION (m % S) among this thread's target rows
    for (int m = m0; m < m1; ++m)
        if ((m % S) + 1 < S && labels[m + 1] != -100) { ++n; f = min(f, m % S); }
    part[tid] = n;
    first[tid] = f;
    __syncthreads();
    if (tid == 0) {
        int run = 0, fmin = S;
        for (int i = 0; i < 1024; ++i) { const int v = part[i]; part[i] = run; run += v; fmin = min(fmin, first[i]); }
        count[0] = run;
        count[1] = fmin;                                        // rows of positions < fmin carry no target in any sequence
        lab[0] = -100;
        lab[1 + run] = -100;
    }
    __syncthreads();
    int pos = part[tid];
    for (int m = m0; m < m1; ++m)
        if ((m % S) + 1 < S && labels[m + 1] != -100) {
            idx[pos] = s_major ? (m % S) * B + m / S : m;          // row id in the position-major / batch-major token grid
            lab[1 + pos] = labels[m + 1];
            ++pos;
        }
}

// scal[0] = number of valid (shifted) targets, scal[1] = 1/scal[0]
__global__ __launch_bounds__(256) void ce_count_k(const long* __restrict__ labels, int B, int S, float* __restrict__ scal) {
    __shared__ float red[4];
    float n = 0.f;
    for (long i = threadIdx.x; i < (long)B * S; i += 256) {
        const int s = (int)(i % S);
        if (s + 1 < S && labels[i + 1] != -100) n += 1.f;
    }
    n = block_sum<256>(n, red);
    if (threadIdx.x == 0) { scal[0] = n; scal[1] = n > 0.f ? 1.0f / n : 0.f; }
}

// one block per row m = (b, s); logits row is overwritten with dlogits (bf16)
__global__ __launch_bounds__(256) void ce_row_k(bf16_t* __restrict__ logits, long ld, const long* __restrict__ labels,
                                                int S, int V, const float* __restrict__ scal,
                                                float* __restrict__ row_loss, int write_grad) {
    __shared__ float red[4];
    const int m = blockIdx.x, s = m % S;
    const long tgt = (s + 1 < S) ? labels[m + 1] : -100;
    bf16_t* row = logits + (long)m * ld;
    const int nv8 = V / 8;
    if (tgt == -100) {
        if (threadIdx.x == 0) row_loss[m] = 0.f;
        if (write_grad) {
            const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = threadIdx.x; i < nv8; i += 256) *(u16x8*)(row + i * 8) = z;
            for (int i = nv8 * 8 + threadIdx.x; i < V; i += 256) row[i] = 0;
        }
        return;
    }
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < nv8; i += 256) {
        const u16x8 v = *(const u16x8*)(row + i * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) mx = fmaxf(mx, bf2f(v[e]));
    }
    for (int i = nv8 * 8 + threadIdx.x; i < V; i += 256) mx = fmaxf(mx, bf2f(row[i]));
    mx = block_max<256>(mx, red);
    float sum = 0.f;
    for (int i = threadIdx.x; i < nv8; i += 256) {
        const u16x8 v = *(const u16x8*)(row + i * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += __expf(bf2f(v[e]) - mx);
    }
    for (int i = nv8 * 8 + threadIdx.x; i < V; i += 256) sum += __expf(bf2f(row[i]) - mx);
    sum = block_sum<256>(sum, red);
    const float lse = mx + __logf(sum);
    if (threadIdx.x == 0) row_loss[m] = lse - bf2f(row[tgt]);
    if (!write_grad) return;
    __syncthreads();                                   // row[tgt] has been read before anyone overwrites it
    const float inv_n = scal[1];
    for (int i = threadIdx.x; i < nv8; i += 256) {
        const u16x8 v = *(const u16x8*)(row + i * 8);
        u16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float g = __expf(bf2f(v[e]) - lse);
            if ((long)(i * 8 + e) == tgt) g -= 1.0f;
            o[e] = f2bf(g * inv_n);
        }
        *(u16x8*)(row + i * 8) = o;
    }
    for (int i = nv8 * 8 + threadIdx.x; i < V; i += 256) {
        float g = __expf(bf2f(row[i]) - lse);
        if ((long)i == tgt) g -= 1.0f;
        row[i] = f2bf(g * inv_n);
    }
}

// Same arithmetic with the WHOLE row held in registers (1024 threads x NV 16-byte chunks): the logits are read
// once and the gradient written once (2.6 GB per step at V = 128256) instead of three reads + one write — the
// 256-KiB rows of ~2000 concurrently resident blocks do not stay in L2 / the Infinity Cache between passes.
template <int NV>
__global__ __launch_bounds__(1024) void ce_row_reg_k(bf16_t* __restrict__ logits, long ld, const long* __restrict__ labels,
                                                     int S, int V, const float* __restrict__ scal,
                                                     float* __restrict__ row_loss, int write_grad) {
    __shared__ float red[16];
    const int m = blockIdx.x, s = m % S, tid = threadIdx.x;
    const long tgt = (s + 1 < S) ? labels[m + 1] : -100;
    bf16_t* row = logits + (long)m * ld;
    const int nv8 = V / 8;
    if (tgt == -100) {
        if (tid == 0) row_loss[m] = 0.f;
        if (write_grad) {
            const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int i = tid; i < nv8; i += 1024) *(u16x8*)(row + i * 8) = z;
        }
        return;
    }
    u16x8 v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int i = tid + 1024 * j;
        if (i < nv8) v[j] = *(const u16x8*)(row + i * 8);
    }
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (tid + 1024 * j < nv8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) mx = fmaxf(mx, bf2f(v[j][e]));
        }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) mx = fmaxf(mx, red[w]);
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (tid + 1024 * j < nv8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) sum += __expf(bf2f(v[j][e]) - mx);
        }
    sum = wave_sum(sum);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    sum = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) sum += red[w];
    const float lse = mx + __logf(sum);
    if (tid == 0) row_loss[m] = lse - bf2f(row[tgt]);
    if (!write_grad) return;
    __syncthreads();                                   // row[tgt] has been read before anyone overwrites it
    const float inv_n = scal[1];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int i = tid + 1024 * j;
        if (i < nv8) {
            u16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float g = __expf(bf2f(v[j][e]) - lse);
                if ((long)(i * 8 + e) == tgt) g -= 1.0f;
                o[e] = f2bf(g * inv_n);
            }
            *(u16x8*)(row + i * 8) = o;
        }
    }
}

// Token log-probabilities (scoring): logprob[r] = x[r, lab] - logsumexp(x[r, :V]) of a bf16 row, READ ONLY — the quantity
// ce_row_k folds into the mean loss before it overwrites the row with its gradient.  One 1024-thread block per row, one pass:
// every thread keeps a running (maximum m, sum s of exp(x - m)) pair, rescaled once per 16-byte chunk; pairs merge in a fixed
// order (wave butterfly, then the 16 waves in turn), so a row's result does not depend on timing.  The row is cut into the
// elements in front of the first 16-byte boundary, whole 16-byte chunks (four loads in flight per thread) and a tail, so rows
// of any alignment (ld % 8 != 0) take the vector loads.
// is_top1: the label is torch.argmax's pick (first index of the row maximum, as sample_greedy_k) iff no entry exceeds x[lab]
// (m <= x[lab]) and no entry in FRONT of it reaches x[lab] (`early`; a chunk that lies wholly in front is judged by its maximum).
constexpr int LPT = 1024;

// From here to lse_logprob the roundings are spelled out and the compiler may not fuse on its own (this file is built with
// -ffp-contract=fast-honor-pragmas for that): token_logprob_k and topk_logprob_k inline the same source and must write the same
// bits for the same row, and left free, s * e + s2 * e2 contracts around either product — two inlined copies did differ.
#pragma clang fp contract(off)

// (m, s) <- (m, s) merged with (m2, s2); -inf maxima (no finite entry yet) carry zero mass and never reach an exponent as inf - inf
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2), ms = mn == -INFINITY ? 0.f : mn;
    const float t2 = s2 * __expf(m2 - ms);
    s = __builtin_fmaf(s, __expf(m - ms), t2);
    m = mn;
}

// One thread's share of a row's (maximum m, sum s of exp(x - m)) pair and of `early` (an entry in front of `lab` reaches xl): the
// pass that token_logprob_k and topk_logprob_k share, so the two write the same bits for the same row.  EARLY = false drops the
// top-1 bookkeeping (no label).
template <bool EARLY>
__device__ __forceinline__ void lse_thread_pass(const bf16_t* __restrict__ row, int V, int lab, float xl, int tid, float& m, float& s,
                                                int& early) {
    auto one = [&](int c, bf16_t b) {
        const float x = bf2f(b);
        if (EARLY) early |= (c < lab) & (x >= xl);
        lse_merge(m, s, x, 1.0f);
    };
    auto chunk = [&](int c0, const u16x8& v) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = bf2f(v[e]);
        const float cm = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), fmaxf(fmaxf(x[4], x[5]), fmaxf(x[6], x[7])));
        if (EARLY) {
            if (c0 + 8 <= lab) early |= cm >= xl;
            else if (c0 < lab) {
#pragma unroll
                for (int e = 0; e < 8; ++e) early |= (c0 + e < lab) & (x[e] >= xl);
            }
        }
        const float mn = fmaxf(m, cm), ms = mn == -INFINITY ? 0.f : mn;
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) a += __expf(x[e] - ms);
        s = __builtin_fmaf(s, __expf(m - ms), a);
        m = mn;
    };
    const int head = min(V, (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 1));      // elements in front of the first 16-byte boundary
    const int n8 = (V - head) >> 3;
    const bf16_t* body = row + head;
    if (tid < head) one(tid, row[tid]);
    int g = tid;
    for (; g + 3 * LPT < n8; g += 4 * LPT) {
        const u16x8 v0 = *(const u16x8*)(body + (long)g * 8);
        const u16x8 v1 = *(const u16x8*)(body + (long)(g + LPT) * 8);
        const u16x8 v2 = *(const u16x8*)(body + (long)(g + 2 * LPT) * 8);
        const u16x8 v3 = *(const u16x8*)(body + (long)(g + 3 * LPT) * 8);
        chunk(head + g * 8, v0);
        chunk(head + (g + LPT) * 8, v1);
        chunk(head + (g + 2 * LPT) * 8, v2);
        chunk(head + (g + 3 * LPT) * 8, v3);
    }
    for (; g < n8; g += LPT) chunk(head + g * 8, *(const u16x8*)(body + (long)g * 8));
    for (int c = head + n8 * 8 + tid; c < V; c += LPT) one(c, row[c]);
}
// The 64 lanes' pairs merged by butterfly; lane 0 of each wave leaves its wave's pair in red_*[wave].
__device__ __forceinline__ void lse_wave_merge(float& m, float& s, int& early, int tid, float* red_m, float* red_s, int* red_e) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        lse_merge(m, s, m2, s2);
        early |= __shfl_xor(early, o, 64);
    }
    if ((tid & 63) == 0) { red_m[tid >> 6] = m; red_s[tid >> 6] = s; red_e[tid >> 6] = early; }
}
// Thread 0, after the barrier: the 16 waves' pairs in turn.
__device__ __forceinline__ void lse_block_merge(float& m, float& s, int& early, const float* red_m, const float* red_s, const int* red_e) {
    for (int w = 1; w < LPT / 64; ++w) {
        lse_merge(m, s, red_m[w], red_s[w]);
        early |= red_e[w];
    }
}
// x[lab] - m is exact in fp32 for bf16 inputs of like magnitude; a -inf entry has probability 0
__device__ __forceinline__ float lse_logprob(float x, float m, float s) { return x == -INFINITY ? -INFINITY : (x - m) - logf(s); }

#pragma clang fp contract(fast)

__global__ __launch_bounds__(LPT) void token_logprob_k(const bf16_t* __restrict__ logits, long ld, const long* __restrict__ labels,
                                                       int V, float* __restrict__ logprob, unsigned char* __restrict__ is_top1) {
    __shared__ float red_m[LPT / 64], red_s[LPT / 64];
    __shared__ int red_e[LPT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const long tgt = labels[r];
    if (tgt < 0 || tgt >= V) {                                   // ignored (-100) or out of range: nothing of the row is read
        if (tid == 0) {
            logprob[r] = 0.f;
            if (is_top1) is_top1[r] = 0;
        }
        return;
    }
    const bf16_t* row = logits + (long)r * ld;
    const int lab = (int)tgt;
    const float xl = bf2f(row[lab]);
    float m = -INFINITY, s = 0.f;
    int early = 0;
    lse_thread_pass<true>(row, V, lab, xl, tid, m, s, early);
    lse_wave_merge(m, s, early, tid, red_m, red_s, red_e);
    __syncthreads();
    if (tid == 0) {
        lse_block_merge(m, s, early, red_m, red_s, red_e);
        logprob[r] = lse_logprob(xl, m, s);
        if (is_top1) is_top1[r] = (xl >= m && !early) ? 1 : 0;
    }
}

// Per-token log-probability and the top_n alternatives of a decode step's rows (desta_topk_logprobs): READ ONLY, one 1024-thread
// block per row.  The (m, s) pair is token_logprob_k's, by the same code.  Selection is exact and by integers only, on the 16-bit
// monotone key of a bf16 value (-0.0 folded onto +0.0):
//   1. a floor t0 that at least 32 entries reach: the smallest of the 32 maxima of the block's 32-thread groups (each is a
//      different entry; a group without entries gives -inf and every entry passes);
//   2. one sweep appends every entry >= t0 to an LDS list (about a hundred on a model's row).  If more than TK_CAP reach it (ties
//      in bulk, short rows) the list is rebuilt exactly instead: two 256-bin histograms (high, then low key byte) give the n-th
//      largest key K and the count above it, a sweep takes every entry above K, and the entries equal to K are taken in index
//      order (1024-entry tiles, ballot + prefix) until n slots are filled;
//   3. each listed entry counts the entries that precede it by (key descending, index ascending) — pairs are unique, so the rank
//      does not depend on the order the atomics filled the list in — and ranks below n are written.
constexpr int TK_CAP = 1024, TK_MAX = 32;

__device__ __forceinline__ unsigned bf16_key(bf16_t b) {        // value order == unsigned order; +-0 -> 0x8000, -inf -> 0x007f
    const unsigned u = b == 0x8000 ? 0u : (unsigned)b;
    return (u & 0x8000) ? (~u & 0xffffu) : (u | 0x8000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
    const unsigned u = (k & 0x8000) ? (k & 0x7fffu) : (~k & 0xffffu);
    return __uint_as_float(u << 16);
}
// f(c, bits) for every entry of the row, whole 16-byte chunks by vector loads (the split of lse_thread_pass)
template <class F>
__device__ __forceinline__ void row_sweep(const bf16_t* __restrict__ row, int V, int tid, F f) {
    const int head = min(V, (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 1));
    const int n8 = (V - head) >> 3;
    const bf16_t* body = row + head;
    if (tid < head) f(tid, row[tid]);
    int g = tid;
    for (; g + LPT < n8; g += 2 * LPT) {
        const u16x8 v0 = *(const u16x8*)(body + (long)g * 8);
        const u16x8 v1 = *(const u16x8*)(body + (long)(g + LPT) * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) f(head + g * 8 + e, v0[e]);
#pragma unroll
        for (int e = 0; e < 8; ++e) f(head + (g + LPT) * 8 + e, v1[e]);
    }
    for (; g < n8; g += LPT) {
        const u16x8 v0 = *(const u16x8*)(body + (long)g * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) f(head + g * 8 + e, v0[e]);
    }
    for (int c = head + n8 * 8 + tid; c < V; c += LPT) f(c, row[c]);
}
// larger == earlier in the output: key descending, then index ascending
__device__ __forceinline__ unsigned long long tk_pack(unsigned key, int c) { return ((unsigned long long)key << 32) | (0xffffffffu - (unsigned)c); }

__global__ __launch_bounds__(LPT) void topk_logprob_k(const bf16_t* __restrict__ logits, long ld, const long* __restrict__ tokens, int V,
                                                      int n, float* __restrict__ token_logprob, int* __restrict__ top_ids,
                                                      float* __restrict__ top_logprobs) {
    __shared__ float red_m[LPT / 64], red_s[LPT / 64], grp[LPT / 32];
    __shared__ int red_e[LPT / 64];
    __shared__ float fin[3];                                     // m, s, t0
    __shared__ int cnt, sel[3];                                  // list length; high digit / key K, entries above, ties to take
    __shared__ int hist[256], wcnt[LPT / 64];
    __shared__ unsigned long long cand[TK_CAP];
    const int r = blockIdx.x, tid = threadIdx.x;
    const long tgt = tokens ? tokens[r] : 0;
    if (tgt < 0 || tgt >= V) {                                   // a finished sequence: nothing of the row is read
        if (tid == 0 && token_logprob) token_logprob[r] = 0.f;
        if (tid < n) { top_ids[(long)r * n + tid] = -1; top_logprobs[(long)r * n + tid] = 0.f; }
        return;
    }
    const bf16_t* row = logits + (long)r * ld;
    const int lab = (int)tgt;
    const float xl = bf2f(row[lab]);
    float m = -INFINITY, s = 0.f;
    int early = 0;
    lse_thread_pass<false>(row, V, lab, xl, tid, m, s, early);
    float gm = m;                                                // this thread's own maximum, then its 32-thread group's
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) gm = fmaxf(gm, __shfl_xor(gm, o, 64));
    if ((tid & 31) == 0) grp[tid >> 5] = gm;
    lse_wave_merge(m, s, early, tid, red_m, red_s, red_e);
    if (tid == 0) cnt = 0;
    __syncthreads();
    if (tid == 0) {
        lse_block_merge(m, s, early, red_m, red_s, red_e);
        if (tokens) token_logprob[r] = lse_logprob(xl, m, s);
        float t0 = grp[0];
        for (int i = 1; i < LPT / 32; ++i) t0 = fminf(t0, grp[i]);
        fin[0] = m; fin[1] = s; fin[2] = t0;
    }
    if (n == 0) return;
    __syncthreads();
    const float t0 = fin[2];
    // wave-aggregated append: one LDS atomic per wave and call, whatever the number of passing lanes
    auto append = [&](bool take, unsigned key, int c) {
        const unsigned long long b = __ballot(take);
        if (b) {
            const int lane = tid & 63, leader = __ffsll((long long)b) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(&cnt, __popcll(b));
            base = __shfl(base, leader, 64);
            const int slot = base + __popcll(b & ((1ull << lane) - 1));
            if (take && slot < TK_CAP) cand[slot] = tk_pack(key, c);
        }
    };
    row_sweep(row, V, tid, [&](int c, bf16_t b) { append(bf2f(b) >= t0, bf16_key(b), c); });
    __syncthreads();
    int total = cnt;
    if (total > TK_CAP) {                                        // block-uniform: the exact rebuild
        unsigned hi = 0;
        int above = 0;
        for (int pass = 0; pass < 2; ++pass) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            if (pass == 0) row_sweep(row, V, tid, [&](int, bf16_t b) { atomicAdd(&hist[bf16_key(b) >> 8], 1); });
            else row_sweep(row, V, tid, [&](int, bf16_t b) { const unsigned k = bf16_key(b); if ((k >> 8) == hi) atomicAdd(&hist[k & 255], 1); });
            __syncthreads();
            if (tid == 0) {                                      // the digit at which the count from the top reaches n
                int d = 255, acc = above;
                while (d > 0 && acc + hist[d] < n) acc += hist[d--];
                sel[0] = d; sel[1] = acc; sel[2] = n - acc;
                if (pass == 1) cnt = 0;
            }
            __syncthreads();
            hi = (hi << 8) | (unsigned)sel[0];
            above = sel[1];
        }
        const unsigned K = hi;
        const int need = sel[2];
        row_sweep(row, V, tid, [&](int c, bf16_t b) { const unsigned k = bf16_key(b); append(k > K, k, c); });      // `above` < n entries
        int got = 0;
        for (int c0 = 0; c0 < V && got < need; c0 += LPT) {      // ties with K, lowest indices first
            const int c = c0 + tid;
            const bool tie = c < V && bf16_key(row[c]) == K;
            const unsigned long long b = __ballot(tie);
            if ((tid & 63) == 0) wcnt[tid >> 6] = __popcll(b);
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < LPT / 64; ++w) { const int k = wcnt[w]; before += w < (tid >> 6) ? k : 0; all += k; }
            const int rank = got + before + __popcll(b & ((1ull << (tid & 63)) - 1));
            if (tie && rank < need) cand[above + rank] = tk_pack(K, c);
            got += all;
            __syncthreads();
        }
        total = n;
    }
    __syncthreads();
    if (tid < total) {
        const unsigned long long mine = cand[tid];
        int rank = 0;
        for (int j = 0; j < total; ++j) rank += cand[j] > mine;
        if (rank < n) {
            top_ids[(long)r * n + rank] = (int)(0xffffffffu - (unsigned)mine);
            top_logprobs[(long)r * n + rank] = lse_logprob(key_value((unsigned)(mine >> 32)), fin[0], fin[1]);
        }
    }
}

// Classifier-free guidance of a decode step's rows (desta_cfg_scores_bf16): out[c] = g * (lc[c] - lu[c]) + lu[c] with lc / lu the
// log-probabilities of the conditional and the unconditional row, by topk_logprob_k's code (lse_thread_pass<false>, the two merges,
// lse_logprob), so they carry the bits that kernel reports.  One 1024-thread block per row.  Pass 1 reads both rows once for
// their (m, s) pairs; pass 2 reads them again (from L2, unmeasured) and stores.  Pass 2 is cut at `out`'s 16-byte boundaries: the
// elements in front of the first one and behind the last whole chunk go one by one, the chunks between by one 16-byte store
// each; an input row takes 16-byte loads there if it is aligned like `out` and 2-byte loads if not.
#pragma clang fp contract(off)
// fl(fl(g * fl(lc - lu)) + lu) rounded to bf16; a -inf entry of either row has no mass under it and stays -inf (never inf - inf)
__device__ __forceinline__ bf16_t cfg_combine(float xc, float xu, float mc, float sc, float mu, float su, float g) {
    if (xc == -INFINITY || xu == -INFINITY) return 0xff80;
    const float lc = lse_logprob(xc, mc, sc), lu = lse_logprob(xu, mu, su);
    const float d = lc - lu;
    const float t = g * d;
    return f2bf(t + lu);
}
#pragma clang fp contract(fast)

// Pass 2 over the whole 16-byte chunks of `out`'s row: two chunks per trip, so four loads are in flight per thread.  ALIGNED: both
// input rows are aligned like `out` (every decode step's buffers are); otherwise a row that is not takes 2-byte loads.
template <bool ALIGNED>
__device__ __forceinline__ void cfg_store_chunks(const bf16_t* __restrict__ rc, const bf16_t* __restrict__ ru, bf16_t* __restrict__ ro,
                                                 int head, int n8, int tid, bool vec_c, bool vec_u, float mc, float sc, float mu, float su,
                                                 float g) {
    auto load8 = [](const bf16_t* src, bool vec) {
        if (ALIGNED || vec) return *(const u16x8*)src;
        u16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = src[e];
        return v;
    };
    auto put = [&](long c0, const u16x8& vc, const u16x8& vu) {
        u16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = cfg_combine(bf2f(vc[e]), bf2f(vu[e]), mc, sc, mu, su, g);
        *(u16x8*)(ro + c0) = o;
    };
    int i = tid;
    for (; i + LPT < n8; i += 2 * LPT) {
        const long c0 = head + (long)i * 8, c1 = head + (long)(i + LPT) * 8;
        const u16x8 vc0 = load8(rc + c0, vec_c), vu0 = load8(ru + c0, vec_u);
        const u16x8 vc1 = load8(rc + c1, vec_c), vu1 = load8(ru + c1, vec_u);
        put(c0, vc0, vu0);
        put(c1, vc1, vu1);
    }
    for (; i < n8; i += LPT) {
        const long c0 = head + (long)i * 8;
        put(c0, load8(rc + c0, vec_c), load8(ru + c0, vec_u));
    }
}

__global__ __launch_bounds__(LPT) void cfg_scores_k(const bf16_t* __restrict__ cond, const bf16_t* __restrict__ uncond, long ld, int V,
                                                    float g, bf16_t* __restrict__ out, long ld_out) {
    __shared__ float red_m[2][LPT / 64], red_s[2][LPT / 64];
    __shared__ int red_e[LPT / 64];
    __shared__ float fin[4];                                     // m, s of the conditional row, then of the unconditional one
    const int r = blockIdx.x, tid = threadIdx.x;
    const bf16_t* rc = cond + (long)r * ld;
    const bf16_t* ru = uncond + (long)r * ld;
    bf16_t* ro = out + (long)r * ld_out;
    float mc = -INFINITY, sc = 0.f, mu = -INFINITY, su = 0.f;
    int early = 0;
    lse_thread_pass<false>(rc, V, 0, 0.f, tid, mc, sc, early);
    lse_thread_pass<false>(ru, V, 0, 0.f, tid, mu, su, early);
    lse_wave_merge(mc, sc, early, tid, red_m[0], red_s[0], red_e);
    lse_wave_merge(mu, su, early, tid, red_m[1], red_s[1], red_e);
    __syncthreads();
    if (tid == 0) {
        lse_block_merge(mc, sc, early, red_m[0], red_s[0], red_e);
        lse_block_merge(mu, su, early, red_m[1], red_s[1], red_e);
        fin[0] = mc; fin[1] = sc; fin[2] = mu; fin[3] = su;
    }
    __syncthreads();
    mc = fin[0]; sc = fin[1]; mu = fin[2]; su = fin[3];
    const int head = min(V, (int)(((16 - ((uintptr_t)ro & 15)) & 15) >> 1));
    const int n8 = (V - head) >> 3;
    const bool vec_c = (((uintptr_t)(rc + head)) & 15) == 0, vec_u = (((uintptr_t)(ru + head)) & 15) == 0;
    if (tid < head) ro[tid] = cfg_combine(bf2f(rc[tid]), bf2f(ru[tid]), mc, sc, mu, su, g);
    if (vec_c && vec_u) cfg_store_chunks<true>(rc, ru, ro, head, n8, tid, true, true, mc, sc, mu, su, g);
    else cfg_store_chunks<false>(rc, ru, ro, head, n8, tid, vec_c, vec_u, mc, sc, mu, su, g);
    for (int c = head + n8 * 8 + tid; c < V; c += LPT) ro[c] = cfg_combine(bf2f(rc[c]), bf2f(ru[c]), mc, sc, mu, su, g);
}

__global__ __launch_bounds__(256) void ce_finish_k(const float* __restrict__ row_loss, int M, const float* __restrict__ scal,
                                                   float* __restrict__ loss) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < M; i += 256) s += row_loss[i];
    s = block_sum<256>(s, red);
    if (threadIdx.x == 0) loss[0] = s * scal[1];
}

constexpr int MAXT = 32;           // tapped encoder layers (4 in the shipped configs; 32 = every layer of whisper-large with orca_use_all_layers)

// out[n][c] = sum_j softmax(lw[k])[j] * x[j][n][c],  n = b*K + k;  x: [taps][N][d] f32
__global__ __launch_bounds__(256) void mix_fwd_k(const float* __restrict__ x, const float* __restrict__ lw, int taps, int N,
                                                 int K, int d, float* __restrict__ out) {
    const int n = blockIdx.x, k = n % K;
    float sm[MAXT];
    float mx = -INFINITY, den = 0.f;
    for (int j = 0; j < taps; ++j) mx = fmaxf(mx, lw[k * taps + j]);
    for (int j = 0; j < taps; ++j) { sm[j] = __expf(lw[k * taps + j] - mx); den += sm[j]; }
    for (int c = threadIdx.x * 4; c < d; c += 1024) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < taps; ++j) {
            const float wj = sm[j] / den;
            const float4 v = *(const float4*)(x + ((long)j * N + n) * d + c);
            acc.x += wj * v.x; acc.y += wj * v.y; acc.z += wj * v.z; acc.w += wj * v.w;
        }
        *(float4*)(out + (long)n * d + c) = acc;
    }
}

// one block per query slot k: dx[j][b*K+k][:] = sm[k][j] * dout[b*K+k][:];  dlw[k][:] = softmax'(...)
__global__ __launch_bounds__(256) void mix_bwd_k(const float* __restrict__ x, const float* __restrict__ lw,
                                                 const float* __restrict__ dout, int taps, int Bn, int K, int d,
                                                 float* __restrict__ dx, float* __restrict__ dlw) {
    __shared__ float red[4];
    const int k = blockIdx.x, N = Bn * K;
    float sm[MAXT], ds[MAXT];
    float mx = -INFINITY, den = 0.f;
    for (int j = 0; j < taps; ++j) mx = fmaxf(mx, lw[k * taps + j]);
    for (int j = 0; j < taps; ++j) { sm[j] = __expf(lw[k * taps + j] - mx); den += sm[j]; }
    for (int j = 0; j < taps; ++j) { sm[j] /= den; ds[j] = 0.f; }
    for (int b = 0; b < Bn; ++b) {
        const long n = (long)b * K + k;
        for (int c = threadIdx.x * 4; c < d; c += 1024) {
            const float4 g = *(const float4*)(dout + n * d + c);
            for (int j = 0; j < taps; ++j) {
                const float4 v = *(const float4*)(x + ((long)j * N + n) * d + c);
                ds[j] += (g.x * v.x + g.y * v.y) + (g.z * v.z + g.w * v.w);
                *(float4*)(dx + ((long)j * N + n) * d + c) = make_float4(sm[j] * g.x, sm[j] * g.y, sm[j] * g.z, sm[j] * g.w);
            }
        }
    }
    float dot = 0.f;
    for (int j = 0; j < taps; ++j) { ds[j] = block_sum<256>(ds[j], red); dot += sm[j] * ds[j]; }
    if (threadIdx.x == 0)
        for (int j = 0; j < taps; ++j) dlw[k * taps + j] = sm[j] * (ds[j] - dot);
}

// x32/x16[(j*B + b)][:] = prompts[j][:]   (rows of n = K*d floats; layer_prompts[j].expand(B,-1,-1))
__global__ __launch_bounds__(256) void prompt_expand_k(const float* __restrict__ prompts, int taps, int Bn, long n,
                                                       float* __restrict__ x32, bf16_t* __restrict__ x16) {
    const long n4 = n / 4, total = (long)taps * Bn * n4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long jb = i / n4, c = (i % n4) * 4;
        const int j = (int)(jb / Bn);
        const float4 v = *(const float4*)(prompts + (long)j * n + c);
        *(float4*)(x32 + jb * n + c) = v;
        u16x4 o;
        o[0] = f2bf(v.x); o[1] = f2bf(v.y); o[2] = f2bf(v.z); o[3] = f2bf(v.w);
        *(u16x4*)(x16 + jb * n + c) = o;
    }
}
// dprompts[j][:] = sum_b dx[(j*B + b)][:]   (fixed order)
__global__ __launch_bounds__(256) void prompt_grad_k(const float* __restrict__ dx, int taps, int Bn, long n,
                                                     float* __restrict__ dprompts) {
    const long n4 = n / 4, total = (long)taps * n4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int j = (int)(i / n4);
        const long c = (i % n4) * 4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b = 0; b < Bn; ++b) {
            const float4 v = *(const float4*)(dx + ((long)j * Bn + b) * n + c);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        *(float4*)(dprompts + (long)j * n + c) = acc;
    }
}

}  // namespace

extern "C" int desta_prompt_expand(const float* prompts, int taps, int batch, int64_t n, float* x_f32, void* x_bf16, void* stream) {
    DESTA_CHECK_ARG(prompts && x_f32 && x_bf16 && taps > 0 && batch > 0 && n > 0 && n % 4 == 0, "prompt_expand: bad argument");
    long blocks = ((long)taps * batch * (n / 4) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(prompt_expand_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, prompts, taps, batch, (long)n, x_f32, (bf16_t*)x_bf16);
    DESTA_CHECK_LAUNCH("prompt_expand");
    return DESTA_OK;
}

extern "C" int desta_prompt_grad(const float* dx, int taps, int batch, int64_t n, float* dprompts, void* stream) {
    DESTA_CHECK_ARG(dx && dprompts && taps > 0 && batch > 0 && n > 0 && n % 4 == 0, "prompt_grad: bad argument");
    long blocks = ((long)taps * (n / 4) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(prompt_grad_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dx, taps, batch, (long)n, dprompts);
    DESTA_CHECK_LAUNCH("prompt_grad");
    return DESTA_OK;
}

extern "C" int desta_embed_gather(const void* table, const void* audio_rows, const int32_t* src_row, int rows, int hidden,
                                  void* out, void* stream) {
    DESTA_CHECK_ARG(table && src_row && out && rows > 0 && hidden % 8 == 0, "embed_gather: bad argument");
    hipLaunchKernelGGL(embed_gather_k, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)table,
                       (const bf16_t*)audio_rows, src_row, rows, hidden, (bf16_t*)out);
    DESTA_CHECK_LAUNCH("embed_gather");
    return DESTA_OK;
}

extern "C" int desta_gather_rows_bf16(const void* in, const int32_t* idx, int rows, int hidden, void* out, void* stream) {
    DESTA_CHECK_ARG(in && idx && out && rows > 0 && hidden % 8 == 0, "gather_rows: bad argument");
    hipLaunchKernelGGL(gather_rows_k, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)in, idx, rows,
                       hidden, (bf16_t*)out);
    DESTA_CHECK_LAUNCH("gather_rows");
    return DESTA_OK;
}

extern "C" int desta_scatter_rows_bf16(const void* in, const int32_t* idx, int rows, int hidden, void* out, void* stream) {
    DESTA_CHECK_ARG(in && idx && out && rows > 0 && hidden % 8 == 0, "scatter_rows: bad argument");
    hipLaunchKernelGGL(scatter_rows_k, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)in, idx, rows,
                       hidden, (bf16_t*)out);
    DESTA_CHECK_LAUNCH("scatter_rows");
    return DESTA_OK;
}

extern "C" int desta_target_rows(const int64_t* labels, int batch, int seq, int32_t* idx, int64_t* compact_labels, int32_t* count,
                                 int s_major, void* stream) {
    DESTA_CHECK_ARG(labels && idx && compact_labels && count && batch > 0 && seq > 0, "target_rows: bad argument");
    hipLaunchKernelGGL(target_rows_k, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const long*)labels, batch, seq, idx,
                       (long*)compact_labels, count, s_major);
    DESTA_CHECK_LAUNCH("target_rows");
    return DESTA_OK;
}

extern "C" size_t desta_ce_workspace_floats(int batch, int seq) { return (size_t)batch * seq + 8; }

extern "C" int desta_causal_lm_loss(void* logits, int64_t ld, const int64_t* labels, int batch, int seq, int vocab,
                                    float* loss, float* workspace, int write_grad, void* stream) {
    DESTA_CHECK_ARG(logits && labels && loss && workspace, "causal_lm_loss: null argument");
    DESTA_CHECK_ARG(batch > 0 && seq > 0 && vocab > 0 && ld >= vocab && ld % 8 == 0, "causal_lm_loss: bad shape");
    DESTA_CHECK_ARG(((uintptr_t)logits % 16) == 0, "causal_lm_loss: logits must be 16-byte aligned");
    float* scal = workspace;
    float* row_loss = workspace + 8;
    hipStream_t st = (hipStream_t)stream;
    const int M = batch * seq;
    hipLaunchKernelGGL(ce_count_k, dim3(1), dim3(256), 0, st, (const long*)labels, batch, seq, scal);
    const int nv8 = vocab / 8;
#define CE_ARGS dim3(M), dim3(1024), 0, st, (bf16_t*)logits, (long)ld, (const long*)labels, seq, vocab, (const float*)scal, row_loss, write_grad
    if (vocab % 8 == 0 && nv8 > 2048 && nv8 <= 1024 * 16) hipLaunchKernelGGL(ce_row_reg_k<16>, CE_ARGS);
    else if (vocab % 8 == 0 && nv8 > 2048 && nv8 <= 1024 * 20) hipLaunchKernelGGL(ce_row_reg_k<20>, CE_ARGS);
    else
        hipLaunchKernelGGL(ce_row_k, dim3(M), dim3(256), 0, st, (bf16_t*)logits, (long)ld, (const long*)labels, seq, vocab,
                           (const float*)scal, row_loss, write_grad);
#undef CE_ARGS
    hipLaunchKernelGGL(ce_finish_k, dim3(1), dim3(256), 0, st, (const float*)row_loss, M, (const float*)scal, loss);
    DESTA_CHECK_LAUNCH("causal_lm_loss");
    return DESTA_OK;
}

extern "C" int desta_token_logprobs(const void* logits_bf16, int64_t ld, const int64_t* labels, int rows, int vocab,
                                    float* logprob, uint8_t* is_top1, void* stream) {
    DESTA_CHECK_ARG(logits_bf16 && labels && logprob, "token_logprobs: null argument");
    DESTA_CHECK_ARG(rows > 0 && vocab > 0 && ld >= vocab, "token_logprobs: bad shape");
    hipLaunchKernelGGL(token_logprob_k, dim3(rows), dim3(LPT), 0, (hipStream_t)stream, (const bf16_t*)logits_bf16, (long)ld,
                       (const long*)labels, vocab, logprob, is_top1);
    DESTA_CHECK_LAUNCH("token_logprobs");
    return DESTA_OK;
}

extern "C" int desta_topk_logprobs(const void* logits_bf16, int64_t ld, const int64_t* tokens, int rows, int vocab, int top_n,
                                   float* token_logprob, int32_t* top_ids, float* top_logprobs, void* stream) {
    DESTA_CHECK_ARG(logits_bf16, "topk_logprobs: null logits");
    DESTA_CHECK_ARG(rows > 0 && vocab > 0 && vocab <= 262144 && ld >= vocab, "topk_logprobs: bad shape");
    DESTA_CHECK_ARG(top_n >= 0 && top_n <= TK_MAX && top_n <= vocab, "topk_logprobs: top_n outside 0..32 (or above vocab)");
    DESTA_CHECK_ARG((tokens != nullptr) == (token_logprob != nullptr), "topk_logprobs: tokens and token_logprob go together");
    DESTA_CHECK_ARG(top_n == 0 || (top_ids && top_logprobs), "topk_logprobs: null top_ids / top_logprobs with top_n > 0");
    DESTA_CHECK_ARG(tokens || top_n > 0, "topk_logprobs: nothing to compute");
    hipLaunchKernelGGL(topk_logprob_k, dim3(rows), dim3(LPT), 0, (hipStream_t)stream, (const bf16_t*)logits_bf16, (long)ld,
                       (const long*)tokens, vocab, top_n, token_logprob, top_ids, top_logprobs);
    DESTA_CHECK_LAUNCH("topk_logprobs");
    return DESTA_OK;
}

extern "C" int desta_cfg_scores_bf16(const void* cond_bf16, const void* uncond_bf16, int64_t ld, int rows, int vocab,
                                     float guidance_scale, void* out_bf16, int64_t ld_out, void* stream) {
    DESTA_CHECK_ARG(cond_bf16 && uncond_bf16 && out_bf16, "cfg_scores: null argument");
    DESTA_CHECK_ARG(out_bf16 != cond_bf16 && out_bf16 != uncond_bf16, "cfg_scores: out may not be an input");
    DESTA_CHECK_ARG(rows > 0 && vocab > 0 && vocab <= 262144 && ld >= vocab && ld_out >= vocab, "cfg_scores: bad shape");
    DESTA_CHECK_ARG(guidance_scale > 0.f && guidance_scale < INFINITY, "cfg_scores: guidance_scale must be finite and > 0");
    hipLaunchKernelGGL(cfg_scores_k, dim3(rows), dim3(LPT), 0, (hipStream_t)stream, (const bf16_t*)cond_bf16,
                       (const bf16_t*)uncond_bf16, (long)ld, vocab, guidance_scale, (bf16_t*)out_bf16, (long)ld_out);
    DESTA_CHECK_LAUNCH("cfg_scores");
    return DESTA_OK;
}

extern "C" int desta_tap_mix_fwd(const float* x, const float* layer_weights, int taps, int batch, int prompt, int d,
                                 float* out, void* stream) {
    DESTA_CHECK_ARG(x && layer_weights && out && taps > 0 && taps <= MAXT && d % 4 == 0, "tap_mix_fwd: bad argument");
    hipLaunchKernelGGL(mix_fwd_k, dim3(batch * prompt), dim3(256), 0, (hipStream_t)stream, x, layer_weights, taps,
                       batch * prompt, prompt, d, out);
    DESTA_CHECK_LAUNCH("tap_mix_fwd");
    return DESTA_OK;
}

extern "C" int desta_tap_mix_bwd(const float* x, const float* layer_weights, const float* dout, int taps, int batch,
                                 int prompt, int d, float* dx, float* dlayer_weights, void* stream) {
    DESTA_CHECK_ARG(x && layer_weights && dout && dx && dlayer_weights && taps > 0 && taps <= MAXT && d % 4 == 0,
                    "tap_mix_bwd: bad argument");
    hipLaunchKernelGGL(mix_bwd_k, dim3(prompt), dim3(256), 0, (hipStream_t)stream, x, layer_weights, dout, taps, batch,
                       prompt, d, dx, dlayer_weights);
    DESTA_CHECK_LAUNCH("tap_mix_bwd");
    return DESTA_OK;
}
