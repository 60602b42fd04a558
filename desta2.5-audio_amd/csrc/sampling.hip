// One decode step of HF's logits chain on bf16 logits (gfx950): repetition penalty -> greedy argmax, or
// temperature -> top-k -> top-p -> min-p -> one draw.  Reference call sites (TF: = transformers 5.15):
//   llm_model.generate(...) ........ modeling_desta25.py:1419-1427 (inputs_embeds), :1703-1711 (input_ids)
//   processor order ................ TF:generation/utils.py:1175 (penalty), :1296-1330 (warpers, do_sample only)
//   processors ..................... TF:generation/logits_process.py RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
//                                    TopKLogitsWarper, TopPLogitsWarper, MinPLogitsWarper; scores are fp32 (TF:generation/utils.py:2894)
//
// One 1024-thread block per row, one launch per step.  Every score is recomputed from the bf16 row on each pass (the row stays
// in L2): s = bf16 logit, penalised through an LDS bitmap of the row's history tokens, then t = s / T.  Scores map to monotone
// 32-bit keys, and both cut-offs are found by a radix select over those keys with LDS histograms (12 + 10 + 10 bits, three
// passes each): top-k on counts, top-p on masses e_j = exp(t_j - t_max) held as 2^-40 fixed point, so every sum is an
// integer sum and its order cannot change the result.  The draw inverts the prefix sum of the kept masses in index order.
//
// sample_truncated_k (desta_sample_truncated_rows_bf16) puts TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper
// between min-p and the draw.  Each renormalises over the survivors so far: one reduction pass per active step gives their
// Z = sum e, sum e * (-a) (a = t - t_max, both 2^-40 fixed point) and largest key; typical-p adds a three-pass radix select over
// the keys of d = |a - c| with the same mass bins.  Both kernels are one body, sampling_chain.h, included once per kernel;
// sample_chain_k compiles to the assembly it had before steps 7-9 existed.
#include "common.h"
#include "desta_hip.h"

namespace {

typedef unsigned long long u64;

constexpr int SNT = 1024;                      // threads per row
constexpr int SBINS = 4096;                    // bins of the first radix digit (key bits 31..20); later digits use 1024
constexpr int PEN_MAX_COLS = 262144;           // LDS bitmap of penalised tokens: 32 KiB
constexpr float MASS_ONE = 1099511627776.0f;   // 2^40: fixed-point scale of exp(t - t_max) <= 1
constexpr int SAMPLE_ROWS_MAX_WIDTH = 8;       // rows per sequence of a grouped launch: a verify step's k + 1 <= SPEC_K_MAX + 1

// monotone map of fp32 order onto u32; -0 maps onto +0 (they compare equal in torch)
__device__ __forceinline__ unsigned f32_key(float v) {
    unsigned b = __float_as_uint(v);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// f(c, bf16 bits) over a row, element c on thread c / 8 % SNT (16-B loads when the row is 16-B aligned)
template <class F>
__device__ __forceinline__ void row_strided(const bf16_t* __restrict__ row, int cols, bool vec, F&& f) {
    int c = threadIdx.x;
    if (vec) {
        const int n8 = cols >> 3;
        for (int g = threadIdx.x; g < n8; g += SNT) {
            const u16x8 v = *(const u16x8*)(row + (long)g * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) f(g * 8 + j, (bf16_t)v[j]);
        }
        c = n8 * 8 + threadIdx.x;
    }
    for (; c < cols; c += SNT) f(c, row[c]);
}
// f(c, bf16 bits) over this thread's contiguous chunk [c0, c1) (c0 a multiple of 8), in index order
template <class F>
__device__ __forceinline__ void row_chunk(const bf16_t* __restrict__ row, int c0, int c1, bool vec, F&& f) {
    int c = c0;
    if (vec)
        for (; c + 8 <= c1; c += 8) {
            const u16x8 v = *(const u16x8*)(row + c);
#pragma unroll
            for (int j = 0; j < 8; ++j) f(c + j, (bf16_t)v[j]);
        }
    for (; c < c1; ++c) f(c, row[c]);
}

__device__ __forceinline__ u64 wave_incl_scan(u64 v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(v, o, 64);
        if (lane >= o) v += y;
    }
    return v;
}

// Radix step over bins[0, R * SNT) (thread t owns bins [t*R, t*R + R)).  mfun(total) gives the target rank m (< total); the
// bin b with excl(b) <= m < excl(b) + bins[b] in ascending order is written to sel[0], excl(b) to sel[1].  Integer sums only.
template <int R, class MF>
__device__ __forceinline__ void select_bin(const u64* bins, u64* wred, u64* sel, MF&& mfun) {
    const int tid = threadIdx.x;
    u64 v[R], local = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        v[j] = bins[tid * R + j];
        local += v[j];
    }
    const u64 inc = wave_incl_scan(local);
    if ((tid & 63) == 63) wred[tid >> 6] = inc;
    __syncthreads();
    u64 total = 0, before = 0;
#pragma unroll
    for (int w = 0; w < SNT / 64; ++w) {
        total += wred[w];
        before += w < (tid >> 6) ? wred[w] : 0ull;
    }
    const u64 m = mfun(total);
    u64 excl = before + inc - local;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if (excl <= m && m < excl + v[j]) {
            sel[0] = (u64)(tid * R + j);
            sel[1] = excl;
        }
        excl += v[j];
    }
    __syncthreads();
}

// The grid is (batch, width): block (b, j) works on row r = b * width + j of the logits, row j of sequence b
// (desta_sample_rows_bf16; width 1, the one-row entry point: r = b, j = 0): emitted position step + j of sequence b, whose history
// is hist[b] followed by the j tokens tail[b][1 .. 1 + j)
struct GroupRow {
    int b, j, r;
};
__device__ __forceinline__ GroupRow group_row(int width) { return {(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.x * width + (int)blockIdx.y}; }

// LDS bitmap of the distinct history tokens of sequence g.b in front of its row g.j (RepetitionPenaltyLogitsProcessor gathers
// from the original scores, so a token that occurs several times is penalised once)
__device__ __forceinline__ void build_penalty_bits(unsigned* pen_bits, int cols, GroupRow g, const long* __restrict__ hist, long hist_ld,
                                                   int hist_len, const long* __restrict__ tail, long tail_ld) {
    for (int i = threadIdx.x; i < (cols + 31) >> 5; i += SNT) pen_bits[i] = 0u;
    __syncthreads();
    const long* h = hist + (long)g.b * hist_ld;
    for (int i = threadIdx.x; i < hist_len; i += SNT) {
        const long id = h[i];
        if (id >= 0 && id < cols) atomicOr(&pen_bits[id >> 5], 1u << (id & 31));
    }
    if ((int)threadIdx.x < g.j) {                                            // g.j > 0 only with a tail (checked on the host)
        const long id = tail[(long)g.b * tail_ld + 1 + threadIdx.x];
        if (id >= 0 && id < cols) atomicOr(&pen_bits[id >> 5], 1u << (id & 31));
    }
    __syncthreads();
}
// the penalised fp32 score of token c: s < 0 ? s * p : s / p for history tokens
__device__ __forceinline__ float penalised(const unsigned* pen_bits, bool pen, float penalty, int c, bf16_t b) {
    float s = bf2f(b);
    if (pen && ((pen_bits[c >> 5] >> (c & 31)) & 1u)) s = s < 0.f ? s * penalty : s / penalty;
    return s;
}

// greedy (do_sample = 0): first index of the maximum penalised score, as torch.argmax
__global__ __launch_bounds__(SNT) void sample_greedy_k(const bf16_t* __restrict__ x, long ld, int cols, const long* __restrict__ hist,
                                                       long hist_ld, int hist_len, const long* __restrict__ tail, long tail_ld, int width,
                                                       float penalty, long* __restrict__ out, unsigned char* __restrict__ keep_mask) {
    __shared__ unsigned pen_bits[PEN_MAX_COLS / 32];
    __shared__ u64 wred[SNT / 64];
    const GroupRow g = group_row(width);
    const int tid = threadIdx.x, r = g.r;
    const bf16_t* row = x + (long)r * ld;
    const bool pen = penalty != 1.0f && hist_len + g.j > 0;
    if (pen) build_penalty_bits(pen_bits, cols, g, hist, hist_ld, hist_len, tail, tail_ld);
    u64 best = 0;
    row_strided(row, cols, ((uintptr_t)row & 15) == 0, [&](int c, bf16_t b) {
        const u64 k = ((u64)f32_key(penalised(pen_bits, pen, penalty, c, b)) << 32) | (unsigned)(~(unsigned)c);
        best = k > best ? k : best;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 ok = __shfl_xor(best, o, 64);
        best = ok > best ? ok : best;
    }
    if ((tid & 63) == 0) wred[tid >> 6] = best;
    __syncthreads();
    best = wred[0];
#pragma unroll
    for (int w = 1; w < SNT / 64; ++w) best = wred[w] > best ? wred[w] : best;
    const int pick = (int)(~(unsigned)(best & 0xffffffffu));
    if (tid == 0) out[r] = pick;
    if (keep_mask)
        for (int c = tid; c < cols; c += SNT) keep_mask[(long)r * cols + c] = c == pick ? 1 : 0;
}

// steps 7-9 of desta_sample_truncated_rows_bf16; 1 / 0 / 0 switch a step off
struct Truncation {
    float typical_p, epsilon_cutoff, eta_cutoff;
};

// the chain kernel and its twin with steps 7-9: one body, sampling_chain.h
#define CHAIN_KERNEL sample_chain_k
#define CHAIN_TR 0
#include "sampling_chain.h"
#define CHAIN_KERNEL sample_truncated_k
#define CHAIN_TR 1
#include "sampling_chain.h"

// the checks and the launch of every entry point: `batch` sequences of `width` rows each; tr == nullptr: steps 7-9 do not exist
int sample_launch(const void* logits, int64_t ld, int batch, int width, int cols, const int64_t* hist, int64_t hist_ld, int hist_len,
                  const int64_t* tail, int64_t tail_ld, float repetition_penalty, int do_sample, float temperature, int top_k, float top_p,
                  float min_p, const Truncation* tr, uint64_t seed, uint32_t step0, int64_t* out, uint8_t* keep_mask, void* stream) {
    DESTA_CHECK_ARG(logits && out && batch > 0 && cols > 0 && ld >= cols, "sample: bad argument");
    DESTA_CHECK_ARG(width >= 1 && width <= SAMPLE_ROWS_MAX_WIDTH, "sample: width %d out of range (1..%d)", width, SAMPLE_ROWS_MAX_WIDTH);
    DESTA_CHECK_ARG(temperature > 0.f, "sample: need temperature > 0");
    DESTA_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "sample: need 0 < top_p <= 1");
    DESTA_CHECK_ARG(top_k >= 0, "sample: need top_k >= 0");
    DESTA_CHECK_ARG(min_p >= 0.f && min_p <= 1.f, "sample: need 0 <= min_p <= 1");
    DESTA_CHECK_ARG(repetition_penalty > 0.f, "sample: need repetition_penalty > 0");
    DESTA_CHECK_ARG(hist_len >= 0 && (hist_len == 0 || (hist && hist_ld >= hist_len)), "sample: bad token history");
    DESTA_CHECK_ARG(width == 1 || repetition_penalty == 1.f || (tail && tail_ld >= width),
                    "sample: a repetition penalty over %d rows per sequence needs the tail tokens", width);
    DESTA_CHECK_ARG(repetition_penalty == 1.f || (hist_len == 0 && width == 1) || cols <= PEN_MAX_COLS,
                    "sample: a repetition penalty needs cols <= %d", PEN_MAX_COLS);
    bool truncated = false;
    if (tr) {
        DESTA_CHECK_ARG(tr->typical_p > 0.f && tr->typical_p <= 1.f, "sample: need 0 < typical_p <= 1");
        DESTA_CHECK_ARG(tr->epsilon_cutoff >= 0.f && tr->epsilon_cutoff < 1.f, "sample: need 0 <= epsilon_cutoff < 1");
        DESTA_CHECK_ARG(tr->eta_cutoff >= 0.f && tr->eta_cutoff < 1.f, "sample: need 0 <= eta_cutoff < 1");
        truncated = tr->typical_p < 1.f || tr->epsilon_cutoff > 0.f || tr->eta_cutoff > 0.f;
    }
    if (!do_sample)
        hipLaunchKernelGGL(sample_greedy_k, dim3(batch, width), dim3(SNT), 0, (hipStream_t)stream, (const bf16_t*)logits, (long)ld, cols,
                           (const long*)hist, (long)hist_ld, hist_len, (const long*)tail, (long)tail_ld, width, repetition_penalty,
                           (long*)out, keep_mask);
    else if (!truncated)
        hipLaunchKernelGGL(sample_chain_k, dim3(batch, width), dim3(SNT), 0, (hipStream_t)stream, (const bf16_t*)logits, (long)ld, cols,
                           (const long*)hist, (long)hist_ld, hist_len, (const long*)tail, (long)tail_ld, width, repetition_penalty,
                           temperature, top_k, top_p, min_p, (unsigned)seed, (unsigned)(seed >> 32), step0, (long*)out, keep_mask);
    else
        hipLaunchKernelGGL(sample_truncated_k, dim3(batch, width), dim3(SNT), 0, (hipStream_t)stream, (const bf16_t*)logits, (long)ld,
                           cols, (const long*)hist, (long)hist_ld, hist_len, (const long*)tail, (long)tail_ld, width, repetition_penalty,
                           temperature, top_k, top_p, min_p, *tr, (unsigned)seed, (unsigned)(seed >> 32), step0, (long*)out, keep_mask);
    DESTA_CHECK_LAUNCH("sample");
    return DESTA_OK;
}

}  // namespace

extern "C" int desta_sample_bf16(const void* logits, int64_t ld, int rows, int cols, const int64_t* hist, int64_t hist_ld, int hist_len,
                                 float repetition_penalty, int do_sample, float temperature, int top_k, float top_p, float min_p,
                                 uint64_t seed, uint32_t step, int64_t* out, uint8_t* keep_mask, void* stream) {
    return sample_launch(logits, ld, rows, 1, cols, hist, hist_ld, hist_len, nullptr, 0, repetition_penalty, do_sample, temperature, top_k,
                         top_p, min_p, nullptr, seed, step, out, keep_mask, stream);
}

extern "C" int desta_sample_rows_bf16(const void* logits, int64_t ld, int batch, int width, int cols, const int64_t* hist, int64_t hist_ld,
                                      int hist_len, const int64_t* tail, int64_t tail_ld, float repetition_penalty, int do_sample,
                                      float temperature, int top_k, float top_p, float min_p, uint64_t seed, uint32_t step0, int64_t* out,
                                      uint8_t* keep_mask, void* stream) {
    return sample_launch(logits, ld, batch, width, cols, hist, hist_ld, hist_len, tail, tail_ld, repetition_penalty, do_sample, temperature,
                         top_k, top_p, min_p, nullptr, seed, step0, out, keep_mask, stream);
}

extern "C" int desta_sample_truncated_rows_bf16(const void* logits, int64_t ld, int batch, int width, int cols, const int64_t* hist,
                                                int64_t hist_ld, int hist_len, const int64_t* tail, int64_t tail_ld,
                                                float repetition_penalty, int do_sample, float temperature, int top_k, float top_p,
                                                float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff, uint64_t seed,
                                                uint32_t step0, int64_t* out, uint8_t* keep_mask, void* stream) {
    const Truncation tr = {typical_p, epsilon_cutoff, eta_cutoff};
    return sample_launch(logits, ld, batch, width, cols, hist, hist_ld, hist_len, tail, tail_ld, repetition_penalty, do_sample, temperature,
                         top_k, top_p, min_p, &tr, seed, step0, out, keep_mask, stream);
}
