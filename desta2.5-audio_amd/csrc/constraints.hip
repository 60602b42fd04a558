// The hard constraints of HF's logits chain on the bf16 scores of one decode step (gfx950): tokens banned as a function of the
// row's history get -inf, every other score keeps its bits.  Reference call sites (TF: = transformers 5.15):
//   llm_model.generate(...) ........ modeling_desta25.py:1419-1427 (inputs_embeds), :1703-1711 (input_ids)
//   processor order ................ TF:generation/utils.py:1174-1290 (_get_logits_processor)
//   processors ..................... TF:generation/logits_process.py NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor,
//                                    SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor,
//                                    MinNewTokensLengthLogitsProcessor
//
// One 1024-thread block per row, one launch per step.  The banned set is an LDS bitmap over the columns: a strided scan of the
// history marks the n-gram continuations (its n - 1 context compares read global memory, which sits in L2), one thread per bad
// word marks that word's last token, the begin and EOS lists are marked by the step number.  In place only the marked columns
// are stored; out of place one pass copies the row with the marked columns replaced.  The pickers that follow treat -inf as
// "never kept", and the repetition penalty maps -inf to -inf, so the pass commutes with it and runs in front of them.
#include "common.h"
#include "desta_hip.h"

namespace {

constexpr int CNT = 1024;                      // threads per row
constexpr int CON_MAX_COLS = 262144;           // LDS bitmap of banned tokens: 32 KiB (the samplers' PEN_MAX_COLS)
constexpr int CON_MAX_WIDTH = 8;               // rows per sequence of a grouped launch (the samplers' SAMPLE_ROWS_MAX_WIDTH)
constexpr int CON_MAX_WORDS = 65536;           // bad words of one table (one thread per word and pass: 64 passes at the cap)
constexpr int CON_MAX_WORD_IDS = 1048576;      // flattened ids of one table (4 MiB of int32)
constexpr bf16_t BF16_NEG_INF = 0xFF80;

// block (b, j) of the (batch, width) grid works on row r = b * width + j: emitted position step0 + j of sequence b, whose history
// is hist[b] followed by the j tokens tail[b][1 .. 1 + j) (the samplers' GroupRow)
struct GroupRow {
    int b, j, r;
};
__device__ __forceinline__ GroupRow group_row(int width) { return {(int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.x * width + (int)blockIdx.y}; }

__device__ __forceinline__ void ban(unsigned* bits, int cols, long id) {
    if (id >= 0 && id < cols) atomicOr(&bits[id >> 5], 1u << (id & 31));       // LDS; any other value can match, never be banned
}

__global__ __launch_bounds__(CNT) void logit_constraints_k(const bf16_t* src, long ld_src, bf16_t* dst, long ld_dst, int width,
                                                           int cols, const long* __restrict__ hist, long hist_ld, int hist_len,
                                                           const long* __restrict__ tail, long tail_ld, unsigned step0, int ngram,
                                                           const int* __restrict__ word_ids, const int* __restrict__ word_off, int n_words,
                                                           int n_word_ids,
                                                           const int* __restrict__ begin_ids, int n_begin,
                                                           const int* __restrict__ eos_ids, int n_eos, int min_new) {
    __shared__ unsigned bits[CON_MAX_COLS / 32];
    const GroupRow g = group_row(width);
    const int tid = threadIdx.x;
    const int nw = (cols + 31) >> 5;
    for (int i = tid; i < nw; i += CNT) bits[i] = 0u;
    __syncthreads();

    const int L = hist_len + g.j;                                            // HF's cur_len of this row
    const unsigned t = step0 + (unsigned)g.j;                                // emitted position (a uint32 sum, as the samplers')
    // token i of the row's history, 0 <= i < L; g.j > 0 only with a tail (checked on the host)
    auto H = [&](int i) -> long { return i < hist_len ? hist[(long)g.b * hist_ld + i] : tail[(long)g.b * tail_ld + 1 + (i - hist_len)]; };

    // NoRepeatNGramLogitsProcessor: the token behind every earlier occurrence of the last n - 1 tokens
    if (ngram > 0 && L + 1 >= ngram) {
        const int ctx = ngram - 1, s0 = L - ctx;
        for (int i = tid; i <= L - ngram; i += CNT) {
            bool same = true;
            for (int q = 0; q < ctx && same; ++q) same = H(i + q) == H(s0 + q);
            if (same) ban(bits, cols, H(i + ctx));
        }
    }
    // NoBadWordsLogitsProcessor (SuppressTokensLogitsProcessor folded in as one-token words): a word longer than the history is
    // skipped, m <= L and not m - 1 <= L (TF:generation/logits_process.py:1303)
    for (int w = tid; w < n_words; w += CNT) {
        const int o = word_off[w], m = word_off[w + 1] - o;
        if (o < 0 || m < 1 || m > n_word_ids - o || (m > 1 && m > L)) continue;      // a table that is not one is not followed
        bool same = true;
        for (int q = 0; q < m - 1 && same; ++q) same = H(L - (m - 1) + q) == (long)word_ids[o + q];
        if (same) ban(bits, cols, word_ids[o + m - 1]);
    }
    // SuppressTokensAtBeginLogitsProcessor, MinNewTokensLengthLogitsProcessor
    if (t == 0u)
        for (int i = tid; i < n_begin; i += CNT) ban(bits, cols, begin_ids[i]);
    if (t < (unsigned)min_new)
        for (int i = tid; i < n_eos; i += CNT) ban(bits, cols, eos_ids[i]);
    __syncthreads();

    const bf16_t* s = src + (long)g.r * ld_src;
    bf16_t* d = dst + (long)g.r * ld_dst;
    if (s == d) {                                                            // in place: only the banned entries are stored
        for (int i = tid; i < nw; i += CNT)
            for (unsigned m = bits[i]; m; m &= m - 1u) d[i * 32 + __builtin_ctz(m)] = BF16_NEG_INF;    // bits >= cols are never set
        return;
    }
    int c = tid;
    if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {                         // 16-byte loads and stores when both rows are aligned
        const int n8 = cols >> 3;
        for (int q = tid; q < n8; q += CNT) {
            u16x8 v = *(const u16x8*)(s + (long)q * 8);
            const unsigned m = (bits[q >> 2] >> ((q & 3) * 8)) & 0xffu;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = ((m >> e) & 1u) ? BF16_NEG_INF : v[e];
            *(u16x8*)(d + (long)q * 8) = v;
        }
        c = n8 * 8 + tid;
    }
    for (; c < cols; c += CNT) d[c] = ((bits[c >> 5] >> (c & 31)) & 1u) ? BF16_NEG_INF : s[c];
}

}  // namespace

extern "C" int desta_logit_constraints_bf16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int batch, int width, int cols,
                                            const int64_t* hist, int64_t hist_ld, int hist_len, const int64_t* tail, int64_t tail_ld,
                                            uint32_t step0, int no_repeat_ngram, const int32_t* word_ids, const int32_t* word_off,
                                            int n_words, int n_word_ids, const int32_t* begin_ids, int n_begin, const int32_t* eos_ids,
                                            int n_eos, int min_new_tokens, int id_max, void* stream) {
    DESTA_CHECK_ARG(src && dst, "logit_constraints: null argument");
    DESTA_CHECK_ARG(batch > 0 && cols > 0 && hist_len >= 0 && no_repeat_ngram >= 0 && n_words >= 0 && n_word_ids >= 0 && n_begin >= 0 &&
                        n_eos >= 0 && min_new_tokens >= 0,
                    "logit_constraints: a size is negative (or batch / cols is 0)");
    DESTA_CHECK_ARG(cols <= CON_MAX_COLS, "logit_constraints: cols %d > %d", cols, CON_MAX_COLS);
    DESTA_CHECK_ARG(ld_src >= cols && ld_dst >= cols, "logit_constraints: a row stride is below cols");
    DESTA_CHECK_ARG(width >= 1 && width <= CON_MAX_WIDTH, "logit_constraints: width %d out of range (1..%d)", width, CON_MAX_WIDTH);
    DESTA_CHECK_ARG(width == 1 || (tail && tail_ld >= width), "logit_constraints: %d rows per sequence need the tail tokens", width);
    DESTA_CHECK_ARG(hist_len == 0 || (hist && hist_ld >= hist_len), "logit_constraints: bad token history");
    DESTA_CHECK_ARG(n_words <= CON_MAX_WORDS && n_word_ids <= CON_MAX_WORD_IDS, "logit_constraints: more than %d bad words or %d ids",
                    CON_MAX_WORDS, CON_MAX_WORD_IDS);
    DESTA_CHECK_ARG(n_words == 0 || (word_ids && word_off && n_word_ids >= n_words), "logit_constraints: bad word table");
    DESTA_CHECK_ARG(n_begin == 0 || begin_ids, "logit_constraints: begin ids missing");
    DESTA_CHECK_ARG(n_eos == 0 || eos_ids, "logit_constraints: EOS ids missing");
    DESTA_CHECK_ARG(id_max < cols, "logit_constraints: token id %d in a table, the rows have %d columns", id_max, cols);
    if (no_repeat_ngram == 0 && n_words == 0 && n_begin == 0 && (min_new_tokens == 0 || n_eos == 0)) return DESTA_OK;      // every rule off
    hipLaunchKernelGGL(logit_constraints_k, dim3(batch, width), dim3(CNT), 0, (hipStream_t)stream, (const bf16_t*)src, (long)ld_src,
                       (bf16_t*)dst, (long)ld_dst, width, cols, (const long*)hist, (long)hist_ld, hist_len, (const long*)tail, (long)tail_ld,
                       step0, no_repeat_ngram, word_ids, word_off, n_words, n_word_ids, begin_ids, n_begin, eos_ids, n_eos, min_new_tokens);
    DESTA_CHECK_LAUNCH("logit_constraints");
    return DESTA_OK;
}
