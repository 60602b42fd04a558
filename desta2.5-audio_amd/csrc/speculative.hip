// Draft-and-verify greedy decoding (gfx950): the two integer kernels around the verify pass of `CausalLMHIP.verify_step`.
// Reference call sites (TF: = transformers 5.15):
//   llm_model.generate(...) ........ modeling_desta25.py:1419 (inputs_embeds), :1703 (input_ids): the greedy loop these serve
//   prompt lookup .................. TF:generation/candidate_generator.py PromptLookupCandidateGenerator.get_candidates
//
// spec_ngram_draft_k: one 256-thread block per row.  The row's last n tokens are looked up in the row's own history, n from
//   n_max down to n_min; every thread walks the candidate starts i = tid, tid + 256, ... and keeps its largest hit, the block
//   takes the maximum through one LDS word.  The tokens behind the latest hit are the draft.
// spec_accept_k: one block.  Pass 1 finds, per row, the accepted run m_b and the first EOS inside it and reduces the lockstep
//   length a through one LDS word; pass 2 (the same rows on the same threads, the scan repeated: k <= 7 compares) writes the
//   emitted columns, the finished flags, the next input token and a.  Everything that reaches HBM is a plain C++ store.
#include <limits.h>
#include "common.h"
#include "desta_hip.h"

namespace {

constexpr int SPEC_NT = 256;
constexpr int SPEC_K_MAX = 7;
constexpr int SPEC_N_MAX = 4;

__global__ __launch_bounds__(SPEC_NT) void spec_ngram_draft_k(const int64_t* __restrict__ hist, int64_t ld, int hist_len,
                                                               const int32_t* __restrict__ row_start, int k, int n_max, int n_min,
                                                               int64_t* __restrict__ draft) {
    __shared__ int s_best;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t* h = hist + (int64_t)b * ld;
    const int start = row_start ? max(row_start[b], 0) : 0;
    int hit = -1, hit_n = 0;
    for (int n = n_max; n >= n_min; --n) {
        const int last = hist_len - 1 - n;                                  // largest start that leaves one token behind the match
        if (last < start) continue;                                         // (uniform over the block)
        int64_t suf[SPEC_N_MAX];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < SPEC_N_MAX; ++j) {
            suf[j] = j < n ? h[hist_len - n + j] : 0;
            ok = ok && suf[j] >= 0;                                         // negative ids (pads, audio placeholders) never match
        }
        if (!ok) continue;
        if (tid == 0) s_best = -1;
        __syncthreads();
        int best = -1;
        for (int i = start + tid; i <= last; i += SPEC_NT) {
            bool eq = true;
#pragma unroll
            for (int j = 0; j < SPEC_N_MAX; ++j) eq = eq && (j >= n || h[i + j] == suf[j]);
            if (eq) best = i;                                               // ascending walk: the last one kept is this thread's largest
        }
        if (best >= 0) atomicMax(&s_best, best);                            // LDS
        __syncthreads();
        const int got = s_best;
        __syncthreads();                                                    // s_best is reset by the next n
        if (got >= 0) {
            hit = got;
            hit_n = n;
            break;
        }
    }
    if (tid < k) {
        const int src = hit + hit_n + tid;
        draft[(int64_t)b * k + tid] = (hit >= 0 && src < hist_len) ? h[src] : (int64_t)-1;
    }
}

// m = accepted drafts of the row (leading j in 1..k with inp[j] >= 0 && inp[j] == pred[j - 1]); e = index of the first EOS among
// pred[0..m], -1 without one
__device__ __forceinline__ void spec_row_scan(const int64_t* __restrict__ pred, const int64_t* __restrict__ inp, int k,
                                              const int64_t* __restrict__ eos, int n_eos, int& m, int& e) {
    m = 0;
    while (m < k && inp[m + 1] >= 0 && inp[m + 1] == pred[m]) ++m;
    e = -1;
    for (int j = 0; j <= m && e < 0; ++j)
        for (int q = 0; q < n_eos; ++q)
            if (pred[j] == eos[q]) {
                e = j;
                break;
            }
}

__global__ __launch_bounds__(SPEC_NT) void spec_accept_k(const int64_t* __restrict__ pred, const int64_t* __restrict__ inp, int batch, int k,
                                                          uint8_t* __restrict__ finished, const int64_t* __restrict__ eos, int n_eos,
                                                          int64_t pad, int max_take, int64_t* __restrict__ out, int64_t ld_out, int n,
                                                          int64_t* __restrict__ next, int32_t* __restrict__ taken,
                                                          int64_t* __restrict__ hist, int64_t hist_ld, int hist_col) {
    __shared__ int s_a;
    const int tid = threadIdx.x, w = k + 1;
    if (tid == 0) s_a = max_take;
    __syncthreads();
    int lim = INT_MAX;
    for (int b = tid; b < batch; b += SPEC_NT) {
        if (finished[b]) continue;
        int m, e;
        spec_row_scan(pred + (int64_t)b * w, inp + (int64_t)b * w, k, eos, n_eos, m, e);
        if (e < 0) lim = min(lim, m + 1);                                   // a row that meets an EOS inside its run limits nobody
    }
    if (lim != INT_MAX) atomicMin(&s_a, lim);                               // LDS
    __syncthreads();
    const int a = s_a;                                                      // >= 1: max_take >= 1 and every m + 1 >= 1
    for (int b = tid; b < batch; b += SPEC_NT) {
        const bool was = finished[b] != 0;
        int m = 0, e = -1;
        if (!was) spec_row_scan(pred + (int64_t)b * w, inp + (int64_t)b * w, k, eos, n_eos, m, e);
        int64_t v = pad;
        for (int j = 0; j < a; ++j) {                                       // j <= m on an unfinished row without an EOS in front of j
            v = (was || (e >= 0 && j > e)) ? pad : pred[(int64_t)b * w + j];
            out[(int64_t)b * ld_out + n + j] = v;
            if (hist) hist[(int64_t)b * hist_ld + hist_col + j] = v;
        }
        next[b] = v;
        if (!was && e >= 0 && e < a) finished[b] = 1;
    }
    if (tid == 0) taken[0] = a;
}

}  // namespace

extern "C" int desta_spec_ngram_draft(const int64_t* hist, int64_t hist_ld, int batch, int hist_len, const int32_t* row_start, int k,
                                      int n_max, int n_min, int64_t* draft, void* stream) {
    DESTA_CHECK_ARG(hist && draft, "spec_ngram_draft: null history or draft");
    DESTA_CHECK_ARG(batch >= 1, "spec_ngram_draft: batch %d must be positive", batch);
    DESTA_CHECK_ARG(k >= 1 && k <= SPEC_K_MAX, "spec_ngram_draft: k %d out of range (1..%d)", k, SPEC_K_MAX);
    DESTA_CHECK_ARG(1 <= n_min && n_min <= n_max && n_max <= SPEC_N_MAX, "spec_ngram_draft: n-gram sizes %d..%d out of range (1 <= n_min <= n_max <= %d)",
                    n_min, n_max, SPEC_N_MAX);
    DESTA_CHECK_ARG(hist_len >= 1 && (int64_t)hist_len <= hist_ld, "spec_ngram_draft: hist_len %d out of range (1..hist_ld = %lld)", hist_len,
                    (long long)hist_ld);
    hipLaunchKernelGGL(spec_ngram_draft_k, dim3(batch), dim3(SPEC_NT), 0, (hipStream_t)stream, hist, hist_ld, hist_len, row_start, k, n_max, n_min,
                       draft);
    DESTA_CHECK_LAUNCH("spec_ngram_draft");
    return DESTA_OK;
}

extern "C" int desta_spec_accept(const int64_t* pred, const int64_t* inp, int batch, int k, uint8_t* finished, const int64_t* eos, int n_eos,
                                 int64_t pad, int max_take, int64_t* out, int64_t ld_out, int n, int64_t* next, int32_t* taken, int64_t* hist,
                                 int64_t hist_ld, int hist_col, void* stream) {
    DESTA_CHECK_ARG(pred && inp && finished && out && next && taken, "spec_accept: null pointer");
    DESTA_CHECK_ARG(batch >= 1, "spec_accept: batch %d must be positive", batch);
    DESTA_CHECK_ARG(k >= 1 && k <= SPEC_K_MAX, "spec_accept: k %d out of range (1..%d)", k, SPEC_K_MAX);
    DESTA_CHECK_ARG(n_eos >= 0 && (n_eos == 0 || eos), "spec_accept: eos list of %d ids needs a pointer", n_eos);
    DESTA_CHECK_ARG(max_take >= 1, "spec_accept: max_take %d must be at least 1", max_take);
    DESTA_CHECK_ARG(n >= 0 && (int64_t)n + max_take <= ld_out, "spec_accept: columns [%d, %d + max_take %d) leave the row of %lld", n, n, max_take,
                    (long long)ld_out);
    DESTA_CHECK_ARG(!hist || (hist_col >= 0 && (int64_t)hist_col + max_take <= hist_ld),
                    "spec_accept: history columns [%d, %d + max_take %d) leave the row of %lld", hist_col, hist_col, max_take, (long long)hist_ld);
    hipLaunchKernelGGL(spec_accept_k, dim3(1), dim3(SPEC_NT), 0, (hipStream_t)stream, pred, inp, batch, k, finished, eos, n_eos, pad, max_take, out,
                       ld_out, n, next, taken, hist, hist_ld, hist_col);
    DESTA_CHECK_LAUNCH("spec_accept");
    return DESTA_OK;
}
