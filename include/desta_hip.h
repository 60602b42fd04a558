/* libdesta_hip.so — C ABI of the MI355X-native DeSTA2.5-Audio training hot path.
 *
 * The reference (voidful/DeSTA2.5-Audio) has no FFI boundary of its own: every FLOP of
 * `DeSTA25AudioModel.forward` + HF-Trainer backward/clip/Adafactor runs inside torch / transformers
 * calls.  This header is the boundary the build defines underneath the reference's Python surface
 * (SURVEY.md §8b): each entry point names the reference call site(s) (file:line, `TF:` =
 * transformers 5.15) whose arithmetic it replaces.  `INTEGRATION.md` shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, raw DEVICE pointers + explicit sizes; no torch / HIP types in signatures;
 *     `stream` is a `hipStream_t` passed as `void*` (0 = default stream);
 *   - every call only ENQUEUES work on `stream` (no allocation, no host sync: graph-capturable);
 *   - return value: 0 = ok, <0 = error (DESTA_EINVAL -1, DESTA_ELAUNCH -2); nothing throws across
 *     the ABI; `desta_last_error()` returns a thread-local message for the last failure;
 *   - state: the data path has none besides what the caller passes in (buffers, descriptors, plans, stream).  The only
 *     process-wide variables are (a) the thread-local error text, (b) TUNING / DIAGNOSTIC switches for A/B runs
 *     (`desta_gemm_set_option`, `desta_gemm_force_variant`, `desta_attention_set_concurrent_bwd`,
 *     `desta_gemm_last_kernel`): defaults are what every test and benchmark runs, a data path never needs to touch them,
 *     and they are not synchronised (set them before launching work from several threads, or not at all), and (c) one
 *     internal side stream + two events per DEVICE for the attention backward's dQ / dK,dV fork (created on first use,
 *     joined before the call returns to the caller's stream);
 *   - caller owns every buffer including workspaces (`*_workspace_bytes` helpers say how much);
 *   - bf16 tensors are `uint16_t` bit patterns; "rows" are always the slow index, row-major.
 */
#ifndef DESTA_HIP_H
#define DESTA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DESTA_ABI_VERSION 8

int desta_abi_version(void);
/* sizeof of the descriptor structs as this library was compiled (0 = desta_gemm_desc, 1 = desta_attn_desc,
 * 2 = desta_opt_plan, 3 = desta_adamw_plan): a binding checks its own struct layouts against these before the first call. */
size_t desta_sizeof_desc(int which);
const char* desta_last_error(void);

/* Optional per-device context.  No data-path call takes it: the path is stateless (see "state" above).  What
 * it owns is item (c) of that list, which the library otherwise makes at first use and keeps until the process ends:
 * `desta_create` checks that `device` is a gfx950 part (the only code objects in the library), makes it current and creates
 * the internal stream / events up front (so a later hipGraph capture never meets a stream creation); `desta_destroy`
 * drains and releases them.  `desta_handle_last_error` = `desta_last_error()` of the calling thread, copied into the handle. */
typedef struct desta_context* desta_handle;
int desta_create(int device, desta_handle* out);
int desta_destroy(desta_handle h);
int desta_handle_info(desta_handle h, int* device, int* compute_units, char* arch, size_t arch_bytes);
const char* desta_handle_last_error(desta_handle h);

/* ------------------------------------------------------------------------------------------
 * Dense contraction  C[M,N] = epi(alpha * A[M,K] · B[N,K]^T)   (bf16 in, fp32 accumulate, MFMA)
 *   epi(v) = act(v + bias[n]) + residual[m,n];  optional copy of (v + bias) before act -> preact.
 *   `batch` > 1 runs independent problems offset by the stride_* fields (stride 0 = shared).
 *   Rows of A may overlap (lda < K): used for the zero-copy im2col of the Whisper conv stem.
 * Replaces every nn.Linear / nn.Conv1d matmul (+ bias, GELU, residual add) on the path:
 *   modeling_desta25.py:563-564 (conv1/conv2+gelu), :606 (proj);
 *   TF:models/whisper/modeling_whisper.py:279-330,379-413; TF:models/bert/modeling_bert.py:354-416;
 *   TF:models/llama/modeling_llama.py:163-176,230-281,480 (q/k/v/o, gate/up/down, lm_head);
 *   and their autograd backward (dX: B = transposed weight copy; dW: A = dY^T, B = X^T).
 * Requirements: K % 64 == 0, N % 4 == 0, lda/ldb % 8 == 0, 16-byte aligned bases. */
typedef struct desta_gemm_desc {
    const void* A; const void* B; void* C;
    int M, N, K, batch;
    int64_t lda, ldb, ldc;
    int64_t stride_a, stride_b, stride_c;
    const float* bias;                 /* [N] fp32 or NULL */
    const void* residual;              /* [M,N] bf16 or fp32, or NULL */
    int64_t ldr, stride_r;
    int residual_f32;
    int act;                           /* 0 = none, 1 = GELU(erf), 2 = SwiGLU fwd, 3 = SwiGLU bwd (see aux),   */
                                       /* 4 = decode SwiGLU (M <= 16): B = [2N,K] gate rows then up rows,      */
                                       /*     C[M,N] (bf16) = silu(gate) * up                                   */
    int out_f32;                       /* C dtype: 0 = bf16, 1 = fp32 */
    void* preact;                      /* optional bf16 [M,N] */
    int64_t ldp, stride_p;
    float alpha;
    void* aux;                         /* act 2 / act 3: fused SwiGLU over the BLOCKED gate|up layout (ABI 6): 64-column  */
    int64_t ld_aux;                    /*   block b of the projection = gate_{32b..32b+31} | up_{32b..32b+31} (weight rows    */
                                       /*   permuted once at load; N % 64 == 0).  act 2 (forward): C[M,N] keeps the bf16      */
                                       /*   projection, aux[M,N/2] (bf16, out) = silu(gate) * up in plain column order.       */
                                       /* act 3 (backward): v = d(act)[M,N] in plain column order, aux[M,2N] (bf16, in) = the */
                                       /*   saved blocked gate|up, C[M,2N] (bf16, ldc = row length) = d(gate|up), blocked.    */
                                       /*   Replaces TF:models/llama/modeling_llama.py:163-176 (LlamaMLP act_fn(gate) * up)   */
                                       /*   and its autograd; same rounding points as desta_swiglu_fwd / _bwd.                */
    float dropout_p;                   /* > 0: inverted dropout of act(acc+bias) BEFORE the residual add, mask = desta_dropout_mask(seed, */
    uint64_t dropout_seed;             /*   (z*M + m)*N + n), z = batch item (BertSelfOutput/BertOutput, p=0.1) */
    void* workspace;                   /* optional fp32 scratch for the split-K tail (NULL = never split);   */
    size_t workspace_bytes;            /* 64 MiB + 4 KiB covers every shape (<= 256 slabs of 256x256 fp32);   */
                                       /* its LAST 4 KiB hold the arrival tickets of the in-kernel K-slice    */
                                       /* reduction (first 1 KiB) and the tile-queue counters of the          */
                                       /* persistent 256x256 kernel (last 64 B): hand the workspace over      */
                                       /* ZEROED once and then leave it alone (both reset themselves after    */
                                       /* every launch); one workspace per stream (two concurrent GEMMs must  */
                                       /* not share it)                                                        */
    int trans_a, trans_b;              /* != 0: the operand is stored transposed, A as [K,M] (lda = row stride), B as   */
                                       /*   [K,N]: autograd's dW = dY^T X (both) and dX = dY W (trans_b) without a        */
                                       /*   materialised transpose; M resp. N must be a multiple of 8                     */
    const float* a_rms_weight;         /* decode path (M <= 16, M*2K <= 65536 B, act 0 or 4): A holds the  */
    float a_rms_eps;                   /*   un-normalised rows; RMSNorm(A; weight, eps) is applied on the fly   */
                                       /*   (LlamaRMSNorm fused into the projection that consumes it). NULL = off */
    /* (ABI 4) rotary embedding in the epilogue of the fused q|k|v projection (apply_rotary_pos_emb,                  */
    /* TF:models/llama/modeling_llama.py:120-160): output columns [0, rope_cols) are rotated in ADJACENT PAIRS          */
    /* (2i, 2i+1) of each rope_head_dim-wide head by the angle of (position rope_pos[m], frequency i):                  */
    /*   y[2i] = x[2i] c - x[2i+1] s,  y[2i+1] = x[2i+1] c + x[2i] s,  (c, s) = rope_cos_sin[(pos * hd/2 + i) * 2 ..].    */
    /* HF pairs column i with i + hd/2 (rotate_half); the caller stores the frozen q / k weight rows of every head in   */
    /* the order 0, hd/2, 1, hd/2 + 1, ... so that the pair is adjacent — q.k is invariant under a permutation of the    */
    /* head dimension applied to both.  The fp32 accumulator is rotated and rounded ONCE (the reference rounds the      */
    /* projection to bf16, rotates, rounds again).  NULL = off.  Needs act 0, no bias / residual / dropout, bf16 output. */
    const float* rope_cos_sin;         /* [positions][rope_head_dim / 2][2] fp32 */
    const int32_t* rope_pos;           /* [M] position of every output row */
    int rope_cols, rope_head_dim;
} desta_gemm_desc;
int desta_gemm_bf16_nt(const desta_gemm_desc* d, void* stream);
/* tuning / tests only: 0 = automatic tile choice, 1 = force 128x128, 2 / 3 = force the 256x256 kernel with the lockstep /
 * staggered four-phase schedule, 6 / 7 = staggered / lockstep two-phase schedule, 4 / 8 = the persistent tile-queue kernel
 * (staggered two-phase; batch 1 with a workspace, else variant 6) */
int desta_gemm_force_variant(int variant);
/* kernel family the most recent desta_gemm_bf16_nt call launched: 1 = 128x128, 2 = 256x256 (+ split-K fix-up), 3 = skinny
 * (bench.py attributes its HIP-event timings to the dominant kernel with this) */
int desta_gemm_last_kernel(void);
/* What desta_gemm_bf16_nt launches for `d` under the current options and force variant, without launching anything (host
 * arithmetic only: no device needed; of the descriptor it reads the shape, batch, act, trans_*, workspace and workspace_bytes).
 * d == NULL: the plan of the most recent desta_gemm_bf16_nt call. */
typedef struct desta_gemm_plan {
    int kernel;          /* 1 = 128x128, 2 = 256x256 one tile per block, 3 = skinny, 4 = 256x256 persistent tile queue */
    int split;           /* K-slices per tail tile (1 = no split-K tail) */
    int full_tiles;      /* whole tiles in front of the tail (256x256 kernels) */
    int items;           /* work items of the main launch: whole tiles + K-slices */
    int slices_first;    /* tile queue: the K-slices precede the whole tiles in every queue (option 12) */
    int inkernel;        /* one tile per block: slabs reduced inside the launch (option 5) */
    int fixup_launch;    /* a gemm_splitk_fixup launch follows */
} desta_gemm_plan;
int desta_gemm_plan_query(const desta_gemm_desc* d, desta_gemm_plan* out);
int desta_gemm_set_persistent(int on);   /* = desta_gemm_set_option(0, on) */
/* A/B switches of the automatic choice: option 0 = persistent tile-queue 256x256 kernel (0 never; 1, default: batch 1, a workspace
 * and more than 256 tiles, with a split-K tail or without; 2: every such grid of more than 256 work items), 1 = staggered, 2 = skinny (M <= 16) kernel variant
 * (0 auto, else COLS*10 + U: 162 164 322 641), 3 = persistent grid size of the skinny kernel (default 512 = 2 blocks per CU),
 * 4 = two-phase schedule of the 256x256 kernel (default 1; 0 = the four-phase schedule), 5 = K-slices of tail tiles reduced inside
 * the GEMM launch instead of by the fix-up launch (default 0), 6 = four-slot software-pipelined ring form of the 128x128 kernel:
 * 0 never, 1 (default) when the grid leaves one block per CU (<= 256 tiles), 2 always; 10 = the two-phase 256x256 kernel stops its
 * half-tile stream at the last K-tile (default 1; 0 = re-load dead slots as rounds 1-3 did); bit-identical results in every setting.
 * 11 = pipeline depth of the weight-only FP8 skinny kernel (0 auto, else 162 / 164; act 0 only; same bits either way).
 * Split-K tails on the tile queue: 12 = the K-slices run in front of a queue's whole tiles (default 0: behind them); same bits
 * either way.  14 = grids that CAN take the tile queue (batch 1, a workspace, more than 256 tiles) cut their tail into slices of
 * >= 8 K-tiles instead of >= 16, whichever kernel then runs them (default 0; another split adds the slices in another order, so
 * this one changes low-order bits).  Option 13 (round 27's reduce inside the queue launch, measured slower) returns DESTA_EINVAL.
 * Options 7, 8 (round 3's de-synchronised start) and 9 (round 4's polynomial GELU) were removed and return DESTA_EINVAL. */
int desta_gemm_set_option(int option, int value);

/* ------------------------------------------------------------------------------------------
 * Weight-only FP8 (W8A16) decode: the frozen LLM weights a second time as OCP e4m3fn bytes with one power-of-two fp32
 * scale per output row, streamed by the projections of a KV-cached decode step (additive to ABI 8: no struct changes).
 * Serves llm_model.generate, modeling_desta25.py:1419-1427 (the nn.Linear calls of
 * TF:models/llama/modeling_llama.py:163-176 (MLP), 230-281 (attention projections), 480 (lm_head)) when the caller opts in;
 * the default path keeps the bf16 weights.
 *
 * desta_quantize_rows_e4m3: w [rows, cols] bf16 (row stride ld elements) -> q [rows, cols] e4m3fn bytes (contiguous) and
 *   scale [rows].  scale = 2^e with e the smallest integer such that amax(row) * 2^-e <= 448; an all-zero row gets 1.
 *   q = e4m3fn(w / scale), round to nearest even (OCP encoding, not the MI300 fnuz one; nothing saturates by construction).
 *   q * scale is exactly representable in bf16.
 * desta_gemm_w8a16_nt: C[M,N] = epilogue( b_scale[n] * (A[M,K] . e4m3(B)[N,K]^T) ) for M <= 16, batch 1.  The descriptor is
 *   desta_gemm_desc unchanged: B points at e4m3 bytes [N, K] ([2N, K] for act 4), ldb counts elements (= bytes, a multiple
 *   of 16), b_scale [N] ([2N] for act 4: gate and up rows carry their own scales) fp32, 16-byte aligned.  Supported: act 0 and 4, residual, ldc,
 *   a_rms_weight / a_rms_eps, alpha, fp32 or bf16 output; anything else returns DESTA_EINVAL.  e4m3 -> bf16 in registers
 *   (exact), the bf16 skinny kernel's MFMA accumulation in the same K order, the row scale on the fp32 sum before any
 *   rounding or activation: bit-identical to desta_gemm_bf16_nt on the dequantised weight bf16(q * scale). */
int desta_quantize_rows_e4m3(const void* w_bf16, int rows, int cols, int64_t ld, uint8_t* q, float* scale, void* stream);
int desta_gemm_w8a16_nt(const desta_gemm_desc* d, const float* b_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight-only MXFP4 (W4A16) decode: the frozen LLM weights a second time as OCP e2m1 nibbles with one e8m0 scale per 32
 * consecutive k, streamed by the projections of a KV-cached decode step (additive to ABI 8: no struct changes).
 * Serves llm_model.generate, modeling_desta25.py:1419-1427 (the nn.Linear calls of
 * TF:models/llama/modeling_llama.py:163-176 (MLP), 230-281 (attention projections), 480 (lm_head)) when the caller opts in;
 * the default path keeps the bf16 weights.
 *
 * Format.  q [rows, K/2] bytes, row stride ldq bytes (a multiple of 16): byte j of a row holds element k = 2j in bits 3..0 and
 *   k = 2j + 1 in bits 7..4.  A code is e2m1: bit 3 the sign, codes 0..7 the magnitudes 0 0.5 1 1.5 2 3 4 6.
 *   s [rows, K/32] bytes, row stride lds bytes: e8m0, byte b = 2^(b - 127), one per block of 32 consecutive k; 255 is never written.
 * desta_quantize_rows_mxfp4: w [rows, cols] bf16 (row stride ld elements, a multiple of 8; cols a multiple of 32) -> q, s.  Per block
 *   e is the smallest integer with amax * 2^-e <= 7 (from the bits of amax; an all-zero block gets byte 127), elements are
 *   w * 2^-e rounded to the nearest grid value, ties to the even code, the magnitude saturating at 6 ((6, 7] -> 6).  Covered:
 *   blocks with amax = 0 or 2^-100 <= amax < 2^100.  code * 2^e is exactly a bf16 value.  Nothing behind `cols` of a row is read.
 * desta_gemm_w4a16_nt: C[M,N] = epilogue( A[M,K] . dequant(B, b_scale_e8m0)[N,K]^T ) for 1 <= M <= 64, batch 1, K % 64 == 0.
 *   d->B points at the nibbles [N, K/2] ([2N, K/2] for act 4) and d->ldb counts BYTES (a multiple of 16); b_scale_e8m0 [N, K/32]
 *   ([2N, ..] for act 4) with row stride ld_scale bytes.  Supported: act 0 and 4 (SwiGLU over concatenated gate|up rows), bf16 or
 *   fp32 output, ldc, a bf16 residual, alpha, and for M <= 16 a_rms_weight / a_rms_eps under the conditions of
 *   desta_gemm_bf16_nt; anything else returns DESTA_EINVAL.  Nibbles become bf16 in registers (exact) and feed the bf16 MFMA
 *   with fp32 accumulation in a fixed order that depends on N and K only: results do not depend on the grid
 *   (desta_gemm_set_option 3) or on M.  The K order is NOT that of desta_gemm_bf16_nt (128-element chunks, one scale block per
 *   lane), so the result is held to the fp64 bound of the operation, not to bit-equality with the bf16 form.  Shapes with few
 *   64-column tiles are cut into K-slices through desta_gemm_desc.workspace (slices * M * N * 4 bytes, 2N for act 4, plus 4096;
 *   too small: DESTA_EINVAL) and the fix-up launch of desta_gemm_wide_nt. */
int desta_quantize_rows_mxfp4(const void* w_bf16, int rows, int cols, int64_t ld, uint8_t* q, int64_t ldq, uint8_t* scale_e8m0, int64_t lds, void* stream);
int desta_gemm_w4a16_nt(const desta_gemm_desc* d, const uint8_t* b_scale_e8m0, int64_t ld_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Decode at batch 17..64: the projections of a KV-cached decode step (llm_model.generate, modeling_desta25.py:1419-1427; the
 * nn.Linear calls of TF:models/llama/modeling_llama.py:163-176 (MLP), 230-281 (attention projections), 480 (lm_head)) as one
 * weight-streaming launch that reads every weight byte once for up to 64 rows (additive to ABI 8: no struct changes).
 *
 * desta_gemm_wide_nt: C[M,N] = epilogue( A[M,K] . B[N,K]^T ) for 17 <= M <= 64, batch 1; M outside that range returns
 *   DESTA_EINVAL (M <= 16 is desta_gemm_bf16_nt / desta_gemm_w8a16_nt).  b_scale == NULL: B is bf16.  Otherwise B holds e4m3
 *   bytes [N, K] ([2N, K] for act 4; ldb in elements = bytes, a multiple of 16) and b_scale one power-of-two fp32 scale per row
 *   ([2N] for act 4), 16-byte aligned; the result is bit-identical to the bf16 form on the dequantised weight.  Supported: act 0
 *   with an optional bf16 residual, act 4 (SwiGLU over concatenated gate|up rows, the rounding points of the 16-row kernel), alpha,
 *   ldc, bf16 output; anything else (bias, GELU, preact, aux, dropout, transposed operands, rotary epilogue, out_f32, batch > 1,
 *   a_rms_weight) returns DESTA_EINVAL.  Shapes with few 64-column tiles are cut into K-slices whose fp32 partial sums go
 *   through desta_gemm_desc.workspace (slices * M * N * 4 bytes, 2N for act 4, plus 4096; too small: DESTA_EINVAL) and a
 *   fix-up launch that adds them in slice order: results do not depend on the grid (desta_gemm_set_option 3) or on M. */
int desta_gemm_wide_nt(const desta_gemm_desc* d, const float* b_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Decode at 65..256 rows: the same projections as one weight-streaming launch for up to 256 rows (additive to ABI 8: no struct
 * changes).
 *
 * desta_gemm_tall_nt: C[M,N] = epilogue( A[M,K] . B[N,K]^T ) for 65 <= M <= 256, batch 1; M outside that range returns
 *   DESTA_EINVAL (17 <= M <= 64 is desta_gemm_wide_nt).  Operands, b_scale, the supported and the rejected features, the K-slice
 *   workspace (slices * M * N * 4 bytes, 2N for act 4, plus 4096: at most 24 MB on the Llama-3.1-8B shapes) and the fix-up launch
 *   are those of desta_gemm_wide_nt.  Every weight byte is requested from HBM once for all M rows.  The e4m3 form is bit-identical
 *   to the bf16 form on the dequantised weight, act 4 to act 0 on the 2N-row weight followed by SwiGLU.  The summation order of an
 *   output element depends on N, K and on the row-group count alone: 2 groups for 65 <= M <= 128, 4 for 129 <= M <= 256.  Inside
 *   one class a row's result does not depend on M, on the row's position or on the grid (desta_gemm_set_option 3); across the
 *   classes, and against desta_gemm_wide_nt, results differ in the last bits. */
int desta_gemm_tall_nt(const desta_gemm_desc* d, const float* b_scale, void* stream);

/* ------------------------------------------------------------------------------------------
 * Global-norm clip + Adafactor over a flat fp32 arena.
 * Replaces `clip_grad_norm_(params, max_grad_norm)` (TF:trainer.py:1780-1782) followed by
 * `Adafactor.step` (TF:optimization.py:1203-1294; scale_parameter=False, relative_step=False,
 * beta1=None, eps=(eps1,.), clip_threshold, decay_rate folded into beta2t = 1 - step^decay_rate by
 * the caller).  `params`/`grads` are the arena; tensors >= 2-D are factored over their last two
 * dims (leading dims = `batch`), 1-D tensors keep a full second-moment vector.  All tables are
 * DEVICE arrays built once by the caller:
 *   tensors  int64 [n_tensors][8] : arena offset, batch, rows, cols, row_state_off, col_state_off,
 *                                   first unit, number of units   (offsets in floats, multiples of 4)
 *   units    int32 [n_units][4]   : tensor index, batch index, first row, number of rows (64 on the chunk path; any count for a
 *                                   tensor with ragged rows, ABI 7)
 *   unit_col_off int64 [n_units]  : offset of the unit's column partial sums in the workspace
 *   vecs     int64 [n_vec][3]     : arena offset, length, state offset
 * `state` (state_floats floats) holds exp_avg_sq_row / exp_avg_sq_col / exp_avg_sq.  workspace
 * (desta_adafactor_workspace_floats floats): [0] = pre-clip global grad norm, [1] = clip coefficient
 * after the call. */
typedef struct desta_opt_plan {
    const int64_t* tensors; const float* tensor_wd; int n_tensors;
    const int32_t* units; const int64_t* unit_col_off; int n_units;
    const int64_t* vecs; const float* vec_wd; int n_vec;
    int64_t state_floats;            /* length of `state`: the row / column factors of the workspace are indexed by state offsets */
    int max_cols;
    /* ABI 3: work items of the update kernels and of the factor kernel.
     * chunks [n_chunks][4] = (tensor, batch index, first element inside the [rows, cols] matrix, count <= 16384), the chunks of
     * one tensor contiguous, tensors in DESCENDING arena order (the update passes walk the arena backwards, from the end the
     * statistics pass has just streamed through the Infinity Cache); ten_chunks [n_tensors][2] = (first chunk, chunk count);
     * fin [n_fin][3] = (tensor, batch index, part): part 0 = the row factors, k >= 1 = columns [256 (k-1), 256 k);
     * group_bounds: HOST array [n_groups + 1] of chunk indices cutting the chunk list at tensor boundaries into groups of
     * <= 64 MB of gradients (the re-read of a group's gradients is then served by the Infinity Cache).  Every tensor with
     * chunks has cols % 4 == 0 (16-B row accesses in the chunk kernels). */
    const int32_t* chunks; const int32_t* ten_chunks; int n_chunks;
    const int32_t* fin; int n_fin;
    int64_t colpart_floats;          /* column partial sums of all units (unit_col_off indexes into them) */
    const int32_t* group_bounds; int n_groups;
    /* ABI 7: factored tensors with ragged rows (cols % 4 != 0, e.g. a Conv1d weight [out, in, 5]) carry NO chunks
     * (ten_chunks = (0, 0)) and are updated by the unit-based kernels: ragged_units = HOST array [n_ragged][2] of
     * (first unit, unit count), one entry per such tensor. */
    const int32_t* ragged_units; int n_ragged;
} desta_opt_plan;
size_t desta_adafactor_workspace_floats(const desta_opt_plan* plan);
int desta_clip_adafactor_step(const desta_opt_plan* plan, float* params, const float* grads, float* state,
                              float* workspace, float lr, float beta2t, float eps1, float clip_threshold,
                              float max_grad_norm, void* stream);

/* ------------------------------------------------------------------------------------------
 * Global-norm clip + AdamW over the same flat fp32 arena (optim="adamw_torch" / "adamw_torch_fused").
 * Replaces `clip_grad_norm_(params, max_grad_norm)` (TF:trainer.py:1780-1782) followed by
 * `torch.optim.AdamW(lr, betas=(adam_beta1, adam_beta2), eps=adam_epsilon).step` over the two weight-decay groups
 * (TF:trainer_optimizer.py:201-208), per element in torch's order:
 *   g = grad * coef;  p *= 1 - lr wd;  m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2;
 *   p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 * with coef = min(1, max_grad_norm / (||grads|| + 1e-6)) (1 when max_grad_norm <= 0) and bc1 = 1 - beta1^t,
 * bc2 = 1 - beta2^t computed by the caller from its own step count t.  beta1 / beta2 are doubles: 1 - beta is formed in
 * double before the fp32 arithmetic, as torch forms it from its Python-float arguments.
 *   items   DEVICE int64 [n_items][2] : arena offset, count (both multiples of 4; count <= DESTA_ADAMW_ITEM_FLOATS), every
 *                                       item inside one tensor, ascending arena order (the update pass walks the table
 *                                       BACKWARDS, from the end the norm pass has just streamed through the Infinity Cache)
 *   item_wd DEVICE float [n_items]    : the item's tensor's weight decay (0 for the no-decay group)
 *   numel   floats in the arena (multiple of 4); padding between tensors must hold zeros in every buffer and stays zero.
 * `grads` is read only; exp_avg / exp_avg_sq are two arena-sized fp32 buffers.  Two launches, no float atomics (bitwise
 * deterministic).  workspace (desta_adamw_workspace_floats floats): [0] = pre-clip global grad norm, [1] = clip coefficient
 * after the call. */
#define DESTA_ADAMW_ITEM_FLOATS 4096
typedef struct desta_adamw_plan {
    const int64_t* items; const float* item_wd; int n_items;
    int64_t numel;
} desta_adamw_plan;
size_t desta_adamw_workspace_floats(const desta_adamw_plan* plan);
int desta_clip_adamw_step(const desta_adamw_plan* plan, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                          float* workspace, float lr, double beta1, double beta2, float eps, float bc1, float bc2,
                          float max_grad_norm, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whisper log-mel front end: wave [batch, n_samples] f32 (row stride wave_stride) ->
 * out [batch, n_mels, 3000] f32.  Replaces WhisperFeatureExtractor.__call__ at
 * desta/trainer/data/simple_dataset.py:239-243 and modeling_desta25.py:1570
 * (TF:models/whisper/feature_extraction_whisper.py:135-168, TF:audio_utils.py:638-729).
 * `tables` = device copy of the buffer desta_logmel_fill_tables() writes on the host
 * (hann window | cos | sin | slaney filter bank [201][n_mels] | non-zero DFT-bin range [n_mels][2] of every filter: an opaque
 * blob of desta_logmel_table_floats(n_mels) floats); workspace: batch*94 floats. */
size_t desta_logmel_table_floats(int n_mels);
size_t desta_logmel_workspace_floats(int batch);
int desta_logmel_fill_tables(int n_mels, float* host_out);
int desta_logmel_f32(const float* wave, int batch, int n_samples, int64_t wave_stride, const float* tables,
                     int n_mels, float* out, float* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Row-wise normalisation.  One wave per row, fp32 statistics, 16-byte accesses; cols % 8 == 0.
 * LayerNorm: nn.LayerNorm at TF:models/whisper/modeling_whisper.py:392,402 (eps 1e-5),
 *   TF:models/bert/modeling_bert.py:296,350 (eps 1e-12), modeling_desta25.py:166; x is fp32 or bf16,
 *   outputs bf16 and/or fp32; stats [rows][2] = (mean, rstd) saved for backward.
 * layernorm_bwd: dx (fp32 and/or bf16) and dgamma/dbeta (written, or added when accumulate != 0);
 *   cols <= 4096; workspace from desta_layernorm_bwd_workspace_floats.
 * RMSNorm: LlamaRMSNorm TF:models/llama/modeling_llama.py:53-67 (bf16 in/out, fp32 weight copy);
 *   rmsnorm_bwd returns dx = dres + d(norm) (dres may be NULL), frozen weight (no dweight). */
int desta_layernorm_fwd(const void* x, int x_f32, const float* gamma, const float* beta, float eps, int rows,
                        int cols, void* y_bf16, float* y_f32, float* stats, void* stream);
size_t desta_layernorm_bwd_workspace_floats(int rows, int cols);
int desta_layernorm_bwd(const void* dy, int dy_f32, const void* x, int x_f32, const float* gamma,
                        const float* stats, int rows, int cols, float* dx_f32, void* dx_bf16, float* dgamma,
                        float* dbeta, int accumulate, float* workspace, void* stream);
int desta_rmsnorm_fwd(const void* x, const float* weight, float eps, int rows, int cols, void* y, float* rstd,
                      void* stream);
int desta_rmsnorm_bwd(const void* dy, const void* x, const float* weight, const float* rstd, const void* dres,
                      int rows, int cols, void* dx, void* stream);

/* Column sums of a bf16 [rows, cols] matrix (bias gradients of nn.Linear), fixed-order two-stage. */
size_t desta_colsum_workspace_floats(int rows, int cols);
int desta_colsum_bf16(const void* x, int rows, int cols, int64_t ld, float* out, int accumulate,
                      float* workspace, void* stream);

/* Rotary embedding applied IN PLACE to the first (n_q_heads + n_kv_heads) heads of a fused
 * [rows, ld] bf16 q|k|v buffer; position = row % seq (position_ids = arange(S) for every row,
 * TF:models/llama/modeling_llama.py:386-389); cos_sin = fp32 [seq][2][head_dim/2].
 * With q_norm_w/k_norm_w != NULL the Qwen3 per-head RMSNorm (TF:models/qwen3/modeling_qwen3.py:237-257)
 * runs first (forward) / is differentiated (backward, needs the saved pre-norm q|k in pre_norm).
 * backward != 0 applies the transposed rotation to gradients. head_dim 64 or 128.
 * pos_shift (int32 [rows/seq] or NULL): position = max(0, row % seq + pos_shift[row / seq]) — generate() derives
 * position_ids from the attention mask (prompt: -left_pad; decode step: cache_len - left_pad).
 * s_major_batch > 0: the token grid is stored position-major (row = s * s_major_batch + b) instead of batch-major
 * (row = b * seq + s) — the training layout, in which "all positions >= s0" is one contiguous row range.
 * The six rotary entry points (this one, desta_rope_kv_append, desta_rope_kv_append_e4m3 and their _bias forms) share one
 * argument check; a call that fails it returns DESTA_EINVAL and launches nothing.  All six: buf and cos_sin 16-byte aligned
 * (desta_rope checked neither before: an unaligned buf or cos_sin is newly rejected), ld a multiple of 8, q_norm_w and
 * k_norm_w both or neither (desta_rope took a lone k_norm_w and ignored it: newly rejected).  ld need not hold the V heads
 * here, which this form never touches. */
int desta_rope(void* buf, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
               const float* cos_sin, const float* q_norm_w, const float* k_norm_w, float eps,
               const void* pre_norm, int64_t ld_pre, int backward, const int32_t* pos_shift, int s_major_batch, void* stream);

/* SwiGLU on a fused [rows, 2*inter] gate|up buffer (LlamaMLP, TF:models/llama/modeling_llama.py:163-176),
 * GELU'(erf) for the Q-Former FFN backward, and small layout helpers. */
int desta_swiglu_fwd(const void* gate_up, void* act, int64_t rows, int inter, void* stream);
int desta_swiglu_bwd(const void* gate_up, const void* dact, void* dgate_up, int64_t rows, int inter, void* stream);
int desta_gelu_bwd(const void* preact, const void* dact, void* dpre, int64_t n, void* stream);
int desta_cast_f32_bf16(const float* x, void* y, int64_t n, void* stream);
int desta_add_f32(float* y, const float* x, int64_t n, void* stream);
/* out[c][r] = in[r][c] as bf16; out row length ld_out >= rows, tail zero-filled (K padding for dW GEMMs) */
int desta_transpose_to_bf16(const void* in, int in_f32, int64_t ld_in, int rows, int cols, void* out,
                            int64_t ld_out, void* stream);
/* mel [B, n_mels, T] fp32 -> channel-last rows [B, T+2, c_pad] bf16 (rows 0 and T+1 stay as the caller
 * zeroed them): the A operand of the zero-copy im2col conv1 GEMM (modeling_desta25.py:563). */
int desta_mel_to_rows(const float* mel, int batch, int n_mels, int frames, int c_pad, void* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Embedding gather + audio splice: out[r] = src_row[r] >= 0 ? table[src_row[r]]
 *                                                           : audio_rows[-(src_row[r]+1)]
 * `src_row` (int32 [rows], built by the caller from input_ids / start positions / transcription
 * ids) restates `embed_tokens(input_ids)` + the slice assignment of cat(audio_features,
 * transcription_embeddings) at modeling_desta25.py:1009-1041.  gather_rows is its backward
 * (rows of dL/d inputs_embeds at the audio positions -> dL/d audio_features). */
int desta_embed_gather(const void* table, const void* audio_rows, const int32_t* src_row, int rows, int hidden,
                       void* out, void* stream);
int desta_gather_rows_bf16(const void* in, const int32_t* idx, int rows, int hidden, void* out, void* stream);

/* ForCausalLMLoss (TF:loss/loss_utils.py:49-71): labels int64 [batch, seq] UNSHIFTED (the shift by one
 * and the -100 padding of the last position happen inside), logits bf16 [batch*seq, ld] upcast to fp32;
 * loss[0] = mean CE over targets != -100.  With write_grad != 0 the logits buffer is overwritten by
 * dloss/dlogits (bf16).  workspace: desta_ce_workspace_floats(batch, seq). */
size_t desta_ce_workspace_floats(int batch, int seq);
int desta_causal_lm_loss(void* logits, int64_t ld, const int64_t* labels, int batch, int seq, int vocab,
                         float* loss, float* workspace, int write_grad, void* stream);

/* Token log-probabilities for scoring (multiple-choice ranking by log-likelihood; what `ForCausalLMLoss`
 * TF:loss/loss_utils.py:49-71 averages, kept per token: -F.cross_entropy(..., reduction="none") and the argmax match).
 * logits bf16 [rows, ld] (ld >= vocab, any alignment), READ ONLY — unlike desta_causal_lm_loss, whose buffer becomes dlogits.
 * Row r predicts labels[r]: the caller does the causal shift.  compact_labels + 1 of desta_target_rows is already aligned
 * this way (compact row i predicts compact_labels[1 + i]), so the compact lm_head grid is scored without another pass.
 *   0 <= labels[r] < vocab:  logprob[r] = x[r, labels[r]] - logsumexp(x[r, :vocab]) in fp32, maximum subtracted first; -inf
 *                            entries carry no mass, a -inf label entry gives -inf.  is_top1[r] (optional, may be NULL) = 1 iff
 *                            labels[r] is the FIRST index of the row maximum (torch.argmax, as desta_sample_bf16's greedy mode).
 *   labels[r] < 0 (-100) or >= vocab:  ignored, logprob[r] = 0, is_top1[r] = 0, the row is not read.
 * One 1024-thread block per row, one pass over the row; fixed reduction order (bitwise reproducible). */
int desta_token_logprobs(const void* logits_bf16, int64_t ld, const int64_t* labels, int rows, int vocab,
                         float* logprob, uint8_t* is_top1 /* may be NULL */, void* stream);

/* Log-probability of each decode step's chosen token and the top_n alternatives of its row: what `llm_model.generate`
 * (modeling_desta25.py:1419-1427) yields with output_logits=True followed by log_softmax — the raw distribution, the one
 * compute_transition_scores(normalize_logits=True) reports for greedy search (TF:generation/utils.py: `raw_logits += (next_token_logits,)`
 * and compute_transition_scores) — not the processed output_scores.  Additive to ABI 8.
 * logits bf16 [rows, ld] (ld >= vocab, any alignment), READ ONLY; vocab <= 262144; 0 <= top_n <= 32 (and <= vocab).
 *   logprob(c) = x[r, c] - logsumexp(x[r, :vocab]) in fp32, maximum subtracted first; -inf entries carry no mass.
 *   token_logprob[r]  for 0 <= tokens[r] < vocab: bit-identical to desta_token_logprobs on the same row and label (shared code).
 *   top_ids[r, :]     the top_n largest entries, descending; among equal values (-0.0 == +0.0) the lower index first; a -inf
 *                     entry appears only when fewer than top_n entries are finite, with logprob -inf.
 *   top_logprobs[r,j] logprob(top_ids[r, j]).
 *   tokens[r] < 0 or >= vocab: the row is ignored (a finished sequence) and not read: token_logprob 0, top_ids -1, top_logprobs 0.
 * tokens and token_logprob are both NULL or both set; without tokens every row is ranked.  With top_n == 0 the top pointers may
 * be NULL.  NaN logits and rows without a finite entry are out of contract.  One 1024-thread block per row; integer selection
 * and a fixed reduction order: bitwise reproducible, independent of rows. */
int desta_topk_logprobs(const void* logits_bf16, int64_t ld, const int64_t* tokens /* may be NULL */, int rows, int vocab,
                        int top_n, float* token_logprob /* [rows], NULL iff tokens NULL */,
                        int32_t* top_ids /* [rows, top_n] */, float* top_logprobs /* [rows, top_n] */, void* stream);

/* Classifier-free guidance of a decode step's rows (`generate(guidance_scale=g)` with a negative prompt; audio-contrastive
 * decoding): `UnbatchedClassifierFreeGuidanceLogitsProcessor.__call__` TF:generation/logits_process.py,
 *   scores = log_softmax(scores); uncond = log_softmax(uncond_logits); out = g * (scores - uncond) + uncond,
 * which `_get_logits_processor` TF:generation/utils.py puts FIRST in the chain: the repetition penalty, temperature and the
 * filters act on `out`.  HF runs a second forward for `uncond`; here both rows come out of one decode step.  Additive to ABI 8.
 * cond, uncond bf16 [rows, ld], READ ONLY; out bf16 [rows, ld_out]; ld, ld_out >= vocab; each of the three may have any
 * (2-byte) alignment.  Per row r and column c < vocab:
 *   lc = logprob of cond[r, c], lu = logprob of uncond[r, c]: the bits desta_topk_logprobs reports for that row (shared code);
 *   out[r, c] = bf16_rne( fl( fl(g * fl(lc - lu)) + lu ) ), every fp32 rounding as written, nothing fused;
 *   cond[r, c] or uncond[r, c] == -inf: out[r, c] = -inf.  A deliberate difference: HF gives NaN (-inf - -inf) wherever the
 *   unconditional entry alone is -inf; a token either distribution rules out stays ruled out here.
 * Columns >= vocab of out are not written.  out may not overlap an input (an equal pointer is refused).  NaN inputs and rows
 * without a finite entry are out of contract, as for desta_topk_logprobs.
 * DESTA_EINVAL, nothing launched, unless: pointers non-NULL, out != cond, out != uncond, rows > 0, 0 < vocab <= 262144,
 * ld >= vocab, ld_out >= vocab, guidance_scale finite and > 0.
 * One 1024-thread block per row: one pass over both rows for their (maximum, sum) pairs, a second that stores (16-byte stores
 * between out's 16-byte boundaries).  Fixed reduction order: bitwise reproducible, independent of rows. */
int desta_cfg_scores_bf16(const void* cond_bf16, const void* uncond_bf16, int64_t ld, int rows, int vocab,
                          float guidance_scale, void* out_bf16, int64_t ld_out, void* stream);

/* Connector tap mix (modeling_desta25.py:600-604): x fp32 [taps][batch*prompt][d], layer_weights
 * fp32 [prompt][taps]; out[b,k,:] = sum_j softmax(layer_weights[k,:])_j x[j,b,k,:]; and its backward. */
int desta_tap_mix_fwd(const float* x, const float* layer_weights, int taps, int batch, int prompt, int d,
                      float* out, void* stream);
int desta_tap_mix_bwd(const float* x, const float* layer_weights, const float* dout, int taps, int batch,
                      int prompt, int d, float* dx, float* dlayer_weights, void* stream);

/* ------------------------------------------------------------------------------------------
 * ORCA hybrid connector / deep injection (ABI 6).  The ORCA branch shares the GEMM,
 * attention and LayerNorm entry points with the qformer_1 path; these are the row-wise pieces it adds
 * (/root/reference/desta/models/modeling_desta25.py, line numbers per entry).  All bf16 streams, fp32 arithmetic.
 *   desta_orca_local_mix      :336-343  out[r,:] = sum_l softmax(layer_weights)[l] x[l,r,:]; x [taps][rows][d], taps <= 8
 *   desta_orca_rope           :22-95, :422-438  rotation of the WHOLE hidden vector (pairs i, i + hidden/2) by the angle
 *                             (t / position_scale) theta^(-i / (hidden/2)); round_cos_sin: cos / sin rounded to bf16 first (bf16 model)
 *   desta_orca_gate_residual  :456-490  hidden[m,:] += sigmoid(gate_hidden[m,:] . gate_w2 + gate_b2[0]) * cross[m,:], in place;
 *                             gate_hidden = GELU(Linear(hidden)) [rows, gate_width] from a GEMM; gate_out (fp32 [rows]) optional
 *   desta_orca_sim_loss       :1174-1198  partials[b * nx + i] = sum_j (xhat_i . yhat_j - [subtract_identity and i == j])^2 over
 *                             L2-normalised rows; y rows picked through y_index[ny] (NULL: 0..ny-1) out of y_rows per batch entry
 *   desta_orca_align          :460-486  out[e] = 1 - cos(mean_t audio[e,t,:], mean_{s0 <= s < s1} hidden[row, s, :]),
 *                             spans[e] = (text row, s0, s1); hidden addressed as row * batch_stride + s * row_stride */
/* Backward pieces (autograd of the modules above; gradients of the trainer's total loss = LM loss + sum of the ORCA losses):
 *   desta_orca_gate_residual_bwd  d_cross[m,:] = gate[m] d_out[m,:];  d_gate_pre[m] = (d_out[m,:] . cross[m,:]) gate[m] (1 - gate[m])
 *   desta_orca_gate_mlp_bwd       d_preact = d_gate_pre (x) w2 * gelu'(preact);  d_w2 = sum_m d_gate_pre[m] gate_hidden[m,:];  d_b2 = sum_m d_gate_pre[m]
 *                                 (workspace: 64 x (gate_width + 1) floats, ABI 7: row slices summed in a fixed order)
 *   desta_orca_align_bwd          d_hidden[row, s, :] += coef * d(1 - cos)/d(mean over the span) / span length   (audio pooled under no_grad, :461-462)
 *   desta_orca_rope_bwd           rotation by the negative angle of the fp32 gradient of the rotated tokens, ADDED to d_first (tokens [0, n_first)
 *                                 of every clip: the global tokens under orca_global_cross_attn) resp. d_rest (the local tokens)
 *   desta_orca_col2im_add         gradient of the Conv1d's im2col view: d_padded[b,t,:] = sum of the d_col windows that cover row t (bf16)
 *   desta_orca_local_mix_bwd      d(local_layer_weights) through the softmax (workspace: 256 x 32 floats; taps <= 32)
 *   desta_orca_sim_loss_bwd       d_x += gradient of coef * sum_ij (xhat_i . yhat_j - [identity])^2 w.r.t. the un-normalised rows of x (fp32, added;
 *                                 rows of x / d_x and of y picked through optional index lists; ny <= 128) */
int desta_orca_local_mix(const void* x, const float* layer_weights, int taps, int64_t rows, int d, void* out, void* stream);
int desta_orca_rope(const void* x, void* y, int batch, int tokens, int hidden, float theta, float position_scale, int round_cos_sin, void* stream);
int desta_orca_gate_residual(void* hidden, int64_t ld_hidden, const void* cross, const void* gate_hidden, const float* gate_w2, const float* gate_b2,
                             int64_t rows, int hidden_size, int gate_width, float* gate_out, void* stream);
int desta_orca_sim_loss(const void* x, const void* y, const int32_t* y_index, int batch, int nx, int ny, int64_t y_rows, int hidden,
                        int subtract_identity, float* partials, void* stream);
int desta_orca_align(const void* audio, int tokens, const void* hidden, int64_t hidden_row_stride, int64_t hidden_batch_stride, int hidden_size,
                     const int32_t* spans, int n_spans, float* out, void* stream);
int desta_orca_gate_residual_bwd(const void* d_out, int64_t ld, const void* cross, const float* gate, int64_t rows, int hidden_size, void* d_cross,
                                 float* d_gate_pre, void* stream);
int desta_orca_gate_mlp_bwd(const float* d_gate_pre, const void* gate_preact, const void* gate_hidden, const float* gate_w2, int64_t rows, int gate_width,
                            void* d_preact, float* d_w2, float* d_b2, float* workspace, void* stream);
int desta_orca_align_bwd(const void* audio, int tokens, const void* hidden, int64_t hidden_row_stride, int64_t hidden_batch_stride, int hidden_size,
                         const int32_t* spans, int n_spans, float coef, void* d_hidden, int64_t d_row_stride, int64_t d_batch_stride, void* stream);
int desta_orca_rope_bwd(const float* d_rotated, int batch, int tokens, int hidden, float theta, float position_scale, int round_cos_sin, int n_first,
                        float* d_first, float* d_rest, void* stream);
int desta_orca_col2im_add(const void* d_col, int batch, int tokens_out, int tokens_padded, int hidden, int kernel, int stride, void* d_padded, void* stream);
int desta_orca_local_mix_bwd(const void* d_out, const void* x, const float* layer_weights, int taps, int64_t rows, int d, float* d_layer_weights,
                             float* workspace, void* stream);
int desta_orca_sim_loss_bwd(const void* x, const int32_t* x_index, int64_t x_rows, const void* y, const int32_t* y_index, int64_t y_rows, int batch, int nx,
                            int ny, int hidden, int subtract_identity, float coef, float* d_x, void* stream);

/* ------------------------------------------------------------------------------------------
 * Flash-style attention, forward and backward (bf16 operands, fp32 softmax, MFMA 32x32x16).
 * Element (b, s, h, d) of a tensor X lives at X + b*x_batch_stride + s*x_row_stride + h*head_dim + d,
 * so q/k/v may be slices of one fused projection buffer.  GQA: kv head = q head / (n_q/n_kv).
 * Mask: key j is visible to query i iff j < seq_k, j >= kv_start[b] (left padding; NULL = 0) and,
 * when causal, j <= i + (seq_k - seq_q).  softmax(scale * q.k).  Rows with no visible key give 0.
 * lse (fp32 [batch][n_q_heads][seq_q], log2 domain) is written by fwd and read by bwd.
 * Replaces: Whisper self-attention TF:models/whisper/modeling_whisper.py:241-357 (q pre-scaled by
 * hd^-0.5 == scale), BERT eager self/cross attention TF:models/bert/modeling_bert.py:100-293,
 * Llama/Qwen3 attention TF:models/llama/modeling_llama.py:179-281 with the mask of
 * `create_causal_mask` (:391), and their autograd backward.  bwd: dK/dV may both be NULL
 * (Whisper states carry no gradient, modeling_desta25.py:594). */
typedef struct desta_attn_desc {
    const void* Q; const void* K; const void* V; void* O;
    const void* dO; void* dQ; void* dK; void* dV;
    float* lse;
    int64_t q_batch_stride, q_row_stride, k_batch_stride, k_row_stride, v_batch_stride, v_row_stride;
    int64_t o_batch_stride, o_row_stride, do_batch_stride, do_row_stride;
    int64_t dq_batch_stride, dq_row_stride, dk_batch_stride, dk_row_stride, dv_batch_stride, dv_row_stride;
    int batch, n_q_heads, n_kv_heads, seq_q, seq_k, head_dim;
    int causal;
    const int32_t* kv_start;
    float scale;
    float dropout_p;                   /* attention-probability dropout (head_dim 64 only), same mask in fwd and bwd */
    uint64_t dropout_seed;
    const float* rope_cos_sin;         /* optional (ABI 4), bwd only: [seq][head_dim / 2][2] fp32 (cos, sin).  Q and K are the rotary-  */
                                       /* embedded projections in the adjacent-pair layout of desta_gemm_desc.rope_*: dQ (row q: position */
                                       /* q) and dK (row k: position k) are rotated back by the transposed rotation before they are       */
                                       /* stored, i.e. they come out as gradients of the projection OUTPUTS.  Needs the 8-wave dQ path   */
                                       /* (seq_q >= 128, no dropout, 16-byte aligned dQ / dK / dV).  NULL = off.                         */
    float* O_f32;                      /* optional (ABI 4): fp32 copy of O written by fwd, indexed with the o_* strides.  bwd then   */
                                       /* takes delta = rowsum(dO * O) from the UNROUNDED output: with delta from the bf16-rounded O */
                                       /* the error of delta is coherent over the keys of a row (dS_err = P * eps_q) and, where the   */
                                       /* softmax is flat over 1500 encoder frames, puts 10-13 % error on the cross-attention query   */
                                       /* weight gradient (eager attention in the reference sums P * dP itself: no such term).        */
    int dkv_transposed;                /* optional (ABI 5), bwd on the one-query-tile path only (head_dim 64, seq_q <= 64, seq_k >= 256, */
    int64_t dkv_t_ld;                  /* seq_k % 4 == 0, no GQA): dK and dV are written TRANSPOSED, as [n_heads * 64][dkv_t_ld] bf16    */
    float* dkv_bias_grad;              /* matrices with element (h * 64 + d, b * seq_k + key) — the operand layout of the K / V          */
                                       /* projection's weight-gradient GEMM (no transpose pass); dk_* / dv_* strides are ignored.       */
                                       /* dkv_bias_grad (optional): fp32 [2][n_heads * 64] = sums over batch and keys of dK | dV (the   */
                                       /* projection's bias gradients), overwritten.                                                    */
} desta_attn_desc;
int desta_attention_fwd(const desta_attn_desc* d, void* stream);
/* floats of `workspace` for desta_attention_bwd: delta [batch][heads][seq_q] and, for seq_q <= 64 (one query tile: the one-pass
 * dQ / dK / dV kernel), up to 4 fp32 dQ partials of 64 x 64 and bias-gradient partials of 2 x 64 per (batch, head), summed in
 * fixed order (no atomics). */
size_t desta_attention_bwd_workspace_floats(int batch, int n_q_heads, int seq_q);
int desta_attention_bwd(const desta_attn_desc* d, float* workspace, void* stream);
/* D = 128 backward: run the dQ kernel on an internal side stream next to dK/dV (fork after delta, join on `stream`);
 * 1 = on (default), 0 = everything on `stream`.  Results are identical either way. */
int desta_attention_set_concurrent_bwd(int on);
/* Process-wide kernel selection switches (A/B measurements; results agree to rounding either way):
 *   which 0: forward for seq_q >= 128 without dropout on the 8-wave kernel (1, default) or the 4-wave kernel (0);
 *   which 1: head_dim 64 non-causal 8-wave forward at two blocks per CU (1) or one (0, default);
 *   which 2: 1 = the 8-wave forward WITH waves 4-7 half a tile behind waves 0-3 (LLM / Whisper shapes only; default 0);
 *   which 3: 1 = backward on round 2's path (separate delta launch, 4-wave dQ kernel on a side stream beside dK / dV) instead
 *            of the 8-wave dQ kernel that computes delta itself (default 0; not available with rope_cos_sin);
 *   which 4: 1 (default) = one query tile (seq_q <= 64, head_dim 64, seq_k >= 256, no GQA, dK / dV requested): dQ, dK, dV in ONE
 *            pass over K / V; 0 = the separate dQ and dK / dV kernels;
 *   which 5: 1 = causal head_dim-128 dK / dV on 64-key blocks of two waves (640 shorter work items instead of 320; measured
 *            SLOWER on the LLM shape, 207 vs 194 us: default 0). */
int desta_attention_set_option(int which, int value);

/* Split-KV GQA decode attention (additive to ABI 8: no struct changes): the attention of one KV-cached decode step inside
 * llm_model.generate (modeling_desta25.py:1419; TF:models/llama/modeling_llama.py:230-281 with past_key_values) for long caches
 * and wide batches.  Takes the descriptor of desta_attention_fwd with seq_q == 1; strides, offsets, kv_start, scale, lse (log2
 * domain, [batch][n_q_heads][1]) and GQA by n_q_heads / n_kv_heads mean what they mean there, any seq_k >= 1.  A work item is
 * (batch row, KV head, chunk c of keys [c * CHUNK, min((c + 1) * CHUNK, seq_k))): every K / V byte is read once per GQA group,
 * a row's chunks run on different CUs, and the chunk boundaries depend on nothing but CHUNK, so a row's result does not depend
 * on the batch, on kv_start of other rows, on the cache's batch stride or on the device.  Cache rows >= seq_k are never read.
 * seq_k <= CHUNK: one launch, `workspace` may be NULL.  Otherwise each item leaves an fp32 partial (max, sum, unnormalised O)
 * in `workspace` and a second launch merges a row's chunks in ascending order (no atomics).
 * Returns DESTA_EINVAL and launches nothing for: seq_q != 1, head_dim != 128, more than 8 query heads per KV head, causal,
 * dropout_p != 0, non-NULL rope_cos_sin / O_f32 / dO / dQ, O (or Q, K, V) not 16-byte aligned or with a batch stride that is
 * no multiple of 8 elements, a workspace smaller than desta_attention_decode_workspace_bytes() or not 16-byte aligned. */
#ifndef DESTA_ATTN_DECODE_CHUNK
#define DESTA_ATTN_DECODE_CHUNK 256
#endif
int    desta_attention_decode_chunk(void);         /* DESTA_ATTN_DECODE_CHUNK as the library was compiled */
size_t desta_attention_decode_workspace_bytes(int batch, int n_q_heads, int seq_k, int head_dim);
int    desta_attention_decode(const desta_attn_desc* d, void* workspace, size_t workspace_bytes, void* stream);

/* Decode attention on the opt-in FP8 KV cache (additive to ABI 8: no struct changes): desta_attention_decode for a cache that
 * holds OCP e4m3fn bytes, the quantised `DynamicCache` of llm_model.generate (modeling_desta25.py:1419;
 * TF:models/llama/modeling_llama.py:230-281 with past_key_values, TF:cache_utils.py QuantizedCache).
 * Cache format, per layer:
 *   bytes  [batch][slots][2 * n_kv_heads * 128]  e4m3fn, K heads then V heads, the element order of the bf16 slab;
 *   scales [batch][slots][2 * n_kv_heads]        fp32, one per (row, slot, K-or-V head).
 * Scale and bytes follow desta_quantize_rows_e4m3 with "row" = one head's 128 values: scale = 2^e, e the smallest integer with
 * amax * 2^-e <= 448, an all-zero head gets 1; q = e4m3fn(x * 2^-e), round to nearest even, nothing saturates.  q * scale is
 * exactly a bf16 value.  2 048 + 64 bytes per cached token and layer at 8 KV heads against 4 096 for bf16.
 * d->K / d->V point at the bytes and their strides count elements (= bytes, the convention of desta_gemm_w8a16_nt's ldb);
 * k_scale / v_scale point at the first K / V scale of head 0 (scales and scales + n_kv_heads of the tensor above) and share
 * scale_batch_stride / scale_row_stride (floats).  Everything else in the descriptor, the workspace
 * (desta_attention_decode_workspace_bytes) and the rejections are desta_attention_decode's, plus NULL scales.  Neither bytes
 * nor scales of slots outside [kv_start, seq_k) are read.  O, lse and every workspace partial equal desta_attention_decode's
 * on the dequantised cache bf16(q * scale), bit for bit, as long as nothing underflows: a power of two commutes with an fp32
 * rounding only in the normal range, so the identity is promised for scales for which score * k_scale and p * v_scale stay
 * normal fp32 values and q * scale stays a normal bf16 value (any head whose amax is above ~2^-100; the caches of real models
 * are many orders of magnitude inside).  Below that the result is still the attention of the dequantised cache to rounding. */
int    desta_attention_decode_kv8(const desta_attn_desc* d, const float* k_scale, const float* v_scale, int64_t scale_batch_stride,
                                  int64_t scale_row_stride, void* workspace, size_t workspace_bytes, void* stream);

/* Split-KV attention of a verify step (additive to ABI 8: no struct changes): the attention of the k + 1 candidate rows that
 * `llm_model.generate(prompt_lookup_num_tokens=k)` checks in one pass against past_key_values (modeling_desta25.py:1419;
 * TF:generation/utils.py _assisted_decoding, TF:models/llama/modeling_llama.py:230-281), on either cache form.  The work
 * items, chunks, workspace protocol and arithmetic of desta_attention_decode{,_kv8}, with seq_q = 2..8 query rows per sequence:
 * the R = (n_q_heads / n_kv_heads) * seq_q <= DESTA_ATTN_VERIFY_MAX_ROWS query rows of a KV head share every K / V byte and
 * scale of an item.  The descriptor is desta_attention_fwd's for that shape: causal = 1 (query row j sees keys
 * kv_start[b] <= key <= j + seq_k - seq_q), Q rows at q_row_stride inside q_batch_stride, O likewise, lse optional,
 * [batch][n_q_heads][seq_q] in the log2 domain.  A row that sees no key gets O = 0 and lse = +inf.
 * Query row j equals, bit for bit in O and lse, desta_attention_decode{,_kv8} on the same cache with
 * seq_k' = seq_k - (seq_q - 1 - j) and that row as the one query: a masked key enters as p = exp2(-inf) = 0 and
 * fma(0, v, acc) = acc, block maximum, row sum, empty chunks and the merge are kept per query row, and the per-row summation
 * order does not depend on R.  Rows >= seq_k of the cache (and their scales) are never read; rows in [seq_k', seq_k) are read
 * and must hold finite values (a verify step has just appended them).
 * Workspace: desta_attention_verify_workspace_bytes (0 while seq_k <= CHUNK; one partial per query row, head and chunk).
 * Returns DESTA_EINVAL and launches nothing for: seq_q outside 2..8, more than 8 query heads per KV head, R > 16,
 * head_dim != 128, causal == 0, dropout_p != 0, non-NULL rope_cos_sin / O_f32 / dO / dQ, O (or Q, K, V) not 16-byte aligned or
 * with a batch or row stride that is no multiple of 8 elements, a workspace that is too small or not 16-byte aligned, and (kv8)
 * NULL scales. */
#define DESTA_ATTN_VERIFY_MAX_SEQ_Q 8
#define DESTA_ATTN_VERIFY_MAX_ROWS 16
size_t desta_attention_verify_workspace_bytes(int batch, int n_q_heads, int seq_q, int seq_k, int head_dim);
int    desta_attention_verify(const desta_attn_desc* d, void* workspace, size_t workspace_bytes, void* stream);
int    desta_attention_verify_kv8(const desta_attn_desc* d, const float* k_scale, const float* v_scale, int64_t scale_batch_stride,
                                  int64_t scale_row_stride, void* workspace, size_t workspace_bytes, void* stream);

/* The FP8 KV cache of one layer back as bf16, for the attention of a prompt chunk (additive to ABI 8): the forward kernel
 * reads bf16, so a chunk that attends cached e4m3 keys gets them through a staging slab.  kv_cache / kv_scale: the bytes and
 * scales of desta_attention_decode_kv8's format, n_heads = K heads + V heads of one slot (2 * n_kv_heads), head_dim 128;
 * strides of the bytes in bytes, of the scales in floats, of the output in bf16 elements.  For every row b, slot s in
 * [kv_start[b], slot1) (kv_start NULL: from 0; values are clamped to [0, slot1]) and head:
 *   out[b][s][head][0..128) = bf16(e4m3(byte) * scale),
 * exactly (the scale is a power of two), the value desta_attention_decode_kv8 forms in registers.  Slots below kv_start[b]
 * and at or above slot1 are neither read (bytes, scales) nor written.  DESTA_EINVAL with nothing launched for head_dim != 128,
 * batch <= 0, n_heads <= 0, slot1 <= 0, a NULL cache / scale / output, a cache that is not 16-byte aligned with strides that
 * are multiples of 16 bytes, an output that is not 16-byte aligned with strides that are multiples of 8 elements, or a row
 * stride narrower than the heads. */
int    desta_kv8_dequant(const uint8_t* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride, const float* kv_scale,
                         int64_t scale_batch_stride, int64_t scale_row_stride, const int32_t* kv_start, int batch, int n_heads,
                         int head_dim, int slot1, void* out_bf16, int64_t out_batch_stride, int64_t out_row_stride, void* stream);

/* layer_prompts[j].expand(B,-1,-1) for all taps at once (modeling_desta25.py:589): prompts fp32
 * [taps][n], n = prompt_size*d -> rows [(taps*batch)][n] in fp32 and bf16; prompt_grad sums the
 * gradient back over the batch. */
int desta_prompt_expand(const float* prompts, int taps, int batch, int64_t n, float* x_f32, void* x_bf16, void* stream);
int desta_prompt_grad(const float* dx, int taps, int batch, int64_t n, float* dprompts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Counter-based dropout (stateless: element `i` of stream `seed` is kept iff rng32(seed, i) >= p*2^32),
 * used by the GEMM epilogue, the attention kernels (i = ((b*H + h)*seq_q + q)*seq_k + k) and:
 *   desta_dropout_bf16      y[r][c] = keep(r*cols + c) ? x[r][c] / (1-p) : 0   (backward of the epilogue dropout)
 *   desta_dropout_mask_u8   materialises the keep mask (tests / debugging)
 * Replaces nn.Dropout(hidden_dropout_prob) / attention_probs dropout of the Q-Former
 * (TF:models/bert/modeling_bert.py:150-160, 296, 350; BertConfig defaults 0.1, modeling_desta25.py:156). */
int desta_dropout_bf16(const void* x, void* y, int rows, int cols, int64_t ld, float p, uint64_t seed, void* stream);
int desta_dropout_mask_u8(uint64_t seed, int64_t n, float p, uint8_t* out, void* stream);

/* lm_head on target rows only.  `ForCausalLMLoss` (TF:loss/loss_utils.py:49-71) ignores every row whose shifted label is
 * -100, so the logits of those rows (context, audio span, last position: 20 % of the synthetic batch, more on real data)
 * and their zero gradients need not be computed.  desta_target_rows lists the rows of the [batch*seq] grid that carry a
 * target (idx, in order; count[0] = n, count[1] = the first POSITION s that carries a target in any sequence, seq if none:
 * `count` is int32[2] since ABI 5) and lays their targets out as compact_labels[0] = -100, [1 + i] = target of compact
 * row i, [1 + n] = -100 (room for batch*seq + 2 entries): desta_causal_lm_loss(batch = 1, seq = n + 1) on a compact
 * [n + 1, vocab] logits buffer then gives the same loss / gradients as the full grid.  desta_scatter_rows_bf16 is the
 * inverse of desta_gather_rows_bf16 (out[idx[i]] = in[i]). */
int desta_target_rows(const int64_t* labels, int batch, int seq, int32_t* idx, int64_t* compact_labels, int32_t* count,
                      int s_major, void* stream);   /* s_major != 0: idx holds position-major row ids s * batch + b */
int desta_scatter_rows_bf16(const void* in, const int32_t* idx, int rows, int hidden, void* out, void* stream);

/* Greedy decoding helper: out[r] = argmax over the first `cols` entries of bf16 row r (first maximum, two-stage
 * reduction; `workspace` holds desta_argmax_workspace_bytes(rows) bytes).  -0.0 and +0.0 are equal, as in torch.argmax and in
 * desta_sample_bf16's greedy mode; a row of -inf alone gives 0.
 * Replaces the argmax of `llm_model.generate(do_sample=False)` (modeling_desta25.py:1419). */
size_t desta_argmax_workspace_bytes(int rows);
/* logits[r, ids[i]] = -inf (bf16 rows of `cols` entries, row stride ld) for every row r: token suppression in front of the argmax
 * (Whisper ASR leg of generate(), modeling_desta25.py:1580-1590 -> TF:generation/logits_process.py SuppressTokensLogitsProcessor). */
int desta_mask_tokens_bf16(void* logits, int64_t ld, int rows, int cols, const int32_t* ids, int n, void* stream);
int desta_argmax_bf16(const void* x, int64_t ld, int rows, int cols, int64_t* out, void* workspace, void* stream);

/* `do_sample=True` step of `llm_model.generate` (modeling_desta25.py:1419-1427: temperature, top_p):
 * TemperatureLogitsWarper -> TopPLogitsWarper -> one multinomial draw per row
 * (TF:generation/logits_process.py, TF:generation/utils.py `_sample`).  Token i is kept iff the softmax mass of all
 * tokens not more probable than i exceeds 1 - top_p; tokens tying with the boundary logit are all kept.  The draw uses
 * the library's counter-based RNG (seed, step, row) — same distribution as torch.multinomial, not the same stream.
 * keep_mask (optional, uint8 [rows, cols]) exports the kept set (tests): the tokens that can be drawn, so a -inf logit
 * (desta_mask_tokens_bf16) is never in it, whatever top_p is; -0.0 and +0.0 are one logit value.  A row without a finite
 * logit keeps nothing and yields token 0. */
int desta_sample_top_p_bf16(const void* logits, int64_t ld, int rows, int cols, float temperature, float top_p,
                            uint64_t seed, uint32_t step, int64_t* out, uint8_t* keep_mask, void* stream);

/* One decode step of HF's whole logits chain, one launch, one 1024-thread block per bf16 row (`rows` x `cols`, stride ld):
 * the decode loop of `llm_model.generate(inputs_embeds=…)` (modeling_desta25.py:1419-1427) and of `llm_model.generate(input_ids)`
 * for text-only chats (modeling_desta25.py:1703-1711), with HF's processors in HF's order (TF:generation/utils.py:1175,
 * 1296-1330), each on the fp32 value of the logit (TF:generation/utils.py:2894):
 *   1. RepetitionPenaltyLogitsProcessor: every DISTINCT token of row r's history hist[r*hist_ld + 0 .. hist_len) gets
 *      s < 0 ? s * p : s / p once (ids outside [0, cols) are ignored); p == 1 or hist_len == 0: off.  Greedy mode too.
 *   2. do_sample == 0: out[r] = first index of the maximum penalised score (torch.argmax); nothing below applies.
 *   3. TemperatureLogitsWarper: t = s / T (fp32 division).
 *   4. TopKLogitsWarper: keep t >= the k-th largest t (ties with it kept); top_k == 0 or >= cols: off.
 *   5. TopPLogitsWarper on the top-k survivors: token i is kept iff the softmax mass of the kept tokens not more probable
 *      than i exceeds 1 - top_p; ties with the boundary are kept; top_p == 1: off.
 *   6. MinPLogitsWarper: keep exp(t_i - t_max) >= min_p (= p_i >= min_p * p_max); min_p == 0: off.
 *   7. one draw per row from the kept masses (index-order prefix sum) with desta_rng32(seed, (step << 32) | row), the
 *      counter of desta_sample_top_p_bf16.
 * Sums are fixed point (2^-40 of the row maximum's mass), so results are deterministic per (seed, step, row).
 * keep_mask (optional, uint8 [rows, cols]) exports the kept set (greedy: the pick): a -inf score is never kept, with every
 * filter off too.  A row without a finite score keeps nothing and yields token 0, in both modes.  DESTA_EINVAL unless T > 0,
 * 0 < top_p <= 1, top_k >= 0, 0 <= min_p <= 1, repetition_penalty > 0, hist_len >= 0 (hist != NULL and hist_ld >= hist_len
 * when hist_len > 0), and cols <= 262144 when the penalty is active. */
int desta_sample_bf16(const void* logits, int64_t ld, int rows, int cols, const int64_t* hist, int64_t hist_ld, int hist_len,
                      float repetition_penalty, int do_sample, float temperature, int top_k, float top_p, float min_p,
                      uint64_t seed, uint32_t step, int64_t* out, uint8_t* keep_mask, void* stream);

/* The two samplers over the rows of a verify step (additive since ABI 8; `CausalLMHIP._speculative_loop` under
 * `set_speculative(k, scope="all")`): the logits hold batch * width rows, batch-major, row r = b * width + j, 1 <= width <= 8
 * (k + 1).  Row (b, j) is DEFINED as what desta_sample_bf16 / desta_sample_top_p_bf16 return for row b of a `batch`-row launch at
 * step = step0 + j (a uint32 sum: it wraps, as step does) — emitted position step0 + j of sequence b in the loop of
 * `llm_model.generate` (modeling_desta25.py:1419-1427, :1703-1711), so a verify step picks what the token-by-token loop picks:
 *   draw ............ desta_rng32(seed, ((uint64)(uint32)(step0 + j) << 32) | b): the counter row is b, not r;
 *   penalty history . (desta_sample_rows_bf16) the distinct ids of hist[b*hist_ld + 0 .. hist_len) and of
 *                     tail[b*tail_ld + 1 .. 1 + j): `tail` is the verify step's input [batch, k + 1], whose column 0 is the last
 *                     emitted token (hist holds it at hist_len - 1) and whose columns 1..k are the drafts; ids outside [0, cols)
 *                     are ignored, so a -1 draft is.  tail may be NULL when width == 1 or repetition_penalty == 1.
 * Everything else is the one-row-per-sequence entry point's, both modes of do_sample included: processor order, fixed-point
 * masses, index-order prefix sum, ties, -inf handling, token 0 for a row without a finite score; out [batch * width] and
 * keep_mask [batch * width, cols] are indexed by r.  The kernels are the same ones (width = 1 there).  DESTA_EINVAL, nothing
 * launched: what the one-row entry points reject, a width outside 1..8, and a NULL tail (or tail_ld < width) when width > 1
 * and repetition_penalty != 1. */
int desta_sample_rows_bf16(const void* logits, int64_t ld, int batch, int width, int cols,
                           const int64_t* hist, int64_t hist_ld, int hist_len,
                           const int64_t* tail, int64_t tail_ld,
                           float repetition_penalty, int do_sample, float temperature, int top_k, float top_p, float min_p,
                           uint64_t seed, uint32_t step0, int64_t* out, uint8_t* keep_mask, void* stream);
int desta_sample_top_p_rows_bf16(const void* logits, int64_t ld, int batch, int width, int cols,
                                 float temperature, float top_p, uint64_t seed, uint32_t step0,
                                 int64_t* out, uint8_t* keep_mask, void* stream);

/* desta_sample_rows_bf16 with HF's truncation warpers between its step 6 (min-p) and its draw (additive to ABI 8;
 * `generate(typical_p=, epsilon_cutoff=, eta_cutoff=)`): TypicalLogitsWarper, EpsilonLogitsWarper, EtaLogitsWarper of
 * TF:generation/logits_process.py in the order of `_get_logits_processor` (TF:generation/utils.py), min_tokens_to_keep = 1.
 * Same grid, rows, history, tail, counter and fixed-point masses as desta_sample_rows_bf16; width == 1 is the one-row case.
 * With S the survivors of steps 4-6, a_i = t_i - t_max, e_i = exp(a_i), and every step renormalising over ITS input set
 * (p_i = e_i / sum of e over that set, as each HF warper takes a fresh softmax of scores that hold -inf on removed tokens):
 *   7. typical_p = m < 1: c = sum_S p_i a_i, d_i = |a_i - c| (= HF's |-log p_i - H|, as H = log Z - c and -log p_i = log Z - a_i);
 *      D = the smallest d with sum over {i in S, d_i <= D} of p_i >= m; keep d_i <= D.  Tokens tied with D all stay, the token
 *      closest to c always stays, and the row's most probable token can go.  typical_p == 1: off.
 *   8. epsilon_cutoff = eps > 0: over the survivors of step 7 keep p_i >= eps, and every token tied with the maximum score OF
 *      THOSE SURVIVORS (after step 7 that need not be t_max).  0: off.
 *   9. eta_cutoff = eta > 0: over the survivors of step 8, H = -sum p_i log p_i, theta = min(eta, sqrt(eta) * exp(-H)); keep
 *      p_i >= theta, and every token tied with the survivors' maximum.  0: off.
 *  10. the draw of desta_sample_bf16 (step 7 there) on what is left.
 * The sums that decide a kept set (Z, sum e a, the mass bins of the radix select over d) are integer sums of 2^-40 fixed point
 * values, so their order cannot change the result.  keep_mask, -inf scores (never kept), rows without a finite score (nothing
 * kept, token 0) and greedy mode (do_sample == 0: steps 3-10 do not apply) are as in desta_sample_bf16.  With all three off the
 * launch IS desta_sample_rows_bf16's: the same kernel, bit-identical picks and keep masks.  DESTA_EINVAL, nothing launched: what
 * desta_sample_rows_bf16 rejects, and unless 0 < typical_p <= 1, 0 <= epsilon_cutoff < 1, 0 <= eta_cutoff < 1. */
int desta_sample_truncated_rows_bf16(const void* logits, int64_t ld, int batch, int width, int cols,
                                     const int64_t* hist, int64_t hist_ld, int hist_len,
                                     const int64_t* tail, int64_t tail_ld,
                                     float repetition_penalty, int do_sample, float temperature, int top_k, float top_p, float min_p,
                                     float typical_p, float epsilon_cutoff, float eta_cutoff,
                                     uint64_t seed, uint32_t step0, int64_t* out, uint8_t* keep_mask, void* stream);

/* The hard constraints of HF's logits chain on the scores of one decode step (additive to ABI 8; `generate(no_repeat_ngram_size=,
 * bad_words_ids=, suppress_tokens=, begin_suppress_tokens=, min_new_tokens=)`, the loop of `llm_model.generate`
 * modeling_desta25.py:1419 / :1703): NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor, SuppressTokensLogitsProcessor,
 * SuppressTokensAtBeginLogitsProcessor and MinNewTokensLengthLogitsProcessor of TF:generation/logits_process.py, in the order
 * of `_get_logits_processor` TF:generation/utils.py:1174-1290.  All five only set scores to -inf, so their order among
 * themselves and against the repetition penalty (-inf stays -inf) does not show; the pass runs behind desta_cfg_scores_bf16
 * and in front of the pickers, which never keep a -inf score.
 * src bf16 [batch * width, ld_src], dst bf16 [batch * width, ld_dst], any (2-byte) alignment.  The grid is (batch, width),
 * 1 <= width <= 8, the convention of desta_sample_rows_bf16: row (b, j) is row r = b * width + j, it picks emitted position
 * t = step0 + j (a uint32 sum), and its history h, of length L = hist_len + j, is hist[b*hist_ld + 0 .. hist_len) followed by
 * tail[b*tail_ld + 1 .. 1 + j) (the verify step's input; width == 1 never reads tail).  h is HF's `input_ids` of the row.  Every
 * value of h is an ordinary token for matching, a -1 or an id >= cols included; only ids in [0, cols) can be banned.
 *   no_repeat_ngram = n > 0: nothing while L + 1 < n; else h[i + n - 1] is banned for every 0 <= i <= L - n with
 *                     h[i .. i + n - 1) == h[L - n + 1 .. L)  (n == 1: every token of h).
 *   words ........... word w is word_ids[word_off[w] .. word_off[w + 1]), m ids (int32, DEVICE memory, word_off holds n_words + 1
 *                     ascending offsets, the last one n_word_ids).  m == 1: the id is banned, always (suppress_tokens are passed
 *                     as such words).  m > 1: the last id is banned iff m <= L and the last m - 1 tokens of h are the word's
 *                     first m - 1: m <= L, not m - 1 <= L, as HF skips a word longer than the context (logits_process.py:1303).
 *                     The caller drops [eos] words first, as HF does.
 *   begin_ids ....... banned iff t == 0.
 *   eos_ids ......... banned iff t < min_new_tokens; off when n_eos == 0.
 * dst[r, c] = -inf (0xFF80) for a banned c, else src[r, c] bit for bit, c < cols; columns >= cols of dst are not written.  dst
 * == src is allowed (equal pointers and strides; any other overlap is not): then only the banned entries are stored and src
 * is not read.  A row with every token banned makes the pickers return token 0.  id_max is the largest id of the three
 * tables as their builder knows it (-1 for none): the tables live on the device, so this is what the call can check.
 * DESTA_EINVAL, nothing launched, unless: src, dst non-NULL; batch > 0; 0 < cols <= 262144; ld_src, ld_dst >= cols; width in
 * 1..8; tail non-NULL and tail_ld >= width when width > 1; hist non-NULL and hist_ld >= hist_len when hist_len > 0; no size
 * negative; n_words <= 65536 and n_words <= n_word_ids <= 1048576, with both tables non-NULL when n_words > 0; begin_ids /
 * eos_ids non-NULL when counted; id_max < cols.  no_repeat_ngram == 0, n_words == 0, n_begin == 0 and min_new_tokens == 0
 * (or n_eos == 0) each switch their rule off; with all off DESTA_OK is returned and nothing is launched or written.
 * One 1024-thread block per row; the banned set is a 32 KiB LDS bitmap; no global atomics, no scratch. */
int desta_logit_constraints_bf16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int batch, int width, int cols,
                                 const int64_t* hist, int64_t hist_ld, int hist_len, const int64_t* tail, int64_t tail_ld,
                                 uint32_t step0, int no_repeat_ngram,
                                 const int32_t* word_ids, const int32_t* word_off, int n_words, int n_word_ids,
                                 const int32_t* begin_ids, int n_begin, const int32_t* eos_ids, int n_eos, int min_new_tokens,
                                 int id_max, void* stream);

/* desta_rope (forward) on a fused q|k|v projection [rows, ld] that ALSO appends the rotated K heads and the V heads of
 * row (b, s) to a KV cache slab: kv_cache + b*kv_batch_stride + (slot0 + s)*kv_row_stride, K heads then V heads.
 * This is what `DynamicCache.update` does inside `llm_model.generate` (modeling_desta25.py:1419) for the prompt
 * (seq = prompt length, slot0 = 0) and for every decode step (seq = 1, slot0 = cache length).
 * The kernel reads the V heads out of `qkv` and writes kv_row_stride-spaced slots of batch rows / seq, so this form is held to
 * what its _bias twin is held to; newly rejected (DESTA_EINVAL, nothing launched) are: rows not a multiple of seq (the last
 * sequence's slots would lie behind the cache); an ld below (n_q_heads + 2 n_kv_heads) * head_dim (the V heads would be read
 * out of the next row); n_q_heads or n_kv_heads <= 0; a kv_row_stride below 2 n_kv_heads * head_dim (slots would overlap) or a
 * negative kv_batch_stride; an unaligned cos_sin; a lone k_norm_w. */
int desta_rope_kv_append(void* qkv, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                         const float* cos_sin, const float* q_norm_w, const float* k_norm_w, float eps,
                         const int32_t* pos_shift, void* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride,
                         int slot0, void* stream);

/* desta_rope_kv_append for the FP8 KV cache (format: desta_attention_decode_kv8): q and k are rotated in place with the bits
 * desta_rope_kv_append leaves (q/k-norm included); the rotated K heads and the V heads of row (b, s) are quantised per head
 * and written as bytes to kv_cache + b*kv_batch_stride + (slot0 + s)*kv_row_stride and as scales to
 * kv_scale + b*scale_batch_stride + (slot0 + s)*scale_row_stride, K heads then V heads.  One launch; head_dim 128 only.
 * `DynamicCache.update` of a quantised cache inside `llm_model.generate` (modeling_desta25.py:1419), prompt (seq = prompt
 * length, slot0 = 0) and decode step (seq = 1, slot0 = cache length).
 * Held to what its _bias twin is held to; newly rejected (DESTA_EINVAL, nothing launched) are: an ld below
 * (n_q_heads + 2 n_kv_heads) * head_dim (the V heads would be read out of the next row); a negative kv_batch_stride; an
 * unaligned cos_sin. */
int desta_rope_kv_append_e4m3(void* qkv, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                              const float* cos_sin, const float* q_norm_w, const float* k_norm_w, float eps,
                              const int32_t* pos_shift, uint8_t* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride,
                              float* kv_scale, int64_t scale_batch_stride, int64_t scale_row_stride, int slot0, void* stream);

/* The three rotary entry points for decoders whose q_proj / k_proj / v_proj carry a bias (Qwen2 / Qwen2.5,
 * TF:models/qwen2/modeling_qwen2.py attention: `nn.Linear(..., bias=True)` for q, k, v and no bias for o).  Additive since
 * ABI 8; forward only (d(pre-bias) = d(post-bias), so the backward is desta_rope's).  The projection GEMM stays bias-free
 * and leaves bf16(x W^T) in the fused [rows, ld] q|k|v buffer; these kernels read it, add qkv_bias (fp32
 * [(n_q_heads + 2 n_kv_heads) * head_dim], q then k then v, 16-byte aligned) and write back IN PLACE: q and k heads rotated
 * in fp32 and rounded once, v heads as bf16(v + b).  So ld must hold all three parts, also for desta_rope_bias.  The cache
 * forms append the rotated K heads and the biased V heads as their bias-free twins do; in the e4m3 form the per-head
 * power-of-two scale is taken from those bf16 values, i.e. after the bias.  With a zero bias every output bit is the twin's.
 * q_norm_w / k_norm_w must be NULL: a bias together with q/k-norm weights returns DESTA_EINVAL and launches nothing, as does
 * any other bad argument.  The remaining arguments are those of the twin. */
int desta_rope_bias(void* buf, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                    const float* cos_sin, const float* q_norm_w, const float* k_norm_w, const float* qkv_bias,
                    const int32_t* pos_shift, int s_major_batch, void* stream);
int desta_rope_kv_append_bias(void* qkv, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                              const float* cos_sin, const float* q_norm_w, const float* k_norm_w, const float* qkv_bias,
                              const int32_t* pos_shift, void* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride,
                              int slot0, void* stream);
int desta_rope_kv_append_e4m3_bias(void* qkv, int64_t ld, int rows, int seq, int n_q_heads, int n_kv_heads, int head_dim,
                                   const float* cos_sin, const float* q_norm_w, const float* k_norm_w, const float* qkv_bias,
                                   const int32_t* pos_shift, uint8_t* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride,
                                   float* kv_scale, int64_t scale_batch_stride, int64_t scale_row_stride, int slot0, void* stream);

/* Draft-and-verify greedy decoding (additive since ABI 8; `CausalLMHIP.verify_step` runs k + 1 rows per sequence through one
 * pass over the weights).  Both kernels work on int64 token ids and take k in 1..7; anything else returns DESTA_EINVAL and
 * launches nothing.
 *
 * desta_spec_ngram_draft: prompt lookup, what PromptLookupCandidateGenerator.get_candidates does on the host for
 * `llm_model.generate(prompt_lookup_num_tokens=k)` (TF:generation/candidate_generator.py; the greedy loop it feeds is
 * modeling_desta25.py:1419 / :1703).  One block per row of hist [batch, hist_ld], of which hist_len entries are valid.  For n from
 * n_max down to n_min (1 <= n_min <= n_max <= 4) it looks for the largest i >= row_start[b] (NULL: 0) with i + n <= hist_len - 1
 * and hist[b, i .. i + n) == hist[b, hist_len - n .. hist_len); negative ids (left pads, audio placeholders) never match.  The
 * first n with a match wins: draft[b, j] = hist[b, i + n + j] while i + n + j < hist_len, else -1; no match: every entry -1. */
int desta_spec_ngram_draft(const int64_t* hist, int64_t hist_ld, int batch, int hist_len, const int32_t* row_start, int k,
                           int n_max, int n_min, int64_t* draft, void* stream);
/* desta_spec_accept: the acceptance rule of the greedy loop of `llm_model.generate` (modeling_desta25.py:1419 / :1703) run with
 * candidates (TF:generation/candidate_generator.py PromptLookupCandidateGenerator feeds HF's assisted decoding), in LOCKSTEP: every
 * row advances by the same number of tokens.  inp [batch, k + 1] is the verify pass's input (last emitted token, then k drafts, -1 =
 * no draft), pred [batch, k + 1] the argmax of its rows.  For an unfinished row m_b = number of leading j in 1..k with
 * inp[b, j] >= 0 && inp[b, j] == pred[b, j - 1]; the row may take pred[b, 0 .. m_b].  A row with one of the n_eos ids among
 * those finishes at it and limits nobody; a = min(max_take, min over the other unfinished rows of m_b + 1) >= 1.  Written:
 * out[b, n .. n + a) (row stride ld_out; predictions, `pad` behind a row's EOS and on rows finished before the call),
 * finished[b], next[b] = out[b, n + a - 1], taken[0] = a, and, with hist != NULL, the same a tokens at
 * hist[b, hist_col .. hist_col + a) (the lookup history).  One block, plain stores.  DESTA_EINVAL unless max_take >= 1,
 * n + max_take <= ld_out and hist_col + max_take <= hist_ld. */
int desta_spec_accept(const int64_t* pred, const int64_t* inp, int batch, int k, uint8_t* finished, const int64_t* eos, int n_eos,
                      int64_t pad, int max_take, int64_t* out, int64_t ld_out, int n, int64_t* next, int32_t* taken, int64_t* hist,
                      int64_t hist_ld, int hist_col, void* stream);

/* ------------------------------------------------------------------------------------------
 * Data-parallel gradient exchange: the MEAN over ranks of the flat fp32 gradient arena as one
 * RCCL all-reduce (ncclAvg) on `stream`, in place — what DDP's bucketed reducer does for the reference (accelerate
 * `accelerator.py:1892`; loss semantics: each rank's loss is its own token mean, gradients are averaged over ranks, hazard H8).
 * For hosts without torch.distributed (the Python host layer issues the same collective through torch's RCCL binding):
 *   rank 0: desta_comm_get_unique_id(&id); hand the 128 bytes to every rank (any channel);
 *   every rank (its device current): desta_comm_create(&comm, world, rank, &id);
 *   every step: desta_allreduce_grads(comm, arena_grads, n, stream) between backward and desta_clip_adafactor_step (or desta_clip_adamw_step);
 *   desta_comm_destroy(comm).
 * RCCL is loaded on first use (dlopen): the other entry points need no RCCL on the box.  One process per GPU. */
typedef struct { char internal[128]; } desta_comm_unique_id;        /* = ncclUniqueId */
typedef void* desta_comm;                                            /* = ncclComm_t */
int desta_comm_get_unique_id(desta_comm_unique_id* id);
int desta_comm_create(desta_comm* comm, int world_size, int rank, const desta_comm_unique_id* id);
int desta_allreduce_grads(desta_comm comm, float* grads, int64_t n, void* stream);
int desta_comm_destroy(desta_comm comm);

#ifdef __cplusplus
}
#endif
#endif /* DESTA_HIP_H */
