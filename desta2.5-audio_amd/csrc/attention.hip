// Flash-style attention for the three attention shapes of the DeSTA2.5 step on gfx950 (MFMA 32x32x16,
// fp32 online softmax, no S x S matrix in HBM), forward + backward:
//   Whisper encoder self-attention (non-causal, D=64)   TF:models/whisper/modeling_whisper.py:241-357
//   Q-Former self-/cross-attention (non-causal, D=64)   TF:models/bert/modeling_bert.py:100-293 (eager)
//   Llama / Qwen3 GQA causal attention with left-pad key mask (D=128 or 64)
//                                                       TF:models/llama/modeling_llama.py:179-281
// and their autograd backward (dQ, dK, dV).
//
// Orientation ("key on the register rows, query on the lane"): S^T = K·Q^T is computed with K as the
// MFMA A operand (ds_read_b128 rows of an XOR-swizzled LDS image) and Q as the B operand (registers),
// so every lane owns ONE query column: row max / row sum / rescale are lane-local scalars.  The fp32
// S^T accumulator converts pairwise to bf16 and is used directly as the B operand of O^T += V^T·P^T
// (no LDS round trip); V^T fragments come from the row-major V image with ds_read_b64_tr_b16.
// K/V tiles are register-staged (global load of tile t+1 issued before the MFMAs of tile t).
// Backward = two kernels without atomics (deterministic): dq (same skeleton as forward) and dkdv
// (one wave owns 32 keys, sweeps the query heads of its GQA group and 32-row query slices).
//
// Fully masked query rows (left-pad positions) produce O = 0 and lse = +inf (their gradients are 0).
#include "common.h"
#include <mutex>
#include "desta_hip.h"

#ifndef ATTN_ABL
#define ATTN_ABL 0     /* forward-kernel timing ablations for tools/attn_bench.py (results are garbage): 1 no LDS stores, 2 no global
                          loads in the loop, 3 no exp, 4 one S MFMA step, 5 one P.V MFMA column block */
#endif

namespace {

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

struct AttnArgs {
    const bf16_t* Q; const bf16_t* K; const bf16_t* V; bf16_t* O;
    const bf16_t* dO; bf16_t* dQ; bf16_t* dK; bf16_t* dV;
    float* lse; const float* delta;
    float* O32;                                                      // optional fp32 copy of O (same strides as O): delta = rowsum(dO * O) from the UNROUNDED output
    const float* rope_cs;                                            // bwd: [seq][D/2][2] (cos, sin): dQ / dK are rotated back (adjacent-pair layout) before the store
    long q_bs, q_rs, k_bs, k_rs, v_bs, v_rs, o_bs, o_rs;           // batch / row strides (elements)
    long do_bs, do_rs, dq_bs, dq_rs, dk_bs, dk_rs, dv_bs, dv_rs;
    int B, Hq, Hkv, Sq, Sk;
    int causal;
    const int* kv_start;                                             // [B] first valid key (left padding) or null
    float scale_log2;                                                // softmax scale * log2(e)
    float scale;
    unsigned drop_thresh, seed_lo, seed_hi; float drop_scale;       // attention-probability dropout (DROP kernels)
    long dkv_t_ld;                                                   // one-query-tile backward: dK / dV stored transposed ([head * 64 + d][dkv_t_ld], column = batch * Sk + key); 0 = off
};

template <int D>
__device__ __forceinline__ int img_off(int row, int ch) {
    const int sw = (D == 128) ? (((row & 3) << 2) | ((row >> 2) & 3)) : ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
    return row * (D * 2) + ((ch ^ sw) << 4);
}

// Register stage of a ROWS x D bf16 tile: N = ROWS*D/8/256 16-B chunks per thread held in ONE first-class
// vector value (ext_vector_type) — an array here ends up in scratch once two stages are alive
// (hipcc keeps allocas that are conditionally re-loaded inside the unrolled-by-two loop in memory).
template <int N> struct stage_vec;
template <> struct stage_vec<1> { typedef __attribute__((ext_vector_type(4))) unsigned type; };
template <> struct stage_vec<2> { typedef __attribute__((ext_vector_type(8))) unsigned type; };
template <> struct stage_vec<4> { typedef __attribute__((ext_vector_type(16))) unsigned type; };
template <int D, int ROWS, int NT = 256> using stage_t = typename stage_vec<ROWS * (D / 8) / NT>::type;

// global -> registers (16-B chunks), rows clamped to [0, max_row]; NT = threads of the block
template <int D, int ROWS, int NT = 256>
__device__ __forceinline__ stage_t<D, ROWS, NT> tile_load(const bf16_t* base, long rs, int row0, int max_row) {
    constexpr int CH = D / 8, N = ROWS * CH / NT;
    stage_t<D, ROWS, NT> out;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int id = i * NT + threadIdx.x;
        const int r = id / CH, c = id % CH;
        const int gr = min(row0 + r, max_row);
        const uint4 v = *(const uint4*)(base + (long)gr * rs + c * 8);
        out[4 * i + 0] = v.x; out[4 * i + 1] = v.y; out[4 * i + 2] = v.z; out[4 * i + 3] = v.w;
    }
    return out;
}
template <int D, int ROWS, int NT = 256>
__device__ __forceinline__ void tile_store(char* img, const stage_t<D, ROWS, NT>& regs) {
    constexpr int CH = D / 8, N = ROWS * CH / NT;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int id = i * NT + threadIdx.x;
        const int r = id / CH, c = id % CH;
        *(uint4*)(img + img_off<D>(r, c)) = make_uint4(regs[4 * i + 0], regs[4 * i + 1], regs[4 * i + 2], regs[4 * i + 3]);
    }
}

// A operand (32x32x16) read by rows: lane (row = row0 + (lane&31), k = 16*ks + 8*(lane>>5) + j)
template <int D>
__device__ __forceinline__ bf16x8 frag_rows(const char* img, int row0, int ks, int lane) {
    const int r = row0 + (lane & 31);
    return *(const bf16x8*)(img + img_off<D>(r, 2 * ks + (lane >> 5)));
}

// Transposed operand from a row-major [row][col] image: returns, for lane (c = col0 + (lane&31), h = lane>>5),
// the 8 elements img[row0 + 8*(j>>2) + 4*h + (j&3)][c], j = 0..7  (the k order of an accumulator-fed MFMA).
template <int D>
__device__ __forceinline__ bf16x8 frag_tr(const char* img, int row0, int col0, int lane) {
    const int i = lane & 15, g = (lane >> 4) & 1, h = lane >> 5;
    const int q = i >> 2, pp = i & 3;
    const int c = col0 + 16 * g + 4 * pp;                  // first column of this lane's 4-element piece
    const int r_lo = row0 + 4 * h + q;
    const int a0 = img_off<D>(r_lo, c >> 3) + ((c & 4) << 1);
    const int a1 = img_off<D>(r_lo + 8, c >> 3) + ((c & 4) << 1);
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(img + a0));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(img + a1));
    bf16x8 out;
    out[0] = lo[0]; out[1] = lo[1]; out[2] = lo[2]; out[3] = lo[3];
    out[4] = hi[0]; out[5] = hi[1]; out[6] = hi[2]; out[7] = hi[3];
    return out;
}

// accumulator registers 8s..8s+7 -> bf16 fragment of k-step s
__device__ __forceinline__ bf16x8 acc_frag(const f32x16& x, int s) {
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (__bf16)x[8 * s + j];
    return o;
}

__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

// XCD-aware work order for the query-block kernels.  Blocks are dealt round-robin over the 8 XCDs (block id % 8), each with
// its own L2: with (q-block, head, batch) = blockIdx the q-blocks of one (batch, head) landed on 8 different XCDs and every
// XCD fetched that head's K / V for itself (rocprofv3 FETCH_SIZE of the Whisper shape: 528 MB per launch against 92 MB of
// Q, K, V).  Here XCD x walks the (batch, kv head) groups g = x, x + 8, ... and, inside a group, the query heads of the GQA
// group and their q-blocks back to back, so the K / V tiles of a group are re-read from that XCD's L2.  Speed only: any
// placement is correct.  Causal: q-blocks in descending order (most keys first).
// What a wave of a query-block kernel works on: batch, kv head, query head, first row of the block and of the wave, this
// lane's row.  wave_on (8-wave blocks): false for a wave past the ragged end, which only helps staging.
struct QWork { int b, hk, h, qb0, q0, qcol; bool wave_on; };

// four-wave (two-wave) blocks: NW * 32 rows of one head
template <int NW>
__device__ __forceinline__ QWork attn_work_item(const AttnArgs& p, int wave, int lane) {
    constexpr int QB = 32 * NW;
    const int nq = (p.Sq + QB - 1) / QB;
    const int id = blockIdx.x, per = nq * (p.Hq / p.Hkv), ngrp = p.B * p.Hkv;       // per = blocks of one (batch, kv head) group
    int g, r;
    if ((ngrp & 7) == 0) {
        const int xcd = id & 7, slot = id >> 3;
        g = (slot / per) * 8 + xcd;
        r = slot % per;
    } else {
        g = id / per;
        r = id % per;
    }
    QWork w;
    w.b = g / p.Hkv;
    w.h = (g % p.Hkv) * (p.Hq / p.Hkv) + r / nq;
    int qblk = r % nq;
    if (p.causal) qblk = nq - 1 - qblk;
    w.qb0 = qblk * QB; w.q0 = w.qb0 + wave * 32;
    w.hk = w.h / (p.Hq / p.Hkv);
    w.qcol = w.q0 + (lane & 31);
    w.wave_on = true;
    return w;
}

// eight-wave blocks: HPB heads of one GQA group x 256 / HPB rows.  Causal launches the heaviest q-blocks of all groups first
// (the K / V of an XCD's groups fit its L2 together), non-causal keeps the q-blocks of a group back to back.
template <bool CAUSAL, int HPB>
__device__ __forceinline__ QWork attn_work_item8(const AttnArgs& p, int wave, int lane) {
    constexpr int RB = 256 / HPB, WPH = RB / 32;                   // query rows of a block (per head), waves per head
    const int G = p.Hq / p.Hkv, nq = (p.Sq + RB - 1) / RB, hgroups = G / HPB, ngrp = p.B * p.Hkv;
    int g, qblk, hg;
    const int id = blockIdx.x, per = nq * hgroups;
    if ((ngrp & 7) == 0) {
        const int xcd = id & 7, slot = id >> 3, gpx = ngrp >> 3;
        if (CAUSAL) {
            const int r = slot % (hgroups * gpx);
            qblk = nq - 1 - slot / (hgroups * gpx); hg = r / gpx; g = (r % gpx) * 8 + xcd;
        } else {
            const int r = slot % per;
            g = (slot / per) * 8 + xcd; hg = r / nq; qblk = r % nq;
        }
    } else if (CAUSAL) {
        const int r = id % (hgroups * ngrp);
        qblk = nq - 1 - id / (hgroups * ngrp); hg = r / ngrp; g = r % ngrp;
    } else {
        const int r = id % per;
        g = id / per; hg = r / nq; qblk = r % nq;
    }
    QWork w;
    w.b = g / p.Hkv; w.hk = g % p.Hkv;
    w.h = w.hk * G + hg * HPB + wave / WPH;
    w.qb0 = qblk * RB; w.q0 = w.qb0 + (wave % WPH) * 32;
    w.qcol = w.q0 + (lane & 31);
    w.wave_on = w.q0 < p.Sq;                                       // scalar
    return w;
}

// Keys a query block of QB rows walks, and what one of its waves and lanes may see.  `causal` is a compile-time constant in the
// 8-wave kernels and p.causal in the others.
struct KeyRange {
    int coff, kv_lo;          // query row q sits on key q + coff; first valid key (left padding)
    int t_lo, t_hi;           // 64-key tiles [t_lo, t_hi) of the block
    int q0, q_abs;            // the wave's first row; last key this lane's row sees under the causal mask
    int wave_kmax;            // last key any row of this wave may see
};
__device__ __forceinline__ KeyRange attn_key_range(const AttnArgs& p, int causal, const QWork& w, int QB) {
    KeyRange k;
    k.coff = p.Sk - p.Sq;
    k.kv_lo = p.kv_start ? max(0, min(p.kv_start[w.b], p.Sk)) : 0;
    int kv_hi = p.Sk;
    if (causal) kv_hi = min(p.Sk, min(w.qb0 + QB - 1, p.Sq - 1) + k.coff + 1);
    k.t_lo = k.kv_lo / 64; k.t_hi = (kv_hi + 63) / 64;
    k.q0 = w.q0; k.q_abs = w.qcol + k.coff;
    k.wave_kmax = causal ? min(w.q0 + 31, p.Sq - 1) + k.coff : p.Sk - 1;
    return k;
}

// Key visibility (ragged Sk, left padding, causal diagonal) of NH 32-key accumulators that start at key0: masked scores become
// -inf (exp2(-inf) = 0).  Boundary tiles only: the guard is wave-uniform and stays a BRANCH through the asm (hipcc otherwise
// if-converts the compares + selects into every tile's straight-line code).
template <int NH>
__device__ __forceinline__ void mask_keys(f32x16* st, const AttnArgs& p, int causal, const KeyRange& k, int key0, int lane) {
    const bool need_mask = (key0 + 32 * NH - 1 >= p.Sk) || (key0 < k.kv_lo) || (causal && key0 + 32 * NH - 1 > k.q0 + k.coff);
    if (need_mask) {
        asm volatile("; boundary tile" ::: "memory");
#pragma unroll
        for (int kb = 0; kb < NH; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int key = key0 + kb * 32 + acc_row(r, lane);
                const bool ok = key < p.Sk && key >= k.kv_lo && (!causal || key <= k.q_abs);
                st[kb][r] = ok ? st[kb][r] : -INFINITY;
            }
    }
}

// K / V tile walk of the four-wave kernels: both tiles register-staged PF tiles ahead (PF = 2: two register sets), one LDS
// image each, two barriers per tile, the loop unrolled by two.  compute(kt) runs between a tile's store and the next one's.
// ABL: the forward's timing ablations (ATTN_ABL); 0 everywhere else.
template <int D, int NW, int PF, int ABL, class Compute>
__device__ __forceinline__ void kv_tile_walk(const AttnArgs& p, const QWork& w, const KeyRange& k, char* kimg, char* vimg, Compute compute) {
    constexpr int NT = 64 * NW;
    const bf16_t* kbase = p.K + (long)w.b * p.k_bs + (long)w.hk * D;
    const bf16_t* vbase = p.V + (long)w.b * p.v_bs + (long)w.hk * D;
    const int t_lo = k.t_lo, t_hi = k.t_hi;
    stage_t<D, 64, NT> kr0 = {}, vr0 = {}, kr1 = {}, vr1 = {};
    if (t_lo < t_hi) {
        kr0 = tile_load<D, 64, NT>(kbase, p.k_rs, t_lo * 64, p.Sk - 1);
        vr0 = tile_load<D, 64, NT>(vbase, p.v_rs, t_lo * 64, p.Sk - 1);
    }
    if (PF == 2 && t_lo + 1 < t_hi) {
        kr1 = tile_load<D, 64, NT>(kbase, p.k_rs, (t_lo + 1) * 64, p.Sk - 1);
        vr1 = tile_load<D, 64, NT>(vbase, p.v_rs, (t_lo + 1) * 64, p.Sk - 1);
    }
#define DESTA_KV_STAGE(KT, KR, VR)                                                   \
    __syncthreads(); /* previous tile's LDS reads are done */                        \
    asm volatile("; stage " #KR ::: "memory"); /* distinct text: keeps the two halves from being tail-merged */ \
    if (ABL != 1 || (KT) == t_lo) {                                                  \
        tile_store<D, 64, NT>(kimg, KR);                                             \
        tile_store<D, 64, NT>(vimg, VR);                                             \
    }                                                                                \
    __syncthreads();                                                                 \
    if (ABL != 2 && (KT) + PF < t_hi) {                                              \
        KR = tile_load<D, 64, NT>(kbase, p.k_rs, ((KT) + PF) * 64, p.Sk - 1);        \
        VR = tile_load<D, 64, NT>(vbase, p.v_rs, ((KT) + PF) * 64, p.Sk - 1);        \
    }
    for (int kt = t_lo; kt < t_hi; kt += 2) {
        DESTA_KV_STAGE(kt, kr0, vr0)
        compute(kt);
        if (kt + 1 < t_hi) {
            if constexpr (PF == 2) {
                DESTA_KV_STAGE(kt + 1, kr1, vr1)
            } else {
                DESTA_KV_STAGE(kt + 1, kr0, vr0)
            }
            compute(kt + 1);
        }
    }
#undef DESTA_KV_STAGE
}

// this lane's row of a [d][query] fp32 accumulator -> bf16, as 8-byte pieces (registers 4 rq .. 4 rq + 3: d = 32 i + 8 rq + 4 h2 + e)
template <int D>
__device__ __forceinline__ void store_row_bf16(bf16_t* row, const f32x16* acc, int h2) {
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            u16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = f2bf(acc[i][4 * rq + e]);
            *(u16x4*)(row + i * 32 + 8 * rq + 4 * h2) = o;
        }
}
// the same row as 16-byte pieces (guide T21).  Registers 8j..8j+3: d = 32i + 16j + 4*h2 + e; 8j+4..8j+7: d = 32i + 16j + 8 + 4*h2 + e.
// After a permlane32 exchange of the packed halves a lane of the lower half holds d = 32i + 16j + 0..7, its partner in the upper
// half 32i + 16j + 8..15: one 16-byte store each
template <int D>
__device__ __forceinline__ void store_row_bf16_16B(bf16_t* row, const f32x16* acc, int h2) {
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            unsigned a[2], c[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                a[e] = (unsigned)f2bf(acc[i][8 * j + 2 * e]) | ((unsigned)f2bf(acc[i][8 * j + 2 * e + 1]) << 16);
                c[e] = (unsigned)f2bf(acc[i][8 * j + 4 + 2 * e]) | ((unsigned)f2bf(acc[i][8 * j + 4 + 2 * e + 1]) << 16);
            }
            const auto r0 = __builtin_amdgcn_permlane32_swap(a[0], c[0], false, false);
            const auto r1 = __builtin_amdgcn_permlane32_swap(a[1], c[1], false, false);
            *(uint4*)(row + i * 32 + 16 * j + 8 * h2) = make_uint4(r0[0], r1[0], r0[1], r1[1]);
        }
}
// and as fp32 (desta_attn_desc.O_f32)
template <int D>
__device__ __forceinline__ void store_row_f32(float* row, const f32x16* acc, int h2) {
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq)
            *(f32x4*)(row + i * 32 + 8 * rq + 4 * h2) = f32x4{acc[i][4 * rq], acc[i][4 * rq + 1], acc[i][4 * rq + 2], acc[i][4 * rq + 3]};
}

// ------------------------------------------------------------------------------------------ forward
// Occupancy beats prefetch depth here (measured, tools/attn_bench.py): with K/V register-staged ONE tile ahead the
// kernel fits 256 VGPRs at D=128 (160 at D=64) -> 2 (3) blocks per CU, whose MFMA / softmax / staging phases overlap
// each other: LLM shape 104 -> 69 us, Whisper shape 190 -> 157 us vs two tiles ahead at one block per CU.
#ifndef ATTN_FWD_PF
#define ATTN_FWD_PF 1
#endif
// NW = waves per block (32 query rows each): 4, or 2 for Sq <= 64 (the Q-Former's 64 prompt queries: with 4 waves half of
// every block computed clamped duplicate rows, and 640 four-wave blocks left most of the chip's wave slots empty)
#ifndef ATTN_FWD64_WAVES
#define ATTN_FWD64_WAVES 3
#endif
template <int D, bool DROP, int NW = 4>
__global__ __launch_bounds__(64 * NW, NW == 4 ? (D == 64 ? ATTN_FWD64_WAVES : 2) : 2) void attn_fwd_k(AttnArgs p) {
    constexpr int QB = 32 * NW;
    __shared__ __attribute__((aligned(16))) char lds[2 * 64 * D * 2];
    char* kimg = lds;
    char* vimg = lds + 64 * D * 2;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h2 = lane >> 5;    // wave index in an SGPR: everything derived from it (q0, mask tests) is scalar -> real branches
    const QWork w = attn_work_item<NW>(p, wave, lane);
    const int b = w.b, h = w.h, qcol = w.qcol;

    const bf16_t* qptr = p.Q + (long)b * p.q_bs + (long)min(qcol, p.Sq - 1) * p.q_rs + (long)h * D;
    bf16x8 qf[D / 16];
#pragma unroll
    for (int ds = 0; ds < D / 16; ++ds) qf[ds] = *(const bf16x8*)(qptr + 16 * ds + 8 * h2);

    const KeyRange rng = attn_key_range(p, p.causal, w, QB);

    f32x16 oacc[D / 32];
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m = -INFINITY, l = 0.f;

    auto compute = [&](const int kt) __attribute__((always_inline)) {
        if (kt * 64 > rng.wave_kmax) return;               // wave-uniform: nothing visible in this tile
        f32x16 st[2];
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[kb][r] = 0.f;
        {
            // K fragments of the first 32 keys are all read before the first MFMA; those of the second 32 keys are read while
            // the first chain runs (hipcc otherwise emits read -> wait -> MFMA pairs: one exposed LDS latency per MFMA)
            constexpr int NS = (ATTN_ABL == 4 ? 1 : D / 16);
            bf16x8 ka[NS], kbf[NS];
#pragma unroll
            for (int ds = 0; ds < NS; ++ds) ka[ds] = frag_rows<D>(kimg, 0, ds, lane);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ds = 0; ds < NS; ++ds) {
                st[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[ds], qf[ds], st[0], 0, 0, 0);
                kbf[ds] = frag_rows<D>(kimg, 32, ds, lane);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int ds = 0; ds < NS; ++ds) st[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kbf[ds], qf[ds], st[1], 0, 0, 0);
        }
        mask_keys<2>(st, p, p.causal, rng, kt * 64, lane);
        float tmax = -INFINITY;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, st[kb][r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * p.scale_log2;         // scale > 0: max commutes
        const float mnew = fmaxf(m, tmax);
        const float muse = (mnew == -INFINITY) ? 0.f : mnew;
        const float alpha = __builtin_amdgcn_exp2f(m - muse);
        // score -> exponent argument and the row sum on register PAIRS (v_pk_fma_f32 / v_pk_add_f32: half the VALU instructions
        // of the two passes; the kernel is bound by instruction issue)
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        f32x2 rs2 = {0.f, 0.f};
        const f32x2 sc2 = {p.scale_log2, p.scale_log2}, nm2 = {-muse, -muse};
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const f32x2 sv = {st[kb][r], st[kb][r + 1]};
                const f32x2 av = sv * sc2 + nm2;
                f32x2 pv;
                pv.x = ATTN_ABL == 3 ? sv.x : __builtin_amdgcn_exp2f(av.x);
                pv.y = ATTN_ABL == 3 ? sv.y : __builtin_amdgcn_exp2f(av.y);
                st[kb][r] = pv.x;
                st[kb][r + 1] = pv.y;
                rs2 += pv;
            }
        float rs = rs2.x + rs2.y;
        rs += __shfl_xor(rs, 32, 64);
        l = l * alpha + rs;
        if constexpr (DROP) {
            // inverted dropout of the probabilities that enter P·V (the normaliser l keeps the full sum).  Accumulator
            // registers 2j, 2j+1 are ADJACENT keys = one element pair = one hash (common.h; Sk even is checked on the host)
            const unsigned long rowbase = (((unsigned long)b * p.Hq + h) * p.Sq + min(qcol, p.Sq - 1)) * p.Sk;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const unsigned long i0 = rowbase + (kt * 64 + kb * 32 + acc_row(r, lane));
                    const unsigned hsh = desta_rng32(p.seed_lo, p.seed_hi, i0 >> 1);     // Sk is even (host check): i0 is even
                    st[kb][r] = (hsh & 0xffffu) >= p.drop_thresh ? st[kb][r] * p.drop_scale : 0.f;
                    st[kb][r + 1] = (hsh >> 16) >= p.drop_thresh ? st[kb][r + 1] * p.drop_scale : 0.f;
                }
        }
        if (__any(mnew != m)) {                            // rescale only when some row's max moved
#pragma unroll
            for (int i = 0; i < D / 32; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
        }
        m = mnew;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 pb = acc_frag(st[kb], s);
#pragma unroll
                for (int i = 0; i < (ATTN_ABL == 5 ? 1 : D / 32); ++i)
                    oacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr<D>(vimg, kb * 32 + 16 * s, i * 32, lane), pb, oacc[i], 0, 0, 0);
            }
    };
    kv_tile_walk<D, NW, ATTN_FWD_PF, ATTN_ABL>(p, w, rng, kimg, vimg, compute);

    if (qcol < p.Sq) {
        const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
        for (int i = 0; i < D / 32; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[i][r] *= inv;
        store_row_bf16<D>(p.O + (long)b * p.o_bs + (long)qcol * p.o_rs + (long)h * D, oacc, h2);
        if (p.O32) store_row_f32<D>(p.O32 + (long)b * p.o_bs + (long)qcol * p.o_rs + (long)h * D, oacc, h2);
        if (p.lse && h2 == 0) p.lse[((long)b * p.Hq + h) * p.Sq + qcol] = l > 0.f ? m + log2f(l) : INFINITY;
    }
}

// ------------------------------------------------------------------------------------------ forward, 8 waves per block
// The forward for long query ranges (LLM prefill / training: D = 128 causal GQA; Whisper: D = 64, 1500 x 1500).  Same
// orientation as above (key on the accumulator rows, query on the lane, P^T straight from the S^T accumulator into the P.V
// MFMAs), restructured around what the four-wave kernel spends its time on (rocprofv3: mfma-busy 0.18-0.29; per 64-key tile and
// wave 32 MFMAs beside ~330 VALU instructions, and the two waves of a SIMD doing the same phase at the same time):
//   * EIGHT waves share one K / V tile: a block is 256 query rows of one head or, under GQA, HPB heads x 256 / HPB rows of one
//     kv head (the heads of a group read the same K / V): half / a quarter of the staging work per unit of MFMA work, and
//     under the causal mask 64- or 128-row blocks waste less of the diagonal tiles;
//   * LDS double buffer, ONE raw s_barrier per tile (no vmcnt drain): tile t+1 is written to the other buffer in the middle of
//     tile t from registers loaded one tile earlier, and the global loads of tile t+2 are issued right behind it: every load
//     has a whole tile of compute to land;
//   * (STAGGER = true, off by default: measured) waves 4-7 — the SIMD partners of waves 0-3 — half a tile behind, on a
//     three-slot ring: between two barriers waves 0-3 do [S, softmax, P.V] of tile t, waves 4-7 [P.V of t-1, S, softmax of t].
//     Equal on the LLM shape (55.9 vs 55.3 us), SLOWER on the Whisper shape (154 vs 120 us): the partners de-synchronise by
//     themselves once one of them is ahead in its MFMA chain, and the forced pairing is worse than the one that forms;
//   * deferred rescale (guide T13): the running reference m only moves when some row's tile maximum exceeds it by more than
//     2^ATTN_DEFER_LOG2: on all other tiles there is no alpha, no O rescale, no l rescale (P <= 2^ATTN_DEFER_LOG2: relative bf16
//     rounding is unchanged, sums stay far inside fp32 range);
//   * softmax VALU diet: row maximum by v_max3 written as asm (fmaxf on MFMA results makes hipcc canonicalise every operand
//     with an extra v_max: 51 instead of 16 instructions), one v_permlane32_swap to cross the half-waves, the row sum kept as a
//     per-lane partial (the halves are combined once, in the epilogue); LDS read addresses and the per-thread staging offsets
//     are computed once (one add of the slot base per read; global loads use a scalar tile base + 32-bit lane offset);
//   * O is stored as 16-byte pieces after a permlane32 exchange of the packed halves (guide T21).
// Work order: XCD x walks the (batch, kv head) groups x, x + 8, ...; causal launches the heaviest q-blocks of all its groups
// first (the K / V of an XCD's ten groups fit its L2 together), non-causal keeps the q-blocks of a group back to back.
#ifndef ATTN_DEFER_LOG2
#define ATTN_DEFER_LOG2 6.0f
#endif
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float vmax2(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float swap_halves_max(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);     // r[0] = [lo, lo], r[1] = [hi, hi]
    return vmax2(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
}
__device__ __forceinline__ float swap_halves_sum(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}
__device__ __forceinline__ bf16x8 tr_pair(const char* lo, const char* hi) {
    const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)lo);
    const bf16x4 c = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)hi);
    return __builtin_shufflevector(a, c, 0, 1, 2, 3, 4, 5, 6, 7);            // one register tuple: no element-wise moves
}

// K | V staging stream of the 8-wave kernels: 512 threads move one 64-key tile of both tensors, global -> registers ->
// a ring slot [K image, V image] of the block's LDS.
template <int D>
struct KVStream8 {
    static constexpr int NT = 512, TILE = 64 * D * 2;              // bytes of one 64-key K (or V) image
    static constexpr int NCH = 64 * (D / 8) / NT;                  // 16-byte chunks per thread, tile and tensor (2 / 1)
    const char* kbase; const char* vbase;
    // this thread's NCH chunks of a tile: (row r, chunk c) -> byte offset from the tile's first row (32-bit; the tile base is
    // wave-uniform: scalar base + vector offset loads) and its place in the swizzled LDS image
    int srow[NCH], sdst[NCH];
    unsigned ksrc[NCH], vsrc[NCH];
    // ONE first-class vector value per tensor (an array that is conditionally re-loaded inside the loop is kept in memory by
    // hipcc — promoted to LDS here: every load was waited for and parked in LDS right behind its issue)
    typename stage_vec<NCH>::type kr, vr;

    __device__ __forceinline__ KVStream8(const AttnArgs& p, const QWork& w) : kr{}, vr{} {
        kbase = (const char*)(p.K + (long)w.b * p.k_bs + (long)w.hk * D);
        vbase = (const char*)(p.V + (long)w.b * p.v_bs + (long)w.hk * D);
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int id = i * NT + threadIdx.x, r = id / (D / 8), c = id % (D / 8);
            srow[i] = r;
            sdst[i] = img_off<D>(r, c);
            ksrc[i] = (unsigned)(r * (int)p.k_rs + c * 8) * 2u;
            vsrc[i] = (unsigned)(r * (int)p.v_rs + c * 8) * 2u;
        }
    }
    // global -> registers.  Rows are clamped: the loads are legal even when the block has no tile at all
    __device__ __forceinline__ void load_tile(const AttnArgs& p, const int kt) {
        const char* kb_ = kbase + (long)kt * 64 * p.k_rs * 2;
        const char* vb_ = vbase + (long)kt * 64 * p.v_rs * 2;
        const bool ragged = kt * 64 + 64 > p.Sk;                    // last tile (or a block without tiles): clamp the rows
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            unsigned ko = ksrc[i], vo = vsrc[i];
            if (ragged) {
                const int rc = max(min(srow[i], p.Sk - 1 - kt * 64), -kt * 64), c = (i * NT + (int)threadIdx.x) % (D / 8);
                ko = (unsigned)(rc * (int)p.k_rs + c * 8) * 2u;     // (rc < 0 only when the block has no tile: row 0 of the tensor)
                vo = (unsigned)(rc * (int)p.v_rs + c * 8) * 2u;
            }
            const uint4 a = *(const uint4*)(kb_ + (long)(int)ko), c4 = *(const uint4*)(vb_ + (long)(int)vo);
            kr[4 * i + 0] = a.x; kr[4 * i + 1] = a.y; kr[4 * i + 2] = a.z; kr[4 * i + 3] = a.w;
            vr[4 * i + 0] = c4.x; vr[4 * i + 1] = c4.y; vr[4 * i + 2] = c4.z; vr[4 * i + 3] = c4.w;
        }
    }
    __device__ __forceinline__ void store_tile(char* slot) const {
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            *(uint4*)(slot + sdst[i]) = make_uint4(kr[4 * i + 0], kr[4 * i + 1], kr[4 * i + 2], kr[4 * i + 3]);
            *(uint4*)(slot + TILE + sdst[i]) = make_uint4(vr[4 * i + 0], vr[4 * i + 1], vr[4 * i + 2], vr[4 * i + 3]);
        }
    }
    // tile kt+1: registers -> its ring slot (last read two barriers ago); then the global loads of tile kt+2
    __device__ __forceinline__ void advance(const AttnArgs& p, const int kt, const int t_hi, char* slot_next) {
        if (kt + 1 < t_hi) {
            store_tile(slot_next);
            if (kt + 2 < t_hi) load_tile(p, kt + 2);
        }
    }
};

// LDS read addresses inside a ring slot (lane constants; "+v": keep them in registers instead of re-deriving them per tile):
// kofs: rows 0..31 of an image as the A operand (rows 32..63: + 32 rows, same swizzle); tofs: the transposed operand from the image
// at byte `tbase` of the slot, rows r0 + 4 h2 + q and + 8 (r0 = multiples of 16: same swizzle)
template <int D>
__device__ __forceinline__ void lds_read_offsets(int lane, int tbase, int (&kofs)[D / 16], int (&tofs)[D / 32][2]) {
    const int h2 = lane >> 5;
#pragma unroll
    for (int ds = 0; ds < D / 16; ++ds) {
        kofs[ds] = img_off<D>(lane & 31, 2 * ds + h2);
        asm volatile("" : "+v"(kofs[ds]));
    }
    const int i16 = lane & 15, gq = (lane >> 4) & 1, qq = i16 >> 2, pp = i16 & 3;
#pragma unroll
    for (int i = 0; i < D / 32; ++i) {
        const int c = i * 32 + 16 * gq + 4 * pp;
        tofs[i][0] = tbase + img_off<D>(4 * h2 + qq, c >> 3) + ((c & 4) << 1);
        tofs[i][1] = tbase + img_off<D>(4 * h2 + qq + 8, c >> 3) + ((c & 4) << 1);
        asm volatile("" : "+v"(tofs[i][0]), "+v"(tofs[i][1]));
    }
}

// one barrier per tile: LDS traffic of this wave is done; global loads stay in flight (no vmcnt drain)
__device__ __forceinline__ void attn_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// MINW = 4 (D = 64 only): two 8-wave blocks per CU (<= 128 registers)
template <int D, bool CAUSAL, int HPB, int MINW = 2, bool STAGGER = false>
__global__ __launch_bounds__(512, MINW) void attn_fwd8_k(AttnArgs p) {
    constexpr int RB = 256 / HPB;                                  // query rows of a block (per head)
    constexpr int TILE = KVStream8<D>::TILE;
    constexpr int SLOT = 2 * TILE, NSLOT = STAGGER ? 3 : 2;        // lockstep: double buffer; staggered: tile t-1's V is still read while t+1 is written
    __shared__ __attribute__((aligned(16))) char lds[NSLOT * SLOT];   // ring of [K image, V image]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h2 = lane >> 5;
    const QWork w = attn_work_item8<CAUSAL, HPB>(p, wave, lane);
    const int b = w.b, h = w.h, qcol = w.qcol;
    const bool wave_on = w.wave_on;
    const KeyRange rng = attn_key_range(p, CAUSAL, w, RB);
    const int t_lo = rng.t_lo, t_hi = rng.t_hi;
    KVStream8<D> kv(p, w);

    // prologue, straight-line on purpose: first K / V tile, then the Q fragments; loads return in order, so once the Q
    // fragments are in (the empty asm makes the compiler wait for them HERE) nothing of the prologue is still in flight and
    // the loop's vmcnt bookkeeping covers only the K / V stream (with the Q loads pending at the loop head hipcc makes every
    // tile's S MFMAs wait for vmcnt(3..0), i.e. for the loads of tile t+2 issued half a tile earlier).  Rows are clamped:
    // the loads are legal even when the block has no tile at all.
    kv.load_tile(p, t_lo);
    const bf16_t* qptr = p.Q + (long)b * p.q_bs + (long)min(qcol, p.Sq - 1) * p.q_rs + (long)h * D;
    bf16x8 qf[D / 16];
#pragma unroll
    for (int ds = 0; ds < D / 16; ++ds) qf[ds] = *(const bf16x8*)(qptr + 16 * ds + 8 * h2);
#pragma unroll
    for (int ds = 0; ds < D / 16; ++ds) asm volatile("" :: "v"(qf[ds]));
    kv.store_tile(lds);
    kv.load_tile(p, t_lo + 1);

    int kofs[D / 16], vofs[D / 32][2];                              // K rows as the A operand; V^T from the V image
    lds_read_offsets<D>(lane, TILE, kofs, vofs);

    f32x16 oacc[D / 32];
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[i][r] = 0.f;
    float m = -INFINITY, l = 0.f;                                   // m: reference in scaled log2 units (may lag the true maximum by <= 2^DEFER); l: this lane's partial sum
    f32x16 st[2];                                                   // S^T of the current tile, then its probabilities (waves 4-7 carry them across the barrier)
    attn_barrier();

    // S^T = K Q^T of tile kt (slot base `sb`), boundary masks, deferred-rescale online softmax: st := probabilities
    auto scores = [&](const int kt, const int sb) __attribute__((always_inline)) {
        if (!(wave_on && kt * 64 <= rng.wave_kmax)) return;         // scalar
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[kb][r] = 0.f;
        bf16x8 ka[D / 16], kbf[D / 16];
        int kad[D / 16];                                            // ONE add of the slot base per address register; the rest are immediates
#pragma unroll
        for (int ds = 0; ds < D / 16; ++ds) { kad[ds] = kofs[ds] + sb; asm volatile("" : "+v"(kad[ds])); }
#pragma unroll
        for (int ds = 0; ds < D / 16; ++ds) ka[ds] = *(const bf16x8*)(lds + kad[ds]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ds = 0; ds < D / 16; ++ds) {
            st[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka[ds], qf[ds], st[0], 0, 0, 0);
            kbf[ds] = *(const bf16x8*)(lds + kad[ds] + 32 * D * 2);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ds = 0; ds < D / 16; ++ds) st[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kbf[ds], qf[ds], st[1], 0, 0, 0);
        mask_keys<2>(st, p, CAUSAL, rng, kt * 64, lane);
        float tmax = vmax3(st[0][0], st[1][0], st[0][1]);
        tmax = vmax3(tmax, st[1][1], st[0][2]);
#pragma unroll
        for (int r = 2; r < 15; ++r) tmax = vmax3(tmax, st[1][r], st[0][r + 1]);
        tmax = vmax2(tmax, st[1][15]);
        tmax = swap_halves_max(tmax) * p.scale_log2;                                          // scale > 0: max commutes
        if (!__all(!(tmax > m + ATTN_DEFER_LOG2))) {                                          // some row outgrew its reference: move every row's
            const float mnew = vmax2(m, tmax);
            const float alpha = __builtin_amdgcn_exp2f(m - (mnew == -INFINITY ? 0.f : mnew)); // m = -inf: 0 (O = l = 0 anyway)
            l *= alpha;
#pragma unroll
            for (int i = 0; i < D / 32; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[i][r] *= alpha;
            m = mnew;
        }
        const float nmu = (m == -INFINITY) ? 0.f : -m;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                st[kb][r] = __builtin_amdgcn_exp2f(fmaf(st[kb][r], p.scale_log2, nmu));
                l += st[kb][r];
            }
    };
    // O^T += V^T P^T of tile kt
    auto pv = [&](const int kt, const int sb) __attribute__((always_inline)) {
        if (!(wave_on && kt * 64 <= rng.wave_kmax)) return;
        int vad[D / 32][2];
#pragma unroll
        for (int i = 0; i < D / 32; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) { vad[i][j] = vofs[i][j] + sb; asm volatile("" : "+v"(vad[i][j])); }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 pb = acc_frag(st[kb], s);
#pragma unroll
                for (int i = 0; i < D / 32; ++i)
                    oacc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                        tr_pair(lds + vad[i][0] + (kb * 32 + 16 * s) * D * 2, lds + vad[i][1] + (kb * 32 + 16 * s) * D * 2), pb, oacc[i], 0, 0, 0);
            }
    };
    auto next_slot = [](int sb) { return sb == (NSLOT - 1) * SLOT ? 0 : sb + SLOT; };
    int sb = 0;                                                     // slot of tile kt (scalar)
    if (!STAGGER || wave < 4) {
        for (int kt = t_lo; kt < t_hi; ++kt) {
            const int sn = next_slot(sb);
            scores(kt, sb);
            kv.advance(p, kt, t_hi, lds + sn);
            pv(kt, sb);
            attn_barrier();
            sb = sn;
        }
    } else if (t_lo < t_hi) {
        // half a tile behind: the same number of barriers as waves 0-3 (one per tile), P.V of tile kt after the barrier that ends it
        scores(t_lo, sb);
        kv.advance(p, t_lo, t_hi, lds + next_slot(sb));
        attn_barrier();
        for (int kt = t_lo; kt + 1 < t_hi; ++kt) {
            const int sn = next_slot(sb);
            pv(kt, sb);
            kv.advance(p, kt + 1, t_hi, lds + next_slot(sn));
            scores(kt + 1, sn);
            attn_barrier();
            sb = sn;
        }
        pv(t_hi - 1, sb);
    }

    if (wave_on && qcol < p.Sq) {
        const float lt = swap_halves_sum(l);
        const float inv = lt > 0.f ? 1.0f / lt : 0.f;
#pragma unroll
        for (int i = 0; i < D / 32; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[i][r] *= inv;
        store_row_bf16_16B<D>(p.O + (long)b * p.o_bs + (long)qcol * p.o_rs + (long)h * D, oacc, h2);
        if (p.O32) store_row_f32<D>(p.O32 + (long)b * p.o_bs + (long)qcol * p.o_rs + (long)h * D, oacc, h2);
        if (p.lse && h2 == 0) p.lse[((long)b * p.Hq + h) * p.Sq + qcol] = lt > 0.f ? m + log2f(lt) : INFINITY;
    }
}

// delta[b,h,q] = sum_d dO[q,d] * O[q,d]
template <int D>
__global__ __launch_bounds__(256) void attn_delta_k(AttnArgs p, float* __restrict__ delta) {
    constexpr int G = D / 8;                               // lanes per row
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long rowid = gid / G;
    const int j = (int)(gid % G);
    const long total = (long)p.B * p.Hq * p.Sq;
    const bool active = rowid < total;
    const long rr = active ? rowid : 0;
    const int q = (int)(rr % p.Sq), h = (int)((rr / p.Sq) % p.Hq), b = (int)(rr / ((long)p.Sq * p.Hq));
    const u16x8 g = *(const u16x8*)(p.dO + (long)b * p.do_bs + (long)q * p.do_rs + (long)h * D + 8 * j);
    float s = 0.f;
    if (p.O32) {                                           // the unrounded forward output (see desta_attn_desc.O_f32)
        const float* o32 = p.O32 + (long)b * p.o_bs + (long)q * p.o_rs + (long)h * D + 8 * j;
        const f32x4 o0 = *(const f32x4*)o32, o1 = *(const f32x4*)(o32 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += o0[e] * bf2f(g[e]) + o1[e] * bf2f(g[4 + e]);
    } else {
        const u16x8 o = *(const u16x8*)(p.O + (long)b * p.o_bs + (long)q * p.o_rs + (long)h * D + 8 * j);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += bf2f(o[e]) * bf2f(g[e]);
    }
#pragma unroll
    for (int o2 = 1; o2 < G; o2 <<= 1) s += __shfl_xor(s, o2, 64);
    if (active && j == 0) delta[rowid] = s;
}

// ------------------------------------------------------------------------------------------ backward: dQ
// same trade as the forward: one tile ahead + two blocks per CU (131 -> 103 us on the LLM shape; two tiles ahead
// squeezed into 256 registers spills and is slower than either)
#ifndef ATTN_DQ_PF
#define ATTN_DQ_PF 1
#endif
#ifndef ATTN_DQ_BLOCKS
#define ATTN_DQ_BLOCKS 2
#endif
template <int D, bool DROP, int NW = 4>
__global__ __launch_bounds__(64 * NW, NW == 4 ? ATTN_DQ_BLOCKS : 2) void attn_bwd_dq_k(AttnArgs p) {
    constexpr int QB = 32 * NW;
    __shared__ __attribute__((aligned(16))) char lds[2 * 64 * D * 2];
    char* kimg = lds;
    char* vimg = lds + 64 * D * 2;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h2 = lane >> 5;    // wave index in an SGPR: everything derived from it (q0, mask tests) is scalar -> real branches
    const QWork w = attn_work_item<NW>(p, wave, lane);
    const int b = w.b, h = w.h, qcol = w.qcol, qc = min(qcol, p.Sq - 1);

    const bf16_t* qptr = p.Q + (long)b * p.q_bs + (long)qc * p.q_rs + (long)h * D;
    const bf16_t* gptr = p.dO + (long)b * p.do_bs + (long)qc * p.do_rs + (long)h * D;
    bf16x8 qf[D / 16], gf[D / 16];
#pragma unroll
    for (int ds = 0; ds < D / 16; ++ds) {
        qf[ds] = *(const bf16x8*)(qptr + 16 * ds + 8 * h2);
        gf[ds] = *(const bf16x8*)(gptr + 16 * ds + 8 * h2);
    }
    const long stat = ((long)b * p.Hq + h) * p.Sq + qc;
    const float lse = p.lse[stat], dlt = p.delta[stat];

    const KeyRange rng = attn_key_range(p, p.causal, w, QB);

    f32x16 dq[D / 32];
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[i][r] = 0.f;

    auto compute = [&](const int kt) __attribute__((always_inline)) {
        if (kt * 64 > rng.wave_kmax) return;
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            f32x16 st, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int ds = 0; ds < D / 16; ++ds) {
                st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(kimg, kb * 32, ds, lane), qf[ds], st, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(vimg, kb * 32, ds, lane), gf[ds], dp, 0, 0, 0);
            }
            unsigned keep = 0xffffu;                                          // bit r: probability r of this lane survived dropout
            if constexpr (DROP) {
                // registers 2j, 2j+1 hold adjacent keys = one element pair = one hash (common.h; Sk even: host check)
                const unsigned long rowbase = (((unsigned long)b * p.Hq + h) * p.Sq + qc) * p.Sk;
                keep = 0;
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const unsigned long i0 = rowbase + (kt * 64 + kb * 32 + acc_row(r, lane));
                    const unsigned hsh = desta_rng32(p.seed_lo, p.seed_hi, i0 >> 1);
                    keep |= ((hsh & 0xffffu) >= p.drop_thresh ? 1u : 0u) << r;
                    keep |= ((hsh >> 16) >= p.drop_thresh ? 1u : 0u) << (r + 1);
                }
            }
            mask_keys<1>(&st, p, p.causal, rng, kt * 64 + kb * 32, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(fmaf(st[r], p.scale_log2, -lse));
                float dpr = dp[r];
                if constexpr (DROP) dpr = ((keep >> r) & 1u) ? dpr * p.drop_scale : 0.f;
                st[r] = pv * (dpr - dlt) * p.scale;        // dS^T
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 dsf = acc_frag(st, s);
#pragma unroll
                for (int i = 0; i < D / 32; ++i)
                    dq[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr<D>(kimg, kb * 32 + 16 * s, i * 32, lane), dsf, dq[i], 0, 0, 0);
            }
        }
    };
    kv_tile_walk<D, NW, ATTN_DQ_PF, 0>(p, w, rng, kimg, vimg, compute);
    if (qcol < p.Sq) store_row_bf16<D>(p.dQ + (long)b * p.dq_bs + (long)qcol * p.dq_rs + (long)h * D, dq, h2);
}

// ------------------------------------------------------------------------------------------ backward: dQ, 8 waves per block
// attn_fwd8_k's geometry for the dQ pass of long query ranges (seq_q >= 128, no dropout): 8 waves share each K / V tile (HPB
// heads of a GQA group x 256 / HPB query rows), LDS double buffer with ONE raw barrier per tile, loads two tiles ahead in
// registers, heaviest q-blocks first per XCD.  Per 32-key half of a tile and wave: S^T = K Q^T and dP^T = V dO^T (16 MFMAs,
// K / V rows by ds_read_b128), dS^T = P (dP - delta) scale in registers, dQ^T += K^T dS^T (8 MFMAs, K^T by ds_read_tr from
// the same image).  delta = rowsum(dO * O) is computed HERE, in the prologue, from the fragments the wave loads anyway (each
// query row belongs to exactly one wave), and written to `delta_out` for the dK / dV kernel that follows on the stream: the
// separate delta launch (0.53 ms per step) is gone.
template <int D, bool CAUSAL, int HPB>
__global__ __launch_bounds__(512, 2) void attn_bwd_dq8_k(AttnArgs p, float* __restrict__ delta_out) {
    constexpr int RB = 256 / HPB;
    constexpr int TILE = KVStream8<D>::TILE, SLOT = 2 * TILE;
    __shared__ __attribute__((aligned(16))) char lds[2 * SLOT];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h2 = lane >> 5;
    const QWork w = attn_work_item8<CAUSAL, HPB>(p, wave, lane);
    const int b = w.b, h = w.h, qcol = w.qcol, qc = min(qcol, p.Sq - 1);
    const bool wave_on = w.wave_on;
    const KeyRange rng = attn_key_range(p, CAUSAL, w, RB);
    const int t_lo = rng.t_lo, t_hi = rng.t_hi;
    KVStream8<D> kv(p, w);

    // prologue in attn_fwd8_k's order: first K / V tile, then the Q, dO and O fragments and lse, then the wait for them
    kv.load_tile(p, t_lo);
    const bf16_t* qptr = p.Q + (long)b * p.q_bs + (long)qc * p.q_rs + (long)h * D;
    const bf16_t* gptr = p.dO + (long)b * p.do_bs + (long)qc * p.do_rs + (long)h * D;
    const bf16_t* optr = p.O + (long)b * p.o_bs + (long)qc * p.o_rs + (long)h * D;
    bf16x8 qf[D / 16], gf[D / 16];
    float dl = 0.f;
#pragma unroll
    for (int ds = 0; ds < D / 16; ++ds) {
        qf[ds] = *(const bf16x8*)(qptr + 16 * ds + 8 * h2);
        gf[ds] = *(const bf16x8*)(gptr + 16 * ds + 8 * h2);
        const bf16x8 of = *(const bf16x8*)(optr + 16 * ds + 8 * h2);
#pragma unroll
        for (int j = 0; j < 8; ++j) dl += (float)of[j] * (float)gf[ds][j];
    }
    const long stat = ((long)b * p.Hq + h) * p.Sq + qc;
    const float nlse = -p.lse[stat];
    const float dlt = swap_halves_sum(dl);                          // this lane's half of the head dim + its partner's
    if (wave_on && qcol < p.Sq && h2 == 0) delta_out[stat] = dlt;
#pragma unroll
    for (int ds = 0; ds < D / 16; ++ds) asm volatile("" :: "v"(qf[ds]), "v"(gf[ds]));
    asm volatile("" :: "v"(nlse));
    kv.store_tile(lds);
    kv.load_tile(p, t_lo + 1);

    int kofs[D / 16], tofs[D / 32][2];                              // K / V rows as the A operand; K^T from the K image
    lds_read_offsets<D>(lane, 0, kofs, tofs);
    f32x16 dq[D / 32];
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[i][r] = 0.f;
    attn_barrier();

    int sb = 0;
    for (int kt = t_lo; kt < t_hi; ++kt) {
        const int sn = SLOT - sb;
        const bool act = wave_on && kt * 64 <= rng.wave_kmax;
        if (act) {
            int kad[D / 16];
#pragma unroll
            for (int ds = 0; ds < D / 16; ++ds) { kad[ds] = kofs[ds] + sb; asm volatile("" : "+v"(kad[ds])); }
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                if (CAUSAL && kt * 64 + kb * 32 > rng.wave_kmax) break;                  // upper half of a diagonal tile: masked for every row of the wave
                f32x16 st, dp;
#pragma unroll
                for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
                for (int ds = 0; ds < D / 16; ++ds) {
                    st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(lds + kad[ds] + kb * 32 * D * 2), qf[ds], st, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(lds + kad[ds] + TILE + kb * 32 * D * 2), gf[ds], dp, 0, 0, 0);
                }
                mask_keys<1>(&st, p, CAUSAL, rng, kt * 64 + kb * 32, lane);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(fmaf(st[r], p.scale_log2, nlse));
                    st[r] = pv * ((dp[r] - dlt) * p.scale);                          // dS^T
                }
                int tad[D / 32][2];
#pragma unroll
                for (int i = 0; i < D / 32; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) { tad[i][j] = tofs[i][j] + sb + kb * 32 * D * 2; asm volatile("" : "+v"(tad[i][j])); }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 dsf = acc_frag(st, s);
#pragma unroll
                    for (int i = 0; i < D / 32; ++i)
                        dq[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_pair(lds + tad[i][0] + 16 * s * D * 2, lds + tad[i][1] + 16 * s * D * 2), dsf, dq[i], 0, 0, 0);
                }
            }
        }
        kv.advance(p, kt, t_hi, lds + sn);
        attn_barrier();
        sb = sn;
    }

    if (wave_on && qcol < p.Sq) {
        bf16_t* dqp = p.dQ + (long)b * p.dq_bs + (long)qcol * p.dq_rs + (long)h * D;
        if (p.rope_cs) {
            // Q is the rotary-embedded projection (adjacent-pair layout): gradient of the projection output = R(pos)^T dQ
            const float* cs = p.rope_cs + (long)qcol * D;           // (D / 2) pairs x 2 floats per position
#pragma unroll
            for (int i = 0; i < D / 32; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {                    // registers 4 jj .. 4 jj + 3: d = 32 i + 8 jj + 4 h2 + e
                    const float4 c4 = *(const float4*)(cs + (32 * i + 8 * jj + 4 * h2));
                    const float g0 = dq[i][4 * jj], g1 = dq[i][4 * jj + 1], g2 = dq[i][4 * jj + 2], g3 = dq[i][4 * jj + 3];
                    dq[i][4 * jj] = g0 * c4.x + g1 * c4.y;     dq[i][4 * jj + 1] = g1 * c4.x - g0 * c4.y;
                    dq[i][4 * jj + 2] = g2 * c4.z + g3 * c4.w; dq[i][4 * jj + 3] = g3 * c4.z - g2 * c4.w;
                }
        }
        store_row_bf16_16B<D>(dqp, dq, h2);
    }
}

// ------------------------------------------------------------------------------------------ backward: dK, dV
// block = 128 keys of one (batch, kv head); wave w owns keys [k0 + 32w, k0 + 32w + 32).  QR query rows (32 or 64) are
// staged per iteration: QR = 64 halves the barriers / staging round trips per unit of MFMA work.
#ifndef ATTN_DKDV_QR
#define ATTN_DKDV_QR 32
#endif

// D = 64: two blocks per CU (<= 256 VGPR + AGPR; the dropout variant took 284 and ran ONE block per CU: 250 us per cross-attention
// launch); D = 128 keeps its 384 registers and one block per CU
// NW = waves per block (32 keys each).  NW = 2 (64-key blocks, D = 128 causal): twice as many, half as long work items — the
// 128-key form's 320 blocks of length 5..1 on 256 CUs run at 0.75 of the balanced makespan, 640 blocks of length 10..1 at 0.93 —
// for twice the Q / dO staging per wave.
template <int D, bool DROP, int NW = 4>
__global__ __launch_bounds__(64 * NW, (NW == 4 && D == 64) ? 2 : 1) void attn_bwd_dkdv_k(AttnArgs p) {   // (NW = 2: 384 registers = one wave per SIMD, so two 2-wave blocks share a CU anyway)
    constexpr int QR = (D == 128) ? ATTN_DKDV_QR : 32;
    constexpr int NT = 64 * NW, KB = 32 * NW;
    constexpr int LDS_LOOP = 2 * QR * D * 2 + 2 * QR * 4, LDS_EPI = NW * 32 * 64 * 4;     // epilogue: a 32 x 64 fp32 transpose tile per wave
    __shared__ __attribute__((aligned(16))) char lds[LDS_LOOP > LDS_EPI ? LDS_LOOP : LDS_EPI];
    char* qimg = lds;
    char* gimg = lds + QR * D * 2;
    float* lse_s = (float*)(lds + 2 * QR * D * 2);
    float* dlt_s = lse_s + QR;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h2 = lane >> 5;    // wave index in an SGPR: everything derived from it (q0, mask tests) is scalar -> real branches
    // 1-D grid with the key block as the SLOWEST index: under the causal mask low key blocks sweep the
    // most query tiles, so the heaviest work items are dispatched first (longest-processing-time order)
    const int nhb = p.Hkv * p.B;
    const int kb0 = (blockIdx.x / nhb) * KB, k0 = kb0 + wave * 32;
    const int hk = (blockIdx.x % nhb) % p.Hkv, b = (blockIdx.x % nhb) / p.Hkv, group = p.Hq / p.Hkv;
    const int kcol = k0 + (lane & 31), kc = min(kcol, p.Sk - 1);
    const int kv_lo = p.kv_start ? max(0, min(p.kv_start[b], p.Sk)) : 0;
    const int coff = p.Sk - p.Sq;

    const bf16_t* kptr = p.K + (long)b * p.k_bs + (long)kc * p.k_rs + (long)hk * D;
    const bf16_t* vptr = p.V + (long)b * p.v_bs + (long)kc * p.v_rs + (long)hk * D;
    bf16x8 kf[D / 16], vf[D / 16];
#pragma unroll
    for (int ds = 0; ds < D / 16; ++ds) {
        kf[ds] = *(const bf16x8*)(kptr + 16 * ds + 8 * h2);
        vf[ds] = *(const bf16x8*)(vptr + 16 * ds + 8 * h2);
    }
    const bool key_ok = kcol < p.Sk && kcol >= kv_lo;

    f32x16 dk[D / 32], dv[D / 32];
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[i][r] = 0.f; dv[i][r] = 0.f; }

    // first query row that can see any key of this block
    const int q_first = p.causal ? max(0, kb0 - coff) : 0;
    const int qt_lo = q_first / QR, qt_hi = (p.Sq + QR - 1) / QR;
    // (query head of the GQA group, QR-row query slice) flattened into one iteration space; the Q / dO
    // tiles and their lse / delta rows are register-staged TWO iterations ahead.
    const int nq = qt_hi - qt_lo, n_it = group * nq;
    stage_t<D, QR, NT> qr0 = {}, gr0 = {}, qr1 = {}, gr1 = {};
    float ls0 = 0.f, dl0 = 0.f, ls1 = 0.f, dl1 = 0.f;
#define DESTA_Q_FETCH(IT, QR_, GR, LS, DL)                                                                      \
    {                                                                                                          \
        const int h_ = hk * group + (IT) / nq, qt_ = qt_lo + (IT) % nq;                                        \
        QR_ = tile_load<D, QR, NT>(p.Q + (long)b * p.q_bs + (long)h_ * D, p.q_rs, qt_ * QR, p.Sq - 1);        \
        GR = tile_load<D, QR, NT>(p.dO + (long)b * p.do_bs + (long)h_ * D, p.do_rs, qt_ * QR, p.Sq - 1);      \
        if (threadIdx.x < QR) {                                                                                \
            const long st_ = ((long)b * p.Hq + h_) * p.Sq + min(qt_ * QR + (int)threadIdx.x, p.Sq - 1);       \
            LS = p.lse[st_];                                                                                   \
            DL = p.delta[st_];                                                                                 \
        }                                                                                                      \
    }
#define DESTA_Q_STAGE(IT, QR_, GR, LS, DL)                                                                      \
    __syncthreads();                                                                                           \
    asm volatile("; stage " #QR_ ::: "memory");                                                                \
    tile_store<D, QR, NT>(qimg, QR_);                                                                          \
    tile_store<D, QR, NT>(gimg, GR);                                                                           \
    if (threadIdx.x < QR) { lse_s[threadIdx.x] = LS; dlt_s[threadIdx.x] = DL; }                                \
    __syncthreads();                                                                                           \
    if ((IT) + 2 < n_it) DESTA_Q_FETCH((IT) + 2, QR_, GR, LS, DL)
    if (n_it > 0) DESTA_Q_FETCH(0, qr0, gr0, ls0, dl0)
    if (n_it > 1) DESTA_Q_FETCH(1, qr1, gr1, ls1, dl1)
    auto compute = [&](const int it) __attribute__((always_inline)) {
        const int qt = qt_lo + it % nq;
        constexpr int NS = QR / 32;
        f32x16 stv[NS], dpv[NS];
        bool act[NS];
        // phase A for every 32-row slice first: with QR = 64 the S / dP MFMAs of slice 1 are in flight while the
        // VALU softmax of slice 0 runs, and slice 0's dV / dK MFMAs overlap the softmax of slice 1
#pragma unroll
        for (int sub = 0; sub < NS; ++sub) {
            const int qb = qt * QR + sub * 32;                                // first query row of this 32-row slice
            // wave-uniform skips: slice past the end, or (causal) all of this wave's keys in the slice's future
            act[sub] = qb < p.Sq && !(p.causal && k0 > qb + 31 + coff);
            if (!act[sub]) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) { stv[sub][r] = 0.f; dpv[sub][r] = 0.f; }
#pragma unroll
            for (int ds = 0; ds < D / 16; ++ds) {
                stv[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(qimg, sub * 32, ds, lane), kf[ds], stv[sub], 0, 0, 0);
                dpv[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(gimg, sub * 32, ds, lane), vf[ds], dpv[sub], 0, 0, 0);
            }
        }
#pragma unroll
        for (int sub = 0; sub < NS; ++sub) {
            if (!act[sub]) continue;
            const int qb = qt * QR + sub * 32;
            f32x16& st = stv[sub];
            f32x16& dp = dpv[sub];
            // st[r]: S[q = qb + acc_row(r)][key = kcol]
            // masks only on boundary tiles (wave-uniform): ragged Sq/Sk, left padding, causal diagonal
            const bool need_mask = (qb + 31 >= p.Sq) || (k0 + 31 >= p.Sk) || (k0 < kv_lo) ||
                                   (p.causal && k0 + 31 > qb + coff);
            // this lane's 16 accumulator rows are 4 runs of 4 consecutive query rows (acc_row): fetch lse / delta as
            // 4 + 4 ds_read_b128 instead of 32 scalar LDS reads inside the dependent exp chain
            float lsv[16], dlv[16];
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {
                const float4 a4 = *(const float4*)(lse_s + sub * 32 + 8 * q4 + 4 * h2);
                const float4 b4 = *(const float4*)(dlt_s + sub * 32 + 8 * q4 + 4 * h2);
                lsv[4 * q4 + 0] = a4.x; lsv[4 * q4 + 1] = a4.y; lsv[4 * q4 + 2] = a4.z; lsv[4 * q4 + 3] = a4.w;
                dlv[4 * q4 + 0] = b4.x; dlv[4 * q4 + 1] = b4.y; dlv[4 * q4 + 2] = b4.z; dlv[4 * q4 + 3] = b4.w;
            }
            unsigned keep = 0xffffu;                                          // bit r: probability (query row r, this key) survived
            if constexpr (DROP) {
                const unsigned long hb = ((unsigned long)b * p.Hq + (hk * group + it / nq)) * p.Sq;
                keep = 0;
                // lanes 2j, 2j+1 hold ADJACENT keys = one element pair = one hash (common.h; Sk even: host check): the even lane
                // hashes query rows 0..7 of the slice, the odd lane rows 8..15, and they swap through DPP (half the integer multiplies)
                const int half = lane & 1, kpair = k0 + (lane & 30);
                unsigned hh[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ql = (j & 3) + 8 * (2 * half + (j >> 2)) + 4 * h2;               // acc_row(8 * half + j, lane)
                    hh[j] = desta_rng32(p.seed_lo, p.seed_hi, ((hb + min(qb + ql, p.Sq - 1)) * p.Sk + kpair) >> 1);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned oth = (unsigned)__builtin_amdgcn_mov_dpp((int)hh[j], 0xB1, 0xf, 0xf, true);       // quad_perm [1,0,3,2]
                    const unsigned mine = half ? (hh[j] >> 16) : (hh[j] & 0xffffu), theirs = half ? (oth >> 16) : (oth & 0xffffu);
                    keep |= (mine >= p.drop_thresh ? 1u : 0u) << (8 * half + j);
                    keep |= (theirs >= p.drop_thresh ? 1u : 0u) << (8 * (1 - half) + j);
                }
            }
            if (need_mask) {                                           // boundary slices only (scalar branch, outside the element loop)
                asm volatile("; boundary slice" ::: "memory");
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int q = qb + acc_row(r, lane);
                    const bool ok = key_ok && q < p.Sq && (!p.causal || kcol <= q + coff);
                    st[r] = ok ? st[r] : -INFINITY;                   // exp2(-inf) = 0
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float pv = __builtin_amdgcn_exp2f(fmaf(st[r], p.scale_log2, -lsv[r]));
                float ms = 1.0f;
                if constexpr (DROP) ms = ((keep >> r) & 1u) ? p.drop_scale : 0.f;
                st[r] = pv * ms;                                             // (dropped) P for dV
                dp[r] = pv * (ms * dp[r] - dlv[r]) * p.scale;                // dS
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16x8 pf = acc_frag(st, s), dsf = acc_frag(dp, s);
#pragma unroll
                for (int i = 0; i < D / 32; ++i) {
                    dv[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, frag_tr<D>(gimg, sub * 32 + 16 * s, i * 32, lane), dv[i], 0, 0, 0);
                    dk[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsf, frag_tr<D>(qimg, sub * 32 + 16 * s, i * 32, lane), dk[i], 0, 0, 0);
                }
            }
        }
    };
    for (int it = 0; it < n_it; it += 2) {
        DESTA_Q_STAGE(it, qr0, gr0, ls0, dl0)
        compute(it);
        if (it + 1 < n_it) {
            DESTA_Q_STAGE(it + 1, qr1, gr1, ls1, dl1)
            compute(it + 1);
        }
    }
#undef DESTA_Q_STAGE
#undef DESTA_Q_FETCH
    // dk[i][r]: dK[key = k0 + acc_row(r)][d = i*32 + (lane&31)]
    bf16_t* dkp = p.dK + (long)b * p.dk_bs + (long)hk * D;
    bf16_t* dvp = p.dV + (long)b * p.dv_bs + (long)hk * D;
    const bool wide = ((p.dk_rs | p.dv_rs | p.dk_bs | p.dv_bs) & 7) == 0 && (((size_t)p.dK | (size_t)p.dV) & 15) == 0;
    if (wide) {
        // A lane owns ONE column of 16 keys: stored directly that is 64 two-byte store instructions per tensor and wave (the
        // cross-attention dK / dV are 245 MB per layer).  Transposed through a wave-private 32 x 64 fp32 LDS tile a lane owns 8
        // CONSECUTIVE columns of one key: 4 x 16-byte stores per 64 columns, 128-byte row segments.
        __syncthreads();                                                     // every wave is done with the Q / dO images
        float* tb = (float*)lds + wave * (32 * 64);
        auto emit = [&](const f32x16 (&acc)[D / 32], bf16_t* base, long rs, const bool rope) __attribute__((always_inline)) {
#pragma unroll
            for (int hf = 0; hf < D / 64; ++hf) {
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tb[acc_row(r, lane) * 64 + ii * 32 + (lane & 31)] = acc[hf * 2 + ii][r];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // same wave: LDS ops complete in order, keep the compiler in order too
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = (lane >> 3) + 8 * j, key = k0 + row;
                    float4 x0 = *(const float4*)(tb + row * 64 + (lane & 7) * 8), x1 = *(const float4*)(tb + row * 64 + (lane & 7) * 8 + 4);
                    if (rope) {                                              // K is the rotary-embedded projection: R(position = key)^T dK
                        const float* cs = p.rope_cs + (long)min(key, p.Sk - 1) * D + hf * 64 + (lane & 7) * 8;
                        const float4 c0 = *(const float4*)cs, c1 = *(const float4*)(cs + 4);
                        const float4 y0 = make_float4(x0.x * c0.x + x0.y * c0.y, x0.y * c0.x - x0.x * c0.y, x0.z * c0.z + x0.w * c0.w, x0.w * c0.z - x0.z * c0.w);
                        const float4 y1 = make_float4(x1.x * c1.x + x1.y * c1.y, x1.y * c1.x - x1.x * c1.y, x1.z * c1.z + x1.w * c1.w, x1.w * c1.z - x1.z * c1.w);
                        x0 = y0; x1 = y1;
                    }
                    u16x8 o;
                    o[0] = f2bf(x0.x); o[1] = f2bf(x0.y); o[2] = f2bf(x0.z); o[3] = f2bf(x0.w);
                    o[4] = f2bf(x1.x); o[5] = f2bf(x1.y); o[6] = f2bf(x1.z); o[7] = f2bf(x1.w);
                    if (key < p.Sk) *(u16x8*)(base + (long)key * rs + hf * 64 + (lane & 7) * 8) = o;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // reads done before the next half overwrites the tile
            }
        };
        emit(dk, dkp, p.dk_rs, p.rope_cs != nullptr);
        emit(dv, dvp, p.dv_rs, false);
        return;
    }
#pragma unroll
    for (int i = 0; i < D / 32; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + acc_row(r, lane);
            if (key < p.Sk) {
                dkp[(long)key * p.dk_rs + i * 32 + (lane & 31)] = f2bf(dk[i][r]);
                dvp[(long)key * p.dv_rs + i * 32 + (lane & 31)] = f2bf(dv[i][r]);
            }
        }
}

// ------------------------------------------------------------------------------------------ backward, ONE query tile (seq_q <= 64, D = 64): dQ, dK, dV in one pass
// The Q-Former's cross-attention (64 queries over 1500 encoder frames, 640 (batch, head) pairs per launch) is HBM-bound: K / V
// are 246 MB, dK / dV another 246 MB.  The two-kernel backward reads K / V twice (the dQ kernel re-computes S and dP) and
// re-fetches Q / dO per 128-key block: 930 MB of traffic, 260 us.  With a single query tile a block can own the WHOLE query
// range: it walks a chunk of key blocks, stages each K / V tile once (coalesced, through LDS), forms S and dP, emits dK / dV
// of that block and keeps dQ = sum_keys dS K in registers across the walk.  The keys of a (batch, head) are cut into `nch`
// chunks (work items = nch x batch x heads, equal length) whose dQ partials are summed in fixed order by attn_dq_sum_k:
// K / V read once, dK / dV written once, + 2 x nch x 16 KB per (batch, head) of partials.  No atomics: bit-identical run to run.
// block = 4 waves, wave w owns keys [128 kb + 32 w, +32) of every key block kb of its chunk.
// TR: dK / dV are written TRANSPOSED (the operand layout of the K / V projection's weight-gradient GEMM: no transpose pass over
// the 246 MB) and their sums over keys (the projection's bias gradients) leave the kernel as one partial row per (chunk, batch).
template <bool DROP, bool TR>
__global__ __launch_bounds__(256, 2) void attn_bwd_q64_k(AttnArgs p, float* __restrict__ dq_part, float* __restrict__ bias_part, int blocks_per_chunk) {
    constexpr int D = 64, WREG = 12288;
    __shared__ __attribute__((aligned(16))) char lds[2 * 64 * D * 2 + 4 * WREG + 2 * 64 * 4];
    char* qimg = lds;                                                       // [64 q][64 d]
    char* gimg = lds + 64 * D * 2;                                          // dO
    char* wreg = lds + 2 * 64 * D * 2;                                      // per wave: its 32 K rows | its 32 V rows | dS [32 keys][64 q]  (= 12 KB, re-used as the 32 x 64 fp32 epilogue tile)
    float* lse_s = (float*)(wreg + 4 * WREG);
    float* dlt_s = lse_s + 64;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), h2 = lane >> 5;
    const int nbh = p.B * p.Hq;
    const int chunk = blockIdx.x / nbh, bh = blockIdx.x % nbh, b = bh / p.Hq, h = bh % p.Hq;
    const int nkb = (p.Sk + 127) / 128;
    const int kb_lo = chunk * blocks_per_chunk, kb_hi = min(kb_lo + blocks_per_chunk, nkb);
    const int kv_lo = p.kv_start ? max(0, min(p.kv_start[b], p.Sk)) : 0;
    char* kimg_w = wreg + wave * WREG;
    char* vimg_w = kimg_w + 4096;
    char* dsimg_w = kimg_w + 8192;
    const bf16_t* kbase = p.K + (long)b * p.k_bs + (long)h * D;
    const bf16_t* vbase = p.V + (long)b * p.v_bs + (long)h * D;

    // the query tile, once
    {
        const stage_t<D, 64> qr = tile_load<D, 64>(p.Q + (long)b * p.q_bs + (long)h * D, p.q_rs, 0, p.Sq - 1);
        const stage_t<D, 64> gr = tile_load<D, 64>(p.dO + (long)b * p.do_bs + (long)h * D, p.do_rs, 0, p.Sq - 1);
        tile_store<D, 64>(qimg, qr);
        tile_store<D, 64>(gimg, gr);
        if (threadIdx.x < 64) {
            const long st_ = ((long)b * p.Hq + h) * p.Sq + min((int)threadIdx.x, p.Sq - 1);
            lse_s[threadIdx.x] = p.lse[st_];
            dlt_s[threadIdx.x] = p.delta[st_];
        }
    }
    // dQ: wave w owns the 32 x 32 tile (query slice w >> 1, d half w & 1) over ALL 128 keys of a block (every wave's dS image and K rows
    // are in LDS anyway): 16 accumulator registers instead of 64 for per-wave partials, and no cross-wave sum at the end
    const int qa = wave >> 1, di = wave & 1;
    f32x16 dq;
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[r] = 0.f;

    stage_t<D, 128> kst = {}, vst = {};
    if (kb_lo < kb_hi) {
        kst = tile_load<D, 128>(kbase, p.k_rs, kb_lo * 128, p.Sk - 1);
        vst = tile_load<D, 128>(vbase, p.v_rs, kb_lo * 128, p.Sk - 1);
    }
    const unsigned long hb = ((unsigned long)b * p.Hq + h) * p.Sq;
    bf16_t* dkp = TR ? p.dK + (long)h * D * p.dkv_t_ld + (long)b * p.Sk : p.dK + (long)b * p.dk_bs + (long)h * D;
    bf16_t* dvp = TR ? p.dV + (long)h * D * p.dkv_t_ld + (long)b * p.Sk : p.dV + (long)b * p.dv_bs + (long)h * D;
    float bsum[2][2] = {{0.f, 0.f}, {0.f, 0.f}};                            // TR: [K | V][d half]: sums over this lane's keys of every block

    for (int kb = kb_lo; kb < kb_hi; ++kb) {
        __syncthreads();                                                    // every wave is done with its region (epilogue tile of the previous block) / the query images are written
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                       // 128 x 64 tile: row r of the tile lives in the region of wave r >> 5
            const int id = i * 256 + threadIdx.x, r = id >> 3, c = id & 7;
            char* dst = wreg + (r >> 5) * WREG + img_off<D>(r & 31, c);
            *(uint4*)dst = make_uint4(kst[4 * i + 0], kst[4 * i + 1], kst[4 * i + 2], kst[4 * i + 3]);
            *(uint4*)(dst + 4096) = make_uint4(vst[4 * i + 0], vst[4 * i + 1], vst[4 * i + 2], vst[4 * i + 3]);
        }
        __syncthreads();
        if (kb + 1 < kb_hi) {                                               // next tile: in flight during this block's arithmetic and epilogue
            kst = tile_load<D, 128>(kbase, p.k_rs, (kb + 1) * 128, p.Sk - 1);
            vst = tile_load<D, 128>(vbase, p.v_rs, (kb + 1) * 128, p.Sk - 1);
        }
        const int k0 = kb * 128 + wave * 32, kcol = k0 + (lane & 31);
        const bool key_ok = kcol < p.Sk && kcol >= kv_lo;
        f32x16 dk[2], dv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) { dk[i][r] = 0.f; dv[i][r] = 0.f; }
#pragma unroll 1
        for (int sub = 0; sub < 2; ++sub) {                                 // (not unrolled: both slices in flight at once spill)
            const int qb = sub * 32;
            if (qb >= p.Sq) {                                                // (wave-uniform) slice past the end: its dS is zero
#pragma unroll
                for (int j = 0; j < 4; ++j) *(uint2*)(dsimg_w + img_off<D>(lane & 31, sub * 4 + j) + 8 * h2) = make_uint2(0u, 0u);
                continue;
            }
            unsigned keep = 0xffffu;                                         // (hashes first: nothing else is live yet)
            if constexpr (DROP) {                                            // same element -> hash map as attn_bwd_dkdv_k (adjacent keys share one hash)
                keep = 0;
                const int half = lane & 1, kpair = k0 + (lane & 30);
                unsigned hh[8];
                const unsigned long e0 = (hb + qb) * p.Sk + kpair;            // element index of (query qb, key pair); rows >= Sq are masked below, their bits are unused
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int ql = (j & 3) + 8 * (2 * half + (j >> 2)) + 4 * h2;
                    hh[j] = desta_rng32(p.seed_lo, p.seed_hi, (e0 + (unsigned)(ql * p.Sk)) >> 1);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned oth = (unsigned)__builtin_amdgcn_mov_dpp((int)hh[j], 0xB1, 0xf, 0xf, true);
                    const unsigned mine = half ? (hh[j] >> 16) : (hh[j] & 0xffffu), theirs = half ? (oth >> 16) : (oth & 0xffffu);
                    keep |= (mine >= p.drop_thresh ? 1u : 0u) << (8 * half + j);
                    keep |= (theirs >= p.drop_thresh ? 1u : 0u) << (8 * (1 - half) + j);
                }
            }
            if constexpr (DROP) asm volatile("" : "+v"(keep));               // keep the hash arithmetic in front of the accumulators' live range
            f32x16 st, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
            for (int ds = 0; ds < D / 16; ++ds) {
                st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(qimg, qb, ds, lane), frag_rows<D>(kimg_w, 0, ds, lane), st, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows<D>(gimg, qb, ds, lane), frag_rows<D>(vimg_w, 0, ds, lane), dp, 0, 0, 0);
            }
            // st[r]: S[q = qb + acc_row(r)][key = kcol]
            const bool need_mask = (qb + 31 >= p.Sq) || (k0 + 31 >= p.Sk) || (k0 < kv_lo);
            if (need_mask) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool ok = key_ok && (qb + acc_row(r, lane)) < p.Sq;
                    st[r] = ok ? st[r] : -INFINITY;
                }
            }
#pragma unroll
            for (int q4 = 0; q4 < 4; ++q4) {                                 // this lane's rows: 4 runs of 4 consecutive queries (acc_row)
                const float4 a4 = *(const float4*)(lse_s + qb + 8 * q4 + 4 * h2);
                const float4 b4 = *(const float4*)(dlt_s + qb + 8 * q4 + 4 * h2);
                const float ls4[4] = {a4.x, a4.y, a4.z, a4.w}, dl4[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * q4 + e;
                    const float pv = __builtin_amdgcn_exp2f(fmaf(st[r], p.scale_log2, -ls4[e]));
                    float ms = 1.0f;
                    if constexpr (DROP) ms = ((keep >> r) & 1u) ? p.drop_scale : 0.f;
                    st[r] = pv * ms;                                         // (dropped) P for dV
                    dp[r] = pv * (ms * dp[r] - dl4[e]) * p.scale;            // dS
                }
            }
            // dS of this slice -> the wave's [key][q] image (row = this lane's key): 4 runs of 4 consecutive query rows
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned lo = (unsigned)f2bf(dp[4 * j + 0]) | ((unsigned)f2bf(dp[4 * j + 1]) << 16);
                const unsigned hi = (unsigned)f2bf(dp[4 * j + 2]) | ((unsigned)f2bf(dp[4 * j + 3]) << 16);
                *(uint2*)(dsimg_w + img_off<D>(lane & 31, sub * 4 + j) + 8 * h2) = make_uint2(lo, hi);
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8 pf = acc_frag(st, s2), dsf = acc_frag(dp, s2);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    dv[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf, frag_tr<D>(gimg, qb + 16 * s2, i * 32, lane), dv[i], 0, 0, 0);
                    dk[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(dsf, frag_tr<D>(qimg, qb + 16 * s2, i * 32, lane), dk[i], 0, 0, 0);
                }
            }
        }
        __syncthreads();                                                    // every wave's dS image is complete
        // dQ[q][d] += sum over the block's 128 keys of dS[q][key] K[key][d]: both operands are transposed reads with the key as the row
#pragma unroll
        for (int wv = 0; wv < 4; ++wv)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
                dq = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr<D>(wreg + wv * WREG + 8192, 16 * s2, qa * 32, lane),
                                                             frag_tr<D>(wreg + wv * WREG, 16 * s2, di * 32, lane), dq, 0, 0, 0);
        __syncthreads();                                                    // the regions are free: each becomes its wave's 32 x 64 fp32 transpose tile
        if constexpr (TR) {
            // transposed store: [d][key] through a wave-private [64 d][36] fp32 tile (a lane holds 4 runs of 4 consecutive keys of
            // ONE d: float4 writes; then a lane reads 4 consecutive keys of one d: 8-byte bf16 stores, 64-byte row segments)
            float* tb = (float*)kimg_w;
            auto emit_t = [&](const f32x16 (&acc)[2], bf16_t* base, float (&bs)[2]) __attribute__((always_inline)) {
#pragma unroll
                for (int ii = 0; ii < 2; ++ii) {
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        *(float4*)(tb + (ii * 32 + (lane & 31)) * 36 + 8 * q4 + 4 * h2) =
                            make_float4(acc[ii][4 * q4], acc[ii][4 * q4 + 1], acc[ii][4 * q4 + 2], acc[ii][4 * q4 + 3]);
                        bs[ii] += (acc[ii][4 * q4] + acc[ii][4 * q4 + 1]) + (acc[ii][4 * q4 + 2] + acc[ii][4 * q4 + 3]);
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int dr = 8 * j + (lane >> 3), key = k0 + 4 * (lane & 7);
                    const float4 x = *(const float4*)(tb + dr * 36 + 4 * (lane & 7));
                    u16x4 o;
                    o[0] = f2bf(x.x); o[1] = f2bf(x.y); o[2] = f2bf(x.z); o[3] = f2bf(x.w);
                    if (key < p.Sk) *(u16x4*)(base + (long)dr * p.dkv_t_ld + key) = o;        // Sk % 4 == 0 (host check): a group is whole or absent
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            };
            emit_t(dk, dkp, bsum[0]);
            emit_t(dv, dvp, bsum[1]);
        } else {
            float* tb = (float*)kimg_w;
            auto emit = [&](const f32x16 (&acc)[2], bf16_t* base, long rs) __attribute__((always_inline)) {
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int r = 0; r < 16; ++r) tb[acc_row(r, lane) * 64 + ii * 32 + (lane & 31)] = acc[ii][r];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = (lane >> 3) + 8 * j, key = k0 + row;
                    const float4 x0 = *(const float4*)(tb + row * 64 + (lane & 7) * 8), x1 = *(const float4*)(tb + row * 64 + (lane & 7) * 8 + 4);
                    u16x8 o;
                    o[0] = f2bf(x0.x); o[1] = f2bf(x0.y); o[2] = f2bf(x0.z); o[3] = f2bf(x0.w);
                    o[4] = f2bf(x1.x); o[5] = f2bf(x1.y); o[6] = f2bf(x1.z); o[7] = f2bf(x1.w);
                    if (key < p.Sk) *(u16x8*)(base + (long)key * rs + (lane & 7) * 8) = o;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            };
            emit(dk, dkp, p.dk_rs);
            emit(dv, dvp, p.dv_rs);
        }
    }
    // the four 32 x 32 tiles -> one [64 q][64 d] fp32 image -> one coalesced partial per work item
    float* acc_s = (float*)wreg;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_s[(qa * 32 + acc_row(r, lane)) * 64 + di * 32 + (lane & 31)] = dq[r];
    __syncthreads();
    float* out = dq_part + ((long)chunk * nbh + bh) * (64 * 64);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = (i * 256 + threadIdx.x) * 4;
        *(float4*)(out + e) = *(const float4*)(acc_s + e);
    }
    if constexpr (TR) {
        if (bias_part) {
            // bias gradients: sum the 8 (wave, key half) rows in fixed order -> this (chunk, batch)'s partial row [K | V][head * 64 + d]
            __syncthreads();
            float* bs_s = (float*)wreg;                                     // [8][128]
#pragma unroll
            for (int kv = 0; kv < 2; ++kv)
#pragma unroll
                for (int ii = 0; ii < 2; ++ii) bs_s[(wave * 2 + h2) * 128 + kv * 64 + ii * 32 + (lane & 31)] = bsum[kv][ii];
            __syncthreads();
            if (threadIdx.x < 128) {
                float t = 0.f;
#pragma unroll
                for (int r = 0; r < 8; ++r) t += bs_s[r * 128 + threadIdx.x];
                const int kv = threadIdx.x >> 6, dd = threadIdx.x & 63, W = 2 * p.Hq * 64;
                bias_part[((long)chunk * p.B + b) * W + kv * (p.Hq * 64) + h * 64 + dd] = t;
            }
        }
    }
}

// bias[c] = sum over the (chunk, batch) partial rows: 64 columns per block, the rows dealt to the block's 4 wave groups (4 independent
// accumulators each: 128 rows = 8 dependent rounds instead of 32), combined in fixed order
__global__ __launch_bounds__(256) void attn_bias_sum_k(const float* __restrict__ part, int nrows, int width, float* __restrict__ out) {
    __shared__ float comb[4][64];
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (c < width) {
        int r = grp;
        for (; r + 12 < nrows; r += 16) {
            a0 += part[(long)r * width + c];
            a1 += part[(long)(r + 4) * width + c];
            a2 += part[(long)(r + 8) * width + c];
            a3 += part[(long)(r + 12) * width + c];
        }
        for (; r < nrows; r += 4) a0 += part[(long)r * width + c];
    }
    comb[grp][lane] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (grp == 0 && c < width) out[c] = (comb[0][lane] + comb[1][lane]) + (comb[2][lane] + comb[3][lane]);
}

// dQ[b][q][h][:] = bf16(sum over the key chunks, in chunk order, of the fp32 partials of attn_bwd_q64_k)
__global__ __launch_bounds__(256) void attn_dq_sum_k(AttnArgs p, const float* __restrict__ dq_part, int nch) {
    const int nbh = p.B * p.Hq, bh = blockIdx.x, b = bh / p.Hq, h = bh % p.Hq;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = (i * 256 + threadIdx.x) * 4, q = e >> 6, d0 = e & 63;
        float4 s = *(const float4*)(dq_part + (long)bh * 4096 + e);
        for (int c = 1; c < nch; ++c) {
            const float4 v = *(const float4*)(dq_part + ((long)c * nbh + bh) * 4096 + e);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        if (q < p.Sq) {
            u16x4 o;
            o[0] = f2bf(s.x); o[1] = f2bf(s.y); o[2] = f2bf(s.z); o[3] = f2bf(s.w);
            *(u16x4*)(p.dQ + (long)b * p.dq_bs + (long)q * p.dq_rs + (long)h * 64 + d0) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------ decode (seq_q = 1), split-KV
// One token per sequence against a KV cache (llm_model.generate, modeling_desta25.py:1419): the forward kernel above gives
// that shape one block per QUERY head, which walks the whole cache serially and re-reads K / V once per head of the GQA group.
// Here a work item is (batch row, KV head, key chunk of DESTA_ATTN_DECODE_CHUNK keys): the G = Hq / Hkv query rows of the
// group share every K / V byte, and the chunks of one row run on different CUs.  Chunk c is keys [c * CH, (c + 1) * CH) of the
// cache whatever the batch, kv_start or the grid are, so a row's result is a function of that row's data alone.
//   * four waves, CH / 4 consecutive keys each.  K and V go straight from global memory to registers (no LDS round trip for the
//     streamed operands): every load of the wave's keys is issued before the first use, clamped to [kv_start, seq_k) rows.
//   * scores: S^T = K . Q^T by mfma_f32_16x16x32_bf16, keys on the A rows, the group's query rows on B columns 0..G-1 (the other
//     columns are zero).  Accumulator register r of lane l is key 16 t + 4 (l >> 4) + r, query row l & 15.
//   * softmax in fp32, log2 domain, against the BLOCK's maximum (one LDS exchange of 4 x 8 floats), so the four waves' sums add.
//   * P . V on the fp32 VALU: V rows are d-contiguous, an MFMA operand wants its k (= key) index on the lane, and a transpose
//     through LDS is what this kernel avoids.  Lane l owns columns 8 (l & 15) .. + 7 of keys = (l >> 4) mod 4 for every query
//     row; P comes back from a [key][8] fp32 LDS image as broadcast reads.  P is never rounded to bf16.
//   * the four key classes of a wave fold by a reduce-scatter over the query rows (xor 32, xor 16), the waves through LDS.
// A row with one chunk is finished here (O, lse).  Otherwise each item writes (max, sum, unnormalised O) in fp32 and
// attn_decode_combine_k merges a row's chunks in ascending order: no atomics, no tickets, a second launch.
// Empty chunk (all keys masked): max = -inf, sum = 0, O = 0; the combine skips it.
//
// FP8 (e4m3) KV cache: the same body on a cache of OCP e4m3 bytes + one power-of-two fp32 scale per (row, slot, K-or-V head) (the
// format of desta_rope_kv_append_e4m3).  Work items, chunk boundaries, lane slots, MFMA calls and summation order are shared, so
// O, lse and every workspace partial equal the bf16 kernel's on the dequantised cache bf16(q * s) bit for bit (while score * s_k
// and p * s_v stay normal fp32 values: a power of two commutes with a rounding only where nothing underflows).  KV8 differs in:
//   1. fragments: a lane's K fragment is 8 contiguous bytes at the element offsets of the bf16 kernel, its V piece the 8 bytes
//      of its 8 columns (DecodeKV);
//   2. the K and V scales of the keys of this lane's st[t][r] are loaded, rows clamped to [kv_start, seq_k) like the data rows;
//   3. K bytes become the bf16 MFMA operand exactly (3 mantissa bits) (k_operand);
//   4. the fp32 score is multiplied by the key's K scale in front of scale_log2;
//   5. the key's V scale is folded into the probability that goes to s_p (pv * s_v, exact), so the fma rounds the product the
//      bf16 kernel rounds; the row sum keeps pv;
//   6. V bytes become fp32 by the packed conversion instead of a shift (v_unpack).
// and, arithmetic aside, in where decode_load_q is called (see there): a scheduling matter, measured.
//
// Verify step of draft-and-verify decoding (ROWS; desta_attention_verify{,_kv8}): seq_q = w = 2..8 query rows per sequence on the
// same items.  The R = G w <= 16 query rows of a KV head take B columns 0..R-1 (column c: query row c / G, head hk G + c % G),
// the mask is the forward kernel's causal rule per column (key <= j + seq_k - seq_q), and maximum, sum, empty chunk and the merge
// are per column already.  At R > 8 the P . V walks two row groups of 8 with V kept in registers.  Row j equals the one-row kernel
// at seq_k - (w - 1 - j) keys bit for bit (include/desta_hip.h says why), which is what lets the speculative loop and the plain
// loop agree from the dispatch threshold on.
typedef __attribute__((ext_vector_type(2))) float f32x2;
__device__ __forceinline__ bf16x8 e4m3x8_to_bf16(const uint2& q) {
    union { unsigned u[4]; bf16x8 v; } o;
    const unsigned w[2] = {q.x, q.y};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
        o.u[2 * i] = __builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u);
        o.u[2 * i + 1] = __builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u);
    }
    return o.v;
}
template <bool KV8> struct DecodeKV { typedef bf16_t elem; typedef bf16x8 kfrag; typedef uint4 vfrag; };
template <> struct DecodeKV<true> { typedef uint8_t elem; typedef uint2 kfrag; typedef uint2 vfrag; };
__device__ __forceinline__ bf16x8 k_operand(const bf16x8& k) { return k; }
__device__ __forceinline__ bf16x8 k_operand(const uint2& k) { return e4m3x8_to_bf16(k); }
__device__ __forceinline__ void v_unpack(const uint4& v, float (&f)[8]) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j2 = 0; j2 < 4; ++j2) { f[2 * j2] = __builtin_bit_cast(float, w[j2] << 16); f[2 * j2 + 1] = __builtin_bit_cast(float, w[j2] & 0xffff0000u); }
}
__device__ __forceinline__ void v_unpack(const uint2& v, float (&f)[8]) {
    const f32x2 vv[4] = {__builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, false), __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, true),
                         __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, false), __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, true)};
#pragma unroll
    for (int j2 = 0; j2 < 4; ++j2) { f[2 * j2] = vv[j2][0]; f[2 * j2 + 1] = vv[j2][1]; }
}

// the B operand: this lane's 4 x 8 elements of its query row, zero for the columns past the group.  ROWS (seq_q = w rows per
// sequence): column c < R = G w is query row c / G of head hk G + c % G
template <bool ROWS>
__device__ __forceinline__ void decode_load_q(const AttnArgs& p, int b, int hk, int G, int c16, int q4, bf16x8 (&qf)[4]) {
    const int R = ROWS ? G * p.Sq : G, c = min(c16, R - 1);
    const bf16_t* qptr = p.Q + (long)b * p.q_bs + (ROWS ? (long)(c / G) * p.q_rs + (long)(hk * G + c % G) * 128 : (long)(hk * G + c) * 128) + 8 * q4;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        qf[ks] = *(const bf16x8*)(qptr + 32 * ks);
        if (c16 >= R)
#pragma unroll
            for (int j = 0; j < 8; ++j) qf[ks][j] = (__bf16)0.f;
    }
}
template <int GP, bool KV8, bool ROWS = false>            // GP: the query rows per KV head (G; ROWS: G seq_q) rounded up to 1, 2, 4, 8 (ROWS: 16 too); KV8: k_scale, v_scale, sc_bs, sc_rs are read
__device__ __forceinline__ void attn_decode_body(const AttnArgs& p, const float* __restrict__ k_scale, const float* __restrict__ v_scale, long sc_bs,
                                                 long sc_rs, float* __restrict__ ws_ml, float* __restrict__ ws_o, int nch) {
    typedef typename DecodeKV<KV8>::elem E;
    typedef typename DecodeKV<KV8>::kfrag KF;
    typedef typename DecodeKV<KV8>::vfrag VF;
    constexpr int CH = DESTA_ATTN_DECODE_CHUNK, KW = CH / 4, NT16 = KW / 16, NV = KW / 4;
    constexpr int PW = GP > 8 ? 16 : 8;                    // score columns kept: every query row of the item
    constexpr int GA = GP > 8 ? 8 : GP;                    // query rows of one P . V pass (acc[GA][8] next to the V fragments)
    static_assert(ROWS ? (GP >= 2 && GP <= 16) : GP <= 8, "one row per sequence: at most 8 rows per KV head");
    __shared__ __attribute__((aligned(16))) float s_p[4][KW][PW];
    __shared__ __attribute__((aligned(16))) float s_red[4][GP][128];
    __shared__ float s_m[4][PW], s_l[4][PW];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), c16 = lane & 15, q4 = lane >> 4;
    const int G = p.Hq / p.Hkv, R = ROWS ? G * p.Sq : G;
    int id = blockIdx.x;
    const int c = id % nch; id /= nch;
    const int hk = id % p.Hkv, b = id / p.Hkv;
    const int kv_lo = p.kv_start ? max(0, min(p.kv_start[b], p.Sk)) : 0;
    const int k0 = c * CH + wave * KW;
    const bool live = k0 < p.Sk && k0 + KW > kv_lo;        // wave-uniform: some key of this wave is visible
    const int row_lo = min(kv_lo, p.Sk - 1), row_hi = p.Sk - 1;
    // ROWS: the forward kernel's causal rule, key <= j + (seq_k - seq_q) for this lane's query row j = c16 / G.  A masked key
    // gives p = exp2(-inf) = 0 and fma(0, v, acc) = acc (v is a loaded, finite cache value), so row j is the one-row kernel's
    // result at seq_k - (seq_q - 1 - j), bit for bit
    const int key_hi = ROWS ? p.Sk - (p.Sq - 1 - min(c16, R - 1) / G) : p.Sk;

    KF kf[NT16][4];
    VF vf[NV];
    float ksc[NT16][4], vsc[NT16][4];                      // KV8: scales of keys k0 + 16 t + 4 q4 + r, the keys of this lane's st[t][r]
    bf16x8 qf[4];
    // The group's query rows.  WHERE the four loads are issued is a scheduling matter only, and the one place where the twins
    // want different things from hipcc (measured, B = 64 x 4 096 keys): behind the byte loads of KV8 it issues them one by one,
    // each after a full drain of the loads in flight (153.9 us against 136.2); in front of the bf16 loads it keeps fewer K / V
    // loads in flight (208 us against 199).
    if constexpr (KV8) decode_load_q<ROWS>(p, b, hk, G, c16, q4, qf);
    if (live) {
        const E* kbase = (const E*)p.K + (long)b * p.k_bs + (long)hk * 128 + 8 * q4;
        const E* vbase = (const E*)p.V + (long)b * p.v_bs + (long)hk * 128 + 8 * c16;
#pragma unroll
        for (int t = 0; t < NT16; ++t) {
            const int row = min(max(k0 + 16 * t + c16, row_lo), row_hi);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) kf[t][ks] = *(const KF*)(kbase + (long)row * p.k_rs + 32 * ks);
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int row = min(max(k0 + 4 * i + q4, row_lo), row_hi);
            vf[i] = *(const VF*)(vbase + (long)row * p.v_rs);
        }
        if constexpr (KV8) {
            const float* ksb = k_scale + (long)b * sc_bs + hk;
            const float* vsb = v_scale + (long)b * sc_bs + hk;
#pragma unroll
            for (int t = 0; t < NT16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = min(max(k0 + 16 * t + 4 * q4 + r, row_lo), row_hi);
                    ksc[t][r] = ksb[(long)row * sc_rs];
                    vsc[t][r] = vsb[(long)row * sc_rs];
                }
        }
    } else {
#pragma unroll
        for (int t = 0; t < NT16; ++t)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                kf[t][ks] = KF{};
                if constexpr (KV8) { ksc[t][ks] = 1.f; vsc[t][ks] = 1.f; }
            }
#pragma unroll
        for (int i = 0; i < NV; ++i) vf[i] = VF{};
    }
    if constexpr (!KV8) decode_load_q<ROWS>(p, b, hk, G, c16, q4, qf);

    // scores of the wave's KW keys, masked and scaled; st[t][r]: key k0 + 16 t + 4 q4 + r, query row c16
    f32x4 st[NT16];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT16; ++t) {
        st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) st[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k_operand(kf[t][ks]), qf[ks], st[t], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = k0 + 16 * t + 4 * q4 + r;
            const float sk = KV8 ? st[t][r] * ksc[t][r] : st[t][r];         // 2^e commutes with every fp32 rounding
            st[t][r] = (key >= kv_lo && key < key_hi) ? sk * p.scale_log2 : -INFINITY;
            mx = fmaxf(mx, st[t][r]);
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (lane < PW) s_m[wave][lane] = mx;
    __syncthreads();
    const int g8 = c16 & (PW - 1);
    const float mblk = fmaxf(fmaxf(s_m[0][g8], s_m[1][g8]), fmaxf(s_m[2][g8], s_m[3][g8]));
    const float muse = (mblk == -INFINITY) ? 0.f : mblk;
    float ls = 0.f;
#pragma unroll
    for (int t = 0; t < NT16; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pv = __builtin_amdgcn_exp2f(st[t][r] - muse);
            ls += pv;
            if (c16 < PW) s_p[wave][16 * t + 4 * q4 + r][c16] = KV8 ? pv * vsc[t][r] : pv;      // exact; the row sum keeps pv
        }
    ls += __shfl_xor(ls, 16, 64);
    ls += __shfl_xor(ls, 32, 64);
    if (lane < PW) s_l[wave][lane] = ls;
    __syncthreads();

    // P . V: acc[g][j] = sum over this lane's keys of P[h0 + g][key] * V[key][8 c16 + j], GA query rows per pass (16 rows: two
    // passes, V stays in registers and P is read again; a row's summation order does not depend on the pass it is in)
#pragma unroll 1
    for (int h0 = 0; h0 < GP; h0 += GA) {
        float acc[GA][8];
#pragma unroll
        for (int g = 0; g < GA; ++g)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const float* pr = &s_p[wave][4 * i + q4][h0];
            float pg[GA];
            if constexpr (GA >= 4) {
#pragma unroll
                for (int g = 0; g < GA; g += 4) {
                    const f32x4 t4 = *(const f32x4*)(pr + g);
                    pg[g] = t4[0]; pg[g + 1] = t4[1]; pg[g + 2] = t4[2]; pg[g + 3] = t4[3];
                }
            } else {
#pragma unroll
                for (int g = 0; g < GA; ++g) pg[g] = pr[g];
            }
            float v8[8];
            if constexpr (GP > GA) {                       // a second pass: keep the fp32 copy of V (128 registers) from being hoisted out of the pass
                if constexpr (KV8) asm volatile("" : "+v"(vf[i].x), "+v"(vf[i].y));
                else asm volatile("" : "+v"(vf[i].x), "+v"(vf[i].y), "+v"(vf[i].z), "+v"(vf[i].w));
            }
            v_unpack(vf[i], v8);
#pragma unroll
            for (int j2 = 0; j2 < 4; ++j2) {
                const float v0 = v8[2 * j2], v1 = v8[2 * j2 + 1];
#pragma unroll
                for (int g = 0; g < GA; ++g) {
                    acc[g][2 * j2] = fmaf(pg[g], v0, acc[g][2 * j2]);
                    acc[g][2 * j2 + 1] = fmaf(pg[g], v1, acc[g][2 * j2 + 1]);
                }
            }
        }
        // fold the four key classes (lanes l, l ^ 16, l ^ 32, l ^ 48): each exchange halves the query rows a lane keeps
        const bool hi32 = (lane & 32) != 0, hi16 = (lane & 16) != 0;
        constexpr int G1 = GA >= 2 ? GA / 2 : GA, G2 = GA >= 4 ? GA / 4 : G1;
        float a1[G1][8], a2[G2][8];
#pragma unroll
        for (int g = 0; g < G1; ++g)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (GA >= 2) {
                    const float keep = hi32 ? acc[g + G1][j] : acc[g][j], send = hi32 ? acc[g][j] : acc[g + G1][j];
                    a1[g][j] = keep + __shfl_xor(send, 32, 64);
                } else {
                    a1[g][j] = acc[g][j] + __shfl_xor(acc[g][j], 32, 64);
                }
            }
#pragma unroll
        for (int g = 0; g < G2; ++g)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if constexpr (GA >= 4) {
                    const float keep = hi16 ? a1[g + G2][j] : a1[g][j], send = hi16 ? a1[g][j] : a1[g + G2][j];
                    a2[g][j] = keep + __shfl_xor(send, 16, 64);
                } else {
                    a2[g][j] = a1[g][j] + __shfl_xor(a1[g][j], 16, 64);
                }
            }
        {
            // query rows (of this pass) this lane now holds: GA >= 4: (hi32 ? G1 : 0) + (hi16 ? G2 : 0) + g;  GA == 2: hi32 (both lanes of an
            // xor-16 pair hold the same sums: one writes);  GA == 1: row 0 on every lane (lanes 0..15 write)
            const int gbase = h0 + (GA >= 2 && hi32 ? G1 : 0) + (GA >= 4 && hi16 ? G2 : 0);
            const bool writer = GA >= 4 ? true : (GA == 2 ? !hi16 : lane < 16);
            if (writer)
#pragma unroll
                for (int g = 0; g < G2; ++g) {
                    float* dst = &s_red[wave][gbase + g][8 * c16];
                    *(f32x4*)dst = f32x4{a2[g][0], a2[g][1], a2[g][2], a2[g][3]};
                    *(f32x4*)(dst + 4) = f32x4{a2[g][4], a2[g][5], a2[g][6], a2[g][7]};
                }
        }
    }
    __syncthreads();

    // the block's result: thread t < 32 GP sums the four waves for query row t / 32, columns 4 (t % 32) .. + 3
    // (16 rows: two rounds).  ROWS: row tg is query row tg / G of head hk G + tg % G; lse and the workspace are [b][h][seq_q]
    const int d4 = threadIdx.x & 31;
#pragma unroll
    for (int t0 = 0; t0 < GP; t0 += 8) {
        const int tg = t0 + (threadIdx.x >> 5);
        if (tg >= R) continue;
        f32x4 o = *(const f32x4*)&s_red[0][tg][4 * d4];
#pragma unroll
        for (int w = 1; w < 4; ++w) o += *(const f32x4*)&s_red[w][tg][4 * d4];
        const float m = fmaxf(fmaxf(s_m[0][tg], s_m[1][tg]), fmaxf(s_m[2][tg], s_m[3][tg]));
        const float l = ((s_l[0][tg] + s_l[1][tg]) + s_l[2][tg]) + s_l[3][tg];
        const int j = ROWS ? tg / G : 0, h = hk * G + (ROWS ? tg % G : tg);
        const long row = ROWS ? ((long)b * p.Hq + h) * p.Sq + j : (long)b * p.Hq + h;
        if (nch == 1) {
            u16x4 ob;
#pragma unroll
            for (int e = 0; e < 4; ++e) ob[e] = f2bf(l > 0.f ? o[e] / l : 0.f);
            *(u16x4*)(p.O + (long)b * p.o_bs + (ROWS ? (long)j * p.o_rs : 0) + (long)h * 128 + 4 * d4) = ob;
            if (p.lse && d4 == 0) p.lse[row] = l > 0.f ? m + log2f(l) : INFINITY;
        } else {
            const long r = row * nch + c;
            *(f32x4*)(ws_o + r * 128 + 4 * d4) = o;
            if (d4 == 0) { ws_ml[2 * r] = m; ws_ml[2 * r + 1] = l; }
        }
    }
}
// seq_q = w rows per sequence (a verify step of draft-and-verify decoding): the same items, the K / V of an item loaded once
// for all R = G w rows.  RP: R rounded up to 2, 4, 8, 16
template <int RP>
__global__ __launch_bounds__(256, 2) void attn_verify_k(AttnArgs p, float* __restrict__ ws_ml, float* __restrict__ ws_o, int nch) {
    attn_decode_body<RP, false, true>(p, nullptr, nullptr, 0, 0, ws_ml, ws_o, nch);
}
template <int RP>
__global__ __launch_bounds__(256, 2) void attn_verify_kv8_k(AttnArgs p, const float* __restrict__ k_scale, const float* __restrict__ v_scale, long sc_bs,
                                                         long sc_rs, float* __restrict__ ws_ml, float* __restrict__ ws_o, int nch) {
    attn_decode_body<RP, true, true>(p, k_scale, v_scale, sc_bs, sc_rs, ws_ml, ws_o, nch);
}
template <int GP>
__global__ __launch_bounds__(256) void attn_decode_k(AttnArgs p, float* __restrict__ ws_ml, float* __restrict__ ws_o, int nch) {
    attn_decode_body<GP, false>(p, nullptr, nullptr, 0, 0, ws_ml, ws_o, nch);
}
template <int GP>
__global__ __launch_bounds__(256) void attn_kv8_k(AttnArgs p, const float* __restrict__ k_scale, const float* __restrict__ v_scale, long sc_bs, long sc_rs,
                                                  float* __restrict__ ws_ml, float* __restrict__ ws_o, int nch) {
    attn_decode_body<GP, true>(p, k_scale, v_scale, sc_bs, sc_rs, ws_ml, ws_o, nch);
}

// Merge of a row's chunk partials, chunks in ascending order, fp32.  32 threads per (batch, query head), 8 heads per block.
// ROWS: per (batch, query head, query row); a chunk that is empty for this row alone is skipped like any empty chunk.
template <bool ROWS>
__device__ __forceinline__ void attn_combine_body(const AttnArgs& p, const float* __restrict__ ws_ml, const float* __restrict__ ws_o, int nch) {
    const long bh = (long)blockIdx.x * 8 + (threadIdx.x >> 5);
    const int d4 = threadIdx.x & 31;
    if (bh >= (long)p.B * p.Hq * (ROWS ? p.Sq : 1)) return;
    const float* ml = ws_ml + 2 * bh * nch;
    const float* po = ws_o + bh * nch * 128 + 4 * d4;
    float m = -INFINITY;
    for (int c = 0; c < nch; ++c) m = fmaxf(m, ml[2 * c]);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    for (int c = 0; c < nch; ++c) {
        const float mc = ml[2 * c], lc = ml[2 * c + 1];
        if (mc == -INFINITY || !(lc > 0.f)) continue;      // empty chunk
        const float w = __builtin_amdgcn_exp2f(mc - m);
        const f32x4 oc = *(const f32x4*)(po + (long)c * 128);
        l = fmaf(w, lc, l);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(w, oc[e], o[e]);
    }
    const long bhh = ROWS ? bh / p.Sq : bh;
    const int b = (int)(bhh / p.Hq), h = (int)(bhh % p.Hq), j = ROWS ? (int)(bh % p.Sq) : 0;
    u16x4 ob;
#pragma unroll
    for (int e = 0; e < 4; ++e) ob[e] = f2bf(l > 0.f ? o[e] / l : 0.f);
    *(u16x4*)(p.O + (long)b * p.o_bs + (ROWS ? (long)j * p.o_rs : 0) + (long)h * 128 + 4 * d4) = ob;
    if (p.lse && d4 == 0) p.lse[bh] = l > 0.f ? m + log2f(l) : INFINITY;
}
__global__ __launch_bounds__(256) void attn_decode_combine_k(AttnArgs p, const float* __restrict__ ws_ml, const float* __restrict__ ws_o, int nch) {
    attn_combine_body<false>(p, ws_ml, ws_o, nch);
}
__global__ __launch_bounds__(256) void attn_verify_combine_k(AttnArgs p, const float* __restrict__ ws_ml, const float* __restrict__ ws_o, int nch) {
    attn_combine_body<true>(p, ws_ml, ws_o, nch);
}

int fill_args(const desta_attn_desc* d, AttnArgs& a) {
    DESTA_CHECK_ARG(d && d->Q && d->K && d->V, "attention: null operand");
    DESTA_CHECK_ARG(d->head_dim == 64 || d->head_dim == 128, "attention: head_dim %d unsupported (64 or 128)", d->head_dim);
    DESTA_CHECK_ARG(d->batch > 0 && d->n_q_heads > 0 && d->n_kv_heads > 0 && d->n_q_heads % d->n_kv_heads == 0,
                    "attention: bad head counts");
    DESTA_CHECK_ARG(d->seq_q > 0 && d->seq_k > 0, "attention: bad sequence lengths");
    DESTA_CHECK_ARG(!d->causal || d->seq_k >= d->seq_q, "attention: causal needs seq_k >= seq_q");
    DESTA_CHECK_ARG(d->q_row_stride % 8 == 0 && d->k_row_stride % 8 == 0 && d->v_row_stride % 8 == 0,
                    "attention: row strides must be multiples of 8 elements");
    DESTA_CHECK_ARG(d->batch <= 65535 && d->n_q_heads <= 65535, "attention: grid too large");
    a.Q = (const bf16_t*)d->Q; a.K = (const bf16_t*)d->K; a.V = (const bf16_t*)d->V; a.O = (bf16_t*)d->O;
    a.dO = (const bf16_t*)d->dO; a.dQ = (bf16_t*)d->dQ; a.dK = (bf16_t*)d->dK; a.dV = (bf16_t*)d->dV;
    a.lse = d->lse; a.delta = nullptr; a.O32 = d->O_f32; a.rope_cs = d->rope_cos_sin;
    a.q_bs = d->q_batch_stride; a.q_rs = d->q_row_stride; a.k_bs = d->k_batch_stride; a.k_rs = d->k_row_stride;
    a.v_bs = d->v_batch_stride; a.v_rs = d->v_row_stride; a.o_bs = d->o_batch_stride; a.o_rs = d->o_row_stride;
    a.do_bs = d->do_batch_stride; a.do_rs = d->do_row_stride; a.dq_bs = d->dq_batch_stride; a.dq_rs = d->dq_row_stride;
    a.dk_bs = d->dk_batch_stride; a.dk_rs = d->dk_row_stride; a.dv_bs = d->dv_batch_stride; a.dv_rs = d->dv_row_stride;
    a.B = d->batch; a.Hq = d->n_q_heads; a.Hkv = d->n_kv_heads; a.Sq = d->seq_q; a.Sk = d->seq_k;
    a.causal = d->causal; a.kv_start = d->kv_start;
    a.scale = d->scale; a.scale_log2 = d->scale * 1.44269504088896340736f;
    DESTA_CHECK_ARG(d->dropout_p >= 0.f && d->dropout_p < 1.f, "attention: dropout_p must be in [0,1)");
    DESTA_CHECK_ARG(d->dropout_p == 0.f || d->head_dim == 64, "attention: dropout is built for head_dim 64 (the Q-Former) only");
    DESTA_CHECK_ARG(d->dropout_p == 0.f || d->seq_k % 2 == 0, "attention: dropout needs an even seq_k (adjacent keys share one hash)");
    a.drop_thresh = d->dropout_p > 0.f ? desta_drop_thresh(d->dropout_p) : 0u;
    a.drop_scale = 1.0f / (1.0f - d->dropout_p);
    a.seed_lo = (unsigned)d->dropout_seed; a.seed_hi = (unsigned)(d->dropout_seed >> 32);
    a.dkv_t_ld = d->dkv_transposed ? d->dkv_t_ld : 0;
    return DESTA_OK;
}

}  // namespace

namespace {
int g_attn_opt[8] = {1, 0, 0, 0, 1, 0, 0, 0};                    // [4]: one-pass backward for a single query tile (seq_q <= 64, D = 64)
// 8-wave blocks (attn_fwd8_k, attn_bwd_dq8_k): hpb heads of one GQA group x 256 / hpb query rows (the heads share the K / V
// tiles; non-causal: one head) -> the 1-D grid, which attn_work_item8() orders per XCD
dim3 attn_grid8(const AttnArgs& a, int head_dim, int& hpb) {
    const int G = a.Hq / a.Hkv;
    hpb = !a.causal ? 1 : (head_dim == 128 ? (G % 4 == 0 ? 4 : (G % 2 == 0 ? 2 : 1)) : (G % 2 == 0 ? 2 : 1));
    const int rb = 256 / hpb;
    return dim3((unsigned)((a.Sq + rb - 1) / rb) * (unsigned)(G / hpb) * (unsigned)(a.B * a.Hkv));
}
}  // namespace
extern "C" int desta_attention_set_option(int which, int value) {
    DESTA_CHECK_ARG(which >= 0 && which < 8, "attention_set_option: unknown option %d", which);
    g_attn_opt[which] = value;
    return DESTA_OK;
}

extern "C" int desta_attention_fwd(const desta_attn_desc* d, void* stream) {
    AttnArgs a;
    if (int rc = fill_args(d, a)) return rc;
    DESTA_CHECK_ARG(d->O, "attention_fwd: null output");
    DESTA_CHECK_ARG(d->o_row_stride % 8 == 0 && d->o_batch_stride % 8 == 0 && ((size_t)d->O & 15) == 0,
                    "attention_fwd: O must be 16-byte aligned with row / batch strides that are multiples of 8 elements");
    if (g_attn_opt[0] && !a.drop_thresh && a.Sq >= 128) {
        int hpb;
        const dim3 g8 = attn_grid8(a, d->head_dim, hpb);
        hipStream_t st = (hipStream_t)stream;
        if (d->head_dim == 128) {
            if (!a.causal) hipLaunchKernelGGL((attn_fwd8_k<128, false, 1>), g8, dim3(512), 0, st, a);
            else if (hpb == 4 && g_attn_opt[2]) hipLaunchKernelGGL((attn_fwd8_k<128, true, 4, 2, true>), g8, dim3(512), 0, st, a);
            else if (hpb == 4) hipLaunchKernelGGL((attn_fwd8_k<128, true, 4>), g8, dim3(512), 0, st, a);
            else if (hpb == 2) hipLaunchKernelGGL((attn_fwd8_k<128, true, 2>), g8, dim3(512), 0, st, a);
            else hipLaunchKernelGGL((attn_fwd8_k<128, true, 1>), g8, dim3(512), 0, st, a);
        } else {
            if (!a.causal && g_attn_opt[1]) hipLaunchKernelGGL((attn_fwd8_k<64, false, 1, 4, false>), g8, dim3(512), 0, st, a);
            else if (!a.causal && g_attn_opt[2]) hipLaunchKernelGGL((attn_fwd8_k<64, false, 1, 2, true>), g8, dim3(512), 0, st, a);
            else if (!a.causal) hipLaunchKernelGGL((attn_fwd8_k<64, false, 1>), g8, dim3(512), 0, st, a);
            else if (hpb == 2) hipLaunchKernelGGL((attn_fwd8_k<64, true, 2>), g8, dim3(512), 0, st, a);
            else hipLaunchKernelGGL((attn_fwd8_k<64, true, 1>), g8, dim3(512), 0, st, a);
        }
        DESTA_CHECK_LAUNCH("attention_fwd");
        return DESTA_OK;
    }
    const bool two = d->head_dim == 64 && a.Sq <= 64;
    dim3 grid((unsigned)((a.Sq + (two ? 63 : 127)) / (two ? 64 : 128)) * a.Hq * a.B);       // 1-D: attn_work_item() orders it per XCD                  // 64-row blocks of two waves (Q-Former queries)
    if (d->head_dim == 128) hipLaunchKernelGGL((attn_fwd_k<128, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else if (two && a.drop_thresh) hipLaunchKernelGGL((attn_fwd_k<64, true, 2>), grid, dim3(128), 0, (hipStream_t)stream, a);
    else if (two) hipLaunchKernelGGL((attn_fwd_k<64, false, 2>), grid, dim3(128), 0, (hipStream_t)stream, a);
    else if (a.drop_thresh) hipLaunchKernelGGL((attn_fwd_k<64, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL((attn_fwd_k<64, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    DESTA_CHECK_LAUNCH("attention_fwd");
    return DESTA_OK;
}

// Decode workspace (rows of more than one chunk only): (max, sum) pairs [batch][n_q_heads][chunks][2], padded to 16 bytes,
// then the unnormalised fp32 outputs [batch][n_q_heads][chunks][head_dim].
static_assert(DESTA_ATTN_DECODE_CHUNK % 64 == 0 && DESTA_ATTN_DECODE_CHUNK >= 64, "the decode chunk is a multiple of 64 keys");
namespace {
inline size_t decode_ml_floats(size_t items) { return (2 * items + 3) / 4 * 4; }
}
extern "C" int desta_attention_decode_chunk(void) { return DESTA_ATTN_DECODE_CHUNK; }
extern "C" size_t desta_attention_decode_workspace_bytes(int batch, int n_q_heads, int seq_k, int head_dim) {
    if (batch <= 0 || n_q_heads <= 0 || seq_k <= DESTA_ATTN_DECODE_CHUNK || head_dim <= 0) return 0;
    const size_t nch = ((size_t)seq_k + DESTA_ATTN_DECODE_CHUNK - 1) / DESTA_ATTN_DECODE_CHUNK;
    const size_t items = (size_t)batch * n_q_heads * nch;
    return (decode_ml_floats(items) + items * (size_t)head_dim) * sizeof(float);
}

extern "C" size_t desta_attention_verify_workspace_bytes(int batch, int n_q_heads, int seq_q, int seq_k, int head_dim) {
    if (n_q_heads <= 0 || seq_q <= 0 || (long)n_q_heads * seq_q > 0x7fffffffL) return 0;
    return desta_attention_decode_workspace_bytes(batch, n_q_heads * seq_q, seq_k, head_dim);     // one partial per (row, head, query row, chunk)
}

// The decode and verify entry points: `who` prefixes every message; k_scale != NULL selects the FP8-cache kernel; rows: the
// verify kernels (seq_q = 2..8 query rows per sequence under the causal mask) instead of the one-row ones.
static int decode_launch(const char* who, bool rows, const desta_attn_desc* d, const float* k_scale, const float* v_scale, int64_t sbs, int64_t srs,
                         void* workspace, size_t workspace_bytes, void* stream) {
    DESTA_CHECK_ARG(d, "%s: null descriptor", who);
    if (rows) {
        DESTA_CHECK_ARG(d->seq_q >= 2 && d->seq_q <= DESTA_ATTN_VERIFY_MAX_SEQ_Q, "%s: seq_q %d unsupported (2..%d query rows per sequence)", who,
                        d->seq_q, DESTA_ATTN_VERIFY_MAX_SEQ_Q);
        DESTA_CHECK_ARG(d->causal, "%s: causal must be 1 (query row j sees keys [kv_start, j + seq_k - seq_q])", who);
    } else {
        DESTA_CHECK_ARG(d->seq_q == 1, "%s: seq_q %d unsupported (one query row per sequence)", who, d->seq_q);
        DESTA_CHECK_ARG(!d->causal, "%s: causal must be 0 (the one query row sees every key of [kv_start, seq_k))", who);
    }
    DESTA_CHECK_ARG(d->head_dim == 128, "%s: head_dim %d unsupported (128)", who, d->head_dim);
    DESTA_CHECK_ARG(d->dropout_p == 0.f, "%s: dropout_p must be 0", who);
    DESTA_CHECK_ARG(!d->rope_cos_sin, "%s: rope_cos_sin must be NULL", who);
    DESTA_CHECK_ARG(!d->O_f32, "%s: O_f32 must be NULL", who);
    DESTA_CHECK_ARG(!d->dO && !d->dQ, "%s: dO and dQ must be NULL (forward only)", who);
    AttnArgs a;
    if (int rc = fill_args(d, a)) return rc;
    const int G = a.Hq / a.Hkv;
    DESTA_CHECK_ARG(G <= 8, "%s: group of %d query heads per kv head unsupported (at most 8)", who, G);
    const int R = G * a.Sq;
    DESTA_CHECK_ARG(R <= DESTA_ATTN_VERIFY_MAX_ROWS, "%s: group %d x seq_q %d = %d query rows per kv head unsupported (at most %d)", who, G, a.Sq, R,
                    DESTA_ATTN_VERIFY_MAX_ROWS);
    DESTA_CHECK_ARG(d->O && ((size_t)d->O & 15) == 0 && d->o_batch_stride % 8 == 0 && (!rows || d->o_row_stride % 8 == 0),
                    "%s: O must be 16-byte aligned with batch and row strides that are multiples of 8 elements", who);
    DESTA_CHECK_ARG((((size_t)d->Q | (size_t)d->K | (size_t)d->V) & 15) == 0 && d->q_batch_stride % 8 == 0 &&
                    d->k_batch_stride % 8 == 0 && d->v_batch_stride % 8 == 0,
                    "%s: Q, K, V must be 16-byte aligned with batch strides that are multiples of 8 elements", who);
    const int nch = (a.Sk + DESTA_ATTN_DECODE_CHUNK - 1) / DESTA_ATTN_DECODE_CHUNK;
    const size_t need = desta_attention_verify_workspace_bytes(a.B, a.Hq, a.Sq, a.Sk, 128);
    DESTA_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need && ((size_t)workspace & 15) == 0),
                    "%s: workspace of %zu bytes is too small or misaligned (%zu needed, 16-byte aligned)", who, workspace_bytes, need);
    DESTA_CHECK_ARG((long)a.B * a.Hkv * nch <= 0x7fffffffL, "%s: grid too large", who);
    float* ws_ml = (float*)workspace;
    float* ws_o = ws_ml ? ws_ml + decode_ml_floats((size_t)a.B * a.Hq * a.Sq * nch) : nullptr;
    const dim3 grid((unsigned)(a.B * a.Hkv * nch));
    hipStream_t st = (hipStream_t)stream;
#define DECODE_LAUNCH(GP)                                                                                                               \
    do {                                                                                                                                \
        if (k_scale) hipLaunchKernelGGL((attn_kv8_k<GP>), grid, dim3(256), 0, st, a, k_scale, v_scale, (long)sbs, (long)srs, ws_ml, ws_o, nch); \
        else hipLaunchKernelGGL((attn_decode_k<GP>), grid, dim3(256), 0, st, a, ws_ml, ws_o, nch);                                      \
    } while (0)
#define VERIFY_LAUNCH(RP)                                                                                                               \
    do {                                                                                                                                \
        if (k_scale) hipLaunchKernelGGL((attn_verify_kv8_k<RP>), grid, dim3(256), 0, st, a, k_scale, v_scale, (long)sbs, (long)srs, ws_ml, ws_o, nch); \
        else hipLaunchKernelGGL((attn_verify_k<RP>), grid, dim3(256), 0, st, a, ws_ml, ws_o, nch);                                      \
    } while (0)
    if (rows) {
        if (R <= 2) VERIFY_LAUNCH(2);
        else if (R <= 4) VERIFY_LAUNCH(4);
        else if (R <= 8) VERIFY_LAUNCH(8);
        else VERIFY_LAUNCH(16);
    } else if (G == 1) DECODE_LAUNCH(1);
    else if (G == 2) DECODE_LAUNCH(2);
    else if (G <= 4) DECODE_LAUNCH(4);
    else DECODE_LAUNCH(8);
#undef VERIFY_LAUNCH
#undef DECODE_LAUNCH
    DESTA_CHECK_LAUNCH(who);
    if (nch > 1) {
        const dim3 cgrid((unsigned)(((long)a.B * a.Hq * a.Sq + 7) / 8));
        if (rows) hipLaunchKernelGGL(attn_verify_combine_k, cgrid, dim3(256), 0, st, a, ws_ml, ws_o, nch);
        else hipLaunchKernelGGL(attn_decode_combine_k, cgrid, dim3(256), 0, st, a, ws_ml, ws_o, nch);
        DESTA_CHECK_LAUNCH(who);
    }
    return DESTA_OK;
}

extern "C" int desta_attention_decode(const desta_attn_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    return decode_launch("attention_decode", false, d, nullptr, nullptr, 0, 0, workspace, workspace_bytes, stream);
}

extern "C" int desta_attention_decode_kv8(const desta_attn_desc* d, const float* k_scale, const float* v_scale, int64_t scale_batch_stride,
                                          int64_t scale_row_stride, void* workspace, size_t workspace_bytes, void* stream) {
    DESTA_CHECK_ARG(d, "attention_decode_kv8: null descriptor");
    DESTA_CHECK_ARG(k_scale && v_scale && scale_batch_stride >= 0 && scale_row_stride > 0, "attention_decode_kv8: null scale or bad scale stride");
    return decode_launch("attention_decode_kv8", false, d, k_scale, v_scale, scale_batch_stride, scale_row_stride, workspace, workspace_bytes, stream);
}

extern "C" int desta_attention_verify(const desta_attn_desc* d, void* workspace, size_t workspace_bytes, void* stream) {
    return decode_launch("attention_verify", true, d, nullptr, nullptr, 0, 0, workspace, workspace_bytes, stream);
}

extern "C" int desta_attention_verify_kv8(const desta_attn_desc* d, const float* k_scale, const float* v_scale, int64_t scale_batch_stride,
                                          int64_t scale_row_stride, void* workspace, size_t workspace_bytes, void* stream) {
    DESTA_CHECK_ARG(d, "attention_verify_kv8: null descriptor");
    DESTA_CHECK_ARG(k_scale && v_scale && scale_batch_stride >= 0 && scale_row_stride > 0, "attention_verify_kv8: null scale or bad scale stride");
    return decode_launch("attention_verify_kv8", true, d, k_scale, v_scale, scale_batch_stride, scale_row_stride, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------------- FP8 KV cache -> bf16 staging slab (chunked prompt pass)
// The forward kernels read bf16: a prompt chunk that attends an FP8 cache first gets the visible slots of ONE layer back as
// bf16(e4m3(byte) * scale), the value attn_kv8_k forms in registers (the scale is a power of two: the product is exact).
// One lane takes 16 values of one head: a 16-byte load of cache bytes, the head's scale (the 8 lanes of a head share the
// address: one request), two 16-byte stores.  Block = KV8_DQ_SLOTS slots of one row; no LDS, no atomics.
namespace {
constexpr int KV8_DQ_SLOTS = 16;
__global__ __launch_bounds__(256) void kv8_dequant_k(const uint8_t* __restrict__ cache, long c_bs, long c_rs, const float* __restrict__ scale,
                                                     long s_bs, long s_rs, const int* __restrict__ kv_start, int n_heads, int slot1,
                                                     bf16_t* __restrict__ out, long o_bs, long o_rs) {
    const int b = blockIdx.y;
    const int kv_lo = kv_start ? max(0, min(kv_start[b], slot1)) : 0;
    const int first = max((int)blockIdx.x * KV8_DQ_SLOTS, kv_lo), last = min((int)blockIdx.x * KV8_DQ_SLOTS + KV8_DQ_SLOTS, slot1);
    if (first >= last) return;                                 // a block in front of kv_start: nothing is read or written
    const int per = n_heads * 8;                               // 16-value pieces of one slot
    const int items = (last - first) * per;
    cache += (long)b * c_bs;
    scale += (long)b * s_bs;
    out += (long)b * o_bs;
    for (int i = threadIdx.x; i < items; i += 256) {
        const int s = first + i / per, r = i % per;
        const uint4 q = *(const uint4*)(cache + (long)s * c_rs + 16 * r);
        const float sc = scale[(long)s * s_rs + (r >> 3)];
        union { bf16x8 v; u16x8 u; } lo, hi;
        lo.v = e4m3x8_to_bf16(make_uint2(q.x, q.y));
        hi.v = e4m3x8_to_bf16(make_uint2(q.z, q.w));
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            lo.u[e] = f2bf(bf2f(lo.u[e]) * sc);
            hi.u[e] = f2bf(bf2f(hi.u[e]) * sc);
        }
        bf16_t* o = out + (long)s * o_rs + 16 * r;
        *(u16x8*)o = lo.u;
        *(u16x8*)(o + 8) = hi.u;
    }
}
}  // namespace

extern "C" int desta_kv8_dequant(const uint8_t* kv_cache, int64_t kv_batch_stride, int64_t kv_row_stride, const float* kv_scale,
                                 int64_t scale_batch_stride, int64_t scale_row_stride, const int32_t* kv_start, int batch, int n_heads,
                                 int head_dim, int slot1, void* out_bf16, int64_t out_batch_stride, int64_t out_row_stride, void* stream) {
    DESTA_CHECK_ARG(kv_cache && kv_scale && out_bf16, "kv8_dequant: null cache, scale or output");
    DESTA_CHECK_ARG(head_dim == 128, "kv8_dequant: head_dim %d unsupported (128)", head_dim);
    DESTA_CHECK_ARG(batch > 0 && batch <= 65535 && n_heads > 0 && n_heads <= 4096, "kv8_dequant: bad batch %d or n_heads %d", batch, n_heads);
    DESTA_CHECK_ARG(slot1 > 0, "kv8_dequant: slot1 %d must be positive", slot1);
    const long w = (long)n_heads * 128;
    DESTA_CHECK_ARG(((size_t)kv_cache & 15) == 0 && kv_row_stride >= w && kv_row_stride % 16 == 0 && kv_batch_stride >= 0 && kv_batch_stride % 16 == 0,
                    "kv8_dequant: cache must be 16-byte aligned with row / batch strides that are multiples of 16 bytes, rows of at least %ld", w);
    DESTA_CHECK_ARG(scale_row_stride >= n_heads && scale_batch_stride >= 0, "kv8_dequant: bad scale stride");
    DESTA_CHECK_ARG(((size_t)out_bf16 & 15) == 0 && out_row_stride >= w && out_row_stride % 8 == 0 && out_batch_stride >= 0 && out_batch_stride % 8 == 0,
                    "kv8_dequant: output must be 16-byte aligned with row / batch strides that are multiples of 8 elements, rows of at least %ld", w);
    const dim3 grid((unsigned)((slot1 + KV8_DQ_SLOTS - 1) / KV8_DQ_SLOTS), (unsigned)batch);
    hipLaunchKernelGGL(kv8_dequant_k, grid, dim3(256), 0, (hipStream_t)stream, kv_cache, (long)kv_batch_stride, (long)kv_row_stride, kv_scale,
                       (long)scale_batch_stride, (long)scale_row_stride, (const int*)kv_start, n_heads, slot1, (bf16_t*)out_bf16,
                       (long)out_batch_stride, (long)out_row_stride);
    DESTA_CHECK_LAUNCH("kv8_dequant");
    return DESTA_OK;
}

// delta [batch][heads][seq_q], then (seq_q <= 64) up to ATTN_Q64_MAX_CHUNKS dQ partials of 64 x 64 floats per (batch, head)
#define ATTN_Q64_MAX_CHUNKS 4
extern "C" size_t desta_attention_bwd_workspace_floats(int batch, int n_q_heads, int seq_q) {
    const size_t delta = ((size_t)batch * n_q_heads * seq_q + 3) / 4 * 4;
    return delta + (seq_q <= 64 ? (size_t)ATTN_Q64_MAX_CHUNKS * batch * n_q_heads * (4096 + 128) : 0);   // + the K | V bias-gradient partial rows
}

// dQ and dK/dV are independent given delta.  The dK/dV grid is makespan-bound under the causal mask (320 blocks of very
// different length on 256 CUs, one block per CU: ~25 % of the CU-time idles behind the heaviest blocks), so the dQ kernel
// is launched on a side stream (fork after delta, join before returning to the caller's stream) and its blocks fill
// the CUs that dK/dV leaves idle.  Results are unchanged (no shared outputs, no atomics).
namespace {
struct BwdFork { hipStream_t side = nullptr; hipEvent_t fork = nullptr, join = nullptr; int handles = 0; };
BwdFork g_bwd_fork[16];
std::mutex g_bwd_fork_mu;                    // creation / release only; the data path reads a fully built entry
int g_bwd_concurrent = 1;
BwdFork* bwd_fork_locked(int dev) {
    BwdFork& f = g_bwd_fork[dev];
    if (!f.side) {
        hipStream_t s = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
        if (hipEventCreateWithFlags(&e0, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&e1, hipEventDisableTiming) != hipSuccess) {
            if (e0) (void)hipEventDestroy(e0);
            (void)hipStreamDestroy(s);
            return nullptr;
        }
        f.fork = e0; f.join = e1; f.side = s;      // published last: a half-built entry is never visible
    }
    return &f;
}
BwdFork* bwd_fork() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
    if (g_bwd_fork[dev].side) return &g_bwd_fork[dev];
    std::lock_guard<std::mutex> lk(g_bwd_fork_mu);
    return bwd_fork_locked(dev);
}
}  // namespace
extern "C" int desta_attention_set_concurrent_bwd(int on) { g_bwd_concurrent = on; return DESTA_OK; }
// desta_create / desta_destroy (api.hip): the current device's internal fork stream and events are shared by every stateless
// desta_attention_bwd caller of the process, so handles only COUNT references: the stream is made with the first handle (or
// lazily by the first backward call) and destroyed when the LAST handle of the device goes, never under another live handle.
// A process that never creates a handle keeps the lazily made stream for its lifetime.  desta_destroy must still not race a
// data-path call of the same device that is inside desta_attention_bwd (documented in include/desta_hip.h).
int desta_internal_reserve(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return DESTA_EINVAL;
    std::lock_guard<std::mutex> lk(g_bwd_fork_mu);
    BwdFork* f = bwd_fork_locked(dev);
    if (!f) return DESTA_ELAUNCH;
    ++f->handles;
    return DESTA_OK;
}
int desta_internal_release(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return DESTA_EINVAL;
    std::lock_guard<std::mutex> lk(g_bwd_fork_mu);
    BwdFork& f = g_bwd_fork[dev];
    if (f.handles > 0 && --f.handles > 0) return DESTA_OK;      // another handle of this device is alive
    if (f.side) { (void)hipStreamSynchronize(f.side); (void)hipStreamDestroy(f.side); }
    if (f.fork) (void)hipEventDestroy(f.fork);
    if (f.join) (void)hipEventDestroy(f.join);
    f = BwdFork();
    return DESTA_OK;
}

extern "C" int desta_attention_bwd(const desta_attn_desc* d, float* workspace, void* stream) {
    AttnArgs a;
    if (int rc = fill_args(d, a)) return rc;
    DESTA_CHECK_ARG(d->O && d->dO && d->lse && workspace && d->dQ, "attention_bwd: null argument");
    DESTA_CHECK_ARG((d->dK == nullptr) == (d->dV == nullptr), "attention_bwd: dK and dV go together");
    DESTA_CHECK_ARG(d->dq_row_stride % 4 == 0 && d->do_row_stride % 8 == 0 && d->o_row_stride % 8 == 0,
                    "attention_bwd: bad strides");
    a.delta = workspace;
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)a.B * a.Hq * a.Sq;
    const int G = d->head_dim / 8;
    dim3 gd((unsigned)((rows * G + 255) / 256));
    dim3 gk_((unsigned)((a.Sk + 127) / 128) * a.Hkv * a.B);
    if (a.rope_cs)
        DESTA_CHECK_ARG(g_attn_opt[0] && !g_attn_opt[3] && !a.drop_thresh && !a.O32 && a.Sq >= 128 && a.Sq == a.Sk && d->dq_row_stride % 8 == 0 &&
                        d->dq_batch_stride % 8 == 0 && ((size_t)d->dQ & 15) == 0 &&
                        (!d->dK || ((((d->dk_row_stride | d->dv_row_stride | d->dk_batch_stride | d->dv_batch_stride) & 7) == 0) &&
                                    (((size_t)d->dK | (size_t)d->dV) & 15) == 0)),
                        "attention_bwd: rope_cos_sin needs seq_q == seq_k >= 128, no dropout and 16-byte aligned dQ / dK / dV");
    if (g_attn_opt[0] && !g_attn_opt[3] && !a.drop_thresh && !a.O32 && a.Sq >= 128 && d->dq_row_stride % 8 == 0 && d->dq_batch_stride % 8 == 0 &&
        ((size_t)d->dQ & 15) == 0) {
        // 8-wave dQ kernel (computes delta itself and leaves it in the workspace), then dK / dV on the same stream
        int hpb;
        const dim3 g8 = attn_grid8(a, d->head_dim, hpb);
        // (the 8-wave dQ kernel on a side stream beside dK / dV, with delta by its own launch again, measured equal in the step:
        // 168.41 / 169.16 vs 168.54 / 169.16 ms in alternating runs on one box; removed)
        if (d->head_dim == 128) {
            if (!a.causal) hipLaunchKernelGGL((attn_bwd_dq8_k<128, false, 1>), g8, dim3(512), 0, st, a, workspace);
            else if (hpb == 4) hipLaunchKernelGGL((attn_bwd_dq8_k<128, true, 4>), g8, dim3(512), 0, st, a, workspace);
            else if (hpb == 2) hipLaunchKernelGGL((attn_bwd_dq8_k<128, true, 2>), g8, dim3(512), 0, st, a, workspace);
            else hipLaunchKernelGGL((attn_bwd_dq8_k<128, true, 1>), g8, dim3(512), 0, st, a, workspace);
            if (d->dK) {
                if (g_attn_opt[5] && a.causal) {                            // 64-key blocks: better balanced under the causal mask
                    dim3 gk2((unsigned)((a.Sk + 63) / 64) * a.Hkv * a.B);
                    hipLaunchKernelGGL((attn_bwd_dkdv_k<128, false, 2>), gk2, dim3(128), 0, st, a);
                } else hipLaunchKernelGGL((attn_bwd_dkdv_k<128, false>), gk_, dim3(256), 0, st, a);
            }
        } else {
            if (!a.causal) hipLaunchKernelGGL((attn_bwd_dq8_k<64, false, 1>), g8, dim3(512), 0, st, a, workspace);
            else if (hpb == 2) hipLaunchKernelGGL((attn_bwd_dq8_k<64, true, 2>), g8, dim3(512), 0, st, a, workspace);
            else hipLaunchKernelGGL((attn_bwd_dq8_k<64, true, 1>), g8, dim3(512), 0, st, a, workspace);
            if (d->dK) hipLaunchKernelGGL((attn_bwd_dkdv_k<64, false>), gk_, dim3(256), 0, st, a);
        }
        DESTA_CHECK_LAUNCH("attention_bwd");
        return DESTA_OK;
    }
    const bool q64 = d->head_dim == 64 && a.Sq <= 64 && a.Sk >= 256 && !a.causal && a.Hq == a.Hkv && d->dK && !a.rope_cs &&
                     ((d->q_batch_stride | d->k_batch_stride | d->v_batch_stride | d->do_batch_stride) & 7) == 0 && ((size_t)d->dO & 15) == 0 &&
                     (d->dq_batch_stride & 3) == 0 && ((size_t)d->dQ & 7) == 0;
    if (d->dkv_transposed)
        DESTA_CHECK_ARG(q64 && a.Sk % 4 == 0 && d->dkv_t_ld % 4 == 0 && d->dkv_t_ld >= (int64_t)a.B * a.Sk && (((size_t)d->dK | (size_t)d->dV) & 7) == 0,
                        "attention_bwd: dkv_transposed needs the one-query-tile path (head_dim 64, seq_q <= 64, seq_k >= 256 and a multiple of 4, no GQA) and 8-byte aligned dK / dV");
    if ((g_attn_opt[4] || d->dkv_transposed) && q64 &&
        (d->dkv_transposed || (((d->dk_row_stride | d->dv_row_stride | d->dk_batch_stride | d->dv_batch_stride) & 7) == 0 && (((size_t)d->dK | (size_t)d->dV) & 15) == 0))) {
        // one query tile (the Q-Former's cross-attention): delta, then dQ / dK / dV in ONE pass over K / V, then the chunk sum
        hipLaunchKernelGGL(attn_delta_k<64>, gd, dim3(256), 0, st, a, workspace);
        const int nkb = (a.Sk + 127) / 128;
        const int nch = nkb >= 8 ? ATTN_Q64_MAX_CHUNKS : (nkb >= 4 ? 2 : 1), bpc = (nkb + nch - 1) / nch;
        float* part = workspace + (rows + 3) / 4 * 4;
        float* bpart = d->dkv_bias_grad ? part + (size_t)ATTN_Q64_MAX_CHUNKS * a.B * a.Hq * 4096 : nullptr;
        dim3 gf((unsigned)(nch * a.B * a.Hq));
        if (d->dkv_transposed) {
            if (a.drop_thresh) hipLaunchKernelGGL((attn_bwd_q64_k<true, true>), gf, dim3(256), 0, st, a, part, bpart, bpc);
            else hipLaunchKernelGGL((attn_bwd_q64_k<false, true>), gf, dim3(256), 0, st, a, part, bpart, bpc);
            if (bpart) hipLaunchKernelGGL(attn_bias_sum_k, dim3((unsigned)(2 * a.Hq)), dim3(256), 0, st, (const float*)bpart,
                                          nch * a.B, 2 * a.Hq * 64, d->dkv_bias_grad);
        } else if (a.drop_thresh) hipLaunchKernelGGL((attn_bwd_q64_k<true, false>), gf, dim3(256), 0, st, a, part, bpart, bpc);
        else hipLaunchKernelGGL((attn_bwd_q64_k<false, false>), gf, dim3(256), 0, st, a, part, bpart, bpc);
        hipLaunchKernelGGL(attn_dq_sum_k, dim3((unsigned)(a.B * a.Hq)), dim3(256), 0, st, a, (const float*)part, nch);
        DESTA_CHECK_LAUNCH("attention_bwd");
        return DESTA_OK;
    }
    const bool two_q = d->head_dim == 64 && a.Sq <= 64;
    dim3 gq((unsigned)((a.Sq + (two_q ? 63 : 127)) / (two_q ? 64 : 128)) * a.Hq * a.B);
    dim3 gk((unsigned)((a.Sk + 127) / 128) * a.Hkv * a.B);
    if (d->head_dim == 128) {
        hipLaunchKernelGGL(attn_delta_k<128>, gd, dim3(256), 0, st, a, workspace);
        BwdFork* f = (g_bwd_concurrent && d->dK) ? bwd_fork() : nullptr;
        if (f && hipEventRecord(f->fork, st) == hipSuccess && hipStreamWaitEvent(f->side, f->fork, 0) == hipSuccess) {
            hipLaunchKernelGGL((attn_bwd_dkdv_k<128, false>), gk, dim3(256), 0, st, a);          // the long one first
            hipLaunchKernelGGL((attn_bwd_dq_k<128, false>), gq, dim3(256), 0, f->side, a);
            DESTA_CHECK_ARG(hipEventRecord(f->join, f->side) == hipSuccess && hipStreamWaitEvent(st, f->join, 0) == hipSuccess,
                            "attention_bwd: could not join the side stream");
        } else {
            hipLaunchKernelGGL((attn_bwd_dq_k<128, false>), gq, dim3(256), 0, st, a);
            if (d->dK) hipLaunchKernelGGL((attn_bwd_dkdv_k<128, false>), gk, dim3(256), 0, st, a);
        }
    } else {
        hipLaunchKernelGGL(attn_delta_k<64>, gd, dim3(256), 0, st, a, workspace);
        const bool two = two_q;
        if (a.drop_thresh) {
            if (two) hipLaunchKernelGGL((attn_bwd_dq_k<64, true, 2>), gq, dim3(128), 0, st, a);
            else hipLaunchKernelGGL((attn_bwd_dq_k<64, true>), gq, dim3(256), 0, st, a);
            if (d->dK) hipLaunchKernelGGL((attn_bwd_dkdv_k<64, true>), gk, dim3(256), 0, st, a);
        } else {
            if (two) hipLaunchKernelGGL((attn_bwd_dq_k<64, false, 2>), gq, dim3(128), 0, st, a);
            else hipLaunchKernelGGL((attn_bwd_dq_k<64, false>), gq, dim3(256), 0, st, a);
            if (d->dK) hipLaunchKernelGGL((attn_bwd_dkdv_k<64, false>), gk, dim3(256), 0, st, a);
        }
    }
    DESTA_CHECK_LAUNCH("attention_bwd");
    return DESTA_OK;
}
