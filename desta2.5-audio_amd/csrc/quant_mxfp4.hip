// OCP MXFP4 quantisation of a frozen bf16 weight [rows, cols] for the weight-only 4-bit decode path (desta_gemm_w4a16_nt
// streams the nibbles; the LLM of modeling_desta25.py:1419-1427 is frozen, so this runs once per weight).
//
// A block is 32 consecutive k of one row.  Its scale is the e8m0 byte e + 127, e the smallest integer with amax * 2^-e <= 7
// (7 = 1.75 * 2^2: the e4m3 rule of quant_fp8.hip with 2 + 1 in place of 8 + 1); an all-zero block gets 127.  The exponent comes
// from the bits of amax (integer arithmetic, no log2).  An element is e2m1(w * 2^-e): nearest grid value of 0 0.5 1 1.5 2 3 4 6,
// ties to the even code, the magnitude saturating at 6 ((6, 7] -> 6); bit 3 of the code is the sign.  Byte j of a row holds
// element 2j in bits 3..0 and 2j + 1 in bits 7..4.  code * 2^e has two significant bits: exactly a bf16 value.
// One thread owns one block: four 16-byte loads, one 16-byte store, one scale byte; no scratch, no LDS.
#include "common.h"
#include "desta_hip.h"

namespace {

__device__ __forceinline__ unsigned e2m1_code(bf16_t w, int e) {
    const float x = ldexpf(bf2f(w & 0x7fff), -e);                        // exact: a power-of-two scaling, <= 7
    const unsigned mag = (x > 0.25f) + (x >= 0.75f) + (x > 1.25f) + (x >= 1.75f) + (x > 2.5f) + (x >= 3.5f) + (x > 5.0f);
    return mag | ((unsigned)(w >> 15) << 3);
}

__global__ __launch_bounds__(256) void quantize_rows_mxfp4_k(const bf16_t* __restrict__ w, int rows, int nblk, long ld,
                                                             uint8_t* __restrict__ q, long ldq, uint8_t* __restrict__ scale, long lds) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)rows * nblk) return;
    const long row = idx / nblk;
    const int b = (int)(idx % nblk);
    const bf16_t* wr = w + row * ld + b * 32;
    u16x8 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *(const u16x8*)(wr + 8 * i);
    unsigned amax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) amax = max(amax, (unsigned)(v[i][j] & 0x7fff));
    // amax = (1 + frac / 128) * 2^(ex - 127): a mantissa <= 1.75 fits under 7 = 1.75 * 2^2, a larger one needs one more
    const int e = amax ? e4m3_row_exponent(amax) + 6 : 0;
    scale[row * lds + b] = (uint8_t)min(max(e + 127, 0), 254);
    unsigned o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned pk = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) pk |= e2m1_code(v[i][j], e) << (4 * j);
        o[i] = pk;
    }
    *(uint4*)(q + row * ldq + b * 16) = make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace

extern "C" int desta_quantize_rows_mxfp4(const void* w_bf16, int rows, int cols, int64_t ld, uint8_t* q, int64_t ldq,
                                         uint8_t* scale_e8m0, int64_t lds, void* stream) {
    DESTA_CHECK_ARG(w_bf16 && q && scale_e8m0, "quantize_rows_mxfp4: null operand");
    DESTA_CHECK_ARG(rows > 0 && cols > 0 && cols % 32 == 0 && ld >= cols, "quantize_rows_mxfp4: bad shape rows=%d cols=%d (a multiple of 32) ld=%ld",
                    rows, cols, (long)ld);
    DESTA_CHECK_ARG(ld % 8 == 0 && ((uintptr_t)w_bf16 % 16) == 0, "quantize_rows_mxfp4: w must be 16-byte aligned and ld a multiple of 8");
    DESTA_CHECK_ARG(ldq % 16 == 0 && ldq >= cols / 2 && ((uintptr_t)q % 16) == 0, "quantize_rows_mxfp4: q must be 16-byte aligned, ldq=%ld a multiple of 16 and >= cols / 2",
                    (long)ldq);
    DESTA_CHECK_ARG(lds >= cols / 32, "quantize_rows_mxfp4: lds=%ld < cols / 32", (long)lds);
    const int nblk = cols / 32;
    const long total = (long)rows * nblk;
    hipLaunchKernelGGL(quantize_rows_mxfp4_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)w_bf16, rows, nblk, (long)ld, q, (long)ldq, scale_e8m0, (long)lds);
    DESTA_CHECK_LAUNCH("quantize_rows_mxfp4");
    return DESTA_OK;
}
