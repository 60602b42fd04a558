// Row-wise OCP e4m3 quantisation of a frozen bf16 weight [rows, cols] for the weight-only FP8 decode path
// (desta_gemm_w8a16_nt streams the bytes; the LLM of modeling_desta25.py:1419-1427 is frozen, so this runs once).
//
// One fp32 scale per row and it is a power of two: scale = 2^e, e the smallest integer with amax(row) * 2^-e <= 448 (the
// largest e4m3fn value); an all-zero row gets 1.  q = e4m3fn(w * 2^-e), round to nearest even; nothing exceeds 448 by
// construction, so no value saturates.  The exponent comes from the bits of amax (integer arithmetic, no log2), and
// q * scale is exactly representable in bf16.
#include "common.h"
#include "desta_hip.h"

namespace {

__global__ __launch_bounds__(256) void quantize_rows_e4m3_k(const bf16_t* __restrict__ w, int cols, long ld, uint8_t* __restrict__ q,
                                                            float* __restrict__ scale) {
    __shared__ unsigned sh[4];
    const long row = blockIdx.x;
    const bf16_t* wr = w + row * ld;
    uint8_t* qr = q + row * (long)cols;
    const bool vec = (cols & 7) == 0 && (ld & 7) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)q & 7) == 0;
    unsigned amax = 0;
    if (vec) {
        for (int c = threadIdx.x * 8; c < cols; c += 256 * 8) {
            const u16x8 v = *(const u16x8*)(wr + c);
#pragma unroll
            for (int i = 0; i < 8; ++i) amax = max(amax, (unsigned)(v[i] & 0x7fff));
        }
    } else {
        for (int c = threadIdx.x; c < cols; c += 256) amax = max(amax, (unsigned)(wr[c] & 0x7fff));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = max(amax, (unsigned)__shfl_xor((int)amax, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
    const int e = amax ? e4m3_row_exponent(amax) : 0;
    if (threadIdx.x == 0) scale[row] = pow2f(e);
    if (vec) {
        for (int c = threadIdx.x * 8; c < cols; c += 256 * 8) {
            const u16x8 v = *(const u16x8*)(wr + c);
            float f[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) f[i] = ldexpf(bf2f(v[i]), -e);
            int lo = 0, hi = 0;
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
            *(uint2*)(qr + c) = make_uint2((unsigned)lo, (unsigned)hi);
        }
    } else {
        for (int c = threadIdx.x; c < cols; c += 256) {
            const float f = ldexpf(bf2f(wr[c]), -e);
            qr[c] = (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(f, 0.f, 0, false) & 0xff);
        }
    }
}

}  // namespace

extern "C" int desta_quantize_rows_e4m3(const void* w_bf16, int rows, int cols, int64_t ld, uint8_t* q, float* scale, void* stream) {
    DESTA_CHECK_ARG(w_bf16 && q && scale, "quantize_rows_e4m3: null operand");
    DESTA_CHECK_ARG(rows > 0 && cols > 0 && ld >= cols, "quantize_rows_e4m3: bad shape rows=%d cols=%d ld=%ld", rows, cols, (long)ld);
    hipLaunchKernelGGL(quantize_rows_e4m3_k, dim3(rows), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w_bf16, cols, (long)ld, q, scale);
    DESTA_CHECK_LAUNCH("quantize_rows_e4m3");
    return DESTA_OK;
}
