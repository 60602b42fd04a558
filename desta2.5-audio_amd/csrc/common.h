// Shared device helpers for the DeSTA2.5 gfx950 kernels (wave = 64 lanes, CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef uint16_t bf16_t;                                            // raw bf16 bits in HBM
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;          // MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) float f32x4;            // 16x16 accumulator
typedef __attribute__((ext_vector_type(16))) float f32x16;          // 32x32 accumulator
typedef __attribute__((ext_vector_type(4))) unsigned short u16x4;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

#define DESTA_OK 0
#define DESTA_EINVAL (-1)
#define DESTA_ELAUNCH (-2)

void desta_set_error(const char* fmt, ...);

#define DESTA_CHECK_ARG(cond, ...)                  \
    do {                                            \
        if (!(cond)) {                              \
            desta_set_error(__VA_ARGS__);           \
            return DESTA_EINVAL;                    \
        }                                           \
    } while (0)

#define DESTA_CHECK_LAUNCH(name)                                                  \
    do {                                                                          \
        hipError_t e__ = hipGetLastError();                                       \
        if (e__ != hipSuccess) {                                                  \
            desta_set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return DESTA_ELAUNCH;                                                 \
        }                                                                         \
    } while (0)

// f32 -> bf16, round-to-nearest-even; plain cast lowers to v_cvt_pk_bf16_f32 on gfx950 and keeps NaN.
__device__ __forceinline__ bf16_t f2bf(float x) {
    __bf16 b = (__bf16)x;
    return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ float bf2f(bf16_t b) {
    return __builtin_bit_cast(float, ((unsigned)b) << 16);
}

// Power-of-two e4m3 scale of one row (desta_quantize_rows_e4m3, the FP8 KV cache): scale = 2^e, e the smallest integer with
// amax * 2^-e <= 448.
// e for one row from the bits of its largest |w| (bf16, sign cleared; integer order == value order)
__device__ __forceinline__ int e4m3_row_exponent(unsigned amax_bits) {
    int ex = (int)(amax_bits >> 7), frac = (int)(amax_bits & 0x7f);
    if (ex == 0) {                                      // bf16 subnormal: frac * 2^-133, normalise
        const int top = 31 - __clz(frac);
        ex = top - 6;                                   // value = 1.f * 2^(top - 133) = 2^(ex - 127)
        frac = (frac << (7 - top)) & 0x7f;
    }
    // amax = (1 + frac/128) * 2^(ex-127);  448 = 1.75 * 2^8:  mantissa <= 1.75 fits under 2^8, a larger one needs one more
    return ex - 127 - 8 + (frac > 96 ? 1 : 0);
}

__device__ __forceinline__ float pow2f(int e) {       // 2^e as fp32 bits, subnormal results included (e >= -149)
    return __uint_as_float(e >= -126 ? (unsigned)(e + 127) << 23 : 1u << (e + 149));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Block-wide sum for blockDim.x == NT (multiple of 64); `red` is NT/64 floats of LDS.
template <int NT>
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}
template <int NT>
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) t = fmaxf(t, red[i]);
    return t;
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
// GELU(erf) for bf16-rounded outputs: erf by Abramowitz-Stegun 7.1.26 (|err| < 1.5e-7 absolute, far below the
// 2^-9 relative rounding of the bf16 store) — 1 v_exp + 1 v_rcp + 7 FMA instead of the ~30-instruction erff.
__device__ __forceinline__ float gelu_erf_fast(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float e = 1.0f - poly * t * __expf(-z * z);          // erf(|x|/sqrt2)
    return 0.5f * x * (1.0f + copysignf(e, x));
}
__device__ __forceinline__ float gelu_erf_grad(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}

// Counter-based dropout RNG: 32 random bits for element `idx` of the tensor/stream identified by `seed` (stateless, so forward
// and backward recompute identical masks).  Two-multiply integer finaliser ("lowbias32": xorshift 16 / * 0x7feb352d / xorshift 15 /
// * 0x846ca68b / xorshift 16): 32-bit integer multiplies are quarter rate on CDNA4 and the previous murmur3-style mix (5 of them)
// was a large part of the dropout attention kernels' time (cross-attention forward 42 us without dropout, 80 us with; 70 us now).
// The seed words and the high index word enter ADDITIVELY through two more multiplies that are wave-uniform in every caller
// (scalar unit) — which alone makes every stream a SHIFTED COPY of one 2^32-pair sequence (mask(seed + d, idx) == mask(seed, idx +
// d * 0x9e3779b9): with the per-forward seed step of round 3, the masks of step t + 60 were the masks of step t shifted by 8.87 M
// pairs, inside the 30.7 M-pair cross-attention tensor).  Round 4: a second, independently mixed word of the seed (`key`,
// wave-uniform as well) is xored in BETWEEN the two multiplies of the finaliser, so two seeds select two different functions of the
// index, and the host derives every site's seed with splitmix64 from (rank seed, forward count, layer, site) instead of packing
// bit fields.  Checked on the host by tests/test_dropout_mask_host.py with the numpy restatement of tests/dropout_reference.py
// (p = 0.1, 2^22 elements, every figure held to 4.5 sigma: 6.6e-4 on the keep fraction, 2.2e-3 on a correlation, 1.1e-3 on a
// bit): keep fraction 0.89989; correlation between the streams of seeds s and s + d for d = 1, 16, 256, 512, 256 * 60,
// 256 * 1000 all |r| < 9e-4, and at the shift the additive offset implies (d = 256 * 60: 8 870 912 pairs) 8e-4 — it is exactly
// 1.0 without the key; seed_hi neighbours 4e-4; adjacent elements 2e-4; every output bit 0.4995..0.5004.  (Earlier figures from
// an uncommitted script at 4-10 M pairs — 0.90004, 6e-4, 1e-3, 4e-5, 4e-4, 0.4998..0.5005 — are the same statement at other
// seeds and sizes: all of these are sampling noise around 0.9, 0 and 0.5.)  tests/test_gpu_dropout_mask.py holds every kernel
// that draws a mask to that restatement, pair for pair.
__device__ __forceinline__ unsigned desta_rng32(unsigned seed_lo, unsigned seed_hi, unsigned long idx) {
    const unsigned key = (seed_lo ^ (seed_hi * 0x632be5abu)) * 0xc2b2ae35u;
    unsigned x = (unsigned)idx + seed_lo * 0x9e3779b9u + ((unsigned)(idx >> 32) + seed_hi) * 0x85ebca6bu;
    x ^= x >> 16; x *= 0x7feb352du; x ^= (x >> 15) ^ key; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// Dropout decision of element `idx`: ONE 32-bit hash serves the element PAIR (idx >> 1) — the even element takes the low 16
// bits, the odd one the high 16 — kept iff its 16 bits >= thresh16 = round(p * 65536) (p resolved to 1.5e-5).  Kernels that
// hold adjacent elements on one lane (attention probabilities: adjacent keys) hash once per pair; the integer multiplies of
// the hash are quarter rate on CDNA4 and were most of the Q-Former attention kernels' VALU time at one hash per element.
__host__ __device__ inline unsigned desta_drop_thresh(float p) {
    const double t = (double)p * 65536.0 + 0.5;
    return t >= 65535.0 ? 0xffffu : (t < 1.0 ? 1u : (unsigned)t);
}
__device__ __forceinline__ bool desta_keep(unsigned seed_lo, unsigned seed_hi, unsigned long idx, unsigned thresh16) {
    const unsigned h = desta_rng32(seed_lo, seed_hi, idx >> 1);
    return ((idx & 1) ? (h >> 16) : (h & 0xffffu)) >= thresh16;
}

// XCD-aware bijective remap of a 1-D block id: blocks that share an XCD (id % 8) get a contiguous
// chunk of the logical grid so neighbouring tiles hit the same L2 (guide T1, bijective form).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, k = bid >> 3;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + k;
}
