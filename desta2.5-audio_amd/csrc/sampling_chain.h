// The body of the chain kernel, included by sampling.hip once per kernel (no include guard on purpose):
//   CHAIN_KERNEL sample_chain_k,     CHAIN_TR 0: HF's chain up to min-p and the draw, the kernel of desta_sample_bf16 / desta_sample_rows_bf16
//   CHAIN_KERNEL sample_truncated_k, CHAIN_TR 1: the same with steps 7-9 (typical-p, epsilon, eta) in front of the draw, and a `Truncation tr`
// The preprocessor, not a template under two thin kernels: with the body in a __forceinline__ device function hipcc compiles
// sample_chain_k's draw passes differently (the precise expf of min-p computed for every element and selected afterwards, instead
// of the branch that skips it), which measured 13-17 us per launch on the MI355X.  With CHAIN_TR 0 the text below is the kernel as
// it was before steps 7-9 existed.
#if CHAIN_TR
#define CHAIN_TR_PARAM Truncation tr,
#else
#define CHAIN_TR_PARAM
#endif
__global__ __launch_bounds__(SNT) void CHAIN_KERNEL(const bf16_t* __restrict__ x, long ld, int cols, const long* __restrict__ hist,
                                                    long hist_ld, int hist_len, const long* __restrict__ tail, long tail_ld, int width,
                                                    float penalty, float temp, int top_k, float top_p, float min_p, CHAIN_TR_PARAM
                                                    unsigned seed_lo, unsigned seed_hi, unsigned step, long* __restrict__ out,
                                                    unsigned char* __restrict__ keep_mask) {
    __shared__ u64 bins[SBINS];
    __shared__ unsigned pen_bits[PEN_MAX_COLS / 32];
    __shared__ u64 wred[SNT / 64];
    __shared__ u64 sel[2];
    const GroupRow g = group_row(width);
    const int tid = threadIdx.x, r = g.r;
    const bf16_t* row = x + (long)r * ld;
    const bool vec = ((uintptr_t)row & 15) == 0;
    const bool pen = penalty != 1.0f && hist_len + g.j > 0;
    if (pen) build_penalty_bits(pen_bits, cols, g, hist, hist_ld, hist_len, tail, tail_ld);
    auto score = [&](int c, bf16_t b) -> float { return penalised(pen_bits, pen, penalty, c, b); };

    auto tval = [&](int c, bf16_t b) -> float { return score(c, b) / temp; };   // TemperatureLogitsWarper: an fp32 division
    const bool do_k = top_k > 0 && top_k < cols;
    const bool do_p = top_p < 1.0f;

    // pass 0: row maximum (+ the first top-k digit histogram)
    if (do_k) {
        for (int i = tid; i < SBINS; i += SNT) bins[i] = 0ull;
        __syncthreads();
    }
    unsigned kmax = 0u;
    row_strided(row, cols, vec, [&](int c, bf16_t b) {
        const unsigned k = f32_key(tval(c, b));
        kmax = k > kmax ? k : kmax;
        if (do_k) atomicAdd(&bins[k >> 20], 1ull);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned ok = __shfl_xor(kmax, o, 64);
        kmax = ok > kmax ? ok : kmax;
    }
    if ((tid & 63) == 0) wred[tid >> 6] = kmax;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SNT / 64; ++w) kmax = (unsigned)wred[w] > kmax ? (unsigned)wred[w] : kmax;
    const float tmax = key_f32(kmax);
    auto mass = [&](float t) -> u64 {                            // exp(t - t_max) in 2^-40 units (0 for -inf)
        return t > -INFINITY ? (u64)(__expf(t - tmax) * MASS_ONE) : 0ull;
    };

    // TopKLogitsWarper: keep t >= the k-th largest t (ties with it included) = the key of ascending rank cols - k
    unsigned kthr = 0u;
    if (do_k) {
        u64 m = (u64)(cols - top_k);
        unsigned prefix = 0u;
        for (int pass = 0; pass < 3; ++pass) {
            const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
            if (pass > 0) {
                bins[tid] = 0ull;
                __syncthreads();
                row_strided(row, cols, vec, [&](int c, bf16_t b) {
                    const unsigned k = f32_key(tval(c, b));
                    if ((k >> (shift + 10)) == (prefix >> (shift + 10))) atomicAdd(&bins[(k >> shift) & 1023u], 1ull);
                });
                __syncthreads();
                select_bin<1>(bins, wred, sel, [&](u64) { return m; });
            } else {
                __syncthreads();
                select_bin<SBINS / SNT>(bins, wred, sel, [&](u64) { return m; });
            }
            prefix |= (unsigned)sel[0] << shift;
            m -= sel[1];
            __syncthreads();
        }
        kthr = prefix;
    }

    // TopPLogitsWarper over the top-k survivors: keep key >= the smallest key K whose ascending cumulative mass exceeds
    // (1 - top_p) * Z; tokens tied with K are all kept
    unsigned pthr = 0u;
    if (do_p) {
        u64 m = 0;
        unsigned prefix = 0u;
        for (int pass = 0; pass < 3; ++pass) {
            const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
            const int nb = pass == 0 ? SBINS : 1024;
            for (int i = tid; i < nb; i += SNT) bins[i] = 0ull;
            __syncthreads();
            row_strided(row, cols, vec, [&](int c, bf16_t b) {
                const float t = tval(c, b);
                const unsigned k = f32_key(t);
                if (k >= kthr && (pass == 0 || (k >> (shift + 10)) == (prefix >> (shift + 10))))
                    atomicAdd(&bins[pass == 0 ? (k >> 20) : ((k >> shift) & 1023u)], mass(t));
            });
            __syncthreads();
            if (pass == 0) {
                select_bin<SBINS / SNT>(bins, wred, sel, [&](u64 total) {
                    u64 cut = (u64)((1.0 - (double)top_p) * (double)total);
                    cut = cut < total ? cut : total - 1;                 // the maximum (mass 2^40) is always kept
                    m = cut;
                    return cut;
                });
            } else {
                select_bin<1>(bins, wred, sel, [&](u64) { return m; });
            }
            prefix |= (unsigned)sel[0] << shift;
            m -= sel[1];
            __syncthreads();
        }
        pthr = prefix;
    }
    const unsigned thr = kthr > pthr ? kthr : pthr;

    // MinPLogitsWarper on the survivors: p_i >= min_p * p_max  <=>  exp(t_i - t_max) >= min_p; then the kept masses per
    // thread over a contiguous index chunk, so the draw's prefix sum runs in index order
    // (a -inf score, as desta_mask_tokens_bf16 leaves it, has mass 0 and is never kept)
#if !CHAIN_TR
    auto kept = [&](float t) -> bool { return t > -INFINITY && f32_key(t) >= thr && (min_p <= 0.f || expf(t - tmax) >= min_p); };
#else
    auto kept6 = [&](float t) -> bool { return t > -INFINITY && f32_key(t) >= thr && (min_p <= 0.f || expf(t - tmax) >= min_p); };

    // Steps 7-9 tighten three values as they go, so `kept` always means "survives every step so far": dthr (typical-p: the key
    // of D, keep d <= D), ethr (epsilon / eta: keep exp(a) >= ethr, i.e. p >= the cut-off, or a tie with the survivors'
    // maximum key smax) and cmean (c, which d = |a - c| is measured from).  A step that is off costs a uniform test per element.
    unsigned dthr = 0xffffffffu, smax = 0u;
    float ethr = 0.f, cmean = 0.f;
    const bool do_typ = tr.typical_p < 1.0f, do_cut = tr.epsilon_cutoff > 0.f || tr.eta_cutoff > 0.f;
    auto dkey = [&](float t) -> unsigned { return f32_key(fabsf((t - tmax) - cmean)); };
    auto kept = [&](float t) -> bool {
        return kept6(t) && (!do_typ || dkey(t) <= dthr) && (!do_cut || __expf(t - tmax) >= ethr || f32_key(t) == smax);
    };
    {
        __shared__ u64 red[3][SNT / 64];
        // over the survivors so far: Z = sum of masses, EA = sum of exp(a) * (-a) in 2^-40 units (x e^-x <= 1 / e: no overflow
        // below 2^60), and their largest key
        u64 Z = 0, EA = 0;
        auto stats = [&]() {
            u64 z = 0, ea = 0;
            unsigned mx = 0u;
            row_strided(row, cols, vec, [&](int c, bf16_t b) {
                const float t = tval(c, b);
                if (kept(t)) {
                    const float a = t - tmax;
                    z += mass(t);
                    ea += (u64)(__expf(a) * -a * MASS_ONE);
                    const unsigned k = f32_key(t);
                    mx = k > mx ? k : mx;
                }
            });
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                z += __shfl_xor(z, o, 64);
                ea += __shfl_xor(ea, o, 64);
                const unsigned ok = __shfl_xor(mx, o, 64);
                mx = ok > mx ? ok : mx;
            }
            __syncthreads();                                     // the previous call's readers are done
            if ((tid & 63) == 0) red[0][tid >> 6] = z, red[1][tid >> 6] = ea, red[2][tid >> 6] = mx;
            __syncthreads();
            Z = 0, EA = 0, mx = 0u;
#pragma unroll
            for (int w = 0; w < SNT / 64; ++w) {
                Z += red[0][w];
                EA += red[1][w];
                mx = (unsigned)red[2][w] > mx ? (unsigned)red[2][w] : mx;
            }
            smax = mx;
        };

        // TypicalLogitsWarper: c = sum p a, d = |a - c| (= |-log p - H|), keep d <= D, the smallest d whose ascending cumulative
        // mass reaches typical_p * Z; tokens tied with D are all kept
        if (tr.typical_p < 1.0f) {
            stats();
            if (Z > 0) {                                         // (a row without a finite score keeps nothing anyway)
                cmean = -(float)((double)EA / (double)Z);
                u64 m = 0;
                unsigned prefix = 0u;
                for (int pass = 0; pass < 3; ++pass) {
                    const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
                    const int nb = pass == 0 ? SBINS : 1024;
                    for (int i = tid; i < nb; i += SNT) bins[i] = 0ull;
                    __syncthreads();
                    row_strided(row, cols, vec, [&](int c, bf16_t b) {
                        const float t = tval(c, b);
                        if (!kept6(t)) return;
                        const unsigned k = dkey(t);
                        if (pass == 0 || (k >> (shift + 10)) == (prefix >> (shift + 10)))
                            atomicAdd(&bins[pass == 0 ? (k >> 20) : ((k >> shift) & 1023u)], mass(t));
                    });
                    __syncthreads();
                    if (pass == 0) {
                        select_bin<SBINS / SNT>(bins, wred, sel, [&](u64 total) {
                            u64 need = (u64)ceil((double)tr.typical_p * (double)total);   // smallest D with mass(d <= D) >= need
                            need = need < 1 ? 1 : (need > total ? total : need);
                            m = need - 1;
                            return m;
                        });
                    } else {
                        select_bin<1>(bins, wred, sel, [&](u64) { return m; });
                    }
                    prefix |= (unsigned)sel[0] << shift;
                    m -= sel[1];
                    __syncthreads();
                }
                dthr = prefix;
            }
        }
        // EpsilonLogitsWarper over the survivors of typical-p: keep p >= epsilon, or a tie with THEIR maximum
        if (tr.epsilon_cutoff > 0.f) {
            stats();
            ethr = (float)((double)tr.epsilon_cutoff * (double)Z * (1.0 / (double)MASS_ONE));
        }
        // EtaLogitsWarper over the survivors of epsilon: H = log Z - sum p a, keep p >= min(eta, sqrt(eta) exp(-H)), or a tie
        // with the maximum (the maximum of step 8's input survives step 8, so smax does not move)
        if (tr.eta_cutoff > 0.f) {
            stats();
            if (Z > 0) {
                const float zr = (float)Z * (1.0f / MASS_ONE);
                const float H = logf(zr) + (float)((double)EA / (double)Z);
                const float theta = fminf(tr.eta_cutoff, sqrtf(tr.eta_cutoff) * expf(-H));
                ethr = fmaxf(ethr, theta * zr);
            }
        }
    }
#endif
    const int chunk = (((cols + SNT - 1) / SNT) + 7) & ~7;
    const int c0 = min(cols, tid * chunk), c1 = min(cols, c0 + chunk);
    u64 mine = 0;
    row_chunk(row, c0, c1, vec, [&](int c, bf16_t b) {
        const float t = tval(c, b);
        const bool keep = kept(t);
        if (keep) mine += mass(t);
        if (keep_mask) keep_mask[(long)r * cols + c] = keep ? 1 : 0;
    });
    bins[tid] = mine;
    __syncthreads();
    u64 target = 0;
    select_bin<1>(bins, wred, sel, [&](u64 total) {
        const unsigned u = desta_rng32(seed_lo, seed_hi, ((unsigned long)(step + (unsigned)g.j) << 32) | (unsigned)g.b);   // uint32 sum: wraps
        target = (u64)((double)(u >> 8) * (1.0 / 16777216.0) * (double)total);   // < total
        if (total == 0) sel[0] = 0, sel[1] = 0;                                   // no finite score: token 0 (below)
        return target;
    });
    if (tid == (int)sel[0]) {
        const u64 rem = target - sel[1];
        u64 run = 0;
        int tok = -1;
        row_chunk(row, c0, c1, vec, [&](int c, bf16_t b) {
            if (tok >= 0) return;
            const float t = tval(c, b);
            if (kept(t)) {
                run += mass(t);
                if (run > rem) tok = c;
            }
        });
        out[r] = tok >= 0 ? tok : 0;
    }
}
#undef CHAIN_TR_PARAM
#undef CHAIN_KERNEL
#undef CHAIN_TR
