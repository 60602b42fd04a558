"""Float64 reference of weight-only MXFP4 decode: the quantiser of csrc/quant_mxfp4.hip (desta_quantize_rows_mxfp4) and the W4A16
GEMM of csrc/gemm_bf16.hip (desta_gemm_w4a16_nt), with per-element bounds in the notation of gemm_reference.py (ulp, H, F, T, S).
Plain torch, float64, device-agnostic; imported by tests/test_mxfp4_decode_host.py and tests/test_gpu_mxfp4_decode.py.

Format (include/desta_hip.h).  A block is 32 consecutive k of one weight row.  e = the smallest integer with amax 2^-e <= 7, in
exact integer form on frexp(amax) = m 2^ex: e = ex - 3 + (m > 0.875); an all-zero block has e = 0.  The scale byte is e + 127
(e8m0).  An element is w 2^-e rounded to the nearest of 0 0.5 1 1.5 2 3 4 6, ties to the even CODE (0.25 -> 0, 0.75 -> 1,
1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), the magnitude saturating at 6; code bit 3 is the sign.  Byte j of a row holds
element 2j in bits 3..0 and 2j + 1 in bits 7..4.  code 2^e has two significant bits and is exactly a bf16 value.

    quantize_ref(w, rule="le7") -> (codes uint8 [rows, K] in 0..15, e int32 [rows, K / 32])
    code_values(codes)          -> float64 grid values with sign
    dequant(codes, e)           -> float64 [rows, K];  dequant_bf16 -> the same as bf16, asserting exactness
    pack(codes)                 -> uint8 [rows, K / 2];  scale_bytes(e) -> uint8 [rows, K / 32]

The GEMM.  v = alpha sum_k A[m,k] W[n,k] on the bf16 activations (a_rms_weight: on A' = bf16(w bf16(x rstd)), gemm_reference's
definition) and the DEQUANTISED weight W = code 2^e, so quantisation error is not part of the operation; then the epilogue of
desta_gemm_bf16_nt's decode forms: act 0 with an optional bf16 residual and a bf16 or fp32 store, or act 4 = swiglu_fwd of the
bf16-rounded gate / up projections.  exact(), bound() and ratio() are gemm_reference's (`_pipeline` on an operand set built here),
so the bf16-store term S, the act 4, RMS and residual terms are the ones every other GEMM path is held to:

    E0 = (c + 1) F S_ab,   S_ab = |alpha| sum_k |a||w|

c, the longest chain of dependent fp32 additions of the new kernel (`plan()`), from its K order (gemm_bf16.hip, "Weight-only MXFP4
GEMM"): a K-chunk is 128 elements = FOUR dependent 16x16x32 MFMAs (lane group g holds k = 128 c + 32 g .. + 31, MFMA j takes
elements 8 j .. 8 j + 7 of every group); wave w of 8 takes chunks w, w + 8, .. of its K-slice; the 8 partial tiles are summed in
wave order through LDS; ks > 1 K-slices are summed in slice order by the wide kernel's fix-up launch.  With nc = ceil(K / 128),
ntiles = ceil(N / 64) (act 4: ceil(N / 32)), ks = max(1, min(256 // ntiles, nc // 8, 8)), cps = ceil(nc / ks):

    both forms (M <= 16 and 17 <= M <= 64)     c = 4 ceil(cps / 8) + 32 + 7 + (ks - 1)

(+ 32 for the unknown order of the 32 products inside one MFMA, as in gemm_reference).  M enters neither ks nor c.

`emulate(o, mutation)` walks exactly that order in fp32 (products exact, one fp32 rounding per MFMA, per wave sum, per slice sum)
and rounds where the kernel rounds.  Mutations, the two errors a nibble-streaming kernel can make:
    scale_next_block     the scale of block i applied to block i + 1
    nibbles_swapped      the two codes of every byte exchanged
"""
import math

import torch

import gemm_reference as G
from gemm_reference import F, SENTINEL, rbf, r32, f32   # noqa: F401

GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MUTATIONS = ("scale_next_block", "nibbles_swapped")
RULES = ("le7", "ocp_floor", "le6")


# ---------------------------------------------------------------------------------------------------------------- quantiser
def block_exponent(amax, rule="le7"):
    """e per block from amax (float64, exact bf16 values) by integer arithmetic on frexp"""
    m, ex = torch.frexp(amax)
    ex = ex.to(torch.int32)
    if rule == "le7":                                      # amax 2^-e <= 7 = 0.875 2^3
        e = ex - 3 + (m > 0.875).to(torch.int32)
    elif rule == "ocp_floor":                              # amax 2^-e < 8: e = floor(log2 amax) - 2
        e = ex - 3
    elif rule == "le6":                                    # amax 2^-e <= 6 = 0.75 2^3: nothing saturates
        e = ex - 3 + (m > 0.75).to(torch.int32)
    else:
        raise KeyError(rule)
    return torch.where(amax == 0, torch.zeros_like(e), e)


def pow2(e):
    """2^e as float64 from its bits (exact on every device; torch.ldexp multiplies by a computed power)"""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def quantize_ref(w, rule="le7"):
    """w [rows, K] (bf16 or any float holding bf16 values), K % 32 == 0 -> (codes uint8 [rows, K], e int32 [rows, K / 32])"""
    rows, K = w.shape
    assert K % 32 == 0
    x = w.double().view(rows, K // 32, 32)
    e = block_exponent(x.abs().amax(dim=2), rule)
    y = x.abs() * pow2(-e)[:, :, None]                                       # exact: a power-of-two scaling
    mag = ((y > 0.25).to(torch.uint8) + (y >= 0.75).to(torch.uint8) + (y > 1.25).to(torch.uint8) + (y >= 1.75).to(torch.uint8) +
           (y > 2.5).to(torch.uint8) + (y >= 3.5).to(torch.uint8) + (y > 5.0).to(torch.uint8))
    sign = torch.signbit(x).to(torch.uint8) << 3
    return (mag | sign).view(rows, K), e


def code_values(codes):
    grid = torch.tensor(GRID, dtype=torch.float64, device=codes.device)
    v = grid[(codes & 7).long()]
    return torch.where((codes & 8) != 0, -v, v)


def dequant(codes, e):
    rows, K = codes.shape
    v = code_values(codes).view(rows, K // 32, 32)
    return (v * pow2(e)[:, :, None]).view(rows, K)


def dequant_bf16(codes, e):
    v = dequant(codes, e)
    b = v.to(torch.bfloat16)
    assert torch.equal(b.double(), v), "code * 2^e must be exactly a bf16 value"
    return b


def pack(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def unpack(q):
    rows, half = q.shape
    return torch.stack([q & 15, q >> 4], 2).reshape(rows, 2 * half)


def scale_bytes(e):
    b = e + 127
    assert int(b.min()) >= 0 and int(b.max()) <= 254
    return b.to(torch.uint8)


def rel_sq_error(w, rule):
    """sum (w - dequant)^2 / sum w^2 of one quantisation rule"""
    c, e = quantize_ref(w, rule)
    d = dequant(c, e) - w.double()
    return float((d * d).sum() / (w.double() ** 2).sum())


# ---------------------------------------------------------------------------------------------------------------- the GEMM
def plan(M, N, K, act):
    """host dispatch of desta_gemm_w4a16_nt restated: tiles, K-slices, chunks per slice, chain length"""
    ntiles = (N + 31) // 32 if act == 4 else (N + 63) // 64
    nc = (K + 127) // 128
    ks = max(1, min(256 // ntiles, nc // 8, 8))
    cps = (nc + ks - 1) // ks
    return dict(ntiles=ntiles, nc=nc, ks=ks, cps=cps, mf=(M + 15) // 16, c=4 * ((cps + 7) // 8) + 32 + 7 + (ks - 1))


def case(M, N, K, act=0, rms=False, res=False, out_f32=False, alpha=1.0):
    return dict(M=M, N=N, K=K, act=act, rms=rms, res=res, out_f32=out_f32, alpha=alpha)


def case_id(c):
    return (f"{c['M']}x{c['N']}x{c['K']}" + ("-act4" if c["act"] == 4 else "") + ("-rms" if c["rms"] else "") +
            ("-res" if c["res"] else "") + ("-f32" if c["out_f32"] else "") + (f"-a{c['alpha']}" if c["alpha"] != 1.0 else ""))


def operands(c, seed=0, device="cpu"):
    """Everything one call takes (random numbers drawn on the host, quantised and returned on `device`), in gemm_reference's operand-set form (so exact / bound / ratio apply), plus the packed weight:
    q [Nb, ldq] uint8 (ldq = K / 2 rounded up to 16, + 16: strided rows), s [Nb, lds] uint8 (lds = K / 32 + 3), both padded with 0xff.
    Weight rows span the magnitude bands 3e-4 / 0.02 / 1 and, for act 4, the up rows sit 4 x above their gate rows."""
    M, N, K, act = c["M"], c["N"], c["K"], c["act"]
    p = plan(M, N, K, act)
    g = torch.Generator().manual_seed(4000 + 1000 * seed + M * 7 + N * 3 + K + 11 * act)
    Nb = 2 * N if act == 4 else N
    ldc = N + 8
    ldr = (N + 7) // 8 * 8 + 8
    o = dict(M=M, N=N, K=K, batch=1, c=p["c"], out_f32=c["out_f32"], alpha=c["alpha"], act=act, rope=0, drop=0.0,
             Nc=N, ldc=ldc, ldp=N + 8, ldr=ldr, ld_aux=0, trans_a=False, trans_b=False, scale=None, bias=None, res=None, mask=None,
             rms_w=None, gu=None, cs=None, dyadic=None, ldp_on=False, plan=p)
    o["A_store"] = (torch.randn(1, M, 3, K, generator=g) * (3.0 if c["rms"] else 1.0)).to(torch.bfloat16)
    o["A_view"], o["lda"], o["sA"] = ((1, M, K), (M * 3 * K, 3 * K, 1), K), 3 * K, 0
    W = torch.randn(Nb, K, generator=g) * ((2.0 if act == 4 else 1.0) / math.sqrt(K))
    band = torch.tensor([1.0, 0.02 * math.sqrt(K) / 4, 3e-4 * math.sqrt(K) / 4])[torch.arange(Nb) % 3]
    W = W * band[:, None]
    if act == 4:
        W[N:] *= 4.0                                                      # up rows on other scales than their gate rows
    codes, e = quantize_ref(W.to(torch.bfloat16).to(device))
    o["codes"], o["e"] = codes, e
    o["B_store"] = dequant_bf16(codes, e).view(1, Nb, K)
    o["B_view"], o["ldb"], o["sB"] = ((1, Nb, K), (Nb * K, K, 1), 0), K, 0
    ldq, lds = (K // 2 + 15) // 16 * 16 + 16, K // 32 + 3
    q = torch.full((Nb, ldq), 0xff, dtype=torch.uint8, device=device)
    q[:, :K // 2] = pack(codes)
    s = torch.full((Nb, lds), 0xff, dtype=torch.uint8, device=device)
    s[:, :K // 32] = scale_bytes(e)
    o["q"], o["ldq"], o["s"], o["lds"] = q, ldq, s, lds
    if c["rms"]:
        o["rms_w"], o["rms_eps"] = 1.0 + 0.1 * torch.randn(K, generator=g), 1e-5
    if c["res"]:
        res = torch.zeros(1, M, ldr)
        res[:, :, :N] = torch.randn(1, M, N, generator=g)
        o["res"] = res.to(torch.bfloat16)
    return G.to_device(o, device)


exact, bound, ratio, to_device, kernel_arg = G.exact, G.bound, G.ratio, G.to_device, G.kernel_arg


def ordered_accumulate(A, W, p):
    """sum_k A[m,k] W[n,k] in the kernel's order, fp32: A [M, K], W [Nb, K] float64 holding bf16 values -> float64 [M, Nb]"""
    M, K = A.shape
    nc, ks, cps = p["nc"], p["ks"], p["cps"]
    pad = nc * 128 - K

    def chunks(x):                                         # [rows, nc, g, j, i]: k = 128 c + 32 g + 8 j + i
        x = torch.nn.functional.pad(x, (0, pad))
        return x.view(x.shape[0], nc, 4, 4, 8)

    a, w = chunks(A), chunks(W)
    # one MFMA = 32 exact products summed, rounded once to fp32 with the accumulator
    P = torch.einsum("mcgji,ncgji->mncj", a, w)            # float64: exact products, near-exact 32-term sum
    slices = []
    for s in range(ks):
        waves = []
        for wv in range(8):
            acc = torch.zeros(M, W.shape[0], dtype=torch.float64)
            for cc in range(s * cps + wv, min((s + 1) * cps, nc), 8):
                for j in range(4):
                    acc = r32(acc + P[:, :, cc, j])
            waves.append(acc)
        tot = waves[0]
        for wv in range(1, 8):
            tot = r32(tot + waves[wv])
        slices.append(tot)
    out = slices[0]
    for s in range(1, ks):
        out = r32(out + slices[s])
    return out


def emulate(o, mutation=None):
    """the whole C buffer a conforming kernel stores ([1, M + GUARD_ROWS, ldc], float64), optionally with a seeded error"""
    M, N, act, alpha = o["M"], o["N"], o["act"], f32(o["alpha"])
    A = G.logical(o, "A")
    if o["rms_w"] is not None:
        A = G._rms_rows(o, A, True)[0]
    codes, e = o["codes"], o["e"]
    if mutation == "scale_next_block":
        e = torch.roll(e, 1, dims=1)
    elif mutation == "nibbles_swapped":
        codes = torch.stack([codes[:, 1::2], codes[:, 0::2]], 2).reshape(codes.shape)
    elif mutation is not None:
        raise KeyError(mutation)
    v = r32(alpha * ordered_accumulate(A[0], dequant(codes, e), o["plan"]))[None]
    if act == 4:
        gt, up = rbf(v[:, :, :N]), rbf(v[:, :, N:])
        C = rbf(rbf(gt * torch.sigmoid(gt)) * up)
    else:
        if o["res"] is not None:
            v = v + o["res"].double()[:, :, :N]
        C = r32(v) if o["out_f32"] else rbf(v)
    return {"C": G._guarded(C, o["ldc"])}


# ---------------------------------------------------------------------------------------------------------------- planted blocks
TIES = ((0.25, 0.0), (0.75, 1.0), (1.25, 1.0), (1.75, 2.0), (2.5, 2.0), (3.5, 4.0), (5.0, 4.0))      # scaled element -> grid value


def planted_blocks():
    """32-blocks with hand-computed answers -> (w bf16 [n, 32], e int32 [n], checks): checks = [(block, element, grid value)],
    the value code_values() must give there (before the block scale).  Blocks, in order, for k in (-20, 0, 5):
        amax exactly 7 2^k (e = k; 7 itself becomes 6) | amax one bf16 step above it, 7.03125 2^k (e = k + 1; 3.515625 -> 4)
    then an all-zero block (e = 0, byte 127), a block whose maximum 6.5 sits in (6, 7] and saturates to 6 (e = 0), and a block with
    amax 6 (e = 0) carrying every tie of the rounding rule with both signs."""
    g = torch.Generator().manual_seed(77)
    rows, es, checks = [], [], []
    for k in (-20, 0, 5):
        for top, e, val in ((7.0, k, 6.0), (7.03125, k + 1, 4.0)):
            b = ((torch.rand(32, generator=g) * 2 - 1) * 3.0).to(torch.bfloat16).double()
            b[5] = -top
            rows.append(b * 2.0 ** k)
            es.append(e)
            checks.append((len(rows) - 1, 5, -val))
    rows.append(torch.zeros(32, dtype=torch.float64))
    es.append(0)
    checks.append((len(rows) - 1, 0, 0.0))
    b = ((torch.rand(32, generator=g) * 2 - 1) * 3.0).to(torch.bfloat16).double()
    b[31] = 6.5
    rows.append(b)
    es.append(0)
    checks.append((len(rows) - 1, 31, 6.0))
    b = torch.zeros(32, dtype=torch.float64)
    b[0] = 6.0
    for i, (x, val) in enumerate(TIES):
        b[1 + 2 * i], b[2 + 2 * i] = x, -x
        checks += [(len(rows), 1 + 2 * i, val), (len(rows), 2 + 2 * i, -val)]
    rows.append(b)
    es.append(0)
    w = torch.stack(rows).to(torch.bfloat16)
    assert torch.equal(w.double(), torch.stack(rows)), "planted values must be bf16 values"
    return w, torch.tensor(es, dtype=torch.int32), checks
