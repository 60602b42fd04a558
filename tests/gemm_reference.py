"""Float64 reference, per-element error bounds and a conforming emulation for every GEMM path and epilogue of
csrc/gemm_bf16.hip (desta_gemm_bf16_nt, desta_gemm_w8a16_nt, desta_gemm_wide_nt).  Plain torch, float64, device-agnostic;
imported by the host test (test_gemm_bound_host.py) and the GPU test (test_gpu_gemm_fp64.py), which share the case table
`CASES`, the operand generator `operands()`, the restated host dispatch `plan()` and the path selection `select()` below.
The notation (ulp, H, F, T, S) is that of rowwise_reference.py, whose SwiGLU reference this module reuses.

    exact(o, stored=None)      -> {"C" [, "preact", "aux"]: float64, "_": what bound() needs}
    bound(o, ref, name, out)   -> per-element bound of output `name` for the result `out` (float64)
    emulate(o, mutation=None)  -> the values a conforming kernel stores (float64), optionally with a seeded error

Every output is a WHOLE buffer: [batch, M + GUARD_ROWS, ld] with the sentinel 7.0 outside the [M, N] the kernel owns; the
reference holds the sentinel there and the bound is 0, so a store past row M or column N is an infinite ratio.

Operation (include/desta_hip.h, desta_gemm_desc).  v = alpha * sum_k A[m,k] B[n,k] on the bf16 values the kernel sees (A through
lda / stride_a / trans_a, lda < K = overlapping rows, a_rms_weight = RMSNorm of the rows first; B through ldb / stride_b /
trans_b, e4m3 bytes * row scale for the weight-only FP8 forms); v += bias[n]; rotary: adjacent pairs (2i, 2i+1) of every
rope_head_dim-wide head below rope_cols rotated by the fp32 table entry (pos[m], i), TAKEN AS GIVEN; preact = bf16(v);
v = GELU_erf(v) (act 1); v = mask ? v * fp32(1 / (1 - p)) : 0 with the mask an OPERAND (on the GPU: desta_dropout_mask at index
(z M + m) N + n, gemm_bf16.hip:110); v += residual[m,n] (bf16 or fp32, ldr, stride_r, 0 = shared); C = bf16(v) or fp32(v).
act 2: C = bf16(v) over the BLOCKED gate|up layout (64-column block b = gate 32b..32b+31 | up 32b..32b+31) and aux[M, N/2] =
swiglu_fwd of the STORED projection (so `exact(o, stored=C)` takes the kernel's own C; without it bf16(v)).  act 3: d =
bf16(v) [M, N] is d(act), aux [M, 2N] the saved blocked gate|up, C [M, 2N] = swiglu_bwd(d) blocked.  act 4: B = [2N, K] gate rows
then up rows, C = swiglu_fwd(bf16(v_gate), bf16(v_up)).  The SwiGLU operations are DEFINED with the rounding points of
rowwise_reference.py (projection / d(act) rounded to bf16, silu(gate) rounded before the product: gemm_bf16.hip:253-261,
:288-302, :1495-1496, :1572-1573).

Bounds.  bf16 store of a result: S(out, ref) = H(max(|out|, |ref|)) + T.  fp32 output: the fp32 terms alone.
  accumulation   E0 = (c + 1) F S_ab,  S_ab = |alpha| sum_k |a||b|;  c = the longest chain of dependent fp32 additions a partial
                 sum goes through, per path (`plan()["c"]`), + 1 for the product with alpha (:89, :169, :199):
                     tile kernels   2 ceil(nk / split) + 32 + (split - 1)     nk = K / 64; a K-tile is two dependent 16x16x32 MFMAs
                                    (:414-428, the 256x256 loops :764-771), i.e. K / 32 accumulations, + 32 for the unknown order
                                    of the 32 products inside one MFMA, + the slice sums of the fix-up (:1317-1320) or the
                                    in-kernel reduce (:1083-1086)
                     skinny         2 ceil(nk / 8) + 32 + 7                   a wave takes every 8th 64-chunk (:1413, :1443), the 8
                                    waves' tiles are summed in wave order through LDS (:1478-1480)
                     wide           2 ceil(cps / 8) + 32 + 7 + (ks - 1)       cps = ceil(nk / ks) chunks per K-slice (:1620, :2027),
                                    LDS combine (:1657-1661), slice sums of the fix-up (:1723-1724)
                 Nobody has measured the rounding inside the MFMA.  F assumes round-to-nearest per step; if the unit truncates, a
                 step errs by up to 2 F and the GPU criterion's factor 2 absorbs exactly that.
  a_rms_weight   The operation is DEFINED on A' = bf16(w bf16(x rstd)) (:1518-1526, the rounding points of rmsnorm_fwd).  The fp32
                 rstd and product carry r = (c_row / 2 + 5) F (rowwise_reference's r_rstd + 1): where t (1 - r) and t (1 + r)
                 round to different bf16 values the inner rounding moves by d1 = ulp(t), y = w bf16(t) by dy = |w| d1 + F |y|,
                 and where y - dy and y + dy round differently A' moves by e = dy + ulp(|y| + dy) (else 0):
                 E0 += |alpha| sum_k e_k |b_k|.
  bias (:92)     E += F |v|                      residual (:117, :121, :188)   E += F |v|
  rotary (:64-65)   y = a c - b s:  E_y = |c| E_a + |s| E_b + 3 F (|a c| + |b s|)
  preact (:98)   S + E at that point
  GELU, bf16 store (common.h:103-112, A&S 7.1.26): E_e = 1.5e-7 + erfc(z) (2 z^2 + 24) F, z = |x| / sqrt 2 (the formula's
                 absolute error; __expf(-z^2) moves erfc by (2 z^2 + 8) F relatively, rcpf by one ulp = 2 F through t and the
                 polynomial (<= 4 F), the five FMAs and two products 12 F);  E = 1.13 E + 0.5 |x| (E_e + 2 F) + 2 F |y|
                 (1.13 = sup |gelu'|; 1 - e CANCELS for x < 0, so its absolute error E_e + F is what 0.5 |x| multiplies)
  GELU, fp32 output (common.h:100, erff): E = 1.13 E + 0.5 |x| (8 F |erf| + 3 F) + 2 F |y|   (erff taken as 4 ulp, twice what
                 the CUDA / HIP tables state; the argument's rounding moves erf by <= F)
  dropout (:112) E = mask (scale E + F |v|)
  act 2          C: S + E0.  aux: rowwise_reference's swiglu_fwd bound on the stored projection.
  act 3 / act 4  rowwise_reference's swiglu_bwd / swiglu_fwd bound at the rounded d / (gate, up), + where v - E0 and v + E0 round
                 to different bf16 values the accumulation error moves the ROUNDED value by up to D(v) = E0 + ulp(|v| + E0)
                 (else 0): D(d) |d out / d d| for act 3; D(u) |silu(g)| + (|u| + D(u)) (1.1 D(g) + ulp(|silu g| + 1.1 D(g))) for
                 act 4 (1.1 = sup |silu'|; the inner rounding of silu can move by one more ulp).
For real operands at large K the accumulation term is looser than the old fp32 limit (K = 4096: about 2e-2 absolute against
atol 2e-3): the DYADIC cases carry the precision there.

`emulate()` rounds where the kernels round: the one bf16 / fp32 store, the pre-activation copy, the projection / d(act) /
silu(gate) in act 2 / 3 / 4, the normalised A of a_rms_weight.  Not emulated (the GPU test's factor 2): accumulation order,
fused multiply-adds, __expf / erff / rcpf / rsqrtf.

Operands (`operands(case)`, seeded).  `real`: randn, B / sqrt(K) as test_gemm_epilogues_and_batch / test_gemm_skinny scale it;
with a bf16 residual and a bf16 output, residual rows 0 and M - 1 are bf16(-0.97 bf16(value before the add)), so that the add
cancels.  `dyadic`: A = integers in [-a, a], B = integers in [-b, b] * 2^-s with K a b < 2^24 (2^21 where alpha = 0.75), bias /
residual integers * 2^-s: every partial sum in any order is exact in fp32, the accumulation term is zero, an fp32 output must
EQUAL float64 and a bf16 output RNE(float64), bit for bit.  (255, 255, 0) at K <= 256 exercises full 8-bit significands.

exact() and emulate() are ONE function (`_pipeline`) switched by a flag, as in the sibling reference modules: they share the
operand addressing, the rotary pair indexing and the blocked gate|up layout, so a structural error there is invisible to the host
test (which compares the two) and is caught only by the GPU run, where the kernel is the independent implementation.

Seeded mutations (`MUTATIONS`), the errors these kernels can actually make; `applies(mutation, case)` says where:
    double_rounding_residual   the value rounded to bf16 BEFORE the residual add (epilogue4 / epilogue_pair_bf16 with f2bf early)
    rope_double_rounding       the projection rounded before the rotation (what desta_hip.h promises does not happen)
    swiglu_unrounded_proj      act 2 / act 4 form the activation from the unrounded accumulator
    kslice_row_missing         in a split tile the last row of slice 1's partition (row 256 * 2 / split - 1) lacks the last slab
    group_tail_tile_swapped    two split tiles of a short last M-group written to each other's place (a fix-up kernel that does
                               not repeat the main kernel's L -> tile map)
    guard_row_written          row M of a ragged tile stored
"""
import math

import torch

import rowwise_reference as R
from rowwise_reference import F, T, SENTINEL, H, S, r32, f32, bf16_ulp, rbf, worst_ratio, rel_l2   # noqa: F401 (re-exported)

GUARD_ROWS = 3
WS_BYTES = (64 << 20) + 4096                   # desta._hip.GEMM_WS_BYTES: the workspace every binding call hands over
NCU = 256
GROUP_M = 8                                    # GEMM_GROUP_M
DEFAULT_OPTIONS = {0: 1, 2: 0, 3: 512, 5: 0, 6: 1, 10: 1}      # the options select() touches, at their defaults
MUTATIONS = ("double_rounding_residual", "rope_double_rounding", "swiglu_unrounded_proj", "kslice_row_missing",
             "group_tail_tile_swapped", "guard_row_written")
HOST_MAX_ELEMENTS = 1 << 21                    # the host test keeps the references of cases up to this many outputs

# ---------------------------------------------------------------------------------------------------------------- epilogues
# res: None / "bf16" / "f32"; ldr: 8 -> a multiple of 8 (the 16-byte swapped load), 4 -> 4 mod 8 (fallback); exact: a dyadic case
# of it must come out exact.
_E0 = dict(out_f32=False, alpha=1.0, bias=False, act=0, res=None, ldr=8, pre=False, drop=0.0, rope=0, batch=1, shared=False,
           rms=False, ldc_pad=8, exact=False)
EPI = {
    "plain": dict(exact=True),
    "f32": dict(out_f32=True, exact=True),
    "ldc12": dict(ldc_pad=12, exact=True),
    "alpha": dict(alpha=0.75, exact=True),
    "bias": dict(bias=True, exact=True),
    "bias_gelu": dict(bias=True, act=1),
    "bias_gelu_f32": dict(bias=True, act=1, out_f32=True),
    "res8": dict(res="bf16", exact=True),
    "res4": dict(res="bf16", ldr=4, exact=True),
    "res32": dict(res="f32", exact=True),
    "f32_stream": dict(bias=True, res="f32", out_f32=True, exact=True),
    "pre": dict(pre=True, exact=True),
    "bias_gelu_res": dict(bias=True, act=1, res="bf16"),
    "rich": dict(alpha=0.75, bias=True, act=1, res="bf16", pre=True),
    "drop": dict(bias=True, act=1, res="bf16", drop=0.1),
    "drop_b2": dict(bias=True, act=1, res="bf16", drop=0.1, batch=2),
    "rope64": dict(rope=64),
    "rope128": dict(rope=128),
    "act2": dict(act=2),
    "act3": dict(act=3),
    "act4": dict(act=4),
    "batch3": dict(bias=True, res="bf16", batch=3, shared=True, exact=True),
    "batch2": dict(bias=True, batch=2),
    "rms": dict(rms=True, res="bf16"),
    "rms_act4": dict(rms=True, act=4),
    "res_alpha": dict(res="bf16", alpha=0.5),
}


def epi(case):
    return {**_E0, **EPI[case["epi"]]}


# ---------------------------------------------------------------------------------------------------------------- case table
def _c(path, M, N, K, e, kind="real", **kw):
    c = dict(path=path, M=M, N=N, K=K, epi=e, kind=kind, variant=0, opts={}, ta=False, tb=False, entry="bf16", im2col=False)
    c.update(kw)
    return c


def _both(out, path, M, N, K, e, **kw):
    out.append(_c(path, M, N, K, e, "real", **kw))
    if EPI[e].get("exact"):
        out.append(_c(path, M, N, K, e, "dyadic", **kw))


TILE_EPIS = ("plain", "f32", "alpha", "bias", "bias_gelu", "bias_gelu_f32", "res8", "res4", "res32", "f32_stream", "pre", "rich",
             "drop", "drop_b2", "batch3", "ldc12")
ALL_EPIS = TILE_EPIS + ("rope64", "rope128", "act2", "act3")
# instances a path's argument checks (or its dispatch rule) do not admit, with the line of gemm_bf16.hip that says so; every other
# instance of ALL_EPIS is in the table on that path (test_gemm_bound_host.py::test_case_table_reaches_every_path)
INADMISSIBLE = {
    "db128": {}, "ring128": {}, "k256": {},
    "split": {"drop_b2": "K-slices need batch == 1 (:1821)", "batch3": "K-slices need batch == 1 (:1821)",
              "act2": "the SwiGLU epilogues take no K-slices (:1821)", "act3": "the SwiGLU epilogues take no K-slices (:1821)"},
    "persist": {"drop_b2": "can_persist needs batch == 1 (:1882): the call runs the one-tile-per-block kernel",
                "batch3": "can_persist needs batch == 1 (:1882): the call runs the one-tile-per-block kernel"},
    "skinny": {"rope64": "the rotary epilogue needs M > 16 (:1834)", "rope128": "the rotary epilogue needs M > 16 (:1834)",
               "act2": "act 2 at M <= 16 stays on the tile kernels (:1841)", "act3": "act 3 at M <= 16 stays on the tile kernels (:1841)"},
}


def _cases():
    out = []
    # 128x128 double-buffered (variant 1, option 6 = 0) and ring (option 6 = 2): every instance at the smallest ragged shape
    for path, ring, k0, ks in (("db128", 0, 192, (64, 128)), ("ring128", 2, 256, (320, 576))):
        sel = dict(variant=1, opts={6: ring})
        for e in TILE_EPIS:
            _both(out, path, 200, 136, k0, e, **sel)
        for hd in (64, 128):
            out.append(_c(path, 200, 160, k0, f"rope{hd}", **sel))                 # rope_cols = 128 < N, M ragged
        for M in (8, 200, 257):
            out.append(_c(path, M, 128, k0, "act2", **sel))
            out.append(_c(path, M, 64, k0, "act3", **sel))
        for K in ks:
            _both(out, path, 200, 136, K, "plain", **sel)
            out.append(_c(path, 200, 136, K, "rich", **sel))
        if not ring:
            _both(out, path, 77, 4, 64, "f32", **sel)
            out.append(_c(path, 77, 4, 64, "rich", **sel))
            _both(out, path, 64, 128, 192, "f32", im2col=True, **sel)              # lda = 128 < K: overlapping rows
    # transposed storage on both 128x128 kernels, lda = M + 8
    for ring, path in ((0, "db128"), (2, "ring128")):
        for ta, tb in ((True, False), (False, True), (True, True)):
            sel = dict(variant=1, opts={6: ring}, ta=ta, tb=tb)
            for M, N, K in ((200, 136, 320), (8, 8, 64)):
                if ring and K < 256:
                    continue                                                       # fewer than four K-tiles: the ring kernel is not taken
                out.append(_c(path, M, N, K, "bias_gelu_res", **sel))
                out.append(_c(path, M, N, K, "drop", **sel))
                out.append(_c(path, M, N, K, "f32", "dyadic", **sel))
    # 256x256, one tile per block: variants 2 / 3 / 6 / 7, K around the 7-half-tile prologue, a 1-row edge tile, N off / on the
    # wide-store path (260: N % 32 != 0; 288: a 32-column edge tile)
    for K in (64, 128, 192, 256, 512):
        for N in (260, 288):
            _both(out, "k256", 257, N, K, "plain", variant=6)
            out.append(_c("k256", 257, N, K, "rich", variant=6))
    for e in TILE_EPIS:
        if e not in ("plain", "rich"):
            _both(out, "k256", 257, 288, 256, e, variant=6)
    for e in ("bias_gelu", "res8", "pre", "drop"):
        out.append(_c("k256", 257, 260, 256, e, variant=6))
    for hd in (64, 128):
        out.append(_c("k256", 257, 288, 256, f"rope{hd}", variant=6))              # the wide-store MODE 4
    for M in (8, 200, 257):
        out.append(_c("k256", M, 320, 256, "act2", variant=6))
        out.append(_c("k256", M, 320, 256, "act3", variant=6))
    for v in (2, 3, 7):
        for K in (64, 128, 192, 256, 512):
            out.append(_c("k256", 257, 288, K, "plain", "dyadic", variant=v))
            out.append(_c("k256", 257, 288, K, "rich", variant=v))
    out.append(_c("k256", 257, 288, 512, "plain", "dyadic", variant=6, opts={10: 0}))
    out.append(_c("k256", 257, 288, 512, "rich", variant=6, opts={10: 0}))
    # split-K tail: fix-up launch, then the ticketed in-kernel reduce (option 5 = 1); split 2 3 4 5 7 8 (3, 5, 7: uneven row
    # partitions of the reduce); (2305, 520): 10 x 3 tiles, a last M-group of 2, every tile split
    for o5 in (0, 1):
        sel = dict(variant=6, opts={5: o5})
        for K in (2048, 3072, 4096, 5120, 7168, 8192):
            _both(out, "split", 257, 288, K, "plain", **sel)
            out.append(_c("split", 257, 288, K, "f32", "dyadic", **sel))
            out.append(_c("split", 257, 288, K, "rich", **sel))
        out.append(_c("split", 257, 288, 3072, "rope128", **sel))                  # epilogue4<true>: the rotary body outside the wide store
        for e in ALL_EPIS:                                                         # the fix-up's / the reduce's generic epilogue4<true>
            if e not in INADMISSIBLE["split"] and e not in ("plain", "rich"):
                _both(out, "split", 257, 288, 2048, e, **sel)
        _both(out, "split", 2305, 520, 2048, "plain", **sel)
        out.append(_c("split", 2305, 520, 2048, "f32", "dyadic", **sel))
        out.append(_c("split", 2305, 520, 2048, "rich", **sel))
    # persistent queue kernel (variant 8): 4 tiles (252 blocks draw an empty ticket), a split tail through the queues, 272 tiles
    for e in ALL_EPIS:
        if e not in INADMISSIBLE["persist"] and e not in ("act2", "act3"):
            _both(out, "persist", 257, 288, 512, e, variant=8)
    for M in (8, 200, 257):
        out.append(_c("persist", M, 320, 512, "act2", variant=8))
        out.append(_c("persist", M, 320, 512, "act3", variant=8))
    _both(out, "persist", 257, 288, 4096, "plain", variant=8)
    out.append(_c("persist", 257, 288, 4096, "f32", "dyadic", variant=8))
    out.append(_c("persist", 257, 288, 4096, "rich", variant=8))
    _both(out, "persist", 4352, 4096, 64, "plain", variant=8)
    out.append(_c("persist", 4352, 4096, 64, "rich", variant=8))
    # skinny, M <= 16: A rows strided by 3K; option 2 in {0, 164, 322, 641}; option 3 = 7
    shapes = ((16, 64), (100, 192), (36, 64 * 37), (1028, 2048))
    for i, M in enumerate((1, 3, 16)):
        for j, (N, K) in enumerate(shapes):
            o2 = (0, 164, 322, 641)[(i + j) % 4]
            out.append(_c("skinny", M, N, K, "plain", opts={2: o2}))
            out.append(_c("skinny", M, N, K, "f32", "dyadic", opts={2: o2}))
            out.append(_c("skinny", M, N, K, "rich", opts={2: (0, 164, 322, 641)[(i + j + 1) % 4]}))
    for o2 in (0, 322, 641):
        out.append(_c("skinny", 3, 100, 192, "plain", "dyadic", opts={2: o2}))
    for e in TILE_EPIS + ("batch2",):
        if e != "rich":
            _both(out, "skinny", 3, 100, 192, e, opts={2: 164} if e == "plain" else {})
    out.append(_c("skinny", 16, 1028, 2048, "rich", opts={3: 7}))
    out.append(_c("skinny", 16, 1028, 2048, "f32", "dyadic", opts={3: 7}))
    out.append(_c("skinny", 3, 104, 192, "act4"))
    out.append(_c("skinny", 16, 512, 256, "act4", opts={3: 7}))
    out.append(_c("skinny", 3, 100, 512, "rms"))
    out.append(_c("skinny", 5, 104, 1536, "rms"))
    out.append(_c("skinny", 5, 104, 1536, "rms_act4"))
    # weight-only FP8 skinny and the wide (17 <= M <= 64) kernels, from their own tests' shape lists; the reference takes the
    # dequantised weight
    out.append(_c("w8", 3, 100, 192, "f32", entry="w8"))
    out.append(_c("w8", 16, 1028, 2048, "res_alpha", entry="w8"))
    out.append(_c("w8", 3, 104, 192, "act4", entry="w8"))
    out.append(_c("wide", 33, 100, 192, "res8", entry="wide"))
    out.append(_c("wide", 64, 1028, 2048, "plain", "dyadic", entry="wide"))         # 17 tiles, 32 chunks: two K-slices + fix-up
    out.append(_c("wide", 48, 36, 64 * 37, "res4", entry="wide"))
    out.append(_c("wide", 17, 104, 192, "act4", entry="wide"))
    out.append(_c("wide", 40, 512, 2048, "act4", entry="wide"))                    # K-sliced act 4: slabs + SwiGLU fix-up
    out.append(_c("wide", 33, 100, 192, "plain", entry="wide8"))
    seen, uniq = set(), []
    for c in out:                                                            # (a cell two loops name is one case)
        if case_id(c) not in seen:
            seen.add(case_id(c))
            uniq.append(c)
    return uniq


def case_id(c):
    s = f"{c['path']}-{c['M']}x{c['N']}x{c['K']}-{c['epi']}-{c['kind']}"
    if c["variant"] not in (0, 1, 6, 8):
        s += f"-v{c['variant']}"
    for k, v in sorted(c["opts"].items()):
        if not (k == 6 and c["path"] in ("db128", "ring128")):
            s += f"-o{k}={v}"
    if c["ta"] or c["tb"]:
        s += "-t" + ("a" if c["ta"] else "") + ("b" if c["tb"] else "")
    if c["im2col"]:
        s += "-im2col"
    if c["entry"] == "wide8":
        s += "-e4m3"
    return s


CASES = _cases()


def select(case):
    """(desta_gemm_force_variant value, {option: value}) that puts the call on the case's path; restore DEFAULT_OPTIONS and
    variant 0 afterwards."""
    return case["variant"], dict(case["opts"])


def _ld(n, pad):
    return n + pad


def layout(case):
    """leading dimensions of the outputs: ldc = N + 8 (12 for `ldc12`, where only ldc % 4 == 0 holds), ldp = N + 8"""
    e = epi(case)
    N = case["N"]
    Nc = 2 * N if e["act"] == 3 else N
    ldr = (N + 7) // 8 * 8 + 8 + (4 if e["ldr"] == 4 else 0)
    return dict(Nc=Nc, ldc=_ld(Nc, e["ldc_pad"]), ldp=_ld(N, 8), ldr=ldr,
                ld_aux=(N // 2 + 8) if e["act"] == 2 else (2 * N + 8) if e["act"] == 3 else 0)


def plan(case):
    """The host dispatch of desta_gemm_bf16_nt (gemm_bf16.hip:1812-1935), desta_gemm_w8a16_nt (:1969-1972) and desta_gemm_wide_nt
    (:2016-2030) restated: kernel family (desta_gemm_last_kernel), kernel, ring, split count, persistent, wide-store, chain c."""
    e = epi(case)
    M, N, K, batch = case["M"], case["N"], case["K"], e["batch"]
    nk = K // 64
    opts = {**DEFAULT_OPTIONS, **case["opts"]}
    variant = case["variant"]
    p = dict(family=0, kernel="", ring=False, split=1, full=0, tilesM=0, tilesN=0, persistent=False, inkernel=False,
             wide_store=False, ks=1, uses_ws=False)
    if case["entry"] in ("wide", "wide8"):
        swiglu = e["act"] == 4
        ntiles = (N + 31) // 32 if swiglu else (N + 63) // 64
        ks = max(1, min(256 // ntiles, nk // 16, 8))
        cps = (nk + ks - 1) // ks
        p.update(family=3, kernel="wide", ks=ks, uses_ws=ks > 1, c=2 * ((cps + 7) // 8) + 32 + 7 + (ks - 1))
        return p
    act = e["act"]
    tM, tN = (M + 255) // 256, (N + 255) // 256
    Tt = tM * tN
    split, full = 1, Tt
    if batch == 1 and nk >= 8 and act not in (2, 3):                   # (the binding always hands a workspace over)
        rem = Tt % NCU
        if 0 < rem <= NCU // 2:
            sp = min(NCU // rem, 8, nk // 16)
            if sp >= 2 and rem * sp * 256 * 256 * 4 + 4096 <= WS_BYTES:
                split, full = sp, Tt - rem
    if case["entry"] == "w8" or act == 4 or (M <= 16 and variant == 0 and not case["ta"] and not case["tb"] and act not in (2, 3)):
        p.update(family=3, kernel="skinny", c=2 * ((nk + 7) // 8) + 32 + 7)
        return p
    big = False
    if M >= 128 and N >= 128 and K >= 512:
        rounds = full * batch / NCU + (1.0 / split if split > 1 else 0.0)
        ideal = Tt * batch / NCU
        big = ideal / (rounds if split > 1 else math.ceil(rounds)) >= 0.78
    if variant == 1:
        big = False
    if variant >= 2:
        big = True
    if case["ta"] or case["tb"]:
        big = False
    lay = layout(case)
    if big:
        items = full + (Tt - full) * split
        persistent = batch == 1 and (variant in (4, 8) or (variant == 0 and ((opts[0] == 1 and split == 1 and Tt > NCU) or
                                                                                (opts[0] == 2 and items > NCU))))
        pre_ok = not e["pre"] or (act == 0 and e["res"] is None and lay["ldp"] % 8 == 0)
        wide = not e["out_f32"] and pre_ok and act <= 1 and e["drop"] == 0 and N % 32 == 0 and lay["ldc"] % 8 == 0
        p.update(family=2, kernel="256p" if persistent else "256", split=split, full=full, tilesM=tM, tilesN=tN,
                 persistent=persistent, inkernel=split > 1 and bool(opts[5]) and not persistent, wide_store=wide,
                 uses_ws=split > 1, c=2 * ((nk + split - 1) // split) + 32 + (split - 1))
    else:
        tm, tn = (M + 127) // 128, (N + 127) // 128
        ring = nk >= 4 and (opts[6] == 2 or (opts[6] == 1 and tm * tn * batch <= NCU))
        p.update(family=1, kernel="ring128" if ring else "db128", ring=ring, tilesM=tm, tilesN=tn, full=tm * tn, c=2 * nk + 32)
    return p


def tile_of(p, L):
    """work item L of the 256x256 grid -> (tile row, tile column): the grouped map of gemm_bf16.hip:931-936, which the fix-up
    (:1308-1313) and the persistent kernel (:1215-1219) must repeat"""
    gspan = GROUP_M * p["tilesN"]
    first_m = (L // gspan) * GROUP_M
    gsz = min(p["tilesM"] - first_m, GROUP_M)
    return first_m + (L % gspan) % gsz, (L % gspan) // gsz


def reduce_rows(split):
    """rows of a split tile that slice s sums in the in-kernel reduce (:1078): [256 s / split, 256 (s + 1) / split)"""
    return [(256 * s // split, 256 * (s + 1) // split) for s in range(split)]


def applies(mut, case):
    e, p = epi(case), plan(case)
    if mut == "double_rounding_residual":
        return e["res"] == "bf16" and not e["out_f32"] and e["act"] <= 1 and case["kind"] == "real"
    if mut == "rope_double_rounding":
        return e["rope"] > 0
    if mut == "swiglu_unrounded_proj":
        return e["act"] in (2, 4)
    if mut == "kslice_row_missing":
        return p["split"] > 1 and case["kind"] == "real"
    if mut == "group_tail_tile_swapped":
        return p["split"] > 1 and p["tilesM"] % GROUP_M != 0 and p["tilesM"] > GROUP_M and p["tilesN"] >= 2
    if mut == "guard_row_written":
        return p["family"] in (1, 2) and case["M"] % (256 if p["family"] == 2 else 128) != 0
    raise KeyError(mut)


# ---------------------------------------------------------------------------------------------------------------- operands
def _bf(x):
    return x.to(torch.bfloat16)


def dyadic_params(case):
    """(a, b, s): A in [-a, a], B in [-b, b] 2^-s, K a b < 2^24 (2^21 with alpha = 0.75: two more bits and the epilogue's adds)"""
    K, e = case["K"], epi(case)
    budget = 2 ** 21 if e["alpha"] not in (1.0, 0.5) else 2 ** 24 - 2 ** 13
    ab = min(255, int(math.isqrt(budget // K)))
    while K * ab * ab >= budget:
        ab -= 1
    return ab, ab, (0 if K <= 256 else 4)


def quantize_rows(w):
    """desta_quantize_rows_e4m3 on the host (tests/test_gpu_fp8_decode.py quantize_ref): (e4m3 bytes as uint8, power-of-two scale)"""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    m, ex = torch.frexp(amax)
    ee = ex.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)
    ee = torch.where(amax == 0, torch.zeros_like(ee), ee)
    scale = torch.ldexp(torch.ones_like(amax), ee)
    return (wf / scale[:, None]).to(torch.float8_e4m3fn).view(torch.uint8), scale


def logical(o, key):
    """operand A or B as the kernel addresses it: float64 [batch or 1, rows, K]"""
    size, stride, off = o[key + "_view"]
    x = torch.as_strided(o[key + "_store"].reshape(-1), size, stride, off)
    if key == "B" and o.get("scale") is not None:
        x = x.view(torch.float8_e4m3fn).float() * o["scale"].view(1, -1, 1)
    return x.double()


def kernel_arg(o, key):
    """the 1-D slice of the operand's storage whose data pointer the kernel takes"""
    return o[key + "_store"].reshape(-1)[o[key + "_view"][2]:]


def to_device(o, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in o.items()}


def _blocked(gate, up):
    """[M, I] gate, up -> the blocked [M, 2I] layout (64-column block = 32 gate | 32 up)"""
    M, I = gate.shape
    return torch.stack([gate.reshape(M, I // 32, 32), up.reshape(M, I // 32, 32)], 2).reshape(M, 2 * I)


def _unblocked(x):
    M, W = x.shape
    v = x.reshape(M, W // 64, 2, 32)
    return v[:, :, 0].reshape(M, W // 2), v[:, :, 1].reshape(M, W // 2)


def dropout_seed(case):
    return (7 << 40) | (12345 + case["M"] + case["N"])


def operands(case, seed=0, mask=None):
    """Everything the call takes.  `mask` (uint8 [batch, M, N], 1 = keep) replaces the seeded Bernoulli mask: the GPU test passes
    desta_dropout_mask's."""
    e, lay, p = epi(case), layout(case), plan(case)
    M, N, K, batch = case["M"], case["N"], case["K"], e["batch"]
    twin = case_id({**case, "opts": {k: v for k, v in case["opts"].items() if k != 5}})     # option 5 twins share their operands
    g = torch.Generator().manual_seed(1000 * seed + sum(ord(ch) for ch in twin) + M * 7 + N * 3 + K)
    dy = case["kind"] == "dyadic"
    Nb = 2 * N if e["act"] == 4 else N
    o = dict(M=M, N=N, K=K, batch=batch, c=p["c"], **{k: e[k] for k in ("out_f32", "alpha", "act", "rope", "drop")}, **lay,
             trans_a=case["ta"], trans_b=case["tb"], scale=None, bias=None, res=None, mask=None, rms_w=None, gu=None, cs=None)
    a_b_s = dyadic_params(case) if dy else None
    o["dyadic"], o["ldp_on"], o["plan"] = a_b_s, e["pre"], p

    def rnd(*shape, scale=1.0, amp=None, shift=0):
        if dy:
            return torch.randint(-amp, amp + 1, shape, generator=g).float() * 2.0 ** -shift
        return torch.randn(*shape, generator=g) * scale

    # ---- A
    if case["ta"]:
        o["A_store"] = _bf(rnd(K, M + 8, amp=a_b_s and a_b_s[0]))
        o["A_view"], o["lda"], o["sA"] = ((1, M, K), (0, 1, M + 8), 0), M + 8, 0
    elif case["im2col"]:
        lda = 128
        o["A_store"] = _bf(rnd((M - 1) * lda + K, amp=a_b_s and a_b_s[0]))
        o["A_view"], o["lda"], o["sA"] = ((1, M, K), (0, lda, 1), 0), lda, 0
    elif p["family"] == 3:
        o["A_store"] = _bf(rnd(batch, M, 3, K, scale=3.0 if e["rms"] else 1.0, amp=a_b_s and a_b_s[0]))
        o["A_view"], o["lda"], o["sA"] = ((batch, M, K), (M * 3 * K, 3 * K, 1), K), 3 * K, M * 3 * K
    else:
        o["A_store"] = _bf(rnd(batch, M, K, amp=a_b_s and a_b_s[0]))
        o["A_view"], o["lda"], o["sA"] = ((batch, M, K), (M * K, K, 1), 0), K, M * K
    # ---- B
    nbb = 1 if (e["shared"] or batch == 1) else batch
    bscale = (2.0 if e["act"] in (2, 4) else 1.0) / math.sqrt(K)
    if e["act"] == 3:
        bscale = 1.0 / math.sqrt(K)
    if case["tb"]:
        o["B_store"] = _bf(rnd(K, N, scale=bscale, amp=a_b_s and a_b_s[1], shift=a_b_s[2] if dy else 0))
        o["B_view"], o["ldb"], o["sB"] = ((1, N, K), (0, 1, N), 0), N, 0
    else:
        W = _bf(rnd(nbb, Nb, K, scale=bscale, amp=a_b_s and a_b_s[1], shift=a_b_s[2] if dy else 0))
        if case["entry"] in ("w8", "wide8"):
            W[0, Nb // 2:] *= 4.0                                        # rows on another scale
            q, sc = quantize_rows(W[0])
            o["B_store"], o["scale"] = q.view(1, Nb, K), sc
        else:
            o["B_store"] = W
        o["B_view"], o["ldb"], o["sB"] = ((nbb, Nb, K), (Nb * K, K, 1), 0), K, (Nb * K if nbb > 1 else 0)
    sh = a_b_s[2] if dy else 0
    if e["bias"]:
        o["bias"] = rnd(N, amp=1000, shift=sh)
    if e["rms"]:
        o["rms_w"], o["rms_eps"] = 1.0 + 0.1 * torch.randn(K, generator=g), 1e-5
    if e["rope"]:
        hd, P = e["rope"], 64
        fr = torch.outer(torch.arange(P, dtype=torch.float32), 1.0 / (10000 ** (torch.arange(0, hd, 2).float() / hd)))
        o["cs"] = torch.stack([fr.cos(), fr.sin()], 2).contiguous()                 # [P, hd / 2, 2]
        o["pos"] = torch.randint(0, P, (M,), generator=g, dtype=torch.int32)        # non-monotonic
        o["rope_cols"] = max(hd, (N - 1) // hd * hd)                                # < N: the rest stays unrotated
    if e["drop"]:
        o["seed"] = dropout_seed(case)
        o["mask"] = (torch.rand(batch, M, N, generator=g) >= e["drop"]).to(torch.uint8) if mask is None else mask.view(batch, M, N)
        one = torch.tensor(1.0, dtype=torch.float32)
        o["drop_scale"] = float(one / (one - torch.tensor(e["drop"], dtype=torch.float32)))   # 1.0f / (1.0f - p), :1804
    if e["act"] == 3:
        o["gu"] = _bf(torch.randn(M, 2 * N, generator=g) * 1.5)
        gu = torch.full((M, lay["ld_aux"]), SENTINEL, dtype=torch.bfloat16)
        gu[:, :2 * N] = o["gu"]
        o["gu_store"] = gu
    if e["res"]:
        rb = 1 if (e["shared"] or batch == 1) else batch
        o["sR"] = M * lay["ldr"] if rb > 1 else 0
        res = torch.zeros(rb, M, lay["ldr"])
        res[:, :, :N] = rnd(rb, M, N, amp=255 if e["res"] == "bf16" else 1000, shift=(sh - 2) if e["res"] == "bf16" and dy else sh)
        o["res"] = _bf(res) if e["res"] == "bf16" else res
        if not dy and e["res"] == "bf16" and not e["out_f32"] and e["act"] <= 1:
            o["res"] = None
            before = _pipeline(o, False, None, stop_before_residual=True)[0]        # float64 [batch, M, N]
            for row in {0, M - 1}:
                res[0, row, :N] = rbf(-0.97 * rbf(before[0, row]))
            o["res"] = _bf(res)
    return o


# ---------------------------------------------------------------------------------------------------------------- the operation
def _gelu(x):
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def _rms_rows(o, A, emu):
    """RMSNorm of the rows of A (a_rms_weight) with its two roundings, bf16(w bf16(x rstd)): emu -> with rstd rounded to fp32;
    else (the same from the float64 rstd, the amount e by which the fp32 error of rstd can move an element)"""
    w = o["rms_w"].double().view(1, 1, -1)
    rstd = torch.rsqrt((A * A).mean(-1, keepdim=True) + f32(o["rms_eps"]))
    if emu:
        return rbf(w * rbf(A * r32(rstd))), None
    cr = R.c_row(o["K"])
    rr = (cr / 2 + 5) * F                                                # rstd (rowwise_reference's r_rstd) and the product x rstd
    t = A * rstd
    d1 = (rbf(t * (1 + rr)) != rbf(t * (1 - rr))).double() * bf16_ulp(t.abs() * (1 + rr))
    y = w * rbf(t)
    dy = w.abs() * d1 + F * y.abs()
    flip = (rbf(y + dy) != rbf(y - dy)).double()
    return rbf(y), flip * (dy + bf16_ulp(y.abs() + dy))


def _pipeline(o, emu, mutation, stop_before_residual=False, stored=None):
    """exact (emu = False: float64 throughout, with the error terms E) or emulated (emu = True: roundings, mutations) operation on
    the valid region -> (C [batch, M, Nc], preact or None, aux or None, extras dict name -> error terms beyond the store)"""
    M, N, K, batch, act, alpha = o["M"], o["N"], o["K"], o["batch"], o["act"], f32(o["alpha"])
    A, B = logical(o, "A"), logical(o, "B")
    eA = None
    if o["rms_w"] is not None:
        A, eA = _rms_rows(o, A, emu)
    Bt = B.transpose(1, 2)
    v = alpha * (A @ Bt)                                                 # [batch, M, Nb]
    E = None
    if not emu:
        E = (o["c"] + 1) * F * abs(alpha) * (A.abs() @ Bt.abs())
        if eA is not None:
            E = E + abs(alpha) * (eA @ Bt.abs())
    if emu and mutation == "kslice_row_missing":
        sp = o["plan"]["split"]
        row, k0 = 256 * 2 // sp - 1, (K // 64) * (sp - 1) // sp * 64
        v[0, row, :256] -= alpha * (A[0, row, k0:] @ Bt[0, k0:, :256])
    extras, pre, aux = {}, None, None
    if act >= 2:
        if act == 2:
            C = rbf(v) if emu else v
            extras["C"] = E
            P = C if emu else (rbf(v) if stored is None else stored)
            gt, up = _unblocked(P[0])
            if emu:
                if mutation == "swiglu_unrounded_proj":
                    gt, up = _unblocked(v[0])
                aux = rbf(rbf(gt * torch.sigmoid(gt)) * up)[None]
            else:
                r = R._swf_exact({"gu": torch.cat([gt, up], 1), "I": N // 2})
                aux, extras["aux"] = r["act"][None], r["aux"]["extra"][None]
            return C, None, aux, extras
        if act == 3:
            gt, up = _unblocked(o["gu"].double())
            d = rbf(v[0])
            r = R._swb_exact({"gu": torch.cat([gt, up], 1), "I": N, "dact": d})
            dg, du = r["dgu"][:, :N], r["dgu"][:, N:]
            if emu:
                return rbf(_blocked(dg, du))[None], None, None, {}
            xg, xu = r["aux"]["extra"][:, :N], r["aux"]["extra"][:, N:]
            sig = torch.sigmoid(gt)
            flip = (rbf(v[0] + E[0]) != rbf(v[0] - E[0])).double() * (E[0] + bf16_ulp(v[0].abs() + E[0]))
            xg = xg + flip * (up * sig * (1 + gt * (1 - sig))).abs()
            xu = xu + flip * (gt * sig).abs()
            return _blocked(dg, du)[None], None, None, {"C": _blocked(xg, xu)[None]}
        # act 4: gate rows then up rows
        vg, vu = v[:, :, :N], v[:, :, N:]
        if emu:
            gt, up = (vg, vu) if mutation == "swiglu_unrounded_proj" else (rbf(vg), rbf(vu))
            return rbf(rbf(gt * torch.sigmoid(gt)) * up), None, None, {}
        gt, up = rbf(vg), rbf(vu)
        r = R._swf_exact({"gu": torch.cat([gt[0], up[0]], 1), "I": N})
        sg = gt * torch.sigmoid(gt)
        Eg, Eu = E[:, :, :N], E[:, :, N:]
        fg = (rbf(vg + Eg) != rbf(vg - Eg)).double()
        fu = (rbf(vu + Eu) != rbf(vu - Eu)).double()
        dU, dG = fu * (Eu + bf16_ulp(vu.abs() + Eu)), fg * (Eg + bf16_ulp(vg.abs() + Eg))
        x = r["aux"]["extra"][None] + dU * rbf(sg).abs() + (up.abs() + dU) * (1.1 * dG + fg * bf16_ulp(sg.abs() + 1.1 * dG))
        return r["act"][None], None, None, {"C": x}
    if o["bias"] is not None:
        v = v + o["bias"].double().view(1, 1, -1)
        if not emu:
            E = E + F * v.abs()
    if o["rope"]:
        hd, rc = o["rope"], o["rope_cols"]
        if emu and mutation == "rope_double_rounding":
            v = rbf(v)
        cs = o["cs"].double()[o["pos"].long()]                           # [M, hd / 2, 2]
        c = cs[:, :, 0].repeat(1, rc // hd).view(1, M, rc // 2)
        s = cs[:, :, 1].repeat(1, rc // hd).view(1, M, rc // 2)
        a, b = v[:, :, 0:rc:2], v[:, :, 1:rc:2]
        y = v.clone()
        y[:, :, 0:rc:2], y[:, :, 1:rc:2] = a * c - b * s, b * c + a * s
        if not emu:
            Ea, Eb = E[:, :, 0:rc:2], E[:, :, 1:rc:2]
            E2 = E.clone()
            E2[:, :, 0:rc:2] = c.abs() * Ea + s.abs() * Eb + 3 * F * ((a * c).abs() + (b * s).abs())
            E2[:, :, 1:rc:2] = c.abs() * Eb + s.abs() * Ea + 3 * F * ((b * c).abs() + (a * s).abs())
            E = E2
        v = y
    if o["ldp_on"]:
        pre = rbf(v) if emu else v
        if not emu:
            extras["preact"] = E
    if act == 1:
        x = v
        v = _gelu(x)
        if not emu:
            if o["out_f32"]:
                E = 1.13 * E + 0.5 * x.abs() * (8 * F * torch.erf(x / math.sqrt(2.0)).abs() + 3 * F) + 2 * F * v.abs()
            else:
                z = x.abs() / math.sqrt(2.0)
                Ee = 1.5e-7 + torch.special.erfc(z) * (2 * z * z + 24) * F
                E = 1.13 * E + 0.5 * x.abs() * (Ee + 2 * F) + 2 * F * v.abs()
    if o["mask"] is not None:
        keep = o["mask"].double()
        v = keep * v * o["drop_scale"]
        if not emu:
            E = keep * (o["drop_scale"] * E + F * v.abs())
    if stop_before_residual:
        return v, None, None, {}
    if o["res"] is not None:
        if emu and mutation == "double_rounding_residual":
            v = rbf(v)
        v = v + o["res"].double()[:, :, :N]
        if not emu:
            E = E + F * v.abs()
    if emu:
        v = r32(v) if o["out_f32"] else rbf(v)
        if mutation == "group_tail_tile_swapped":
            p = o["plan"]
            r0 = (p["tilesM"] // GROUP_M) * GROUP_M * 256                # first tile row of the short last group
            t = v[0, r0:r0 + 256, 0:256].clone()
            v[0, r0:r0 + 256, 0:256] = v[0, r0:r0 + 256, 256:512]
            v[0, r0:r0 + 256, 256:512] = t
    extras["C"] = E
    return v, pre, None, extras


def _guarded(x, ld, fill=SENTINEL):
    """valid [batch, M, n] -> whole buffer [batch, M + GUARD_ROWS, ld]"""
    b, M, n = x.shape
    full = torch.full((b, M + GUARD_ROWS, ld), fill, dtype=torch.float64, device=x.device)
    full[:, :M, :n] = x
    return full


def _lds(o):
    return {"C": o["ldc"], "preact": o["ldp"], "aux": o["ld_aux"]}


def exact(o, stored=None):
    """float64 result of every output as whole guarded buffers, and under "_" the error terms beyond the store (0 outside the
    valid region) and S_ab through them.  act 2: `stored` = the kernel's own C buffer (the activation is defined on it)."""
    if stored is not None:
        stored = stored.double()[:, :o["M"], :o["N"]]
    C, pre, aux, extras = _pipeline(o, False, None, stored=stored)
    ref, lds = {"_": {}}, _lds(o)
    for name, x in (("C", C), ("preact", pre), ("aux", aux)):
        if x is not None:
            ref[name] = _guarded(x, lds[name])
            ref["_"][name] = _guarded(extras[name], lds[name], fill=0.0)
            ref["_"][name + "_valid"] = _guarded(torch.ones_like(x), lds[name], fill=0.0) > 0
    return ref


def is_f32(o, name):
    return name == "C" and o["out_f32"]


def bound(o, ref, name, out):
    """per-element bound of output `name` (whole buffer); 0 outside the region the kernel owns"""
    out = out.double()
    b = ref["_"][name] if is_f32(o, name) else S(out, ref[name]) + ref["_"][name]
    return torch.where(ref["_"][name + "_valid"], b, torch.zeros_like(b))


def ratio(o, ref, name, out):
    out = out.double()
    return worst_ratio((out - ref[name]).abs(), bound(o, ref, name, out))


def emulate(o, mutation=None):
    C, pre, aux, _ = _pipeline(o, True, mutation)
    lds, res = _lds(o), {}
    for name, x in (("C", C), ("preact", pre), ("aux", aux)):
        if x is not None:
            res[name] = _guarded(x, lds[name])
    if mutation == "guard_row_written":
        res["C"][:, o["M"], :C.shape[2]] = res["C"][:, o["M"] - 1, :C.shape[2]]
    return res


def outputs(o):
    return ("C",) + (("preact",) if o["ldp_on"] else ()) + (("aux",) if o["act"] == 2 else ())


# the whole-tensor criteria of tests/test_gpu_kernels.py that the per-element bound is compared with
def old_plain_bf16(out, ref, K):
    return bool(((out - ref).abs() <= 1e-2 * math.sqrt(K) + 1e-2 * ref.abs()).all())


def old_epilogue_bf16(out, ref):
    return bool(((out - ref).abs() <= 2e-2 + 2e-2 * ref.abs()).all())


def old_rope(out, ref):
    return rel_l2(out, ref) < 6e-3
