"""The dropout mask, restated independently of the kernels, and the constructions that read a kernel's mask back out of it.
Plain numpy / torch integers and float64 on the CPU (the readouts run on whatever device their operands live on); imported by
the host test (test_dropout_mask_host.py) and the GPU test (test_gpu_dropout_mask.py), which run the SAME readout code.

The contract restated (csrc/common.h):
    rng32(seed, idx)        desta_rng32 with seed_lo = seed & 0xffffffff, seed_hi = seed >> 32, idx a 64-bit counter
    drop_thresh(p)          desta_drop_thresh: p is the fp32 value the C ABI receives, thresh = int(p * 65536 + 0.5) clamped to
                            [1, 0xffff]
    drop_scale(p)           the fp32 1.0f / (1.0f - p) every host entry point hands its kernel, as a Python float
    bits16(seed, idx)       desta_keep's 16 bits of element idx: ONE hash per element pair (idx >> 1); the even element takes the
                            low 16 bits, the odd one the high 16
    keep(seed, n, p)        bits16 >= thresh for elements [0, n)                                      (dropout_mask_k, dropout_bf16_k)
    attn_keep(...)          [B, Hq, Sq, Sk], element index ((b Hq + h) Sq + q) Sk + k                 (attention.hip, all DROP kernels)
    gemm_keep(...)          [batch, M, N], element index (z M + m) N + n                              (gemm_bf16.hip epilogue4)

The readout.  Head dim 64 and ZERO scores (Q = 0 or K = 0), so P is uniform, 1 / n with n = Sk, and no rounding can blur the
answer; c = drop_scale.  One pass t handles 64 keys or 64 queries; operands [B, S, H, 64] as in tests/attention_reference.py:
    fwd   Q = 0, V[k, d] = [k == 64 t + d]                       O[q, d]  = c keep[q, 64 t + d] / n     != 0 iff kept
    dV    Q = 0, dO[q, d] = [q == 64 t + d]                      dV[k, d] = c keep[64 t + d, k] / n     != 0 iff kept
    dQ    Q = 0, V[k, 0] = dO[q, 0] = 1, K[k, d] = [k == 64 t + d]
                                                                 dQ[q, d] = scale (c keep[q, 64 t + d] - delta[q]) / n
    dK    K = 0, V and dO as for dQ, Q[q, d] = [q == 64 t + d]   dK[k, d] = scale (c keep[64 t + d, k] - delta[64 t + d]) / n
with cnt[q] the kept keys of row q and delta[q] = c cnt[q] / n (dP = 1 everywhere, delta = O[q, 0]).  The fwd and dV values that
are not zero must lie within 2^-7 relative of c / n (one bf16 rounding of P, one of the store).  dQ and dK are compared with the
float64 formula on the reference mask, |out - formula| <= gap / 64 with gap = scale c / n the distance between the kept and the
dropped class: the roundings in play are O to bf16 inside delta, dS to bf16 for the MFMA and the bf16 store, each 2^-9 relative
of a term no larger than the gap, so 2^-6 of the gap is several times their sum (a derived margin, not a measured one).  Values
rather than signs keep a row with nothing dropped well defined (delta = c there: the kept class sits at 0; frequent at Sk = 2).
The mask is then decoded as dQ n / scale + delta_ref > c / 2 and must equal the reference everywhere.
dV / dK sum over the query heads of a GQA group: under a group of G heads the dV and dK readouts take G passes per t, pass g
with the one-hot operand (dO or Q) set only in the heads h = hk G + g, so that dV[k, hk] / dK[k, hk] carry head hk G + g alone.

`attention()` is the plain float64 dropout attention the host test proves the readouts on: it takes one mask per kernel family
({"fwd", "dq", "dkdv"}: O, dQ, dK | dV), the normaliser keeps the full sum, delta comes from the forward's O.  `planted_keeps()`
builds those masks, optionally with one of `MUTATIONS`, each a way these kernels can actually get the mask wrong:
    pair_halves_swapped      the even element takes the HIGH 16 bits                                          every kernel
    thresh_strict            kept iff bits > thresh                                                           every kernel
    head_uses_hkv            the row base uses b Hkv + h (changes nothing without a GQA group)                every kernel
    row_unclamped_tail       the last key pair of a partial 64-key tile takes the next row's first pair       forward only
    bwd_rows_8_15_from_0_7   query rows 8..15 of each 16-row slice reuse rows 0..7: the DPP swap gone wrong   dK | dV only
"""
import numpy as np
import torch

M32 = 0xFFFFFFFF
MUTATIONS = ("pair_halves_swapped", "thresh_strict", "head_uses_hkv", "row_unclamped_tail", "bwd_rows_8_15_from_0_7")
KINDS = ("fwd", "dV", "dQ", "dK")
D = 64


# ------------------------------------------------------------------------------------------------------------- the mask
def rng32(seed, idx):
    """desta_rng32 -> uint64 array holding 32-bit values; idx: array of 64-bit counters."""
    seed_lo, seed_hi = int(seed) & M32, (int(seed) >> 32) & M32
    key = np.uint64(((seed_lo ^ ((seed_hi * 0x632BE5AB) & M32)) * 0xC2B2AE35) & M32)
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    m = np.uint64(M32)
    with np.errstate(over="ignore"):
        hi = ((idx >> np.uint64(32)) + np.uint64(seed_hi)) & m
        x = ((idx & m) + np.uint64((seed_lo * 0x9E3779B9) & M32) + ((hi * np.uint64(0x85EBCA6B)) & m)) & m
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7FEB352D)) & m
        x ^= (x >> np.uint64(15)) ^ key
        x = (x * np.uint64(0x846CA68B)) & m
        x ^= x >> np.uint64(16)
    return x


def drop_thresh(p):
    t = float(np.float32(p)) * 65536.0 + 0.5
    return 0xFFFF if t >= 65535.0 else (1 if t < 1.0 else int(t))


def drop_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def bits16(seed, idx, swapped=False):
    idx = np.atleast_1d(np.asarray(idx, dtype=np.uint64))
    h = rng32(seed, idx >> np.uint64(1))
    odd = (idx & np.uint64(1)).astype(bool)
    return np.where(odd != swapped, h >> np.uint64(16), h & np.uint64(0xFFFF))


def keep(seed, n, p):
    return bits16(seed, np.arange(n, dtype=np.uint64)) >= np.uint64(drop_thresh(p))


def attn_keep(seed, B, Hq, Sq, Sk, p):
    return keep(seed, B * Hq * Sq * Sk, p).reshape(B, Hq, Sq, Sk)


def gemm_keep(seed, batch, M, N, p):
    return keep(seed, batch * M * N, p).reshape(batch, M, N)


def seed_with_boundary(n, p, first_seed):
    """The first seed >= first_seed for which some element of [0, n) has bits == thresh (the element `>` and `>=` disagree on)
    -> (seed, index of the first such element)."""
    t = np.uint64(drop_thresh(p))
    idx = np.arange(n, dtype=np.uint64)
    for seed in range(first_seed, first_seed + 100000):
        hit = np.flatnonzero(bits16(seed, idx) == t)
        if hit.size:
            return seed, int(hit[0])
    raise AssertionError("no seed with an element on the threshold")


def planted_keeps(seed, B, Hq, Hkv, Sq, Sk, p, mutation=None):
    """{"fwd", "dq", "dkdv"}: the mask of each kernel family as bool [B, Hq, Sq, Sk], with `mutation` planted."""
    assert mutation is None or mutation in MUTATIONS
    b, h, q, k = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(Hq, dtype=np.uint64), np.arange(Sq, dtype=np.uint64),
                             np.arange(Sk, dtype=np.uint64), indexing="ij", sparse=True)
    heads = Hkv if mutation == "head_uses_hkv" else Hq
    idx = ((b * np.uint64(heads) + h) * np.uint64(Sq) + q) * np.uint64(Sk) + k
    bits = bits16(seed, idx.reshape(-1), swapped=mutation == "pair_halves_swapped").reshape(B, Hq, Sq, Sk)
    t = np.uint64(drop_thresh(p))
    m = bits > t if mutation == "thresh_strict" else bits >= t
    out = {"fwd": m, "dq": m.copy(), "dkdv": m.copy()}
    if mutation == "row_unclamped_tail" and Sk % 64:
        tail = bits16(seed, (idx[..., Sk - 2:] + np.uint64(2)).reshape(-1)).reshape(B, Hq, Sq, 2)
        out["fwd"] = m.copy()
        out["fwd"][..., Sk - 2:] = tail >= t
    if mutation == "bwd_rows_8_15_from_0_7":
        rows = np.arange(Sq)
        out["dkdv"] = m[:, :, np.where(rows % 16 >= 8, rows - 8, rows)]
    return {n: torch.from_numpy(np.ascontiguousarray(x)) for n, x in out.items()}


# ------------------------------------------------------------------------------------------- plain fp64 dropout attention
def attention(q, k, v, do, scale, keeps, c):
    """q, dO [B, Sq, Hq, D], k, v [B, Sk, Hkv, D] -> {"O", "dQ", "dK", "dV"} float64 in the operands' layout.  `keeps`: one bool
    [B, Hq, Sq, Sk] for every kernel family, or the dict of planted_keeps()."""
    if not isinstance(keeps, dict):
        keeps = {"fwd": keeps, "dq": keeps, "dkdv": keeps}
    Hq, Hkv = q.shape[2], k.shape[2]
    G = Hq // Hkv
    hf = lambda x, rep=1: x.double().permute(0, 2, 1, 3).repeat_interleave(rep, dim=1)                     # noqa: E731
    rl = lambda x: x.permute(0, 2, 1, 3).contiguous()                                                       # noqa: E731
    gs = lambda x: x.view(x.shape[0], Hkv, G, x.shape[2], x.shape[3]).sum(2)                                # noqa: E731
    qh, gh, kh, vh = hf(q), hf(do), hf(k, G), hf(v, G)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    m = {n: x.to(p.device).double() * c for n, x in keeps.items()}
    O = (p * m["fwd"]) @ vh
    dP = gh @ vh.transpose(-1, -2)
    delta = (gh * O).sum(-1, keepdim=True)
    dS_q = p * (m["dq"] * dP - delta) * scale
    dS_k = p * (m["dkdv"] * dP - delta) * scale
    return {"O": rl(O), "dQ": rl(dS_q @ kh), "dK": rl(gs(dS_k.transpose(-1, -2) @ qh)), "dV": rl(gs((p * m["dkdv"]).transpose(-1, -2) @ gh))}


# ----------------------------------------------------------------------------------------------------------- the readouts
def passes(kind, Sq, Sk):
    return ((Sk if kind in ("fwd", "dQ") else Sq) + 63) // 64


def readout_operands(kind, t, B, Hq, Hkv, Sq, Sk, device="cpu", dtype=torch.float64, g=0):
    """(q, k, v, do) of pass t of readout `kind` (module docstring); g: the head of each GQA group that dV / dK read."""
    q, do = (torch.zeros(B, Sq, Hq, D, dtype=dtype, device=device) for _ in range(2))
    k, v = (torch.zeros(B, Sk, Hkv, D, dtype=dtype, device=device) for _ in range(2))
    target, S = {"fwd": (v, Sk), "dV": (do, Sq), "dQ": (k, Sk), "dK": (q, Sq)}[kind]
    d = torch.arange(min(D, S - 64 * t), device=device)
    if kind in ("dV", "dK") and Hq != Hkv:
        target[:, 64 * t + d, g::Hq // Hkv, d] = 1
    else:
        target[:, 64 * t + d, :, d] = 1
    if kind in ("dQ", "dK"):
        v[..., 0] = 1
        do[..., 0] = 1
    return q, k, v, do


def decode(kind, t, out, ref_keep, p, scale, g=0):
    """One pass of a readout.  out: the kernel's O (fwd), dV, dQ or dK, [B, S, H, 64]; ref_keep: bool [B, Hq, Sq, Sk] on out's
    device -> (slice of the mask this pass covers, the decoded bool tensor of that slice's shape, worst value error in units of
    the tolerance; inf where a value that must be exactly 0 is not)."""
    B, H, Sq, Sk = ref_keep.shape
    heads = slice(None) if out.shape[2] == H else slice(g, None, H // out.shape[2])       # dV / dK under GQA: head hk G + g
    c, n = drop_scale(p), Sk
    S = Sk if kind in ("fwd", "dQ") else Sq
    w = min(D, S - 64 * t)
    x = out.double().permute(0, 2, 1, 3)                                   # [B, H, S, 64]
    dead = x[..., w:]
    bad = float("inf") if bool((dead != 0).any()) else 0.0                 # columns past the last key / query of the pass: exactly 0
    x = x[..., :w]
    if kind in ("fwd", "dQ"):                                              # x[b, h, q, d] is pair (q, 64 t + d)
        where = (slice(None), heads, slice(None), slice(64 * t, 64 * t + w))
    else:                                                                  # x[b, h, k, d] is pair (64 t + d, k)
        where = (slice(None), heads, slice(64 * t, 64 * t + w), slice(None))
        x = x.transpose(-1, -2)
    ref = ref_keep[where]
    if kind in ("fwd", "dV"):
        got = x != 0
        err = torch.where(got, (x / (c / n) - 1.0).abs() / 2.0 ** -7, torch.zeros_like(x))
    else:
        delta = c * ref_keep[:, heads].sum(-1, keepdim=True).double() / n  # [B, H, Sq, 1]
        delta = delta if kind == "dQ" else delta[:, :, 64 * t:64 * t + w]
        gap = scale * c / n
        err = (x - scale * (c * ref.double() - delta) / n).abs() / (gap / 64.0)
        got = x * (n / scale) + delta > c / 2
    return where, got, max(bad, float(err.max()) if err.numel() else 0.0)


def read_mask(kind, run, ref_keep, Hkv, p, scale, device="cpu", dtype=torch.float64):
    """All passes of readout `kind`.  run(q, k, v, do) -> {"O", "dQ", "dK", "dV"} [B, S, H, 64] (the kernels, or attention() with
    planted masks) -> (decoded bool [B, H, Sq, Sk] on the CPU, worst value error in units of the tolerance)."""
    B, Hq, Sq, Sk = ref_keep.shape
    ref_dev = ref_keep.to(device)
    mask = torch.zeros(B, Hq, Sq, Sk, dtype=torch.bool, device=device)
    worst = 0.0
    for t in range(passes(kind, Sq, Sk)):
        for g in range(Hq // Hkv if kind in ("dV", "dK") else 1):
            res = run(*readout_operands(kind, t, B, Hq, Hkv, Sq, Sk, device, dtype, g))
            where, got, err = decode(kind, t, res["O" if kind == "fwd" else kind], ref_dev, p, scale, g)
            mask[where] = got
            worst = max(worst, err)
    return mask.cpu(), worst


def first_mismatch(decoded, ref_keep):
    """None, or a line naming the first pair the decoded mask gets wrong and where it sits in the kernels' tiles."""
    bad = (decoded != ref_keep).nonzero()
    if bad.shape[0] == 0:
        return None
    b, h, q, k = (int(i) for i in bad[0])
    Sk = ref_keep.shape[-1]
    return (f"{bad.shape[0]} pairs differ; first (b, h, q, k) = ({b}, {h}, {q}, {k}): kernel {'kept' if bool(decoded[b, h, q, k]) else 'dropped'}, "
            f"reference {'kept' if bool(ref_keep[b, h, q, k]) else 'dropped'}; key tile {k // 64} of {(Sk + 63) // 64} (key {k % 64} of the tile, "
            f"{'odd' if k & 1 else 'even'} half of its pair, {Sk - k} keys from the end), query row {q % 32} of 32-row slice {q // 32} "
            f"(row {q % 16} of its 16-row group)")
