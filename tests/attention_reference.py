"""Float64 reference, per-element error bounds and a conforming emulation for the training attention kernels
(desta_attention_fwd / desta_attention_bwd, csrc/attention.hip).  Plain torch on the CPU; imported by the host test
(test_attention_bound_host.py) and the GPU test (test_gpu_attention_fp64.py).

Operands are the bf16 values the kernels see: q, dO [B, Sq, Hq, D], k, v [B, Sk, Hkv, D], scale, causal, kv_start [B] or None.
Key j is visible to query i iff kv_start[b] <= j < Sk and, when causal, j <= i + (Sk - Sq); the kv head of query head h is
h // (Hq // Hkv) (include/desta_hip.h).

`exact()` returns, in float64 with p the exact probabilities:
    O, lse (log2 domain: log2 sum_j 2^(scale log2(e) q.k_j); +inf for a row without a visible key), dQ, dK, dV
        rows without a visible key: O = 0 and zero gradients; keys in front of kv_start: dK = dV = 0;
    M_O  = sum_j p_ij |v_j|                      M_dV = sum_i p_ij |dO_i|   (summed over the query heads of a GQA group)
    A_ij = p_ij (|dP_ij| + |delta_i|)            dP = dO V^T, delta_i = sum_d dO_id O_id
    Ed_i = 2^-9 sum_d |dO_id O_id|               the error of delta taken from the bf16-rounded O (0 when O_f32 feeds delta)
    M_dQ = scale sum_j (2^-8 A_ij + 2 p_ij Ed_i) |k_j|
    M_dK = scale sum_i (2^-8 A_ij + 2 p_ij Ed_i) |q_i|                      (summed over the query heads of a GQA group)

Bounds (`bounds()`; the form of tests/test_gpu_decode_attention.py, same `bf16_ulp`):
    bound(O)  = 0.5 ulp_bf16(max(|out|, |ref|)) + 2^-8 M_O
    bound(dV) = 0.5 ulp_bf16(max(|out|, |ref|)) + 2^-8 M_dV
    bound(dQ) = 0.5 ulp_bf16(max(|out|, |ref|)) + M_dQ          bound(dK) likewise with M_dK
Derivation.  A bf16 rounding is a relative error of at most 2^-9 (half an ulp of an 8-bit significand).  The store of a result
is the first term.  O = sum_j p_ij v_j with p rounded once to bf16 before the MFMA: |error| <= 2^-9 sum_j p_ij |v_j|; doubled
(2^-8 = twice the half-ulp of one bf16-rounded operand) for what else a conforming kernel carries: the normaliser being the sum
of the unrounded p, fp32 accumulation, exp2.  dV = sum_i p_ij dO_i: the same with |dO|.  dS_ij = scale p_ij (dP_ij - delta_i)
is rounded once to bf16 before the dQ and dK MFMAs: |error| <= 2^-9 scale p_ij (|dP_ij| + |delta_i|) = 2^-9 scale A_ij, doubled
as above; and delta_i itself is off by up to Ed_i when it is formed from the rounded O (each O_id off by 2^-9 |O_id|), which
moves dS_ij by scale p_ij Ed_i, coherently over the keys of the row (the reason for desta_attn_desc.O_f32); doubled again.
Where every term of a sum is zero (padded query rows, keys in front of kv_start) the M's are zero, the reference is zero and
the bound collapses to "exactly 0".

Dropout (`keep` bool [B, Hq, Sq, Sk], `drop_scale` = c, the fp32 1 / (1 - p) the kernels multiply by; the DROP kernels of
csrc/attention.hip).  With pd_ij = c keep_ij p_ij the probabilities that enter P V and dV (the normaliser keeps the FULL sum):
    O = sum_j pd_ij v_j        dV = sum_i pd_ij dO_i        delta_i = sum_d dO_id O_id (of the dropped O)
    dS_ij = scale (pd_ij dP_ij - p_ij delta_i) = scale p_ij (c keep_ij dP_ij - delta_i)
The same derivation holds term by term, no extra term is needed: the kernels round c keep P ONCE to bf16 (forward :423-424 then
:438; dK / dV :1129 then :1134), so M_O and M_dV take pd for p; dS is rounded once, |error| <= 2^-9 scale (pd |dP| + p |delta|),
so A_ij = pd_ij |dP_ij| + p_ij |delta_i|; and the error of delta from the rounded O still moves dS_ij by scale p_ij Ed_i (p,
not pd: the delta term is not masked).  The product with c is one more fp32 rounding, under the doubling with the other fp32
work.  A dropped pair contributes nothing to M_O, M_dV or the dP part of A, so the bound TIGHTENS by what was dropped.  Measured
on the host (test_attention_bound_host.py, p = 0.1, mask of tests/dropout_reference.py): the emulation stays inside, ratios in
that file's docstring.  The mask comes from the caller; tests/dropout_reference.py restates it independently of the kernels.

`emulate()` is the same computation in float64 with a bf16 rounding at each point where the kernels round.  Rounding points,
by line of csrc/attention.hip (acc_frag, :116-121, is the fp32 -> bf16 conversion of an accumulator into an MFMA operand):
  forward, 4 waves (attn_fwd_k)         P = exp2(s - m), m the RUNNING maximum after the current 64-key tile, unnormalised: :438
                                        O = acc / l (l = sum of the unrounded P): :451, rounded in store_row_bf16, :288;  O_f32 copy unrounded: :453;  lse fp32: :454
  forward, 8 waves (attn_fwd8_k)        P against a reference that moves only when a tile maximum of the wave exceeds it by
                                        more than 2^6 (:668-677), unnormalised: :699;  O: :739, rounded in store_row_bf16_16B, :304-305;  O_f32: :741;  lse: :742.
                                        OTHER values are rounded than in the 4-wave kernel (the same p against another power-of-two-
                                        free reference), independently of it: its own emulation flag, `fwd8`
  delta (attn_delta_k)                  fp32 sum of dO * O from the bf16 O (:767) or from O_f32 (:763): no rounding of its own
  dQ, 4 waves (attn_bwd_dq_k)           P = exp2(s - lse) kept in fp32; dS = P (dP - delta) scale: :847;  dQ: :855 (store_row_bf16)
  dQ, 8 waves (attn_bwd_dq8_k)          delta formed in the kernel from the bf16 O in fp32 (:892-896): the SAME values as
                                        attn_delta_k up to summation order, so no flag of its own;  dS: :945;  dQ: :972 (store_row_bf16_16B)
  dK / dV (attn_bwd_dkdv_k)             P = exp2(s - lse), NORMALISED, for dV and dS for dK: :1134;  dK, dV: :1183 / :1200
  one query tile (attn_bwd_q64_k)       dS: :1351-1352 (the LDS image read by the dQ MFMAs) and :1357 (same values); P: :1357;
                                        dK, dV: :1394 / :1414;  the per-chunk dQ partials stay fp32 (:1428-1434) and are summed
                                        in fp32 before the ONE rounding of attn_dq_sum_k, :1491: no rounding point beyond the
                                        two-kernel path's, so no flag of its own either
  bias sums (attn_bwd_q64_k, TR)        fp32 sums of the UNROUNDED dK / dV accumulators: :1385
The emulation flags are therefore `o_f32` (delta from the unrounded output) and `fwd8` (the 8-wave forward's deferred
reference; every backward path takes O and so delta from the forward that ran).  Not emulated (the GPU test's factor 2 is for
these): fp32 accumulation order, the exp2 approximation, lse stored in fp32.

Seeded mutations of the emulation (`MUTATIONS`; `emulate(..., mutation=name)`), the errors these kernels can actually make:
  tile_edge_key     the last key of the first visible 64-key tile is hidden from the last 32 query rows of one head
  diagonal_key      the diagonal key (i + Sk - Sq) is hidden from the last 32-row block of one head
  o_row_scaled      one row of O is 1.05 x what it should be
  delta_neighbour   one row's delta is its neighbour's (shows on dQ and dK)
  gqa_short_sum     dK of one (late) key sums one query head of its GQA group too few (needs Hq > Hkv)
"""
import torch

LOG2E = 1.4426950408889634
DEFER_LOG2 = 6.0                                                       # ATTN_DEFER_LOG2 of csrc/attention.hip
MUTATIONS = ("tile_edge_key", "diagonal_key", "o_row_scaled", "delta_neighbour", "gqa_short_sum")
OLD_LIMIT = {"O": 8e-3, "dQ": 1.5e-2, "dK": 1.5e-2, "dV": 1.5e-2}      # the whole-tensor rel-L2 limits of test_attention_fwd_bwd
TENSORS = ("O", "dQ", "dK", "dV")


def bf16_ulp(x):
    return torch.exp2(torch.floor(torch.log2(x.clamp_min(2.0 ** -126))) - 7)


def rbf(x):
    """float64 -> nearest bf16 value, as float64."""
    return x.float().bfloat16().double()


def _visible(B, Sq, Sk, causal, kv_start):
    ok = torch.ones(B, 1, Sq, Sk, dtype=torch.bool)
    if causal:
        ok = ok & (torch.arange(Sk)[None, :] <= torch.arange(Sq)[:, None] + (Sk - Sq))[None, None]
    if kv_start is not None:
        ok = ok & (torch.arange(Sk)[None, None, None, :] >= kv_start.clamp(0, Sk).long()[:, None, None, None])
    return ok


def _heads_first(x, rep=1):
    """[B, S, H, D] -> float64 [B, H * rep, S, D]"""
    x = x.double().permute(0, 2, 1, 3)
    return x.repeat_interleave(rep, dim=1) if rep > 1 else x


def _group_sum(x, Hkv):
    """[B, Hq, Sk, D] -> [B, Hkv, Sk, D]: sum over the query heads of each GQA group"""
    B, Hq, Sk, D = x.shape
    return x.view(B, Hkv, Hq // Hkv, Sk, D).sum(2)


def _rows_last(x):
    """[B, H, S, D] -> [B, S, H, D] (the layout of the operands)"""
    return x.permute(0, 2, 1, 3).contiguous()


def _softmax2(s2, ok):
    """scores in the log2 domain + visibility -> (p unnormalised against the row maximum, row maximum, row sum, any key visible)"""
    s2 = s2.masked_fill(~ok, float("-inf"))
    m = s2.amax(-1, keepdim=True)
    live = torch.isfinite(m)
    m = torch.where(live, m, torch.zeros_like(m))
    pu = torch.exp2(s2 - m)
    return pu, m, pu.sum(-1, keepdim=True), live


def _drop(keep, drop_scale, like):
    """The factor c * keep on the probabilities that enter P V and dV (1 without dropout): float64, like's shape."""
    if keep is None:
        return torch.ones_like(like)
    assert drop_scale is not None and tuple(keep.shape) == tuple(like.shape)
    return keep.double() * drop_scale


def exact(q, k, v, do, scale, causal=False, kv_start=None, o_f32=False, keep=None, drop_scale=None):
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G = Hq // Hkv
    qh, gh, kh, vh = _heads_first(q), _heads_first(do), _heads_first(k, G), _heads_first(v, G)
    ok = _visible(B, Sq, Sk, causal, kv_start)
    pu, m, l, live = _softmax2(qh @ kh.transpose(-1, -2) * (scale * LOG2E), ok)
    p = torch.where(live, pu / l.clamp_min(1e-300), torch.zeros_like(pu))
    lse = torch.where(live, m + torch.log2(l.clamp_min(1e-300)), torch.full_like(m, float("inf"))).squeeze(-1)
    cm = _drop(keep, drop_scale, p)
    pd = p * cm                                                        # dropout: what enters P V and dV; the normaliser kept the full sum
    O = pd @ vh
    dP = gh @ vh.transpose(-1, -2)
    delta = (gh * O).sum(-1, keepdim=True)
    dS = p * (cm * dP - delta) * scale
    A = p * (cm * dP.abs() + delta.abs())
    Ed = torch.zeros_like(delta) if o_f32 else 2.0 ** -9 * (gh * O).abs().sum(-1, keepdim=True)
    W = scale * (2.0 ** -8 * A + 2.0 * p * Ed)
    return {
        "O": _rows_last(O), "lse": lse, "live": live.squeeze(-1),
        "dQ": _rows_last(dS @ kh),
        "dK": _rows_last(_group_sum(dS.transpose(-1, -2) @ qh, Hkv)),
        "dV": _rows_last(_group_sum(pd.transpose(-1, -2) @ gh, Hkv)),
        "M_O": _rows_last(pd @ vh.abs()),
        "M_dV": _rows_last(_group_sum(pd.transpose(-1, -2) @ gh.abs(), Hkv)),
        "M_dQ": _rows_last(W @ kh.abs()),
        "M_dK": _rows_last(_group_sum(W.transpose(-1, -2) @ qh.abs(), Hkv)),
    }


def bounds(ref, name, out):
    """Per-element bound of tensor `name` ("O", "dQ", "dK", "dV") for the result `out` (float64, the reference's layout)."""
    half_ulp = 0.5 * bf16_ulp(torch.maximum(out.abs(), ref[name].abs()))
    if name in ("O", "dV"):
        return half_ulp + 2.0 ** -8 * ref["M_" + name]
    return half_ulp + ref["M_" + name]


def worst_ratio(ref, name, out):
    """max over the elements of |out - ref| / bound; inf if an element that must be exactly 0 is not (or out is not finite)."""
    out = out.double()
    if not bool(torch.isfinite(out).all()):
        return float("inf")
    err, bnd = (out - ref[name]).abs(), bounds(ref, name, out)
    zero = ref[name] == 0
    if bool((zero & (ref["M_" + name] == 0) & (out != 0)).any()):
        return float("inf")
    return float((err / bnd).max())


def rel_l2(out, ref):
    return float((out.double() - ref).norm() / (ref.norm() + 1e-30))


def accepted(ratio, emu_ratio):
    """The per-element criterion: within twice the conforming emulation's worst ratio on the same case and tensor, and within 2."""
    return ratio <= min(2.0, 2.0 * emu_ratio)


def emulate(q, k, v, do, scale, causal=False, kv_start=None, o_f32=False, mutation=None, fwd8=False, keep=None, drop_scale=None):
    """The conforming kernel (module docstring), optionally with one seeded mutation -> {"O", "dQ", "dK", "dV"} as float64 holding
    bf16 values, "lse" float64, and dK / dV before the store's rounding."""
    assert mutation is None or mutation in MUTATIONS
    B, Sq, Hq, D = q.shape
    Sk, Hkv = k.shape[1], k.shape[2]
    G, coff = Hq // Hkv, Sk - Sq
    qh, gh, kh, vh = _heads_first(q), _heads_first(do), _heads_first(k, G), _heads_first(v, G)
    ok = _visible(B, Sq, Sk, causal, kv_start).expand(B, Hq, Sq, Sk).clone()
    kv_lo = 0 if kv_start is None else int(kv_start.clamp(0, Sk)[0])
    r32 = torch.arange(max(0, Sq - 32), Sq)                              # the last 32 query rows
    if mutation == "tile_edge_key":
        ok[0, 0, r32, min(kv_lo // 64 * 64 + 63, Sk - 1)] = False
    if mutation == "diagonal_key":
        ok[0, Hq - 1, r32, r32 + coff] = False
    s2 = qh @ kh.transpose(-1, -2) * (scale * LOG2E)
    pu, m, l, live = _softmax2(s2, ok)
    # forward: P of each 64-key tile is rounded against the running maximum after that tile (4 waves) / the deferred reference (8 waves)
    nt = (Sk + 63) // 64
    s2m = torch.nn.functional.pad(s2.masked_fill(~ok, float("-inf")), (0, nt * 64 - Sk), value=float("-inf"))
    tmax = s2m.view(B, Hq, Sq, nt, 64).amax(-1)
    if fwd8:
        # attention.hip:662-677: a wave (32 query rows) moves EVERY row's reference to max(reference, tile maximum) when some row's
        # tile maximum exceeds its reference by more than 2^6, and leaves all of them where they are otherwise
        nw = (Sq + 31) // 32
        mref, refs = torch.full((B, Hq, Sq), float("-inf"), dtype=torch.float64), []
        for t in range(nt):
            trig = torch.nn.functional.pad(tmax[..., t] > mref + DEFER_LOG2, (0, nw * 32 - Sq)).view(B, Hq, nw, 32).any(-1)
            trig = trig.repeat_interleave(32, dim=-1)[..., :Sq]
            mref = torch.where(trig, torch.maximum(mref, tmax[..., t]), mref)
            refs.append(mref)
        mrun = torch.stack(refs, -1)
    else:
        mrun = torch.cummax(tmax, dim=-1).values
    mrun = mrun.repeat_interleave(64, dim=-1)[..., :Sk]
    mrun = torch.where(torch.isfinite(mrun), mrun, m.expand_as(mrun))   # tiles in front of the first visible key: P = 0 whatever the reference
    cm = _drop(keep, drop_scale, s2)
    pr = rbf(torch.exp2(s2.masked_fill(~ok, float("-inf")) - mrun) * cm) * torch.exp2(mrun - m)
    linv = torch.where(live, 1.0 / l.clamp_min(1e-300), torch.zeros_like(l))
    O32 = (pr @ vh) * linv
    if mutation == "o_row_scaled":
        row = min(Sq - 1, (kv_lo + 8 - coff) if causal else Sq // 2)       # a row with few visible keys: its outputs are large
        O32[0, 0, max(row, 0)] *= 1.05
    Ob = rbf(O32)
    lse = torch.where(live, m + torch.log2(l.clamp_min(1e-300)), torch.full_like(m, float("inf")))
    # backward: P = exp2(s - lse) (normalised), delta from the rounded O unless O_f32 feeds it
    p = torch.where(live, pu * linv, torch.zeros_like(pu))
    delta = (gh * (O32 if o_f32 else Ob)).sum(-1, keepdim=True)
    if mutation == "delta_neighbour":
        row = Sq // 2 + 1
        delta[0, 0, row] = delta[0, 0, row - 1]
    dS = rbf(p * (cm * (gh @ vh.transpose(-1, -2)) - delta) * scale)
    dK_h = dS.transpose(-1, -2) @ qh
    if mutation == "gqa_short_sum" and G > 1:
        dK_h[0, G - 1, max(Sk - 40, kv_lo)] = 0.0                    # a late key: few rows see it under the causal mask
    dK32, dV32 = _rows_last(_group_sum(dK_h, Hkv)), _rows_last(_group_sum(rbf(p * cm).transpose(-1, -2) @ gh, Hkv))
    return {"O": _rows_last(Ob), "lse": lse.squeeze(-1), "dQ": _rows_last(rbf(dS @ kh)), "dK": rbf(dK32), "dV": rbf(dV32),
            "dK_unrounded": dK32, "dV_unrounded": dV32}      # (the accumulators the one-pass kernel's bias sums are taken from)


def operands(case, seed=None):
    """The operands of test_attention_fwd_bwd for an entry of its ATTN_CASES (same generator, same draws): ->
    dict(q, k, v, do as bf16 [B, S, H, D] views; the flat buffers and column offsets the kernels are given; scale; kv_start)."""
    B, Hq, Hkv, Sq, Sk, D, causal, pad = case
    g = torch.Generator().manual_seed(Sq * 3 + Sk + D if seed is None else seed)
    fused = Sq == Sk
    wq, wkv = Hq * D, Hkv * D
    if fused:
        qb = kvb = torch.randn(B * Sq, wq + 2 * wkv, generator=g).bfloat16()
        q_off, k_off, v_off = 0, wq, wq + wkv
    else:
        qb = torch.randn(B * Sq, wq, generator=g).bfloat16()
        kvb = torch.randn(B * Sk, 2 * wkv, generator=g).bfloat16()
        q_off, k_off, v_off = 0, 0, wkv
    do = torch.randn(B * Sq, wq, generator=g).bfloat16()
    return {
        "case": case, "fused": fused, "qb": qb, "kvb": kvb, "do_b": do, "q_off": q_off, "k_off": k_off, "v_off": v_off,
        "q": qb[:, q_off:q_off + wq].reshape(B, Sq, Hq, D), "k": kvb[:, k_off:k_off + wkv].reshape(B, Sk, Hkv, D),
        "v": kvb[:, v_off:v_off + wkv].reshape(B, Sk, Hkv, D), "do": do.view(B, Sq, Hq, D),
        "scale": D ** -0.5, "causal": causal, "kv_start": torch.tensor(pad, dtype=torch.int32) if pad is not None else None,
    }


def reference(ops, o_f32=False, keep=None, drop_scale=None):
    """(exact, {forward kind: emulation}, {forward kind: {tensor: the emulation's worst |err| / bound}}) of operands()' result;
    forward kind False = the 4-wave forward, True = the 8-wave forward.  keep (bool [B, Hq, Sq, Sk]) and drop_scale: dropout."""
    a = (ops["q"], ops["k"], ops["v"], ops["do"], ops["scale"], ops["causal"], ops["kv_start"])
    ref = exact(*a, o_f32=o_f32, keep=keep, drop_scale=drop_scale)
    emu = {f8: emulate(*a, o_f32=o_f32, fwd8=f8, keep=keep, drop_scale=drop_scale) for f8 in (False, True)}
    return ref, emu, {f8: {n: worst_ratio(ref, n, emu[f8][n]) for n in TENSORS} for f8 in (False, True)}
