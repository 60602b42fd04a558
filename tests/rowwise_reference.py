"""Float64 references, per-element error bounds and conforming emulations for the row-wise training kernels of
csrc/norm_act.hip and csrc/embed_ce.hip (LayerNorm, RMSNorm, RoPE with q/k-norm, SwiGLU, GELU', the causal-LM loss, the tap
mix, prompt expand / grad).  Plain torch, float64; imported by the host test (test_rowwise_bound_host.py) and the GPU test
(test_gpu_rowwise_fp64.py), which share the case table `CASES` and the operand generator `operands()` below.  Every function
is device-agnostic (the GPU test evaluates the one large element-wise case on the device).

Per operation `OPS[name]` holds three functions over a dict of operands `o` (the bf16 / fp32 values the kernel sees):
    exact(o)                 -> {output: float64 result, "aux": whatever bound() needs}
    bound(o, ref, name, out) -> per-element bound of output `name` for the result `out` (float64)
    emulate(o, mutation)     -> {output: float64 holding the values a conforming kernel stores}, optionally with a seeded error

Notation.  ulp(v) = bf16_ulp(|v|) = 2^(floor(log2 |v|) - 7); H(v) = 0.5 ulp(v) is the error of ONE round-to-nearest-even to bf16
of a value of magnitude v (written in ulps: half an ulp is up to 2^-8 |v| just above a power of two, so 2^-9 |v| is NOT a bound).
F = 2^-24 is the relative error of one fp32 operation.  T = 2^-126 (the smallest normal fp32) is added to every bf16-store
bound: a conforming kernel may flush an fp32 subnormal (silu(-100) = -3.7e-42) to zero.

    bf16 store of a result r              S(out, ref) = H(max(|out|, |ref|)) + T                (the project's form)
    a bf16 rounding upstream of it        its H, evaluated at the exact value plus what was added before it, times the factor
                                          the rounded value is multiplied by afterwards
    fp32 sum of n terms t_i               c F sum |t_i|, c = the longest chain of dependent fp32 operations the kernel spends on
                                          it (the lane's sequential adds + the butterfly / LDS combine + the roundings of a term)
    fp32 output                           the fp32 terms alone

Chains.  A norm row of `cols` columns: a lane adds 8 values per 16-byte vector, ceil(cols / 512) vectors, then 6 butterfly
steps and the division: c_row = 8 ceil(cols / 512) + 7.  rsqrtf and the division by cols are counted in the +8 / +4 below.

layernorm_fwd (norm_act.hip:42-84; mean :59, rstd :69, stats :70, y :79-81).  d_mean = c_row F max|x| (the issue's conditioning
    term with the chain's factor: the mean is an fp32 sum of the row and is itself stored in fp32, and an offset row of mean 100
    and spread 0.05 turns an error of the mean into rstd d_mean of y), r_rstd = (c_row / 2 + 4) F + 0.5 (d_mean rstd)^2 (the
    variance is a sum of squares about the rounded mean: sum (x - m - d)^2 = sum (x - m)^2 + cols d^2).
        bound(mean) = d_mean        bound(rstd) = rstd r_rstd
        bound(y32)  = F ((c_row / 2 + 8) |xhat gamma| + |y|) + 0.5 (d_mean rstd)^2 |xhat gamma| + rstd |gamma| d_mean
        bound(y16)  = S + bound(y32)
    A constant row whose multiples are exact in fp32 has mean = the constant, every x - mean = 0 and y = beta EXACTLY; the tests
    assert that on its own (the bound there is dominated by rstd d_mean with rstd = eps^-1/2).
layernorm_bwd (:88-155, dx :131-133, partial sums :118-119, :150; reduce_partials_k :159-187).  stats are OPERANDS.
    gy = dy gamma, xh = (x - mean) rstd, s1 = mean(gy), s2 = mean(gy xh), dx = rstd (gy - s1 - xh s2)
        bound(dx32)   = F rstd (4 (|gy| + |s1| + |xh s2|) + (c_row + 3) (mean|gy| + |xh| mean|gy xh|))
        bound(dx16)   = S + bound(dx32)
        bound(dgamma) = c_col F sum_rows |dy xh| [+ F (|before| + |sum|) with accumulate],  dbeta likewise with |dy|
    c_col = trips + ceil(nb / 64) + 15: nb = min(ceil(rows / 4), 512) blocks, a wave adds `trips` = ceil(rows / (4 nb)) rows,
    the 4 waves combine in 2 steps (:150), a reduce group adds ceil(nb / 64) (+1) rows per accumulator, 2 + 6 steps to combine
    (:178, :183), and a term carries the 3 roundings of xh and the product.
rmsnorm_fwd (:223-252; rstd :238, y = w * bf16(x * rstd) :248, store :249).  t = x rstd, r_rstd = (c_row / 2 + 4) F.
        bound(rstd) = rstd r_rstd
        bound(y)    = S + |w| H(|t| (1 + r_rstd)) + F (c_row / 2 + 6) |w t|
rmsnorm_bwd (:256-304; s :283-286, dx :296-301).  rstd is an operand.  u = dy w, t = x rstd, s = mean(u t), dx = rstd (u - t s) + dres
        bound(dx) = S + F (4 rstd (|u| + |t s|) + |dres| + |dx| + (c_row + 3) rstd |t| mean|u t|)
rope (:314-404).  Pair (a, b) = elements (e, e + hd / 2) of a head, (c, s) = cos_sin[pos]; pos = max(0, spos + pos_shift[b]) (:336),
    (spos, b) = (row // s_major_batch, row % s_major_batch) or (row % seq, row // seq) (:335).
    forward, no norm (:363-365)     out_a = a c - b s, out_b = b c + a s: bound = S + 3 F (|a c| + |b s|)
    forward, q/k-norm (:357-358)    a' = bf16(w bf16(a rstd)): E_a = |w| H(|a rstd| (1 + 16 F)) + H(|w a rstd| + |w| H(a rstd)) + 16 F |w a rstd|
                                    bound = S + |c| E_a + |s| E_b + 3 F (|a' c| + |b' s|)
    backward, no norm (:374)        ga = a c + b s, gb = b c - a s: as the forward
    backward, q/k-norm (:375-401)   from the SAVED pre-norm x: g = (rotated gradient) w, xh = x rstd, t = mean(g xh),
                                    out = rstd (g - xh t), all fp32: bound = S + F rstd (8 (|g| + |xh t|) + 32 |xh| mean|g xh|)
    Columns outside the rotated heads (V, padding up to ld) are not touched: bound 0, compared bit for bit.
swiglu_fwd (:408-423; silu rounded :419, store :421).  sg = g / (1 + exp(-g)).  The operation is DEFINED with the inner rounding
    (the bf16 module output of silu, as the model it follows computes it): exact() = bf16(sg) u, so a kernel that does not
    round differs by up to |u| H(sg), beyond the store's half ulp.  r_e = (2 |g| + 8) F is the relative error of the fp32 sg
    (__expf(x) = exp2(x log2 e): the product's rounding moves the result by |x| F relatively); where sg (1 - r_e) and
    sg (1 + r_e) round to different bf16 values the fp32 error can move the inner rounding by one ulp:
        bound = S + r_e |sg u| + (|u| ulp(sg) where the inner rounding can flip, else 0)
swiglu_bwd (:424-444).  sig = 1 / (1 + exp(-g)); du = d g sig; dg = d u sig (1 + g (1 - sig)):
        bound(du) = S + r_e |du|        bound(dg) = S + r_e |d u| sig (1 + |g| (1 - sig)) + 4 F |d u| sig (1 + |g|)
        (1 - sig and 1 + g (1 - sig) cancel: their ABSOLUTE error is F, times what multiplies them)
gelu_bwd (:445-455, common.h gelu_erf_grad).  out = d (cdf + x pdf), cdf = 0.5 (1 + erf(x / sqrt 2)) formed in fp32:
        bound = S + |d| (4 F (0.5 + 0.5 |erf|) + r_x |x| pdf),   r_x = (x^2 + 8) F
    (left of -4 the fp32 cdf is 0.5 - 0.5 = 0 + an absolute error of F: the sum's terms, not its value, set the error.)
causal_lm_loss (embed_ce.hip:78-87 count, :90-144 ce_row_k with scalar tails :103 :113 :121 :139, :150-218 ce_row_reg_k, :313-320).
    Row m = (b, s) predicts labels[b, s + 1]; the last row of a sequence and rows whose target is -100 are ignored; n = number
    of the others; loss = sum_m (lse_m - x_m[tgt]) / n; dlogits = (softmax(x) - onehot) / n in bf16 (:135, :142, :213).
        bound(loss)    = 2e-5 max(1, loss)                                   (the project's limit, now against float64)
        bound(dlogits) = S + (p r_p + 2 F (p + onehot)) / n,   r_p = E_lse + (2.5 |x - lse| + 3) F,
                         E_lse = (c_V + 2 + |lse| + |log sum|) F + sum_i p_i (1.5 |x_i - max| + 2) F,  c_V = 8 ceil(V / 2048) + 16
    Ignored rows: exactly 0 (bound 0).  Columns [V, ld): not touched (bound 0, bit for bit).  All rows ignored: 1 / n is
    taken as 0 (:86), loss and every gradient exactly 0.  write_grad = 0: the logits stay bit for bit.
tap_mix_fwd (:325-341).  w = softmax(lw[k]); out = sum_j w_j x_j: bound = (taps + 8 + 2 max_j |lw_j - max|) F sum_j w_j |x_j|
tap_mix_bwd (:344-369).  dx_j = w_j dout: bound (taps + 8 + 2 max|lw - max|) F |dx|.  ds_j = sum_{b, c} dout x_j (a thread adds
    batch ceil(d / 1024) four-element dots, then 6 + 4 steps), dlw_j = w_j (ds_j - sum_i w_i ds_i):
        bound(dlw) = c F w_j (A_j + sum_i w_i A_i),  A_j = sum |dout x_j|,  c = 3 batch ceil(d / 1024) + taps + 24 + 2 max|lw - max|
prompt_expand (:372-384): the fp32 copy and its round-to-nearest-even to bf16 are exact: bound 0 both.
prompt_grad (:386-399): fixed-order fp32 sum over the batch: bound = batch F sum_b |dx|.

`emulate()` is float64 with a rounding where the kernel rounds to bf16 (the lines cited above) and where it STORES fp32 (stats,
rstd, y32, dx32, dgamma / dbeta, loss, the tap mix, the prompt gradient: rounded once to fp32).  Not emulated (the GPU test's
factor 2 is for these): fp32 accumulation order, fused multiply-adds, __expf / __logf / rsqrtf / erff.

Seeded mutations (`MUTATIONS`: name -> operations it applies to), the errors these kernels can actually make:
    rstd_scaled        rstd x 1.003                                                  layernorm_fwd, rmsnorm_fwd
    eps_1e-2           eps replaced by 1e-2                                          layernorm_fwd, rmsnorm_fwd
    neighbour_vector   the last 16-byte vector of the last row is the row above's    layernorm_fwd, rmsnorm_fwd
    one_pass_variance  var = E[x^2] - mean^2 in fp32                                 layernorm_fwd
    ce_tail_unwritten  columns [V - V % 8, V) left as logits                         causal_lm_loss
    ce_offtarget_2pct  non-target gradients x 1.02                                   causal_lm_loss
    ce_count_unshifted 1 / n counted over the unshifted labels                       causal_lm_loss
    rope_no_clamp      position not clamped at 0 (the table is read from its end)    rope
    rope_batch_major   position taken batch-major under s_major_batch                rope
    silu_unrounded     silu not rounded before the product                           swiglu_fwd
    ln_second_trip     rows of the second grid-stride trip missing in dgamma / dbeta layernorm_bwd
    mix_cols_1024      tap mix columns >= 1024 not written (left 0)                  tap_mix_fwd

`OLD_LIMIT` records the whole-tensor criteria of tests/test_gpu_ops.py per operation and output: ("rel_l2", limit) or
("close", rtol, atol) (torch.testing.assert_close); `old_passes` applies one.
"""
import math

import torch

from attention_reference import bf16_ulp, rbf

F = 2.0 ** -24
T = 2.0 ** -126
SENTINEL = 7.0

MUTATIONS = {
    "rstd_scaled": ("layernorm_fwd", "rmsnorm_fwd"),
    "eps_1e-2": ("layernorm_fwd", "rmsnorm_fwd"),
    "neighbour_vector": ("layernorm_fwd", "rmsnorm_fwd"),
    "one_pass_variance": ("layernorm_fwd",),
    "ce_tail_unwritten": ("causal_lm_loss",),
    "ce_offtarget_2pct": ("causal_lm_loss",),
    "ce_count_unshifted": ("causal_lm_loss",),
    "rope_no_clamp": ("rope",),
    "rope_batch_major": ("rope",),
    "silu_unrounded": ("swiglu_fwd",),
    "ln_second_trip": ("layernorm_bwd",),
    "mix_cols_1024": ("tap_mix_fwd",),
}

OLD_LIMIT = {
    "layernorm_fwd": {"y32": ("close", 1e-5, 2e-5), "y16": ("close", 1e-2, 1e-2)},
    "layernorm_bwd": {"dx32": ("close", 1e-4, 1e-4), "dx16": ("rel_l2", 1e-2), "dgamma": ("close", 1e-4, 1e-4),
                      "dbeta": ("close", 1e-4, 1e-4)},
    "rmsnorm_fwd": {"y": ("rel_l2", 6e-3)},
    "rmsnorm_bwd": {"dx": ("rel_l2", 6e-3)},
    "rope": {"out": ("rel_l2", 8e-3)},
    "swiglu_fwd": {"act": ("rel_l2", 6e-3)},
    "swiglu_bwd": {"dgu": ("rel_l2", 6e-3)},
    "gelu_bwd": {"dpre": ("rel_l2", 6e-3)},
    "causal_lm_loss": {"dlogits": ("rel_l2", 5e-3), "loss": ("loss", 2e-5)},
    "tap_mix_fwd": {"out": ("close", 1e-5, 1e-5)},
    "tap_mix_bwd": {"dx": ("close", 1e-5, 1e-5), "dlw": ("close", 1e-4, 1e-4)},
}


def H(v):
    """error of one round-to-nearest-even to bf16 of a value of magnitude v"""
    return 0.5 * bf16_ulp(v.abs())


def S(out, ref):
    """the bf16 store of a result"""
    return H(torch.maximum(out.abs(), ref.abs())) + T


def r32(x):
    """float64 -> nearest fp32 value, as float64"""
    return x.float().double()


def f32(v):
    """a python float as the fp32 value a kernel argument carries"""
    return float(torch.tensor(v, dtype=torch.float32))


def c_row(cols):
    return 8 * ((cols + 511) // 512) + 7


def rel_l2(out, ref):
    return float((out.double() - ref).norm() / (ref.norm() + 1e-30))


def old_passes(limit, out, ref):
    out, ref = out.double(), ref.double()
    if limit[0] == "rel_l2":
        return rel_l2(out, ref) < limit[1]
    if limit[0] == "loss":
        return abs(float(out) - float(ref)) < limit[1] * max(1.0, float(ref))
    return bool(((out - ref).abs() <= limit[2] + limit[1] * ref.abs()).all())


def worst_ratio(err, bnd):
    """max |err| / bound; where the bound is 0 the error must be 0 (inf otherwise, and for a result that is not finite)."""
    if err.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    zero = bnd == 0
    if bool((zero & (err != 0)).any()):
        return float("inf")
    return float((err / torch.where(zero, torch.ones_like(bnd), bnd)).max())


def ratio(op, o, ref, name, out):
    out = out.double()
    return worst_ratio((out - ref[name]).abs(), OPS[op].bound(o, ref, name, out))


class Op:
    def __init__(self, outputs, exact, bound, emulate):
        self.outputs, self.exact, self.bound, self.emulate = outputs, exact, bound, emulate


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def _ln_exact(o):
    x, g, b = o["x"].double(), o["gamma"].double(), o["beta"].double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + f32(o["eps"]))
    xg = (x - mean) * rstd * g
    return {"y32": xg + b, "y16": xg + b, "mean": mean.squeeze(-1), "rstd": rstd.squeeze(-1),
            "aux": {"xg": xg.abs(), "xmax": x.abs().amax(-1, keepdim=True), "g": g.abs(), "rstd": rstd}}


def _ln_bound(o, ref, name, out):
    a, c = ref["aux"], c_row(o["x"].shape[-1])
    dm = c * F * a["xmax"]
    sq = 0.5 * (dm * a["rstd"]) ** 2
    if name == "mean":
        return dm.squeeze(-1)
    if name == "rstd":
        return (a["rstd"] * ((c / 2 + 4) * F + sq)).squeeze(-1)
    b32 = F * ((c / 2 + 8) * a["xg"] + ref["y32"].abs()) + sq * a["xg"] + a["rstd"] * a["g"] * dm
    return b32 if name == "y32" else S(out, ref["y16"]) + b32


def _neighbour(y):
    if y.shape[0] > 1:
        y[-1, -8:] = y[-2, -8:]
    return y


def _ln_emulate(o, mutation=None):
    x, g, b = o["x"].double(), o["gamma"].double(), o["beta"].double()
    eps = 1e-2 if mutation == "eps_1e-2" else f32(o["eps"])
    mean = r32(x.mean(-1, keepdim=True))
    if mutation == "one_pass_variance":
        xf = o["x"].float()
        m = xf.mean(-1, keepdim=True)
        var = ((xf * xf).mean(-1, keepdim=True) - m * m).clamp_min(0).double()
    else:
        var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = r32(1.0 / torch.sqrt(var + eps))
    if mutation == "rstd_scaled":
        rstd = rstd * 1.003
    y = (x - mean) * rstd * g + b
    if mutation == "neighbour_vector":
        y = _neighbour(y)
    return {"y32": r32(y), "y16": rbf(y), "mean": mean.squeeze(-1), "rstd": rstd.squeeze(-1)}


def ln_bwd_blocks(rows):
    return min((rows + 3) // 4, 512)


def _lnb_terms(o):
    dy, x, g, st = o["dy"].double(), o["x"].double(), o["gamma"].double(), o["stats"].double()
    mean, rstd = st[:, 0:1], st[:, 1:2]
    xh, gy = (x - mean) * rstd, dy * g
    return dy, xh, gy, rstd


def _lnb_exact(o):
    dy, xh, gy, rstd = _lnb_terms(o)
    s1, s2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    dx = rstd * (gy - s1 - xh * s2)
    dg, db = (dy * xh).sum(0), dy.sum(0)
    prev = o.get("prev")
    aux = {"mag": rstd * (gy.abs() + s1.abs() + (xh * s2).abs()),
           "red": rstd * (gy.abs().mean(-1, keepdim=True) + xh.abs() * (gy * xh).abs().mean(-1, keepdim=True)),
           "A_dgamma": (dy * xh).abs().sum(0), "A_dbeta": dy.abs().sum(0), "sum_dgamma": dg, "sum_dbeta": db}
    if prev is not None:
        dg, db = dg + prev[0].double(), db + prev[1].double()
    return {"dx32": dx, "dx16": dx, "dgamma": dg, "dbeta": db, "aux": aux}


def _lnb_bound(o, ref, name, out):
    a, rows, cols = ref["aux"], o["x"].shape[0], o["x"].shape[1]
    if name in ("dx32", "dx16"):
        b32 = F * (4 * a["mag"] + (c_row(cols) + 3) * a["red"])
        return b32 if name == "dx32" else S(out, ref["dx16"]) + b32
    nb = ln_bwd_blocks(rows)
    c_col = (rows + 4 * nb - 1) // (4 * nb) + (nb + 63) // 64 + 15
    b = c_col * F * a["A_" + name]
    if o.get("prev") is not None:
        b = b + F * (o["prev"][0 if name == "dgamma" else 1].double().abs() + a["sum_" + name].abs())
    return b


def _lnb_emulate(o, mutation=None):
    dy, xh, gy, rstd = _lnb_terms(o)
    s1, s2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    dx = rstd * (gy - s1 - xh * s2)
    keep = slice(0, 4 * ln_bwd_blocks(dy.shape[0])) if mutation == "ln_second_trip" else slice(None)
    dg, db = r32((dy * xh)[keep].sum(0)), r32(dy[keep].sum(0))
    if o.get("prev") is not None:
        dg, db = r32(dg + o["prev"][0].double()), r32(db + o["prev"][1].double())
    return {"dx32": r32(dx), "dx16": rbf(dx), "dgamma": dg, "dbeta": db}


# ------------------------------------------------------------------------------------------------------------ RMSNorm
def _rms_exact(o):
    x, w = o["x"].double(), o["w"].double()
    rstd = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + f32(o["eps"]))
    t = x * rstd
    return {"y": w * t, "rstd": rstd.squeeze(-1), "aux": {"t": t.abs(), "w": w.abs(), "rstd": rstd}}


def _rms_bound(o, ref, name, out):
    a, c = ref["aux"], c_row(o["x"].shape[-1])
    rr = (c / 2 + 4) * F
    if name == "rstd":
        return (a["rstd"] * rr).squeeze(-1)
    return S(out, ref["y"]) + a["w"] * H(a["t"] * (1 + rr)) + F * (c / 2 + 6) * a["w"] * a["t"]


def _rms_emulate(o, mutation=None):
    x, w = o["x"].double(), o["w"].double()
    eps = 1e-2 if mutation == "eps_1e-2" else f32(o["eps"])
    rstd = r32(1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps))
    if mutation == "rstd_scaled":
        rstd = rstd * 1.003
    y = rbf(w * rbf(x * rstd))
    if mutation == "neighbour_vector":
        y = _neighbour(y)
    return {"y": y, "rstd": rstd.squeeze(-1)}


def _rmsb_exact(o):
    dy, x, w, rstd = o["dy"].double(), o["x"].double(), o["w"].double(), o["rstd"].double()[:, None]
    u, t = dy * w, x * rstd
    s = (u * t).mean(-1, keepdim=True)
    dres = o["dres"].double() if o.get("dres") is not None else torch.zeros_like(x)
    dx = rstd * (u - t * s) + dres
    return {"dx": dx, "aux": {"b32": F * (4 * rstd * (u.abs() + (t * s).abs()) + dres.abs() + dx.abs()
                                          + (c_row(x.shape[-1]) + 3) * rstd * t.abs() * (u * t).abs().mean(-1, keepdim=True))}}


def _rmsb_bound(o, ref, name, out):
    return S(out, ref["dx"]) + ref["aux"]["b32"]


def _rmsb_emulate(o, mutation=None):
    return {"dx": rbf(_rmsb_exact(o)["dx"])}


# ------------------------------------------------------------------------------------------------------------ RoPE
def rope_positions(o, mutation=None):
    rows, seq, smb = o["buf"].shape[0], o["seq"], o.get("s_major_batch", 0)
    r = torch.arange(rows)
    if smb and mutation != "rope_batch_major":
        spos, bidx = r // smb, r % smb
    else:
        spos, bidx = r % seq, r // seq
    if o.get("pos_shift") is None:
        return spos
    pos = spos + o["pos_shift"].long()[bidx]
    return pos if mutation == "rope_no_clamp" else pos.clamp_min(0)


def _rope_parts(o, mutation=None):
    hd, nh = o["hd"], o["n_q"] + o["n_kv"]
    rows = o["buf"].shape[0]
    h2 = hd // 2
    heads = o["buf"][:, :nh * hd].double().view(rows, nh, hd)
    cs = o["cos_sin"].double()[rope_positions(o, mutation)]            # [rows, 2, h2] (negative positions index from the end)
    c, s = cs[:, 0][:, None, :], cs[:, 1][:, None, :]
    w = None
    if o.get("wq") is not None:
        w = torch.cat([o["wq"].double()[None].expand(o["n_q"], -1), o["wk"].double()[None].expand(o["n_kv"], -1)])[None]
    return heads[..., :h2], heads[..., h2:], c, s, w, h2


def _rope_compute(o, rounded, mutation=None):
    """-> (out [rows, ld] float64 before the store's rounding, fp32 / upstream part of the bound over the head columns)"""
    a, b, c, s, w, h2 = _rope_parts(o, mutation)
    rows, nh, hd = a.shape[0], a.shape[1], o["hd"]
    eps = f32(o.get("eps", 1e-6))
    if not o["backward"]:
        if w is not None:
            rstd = 1.0 / torch.sqrt((a * a + b * b).sum(-1, keepdim=True) / hd + eps)
            wa, wb = w[..., :h2], w[..., h2:]
            ta, tb = a * rstd, b * rstd
            Ea = wa.abs() * H(ta * (1 + 16 * F)) + H((wa * ta).abs() + wa.abs() * H(ta)) + 16 * F * (wa * ta).abs()
            Eb = wb.abs() * H(tb * (1 + 16 * F)) + H((wb * tb).abs() + wb.abs() * H(tb)) + 16 * F * (wb * tb).abs()
            a, b = (rbf(wa * rbf(ta)), rbf(wb * rbf(tb))) if rounded else (wa * ta, wb * tb)
        else:
            Ea = Eb = torch.zeros_like(a)
        oa, ob = a * c - b * s, b * c + a * s
        extra_a = c.abs() * Ea + s.abs() * Eb + 3 * F * ((a * c).abs() + (b * s).abs())
        extra_b = c.abs() * Eb + s.abs() * Ea + 3 * F * ((b * c).abs() + (a * s).abs())
    else:
        ga, gb = a * c + b * s, b * c - a * s
        extra_a = 3 * F * ((a * c).abs() + (b * s).abs())
        extra_b = 3 * F * ((b * c).abs() + (a * s).abs())
        if w is not None:
            pre = o["pre"][:, :nh * hd].double().view(rows, nh, hd)
            xa, xb = pre[..., :h2], pre[..., h2:]
            rstd = 1.0 / torch.sqrt((xa * xa + xb * xb).sum(-1, keepdim=True) / hd + eps)
            ga, gb, xa, xb = ga * w[..., :h2], gb * w[..., h2:], xa * rstd, xb * rstd
            t = (ga * xa + gb * xb).sum(-1, keepdim=True) / hd
            tabs = ((ga * xa).abs() + (gb * xb).abs()).sum(-1, keepdim=True) / hd
            extra_a = F * rstd * (8 * (ga.abs() + (xa * t).abs()) + 32 * xa.abs() * tabs)
            extra_b = F * rstd * (8 * (gb.abs() + (xb * t).abs()) + 32 * xb.abs() * tabs)
            ga, gb = rstd * (ga - xa * t), rstd * (gb - xb * t)
        oa, ob = ga, gb
    out = o["buf"].double().clone()
    out[:, :nh * hd] = torch.cat([oa, ob], -1).reshape(rows, nh * hd)
    extra = torch.zeros_like(out)
    extra[:, :nh * hd] = torch.cat([extra_a, extra_b], -1).reshape(rows, nh * hd)
    return out, extra


def _rope_exact(o):
    out, extra = _rope_compute(o, rounded=False)
    return {"out": out, "aux": {"extra": extra}}


def _rope_bound(o, ref, name, out):
    nhd = (o["n_q"] + o["n_kv"]) * o["hd"]
    b = torch.zeros_like(out)                                          # V heads and padding: not touched
    b[:, :nhd] = (S(out, ref["out"]) + ref["aux"]["extra"])[:, :nhd]
    return b


def _rope_emulate(o, mutation=None):
    out, _ = _rope_compute(o, rounded=True, mutation=mutation)
    nhd = (o["n_q"] + o["n_kv"]) * o["hd"]
    out[:, :nhd] = rbf(out[:, :nhd])
    return {"out": out}


# ------------------------------------------------------------------------------------------------------------ SwiGLU / GELU'
def _sig(g):
    return torch.sigmoid(g)                                            # float64: exact to 1e-16 relative on both tails


def _gu(o):
    I = o["I"]
    gu = o["gu"].double()
    return gu[:, :I], gu[:, I:]


def _swf_exact(o):
    g, u = _gu(o)
    sg = g * _sig(g)
    re = (2 * g.abs() + 8) * F
    flip = rbf(sg * (1 + re)) != rbf(sg * (1 - re))                     # the fp32 error can move silu(g) across a rounding boundary
    extra = torch.where(flip, u.abs() * bf16_ulp(sg.abs() * (1 + re)), torch.zeros_like(sg)) + re * (sg * u).abs()
    return {"act": rbf(sg) * u, "aux": {"extra": extra}}


def _swf_bound(o, ref, name, out):
    return S(out, ref["act"]) + ref["aux"]["extra"]


def _swf_emulate(o, mutation=None):
    g, u = _gu(o)
    sg = g * _sig(g)
    return {"act": rbf((sg if mutation == "silu_unrounded" else rbf(sg)) * u)}


def _swb_exact(o):
    g, u = _gu(o)
    d = o["dact"].double()
    sig = _sig(g)
    re = (2 * g.abs() + 8) * F
    du = d * g * sig
    dg = d * u * sig * (1 + g * (1 - sig))
    extra_g = re * (d * u).abs() * sig * (1 + g.abs() * (1 - sig)) + 4 * F * (d * u).abs() * sig * (1 + g.abs())
    return {"dgu": torch.cat([dg, du], 1), "aux": {"extra": torch.cat([extra_g, re * du.abs()], 1)}}


def _swb_bound(o, ref, name, out):
    return S(out, ref["dgu"]) + ref["aux"]["extra"]


def _swb_emulate(o, mutation=None):
    return {"dgu": rbf(_swb_exact(o)["dgu"])}


def _gelu_exact(o):
    x, d = o["pre"].double(), o["dact"].double()
    cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))                 # no cancellation on the left tail
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    erf = torch.erf(x / math.sqrt(2.0)).abs()
    return {"dpre": d * (cdf + x * pdf),
            "aux": {"extra": d.abs() * (4 * F * (0.5 + 0.5 * erf) + (x * x + 8) * F * x.abs() * pdf)}}


def _gelu_bound(o, ref, name, out):
    return S(out, ref["dpre"]) + ref["aux"]["extra"]


def _gelu_emulate(o, mutation=None):
    return {"dpre": rbf(_gelu_exact(o)["dpre"])}


# ------------------------------------------------------------------------------------------------------------ causal-LM loss
def ce_targets(labels):
    """labels [B, S] -> target of row m = (b, s): labels[b, s + 1], -100 for the last row of a sequence"""
    t = torch.full_like(labels, -100)
    t[:, :-1] = labels[:, 1:]
    return t.reshape(-1)


def _ce_compute(o, mutation=None):
    V = o["V"]
    x = o["logits"][:, :V].double()
    tgt = ce_targets(o["labels"]).to(x.device)
    valid = tgt != -100
    n = int((o["labels"] != -100).sum()) if mutation == "ce_count_unshifted" else int(valid.sum())
    inv_n = 1.0 / n if n > 0 else 0.0
    mx = x.amax(-1, keepdim=True)
    e = torch.exp(x - mx)
    ssum = e.sum(-1, keepdim=True)
    lse = mx + torch.log(ssum)
    p = e / ssum
    onehot = torch.zeros_like(x)
    rows = torch.nonzero(valid).squeeze(-1)
    onehot[rows, tgt[rows]] = 1.0
    row_loss = torch.where(valid, lse.squeeze(-1) - (x * onehot).sum(-1), torch.zeros_like(mx.squeeze(-1)))
    loss = row_loss.sum() * inv_n
    grad = torch.where(valid[:, None], (p - onehot) * inv_n, torch.zeros_like(p))
    return x, valid, inv_n, mx, ssum, lse, p, onehot, loss, grad


def _ce_exact(o):
    V = o["V"]
    x, valid, inv_n, mx, ssum, lse, p, onehot, loss, grad = _ce_compute(o)
    c_V = 8 * ((V + 2047) // 2048) + 16
    E_lse = (c_V + 2 + lse.abs() + torch.log(ssum).abs()) * F + (p * (1.5 * (x - mx).abs() + 2) * F).sum(-1, keepdim=True)
    r_p = E_lse + (2.5 * (x - lse).abs() + 3) * F
    extra = torch.where(valid[:, None], (p * r_p + 2 * F * (p + onehot)) * inv_n, torch.zeros_like(p))
    out = o["logits"].double().clone()
    ex = torch.zeros_like(out)
    if o.get("write_grad", True):
        out[:, :V] = grad
        ex[:, :V] = extra
    return {"loss": loss, "dlogits": out, "aux": {"extra": ex, "valid": valid}}


def _ce_bound(o, ref, name, out):
    if name == "loss":
        return torch.tensor(2e-5 * max(1.0, float(ref["loss"])), dtype=torch.float64)
    V = o["V"]
    b = torch.zeros_like(out)                                          # [V, ld), ignored rows, write_grad = 0: exact
    if o.get("write_grad", True):
        rows = ref["aux"]["valid"]
        b[rows, :V] = (S(out, ref["dlogits"]) + ref["aux"]["extra"])[rows, :V]
    return b


def _ce_emulate(o, mutation=None):
    V = o["V"]
    x, valid, inv_n, mx, ssum, lse, p, onehot, loss, grad = _ce_compute(o, mutation)
    inv32 = float(r32(torch.tensor(inv_n, dtype=torch.float64)))
    g = torch.where(valid[:, None], (p - onehot) * inv32, torch.zeros_like(p))
    if mutation == "ce_offtarget_2pct":
        g = torch.where(onehot == 0, g * 1.02, g)
    g = rbf(g)
    if mutation == "ce_tail_unwritten":
        g[:, V - V % 8:] = x[:, V - V % 8:]
    out = o["logits"].double().clone()
    if o.get("write_grad", True):
        out[:, :V] = g
    return {"loss": r32(loss), "dlogits": out}


# ------------------------------------------------------------------------------------------------------------ tap mix
def _mix_parts(o):
    taps, B, K, d = o["taps"], o["batch"], o["prompt"], o["d"]
    x = o["x"].double().view(taps, B, K, d)
    lw = o["lw"].double()                                              # [K, taps]
    w = torch.softmax(lw, -1)
    spread = (lw - lw.amax(-1, keepdim=True)).abs().amax(-1)           # [K]
    return x, w, spread


def _mixf_exact(o):
    x, w, spread = _mix_parts(o)
    wt = w.t()[:, None, :, None]                                       # [taps, 1, K, 1]
    c = (o["taps"] + 8 + 2 * spread)[None, :, None]
    return {"out": (wt * x).sum(0).reshape(-1, o["d"]), "aux": {"b": (c * F * (wt * x.abs()).sum(0)).reshape(-1, o["d"])}}


def _mixf_bound(o, ref, name, out):
    return ref["aux"]["b"]


def _mixf_emulate(o, mutation=None):
    out = r32(_mixf_exact(o)["out"])
    if mutation == "mix_cols_1024":
        out[:, 1024:] = 0.0
    return {"out": out}


def _mixb_exact(o):
    x, w, spread = _mix_parts(o)
    taps, B, K, d = o["taps"], o["batch"], o["prompt"], o["d"]
    g = o["dout"].double().view(B, K, d)
    wt = w.t()[:, None, :, None]
    dx = (wt * g[None]).reshape(taps, B * K, d)
    ds = (g[None] * x).sum((1, 3)).t()                                 # [K, taps]
    A = (g[None] * x).abs().sum((1, 3)).t()
    dlw = w * (ds - (w * ds).sum(-1, keepdim=True))
    c = 3 * B * ((d + 1023) // 1024) + taps + 24 + 2 * spread[:, None]
    cx = (taps + 8 + 2 * spread)[None, None, :, None]
    return {"dx": dx, "dlw": dlw, "aux": {"dx": (cx * F * (wt * g[None]).abs()).reshape(taps, B * K, d),
                                          "dlw": c * F * w * (A + (w * A).sum(-1, keepdim=True))}}


def _mixb_bound(o, ref, name, out):
    return ref["aux"][name]


def _mixb_emulate(o, mutation=None):
    e = _mixb_exact(o)
    return {"dx": r32(e["dx"]), "dlw": r32(e["dlw"])}


# ------------------------------------------------------------------------------------------------------------ prompts
def _pe_exact(o):
    taps, B, n = o["taps"], o["batch"], o["n"]
    x = o["prompts"].double().view(taps, 1, n).expand(taps, B, n).reshape(taps * B, n)
    return {"x32": x, "x16": rbf(x), "aux": {}}


def _pe_bound(o, ref, name, out):
    return torch.zeros_like(out)


def _pe_emulate(o, mutation=None):
    e = _pe_exact(o)
    return {"x32": e["x32"], "x16": e["x16"]}


def _pg_exact(o):
    taps, B, n = o["taps"], o["batch"], o["n"]
    dx = o["dx"].double().view(taps, B, n)
    return {"dprompts": dx.sum(1), "aux": {"b": B * F * dx.abs().sum(1)}}


def _pg_bound(o, ref, name, out):
    return ref["aux"]["b"]


def _pg_emulate(o, mutation=None):
    taps, B, n = o["taps"], o["batch"], o["n"]
    dx = o["dx"].double().view(taps, B, n)
    acc = torch.zeros(taps, n, dtype=torch.float64)
    for b in range(B):                                                 # the kernel's fixed order, an fp32 add each
        acc = r32(acc + dx[:, b])
    return {"dprompts": acc}


OPS = {
    "layernorm_fwd": Op(("y32", "y16", "mean", "rstd"), _ln_exact, _ln_bound, _ln_emulate),
    "layernorm_bwd": Op(("dx32", "dx16", "dgamma", "dbeta"), _lnb_exact, _lnb_bound, _lnb_emulate),
    "rmsnorm_fwd": Op(("y", "rstd"), _rms_exact, _rms_bound, _rms_emulate),
    "rmsnorm_bwd": Op(("dx",), _rmsb_exact, _rmsb_bound, _rmsb_emulate),
    "rope": Op(("out",), _rope_exact, _rope_bound, _rope_emulate),
    "swiglu_fwd": Op(("act",), _swf_exact, _swf_bound, _swf_emulate),
    "swiglu_bwd": Op(("dgu",), _swb_exact, _swb_bound, _swb_emulate),
    "gelu_bwd": Op(("dpre",), _gelu_exact, _gelu_bound, _gelu_emulate),
    "causal_lm_loss": Op(("loss", "dlogits"), _ce_exact, _ce_bound, _ce_emulate),
    "tap_mix_fwd": Op(("out",), _mixf_exact, _mixf_bound, _mixf_emulate),
    "tap_mix_bwd": Op(("dx", "dlw"), _mixb_exact, _mixb_bound, _mixb_emulate),
    "prompt_expand": Op(("x32", "x16"), _pe_exact, _pe_bound, _pe_emulate),
    "prompt_grad": Op(("dprompts",), _pg_exact, _pg_bound, _pg_emulate),
}

# ------------------------------------------------------------------------------------------------------------ cases
# The smallest shapes that reach each path (the dispatch edges of LN_DISPATCH at 512 / 1024 / 2048 / 4096, the extremes 8 and
# 8192, a ragged last block over its 4 waves; the grid caps; the three loss kernels and their edges), shared by both tests.
NORM_COLS = (8, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192)
CE_VOCABS = (7, 1003, 16384, 50257, 163848,            # ce_row_k (scalar tails; above the register kernels' range)
             16392, 131072,                            # ce_row_reg_k<16>
             131080, 163840)                           # ce_row_reg_k<20>
ELEMENTWISE_BIG = (1200, 14336)                        # rows x I / 8 > 8192 x 256: a second grid-stride pass


def _cases():
    C = {k: [] for k in OPS}
    for cols in NORM_COLS:
        for rows in (1, 5):
            C["layernorm_fwd"].append({"rows": rows, "cols": cols, "x_f32": cols % 16 == 8, "eps": 1e-5, "data": "randn"})
            C["rmsnorm_fwd"].append({"rows": rows, "cols": cols})
            C["rmsnorm_bwd"].append({"rows": rows, "cols": cols, "dres": rows == 5})
            if cols <= 4096:
                for x_f32, dy_f32 in ((False, False), (True, True), (False, True), (True, False)):
                    C["layernorm_bwd"].append({"rows": rows, "cols": cols, "x_f32": x_f32, "dy_f32": dy_f32, "accumulate": False})
    for x_f32 in (True, False):
        for eps in (1e-5, 1e-12):
            C["layernorm_fwd"].append({"rows": 6, "cols": 1280, "x_f32": x_f32, "eps": eps, "data": "edges"})
    C["layernorm_bwd"] += [
        {"rows": 2053, "cols": 136, "x_f32": False, "dy_f32": False, "accumulate": False},     # > 512 x 4 rows, ragged: a second trip
        {"rows": 2053, "cols": 136, "x_f32": True, "dy_f32": True, "accumulate": True},
        {"rows": 261, "cols": 520, "x_f32": False, "dy_f32": True, "accumulate": False},      # 66 partial rows: unrolled loop + remainder
        {"rows": 261, "cols": 520, "x_f32": True, "dy_f32": False, "accumulate": True},
    ]
    for hd in (64, 128):
        for norm in (False, True):
            for backward in (False, True):
                heads = (6, 2) if hd == 64 else (2, 2)                          # 8 rows x heads x hd / 16 threads = 256 exactly
                C["rope"].append({"hd": hd, "norm": norm, "backward": backward, "B": 2, "S": 4, "n_q": heads[0], "n_kv": heads[1],
                                  "pos_shift": None, "s_major": False})
                C["rope"].append({"hd": hd, "norm": norm, "backward": backward, "B": 2, "S": 5, "n_q": 2, "n_kv": 1,
                                  "pos_shift": [-8, 2], "s_major": False})       # ragged grid; -8 < -seq: the clamp
                C["rope"].append({"hd": hd, "norm": norm, "backward": backward, "B": 2, "S": 5, "n_q": 2, "n_kv": 1,
                                  "pos_shift": [-2, 3], "s_major": True})
    for op in ("swiglu_fwd", "swiglu_bwd", "gelu_bwd"):
        C[op] += [{"rows": 3, "I": 8}, {"rows": 3, "I": 104}, {"rows": ELEMENTWISE_BIG[0], "I": ELEMENTWISE_BIG[1]}]
    for V in CE_VOCABS:
        C["causal_lm_loss"].append({"V": V, "labels": "mixed", "write_grad": True})
    C["causal_lm_loss"].append({"V": 50257, "labels": "mixed", "write_grad": True, "rows": "randn"})   # no saturated / flat row
    C["causal_lm_loss"] += [{"V": 1003, "labels": "mixed", "write_grad": False}, {"V": 16392, "labels": "mixed", "write_grad": False},
                            {"V": 1003, "labels": "ignored", "write_grad": True}, {"V": 131080, "labels": "ignored", "write_grad": True}]
    for taps, d in ((1, 4), (4, 1280), (32, 1028)):
        C["tap_mix_fwd"].append({"taps": taps, "d": d, "batch": 3, "prompt": 5})
        C["tap_mix_bwd"].append({"taps": taps, "d": d, "batch": 3, "prompt": 5})
    for n in (4, 5 * 1280):
        C["prompt_expand"].append({"taps": 4, "batch": 3, "n": n})
        C["prompt_grad"].append({"taps": 4, "batch": 3, "n": n})
    return C


CASES = _cases()
CE_B, CE_S = 2, 5
EDGE_CONST = 1.5            # the constant row: every multiple up to 8192 x 1.5 is exact in fp32


def case_id(case):
    return "-".join(f"{k}={v}" for k, v in case.items()).replace(" ", "")


def _bf(x):
    return x.to(torch.bfloat16)


def _spanning(shape, g, scale):
    """randn x scale with the saturation values +-100, +-30, +-8, +-5 and 0 planted at the front of every row"""
    x = torch.randn(*shape, generator=g) * scale
    pts = torch.tensor([0.0, 100.0, -100.0, 30.0, -30.0, 8.0, -8.0, 5.0, -5.0])
    n = min(shape[-1], pts.numel())
    x[..., :n] = pts[:n]
    if shape[0] > 1 and shape[-1] >= 8:
        x[1, :8] = torch.tensor([-100.0, 100.0, -60.0, 60.0, -12.0, 12.0, -1.25, 0.0])
    return x


def operands(op, case, seed=0):
    """The operands of one case, on the CPU, as the dtypes the kernel is given (deterministic in (op, case, seed))."""
    g = torch.Generator().manual_seed(1000 * seed + sum(ord(ch) for ch in op + case_id(case)))
    rn = lambda *s: torch.randn(*s, generator=g)
    if op == "layernorm_fwd":
        rows, cols = case["rows"], case["cols"]
        x = rn(rows, cols) * 2 + 0.5
        if case["data"] == "edges":
            x[1] = 100.0 + 0.05 * rn(cols)                              # mean 100, spread 0.05
            x[2] = EDGE_CONST                                           # variance 0
            x[3] = 1e-3 * rn(cols)
        x = x if case["x_f32"] else _bf(x)
        return {"x": x, "gamma": 1 + 0.1 * rn(cols), "beta": 0.1 * rn(cols), "eps": case["eps"]}
    if op == "layernorm_bwd":
        rows, cols = case["rows"], case["cols"]
        x, dy = rn(rows, cols) * 2 + 0.5, rn(rows, cols)
        x, dy = x if case["x_f32"] else _bf(x), dy if case["dy_f32"] else _bf(dy)
        gamma = 1 + 0.1 * rn(cols)
        e = _ln_exact({"x": x, "gamma": gamma, "beta": torch.zeros(cols), "eps": 1e-5})
        o = {"x": x, "dy": dy, "gamma": gamma, "stats": torch.stack([e["mean"], e["rstd"]], 1).float()}
        if case["accumulate"]:
            o["prev"] = (rn(cols) * 3, rn(cols) * 3)
        return o
    if op in ("rmsnorm_fwd", "rmsnorm_bwd"):
        rows, cols = case["rows"], case["cols"]
        x, w = _bf(rn(rows, cols) * 1.5), 1 + 0.1 * rn(cols)
        if op == "rmsnorm_fwd":
            return {"x": x, "w": w, "eps": 1e-5}
        o = {"x": x, "w": w, "dy": _bf(rn(rows, cols)), "rstd": _rms_exact({"x": x, "w": w, "eps": 1e-5})["rstd"].float()}
        o["dres"] = _bf(rn(rows, cols)) if case["dres"] else None
        return o
    if op == "rope":
        hd, B, Sq, nq, nkv = case["hd"], case["B"], case["S"], case["n_q"], case["n_kv"]
        rows, ld = B * Sq, (nq + 2 * nkv) * hd + 8                       # q | k | v | 8 padding columns
        P = Sq + 7                                                      # a table longer than seq
        inv = 10000.0 ** (-torch.arange(0, hd, 2).float() / hd)
        fr = torch.outer(torch.arange(P).float(), inv)
        o = {"buf": _bf(rn(rows, ld)), "ld": ld, "seq": Sq, "n_q": nq, "n_kv": nkv, "hd": hd, "eps": 1e-6,
             "cos_sin": torch.stack([fr.cos(), fr.sin()], 1).contiguous(), "backward": case["backward"],
             "pos_shift": torch.tensor(case["pos_shift"], dtype=torch.int32) if case["pos_shift"] is not None else None,
             "s_major_batch": B if case["s_major"] else 0, "wq": None, "wk": None, "pre": None}
        if case["norm"]:
            o["wq"], o["wk"] = 1 + 0.2 * rn(hd), 1 + 0.2 * rn(hd)
            if case["backward"]:
                o["pre"], o["ld_pre"] = _bf(rn(rows, (nq + nkv) * hd + 16) * 1.5), (nq + nkv) * hd + 16
        return o
    if op in ("swiglu_fwd", "swiglu_bwd", "gelu_bwd"):
        rows, I = case["rows"], case["I"]
        d = _bf(rn(rows, I))
        if op == "gelu_bwd":
            return {"pre": _bf(_spanning((rows, I), g, 2.0)), "dact": d, "n": rows * I}
        gu = torch.cat([_spanning((rows, I), g, 2.0), rn(rows, I) * 2], 1)
        o = {"gu": _bf(gu), "I": I, "rows": rows}
        if op == "swiglu_bwd":
            o["dact"] = d
        return o
    if op == "causal_lm_loss":
        V, B, Sq = case["V"], CE_B, CE_S
        ld = (V + 7) // 8 * 8
        logits = torch.full((B * Sq, ld), SENTINEL)
        logits[:, :V] = rn(B * Sq, V) * 3
        if case.get("rows") != "randn":
            logits[5, :V] = rn(V)
            logits[5, (V // 2 + 3) % V] = float(logits[5, :V].max()) + 60.0   # row (1, 0): saturated, the target elsewhere
            logits[8, :V] = 0.5                                         # row (1, 3): flat
        labels = torch.randint(0, V, (B, Sq), generator=g)
        labels[0, 1], labels[0, 2], labels[0, 3], labels[0, 4] = 0, V - 1, max(V - 2, 0), -100     # column 0, V - 1, the scalar tail
        labels[1, 0], labels[1, 3] = -100, -100
        if case["labels"] == "ignored":
            labels[:] = -100
        return {"logits": _bf(logits), "ld": ld, "labels": labels, "V": V, "write_grad": case["write_grad"]}
    if op in ("tap_mix_fwd", "tap_mix_bwd"):
        taps, B, K, d = case["taps"], case["batch"], case["prompt"], case["d"]
        o = {"taps": taps, "batch": B, "prompt": K, "d": d, "x": rn(taps, B * K, d), "lw": rn(K, taps) * 2}
        if op == "tap_mix_bwd":
            o["dout"] = rn(B * K, d)
        return o
    taps, B, n = case["taps"], case["batch"], case["n"]
    if op == "prompt_expand":
        return {"taps": taps, "batch": B, "n": n, "prompts": rn(taps, n)}
    return {"taps": taps, "batch": B, "n": n, "dx": rn(taps * B, n)}


ELEMENTWISE = ("swiglu_fwd", "swiglu_bwd", "gelu_bwd")
_ROW_KEYS = ("gu", "dact", "pre")


def row_chunks(op, o, step=128):
    """Operand dicts over row slices of an element-wise case (every row is independent): keeps float64 temporaries small."""
    if op not in ELEMENTWISE:
        yield slice(None), o
        return
    rows = next(o[k] for k in _ROW_KEYS if k in o).shape[0]
    for r0 in range(0, rows, step):
        sl = slice(r0, min(rows, r0 + step))
        yield sl, {k: (v[sl] if k in _ROW_KEYS else v) for k, v in o.items()}
