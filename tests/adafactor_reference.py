"""Float64 reference, per-element error bounds, a conforming emulation and the restated launch plan of the fused clip + Adafactor
step (csrc/adafactor.hip, planned by desta/optim.py:FusedAdafactor).  Plain torch; imports neither the library nor the GPU.
Imported by the host test (test_adafactor_bound_host.py) and the GPU test (test_gpu_adafactor_fp64.py), which share `CASES`.

One step, on exactly what the kernel sees (fp32 params / grads / state, the fp32 casts of lr, beta2t, eps1, clip_threshold,
max_grad_norm and of each tensor's weight decay) - the semantics of transformers.Adafactor(scale_parameter=False,
relative_step=False, beta1=None) after clip_grad_norm_, as oracle/desta_oracle.py:adafactor_step restates them:

    S = sum g^2 over the arena, norm = sqrt(S), c = min(1, max_norm / (norm + 1e-6f))   (c = 1 for max_norm <= 0)
    factored [nb, R, C]:  row' = b row + (1 - b) (c^2 sum_cols g^2 / C + eps1)     col' = b col + (1 - b) (c^2 sum_rows g^2 / R + eps1)
                          rfac = (row' / mean_R row')^-1/2  (PER BATCH ITEM)        cfac = col'^-1/2       u = c g rfac cfac
    1-D:                  sq' = b sq + (1 - b) ((c g)^2 + eps1)                     u = c g sq'^-1/2
    rms = sqrt(sum u^2 / numel) over the WHOLE tensor,  scale = lr / max(1, rms / clip_threshold),  p' = p (1 - wd lr) - scale u

Outputs are keyed "grad_norm", "coef", ("p", i), ("row", i), ("col", i), ("sq", i) with i the tensor's arena index.
    exact(o)            -> {key: float64}, plus "aux" for bound()
    bound(o, ref)       -> {key: per-element bound}
    emulate(o, mutation)-> {key: float64 holding fp32 values}: the step in float64 with one rounding to fp32 wherever the kernel
                           STORES or holds an fp32 scalar (the lines below); not emulated: the fp32 order inside a sum, fused
                           multiply-adds, rsqrtf / sqrtf / the division (the GPU test's factor 2 is for these)
    plan(shapes, group_floats) -> the tables FusedAdafactor.__init__ builds, each tensor's kernel form and its loop lengths

Bounds.  F = 2^-24, one fp32 rounding.  Every sum here has non-negative terms, so a term that passes through d roundings
(its own square + the adds it rides through) makes the sum's RELATIVE error at most d F (first order).  The depths, from the
loop lengths plan() returns (adafactor.hip lines):
    vec4 and ragged-wide units (stats_rows :71-99, scalar form :161-177; combine :181-197)
        d_row  = 1 + 2 + nseg + 6                 square :90/:170, (x + y) + (z + w) :92/:172, rsum += per segment, wave_sum
        d_unit = d_row + rows_per_wave + 2        tot += rsum :97/:176, the 4 waves :197
        d_col  = 1 + rows_per_wave + 2 + upb      cacc += :91/:171, the 4 waves :190, the units of a batch item :246
    narrow units (:138-158)
        d_row  = 1 + C                            :143
        d_unit = d_row + trips + 10               tot += rsum :146, block_sum :157 (6 butterfly steps + 4 serial adds)
        d_col  = 1 + trips + 10 + upb             ca[c] += :143, block_sum :152, the units :246
    1-D (:112-113)        d_vec = 1 + ceil(n / 256) + 10
    arena (:203-205)      d_all = ceil(U / 256) + ceil(V / 256) + 10
    sum u^2:  chunked 1 + 2 + 16 + 10 + ceil(chunks / 256) + 10  (:307, block_sum :320/:337, the chunk sums :351-352)
              narrow  1 + trips C + 10 + ceil(units / 256) + 10   (:428, :433, k34_totals_range :385-386)
              ragged-wide 1 + 4 nseg rows_per_wave + 10 + ceil(units / 256) + 10   (:463, :469, :385-386)
              1-D     1 + ceil(n / 256) + 10                      (:268, :270)
Library functions (ROCm's HIP math API accuracy table; build.py passes -O3 -ffp-contract=fast, no fast-math, and leaves clang's
default -fhip-fp32-correctly-rounded-divide-sqrt on): sqrtf 1 ulp, rsqrtf 1 ulp, `/` correctly rounded; all three are allowed
1 ulp = 2 F here.  -ffp-contract=fast may fuse any a * b + c: the fused form drops a rounding, so a bound that allows the
unfused form allows both.
    e_S    = (max d_unit, d_vec  +  d_all) F                  norm :206:   e_n = e_S / 2 + 2F        bound(grad_norm) = norm e_n
    coef :208   x = max_norm / (norm + 1e-6f): e_x = e_n + F + 2F; min(., 1) is continuous and cannot grow an error:
                bound(coef) = x e_x where x (1 - e_x) < 1, else 0 (both sides are exactly 1);  e_c = bound / coef
    c2 = c c :223: e_c2 = 2 e_c + F;   1.0f - beta2t :223: F
    row' :230   e_row = e_c2 + d_row F + 7F     (c2 * rowsum, / C, + eps1, omb *, beta2t * old, the add; relative: all terms >= 0)
    col' :247   e_col = e_c2 + d_col F + 7F
    sq'  :264-265  e_sq = 2 e_c + 8F
    rfac :235-237  e_rfac = e_row + (ceil(R / 256) + 10) F / 2 + 4F     (the row sum over the stored row', / R, / rmean, rsqrtf)
    cfac :249      e_cfac = e_col / 2 + 2F
    u    :304-306, :426, :450, :461   e_u = e_rfac + e_cfac + e_c + 3F;    1-D :275: e_u = e_c + e_sq / 2 + 4F
    rms  :353, :409, :271   e_rms = (2 e_u + d_usq F + 4F) / 2 + 2F    ((float) numel, the division, sqrtf)
    scale :354, :410, :272  e_scale = 2F + (e_rms + 2F where (rms / clip_thr)(1 + e_rms + 2F) > 1, else 0: max(1, .) is continuous)
    p'   :371, :427, :453, :462, :276   decay = 1 - wd lr: F (wd lr + 1) absolute; the two roundings of p decay - scale u:
         bound(p) = |p| F (wd lr + 1) + F |p decay| + |scale u| (e_scale + e_u + F) + F |p'|
No element is masked and no case is excused near max(1, .) or min(., 1).  Where a bound is 0 (a zero norm, coef = 1 well
inside the clip's inactive side) the output must be exact.

`MUTATIONS` are seeded wrong variants of emulate(), the errors this kernel and its plan can actually make:
    col_mean_over_cols   column mean divided by cols instead of rows
    eps_inside_c2        c^2 (mean + eps1)
    rfac_all_batches     row factor normalised over all batch items of a 3-D tensor
    rms_one_chunk        rms(u) from the first chunk / unit instead of the tensor
    c_not_squared        second moments scaled by c instead of c^2
    decay_after_update   (p - scale u)(1 - wd lr)
    decay_on_no_decay    the decayed group's weight decay on every tensor
    last_unit_dropped    the last unit of a batch item missing in the column reduction
    vec_unclipped        a 1-D state fed the unclipped gradient
    beta2t_previous      beta2t of the previous step
    coef_no_min          coef without min(., 1)
"""
import math

import torch

F = 2.0 ** -24
ALIGN, UNIT_ROWS, CHUNK, NARROW, MAXSEG = 64, 64, 16384, 16, 16
GROUP_FLOATS = 16 << 20
DECAY_RATE = -0.8
SENTINEL = 3.0e4                  # a large finite value: 9e8 squared, a read of it wrecks every sum it enters
OLD_RTOL, OLD_ATOL = 2e-6, 3e-7   # the parameters-only limits of tests/test_gpu_kernels.py:_run_adafactor_case
FORMS = ("vec4-5", "vec4-12", "vec4-16", "narrow", "ragged-wide", "1-D")

MUTATIONS = ("col_mean_over_cols", "eps_inside_c2", "rfac_all_batches", "rms_one_chunk", "c_not_squared", "decay_after_update",
             "decay_on_no_decay", "last_unit_dropped", "vec_unclipped", "beta2t_previous", "coef_no_min")


def _al(n, a=ALIGN):
    return (n + a - 1) // a * a


def _cdiv(a, b):
    return (a + b - 1) // b


def f32(v):
    """a python float as the fp32 value a kernel argument carries"""
    return float(torch.tensor(v, dtype=torch.float32))


def r32(x):
    """float64 -> nearest fp32 value, as float64"""
    return x.float().double()


def beta2t(step):
    return 1.0 - math.pow(step, DECAY_RATE)


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


# ------------------------------------------------------------------------------------------------------------ the plan
def unit_rows(R, C):
    """rows per statistics unit (optim.py: 64, or up to 32 K elements for a tensor with ragged rows)"""
    return UNIT_ROWS if C % 4 == 0 else max(UNIT_ROWS, min(R, 32768 // C))


def form_of(shape):
    if len(shape) < 2:
        return "1-D"
    C = shape[-1]
    if C % 4 == 0:
        nseg = _cdiv(C, 256)
        return "vec4-5" if nseg <= 5 else "vec4-12" if nseg <= 12 else "vec4-16"
    return "narrow" if C <= NARROW else "ragged-wide"


def plan(shapes, group_floats=GROUP_FLOATS):
    """FusedAdafactor.__init__'s tables for an arena of `shapes` (arena order, every tensor on a 64-float boundary), each tensor's
    kernel form and the loop lengths the bounds need."""
    offs, off = [], 0
    for s in shapes:
        offs.append(off)
        off += _al(math.prod(s))
    tensors, units, ucol, vecs, slots, forms, lens = [], [], [], [], [], [], []
    st, cw = 0, 0
    for i, s in enumerate(shapes):
        forms.append(form_of(s))
        if len(s) >= 2:
            R, C, nb = s[-2], s[-1], math.prod(s[:-2])
            row_off = st
            st += _al(nb * R, 4)
            col_off = st
            st += _al(nb * C, 4)
            ur = unit_rows(R, C)
            upb = _cdiv(R, ur)
            unit0 = len(units)
            for b in range(nb):
                for k in range(upb):
                    units.append([len(tensors), b, k * ur, min(ur, R - k * ur)])
                    ucol.append(cw)
                    cw += _al(C, 4)
            tensors.append([offs[i], nb, R, C, row_off, col_off, unit0, nb * upb])
            slots.append({"row": (row_off, nb * R), "col": (col_off, nb * C)})
            nseg, h = _cdiv(C, 256), min(ur, R)
            if forms[i] == "narrow":
                ln = {"cols_per_lane": C, "rows_per_wave": _cdiv(h, 256), "nseg": 1}
            elif forms[i] == "ragged-wide":
                ln = {"cols_per_lane": 4 * nseg, "rows_per_wave": _cdiv(h, 4), "nseg": nseg}
            else:
                rows = {"vec4-5": 4, "vec4-12": 2, "vec4-16": 1}[forms[i]]
                ln = {"cols_per_lane": 4 * nseg, "rows_per_wave": rows * _cdiv(h, 4 * rows), "nseg": nseg}
            ln.update(units_per_item=upb, units=nb * upb, unit_rows=ur, stats_rows={"vec4-5": 4, "vec4-12": 2, "vec4-16": 1}.get(forms[i]))
            lens.append(ln)
        else:
            n = math.prod(s)
            vecs.append([offs[i], n, st])
            slots.append({"sq": (st, n)})
            st += _al(n, 4)
            lens.append({"trips": _cdiv(n, 256)})
    fact = [i for i, s in enumerate(shapes) if len(s) >= 2]            # arena index of factored tensor ti
    chunks, ten_chunks, fin = [], [[0, 0] for _ in tensors], []
    ragged = [ti for ti, t in enumerate(tensors) if t[3] % 4]
    bounds, acc = [0], 0
    for ti in reversed(range(len(tensors))):
        _, nb, R, C = tensors[ti][:4]
        if ti in ragged:
            continue
        if acc and acc + nb * R * C > group_floats:
            bounds.append(len(chunks))
            acc = 0
        acc += nb * R * C
        ten_chunks[ti][0] = len(chunks)
        for b in range(nb):
            for e0 in range(0, R * C, CHUNK):
                chunks.append([ti, b, e0, min(CHUNK, R * C - e0)])
        ten_chunks[ti][1] = len(chunks) - ten_chunks[ti][0]
    bounds.append(len(chunks))
    for ti, (_, nb, R, C, *_r) in enumerate(tensors):
        for b in range(nb):
            fin += [[ti, b, part] for part in range(1 + _cdiv(C, 256))]
        lens[fact[ti]]["chunks"] = ten_chunks[ti][1]
    return {"offsets": offs, "numel": off, "tensors": tensors, "units": units, "unit_col_off": ucol, "vecs": vecs, "chunks": chunks,
            "ten_chunks": ten_chunks, "fin": fin, "ragged_units": [v for ti in ragged for v in tensors[ti][6:8]],
            "group_bounds": bounds, "n_groups": len(bounds) - 1, "state_floats": st, "colpart_floats": cw, "slots": slots,
            "forms": forms, "lens": lens, "units_plus_vecs": (len(units), len(vecs))}


# ------------------------------------------------------------------------------------------------------------ one step
def _step(o, rnd, mutation=None):
    """The step in float64 with `rnd` applied wherever the kernel holds an fp32 value (identity: the exact result)."""
    shapes, P, G, St = o["shapes"], o["params"], o["grads"], o["state"]
    lr, b2, eps1 = f32(o["lr"]), f32(o["beta2t"]), f32(o["eps1"])
    thr, mn = f32(o["clip_threshold"]), f32(o["max_grad_norm"])
    if mutation == "beta2t_previous":
        b2 = f32(o["beta2t_prev"])
    wds = [f32(o["weight_decay"]) if (d or mutation == "decay_on_no_decay") else 0.0 for d in o["decay"]]
    g64 = [g.double() for g in G]
    S = rnd(sum((g * g).sum() for g in g64) + torch.zeros((), dtype=torch.float64))                 # :203-205
    norm = rnd(torch.sqrt(S))                                                                       # :206
    x = mn / rnd(norm + f32(1e-6)) if mn > 0 else torch.ones((), dtype=torch.float64)
    c = rnd(x if mutation == "coef_no_min" else x.clamp(max=1.0)) if mn > 0 else x                  # :208
    c2 = rnd(c) if mutation == "c_not_squared" else rnd(c * c)                                      # :223
    omb = rnd(torch.tensor(1.0 - b2, dtype=torch.float64))
    out = {"grad_norm": norm, "coef": c}
    aux = {"x": x, "u": {}, "scale": {}, "rms": {}, "decay": {}}
    for i, s in enumerate(shapes):
        p, g = P[i].double(), g64[i]
        decay = rnd(1.0 - rnd(torch.tensor(wds[i] * lr, dtype=torch.float64)))                    # :355, :411, :273
        if len(s) >= 2:
            R, C = s[-2], s[-1]
            nb = math.prod(s[:-2])
            g3, g2 = g.reshape(nb, R, C), (g * g).reshape(nb, R, C)
            ur = unit_rows(R, C)
            upb = _cdiv(R, ur)
            rowsum = rnd(g2.sum(-1))                                                                # :96, :145, :175
            keep = upb - 1 if (mutation == "last_unit_dropped" and upb > 1) else upb
            colsum = rnd(sum(rnd(g2[:, k * ur:(k + 1) * ur].sum(1)) for k in range(keep)))           # :190, :153; :246
            cdiv = C if mutation == "col_mean_over_cols" else R
            if mutation == "eps_inside_c2":
                rm, cm = c2 * (rowsum / C + eps1), c2 * (colsum / cdiv + eps1)
            else:
                rm, cm = c2 * rowsum / C + eps1, c2 * colsum / cdiv + eps1
            row = rnd(b2 * St[i]["row"].double().reshape(nb, R) + omb * rm)                         # :230-231
            col = rnd(b2 * St[i]["col"].double().reshape(nb, C) + omb * cm)                         # :247-248
            rmean = rnd(row.mean() if mutation == "rfac_all_batches" else row.mean(-1, keepdim=True))   # :235-236
            rfac = rnd(torch.rsqrt(row / rmean))                                                    # :237
            cfac = rnd(torch.rsqrt(col))                                                            # :249
            u = rnd(c * g3 * rfac[:, :, None] * cfac[:, None, :])                                   # :304-306
            usq, n = (u * u).sum(), nb * R * C
            if mutation == "rms_one_chunk":
                if C % 4 == 0:
                    first = u[0].reshape(-1)[:CHUNK]
                else:
                    first = u[0, :ur].reshape(-1)
                usq, n = (first * first).sum(), first.numel()
            out[("row", i)], out[("col", i)] = row.reshape(s[:-1]), col.reshape(s[:-2] + s[-1:])
            u = u.reshape(s)
        else:
            n = g.numel()
            gc = rnd(g * (1.0 if mutation == "vec_unclipped" else c))                               # :264
            inner = c2 * (g * g + eps1) if mutation == "eps_inside_c2" else gc * gc + eps1
            sq = rnd(b2 * St[i]["sq"].double() + omb * inner)                                       # :265-266
            u = rnd(rnd(g * c) * torch.rsqrt(sq))                                                   # :267, :275
            usq = (u * u).sum()
            out[("sq", i)] = sq
        rms = rnd(torch.sqrt(rnd(usq) / n))                                                         # :353, :409, :271
        scale = rnd(lr / torch.clamp(rnd(rms / thr), min=1.0))                                      # :354, :410, :272
        if mutation == "decay_after_update":
            out[("p", i)] = rnd((p - scale * u) * decay)
        else:
            out[("p", i)] = rnd(rnd(p * decay) - rnd(scale * u))                                    # :371, :427, :276
        aux["u"][i], aux["scale"][i], aux["rms"][i], aux["decay"][i] = u, scale, rms, decay
    out["aux"] = aux
    return out


def exact(o):
    return _step(o, lambda v: v)


def emulate(o, mutation=None):
    out = _step(o, r32, mutation)
    del out["aux"]
    return out


def outputs(o):
    keys = ["grad_norm", "coef"]
    for i, s in enumerate(o["shapes"]):
        keys += [("p", i)] + ([("row", i), ("col", i)] if len(s) >= 2 else [("sq", i)])
    return keys


def bound(o, ref):
    """{output key: per-element bound} for the exact result `ref` (the derivation is in the module docstring)."""
    shapes = o["shapes"]
    pl = plan(shapes)
    lr, thr, mn = f32(o["lr"]), f32(o["clip_threshold"]), f32(o["max_grad_norm"])
    U, V = pl["units_plus_vecs"]
    d_all = _cdiv(U, 256) + _cdiv(V, 256) + 10
    dep = []
    for i, s in enumerate(shapes):
        ln, form = pl["lens"][i], pl["forms"][i]
        if form == "1-D":
            d = 1 + ln["trips"] + 10
            dep.append({"unit": d, "usq": d})
            continue
        C, rpw, upb, nun = s[-1], ln["rows_per_wave"], ln["units_per_item"], ln["units"]
        if form == "narrow":
            d_row = 1 + C
            dep.append({"row": d_row, "unit": d_row + rpw + 10, "col": 1 + rpw + 10 + upb,
                        "usq": 1 + rpw * C + 10 + _cdiv(nun, 256) + 10})
        else:
            d_row = 1 + 2 + ln["nseg"] + 6
            usq = (1 + 4 * ln["nseg"] * rpw + 10 + _cdiv(nun, 256) + 10 if form == "ragged-wide"
                   else 1 + 2 + 16 + 10 + _cdiv(ln["chunks"], 256) + 10)
            dep.append({"row": d_row, "unit": d_row + rpw + 2, "col": 1 + rpw + 2 + upb, "usq": usq})
    e_S = (max(d["unit"] for d in dep) + d_all) * F
    e_n = e_S / 2 + 2 * F
    norm, coef, a = ref["grad_norm"], ref["coef"], ref["aux"]
    B = {"grad_norm": norm * e_n}
    if mn > 0:
        e_x = e_n + 3 * F
        b_c = a["x"] * e_x if float(a["x"]) * (1 - e_x) < 1.0 else torch.zeros((), dtype=torch.float64)
    else:
        b_c = torch.zeros((), dtype=torch.float64)
    B["coef"] = b_c
    e_c = float(b_c / coef)
    e_c2 = 2 * e_c + F
    for i, s in enumerate(shapes):
        d = dep[i]
        wd = f32(o["weight_decay"]) if o["decay"][i] else 0.0
        if len(s) >= 2:
            e_row, e_col = e_c2 + (d["row"] + 7) * F, e_c2 + (d["col"] + 7) * F
            B[("row", i)], B[("col", i)] = ref[("row", i)] * e_row, ref[("col", i)] * e_col
            e_u = (e_row + (_cdiv(s[-2], 256) + 10) * F / 2 + 4 * F) + (e_col / 2 + 2 * F) + e_c + 3 * F
        else:
            e_sq = 2 * e_c + 8 * F
            B[("sq", i)] = ref[("sq", i)] * e_sq
            e_u = e_c + e_sq / 2 + 4 * F
        e_rms = (2 * e_u + d["usq"] * F + 4 * F) / 2 + 2 * F
        e_scale = 2 * F + (e_rms + 2 * F if float(a["rms"][i]) / thr * (1 + e_rms + 2 * F) > 1.0 else 0.0)
        p, su = o["params"][i].double(), (a["scale"][i] * a["u"][i]).abs()
        B[("p", i)] = p.abs() * F * (wd * lr + 1) + F * (p * a["decay"][i]).abs() + su * (e_scale + e_u + F) + F * ref[("p", i)].abs()
    return B


def ratios(o, ref, out, bnd=None):
    """{output key: worst |out - ref| / bound}"""
    bnd = bound(o, ref) if bnd is None else bnd
    return {k: worst_ratio((out[k].double().reshape(ref[k].shape) - ref[k]).abs(), bnd[k]) for k in outputs(o)}


def by_kind(rt):
    """worst ratio per kind of output: grad_norm, coef, p, row, col, sq"""
    w = {}
    for k, r in rt.items():
        kind = k if isinstance(k, str) else k[0]
        w[kind] = max(w.get(kind, 0.0), r)
    return w


def old_params_pass(o, ref, out):
    """the parameters-only comparison of tests/test_gpu_kernels.py at its limits"""
    return all(bool(((out[("p", i)] - ref[("p", i)]).abs() <= OLD_ATOL + OLD_RTOL * ref[("p", i)].abs()).all())
               for i in range(len(o["shapes"])))


# ------------------------------------------------------------------------------------------------------------ cases
# The smallest shapes at which each branch of af_stats / af_finalize / the update kernels can still go wrong.  `gnorm`: the global
# gradient norm per step (the generated gradients are rescaled to it), against max_grad_norm 1: above = the clip is active.
# `gscale`: the gradients' own scale, no rescale.  Every plan mixes decayed and undecayed tensors (`decay_of`).
STEPS = 3
LRS = (5e-3, 1e-2, 7.5e-3)
ACTIVE, INACTIVE, GROWING = (3.0, 7.0, 2.0), (0.3, 0.6, 0.45), (3.0, 12.0, 48.0)


def _case(name, shapes, grad="gauss", gnorm=None, gscale=1.0, max_grad_norm=1.0, clip_threshold=1.0, eps1=1e-30,
          weight_decay=0.01, group_floats=None, big=False):
    return {"name": name, "shapes": [tuple(s) for s in shapes], "grad": grad, "gnorm": gnorm, "gscale": gscale,
            "max_grad_norm": max_grad_norm, "clip_threshold": clip_threshold, "eps1": eps1, "weight_decay": weight_decay,
            "group_floats": group_floats, "big": big}


GROUP_SHAPES = [(64, 256), (33, 7), (130, 260), (7,), (5, 3, 9), (65, 260), (3, 24), (40,)]
SMALL_GROUP_FLOATS = 20000         # (3, 24) + (65, 260) | (130, 260), alone above the limit | (64, 256) + the 1-D tensors
ZERO_SHAPES = [(24, 40), (3, 8, 24), (33, 7), (7,), (20, 30), (256,), (2, 70, 5)]

CASES = [
    _case("vec4-small", [(1, 4), (3, 24), (7,), (64, 256), (65, 260), (1,), (130, 260), (2, 3, 8, 24)], gnorm=ACTIVE),
    _case("vec4-edges", [(4097, 4), (300, 8), (256,), (5, 1284), (3, 3072), (257,)], grad="scaled", gnorm=INACTIVE,
          clip_threshold=0.5, weight_decay=0.1),
    _case("wide-rows", [(16, 4096), (70, 3076), (3072,), (3, 24)], gnorm=GROWING, max_grad_norm=0.0),
    _case("narrow", [(33, 7), (5, 3, 9), (2, 300, 5), (7,), (6600, 5), (40, 1), (64, 256)], grad="scaled", gnorm=ACTIVE,
          weight_decay=0.1),
    _case("narrow-units", [(300, 64, 5), (1,), (3, 24)], gnorm=INACTIVE, clip_threshold=0.5),
    _case("ragged-wide", [(20, 30), (3, 70, 259), (200, 259), (257,), (70, 4095), (8, 12)], grad="scaled", gnorm=GROWING,
          max_grad_norm=0.0, clip_threshold=0.5),
    _case("all-ragged", [(33, 7), (9,), (5, 3, 9), (20, 30)], grad="scaled", gnorm=ACTIVE, clip_threshold=0.5),
    _case("no-1d", [(24, 40), (33, 7), (130, 260)], gnorm=INACTIVE, weight_decay=0.1),
    _case("eps1", [(130, 260), (65, 260), (64, 256), (40,), (2, 300, 5), (20, 30)], gscale=1e-2, eps1=1e-3, weight_decay=0.1),
    _case("eps1-no-clip", [(24, 40), (5, 3, 9), (40,), (3, 70, 259)], gscale=1e-2, eps1=1e-3, max_grad_norm=0.0, clip_threshold=0.5),
    _case("growing", [(24, 40), (40,), (16, 4)], gnorm=GROWING, max_grad_norm=0.0, clip_threshold=0.5),
    _case("batched", [(4, 24, 40), (2, 3, 8, 24), (5, 3, 9), (40,)], grad="scaled", gnorm=INACTIVE),
    _case("zeros", ZERO_SHAPES, grad="zeros", gnorm=ACTIVE),
    _case("zeros-no-clip", ZERO_SHAPES, grad="zeros", gnorm=INACTIVE, max_grad_norm=0.0, eps1=1e-3, clip_threshold=0.5),
    _case("all-zero", ZERO_SHAPES, grad="allzero"),
    _case("groups", GROUP_SHAPES, grad="scaled", gnorm=ACTIVE, group_floats=SMALL_GROUP_FLOATS),
    _case("many-chunks", [(8, 64), (4100, 1280), (1280,), (257, 516)], gnorm=ACTIVE, big=True),
]
CASE_IDS = [c["name"] for c in CASES]


def decay_of(shapes):
    """decayed and undecayed tensors of both kinds in every plan"""
    return [i % 3 != 1 for i in range(len(shapes))]


def _pow2(n, gen):
    """n powers of two spread over 2^-6 .. 2^6"""
    return 2.0 ** torch.randint(-6, 7, (n,), generator=gen).float()


def grads_for(case, step):
    """The gradients of step `step` (1-based), fp32, deterministic in (case, step)."""
    gen = torch.Generator().manual_seed(7919 * step + sum(ord(ch) for ch in case["name"]))
    gs = []
    for i, s in enumerate(case["shapes"]):
        g = torch.randn(*s, generator=gen)
        if case["grad"] == "scaled":
            if len(s) >= 2:
                nb = math.prod(s[:-2])
                g = (g.reshape(nb, s[-2], s[-1]) * _pow2(nb, gen)[:, None, None] * _pow2(s[-2], gen)[None, :, None]
                     * _pow2(s[-1], gen)[None, None, :]).reshape(s)
            else:
                g = g * _pow2(s[0], gen)
        elif case["grad"] == "zeros":
            if len(s) >= 2:
                g[..., ::3, :] = 0.0                                    # rows 0, 3, 6, ... of every batch item
                g[..., :, 1::4] = 0.0                                   # columns 1, 5, 9, ...
                if len(s) >= 3:
                    g[0] = 0.0                                          # a whole batch item
            else:
                g[::2] = 0.0
            if i in (0, 5):
                g.zero_()                                               # a whole factored tensor, a whole 1-D tensor
        elif case["grad"] == "allzero":
            g.zero_()
        gs.append(g * case["gscale"])
    if case["gnorm"] is not None:
        n = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
        gs = [g * (case["gnorm"][step - 1] / n) for g in gs]
    return gs


def initial(case):
    """fp32 parameters and a zero state, per tensor"""
    gen = torch.Generator().manual_seed(17 + sum(ord(ch) for ch in case["name"]))
    params = [torch.randn(*s, generator=gen) for s in case["shapes"]]
    state = [({"row": torch.zeros(s[:-1]), "col": torch.zeros(s[:-2] + s[-1:])} if len(s) >= 2 else {"sq": torch.zeros(s)})
             for s in case["shapes"]]
    return params, state


def operands(case, step, params, state):
    """What the kernel sees at step `step` (1-based) from `params` / `state` (the fp32 results of step - 1)."""
    return {"shapes": case["shapes"], "decay": decay_of(case["shapes"]), "params": params, "grads": grads_for(case, step),
            "state": state, "lr": LRS[step - 1], "beta2t": beta2t(step), "beta2t_prev": beta2t(max(step - 1, 1)),
            "eps1": case["eps1"], "clip_threshold": case["clip_threshold"], "max_grad_norm": case["max_grad_norm"],
            "weight_decay": case["weight_decay"]}


def carry(case, out):
    """(params, state) of the next step from a step's outputs (the kernel's own, or the emulation's): fp32"""
    params = [out[("p", i)].float().reshape(s) for i, s in enumerate(case["shapes"])]
    state = [({"row": out[("row", i)].float(), "col": out[("col", i)].float()} if len(s) >= 2 else {"sq": out[("sq", i)].float()})
             for i, s in enumerate(case["shapes"])]
    return params, state
