"""GPU: every `desta_orca_*` entry point (desta2.5-audio_amd/csrc/orca.hip) on its own against a plain float64 torch restatement of
the same operation, at the shipped shapes (LLM hidden 1024 / 2560 / 4096, gate width h / 4, Whisper d 1280, 1500 frames -> 375 local
tokens, 4 global tokens, 4 or 32 tapped layers) and at the edges of each kernel's structure.  Backward entry points are compared with
fp64 autograd of the restatement.

Where a kernel copies a rounding point of the reference on a bf16 model (cos / sin rounded to bf16 under `round_cos_sin`, the gate
rounded to bf16, `bf16(gate * cross)` before the add) the restatement rounds there too, so every comparison is element by element:
bf16 outputs within half a bf16 ulp of the fp64 value plus a bound on the kernel's fp32 arithmetic, fp32 outputs within that bound.
The fp32 bounds are worst-case summation bounds, (number of sequential additions) x 2^-24 x (sum of the magnitudes of the terms).
Results a kernel ADDS to its destination are checked on a pre-filled destination, with every element it must not touch bit-unchanged;
reductions with a fixed order must give bit-identical reruns."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F64, BF16 = torch.float64, torch.bfloat16
U = 2.0 ** -24                                        # fp32 unit roundoff


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bf(shape, gen, scale=1.0):
    return (scale * torch.randn(*shape, generator=gen)).to(BF16)


def _ulp(t):
    """bf16 ulp of |t| (t fp64), normal range."""
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -126))) - 7)


def _r(t):
    """Round fp64 values to bf16 (through fp32, exact for the products of bf16 values rounded here) and back to fp64."""
    return t.float().to(BF16).to(F64)


def _check(out, ref, slack, what, half_ulp=True):
    """Element-wise: |out - ref| <= (0.5 bf16 ulp if the output is bf16) + slack."""
    out, ref = out.detach().cpu().to(F64), ref.detach().to(F64)
    err = (out - ref).abs()
    bound = slack + (0.5 * _ulp(torch.maximum(out.abs(), ref.abs())) if half_ulp else 0.0)
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), float(err[bad].max()), float(bound[bad].min()),
                                 float((err / _ulp(ref)).max()))


# ------------------------------------------------------------------------------------------------ local tap mix
@pytest.mark.parametrize("taps,rows,d,spread", [(1, 37, 8, 1.0), (4, 2 * 1500, 1280, 1.0), (4, 300, 128, 40.0), (32, 64, 1280, 1.0),
                                                (32, 200, 128, 40.0), (4, 1000, 8, 3.0)])
def test_local_mix_fwd_bwd(taps, rows, d, spread):
    """out = sum_l softmax(w)_l x_l, d(layer weights) through the softmax Jacobian.  rows = 2 x 1500 frames at Whisper-large width;
    32 taps (every layer with orca_use_all_layers) fills the 32 accumulators of the backward; spread 40 saturates the softmax."""
    from desta import _hip as H
    g = _gen(100 + taps * 7 + d)
    x = _bf((taps, rows, d), g)
    w = spread * torch.randn(taps, generator=g)
    xd, wd = x.cuda(), w.cuda()
    out = torch.empty(rows, d, dtype=BF16, device="cuda")
    H.orca_local_mix(xd, wd, taps, rows, d, out)
    p = torch.softmax(w.double(), 0)
    x64 = x.to(F64)
    ref = torch.einsum("l,lrd->rd", p, x64)
    f = (1.5 * (w.double() - w.double().max()).abs() + 16) * U         # softmax weight: __expf(w - max) to (1.5 |w - max| + a few) ulp
    mag = torch.einsum("l,lrd->rd", p * (f + taps * U), x64.abs())     # + taps fp32 adds
    _check(out, ref, mag, "local_mix")
    dout = _bf((rows, d), g)
    dw = torch.empty(taps, device="cuda")
    H.orca_local_mix_bwd(dout.cuda(), xd, wd, taps, rows, d, dw)
    dw2 = torch.empty(taps, device="cuda")
    H.orca_local_mix_bwd(dout.cuda(), xd, wd, taps, rows, d, dw2)
    assert torch.equal(dw, dw2)                                      # fixed-order reduction
    d64 = dout.to(F64)
    dots = torch.einsum("rd,lrd->l", d64, x64)
    A = torch.einsum("rd,lrd->l", d64.abs(), x64.abs())
    w64 = w.double().requires_grad_(True)
    (torch.softmax(w64, 0) * dots).sum().backward()
    n8 = rows * (d // 8)
    nadd = 8 * math.ceil(n8 / (256 * 256)) + 8 + 256                 # per-thread items, wave + block tree, 256 block partials in order
    e = nadd * U * A                                                 # bound on each fp32 dot
    mean = (p * dots).sum()
    slack = p * (e + (p * e).sum()) + p * f * (dots.abs() + mean.abs()) + p * (p * f * dots.abs()).sum() + 8 * U * w64.grad.abs()
    slack = slack + 2.0 ** -125                                      # softmax weights far below the largest underflow fp32
    _check(dw, w64.grad, slack, "local_mix_bwd", half_ulp=False)


# ------------------------------------------------------------------------------------------------ whole-vector rotation
def _rope_cs(T, Hd, theta, scale, round_cs):
    """cos / sin of the kernel's fp32 angle (t / scale) * theta^e, e = fp32(-c / half), in fp64, rounded to bf16 under round_cs, and how
    far the kernel's may be from them: its fp32 powf / cosf / sinf are allowed an angle error of 64 fp32 ulp, which moves cos / sin by
    |sin| / |cos| times that, plus one bf16 ulp where a rounding near a midpoint goes the other way."""
    half = Hd // 2
    t32 = torch.arange(T, dtype=torch.float32) / scale
    e32 = -(torch.arange(half, dtype=torch.float32) / half)
    inv32 = (float(theta) ** e32.to(F64)).float()
    ang = (t32[:, None] * inv32[None, :]).to(F64)
    dang = 64 * U * ang.abs() + 1e-7
    cs, sn = torch.cos(ang), torch.sin(ang)
    dcs, dsn = sn.abs() * dang + dang ** 2 + 4 * U, cs.abs() * dang + dang ** 2 + 4 * U
    if round_cs:
        cs, sn = _r(cs), _r(sn)
        dcs, dsn = dcs + _ulp(cs), dsn + _ulp(sn)
    return cs, sn, dcs, dsn


@pytest.mark.parametrize("B,T,Hd,scale,round_cs", [(3, 10, 256, 2.5, True), (3, 10, 256, 2.5, False), (2, 379, 2560, 2.5, True),
                                                   (2, 379, 2560, 1.0, False), (1, 1500, 4096, 2.5, True), (1, 1500, 4096, 1.0, True)])
def test_rope_fwd_bwd(B, T, Hd, scale, round_cs):
    """y = (x1 cos - x2 sin, x1 sin + x2 cos) over the whole vector; its transpose split at n_first into two destinations it ADDS to;
    the adjoint identity <rope(x), dy> = <x, rope_bwd(dy)> between the two kernels.  T = 379 = 4 global + 375 local tokens."""
    from desta import _hip as H
    theta = 10000.0
    g = _gen(T + Hd)
    half = Hd // 2
    x = _bf((B, T, Hd), g)
    y = torch.empty(B * T, Hd, dtype=BF16, device="cuda")
    H.orca_rope(x.cuda(), y, B, T, Hd, theta, scale, round_cos_sin=round_cs)
    cs, sn, dcs, dsn = _rope_cs(T, Hd, theta, scale, round_cs)
    x64 = x.to(F64)
    x1, x2 = x64[..., :half], x64[..., half:]
    ref = torch.cat([x1 * cs - x2 * sn, x1 * sn + x2 * cs], -1)
    slack = torch.cat([x1.abs() * dcs + x2.abs() * dsn, x1.abs() * dsn + x2.abs() * dcs], -1) + 4 * U * torch.cat([(x1 * cs).abs() + (x2 * sn).abs(),
                                                                                     (x1 * sn).abs() + (x2 * cs).abs()], -1)
    _check(y.view(B, T, Hd), ref, slack, "rope")
    dy = torch.randn(B, T, Hd, generator=g)
    d1, d2 = dy.to(F64)[..., :half], dy.to(F64)[..., half:]
    full = torch.cat([d1 * cs + d2 * sn, -d1 * sn + d2 * cs], -1)                  # = R^T dy (fp64 autograd of the rotation below)
    xa = x64.clone().requires_grad_(True)
    (torch.cat([xa[..., :half] * cs - xa[..., half:] * sn, xa[..., :half] * sn + xa[..., half:] * cs], -1) * dy.to(F64)).sum().backward()
    assert float((xa.grad - full).abs().max()) < 1e-12
    dslack = torch.cat([d1.abs() * dcs + d2.abs() * dsn, d1.abs() * dsn + d2.abs() * dcs], -1)
    for nf in sorted({0, 4, T}):
        pre0 = torch.randn(B, max(nf, 1), Hd, generator=g)
        pre1 = torch.randn(B, max(T - nf, 1), Hd, generator=g)
        o0, o1 = pre0.cuda(), pre1.cuda()
        H.orca_rope_bwd(dy.cuda(), B, T, Hd, theta, scale, round_cs, nf, o0, o1)
        for o, pre, sl in ((o0, pre0, slice(0, nf)), (o1, pre1, slice(nf, T))):
            if sl.stop == sl.start:
                assert torch.equal(o.cpu(), pre), nf                                  # the empty side is not touched
                continue
            want = pre.to(F64) + full[:, sl]
            _check(o, want, dslack[:, sl] + 4 * U * (pre.abs().to(F64) + full[:, sl].abs() + dslack[:, sl]), f"rope_bwd n_first={nf}",
                   half_ulp=False)
    # adjoint identity (both kernels, the same cos / sin): only y's bf16 output rounding and fp32 arithmetic separate the two sides
    z = torch.zeros(B * T, Hd, device="cuda")
    H.orca_rope_bwd(dy.cuda(), B, T, Hd, theta, scale, round_cs, 0, None, z)
    y64 = y.cpu().to(F64).view(B, T, Hd)
    lhs, rhs = float((y64 * dy.to(F64)).sum()), float((x64 * z.cpu().to(F64).view(B, T, Hd)).sum())
    bound = float((dy.to(F64).abs() * 0.5 * _ulp(y64)).sum()) + 8 * U * float((x64.abs() * z.cpu().to(F64).abs().view(B, T, Hd)).sum()) + 1e-9
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ------------------------------------------------------------------------------------------------ gate + residual and its backward
@pytest.mark.parametrize("M,Hd,ld_extra", [(1, 256, 0), (3, 1024, 8), (37, 2600, 0), (63, 2560, 64), (64, 4096, 0), (65, 2600, 16),
                                           (4100, 1024, 0)])
def test_gate_residual_fwd_bwd(M, Hd, ld_extra):
    """hs += bf16(bf16(sigmoid(g1 . w2 + b2)) * cross) in place (row stride ld >= H), then the backward pieces: d_cross, the pre-sigmoid
    gate gradient, and the gate MLP's d_preact, d_w2, d_b2 (64 fixed row slices: M < 64 leaves slices empty; column blocks of 64,
    H = 2600 gives a gate width of 650, not a multiple of 64)."""
    from desta import _hip as H
    Hq, ld = Hd // 4, Hd + ld_extra
    g = _gen(M * 3 + Hd)
    hs = _bf((M, ld), g)
    c = _bf((M, Hd), g)
    pre = _bf((M, Hq), g, 1.5)
    g1 = F.gelu(pre.float()).to(BF16)                                  # what the GEMM's GELU epilogue hands on
    w2 = torch.randn(Hq, generator=g) * (3.0 / math.sqrt(Hq))
    b2 = torch.tensor([0.1])
    hsd, gate = hs.cuda(), torch.empty(M, device="cuda")
    H.orca_gate_residual(hsd, ld, c.cuda(), g1.cuda(), w2.cuda(), b2.cuda(), M, Hd, Hq, gate_out=gate)
    z = g1.to(F64) @ w2.double() + float(b2)
    gref = torch.sigmoid(z)
    A = g1.to(F64).abs() @ w2.double().abs() + abs(float(b2))
    # dot: Hq / 64 lane adds + 6 shuffle levels; sigmoid: __expf of z to ~(|z| + 2) ulp, add, divide
    dg = 0.25 * (Hq / 64 + 8) * U * A + gref * (1 - gref) * (z.abs() + 4) * 2 * U + 2 * U
    _check(gate, gref, dg, "gate", half_ulp=False)
    gate_c = gate.cpu()
    # the bf16 arithmetic of the reference: exact for the kernel's own gate, and for any gate the rounding point can flip to
    out = hsd.cpu()
    assert torch.equal(out[:, Hd:], hs[:, Hd:])                       # row padding untouched
    ok = torch.zeros(M, Hd, dtype=torch.bool)
    for gc in (_r(gref - dg), _r(gref), _r(gref + dg)):
        cand = (hs[:, :Hd].float() + (gc[:, None] * c.to(F64)).float().to(BF16).float()).to(BF16)
        ok |= out[:, :Hd] == cand
    assert bool(ok.all()), ("gate_residual", int((~ok).sum()))
    # backward: dc = gate * dxo, d(pre-sigmoid gate) = (dxo . c) gate (1 - gate)
    dxo = _bf((M, ld), g)
    dc, dg2 = torch.empty(M, Hd, dtype=BF16, device="cuda"), torch.empty(M, device="cuda")
    H.orca_gate_residual_bwd(dxo.cuda(), ld, c.cuda(), gate, M, Hd, dc, dg2)
    gv = gate_c.double()
    zz = torch.log(gv / (1 - gv)).requires_grad_(True)
    cc = c.to(F64).requires_grad_(True)
    (torch.sigmoid(zz)[:, None] * cc * dxo[:, :Hd].to(F64)).sum().backward()
    _check(dc, cc.grad, 2 * U * cc.grad.abs() + 1e-300, "gate_residual_bwd d_cross")
    Adc = (dxo[:, :Hd].to(F64).abs() * c.to(F64).abs()).sum(1)
    _check(dg2, zz.grad, (Hd / 64 + 8) * U * Adc * gv * (1 - gv) + 4 * U * zz.grad.abs(), "gate_residual_bwd d_gate_pre", half_ulp=False)
    # gate MLP: g2 = gelu(pre) . w2 + b2 with the forward's bf16 GELU output in the dot (straight through to pre)
    dg2_c = dg2.cpu()
    dpre, dw2, db2 = torch.empty(M, Hq, dtype=BF16, device="cuda"), torch.empty(Hq, device="cuda"), torch.empty(1, device="cuda")
    H.orca_gate_mlp_bwd(dg2, pre.cuda(), g1.cuda(), w2.cuda(), M, Hq, dpre, dw2, db2)
    again = (torch.empty_like(dpre), torch.empty_like(dw2), torch.empty_like(db2))
    H.orca_gate_mlp_bwd(dg2, pre.cuda(), g1.cuda(), w2.cuda(), M, Hq, *again)
    assert torch.equal(dpre, again[0]) and torch.equal(dw2, again[1]) and torch.equal(db2, again[2])   # fixed-order reduction
    p64 = pre.to(F64).requires_grad_(True)
    w64 = w2.double().requires_grad_(True)
    b64 = b2.double().requires_grad_(True)
    gel = F.gelu(p64)
    G1 = gel + (g1.to(F64) - gel).detach()
    ((G1 @ w64 + b64) * dg2_c.double()).sum().backward()
    dgw = (dg2_c.double()[:, None] * w2.double()[None, :]).abs()
    _check(dpre, p64.grad, 4e-6 * dgw, "gate_mlp_bwd d_preact")          # gelu'(x) in fp32 (erff, __expf) to ~4e-6
    nadd = math.ceil(math.ceil(M / 64) / 4) + 3 + 64                       # rows per lane of a slice, 4 lanes, 64 slices in order
    _check(dw2, w64.grad, (nadd + 1) * U * (dg2_c.double().abs() @ g1.to(F64).abs()) + 1e-300, "gate_mlp_bwd d_w2", half_ulp=False)
    _check(db2, b64.grad, nadd * U * dg2_c.double().abs().sum() + 1e-300, "gate_mlp_bwd d_b2", half_ulp=False)


# ------------------------------------------------------------------------------------------------ diversity / orthogonality losses
def _sims(x, y, eps=1e-12):
    return F.normalize(x, dim=-1, eps=eps) @ F.normalize(y, dim=-1, eps=eps).transpose(-1, -2)


def _sim_bounds(Hd, ny):
    """(bound on each computed similarity: fp32 dot over H and two norms, relative bound of the fp32 sums over j) for one kernel call."""
    return (Hd / 256 + 24) * U, (ny + 16) * U


@pytest.mark.parametrize("Kg,Hd", [(4, 256), (64, 1024), (128, 4096)])
def test_sim_loss_identity_fwd_bwd(Kg, Hd):
    """Diversity loss sum_ij (g_i . g_j / |g_i| |g_j| - [i == j])^2 and its gradient (the symmetric form: row i also appears as a y).
    Kg = 128 is the backward's shared-memory limit.  One row is all zero and one is below F.normalize's eps (x / eps there)."""
    from desta import _hip as H
    B = 2
    gen = _gen(Kg + Hd)
    x = torch.randn(B, Kg, Hd, generator=gen)
    x[0, 1] = 0.0
    x[1, Kg - 1] *= 0.5e-12 / math.sqrt(Hd)                               # |x| ~ eps / 2: x / eps keeps a projection-sized part
    x[1, 0] *= 1e-3                                                        # small, above eps
    x = x.to(BF16)
    x64 = x.to(F64)
    part = torch.empty(B * Kg, device="cuda")
    H.orca_sim_loss(x.cuda(), x.cuda(), None, B, Kg, Kg, Kg, Hd, True, part)
    part2 = torch.empty_like(part)
    H.orca_sim_loss(x.cuda(), x.cuda(), None, B, Kg, Kg, Kg, Hd, True, part2)
    assert torch.equal(part, part2)
    s = _sims(x64, x64) - torch.eye(Kg, dtype=F64)
    es, er = _sim_bounds(Hd, Kg)
    _check(part, (s ** 2).sum(-1).reshape(-1), (2 * s.abs() * es + es * es).sum(-1).reshape(-1) + er * (s ** 2).sum(-1).reshape(-1),
           "sim_loss identity", half_ulp=False)
    coef = 0.01 / (B * Kg * Kg)
    pre = torch.randn(B * Kg, Hd, generator=gen)
    dx = pre.cuda()
    H.orca_sim_loss_bwd(x.cuda(), None, Kg, x.cuda(), None, Kg, B, Kg, Kg, Hd, True, coef, dx)
    dx2 = pre.cuda()
    H.orca_sim_loss_bwd(x.cuda(), None, Kg, x.cuda(), None, Kg, B, Kg, Kg, Hd, True, coef, dx2)
    assert torch.equal(dx, dx2)
    xa = x64.clone().requires_grad_(True)
    (coef * ((_sims(xa, xa) - torch.eye(Kg, dtype=F64)) ** 2).sum()).backward()
    _check(dx, pre.double() + xa.grad.reshape(B * Kg, Hd), _sim_grad_slack(x64, x64, s, coef, 2, es, er, pre), "sim_loss_bwd identity",
           half_ulp=False)


def _sim_grad_slack(x64, y64, s, coef, mult, es, er, pre):
    """Majorant of the kernel's fp32 error on dx_i += 2 mult coef (v - (v . xh_i) xh_i) / |x_i|, v = sum_j s_ij yh_j, per element:
    the error of every s_ij carried through, the fp32 sums over j and over H, and the final add to the pre-filled value."""
    xn = x64.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    xh, yh = x64 / xn, y64 / y64.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    e = s.abs() * er + es
    emag = torch.einsum("bij,bjk->bik", e, yh.abs()) + e.sum(-1, keepdim=True) * xh.abs()
    vmag = torch.einsum("bij,bjk->bik", s.abs(), yh.abs()) + s.abs().sum(-1, keepdim=True) * xh.abs()
    c = 2 * mult * abs(coef) / xn
    g = c * (emag + (16 + x64.shape[-1] / 256) * U * vmag) + 2 * U * c * vmag
    return g.reshape(pre.shape) + 2 * U * pre.double().abs()


@pytest.mark.parametrize("Kg,Tl,Hd", [(4, 24, 256), (8, 101, 1024), (64, 375, 256), (4, 1500, 4096)])
def test_sim_loss_cross_fwd_bwd(Kg, Tl, Hd):
    """Global / local orthogonality: the model's two calls — global rows against the sampled local rows (y index), and the sampled local
    rows against the global ones (x index) — with the model's list (the reference's device `linspace` of 100 above 100 tokens).  Both
    destinations are pre-filled; local rows outside the sample stay bit-identical.  A sampled local row and a global row sit below eps."""
    from desta import _hip as H
    from desta.models.modeling_desta25 import OrcaHIP
    B = 2
    gen = _gen(Kg * Tl + Hd)
    o = OrcaHIP.__new__(OrcaHIP)
    o.dev, o._lidx = torch.device("cuda"), {}
    idx = o.local_index(Tl)
    ny = Tl if idx is None else idx.numel()
    ii = torch.arange(Tl) if idx is None else idx.cpu().long()
    gl = torch.randn(B, Kg, Hd, generator=gen)
    lo = torch.randn(B, Tl, Hd, generator=gen)
    gl[1, Kg - 1] *= 0.5e-12 / math.sqrt(Hd)
    lo[0, int(ii[ny // 2])] *= 0.5e-12 / math.sqrt(Hd)
    lo[1, int(ii[1])] = 0.0
    gl, lo = gl.to(BF16), lo.to(BF16)
    g64, l64 = gl.to(F64), lo.to(F64)
    gd, ld_ = gl.cuda(), lo.cuda()
    part = torch.empty(B * Kg, device="cuda")
    H.orca_sim_loss(gd, ld_, idx, B, Kg, ny, Tl, Hd, False, part)
    part2 = torch.empty_like(part)
    H.orca_sim_loss(gd, ld_, idx, B, Kg, ny, Tl, Hd, False, part2)
    assert torch.equal(part, part2)
    s = _sims(g64, l64[:, ii])
    es, er = _sim_bounds(Hd, ny)
    _check(part, (s ** 2).sum(-1).reshape(-1), ((2 * s.abs() * es + es * es).sum(-1) + er * (s ** 2).sum(-1)).reshape(-1), "sim_loss cross",
           half_ulp=False)
    co = 0.01 / (B * Kg * ny)
    pre_g, pre_l = torch.randn(B * Kg, Hd, generator=gen), torch.randn(B * Tl, Hd, generator=gen)
    outs = []
    for _ in range(2):
        dg, dl = pre_g.cuda(), pre_l.cuda()
        H.orca_sim_loss_bwd(gd, None, Kg, ld_, idx, Tl, B, Kg, ny, Hd, False, co, dg)
        H.orca_sim_loss_bwd(ld_, idx, Tl, gd, None, Kg, B, ny, Kg, Hd, False, co, dl)
        outs.append((dg.cpu(), dl.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    dg, dl = outs[0]
    ga, la = g64.clone().requires_grad_(True), l64.clone().requires_grad_(True)
    (co * (_sims(ga, la[:, ii]) ** 2).sum()).backward()
    _check(dg, pre_g.double() + ga.grad.reshape(B * Kg, Hd), _sim_grad_slack(g64, l64[:, ii], s, co, 1, es, er, pre_g), "sim_loss_bwd global",
           half_ulp=False)
    dl3, pre3, want3 = dl.view(B, Tl, Hd), pre_l.view(B, Tl, Hd), pre_l.double().view(B, Tl, Hd) + la.grad
    sl = _sim_grad_slack(l64[:, ii], g64, s.transpose(1, 2), co, 1, es, (Kg + 16) * U, pre3[:, ii].reshape(B * ny, Hd)).view(B, ny, Hd)
    _check(dl3[:, ii], want3[:, ii], sl, "sim_loss_bwd local", half_ulp=False)
    rest = torch.ones(Tl, dtype=torch.bool)
    rest[ii] = False
    assert torch.equal(dl3[:, rest], pre3[:, rest])                          # local rows outside the sample: untouched


# ------------------------------------------------------------------------------------------------ per-layer alignment loss
@pytest.mark.parametrize("Hd,padded", [(256, False), (2560, False), (1024, True)])
def test_align_fwd_bwd(Hd, padded):
    """1 - cos(mean_t audio_e, mean of hidden rows [s0, s1) of text row r_e) and its gradient ADDED in bf16 to those rows: a span of
    length 1, a full row, a span ending at S, two disjoint spans in one row; hidden with the model's strides (h, S h) or a padded row
    and batch stride (and other strides again for d_hidden); every element outside the spans bit-unchanged."""
    from desta import _hip as H
    S, T, R = 16, 10, 4
    spans = [(0, 3, 4), (1, 0, S), (2, 9, S), (0, 6, 9), (3, 1, 5)]
    n = len(spans)
    gen = _gen(Hd + int(padded))
    rs, bs = (Hd + 64, S * (Hd + 64) + 128) if padded else (Hd, S * Hd)
    drs, dbs = (Hd + 32, S * (Hd + 32) + 64) if padded else (Hd, S * Hd)
    a = _bf((n, T, Hd), gen)
    buf = _bf((R * bs,), gen)
    hid = buf.as_strided((R, S, Hd), (bs, rs, 1))
    sp = torch.tensor(spans, dtype=torch.int32)
    out = torch.empty(n, device="cuda")
    H.orca_align(a.cuda(), T, buf.cuda(), rs, bs, Hd, sp.cuda(), n, out)
    am = a.to(F64).mean(1)
    tm = torch.stack([hid[r, s0:s1].to(F64).mean(0) for r, s0, s1 in spans])
    ref = 1 - (am * tm).sum(-1) / (am.norm(dim=-1) * tm.norm(dim=-1))
    eps = 4 * (T + S + Hd / 256 + 24) * U                                   # means, dots and norms in fp32 (cos relative to |a| |t|)
    _check(out, ref, torch.full((n,), eps), "align", half_ulp=False)
    # backward into a pre-filled bf16 gradient, of a magnitude where the added gradient shows
    coef = 0.05 / n * Hd
    h64 = hid.to(F64).clone().requires_grad_(True)
    tm_ = torch.stack([h64[r, s0:s1].mean(0) for r, s0, s1 in spans])
    (coef * (1 - (am * tm_).sum(-1) / (am.norm(dim=-1) * tm_.norm(dim=-1).clamp_min(1e-12))).sum()).backward()
    G = h64.grad
    dbuf = (torch.randn(R * dbs, generator=gen) * float(G[G != 0].abs().mean())).to(BF16)
    dd = dbuf.cuda()
    H.orca_align_bwd(a.cuda(), T, buf.cuda(), rs, bs, Hd, sp.cuda(), n, coef, dd, drs, dbs)
    got = dd.cpu()
    pre = dbuf.as_strided((R, S, Hd), (dbs, drs, 1)).to(F64)
    want = pre + G
    # the gradient element: coef (ma / |a| - cos mh / |t|) / |t| / len in fp32: relative to its two terms' magnitudes
    gmag = torch.zeros(R, S, Hd, dtype=F64)
    for e, (r, s0, s1) in enumerate(spans):
        an, tn = am[e].norm(), tm[e].norm()
        gmag[r, s0:s1] = coef * (am[e].abs() / an + tm[e].abs() / tn) / tn / (s1 - s0)
    _check(got.as_strided((R, S, Hd), (dbs, drs, 1)), want, eps * gmag + 2 * U * want.abs(), "align_bwd")
    touched = torch.zeros(R * dbs, dtype=torch.bool)
    tv = touched.as_strided((R, S, Hd), (dbs, drs, 1))
    for r, s0, s1 in spans:
        tv[r, s0:s1] = True
    assert torch.equal(got[~touched], dbuf[~touched])


# ------------------------------------------------------------------------------------------------ col2im of the strided Conv1d
@pytest.mark.parametrize("k,st,Tout,Tp,Hd,B", [(5, 4, 375, 1504, 256, 2), (5, 4, 375, 1504, 1024, 1), (3, 2, 50, 104, 128, 2),
                                               (3, 1, 60, 64, 64, 1), (2, 4, 40, 163, 128, 2), (1, 1, 30, 33, 8, 3)])
def test_col2im(k, st, Tout, Tp, Hd, B):
    """d(padded stream) from d(im2col rows) of the `as_strided` view the model builds (k = 5, stride 4 as shipped: windows overlap;
    k < stride leaves gaps; Tp past the last window leaves rows no window covers): WRITTEN, zero where no window reads."""
    from desta import _hip as H
    assert (Tout - 1) * st + k <= Tp
    gen = _gen(k * 100 + st + Hd)
    dcol = _bf((B, Tout, k * Hd), gen)
    dx = _bf((B, Tp, Hd), gen).cuda()                                       # stale values: every row is overwritten
    H.orca_col2im_add(dcol.cuda(), B, Tout, Tp, Hd, k, st, dx)
    xp = torch.zeros(B, Tp, Hd, dtype=F64, requires_grad=True)
    (xp.as_strided((B, Tout, k * Hd), (Tp * Hd, st * Hd, 1)) * dcol.to(F64)).sum().backward()
    xa = torch.zeros(B, Tp, Hd, dtype=F64, requires_grad=True)
    (xa.as_strided((B, Tout, k * Hd), (Tp * Hd, st * Hd, 1)) * dcol.to(F64).abs()).sum().backward()
    _check(dx, xp.grad, k * U * xa.grad, f"col2im k={k} stride={st}")
    none = xa.grad.abs().sum((0, 2)) == 0
    assert bool(none.any()) and bool((dx.cpu()[:, none] == 0).all())


# ------------------------------------------------------------------------------------------------ argument checks
def test_sim_loss_bwd_rejects_more_than_128_y_rows():
    from desta import _hip as H
    x = torch.zeros(1, 4, 64, dtype=BF16, device="cuda")
    y = torch.zeros(1, 129, 64, dtype=BF16, device="cuda")
    dx = torch.zeros(4, 64, device="cuda")
    with pytest.raises(RuntimeError, match="ny <= 128"):
        H.orca_sim_loss_bwd(x, None, 4, y, None, 129, 1, 4, 129, 64, False, 1.0, dx)
