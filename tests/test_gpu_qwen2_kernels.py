"""GPU: the bias-taking forms of the three rotary kernels (Qwen2 / Qwen2.5 q|k|v projection bias; include/desta_hip.h,
desta_rope_bias / desta_rope_kv_append_bias / desta_rope_kv_append_e4m3_bias) held PER ELEMENT to float64.

The rule: the kernel reads bf16(x W^T), adds the fp32 bias, rotates q and k in fp32 and rounds once; v = bf16(v + b).

q, k: reference and bound are those tests/test_gpu_rowwise_fp64.py holds rope_k to, `rowwise_reference.OPS["rope"]` on the
      operand a + bias formed in float64 (exact: a bf16 plus an fp32 value of this magnitude fits 53 bits), asserted as
      |out - fp64| <= FACTOR x (S + 3 F (|a c| + |b s|)) with that file's FACTOR = 2.  The one fp32 rounding of a + bias the
      unbiased kernel does not have is F |a| |c| + F |b| |s| <= F (|a c| + |b s|): inside the factor (4 F < 2 x 3 F).
v:    |out - (v + b)| <= FACTOR x (S + F |v + b|): one fp32 add, one bf16 store.
Columns behind the heads (row padding up to ld) are compared bit for bit; so are cache slots outside [slot0, slot0 + seq).
e4m3: K bytes / scales = the host rule (`quantize_ref`: exact integer / power-of-two arithmetic, torch's CPU e4m3 cast) applied
      to the bf16 k the kernel left in place; V bytes / scales = the same rule applied to a float64 emulation of bf16(v + b)
      (sum in float64, rounded to fp32 as the kernel's add, then to bf16): "add bias, scale, round", independent of the kernel."""
import pytest
import torch

import rowwise_reference as R
from test_gpu_fp8_decode import quantize_ref
from test_gpu_rowwise_fp64 import FACTOR, GUARD, guarded, intact

pytestmark = pytest.mark.gpu

SHAPES = [(7, 1, 128), (4, 2, 64), (2, 2, 128)]
GRIDS = [(3, 5), (20, 4)]                       # (batch, rows per sequence): one block, and several with a ragged last one
PAD = 8                                         # row stride = heads + 8 columns the kernels must not touch


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _cos_sin(n, hd):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd))
    fr = torch.outer(torch.arange(n).float(), inv)
    return torch.stack([fr.cos(), fr.sin()], dim=1).contiguous()


def _inputs(Hq, Hkv, hd, B, S, zero_bias=False):
    g = torch.Generator().manual_seed(1000 * Hq + 100 * Hkv + hd + 7 * B + S)
    w = (Hq + 2 * Hkv) * hd
    ld = w + PAD
    qkv = torch.randn(B * S, ld, generator=g).bfloat16()
    bias = torch.randn(w, generator=g)
    k0 = Hq * hd
    idx = torch.randint(0, Hkv * hd, (5,), generator=g)
    bias[k0 + idx] = torch.tensor([30.0, -30.0, 30.0, -30.0, 30.0])          # the k-bias outliers of a real Qwen2.5 checkpoint
    if zero_bias:
        bias.zero_()
    shift = ((torch.arange(B) * 5) % 7 - 2).to(torch.int32)                  # non-zero per-row shift, some negative (clamped at 0)
    cs = _cos_sin(S + 16, hd)
    return ld, qkv, bias, shift, cs


def _check_heads(qkv, bias, out, Hq, Hkv, hd, S, cs, shift, smb, what):
    """q|k against rowwise_reference's rope, v against v + b, padding bit for bit -> prints the worst error / bound ratios"""
    w, nqk = (Hq + 2 * Hkv) * hd, (Hq + Hkv) * hd
    x = qkv.double()
    x[:, :w] += bias.double()[None]
    o = dict(buf=x, hd=hd, n_q=Hq, n_kv=Hkv, cos_sin=cs, seq=S, pos_shift=shift, s_major_batch=smb, backward=False)
    ref = R.OPS["rope"].exact(o)
    got = out.double()
    r_qk = R.worst_ratio((got - ref["out"]).abs()[:, :nqk], R.OPS["rope"].bound(o, ref, "out", got)[:, :nqk])
    v_ref, v_got = x[:, nqk:w], got[:, nqk:w]
    r_v = R.worst_ratio((v_got - v_ref).abs(), R.S(v_got, v_ref) + R.F * v_ref.abs())
    print(f"\n{what} Hq={Hq} Hkv={Hkv} hd={hd} rows={qkv.shape[0]}: q|k {r_qk:.3f} v {r_v:.3f}", end="")
    assert r_qk <= FACTOR and r_v <= FACTOR, (what, r_qk, r_v)
    assert torch.equal(out[:, w:].view(torch.int16), qkv[:, w:].view(torch.int16)), "row padding touched"
    # the bias is really in: without it the reference is far outside the bound
    assert float((got[:, :w] - qkv.double()[:, :w]).abs().max()) > 1.0


@pytest.mark.parametrize("B,S", GRIDS)
@pytest.mark.parametrize("Hq,Hkv,hd", SHAPES)
@pytest.mark.parametrize("s_major", [False, True])
def test_rope_bias_in_place(hip, Hq, Hkv, hd, B, S, s_major):
    ld, qkv, bias, shift, cs = _inputs(Hq, Hkv, hd, B, S)
    full, buf = guarded((B * S, ld), torch.bfloat16)
    buf.copy_(qkv)
    smb = B if s_major else 0
    hip.rope(buf, ld, B * S, S, Hq, Hkv, hd, cs.cuda(), pos_shift=shift.cuda(), s_major_batch=smb, bias=bias.cuda())
    torch.cuda.synchronize()
    assert intact(full)
    _check_heads(qkv, bias, buf.cpu(), Hq, Hkv, hd, S, cs, shift, smb, "rope_bias")
    # without a shift: positions arange(S), the training call
    buf.copy_(qkv)
    hip.rope(buf, ld, B * S, S, Hq, Hkv, hd, cs.cuda(), s_major_batch=smb, bias=bias.cuda())
    torch.cuda.synchronize()
    _check_heads(qkv, bias, buf.cpu(), Hq, Hkv, hd, S, cs, None, smb, "rope_bias (no shift)")


def _caches(B, Smax, Hkv, hd):
    kvw = 2 * Hkv * hd
    f16, c16 = guarded((B, Smax, kvw), torch.bfloat16, fill=-3.0)
    c8 = torch.full((B, Smax, kvw), 0xAB, dtype=torch.uint8, device="cuda")
    sc = torch.full((B, Smax, 2 * Hkv), -7.0, dtype=torch.float32, device="cuda")
    return f16, c16, c8, sc


@pytest.mark.parametrize("B,S", GRIDS)
@pytest.mark.parametrize("Hq,Hkv,hd", SHAPES)
def test_rope_kv_append_bias(hip, Hq, Hkv, hd, B, S):
    ld, qkv, bias, shift, cs = _inputs(Hq, Hkv, hd, B, S)
    slot0, Smax = 3, S + 6
    nqk, w = (Hq + Hkv) * hd, (Hq + 2 * Hkv) * hd
    full, buf = guarded((B * S, ld), torch.bfloat16)
    buf.copy_(qkv)
    f16, c16, _, _ = _caches(B, Smax, Hkv, hd)
    hip.rope_kv_append(buf, ld, B * S, S, Hq, Hkv, hd, cs.cuda(), None, None, 1e-6, shift.cuda(), c16, c16.stride(0), c16.stride(1), slot0, bias=bias.cuda())
    torch.cuda.synchronize()
    assert intact(full) and bool((f16[-GUARD:] == -3.0).all())
    out, c16 = buf.cpu(), c16.cpu()
    _check_heads(qkv, bias, out, Hq, Hkv, hd, S, cs, shift, 0, "rope_kv_append_bias")
    # the cache holds the k | v bits left in place, at slots [slot0, slot0 + S) of the row's sequence; every other slot is as it was
    assert torch.equal(c16[:, slot0:slot0 + S].reshape(B * S, -1).view(torch.int16), out[:, Hq * hd:w].contiguous().view(torch.int16))
    rest = torch.ones(Smax, dtype=torch.bool)
    rest[slot0:slot0 + S] = False
    assert bool((c16[:, rest] == -3.0).all())


@pytest.mark.parametrize("B,S", GRIDS)
@pytest.mark.parametrize("Hq,Hkv,hd", [s for s in SHAPES if s[2] == 128])
def test_rope_kv_append_e4m3_bias(hip, Hq, Hkv, hd, B, S):
    ld, qkv, bias, shift, cs = _inputs(Hq, Hkv, hd, B, S)
    qkv[0, (Hq + Hkv) * hd:(Hq + Hkv + 1) * hd] = 0                           # a zero V head: after the bias it is not a zero head
    slot0, Smax = 3, S + 6
    nqk, w = (Hq + Hkv) * hd, (Hq + 2 * Hkv) * hd
    a, b = qkv.cuda(), qkv.cuda()
    _, c16, c8, sc = _caches(B, Smax, Hkv, hd)
    args = (cs.cuda(), None, None, 1e-6, shift.cuda())
    hip.rope_kv_append(a, ld, B * S, S, Hq, Hkv, hd, *args, c16, c16.stride(0), c16.stride(1), slot0, bias=bias.cuda())
    hip.rope_kv_append_e4m3(b, ld, B * S, S, Hq, Hkv, hd, *args, c8, c8.stride(0), c8.stride(1), sc, sc.stride(0), sc.stride(1), slot0, bias=bias.cuda())
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))              # q|k|v in place: the bits of the bf16 form (checked above)
    out, c8, sc = b.cpu(), c8.cpu(), sc.cpu()
    _check_heads(qkv, bias, out, Hq, Hkv, hd, S, cs, shift, 0, "rope_kv_append_e4m3_bias")
    k_bits = out[:, Hq * hd:nqk]                                              # K: the bf16 values a bf16 cache would hold
    v_emul = (qkv[:, nqk:w].double() + bias[nqk:].double()[None]).float().bfloat16()     # V: add bias (fp32), round (bf16)
    heads = torch.cat([k_bits, v_emul], dim=1).reshape(B * S * 2 * Hkv, hd).contiguous()
    q, s = quantize_ref(heads)                                                # scale (after the bias), round
    assert torch.equal(c8[:, slot0:slot0 + S].reshape(-1, hd), q.view(torch.uint8))
    assert torch.equal(sc[:, slot0:slot0 + S].reshape(-1), s)
    rest = torch.ones(Smax, dtype=torch.bool)
    rest[slot0:slot0 + S] = False
    assert bool((c8[:, rest] == 0xAB).all()) and bool((sc[:, rest] == -7.0).all())
    # the zero V head took the scale of its bias, not the all-zero head's scale of 1 with zero bytes
    zq, zs = quantize_ref(bias[nqk:nqk + hd].bfloat16()[None])
    assert float(sc[0, slot0, Hkv]) == float(zs[0]) and torch.equal(c8[0, slot0, Hkv * hd:(Hkv + 1) * hd], zq.view(torch.uint8)[0])


@pytest.mark.parametrize("Hq,Hkv,hd", SHAPES)
def test_zero_bias_gives_the_bias_free_kernels_bits(hip, Hq, Hkv, hd):
    B, S, slot0 = 20, 4, 3
    Smax = S + 6
    ld, qkv, bias, shift, cs = _inputs(Hq, Hkv, hd, B, S, zero_bias=True)
    cs, shift, bias = cs.cuda(), shift.cuda(), bias.cuda()
    for smb in (0, B):
        a, b = qkv.cuda(), qkv.cuda()
        hip.rope(a, ld, B * S, S, Hq, Hkv, hd, cs, pos_shift=shift, s_major_batch=smb)
        hip.rope(b, ld, B * S, S, Hq, Hkv, hd, cs, pos_shift=shift, s_major_batch=smb, bias=bias)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and not torch.equal(a.cpu().view(torch.int16), qkv.view(torch.int16))
    a, b = qkv.cuda(), qkv.cuda()
    _, ca, c8a, sa = _caches(B, Smax, Hkv, hd)
    _, cb, c8b, sb = _caches(B, Smax, Hkv, hd)
    hip.rope_kv_append(a, ld, B * S, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, ca, ca.stride(0), ca.stride(1), slot0)
    hip.rope_kv_append(b, ld, B * S, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, cb, cb.stride(0), cb.stride(1), slot0, bias=bias)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(ca.view(torch.int16), cb.view(torch.int16))
    if hd == 128:
        a, b = qkv.cuda(), qkv.cuda()
        hip.rope_kv_append_e4m3(a, ld, B * S, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c8a, c8a.stride(0), c8a.stride(1), sa, sa.stride(0), sa.stride(1), slot0)
        hip.rope_kv_append_e4m3(b, ld, B * S, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c8b, c8b.stride(0), c8b.stride(1), sb, sb.stride(0), sb.stride(1), slot0,
                                bias=bias)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(c8a, c8b) and torch.equal(sa, sb)
        assert not bool((c8a[:, slot0:slot0 + S] == 0xAB).all())


def test_bad_arguments_return_einval_and_launch_nothing(hip):
    Hq, Hkv, hd, B, S, slot0 = 2, 2, 128, 3, 5, 3
    Smax = S + 6
    ld, qkv, bias, shift, cs = _inputs(Hq, Hkv, hd, B, S)
    buf, cs, shift = qkv.cuda(), cs.cuda(), shift.cuda()
    bias_pad = torch.zeros(bias.numel() + 4, device="cuda")
    bias_pad[:-4] = bias
    bias = bias_pad[:-4]
    norm = torch.ones(hd, device="cuda")
    _, c16, c8, sc = _caches(B, Smax, Hkv, hd)
    st = (c16.stride(0), c16.stride(1))
    s8 = (sc, sc.stride(0), sc.stride(1))
    M = B * S
    bad = [
        ("q/k-norm", lambda: hip.rope(buf, ld, M, S, Hq, Hkv, hd, cs, norm, norm, bias=bias)),
        ("q/k-norm", lambda: hip.rope_kv_append(buf, ld, M, S, Hq, Hkv, hd, cs, norm, norm, 1e-6, shift, c16, *st, slot0, bias=bias)),
        ("q/k-norm", lambda: hip.rope_kv_append_e4m3(buf, ld, M, S, Hq, Hkv, hd, cs, norm, norm, 1e-6, shift, c8, *st, *s8, slot0, bias=bias)),
        ("head_dim", lambda: hip.rope(buf, ld, M, S, Hq, Hkv, 96, cs, bias=bias)),
        ("head_dim", lambda: hip.rope_kv_append_e4m3(buf, ld, M, S, 2 * Hq, 2 * Hkv, 64, cs, None, None, 1e-6, shift, c8, *st, *s8, slot0, bias=bias)),
        ("ld", lambda: hip.rope(buf, (Hq + Hkv) * hd, M, S, Hq, Hkv, hd, cs, bias=bias)),                 # a row that holds q|k only: the V heads would be out of it
        ("ld", lambda: hip.rope_kv_append_e4m3(buf, (Hq + Hkv) * hd, M, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c8, *st, *s8, slot0, bias=bias)),
        ("aligned", lambda: hip.rope(buf, ld, M, S, Hq, Hkv, hd, cs, bias=bias_pad[1:])),
        ("aligned", lambda: hip.rope_kv_append_e4m3(buf, ld, M, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c8, *st, *s8, slot0, bias=bias_pad[1:])),
        ("s_major_batch", lambda: hip.rope(buf, ld, M, S, Hq, Hkv, hd, cs, s_major_batch=4, bias=bias)),
        ("multiple of seq", lambda: hip.rope_kv_append(buf, ld, M, 4, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c16, *st, slot0, bias=bias)),
        ("cache", lambda: hip.rope_kv_append(buf, ld, M, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c16, st[0], Hkv * hd, slot0, bias=bias)),
        ("cache", lambda: hip.rope_kv_append(buf, ld, M, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c16, *st, -1, bias=bias)),
        ("cache", lambda: hip.rope_kv_append_e4m3(buf, ld, M, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c8, *st, None, 0, 0, slot0, bias=bias)),
    ]
    for name, call in bad:
        with pytest.raises(RuntimeError, match=name) as ei:
            call()
        assert "(-1)" in str(ei.value), name                                 # DESTA_EINVAL
    # a NULL bias reaches the entry point only directly (the binding routes bias=None to the bias-free kernel)
    assert hip._rope_bias(buf.data_ptr(), ld, M, S, Hq, Hkv, hd, cs.data_ptr(), 0, 0, 0, 0, 0, hip.stream()) == -1
    with pytest.raises(ValueError, match="backward"):
        hip.rope(buf, ld, M, S, Hq, Hkv, hd, cs, backward=True, bias=bias)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu().view(torch.int16), qkv.view(torch.int16))   # nothing was launched
    assert bool((c16 == -3.0).all()) and bool((c8 == 0xAB).all()) and bool((sc == -7.0).all())


def test_bias_free_cache_forms_reject_what_their_twins_reject(hip):
    """The six entry points share one argument check: rope_kv_append and rope_kv_append_e4m3 read the V heads out of `buf` and write
    kv_row_stride-spaced slots with or without a bias, so without one they return DESTA_EINVAL for the same calls."""
    Hq, Hkv, hd, B, S, slot0 = 2, 2, 128, 3, 5, 3
    Smax = S + 6
    ld, qkv, _, shift, cs = _inputs(Hq, Hkv, hd, B, S)
    buf, shift = qkv.cuda(), shift.cuda()
    cs_pad = torch.zeros(cs.numel() + 4, device="cuda")
    cs_pad[1:-3] = cs.reshape(-1)
    cs_off = cs_pad[1:-3]                                                    # the table one float into an aligned allocation
    cs = cs.cuda()
    _, c16, c8, sc = _caches(B, Smax, Hkv, hd)
    st = (c16.stride(0), c16.stride(1))
    s8 = (sc, sc.stride(0), sc.stride(1))
    M = B * S

    def bf16(ld=ld, seq=S, cs=cs, rs=st[1], slot0=slot0):
        hip.rope_kv_append(buf, ld, M, seq, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c16, st[0], rs, slot0)

    def e4m3(ld=ld, seq=S, cs=cs, rs=st[1], slot0=slot0):
        hip.rope_kv_append_e4m3(buf, ld, M, seq, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c8, st[0], rs, *s8, slot0)

    bad = [("multiple of seq", dict(seq=4)), ("ld", dict(ld=(Hq + Hkv) * hd)), ("cache", dict(rs=Hkv * hd)), ("cache", dict(slot0=-1)),
           ("aligned", dict(cs=cs_off))]
    for form in (bf16, e4m3):
        for name, kw in bad:
            with pytest.raises(RuntimeError, match=name) as ei:
                form(**kw)
            assert "(-1)" in str(ei.value), (form.__name__, name)            # DESTA_EINVAL
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu().view(torch.int16), qkv.view(torch.int16))   # nothing was launched
    assert bool((c16 == -3.0).all()) and bool((c8 == 0xAB).all()) and bool((sc == -7.0).all())
    bf16()
    buf.copy_(qkv)
    e4m3()
    torch.cuda.synchronize()
    assert not bool((c16[:, slot0:slot0 + S] == -3.0).all()) and not bool((c8[:, slot0:slot0 + S] == 0xAB).all())
    assert not bool((sc[:, slot0:slot0 + S] == -7.0).all())
