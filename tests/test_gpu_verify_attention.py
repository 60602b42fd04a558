"""GPU: split-KV verify attention (desta_attention_verify, desta_attention_verify_kv8): seq_q = w = 2..8 query rows per sequence
under the forward kernel's causal rule, the G w <= 16 query rows of a KV head sharing every K / V byte.

Operands as `verify_step` passes them: Q at a column offset of a fused [B w, qkvw] buffer, K | V the halves of a [B, Smax, kvw] slab,
Smax > seq_k.  Shapes: G = 1, 2, 3, 4, 8 at w = 2..8 (R = G w from 2 to 16: every instantiation, R = 15 and 16 on the two-pass one),
seq_k from w to 5 CH + 3 with the rows' last visible keys on both sides of a chunk boundary, B = 1 and 3 with left pads.

1. per element against float64 (tests/verify_attention_reference.py), the bound and limits of tests/test_gpu_decode_attention.py:
   |out - ref| <= 0.5 ulp_bf16(max(|out|, |ref|)) + 2^-8 sum_j p_j |v_j|, rel-L2 < 8e-3, |lse - ref| <= 1e-4;
2. query row j equals desta_attention_decode{,_kv8} at seq_q = 1, seq_k - (w - 1 - j) keys, bit for bit in O and lse: the
   contract the speculative loop rests on (a masked key adds exp2(-inf) = 0, fma(0, v, acc) = acc);
3. the kv8 kernel equals the bf16 kernel on the dequantised cache bit for bit, also with per-(slot, head) scales 2^-6..2^6;
4. nothing beyond seq_k is used (NaN in the slots, their scales and the workspace);
5. reruns, a batch slice alone and another Smax give the same bits;
6. every rejection of the entry points, and the workspace size;
7. printed only: rel-L2 against float64 next to the forward kernel's at the same seq_q.
Measured (MI355X, chunk 256, profiles/r31_verify_attention_tests.log): worst |diff| / bound per group size 0.491 (G = 1), 0.495
(G = 2), 0.496 (G = 3), 0.497 (G = 4, also the query-spread-30 case at 0.495), 0.497 (G = 8); rel-L2 <= 1.8e-3 and 0.71-0.99 x the
forward kernel's on the same operands; |lse - ref| <= 1.2e-6, 2.4e-5 at spread 30; every bit test equal on every case."""
import copy

import pytest
import torch

from helpers import rel_err
from test_gpu_decode_attention import _bf16_ulp
from test_gpu_kv8_cache import pow2_spread, quantize_slab
from verify_attention_reference import verify_reference

pytestmark = pytest.mark.gpu

HD = 128
Q_OFF = 64                                                                   # Q starts at this column of the fused [B w, qkvw] buffer
SHAPES = [(2, 2, 2), (2, 2, 4), (2, 2, 8), (4, 2, 2), (4, 2, 8), (8, 2, 2), (8, 2, 3), (8, 2, 4), (8, 1, 2), (6, 2, 2), (6, 2, 5)]   # (Hq, Hkv, w)


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _seq_ks(CH, w):
    return [w, 63, CH - 1, CH, CH + 1, CH + w - 1, 2 * CH + 37, 5 * CH + 3]


class VCase:
    """One verify step's attention operands on the CPU (bf16) and, once asked for, on the device; the float64 reference once."""

    def __init__(self, B, Hq, Hkv, w, sk, kv_start, seed, spread=1.0, extra=9):
        g = torch.Generator().manual_seed(seed)
        self.B, self.Hq, self.Hkv, self.w, self.sk, self.Smax = B, Hq, Hkv, w, sk, sk + extra
        self.qkvw, self.kvw = Q_OFF + (Hq + 2 * Hkv) * HD, 2 * Hkv * HD
        self.qbuf = (torch.randn(B * w, self.qkvw, generator=g) * spread).bfloat16()
        self.cache = torch.randn(B, self.Smax, self.kvw, generator=g).bfloat16()
        self.kv = torch.tensor([int(k) for k in kv_start], dtype=torch.int32)
        self.scale = HD ** -0.5
        self.dev = self.ref = self.q8 = None

    def reference(self):
        """(out [B, w, Hq, 128], sum_j p_j |v_j|, lse [B, Hq, w] in the log2 domain), float64."""
        if self.ref is None:
            q = self.qbuf[:, Q_OFF:Q_OFF + self.Hq * HD].reshape(self.B, self.w, self.Hq, HD)
            k = self.cache[:, :self.sk, :self.Hkv * HD].reshape(self.B, self.sk, self.Hkv, HD)
            v = self.cache[:, :self.sk, self.Hkv * HD:].reshape(self.B, self.sk, self.Hkv, HD)
            self.ref = verify_reference(q, k, v, self.kv, self.scale)
        return self.ref

    def device(self):
        if self.dev is None:
            self.dev = (self.qbuf.cuda(), self.cache.cuda(), self.kv.cuda())
        return self.dev

    def quantised(self):
        """(bytes, scales) of the cache on the device, and a VCase on the DEQUANTISED cache."""
        if self.q8 is None:
            by, sc, deq = quantize_slab(self.cache)
            c = copy.copy(self)
            c.cache, c.ref, c.dev, c.q8 = deq, None, None, None
            self.q8 = (by.cuda(), sc.cuda(), c)
        return self.q8


def _desc(hip, c, q, cache, kv, out, lse, *, sq, sk, causal, Smax, q_bs, o_bs):
    kvw = 2 * c.Hkv * HD
    return hip.attn_desc(q, cache, cache, out, lse, batch=kv.shape[0], hq=c.Hq, hkv=c.Hkv, sq=sq, sk=sk, hd=HD, scale=c.scale, causal=causal,
                         kv_start=kv, q_off=Q_OFF, k_off=0, v_off=c.Hkv * HD, q_rs=c.qkvw, k_rs=kvw, v_rs=kvw, o_rs=c.Hq * HD,
                         q_bs=q_bs, k_bs=Smax * kvw, v_bs=Smax * kvw, o_bs=o_bs)


def _ws(n, fill=float("nan")):
    return torch.full((n // 4,), fill, dtype=torch.float32, device="cuda") if n else None


def _run(hip, c, *, rows=None, tensors=None, scales=None, ws_fill=float("nan"), old=False):
    """The verify kernel (scales: the kv8 one; old: the forward kernel) -> (O [B, w, Hq, 128] bf16, lse [B, Hq, w]) on the CPU."""
    qbuf, cache, kv = tensors if tensors is not None else c.device()
    if rows is not None:
        b0, b1 = rows
        qbuf, cache, kv = qbuf[b0 * c.w:b1 * c.w].contiguous(), cache[b0:b1].contiguous(), kv[b0:b1].contiguous()
        scales = None if scales is None else scales[b0:b1].contiguous()
    B, w = kv.shape[0], c.w
    out = torch.full((B * w, c.Hq * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, c.Hq, w), 7.0, dtype=torch.float32, device="cuda")
    d = _desc(hip, c, qbuf, cache, kv, out, lse, sq=w, sk=c.sk, causal=True, Smax=cache.shape[1], q_bs=w * c.qkvw, o_bs=w * c.Hq * HD)
    ws = _ws(hip.attention_verify_workspace_bytes(B, c.Hq, w, c.sk, HD), ws_fill)
    if old:
        hip.attention_fwd(d)
    elif scales is not None:
        hip.attention_verify_kv8(d, scales, scales[:, :, c.Hkv:], scales.stride(0), scales.stride(1), ws)
    else:
        hip.attention_verify(d, ws)
    torch.cuda.synchronize()
    return out.cpu().reshape(B, w, c.Hq, HD), lse.cpu()


def _run_one_row(hip, c, j, *, tensors=None, scales=None):
    """The one-row kernel on query row j of every sequence with seq_k - (w - 1 - j) keys -> (O [B, Hq, 128], lse [B, Hq])."""
    qbuf, cache, kv = tensors if tensors is not None else c.device()
    B, sk = c.B, c.sk - (c.w - 1 - j)
    out = torch.full((B, c.Hq * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, c.Hq, 1), 7.0, dtype=torch.float32, device="cuda")
    d = _desc(hip, c, qbuf[j:], cache, kv, out, lse, sq=1, sk=sk, causal=False, Smax=cache.shape[1], q_bs=c.w * c.qkvw, o_bs=c.Hq * HD)
    ws = _ws(hip.attention_decode_workspace_bytes(B, c.Hq, sk, HD))
    if scales is not None:
        hip.attention_decode_kv8(d, scales, scales[:, :, c.Hkv:], scales.stride(0), scales.stride(1), ws)
    else:
        hip.attention_decode(d, ws)
    torch.cuda.synchronize()
    return out.cpu().reshape(B, c.Hq, HD), lse.cpu().reshape(B, c.Hq)


_CASES = {}


def _case(hip, Hq, Hkv, w, sk, B, spread=1.0):
    """The shared cases: built (and their reference computed, their cache quantised) once per module."""
    CH = hip.DECODE_ATTN_CHUNK
    key = (Hq, Hkv, w, sk, B, spread)
    if key not in _CASES:
        kv = [min(s, sk - w) for s in [5, CH + 9, 0][:B]]                    # every row of every sequence sees at least one key
        _CASES[key] = VCase(B, Hq, Hkv, w, sk, kv, seed=Hq * 1000 + Hkv * 100 + 17 * w + sk + B, spread=spread)
    return _CASES[key]


def _cases(hip, Hq, Hkv, w):
    CH = hip.DECODE_ATTN_CHUNK
    for sk in _seq_ks(CH, w):
        for B in (1, 3):
            yield _case(hip, Hq, Hkv, w, sk, B)
    if (Hq, Hkv, w) == (8, 2, 4):
        yield _case(hip, 8, 2, 4, CH + 3, 3, spread=30.0)                    # saturated softmax: query spread 30, R = 16, a chunk boundary inside the rows


# ---------------------------------------------------------------------------------------------------------------- 1, 7
@pytest.mark.parametrize("Hq,Hkv,w", SHAPES)
def test_verify_attention_vs_fp64(hip, Hq, Hkv, w):
    worst = 0.0
    for c in _cases(hip, Hq, Hkv, w):
        ref, absv, lse_ref = c.reference()
        assert bool(torch.isfinite(lse_ref).all())                           # every row sees a key
        out, lse = _run(hip, c)
        got = out.double()
        assert bool(torch.isfinite(got).all())
        bound = 0.5 * _bf16_ulp(torch.maximum(got.abs(), ref.abs())) + 2.0 ** -8 * absv
        frac = float(((got - ref).abs() / bound).max())
        l2 = rel_err(got, ref)
        dl = float((lse.double() - lse_ref).abs().max())
        worst = max(worst, frac)
        old, _ = _run(hip, c, old=True)                                      # printed only
        print(f"Hq {Hq} Hkv {Hkv} w {w} B {c.B} sk {c.sk:5d} kv_start {c.kv.tolist()}: max |diff| / bound {frac:.3f}  rel-L2 {l2:.2e} "
              f"(forward kernel {rel_err(old.double(), ref):.2e})  |dlse| {dl:.2e}")
        assert frac <= 1.0, (c.B, c.sk, frac)
        assert l2 < 8e-3, (c.B, c.sk, l2)
        assert dl <= 1e-4, (c.B, c.sk, dl)
    print(f"VERIFY_FP64 G {Hq // Hkv} w {w}: worst fraction of the per-element bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("kind", ["bf16", "kv8"])
@pytest.mark.parametrize("Hq,Hkv,w", SHAPES)
def test_row_j_equals_the_one_row_kernel(hip, Hq, Hkv, w, kind):
    CH = hip.DECODE_ATTN_CHUNK
    n = 0
    for c in _cases(hip, Hq, Hkv, w):
        if kind == "kv8":
            by, sc, cq = c.quantised()
            tensors = (c.device()[0], by, c.device()[2])
        else:
            sc, tensors = None, None
        out, lse = _run(hip, c, tensors=tensors, scales=sc)
        for j in range(w):
            o1, l1 = _run_one_row(hip, c, j, tensors=tensors, scales=sc)
            assert torch.equal(out[:, j], o1), (c.B, c.sk, j, (out[:, j].float() - o1.float()).abs().max())
            assert torch.equal(lse[:, :, j], l1), (c.B, c.sk, j)
            n += (c.sk - 1) // CH != (c.sk - (w - 1 - j) - 1) // CH          # the two kernels split the keys into different chunk counts
    assert n > 0


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("Hq,Hkv,w", SHAPES)
def test_kv8_equals_bf16_on_the_dequantised_cache(hip, Hq, Hkv, w):
    for c in _cases(hip, Hq, Hkv, w):
        by, sc, cq = c.quantised()
        o8, l8 = _run(hip, c, tensors=(c.device()[0], by, c.device()[2]), scales=sc)
        o16, l16 = _run(hip, cq)
        assert torch.equal(o8, o16) and torch.equal(l8, l16), (c.B, c.sk)
        assert rel_err(o8.double(), cq.reference()[0]) < 8e-3
        wide = pow2_spread(c.cache, seed=c.sk + w)                           # K and V of every (slot, head) times 2^-6..2^6
        by, sc, deq = quantize_slab(wide)
        o8, l8 = _run(hip, c, tensors=(c.device()[0], by.cuda(), c.device()[2]), scales=sc.cuda())
        o16, l16 = _run(hip, c, tensors=(c.device()[0], deq.cuda(), c.device()[2]))
        assert torch.equal(o8, o16) and torch.equal(l8, l16), (c.B, c.sk, "spread")
        assert float(sc.max() / sc.min()) >= 2.0 ** 8


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("kind", ["bf16", "kv8"])
def test_nothing_beyond_seq_k_is_used(hip, kind):
    CH = hip.DECODE_ATTN_CHUNK
    for Hq, Hkv, w, sk in ((8, 2, 4, CH - 1), (8, 2, 4, 2 * CH + 37), (6, 2, 5, CH + 2)):
        c = VCase(3, Hq, Hkv, w, sk, [5, min(CH + 9, sk - w), 0], seed=5 + sk)
        q, _, kv = c.device()
        if kind == "kv8":
            by, sc, deq = quantize_slab(c.cache)
            bad_b, bad_s = by.clone(), sc.clone()
            bad_b[:, sk:] = 0x7F                                             # e4m3fn NaN
            bad_s[:, sk:] = float("nan")
            zero_b, zero_s = by.clone(), sc.clone()
            zero_b[:, sk:] = 0
            zero_s[:, sk:] = 1.0
            o_nan, l_nan = _run(hip, c, tensors=(q, bad_b.cuda(), kv), scales=bad_s.cuda(), ws_fill=float("nan"))
            o_z, l_z = _run(hip, c, tensors=(q, zero_b.cuda(), kv), scales=zero_s.cuda(), ws_fill=0.0)
            ref = verify_reference(c.qbuf[:, Q_OFF:Q_OFF + Hq * HD].reshape(3, w, Hq, HD), deq[:, :sk, :Hkv * HD].reshape(3, sk, Hkv, HD),
                                   deq[:, :sk, Hkv * HD:].reshape(3, sk, Hkv, HD), c.kv, c.scale)[0]
        else:
            bad, zero = c.cache.clone(), c.cache.clone()
            bad[:, sk:] = float("nan")
            zero[:, sk:] = 0
            o_nan, l_nan = _run(hip, c, tensors=(q, bad.cuda(), kv), ws_fill=float("nan"))
            o_z, l_z = _run(hip, c, tensors=(q, zero.cuda(), kv), ws_fill=0.0)
            ref = c.reference()[0]
        assert bool(torch.isfinite(o_nan.float()).all()) and bool(torch.isfinite(l_nan).all())
        assert torch.equal(o_nan, o_z) and torch.equal(l_nan, l_z)
        assert rel_err(o_nan.double(), ref) < 8e-3


def test_rows_in_front_of_kv_start_see_nothing(hip):
    """kv_start = seq_k - 1 at w = 4: rows 0..2 of every sequence see no key (O = 0, lse = +inf), row 3 sees exactly one."""
    CH = hip.DECODE_ATTN_CHUNK
    for sk in (CH + 2, 37):                                                  # the one visible key in the second chunk; one chunk
        c = VCase(2, 8, 2, 4, sk, [sk - 1, sk - 1], seed=11 + sk)
        by, sc, deq = quantize_slab(c.cache)
        for scales, tensors in ((None, None), (sc.cuda(), (c.device()[0], by.cuda(), c.device()[2]))):
            out, lse = _run(hip, c, tensors=tensors, scales=scales)
            assert bool((out[:, :3] == 0).all()) and bool((lse[:, :, :3] == float("inf")).all())
            slab = c.cache if scales is None else deq
            want = slab[:, sk - 1, 2 * HD:].reshape(2, 2, HD).repeat_interleave(4, dim=1)       # the V row of the one visible key
            assert torch.equal(out[:, 3], want) and bool(torch.isfinite(lse[:, :, 3]).all())


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("kind", ["bf16", "kv8"])
@pytest.mark.parametrize("Hq,Hkv,w", [(8, 2, 4), (6, 2, 5), (2, 2, 8)])
def test_determinism_and_row_independence(hip, Hq, Hkv, w, kind):
    CH = hip.DECODE_ATTN_CHUNK
    c = _case(hip, Hq, Hkv, w, 5 * CH + 3, 3)                                # six chunks
    q, cache, kv = c.device()
    sc = None
    if kind == "kv8":
        cache, sc, _ = c.quantised()
    first, lse0 = _run(hip, c, tensors=(q, cache, kv), scales=sc)
    again, lse1 = _run(hip, c, tensors=(q, cache, kv), scales=sc)
    assert torch.equal(first, again) and torch.equal(lse0, lse1)
    for b in range(3):                                                       # each sequence alone at B = 1
        alone, lse_b = _run(hip, c, tensors=(q, cache, kv), scales=sc, rows=(b, b + 1))
        assert torch.equal(alone[0], first[b]) and torch.equal(lse_b[0], lse0[b]), b
    big = torch.full((3, c.Smax + 77, c.kvw), 0x7F if kind == "kv8" else float("nan"), dtype=cache.dtype, device="cuda")
    big[:, :c.sk] = cache[:, :c.sk]                                          # another Smax: another batch stride, another allocation
    big_sc = None
    if kind == "kv8":
        big_sc = torch.full((3, c.Smax + 77, 2 * Hkv), float("nan"), dtype=torch.float32, device="cuda")
        big_sc[:, :c.sk] = sc[:, :c.sk]
    moved, lse2 = _run(hip, c, tensors=(q, big, kv), scales=big_sc)
    assert torch.equal(moved, first) and torch.equal(lse2, lse0)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_rejections_and_workspace_size(hip):
    CH = hip.DECODE_ATTN_CHUNK
    c = VCase(2, 8, 2, 4, 2 * CH + 5, [0, 3], seed=6)
    qbuf, cache, kv = c.device()
    by, sc, _ = quantize_slab(c.cache)
    by, sc = by.cuda(), sc.cuda()
    out = torch.full((2 * 8, 16 * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((2, 16, 8), 7.0, dtype=torch.float32, device="cuda")
    other = torch.zeros(2, 16 * HD, dtype=torch.float32, device="cuda")
    need = hip.attention_verify_workspace_bytes(2, 8, 4, c.sk, HD)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")

    def desc(slab):
        return _desc(hip, c, qbuf, slab, kv, out, lse, sq=4, sk=c.sk, causal=True, Smax=c.Smax, q_bs=4 * c.qkvw, o_bs=4 * 8 * HD)

    def setter(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f
    bad = [("seq_q", setter(seq_q=1)), ("seq_q", setter(seq_q=9)), ("head_dim", setter(head_dim=64)), ("group", setter(n_q_heads=16, n_kv_heads=1, seq_q=2)),
           ("query rows per kv head", setter(seq_q=5)), ("causal", setter(causal=0)), ("dropout", setter(dropout_p=0.1)),
           ("rope_cos_sin", setter(rope_cos_sin=other.data_ptr())), ("O_f32", setter(O_f32=other.data_ptr())), ("dO", setter(dO=other.data_ptr())),
           ("dQ", setter(dQ=other.data_ptr())), ("O must be 16-byte aligned", setter(O=out.data_ptr() + 2)),
           ("O must be 16-byte aligned", setter(o_row_stride=8 * HD + 4)), ("Q, K, V must be 16-byte aligned", setter(K=cache.data_ptr() + 2)),
           ("Q, K, V must be 16-byte aligned", setter(q_batch_stride=4 * c.qkvw + 4))]
    launches = [lambda d, w_: hip.attention_verify(d, w_), lambda d, w_: hip.attention_verify_kv8(d, sc, sc[:, :, 2:], sc.stride(0), sc.stride(1), w_)]
    for kind, launch in enumerate(launches):
        slab = by if kind else cache
        for name, change in bad:
            d = desc(slab)
            change(d)
            with pytest.raises(RuntimeError, match=name):
                launch(d, ws[:need])
        with pytest.raises(RuntimeError, match="workspace"):                 # one byte short
            launch(desc(slab), ws[:need - 1])
        with pytest.raises(RuntimeError, match="workspace"):                 # misaligned
            launch(desc(slab), ws[4:need + 4])
        with pytest.raises(RuntimeError, match="workspace"):                 # none at all for rows of three chunks
            launch(desc(slab), None)
    with pytest.raises(RuntimeError, match="scale"):
        hip.attention_verify_kv8(desc(by), None, sc[:, :, 2:], sc.stride(0), sc.stride(1), ws[:need])
    with pytest.raises(RuntimeError, match="scale"):
        hip.attention_verify_kv8(desc(by), sc, sc[:, :, 2:], sc.stride(0), 0, ws[:need])
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all())             # nothing was launched
    # one partial per (sequence, head, query row, chunk): the one-row formula at n_q_heads * seq_q rows
    sizes = [hip.attention_verify_workspace_bytes(2, 8, 4, sk, HD) for sk in (CH, CH + 1, 2 * CH, 2 * CH + 1, 3 * CH, 5 * CH + 3)]
    assert sizes[0] == 0 and 0 < sizes[1] == sizes[2] < sizes[3] == sizes[4] < sizes[5]
    assert sizes[5] * 2 == sizes[1] * 6 and need == sizes[3]
    for sk in (CH + 1, 3 * CH):
        items = 2 * 8 * 4 * ((sk + CH - 1) // CH)
        assert hip.attention_verify_workspace_bytes(2, 8, 4, sk, HD) == 4 * ((2 * items + 3) // 4 * 4 + HD * items) == hip.attention_decode_workspace_bytes(2, 32, sk, HD)
    hip.attention_verify(desc(cache), ws[:need])                             # what it reports is enough
    torch.cuda.synchronize()
    got = out.reshape(-1)[:2 * 4 * 8 * HD].cpu().reshape(2, 4, 8, HD)      # the descriptor's o_row_stride is 8 heads
    assert rel_err(got.double(), c.reference()[0]) < 8e-3
