"""GPU: the opt-in FP8 (e4m3) KV cache — the quantising rotary append (desta_rope_kv_append_e4m3), decode attention on the
byte cache (desta_attention_decode_kv8) and the model paths behind `set_kv_cache("fp8")`.

The scale of a head is a power of two, so q * s is exactly a bf16 value and the kv8 kernel is pinned WITHOUT a tolerance: on every
case of tests/test_gpu_decode_attention.py it must give the bits desta_attention_decode gives on the dequantised cache, O and
lse, with a NaN-filled workspace.  Independently of the bf16 kernel it is held to that file's per-element fp64 bound on the
dequantised operands.  The append must leave the q|k|v buffer desta_rope_kv_append leaves and write the bytes and scales the
host rule (tests/test_gpu_fp8_decode.py::quantize_ref, per head) gives on the bf16 cache rows, and nothing else.

Model (tiny Qwen3 geometry, G = 2 and G = 4, B = 3 with left pads, 12 forced tokens from the fp32 oracle): per-step logits rel-L2
against the oracle, worst over both prompts and both geometries — see KV8_WORST_MEASURED below for the measured numbers and
the bound that follows from them by the rule (the decode path's own 3e-2 / 0.1 when the FP8-cache worst is at most
2e-2, else 1.5 x the measured worst, never above 1e-1)."""
import copy
import math
import os

import pytest
import torch

import desta_oracle as O
from helpers import cfg_from_dims, rel_err
from test_gpu_decode_attention import HEADS, Case, _bf16_ulp, _seq_ks
from test_gpu_fp8_decode import dequant_bf16, quantize_ref

pytestmark = pytest.mark.gpu

HD = 128
Q_OFF = 64                                                                   # Case puts Q at this column of its [B, qkvw] buffer

# Worst per-step logits rel-L2 against the fp32 oracle over test_model_fp8_cache_vs_oracle's four runs, measured on an MI355X:
#   bf16 cache 6.5e-3 (gap / spread 0.000), FP8 cache 1.52e-2 (gap / spread 0.053); both worst values at the 13-token prompt,
#   where 13-24 keys share the softmax (at prompt 251 with pads 0 / 5 / 131: 6.0e-3 against 7.7e-3).  ORCA run: 9.2e-3, gap / spread 0.023.
# 1.52e-2 <= 2e-2, so the decode path's own bounds hold for the FP8 cache: rel-L2 < 3e-2, argmax gap / spread < 0.1.
KV8_WORST_MEASURED = 1.52e-2
REL_BOUND = 3e-2 if KV8_WORST_MEASURED <= 2e-2 else min(1.5 * KV8_WORST_MEASURED, 1e-1)
GAP_BOUND = 0.1


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def quantize_slab(cache):
    """bf16 [B, Smax, 2 Hkv 128] -> (e4m3 bytes as uint8, same shape; fp32 scales [B, Smax, 2 Hkv]; the dequantised bf16 slab),
    the host rule per head of 128 values."""
    B, Smax, kvw = cache.shape
    q, s = quantize_ref(cache.reshape(-1, HD).contiguous())
    return q.view(torch.uint8).reshape(B, Smax, kvw), s.reshape(B, Smax, kvw // HD), dequant_bf16(q, s).reshape(B, Smax, kvw)


def pow2_spread(cache, seed):
    """K and V of every (slot, head) times a power of two from 2^-6 to 2^6 (exact in bf16): scales differ inside one 16-key tile."""
    B, Smax, kvw = cache.shape
    g = torch.Generator().manual_seed(seed)
    e = torch.randint(-6, 7, (B, Smax, kvw // HD, 1), generator=g).float()
    return (cache.float().reshape(B, Smax, kvw // HD, HD) * torch.exp2(e)).reshape(B, Smax, kvw).bfloat16()


class Case8:
    """A Case of the bf16 file with its cache quantised: .c is a Case on the DEQUANTISED cache (reference() = fp64 on it)."""

    def __init__(self, base, spread_seed=None):
        cache = base.cache if spread_seed is None else pow2_spread(base.cache, spread_seed)
        self.bytes, self.scales, deq = quantize_slab(cache)
        self.base = base
        self.c = copy.copy(base)                                             # the unquantised case itself stays as it is
        self.c.cache, self.c.ref, self.c.dev = deq, None, None
        self.dev = None

    def device(self):
        if self.dev is None:
            self.dev = (self.c.qbuf.cuda(), self.bytes.cuda(), self.scales.cuda(), self.c.kv.cuda(), self.c.cache.cuda())
        return self.dev


def _desc(hip, c, qbuf, cache, kv, out, lse, Smax):
    B, kvw = qbuf.shape[0], 2 * c.Hkv * HD
    return hip.attn_desc(qbuf, cache, cache, out, lse, batch=B, hq=c.Hq, hkv=c.Hkv, sq=1, sk=c.sk, hd=HD, scale=c.scale, causal=False,
                         kv_start=kv, q_off=Q_OFF, k_off=0, v_off=c.Hkv * HD, q_rs=c.qkvw, k_rs=kvw, v_rs=kvw, o_rs=c.Hq * HD,
                         q_bs=c.qkvw, k_bs=Smax * kvw, v_bs=Smax * kvw, o_bs=c.Hq * HD)


def _workspace(hip, B, Hq, sk, fill=float("nan")):
    n = hip.attention_decode_workspace_bytes(B, Hq, sk, HD)
    return torch.full((n // 4,), fill, dtype=torch.float32, device="cuda") if n else None


def _outputs(B, Hq):
    return (torch.full((B, Hq * HD), 7.0, dtype=torch.bfloat16, device="cuda"), torch.full((B, Hq, 1), 7.0, dtype=torch.float32, device="cuda"))


def _run8(hip, c8, *, rows=None, tensors=None, ws_fill=float("nan")):
    """kv8 kernel -> (O [B, Hq, 128] bf16, lse [B, Hq]) on the CPU.  tensors: (bytes, scales) on the device, any Smax."""
    c = c8.c
    qbuf, by, sc, kv, _ = c8.device()
    if tensors is not None:
        by, sc = tensors
    if rows is not None:
        qbuf, by, sc, kv = qbuf[rows].contiguous(), by[rows].contiguous(), sc[rows].contiguous(), kv[rows].contiguous()
    B = qbuf.shape[0]
    out, lse = _outputs(B, c.Hq)
    d = _desc(hip, c, qbuf, by, kv, out, lse, by.shape[1])
    hip.attention_decode_kv8(d, sc, sc[:, :, c.Hkv:], sc.stride(0), sc.stride(1), _workspace(hip, B, c.Hq, c.sk, ws_fill))
    torch.cuda.synchronize()
    return out.cpu().reshape(B, c.Hq, HD), lse.cpu().reshape(B, c.Hq)


def _run16(hip, c8):
    """The bf16 split-KV kernel on the dequantised cache."""
    c = c8.c
    qbuf, _, _, kv, deq = c8.device()
    out, lse = _outputs(c.B, c.Hq)
    hip.attention_decode(_desc(hip, c, qbuf, deq, kv, out, lse, c.Smax), _workspace(hip, c.B, c.Hq, c.sk))
    torch.cuda.synchronize()
    return out.cpu().reshape(c.B, c.Hq, HD), lse.cpu().reshape(c.B, c.Hq)


_CASES8 = {}


def _case8(hip, Hq, Hkv, sk_i, B, spread=1.0):
    """The cases of tests/test_gpu_decode_attention.py (same seeds, same kv_start), quantised once per module."""
    CH = hip.DECODE_ATTN_CHUNK
    sk = _seq_ks(CH)[sk_i]
    key = (Hq, Hkv, sk, B, spread)
    if key not in _CASES8:
        kv = [5, CH + 9, 0] if B == 3 else [sk - 1]
        _CASES8[key] = Case8(Case(B, Hq, Hkv, sk, kv, seed=Hq * 1000 + Hkv * 100 + sk + B, spread=spread))
    return _CASES8[key]


def _all_cases8(hip):
    for Hq, Hkv in HEADS:
        for sk_i in range(7):
            for B in (1, 3):
                yield _case8(hip, Hq, Hkv, sk_i, B)
    yield _case8(hip, 8, 2, 5, 3, spread=30.0)


# ---------------------------------------------------------------------------------------------------------------- 1
def _cos_sin(n):
    inv = 1.0 / (10000.0 ** (torch.arange(0, HD, 2).float() / HD))
    fr = torch.outer(torch.arange(n).float(), inv)
    return torch.stack([fr.cos(), fr.sin()], dim=1).contiguous()


APPEND_CONFIGS = [(Hq, Hkv, norm, form) for form in ("prompt", "decode") for norm in (False, True) for Hq, Hkv in ((4, 2), (8, 1))]


def append_inputs(Hq, Hkv, norm, form):
    """-> (B, S, slot0, Smax, ld, qkv on the CPU, cos_sin, q-norm weight, k-norm weight, pos_shift on the device)"""
    B, S, slot0, Smax = (2, 5, 0, 9) if form == "prompt" else (3, 1, 7, 12)
    g = torch.Generator().manual_seed(Hq * 10 + Hkv + 2 * norm + S)
    nh, kvw = Hq + 2 * Hkv, 2 * Hkv * HD
    ld = nh * HD + 8                                                         # a row stride wider than the heads
    qkv = torch.randn(B * S, ld, generator=g).bfloat16()
    heads = qkv[:, :nh * HD].view(B * S, nh, HD)
    v0 = Hq + Hkv                                                            # first V head: V goes to the cache as stored, so values can be planted
    heads[0, Hq] = 0                                                         # an all-zero K head stays zero through the norm and the rotation
    sub = torch.zeros(HD, dtype=torch.int16)
    sub[5], sub[64] = 0x0008, -0x7FFD                                        # bf16 subnormals: 8 * 2^-133 and -(3 * 2^-133)
    heads[0, v0] = sub.view(torch.bfloat16)
    heads[1, v0] = (torch.rand(HD, generator=g) * 2 - 1).bfloat16()
    heads[1, v0, 17] = 448.0 * 2.0 ** -5                                     # amax exactly 448 * 2^-5: e = -5, q = 448
    heads[2, v0 + Hkv - 1] = (torch.rand(HD, generator=g) * 2 - 1).bfloat16()
    heads[2, v0 + Hkv - 1, 99] = -(448.0 * 2.0 ** -5 + 2.0 ** -4)            # the next bf16 above it: e = -4
    if form == "prompt":
        heads[3, v0] = 0                                                     # all-zero V head: scale 1, bytes 0
    cs = _cos_sin(Smax + 8).cuda()
    qn = (1 + 0.1 * torch.randn(HD, generator=g)).cuda() if norm else None
    kn = (1 + 0.1 * torch.randn(HD, generator=g)).cuda() if norm else None
    shift = torch.tensor([3, 0, 6][:B], dtype=torch.int32).cuda()            # non-zero pos_shift
    return B, S, slot0, Smax, ld, qkv, cs, qn, kn, shift


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("form", ["prompt", "decode"])
def test_append_is_exact(hip, Hq, Hkv, norm, form):
    B, S, slot0, Smax, ld, qkv, cs, qn, kn, shift = append_inputs(Hq, Hkv, norm, form)
    kvw = 2 * Hkv * HD
    a, b = qkv.cuda(), qkv.cuda()
    c16 = torch.full((B, Smax, kvw), -3.0, dtype=torch.bfloat16, device="cuda")
    c8 = torch.full((B, Smax, kvw), 0xAB, dtype=torch.uint8, device="cuda")
    sc = torch.full((B, Smax, 2 * Hkv), -7.0, dtype=torch.float32, device="cuda")
    hip.rope_kv_append(a, ld, B * S, S, Hq, Hkv, HD, cs, qn, kn, 1e-6, shift, c16, c16.stride(0), c16.stride(1), slot0)
    hip.rope_kv_append_e4m3(b, ld, B * S, S, Hq, Hkv, HD, cs, qn, kn, 1e-6, shift, c8, c8.stride(0), c8.stride(1), sc, sc.stride(0), sc.stride(1), slot0)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))             # q|k|v: the bits desta_rope_kv_append leaves
    assert not torch.equal(a.cpu().view(torch.int16), qkv.view(torch.int16))
    c16, c8, sc = c16.cpu(), c8.cpu(), sc.cpu()
    written = c16[:, slot0:slot0 + S]
    assert not bool((written == -3.0).all(-1).any())
    q, s, _ = quantize_slab(written.contiguous())
    assert torch.equal(c8[:, slot0:slot0 + S], q)
    assert torch.equal(sc[:, slot0:slot0 + S], s)
    rest = torch.ones(Smax, dtype=torch.bool)
    rest[slot0:slot0 + S] = False
    assert bool((c8[:, rest] == 0xAB).all()) and bool((sc[:, rest] == -7.0).all())
    # the planted heads (row r of the token grid is batch r // S, slot slot0 + r % S; scale column Hkv + j = V head j)
    def at(r):
        return r // S, slot0 + r % S
    assert float(sc[at(0) + (0,)]) == 1.0 and bool((c8[at(0)][:HD] & 0x7F == 0).all())      # the rotation leaves 0 * cos - 0 * sin = -0 in places: zero bytes of either sign
    assert float(sc[at(0) + (Hkv,)]) == 2.0 ** (3 - 133 - 8) and int(c8[at(0)][Hkv * HD + 5]) == 0x78       # 8 * 2^-133 -> 256
    assert float(sc[at(1) + (Hkv,)]) == 2.0 ** -5 and int(c8[at(1)][Hkv * HD + 17]) == 0x7E                 # 448
    assert float(sc[at(2) + (2 * Hkv - 1,)]) == 2.0 ** -4
    if form == "prompt":
        assert float(sc[at(3) + (Hkv,)]) == 1.0 and bool((c8[at(3)][Hkv * HD:(Hkv + 1) * HD] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_kv8_equals_bf16_kernel_on_dequantised_cache(hip, Hq, Hkv):
    cases = [c for c in _all_cases8(hip) if (c.c.Hq, c.c.Hkv) == (Hq, Hkv)]
    assert len(cases) >= 14
    for i, plain in enumerate(cases):
        for c8 in (plain, Case8(plain.base, spread_seed=100 + i)):
            o8, l8 = _run8(hip, c8)
            o16, l16 = _run16(hip, c8)
            assert bool(torch.isfinite(o8.float()).all()) and bool(torch.isfinite(l8).all())
            assert torch.equal(o8.view(torch.int16), o16.view(torch.int16)), (c8.c.B, c8.c.sk, (o8.float() - o16.float()).abs().max())
            assert torch.equal(l8.view(torch.int32), l16.view(torch.int32)), (c8.c.B, c8.c.sk)
    spread = Case8(cases[-1].base, spread_seed=7)                            # the power-of-two factors reach inside one 16-key tile
    assert int(spread.scales[0, :16, 0].unique().numel()) >= 3


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_kv8_vs_fp64(hip, Hq, Hkv):
    """Independent of the bf16 kernel: per element against fp64 on the dequantised operands, the bound of
    test_decode_attention_vs_fp64: 0.5 ulp_bf16 + 2^-8 sum p |v|, lse within 1e-4."""
    cases = [c for c in _all_cases8(hip) if (c.c.Hq, c.c.Hkv) == (Hq, Hkv)]
    worst = 0.0
    for c8 in cases:
        c = c8.c
        ref, absv, lse_ref = c.reference()
        out, lse = _run8(hip, c8)
        got = out.double()
        assert bool(torch.isfinite(got).all())
        bound = 0.5 * _bf16_ulp(torch.maximum(got.abs(), ref.abs())) + 2.0 ** -8 * absv
        frac = float(((got - ref).abs() / bound).max())
        dl = float((lse.double() - lse_ref).abs().max())
        worst = max(worst, frac)
        print(f"Hq {Hq} Hkv {Hkv} B {c.B} sk {c.sk:5d}: max |diff| / bound {frac:.3f}  rel-L2 {rel_err(got, ref):.2e}  |dlse| {dl:.2e}")
        assert frac <= 1.0, (c.B, c.sk, frac)
        assert dl <= 1e-4, (c.B, c.sk, dl)
    print(f"worst fraction of the per-element bound: {worst:.3f}")


def test_record_quantisation_distance(hip):
    """Recorded, not asserted beyond sanity: attention output of the FP8 cache against the UNQUANTISED bf16 cache (fp64 both)."""
    es = []
    for c8 in _all_cases8(hip):
        if c8.c.B == 3 and c8.c.sk >= 63:
            es.append(rel_err(c8.c.reference()[0], c8.base.reference()[0]))
    print("attention output rel-L2, FP8 cache vs bf16 cache (fp64 on both):", [round(e, 4) for e in es])
    assert max(es) < 0.1                                                     # e4m3 rounding: 2.65 % per Gaussian element


# ---------------------------------------------------------------------------------------------------------------- 4
def _int_v(B, Smax, Hkv):
    """Integers in [-8, 8] (exact in e4m3) times a per-key power of two, different by row, key, head and column."""
    b = torch.arange(B)[:, None, None, None]
    k = torch.arange(Smax)[None, :, None, None]
    h = torch.arange(Hkv)[None, None, :, None]
    col = torch.arange(HD)[None, None, None, :]
    iv = ((k * 7 + h * 3 + col * 5 + b * 11 + (k * col) % 13 + (k // 16) * 2) % 17 - 8).float()
    return iv * torch.exp2(((k * 3 + h) % 5 - 2).float())


def _exact_case(B, Hq, Hkv, sk, kv, seed):
    c = Case(B, Hq, Hkv, sk, kv, seed=seed)
    c.qbuf.zero_()
    v = _int_v(B, c.Smax, Hkv).reshape(B, c.Smax, Hkv * HD).bfloat16()
    c.cache[:, :, Hkv * HD:] = v
    return c, v


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("chunks", [1, 3])
def test_exact_layout_uniform_softmax(hip, Hq, Hkv, chunks):
    CH = hip.DECODE_ATTN_CHUNK
    sk = 2 * CH + 37 if chunks == 3 else CH - 3
    vis = (2 * CH, 64) if chunks == 3 else (128, 64)
    c, v = _exact_case(2, Hq, Hkv, sk, [sk - vis[0], sk - vis[1]], seed=3)
    c8 = Case8(c)
    assert torch.equal(c8.c.cache[:, :, Hkv * HD:], v)                       # V survives the quantisation exactly
    assert int(c8.scales[0, :16, Hkv].unique().numel()) >= 3                 # V scales differ inside a 16-key tile
    out, lse = _run8(hip, c8)
    G = Hq // Hkv
    for b, n in enumerate(vis):
        mean = c.v()[b, sk - n:].double().sum(0) / n                         # exact in fp32: multiples of 2^-2 over a power of two
        want = mean.float().bfloat16().repeat_interleave(G, dim=0)
        assert torch.equal(out[b], want), (b, (out[b].float() - want.float()).abs().max())
        assert float((lse[b].double() - math.log2(n)).abs().max()) <= 1e-6


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 1)])
@pytest.mark.parametrize("chunks", [1, 3])
def test_exact_layout_one_hot_softmax(hip, Hq, Hkv, chunks):
    CH = hip.DECODE_ATTN_CHUNK
    sk, B, G = (2 * CH + 11 if chunks == 3 else CH - 3), 2, Hq // Hkv
    c, v = _exact_case(B, Hq, Hkv, sk, [0, 3], seed=4)
    c.cache[:, :, :Hkv * HD] = 0
    want = torch.empty(B, Hq, HD, dtype=torch.bfloat16)
    q = c.qbuf[:, Q_OFF:Q_OFF + Hq * HD].view(B, Hq, HD)
    kview = c.cache[:, :, :Hkv * HD].view(B, c.Smax, Hkv, HD)
    hit = set()
    for b in range(B):
        for h in range(Hq):
            chunk = (h + b) % chunks
            j = chunk * CH + 3 + (13 * h + 5 * b) % (min(CH, sk - chunk * CH) - 3)
            hit.add(j // CH)
            q[b, h, h] = 64.0                                                # score of key j for head h: 64 * 64 / sqrt(128) = 362, all others 0
            kview[b, j, h // G, h] = 64.0
            want[b, h] = c.v()[b, j, h // G]
    assert len(hit) == chunks
    c8 = Case8(c)
    assert torch.equal(c8.c.cache, c.cache)                                  # K (0 / 64) and V are on the e4m3 grid
    out, _ = _run8(hip, c8)
    assert torch.equal(out, want), (out.float() - want.float()).abs().max()


# ---------------------------------------------------------------------------------------------------------------- 5
def test_nothing_outside_the_visible_slots_is_used(hip):
    CH = hip.DECODE_ATTN_CHUNK
    for sk in (CH - 1, 2 * CH + 37):
        c8 = Case8(Case(3, 8, 2, sk, [5, CH + 9, 0], seed=5))
        c = c8.c
        clean, lse_clean = _run8(hip, c8, ws_fill=0.0)
        by, sc = c8.bytes.clone(), c8.scales.clone()
        by[:, sk:], sc[:, sk:] = 0x7F, float("nan")                          # beyond seq_k: NaN bytes, NaN scales
        for b, k0 in enumerate(c.kv.tolist()):                               # in front of kv_start (row 1: a whole masked chunk)
            by[b, :k0], sc[b, :k0] = 0x7F, float("nan")
        out, lse = _run8(hip, c8, tensors=(by.cuda(), sc.cuda()))
        assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
        assert torch.equal(out, clean) and torch.equal(lse, lse_clean)


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (8, 1), (2, 2)])
def test_determinism_and_row_independence(hip, Hq, Hkv):
    c8 = _case8(hip, Hq, Hkv, 6, 3)                                          # 5 CH + 3 keys: six chunks
    c = c8.c
    first, lse0 = _run8(hip, c8)
    again, lse1 = _run8(hip, c8)
    assert torch.equal(first, again) and torch.equal(lse0, lse1)
    for b in range(3):
        alone, lse_b = _run8(hip, c8, rows=slice(b, b + 1))
        assert torch.equal(alone[0], first[b]) and torch.equal(lse_b[0], lse0[b]), b
    big = torch.full((3, c.Smax + 77, c.kvw), 0x7F, dtype=torch.uint8, device="cuda")       # another Smax, another scale batch stride
    big_s = torch.full((3, c.Smax + 77, 2 * Hkv), float("nan"), dtype=torch.float32, device="cuda")
    big[:, :c.sk], big_s[:, :c.sk] = c8.device()[1][:, :c.sk], c8.device()[2][:, :c.sk]
    moved, lse2 = _run8(hip, c8, tensors=(big, big_s))
    assert torch.equal(moved, first) and torch.equal(lse2, lse0)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_rejections(hip):
    CH = hip.DECODE_ATTN_CHUNK
    c8 = Case8(Case(2, 8, 2, 2 * CH + 5, [0, 3], seed=6))
    c = c8.c
    qbuf, by, sc, kv, _ = c8.device()
    out = torch.full((2, 16 * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((2, 16, 1), 7.0, dtype=torch.float32, device="cuda")
    need = hip.attention_decode_workspace_bytes(2, 8, c.sk, HD)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    sv = sc[:, :, c.Hkv:]

    def desc(**kw):
        d = _desc(hip, c, qbuf, by, kv, out, lse, c.Smax)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    n0, n16 = hip.ATTN_KV8_CALLS, hip.ATTN_DECODE_CALLS
    bad = [("scale", desc(), None, sv, ws[:need]), ("scale", desc(), sc, None, ws[:need]),
           ("seq_q", desc(seq_q=2), sc, sv, ws[:need]), ("head_dim", desc(head_dim=64), sc, sv, ws[:need]),
           ("group", desc(n_q_heads=16, n_kv_heads=1), sc, sv, ws[:need]), ("causal", desc(causal=1), sc, sv, ws[:need]),
           ("workspace", desc(), sc, sv, ws[:need - 1]), ("workspace", desc(), sc, sv, None), ("workspace", desc(), sc, sv, ws[4:need + 4])]
    for name, d, ks, vs, w in bad:
        with pytest.raises(RuntimeError, match=name) as ei:
            hip.attention_decode_kv8(d, ks, vs, sc.stride(0), sc.stride(1), w)
        assert "(-1)" in str(ei.value)                                       # DESTA_EINVAL
    torch.cuda.synchronize()
    assert hip.ATTN_KV8_CALLS == n0
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all())             # nothing was launched
    hip.attention_decode_kv8(desc(), sc, sv, sc.stride(0), sc.stride(1), ws[:need])
    torch.cuda.synchronize()
    assert hip.ATTN_KV8_CALLS == n0 + 1 and hip.ATTN_DECODE_CALLS == n16
    assert rel_err(out.reshape(-1)[:2 * 8 * HD].cpu().reshape(2, 8, HD), c.reference()[0]) < 8e-3


# ---------------------------------------------------------------------------------------------------------------- 8
def _dims(g4):
    d = copy.copy(O.tiny_dims(True))                                         # Qwen3: head_dim 128, 4 / 2 heads
    if g4:
        d.llm_hq, d.llm_hkv = 8, 2
    return d


def _text_inputs(d, S, pads, seed):
    gen = torch.Generator().manual_seed(seed)
    B = len(pads)
    ids = torch.randint(3, d.vocab, (B, S), generator=gen)
    am = torch.ones(B, S, dtype=torch.long)
    for b, n in enumerate(pads):
        am[b, :n] = 0
        ids[b, :n] = 0
    return ids, am, {"context_input_ids": ids, "context_attention_mask": am, "context_batch_start_positions": [],
                     "batch_features": None, "batch_transcription_ids": []}


def _errors(logits, lo, T):
    es = [rel_err(logits[t].float(), lo[t]) for t in range(T)]
    pick = logits.float().cpu().argmax(-1)
    gap = lo.max(-1).values - lo.gather(-1, pick.unsqueeze(-1)).squeeze(-1)
    return max(es), float((gap / lo.std(-1)).max())


def _gen(model, inputs, T, forced=None):
    return model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=forced, collect_logits=True, eos_token_id=[])


@pytest.mark.parametrize("g4", [False, True])
def test_model_fp8_cache_vs_oracle(g4):
    """See the module docstring and KV8_WORST_MEASURED for the measured numbers and the bound."""
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    T, CH = 12, H.DECODE_ATTN_CHUNK
    d = _dims(g4)
    w = O.init_weights(d, seed=7)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    with pytest.raises(ValueError, match="int4"):
        model.set_kv_cache("int4")
    assert model.llm.kv_cache_kind == "bf16"
    worst16 = worst8 = 0.0
    for S in (13, CH - 5):                                                   # a short prompt; one from which decoding crosses a chunk boundary
        ids, am, inputs = _text_inputs(d, S, [0, 5, CH // 2 + 3] if S > CH // 2 + 3 else [0, 5, 2], seed=S)
        with torch.no_grad():
            ref, lo = O.greedy_generate(w, d, O.embed_splice(w, d, ids, None, [], []), am, T, 0)
        model.set_kv_cache("bf16")
        out16, lg16 = _gen(model, inputs, T, ref)
        slabs16 = [c[:, :S].cpu() for c in model.llm.kv_cache]
        assert slabs16[0].dtype == torch.bfloat16
        model.set_kv_cache("fp8")
        n8, n16 = H.ATTN_KV8_CALLS, H.ATTN_DECODE_CALLS
        out8, lg8 = _gen(model, inputs, T, ref)
        assert H.ATTN_KV8_CALLS - n8 == d.llm_layers * (T - 1) and H.ATTN_DECODE_CALLS == n16
        assert out8.cpu().tolist() == ref.tolist() and lg8.shape == lo.shape
        assert torch.equal(lg8[0], lg16[0])                                  # prompt logits do not depend on the cache kind
        assert len(model.llm.kv_cache) == len(model.llm.kv_scale) == d.llm_layers
        for li in range(d.llm_layers):                                       # the prompt slots hold the host rule of the bf16 run's slots
            by, sc = model.llm.kv_cache[li], model.llm.kv_scale[li]
            assert by.dtype == torch.uint8 and by.shape == (3, S + T, 2 * d.llm_hkv * HD) and sc.shape == (3, S + T, 2 * d.llm_hkv)
            q, s, _ = quantize_slab(slabs16[li].contiguous())
            assert torch.equal(by[:, :S].cpu(), q) and torch.equal(sc[:, :S].cpu(), s), li
        out8b, lg8b = _gen(model, inputs, T, ref)                            # two FP8-cache runs: the same bits
        assert torch.equal(out8, out8b) and torch.equal(lg8, lg8b)
        e16, g16 = _errors(lg16, lo, T)
        e8, g8 = _errors(lg8, lo, T)
        agree = float((lg8.float().argmax(-1) == lg16.float().argmax(-1)).float().mean())
        print(f"G {d.llm_hq // d.llm_hkv} S {S}: worst per-step logits rel-L2 vs fp32 oracle  bf16 cache {e16:.3e} (gap/spread {g16:.3f})  "
              f"FP8 cache {e8:.3e} (gap/spread {g8:.3f})  greedy agreement FP8 vs bf16 cache {agree:.3f}")
        worst16, worst8 = max(worst16, e16), max(worst8, e8)
        assert e8 < REL_BOUND and g8 < GAP_BOUND, (S, e8, g8)
        model.set_kv_cache("bf16")                                           # back: the original run, bit for bit
        assert model.llm.kv_scale is None
        out16b, lg16b = _gen(model, inputs, T, ref)
        assert torch.equal(out16, out16b) and torch.equal(lg16, lg16b)
        assert model.llm.kv_cache[0].dtype == torch.bfloat16
    print(f"worst over the prompts: bf16 cache {worst16:.3e}  FP8 cache {worst8:.3e}")


def test_fp8_cache_needs_the_split_kv_geometry():
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    model = DeSTA25AudioModel(cfg_from_dims(O.tiny_dims(False)), weights=O.init_weights(O.tiny_dims(False), seed=7))     # Llama tiny: head_dim 64
    with pytest.raises(ValueError, match="head_dim"):
        model.set_kv_cache("fp8")
    assert model.llm.kv_cache_kind == "bf16"


def test_fp8_cache_with_fp8_weights_equals_bf16_weights_on_snapped_weights():
    """The cache kind and the weight format are independent: on weights that sit on the FP8 grid the two runs agree exactly."""
    from desta import _hip as H
    from test_gpu_fp8_decode import snap_llm_weights
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    T, CH = 12, H.DECODE_ATTN_CHUNK
    d = _dims(False)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=snap_llm_weights(O.init_weights(d, seed=7)))
    model.set_kv_cache("fp8")
    S = CH - 5
    _, _, inputs = _text_inputs(d, S, [0, 5, CH // 2 + 3], seed=S)
    n8, n16, nw = H.ATTN_KV8_CALLS, H.ATTN_DECODE_CALLS, H.GEMM_W8_CALLS
    ids_b, lg_b = _gen(model, inputs, T)
    assert H.GEMM_W8_CALLS == nw
    model.set_decode_weights("fp8")
    ids_f, lg_f = _gen(model, inputs, T)
    assert H.GEMM_W8_CALLS > nw
    assert H.ATTN_KV8_CALLS - n8 == 2 * d.llm_layers * (T - 1) and H.ATTN_DECODE_CALLS == n16
    assert torch.equal(ids_b, ids_f) and torch.equal(lg_b, lg_f)


def test_fp8_cache_with_orca_injection(golden_dir):
    """The ORCA golden's inputs on the Qwen3 tiny geometry (the golden's own LLM has head_dim 64, which the FP8 cache
    rejects): the LLM's cache is FP8, ORCA's audio K|V stay its own; per-step logits against the ORCA oracle within the bound."""
    import orca_oracle as R
    from safetensors.torch import load_file
    from test_gpu_orca import _oracle_with_theta
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    g = load_file(os.path.join(golden_dir, "ref_orca_tiny.safetensors"))
    kg, ds, ks, ntr = (int(x) for x in g["orca_dims"])
    d = copy.copy(O.tiny_dims(True))
    d.prompt_size = kg + ntr
    o = R.OrcaDims(global_num_tokens=kg, local_downsample=ds, local_kernel_size=ks, ortho_diversity_weight=0.05,
                   ortho_weight_qformer_local=0.05, align_weight_local=0.05, global_cross_attn=False, local_enabled=True)
    w = R.init_weights(d, o, seed=7)
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=ds,
                        orca_local_kernel_size=ks, orca_ortho_diversity_weight=0.05, orca_ortho_weight_qformer_local=0.05,
                        orca_align_weight_local=0.05, orca_rope_theta=float(g["rope_theta_used"]), orca_global_cross_attn=False, orca_local_enabled=True)
    n_ctx, T = int(g["gen_ctx_len"]), int(g["gen_ids"].shape[1])
    n = g["starts"].shape[0]
    inputs = {"context_input_ids": g["input_ids"][:, :n_ctx], "context_attention_mask": g["attention_mask"][:, :n_ctx],
              "context_batch_start_positions": [(int(b), int(p)) for b, p in g["starts"].tolist()], "batch_features": g["batch_features"],
              "batch_transcription_ids": [g["transcription_ids"][i:i + 1] for i in range(n)]}
    model = DeSTA25AudioModel(cfg, weights=w).eval()
    model.set_kv_cache("fp8")
    orig = _oracle_with_theta(float(g["rope_theta_used"]))
    try:
        with torch.no_grad():
            ref_ids = R.generate(w, d, o, inputs, T, 0)[0]
            lo = R.generate(w, d, o, inputs, T, 0, forced_tokens=ref_ids)[1]
        n8 = H.ATTN_KV8_CALLS
        ids, logits = _gen(model, inputs, T, ref_ids)
        assert H.ATTN_KV8_CALLS - n8 == d.llm_layers * (T - 1)
        assert ids.cpu().tolist() == ref_ids.tolist()
        e, gap = _errors(logits, lo, T)
        print(f"orca, FP8 cache: worst per-step logits rel-L2 {e:.3e}  gap/spread {gap:.3f}")
        assert e < REL_BOUND and gap < GAP_BOUND
    finally:
        R.rope_whole_vector = orig
