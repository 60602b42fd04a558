"""GPU: split-KV GQA decode attention (desta_attention_decode) and the decode step that dispatches to it.

Kernel: per element against masked softmax + P @ V in float64 on the bf16 operands, at every chunk count from one to six, every
group size, left padding that hides a whole first chunk or all keys but one, operands as slices of fused buffers; exact-integer
layouts (uniform softmax = exact mean, one-hot softmax = one V row), both bit for bit; nothing beyond seq_k is read; reruns, rows
alone and other batch strides give the same bits; rejections; agreement with the forward kernel the decode step used before.
Model: tiny Qwen3 geometry (G = 2 and G = 4), B = 3 with left pads, a prompt from which decoding crosses the dispatch threshold
and a chunk boundary, against the fp32 oracle within the decode path's own bounds; FP8 weights equal bf16 weights exactly.

Error bound of the per-element test: |out - ref| <= 0.5 ulp_bf16(max(|out|, |ref|)) + 2^-8 sum_j p_j |v_j|.  The largest error a
conforming kernel may carry is P rounded to bf16 for an MFMA (2^-9 relative per term); the bound doubles it for the sum / max
mismatch, the fp32 accumulation and exp2.  This kernel keeps P in fp32, so it sits inside.
Measured (MI355X, this file's shapes, chunk 256): worst |diff| / bound 0.36 (G = 1), 0.31 (G = 2), 0.49 (G = 4, the query-spread-30
case; 0.34 otherwise), 0.36 (G = 8); rel-L2 <= 1.7e-3; |lse - ref| <= 1.0e-6 (1.8e-5 at spread 30); rel-L2 against fp64 0.73-0.99 x
the forward kernel's on the same operands."""
import copy
import math

import pytest
import torch

import desta_oracle as O
from helpers import cfg_from_dims, rel_err

pytestmark = pytest.mark.gpu

HD = 128
HEADS = [(2, 2), (4, 2), (8, 2), (8, 1)]                                     # G = 1, 2, 4, 8
Q_OFF = 64                                                                   # Q starts at this column of the fused [B, qkvw] buffer


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _seq_ks(CH):
    return [1, 63, CH - 1, CH, CH + 1, 2 * CH + 37, 5 * CH + 3]


class Case:
    """Operands as decode_step passes them: Q at a column offset of a [B, qkvw] buffer, K | V the halves of a [B, Smax, 2 Hkv 128] slab."""

    def __init__(self, B, Hq, Hkv, sk, kv_start, seed, spread=1.0, extra=9):
        g = torch.Generator().manual_seed(seed)
        self.B, self.Hq, self.Hkv, self.sk, self.Smax = B, Hq, Hkv, sk, sk + extra
        self.qkvw, self.kvw = Q_OFF + (Hq + 2 * Hkv) * HD, 2 * Hkv * HD
        self.qbuf = (torch.randn(B, self.qkvw, generator=g) * spread).bfloat16()
        self.cache = torch.randn(B, self.Smax, self.kvw, generator=g).bfloat16()
        self.kv = torch.tensor([min(int(k), sk - 1) for k in kv_start], dtype=torch.int32)
        self.scale = HD ** -0.5
        self.dev = None
        self.ref = None

    def q(self):
        return self.qbuf[:, Q_OFF:Q_OFF + self.Hq * HD].reshape(self.B, self.Hq, HD)

    def k(self):
        return self.cache[:, :self.sk, :self.Hkv * HD].reshape(self.B, self.sk, self.Hkv, HD)

    def v(self):
        return self.cache[:, :self.sk, self.Hkv * HD:].reshape(self.B, self.sk, self.Hkv, HD)

    def reference(self):
        """(out [B, Hq, 128], sum_j p_j |v_j|, lse in the log2 domain), float64, computed once."""
        if self.ref is None:
            G = self.Hq // self.Hkv
            q, k, v = self.q().double(), self.k().double().repeat_interleave(G, dim=2), self.v().double().repeat_interleave(G, dim=2)
            s = torch.einsum("bhd,bkhd->bhk", q, k) * self.scale
            hidden = torch.arange(self.sk)[None, None, :] < self.kv[:, None, None]
            s = s.masked_fill(hidden, float("-inf"))
            p = torch.softmax(s, dim=-1)
            self.ref = (torch.einsum("bhk,bkhd->bhd", p, v), torch.einsum("bhk,bkhd->bhd", p, v.abs()),
                        torch.logsumexp(s, dim=-1) / math.log(2.0))
        return self.ref

    def device(self):
        if self.dev is None:
            self.dev = (self.qbuf.cuda(), self.cache.cuda(), self.kv.cuda())
        return self.dev


def _desc(hip, qbuf, cache, kv, out, lse, B, Hq, Hkv, sk, qkvw, Smax, scale):
    kvw = 2 * Hkv * HD
    return hip.attn_desc(qbuf, cache, cache, out, lse, batch=B, hq=Hq, hkv=Hkv, sq=1, sk=sk, hd=HD, scale=scale, causal=False, kv_start=kv,
                         q_off=Q_OFF, k_off=0, v_off=Hkv * HD, q_rs=qkvw, k_rs=kvw, v_rs=kvw, o_rs=Hq * HD,
                         q_bs=qkvw, k_bs=Smax * kvw, v_bs=Smax * kvw, o_bs=Hq * HD)


def _workspace(hip, B, Hq, sk, fill):
    n = hip.attention_decode_workspace_bytes(B, Hq, sk, HD)
    return torch.full((n // 4,), fill, dtype=torch.float32, device="cuda") if n else None


def _run(hip, c, *, ws_fill=float("nan"), rows=None, tensors=None, Smax=None, old=False):
    """-> (O [B, Hq, 128] bf16, lse [B, Hq] fp32) on the CPU.  rows: a slice of the batch; old: the forward kernel."""
    qbuf, cache, kv = tensors if tensors is not None else c.device()
    if rows is not None:
        qbuf, cache, kv = qbuf[rows].contiguous(), cache[rows].contiguous(), kv[rows].contiguous()
    B = qbuf.shape[0]
    out = torch.full((B, c.Hq * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, c.Hq, 1), 7.0, dtype=torch.float32, device="cuda")
    d = _desc(hip, qbuf, cache, kv, out, lse, B, c.Hq, c.Hkv, c.sk, c.qkvw, Smax or c.Smax, c.scale)
    if old:
        hip.attention_fwd(d)
    else:
        hip.attention_decode(d, _workspace(hip, B, c.Hq, c.sk, ws_fill))
    torch.cuda.synchronize()
    return out.cpu().reshape(B, c.Hq, HD), lse.cpu().reshape(B, c.Hq)


_CASES = {}


def _case(hip, Hq, Hkv, sk_i, B, spread=1.0):
    """The shared cases of the fp64 tests: built (and their reference computed) once per module."""
    CH = hip.DECODE_ATTN_CHUNK
    sk = _seq_ks(CH)[sk_i]
    key = (Hq, Hkv, sk, B, spread)
    if key not in _CASES:
        kv = [5, CH + 9, 0] if B == 3 else [sk - 1]                          # a wholly masked first chunk; one visible key
        _CASES[key] = Case(B, Hq, Hkv, sk, kv, seed=Hq * 1000 + Hkv * 100 + sk + B, spread=spread)
    return _CASES[key]


def _all_cases(hip):
    for Hq, Hkv in HEADS:
        for sk_i in range(7):
            for B in (1, 3):
                yield _case(hip, Hq, Hkv, sk_i, B)
    yield _case(hip, 8, 2, 5, 3, spread=30.0)                                # saturated softmax: query spread 30


def _bf16_ulp(x):
    return torch.exp2(torch.floor(torch.log2(x.clamp_min(2.0 ** -126))) - 7)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_decode_attention_vs_fp64(hip, Hq, Hkv):
    cases = [c for c in _all_cases(hip) if (c.Hq, c.Hkv) == (Hq, Hkv)]
    assert len(cases) >= 14
    worst_frac = 0.0
    for c in cases:
        ref, absv, lse_ref = c.reference()
        out, lse = _run(hip, c)
        got = out.double()
        assert bool(torch.isfinite(got).all())
        bound = 0.5 * _bf16_ulp(torch.maximum(got.abs(), ref.abs())) + 2.0 ** -8 * absv
        frac = float(((got - ref).abs() / bound).max())
        l2 = rel_err(got, ref)
        dl = float((lse.double() - lse_ref).abs().max())
        worst_frac = max(worst_frac, frac)
        print(f"Hq {Hq} Hkv {Hkv} B {c.B} sk {c.sk:5d} kv_start {c.kv.tolist()}: max |diff| / bound {frac:.3f}  rel-L2 {l2:.2e}  |dlse| {dl:.2e}")
        assert frac <= 1.0, (c.B, c.sk, frac)
        assert l2 < 8e-3, (c.B, c.sk, l2)
        assert dl <= 1e-4, (c.B, c.sk, dl)
    print(f"worst fraction of the per-element bound: {worst_frac:.3f}")


# ---------------------------------------------------------------------------------------------------------------- 2
def _int_v(B, Smax, Hkv):
    """Small integers in [-8, 8] that differ by row, key, head and column, asymmetric in (key, column)."""
    b = torch.arange(B)[:, None, None, None]
    k = torch.arange(Smax)[None, :, None, None]
    h = torch.arange(Hkv)[None, None, :, None]
    col = torch.arange(HD)[None, None, None, :]
    return ((k * 7 + h * 3 + col * 5 + b * 11 + (k * col) % 13 + (k // 16) * 2) % 17 - 8).float()


@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_exact_layout_uniform_softmax(hip, Hq, Hkv):
    CH = hip.DECODE_ATTN_CHUNK
    sk = 2 * CH + 37                                                         # row 0: 2 CH visible keys over chunks 0, 1, 2; row 1: 64 keys of chunk 2
    c = Case(2, Hq, Hkv, sk, [37, sk - 64], seed=3)
    c.qbuf.zero_()
    c.cache[:, :, Hkv * HD:] = _int_v(2, c.Smax, Hkv).reshape(2, c.Smax, Hkv * HD).bfloat16()
    out, lse = _run(hip, c)
    G = Hq // Hkv
    for b, n in ((0, 2 * CH), (1, 64)):
        mean = c.v()[b, sk - n:].double().sum(0) / n                         # [Hkv, 128]: exact in fp32 (integers over a power of two)
        want = mean.float().bfloat16().repeat_interleave(G, dim=0)
        assert torch.equal(out[b], want), (b, (out[b].float() - want.float()).abs().max())
        assert float((lse[b].double() - math.log2(n)).abs().max()) <= 1e-6


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_exact_layout_one_hot_softmax(hip, Hq, Hkv):
    CH = hip.DECODE_ATTN_CHUNK
    sk, B, G = 3 * CH + 11, 2, Hq // Hkv                                     # four chunks, the last of 11 keys
    c = Case(B, Hq, Hkv, sk, [0, 3], seed=4)
    c.qbuf.zero_()
    c.cache[:, :, :Hkv * HD] = 0
    want = torch.empty(B, Hq, HD, dtype=torch.bfloat16)
    q = c.qbuf[:, Q_OFF:Q_OFF + Hq * HD].view(B, Hq, HD)
    kview = c.cache[:, :, :Hkv * HD].view(B, c.Smax, Hkv, HD)
    chunks = set()
    for b in range(B):
        for h in range(Hq):
            chunk = (h + b) % 4
            j = chunk * CH + 3 + (13 * h + 5 * b) % (min(CH, sk - chunk * CH) - 3)   # a different key, in a different chunk, per head
            chunks.add(j // CH)
            q[b, h, h] = 64.0                                                # score of key j for head h: 64 * 64 / sqrt(128) = 362, all others 0
            kview[b, j, h // G, h] = 64.0
            want[b, h] = c.v()[b, j, h // G]
    assert chunks == {0, 1, 2, 3} or Hq < 4
    out, _ = _run(hip, c)
    assert torch.equal(out, want), (out.float() - want.float()).abs().max()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_nothing_beyond_seq_k_is_used(hip):
    CH = hip.DECODE_ATTN_CHUNK
    for sk in (CH - 1, 2 * CH + 37):
        c = Case(3, 8, 2, sk, [5, CH + 9, 0], seed=5)
        c.cache[:, sk:] = float("nan")
        out_nan, lse_nan = _run(hip, c, ws_fill=float("nan"))
        z = c.cache.clone()
        z[:, sk:] = 0
        out_z, lse_z = _run(hip, c, ws_fill=0.0, tensors=(c.qbuf.cuda(), z.cuda(), c.kv.cuda()))
        assert bool(torch.isfinite(out_nan.float()).all()) and bool(torch.isfinite(lse_nan).all())
        assert torch.equal(out_nan, out_z) and torch.equal(lse_nan, lse_z)
        assert rel_err(out_nan, c.reference()[0]) < 8e-3


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("Hq,Hkv", [(8, 2), (8, 1), (2, 2)])
def test_determinism_and_row_independence(hip, Hq, Hkv):
    c = _case(hip, Hq, Hkv, 6, 3)                                            # 5 CH + 3 keys: six chunks
    first, lse0 = _run(hip, c)
    again, lse1 = _run(hip, c)
    assert torch.equal(first, again) and torch.equal(lse0, lse1)
    for b in range(3):                                                       # each row alone at B = 1
        alone, lse_b = _run(hip, c, rows=slice(b, b + 1))
        assert torch.equal(alone[0], first[b]) and torch.equal(lse_b[0], lse0[b]), b
    qbuf, cache, kv = c.device()                                             # another Smax: another batch stride, another allocation
    big = torch.full((3, c.Smax + 77, c.kvw), float("nan"), dtype=torch.bfloat16, device="cuda")
    big[:, :c.sk] = cache[:, :c.sk]
    moved, lse2 = _run(hip, c, tensors=(qbuf, big, kv), Smax=c.Smax + 77)
    assert torch.equal(moved, first) and torch.equal(lse2, lse0)


# ---------------------------------------------------------------------------------------------------------------- 6, 9
def test_rejections_and_workspace_size(hip):
    CH = hip.DECODE_ATTN_CHUNK
    c = Case(2, 8, 2, 2 * CH + 5, [0, 3], seed=6)
    qbuf, cache, kv = c.device()
    out = torch.full((2, 16 * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((2, 16, 1), 7.0, dtype=torch.float32, device="cuda")
    other = torch.zeros(2, 16 * HD, dtype=torch.float32, device="cuda")
    need = hip.attention_decode_workspace_bytes(2, 8, c.sk, HD)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")

    def desc():
        return _desc(hip, qbuf, cache, kv, out, lse, 2, 8, 2, c.sk, c.qkvw, c.Smax, c.scale)

    def setter(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f
    n0 = hip.ATTN_DECODE_CALLS
    bad = [("seq_q", setter(seq_q=2)), ("head_dim", setter(head_dim=64)), ("group", setter(n_q_heads=16, n_kv_heads=1)),
           ("causal", setter(causal=1)), ("dropout", setter(dropout_p=0.1)), ("rope_cos_sin", setter(rope_cos_sin=other.data_ptr())),
           ("O_f32", setter(O_f32=other.data_ptr())), ("dO", setter(dO=other.data_ptr())), ("dQ", setter(dQ=other.data_ptr())),
           ("O must be 16-byte aligned", setter(O=out.data_ptr() + 2))]
    for name, change in bad:
        d = desc()
        change(d)
        with pytest.raises(RuntimeError, match=name):
            hip.attention_decode(d, ws)
    with pytest.raises(RuntimeError, match="workspace"):                     # one byte short
        hip.attention_decode(desc(), ws[:need - 1])
    with pytest.raises(RuntimeError, match="workspace"):                     # none at all for a row of three chunks
        hip.attention_decode(desc(), None)
    torch.cuda.synchronize()
    assert hip.ATTN_DECODE_CALLS == n0
    assert bool((out == 7.0).all()) and bool((lse == 7.0).all())             # nothing was launched
    # the size grows with ceil(seq_k / CH), and what it reports is enough
    sizes = [hip.attention_decode_workspace_bytes(2, 8, sk, HD) for sk in (CH, CH + 1, 2 * CH, 2 * CH + 1, 3 * CH, 5 * CH + 3)]
    assert sizes[0] == 0 and 0 < sizes[1] == sizes[2] < sizes[3] == sizes[4] < sizes[5]
    assert sizes[5] * 2 == sizes[1] * 6 and need == sizes[3]
    hip.attention_decode(desc(), ws)
    short = Case(2, 8, 2, CH, [0, 3], seed=7)                                # one chunk: no workspace at all
    o1, _ = _run(hip, short)
    torch.cuda.synchronize()
    assert hip.ATTN_DECODE_CALLS == n0 + 2
    assert rel_err(out.reshape(-1)[:2 * 8 * HD].cpu().reshape(2, 8, HD), c.reference()[0]) < 8e-3 and rel_err(o1, short.reference()[0]) < 8e-3


# ---------------------------------------------------------------------------------------------------------------- 7
def test_agreement_with_the_forward_kernel(hip):
    """The new kernel's error against fp64 is at most 1.5x that of the forward kernel the decode step used before."""
    n = 0
    for c in _all_cases(hip):
        if c.sk < 64:
            continue
        ref = c.reference()[0]
        new, _ = _run(hip, c)
        old, _ = _run(hip, c, old=True)
        e_new, e_old = rel_err(new, ref), rel_err(old, ref)
        print(f"Hq {c.Hq} Hkv {c.Hkv} B {c.B} sk {c.sk:5d}: rel-L2 vs fp64  decode {e_new:.3e}  forward {e_old:.3e}")
        assert e_new <= 1.5 * e_old, (c.Hq, c.Hkv, c.B, c.sk, e_new, e_old)
        n += 1
    assert n == 4 * 5 * 2 + 1


# ---------------------------------------------------------------------------------------------------------------- 8
def _check_against_oracle(logits, lo, T):
    """The bounds of tests/test_gpu_wide_decode.py::_check_against_oracle, the decode path's own."""
    es = [rel_err(logits[t].float(), lo[t]) for t in range(T)]
    pick = logits.float().cpu().argmax(-1)
    gap = lo.max(-1).values - lo.gather(-1, pick.unsqueeze(-1)).squeeze(-1)
    worst = float((gap / lo.std(-1)).max())
    print("per-step logits rel-L2", [round(e, 4) for e in es], "gap/spread", worst)
    assert max(es) < 3e-2, es
    assert worst < 0.1, worst


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


def _prompt_lengths(H):
    """Prompts from which T = 12 steps cross the dispatch threshold and a chunk boundary (one prompt when they coincide)."""
    CH, MIN = H.DECODE_ATTN_CHUNK, H.DECODE_ATTN_MIN_KEYS
    lens = [MIN - 6]
    if MIN % CH:
        lens.append((MIN // CH + 1) * CH - 5)
    return lens


@pytest.mark.parametrize("g4", [False, True])
def test_decode_step_dispatch_vs_oracle(g4):
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    T, CH, MIN = 12, H.DECODE_ATTN_CHUNK, H.DECODE_ATTN_MIN_KEYS
    d = _dims(g4)
    w = O.init_weights(d, seed=7)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    crossed_min = crossed_chunk = False
    for S in _prompt_lengths(H):
        ids, am, inputs = _text_inputs(d, S, [0, 5, CH // 2 + 3], seed=S)
        with torch.no_grad():
            ref, lo = O.greedy_generate(w, d, O.embed_splice(w, d, ids, None, [], []), am, T, 0)
        keys = [S + t + 1 for t in range(T - 1)]                             # seq_k of the decode steps
        crossed_min |= keys[0] < MIN <= keys[-1]
        crossed_chunk |= any(k >= MIN and k % CH == 1 for k in keys[1:])
        n0 = H.ATTN_DECODE_CALLS
        out, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref, collect_logits=True,
                                           eos_token_id=[])
        assert H.ATTN_DECODE_CALLS - n0 == d.llm_layers * sum(k >= MIN for k in keys)
        assert out.cpu().tolist() == ref.tolist() and logits.shape == lo.shape
        _check_against_oracle(logits, lo, T)
    assert crossed_min and crossed_chunk
    # a 13-token prompt stays on the forward kernel
    ids, am, inputs = _text_inputs(d, 13, [0, 5, 2], seed=13)
    n0 = H.ATTN_DECODE_CALLS
    model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, eos_token_id=[])
    assert H.ATTN_DECODE_CALLS == n0


def test_decode_step_dispatch_fp8_equals_bf16_on_snapped_weights():
    """Attention is the same kernel under both weight formats: on weights that sit on the FP8 grid the two runs agree exactly."""
    from desta import _hip as H
    from test_gpu_fp8_decode import snap_llm_weights
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    T, CH, MIN = 12, H.DECODE_ATTN_CHUNK, H.DECODE_ATTN_MIN_KEYS
    d = _dims(False)
    w = snap_llm_weights(O.init_weights(d, seed=7))
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    S = _prompt_lengths(H)[-1]
    ids, am, inputs = _text_inputs(d, S, [0, 5, CH // 2 + 3], seed=S)
    n0 = H.ATTN_DECODE_CALLS
    ids_b, lg_b = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[])
    model.set_decode_weights("fp8")
    ids_f, lg_f = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[])
    per_run = d.llm_layers * sum(S + t + 1 >= MIN for t in range(T - 1))
    assert per_run > 0 and H.ATTN_DECODE_CALLS - n0 == 2 * per_run
    assert all("q8" in ly for ly in model.llm.layers)
    assert torch.equal(ids_b, ids_f)
    for t in range(T):
        assert torch.equal(lg_b[t], lg_f[t]), t
