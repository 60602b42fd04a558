"""GPU: draft-and-verify greedy decoding (`set_speculative`, `CausalLMHIP.verify_step`, desta_spec_ngram_draft, desta_spec_accept).

Kernels: both integer kernels bit for bit against tests/speculative_reference.py, sentinels around everything they write; rejected
arguments return DESTA_EINVAL and launch nothing.
Attention: the forward kernel in exactly the configuration `verify_step` uses (2 - 8 query rows per sequence over a cache slab,
causal with cached keys in front, left pads), per element against fp64 by the criterion of tests/attention_reference.py.
Verify step: after one prompt pass, `verify_step` on the plain run's tokens against `decode_step` at the same positions: the cache
slots [cur, cur + k] of every layer and every row's logits.  Both paths run the same computation in bf16 with fp32 accumulation and
differ only in kernel choice (row count) and summation order, so their distance is bounded by 1.5 x the plain path's own distance
from the fp32 oracle on the same inputs, the rule of tests/test_gpu_prefill_chunk.py::test_chunked_vs_oracle; the cache rows are
intermediate activations of that same computation and are held to the same figure.
Launches: `verify_step` and `decode_step` are one body (`CausalLMHIP._step_rows`); at equal row counts (M = 12 and 24, bf16 and FP8
decode weights) the recorded launches of the two are equal lists (name, M, N, K, act, fused norm, residual), the attention entry
and the append's rows per sequence apart, and those two are what each width is meant to run.
Model (tiny Qwen3 geometry, B = 3 with left pads, T = 24): the emitted tokens do not depend on where the drafts come from (perfect,
none, corrupted, random, the lookup kernel) and equal the plain loop's and the fp32 oracle's; the number of verify steps is the one
the drafts imply; every fallback runs the plain loop with the bits of `set_speculative(None)`.

The oracle comparison of the invariance test: a row is compared with the oracle's greedy ids up to its first differing step, and the
difference is excused (the rest of the row cut) only where the ORACLE rates the other token within 0.1 of its maximum (gap / spread,
the sense of `_errors`); at most 10 % of the (row, step) cases may be cut.  The literal "top-2 gap / spread of the oracle below 0.1"
cannot be the cut on these fixtures: with 512 nearly Gaussian logits per step it holds at about one step in four, and on the
prompts of tests/test_gpu_prefill_chunk.py (seed = S) it would cut 82 - 96 % of the cases (measured with the oracle alone).  The
prompt seeds are instead chosen, with the oracle alone, so that no step is closer than MIN_TOP2 (see SPEC_SEEDS).

Measured (MI355X, profiles/r20_spec_tests.log):
  * verify step against single steps, G = 2 and 4, bf16 and FP8 decode weights, M = 12 and 24: logits rel-L2 0.000e+00 in all eight
    cases, the appended cache slots too (the bits are equal); the single steps' own worst against the fp32 oracle 5.6e-3 - 5.9e-3
    (bf16 weights), 2.9e-2 (FP8 weights);
  * invariance: 0.000 of the (row, step) cases cut in all four configurations; per-step logits rel-L2 against the oracle <= 5.8e-3,
    gap / spread 0.000; perfect drafts 6 (k = 3) and 3 (k = 7) verify steps, all -1 and random drafts 23, the corrupted drafts 8 and 5;
    the lookup kernel accepts nothing on random weights (23 steps);
  * verify attention against fp64, worst |err| / bound 0.476 (sq 2, sk 62), equal to the emulation's ratio in every case.
"""
import copy
import math
import os
import random

import pytest
import torch

import attention_reference as R
import desta_oracle as O
import speculative_reference as SR
from helpers import cfg_from_dims, rel_err
from test_gpu_decode_attention import _check_against_oracle
from test_gpu_kv8_cache import HD, _dims, _gen, _text_inputs
from test_gpu_prefill_chunk import PADS, _model, _oracle, _poison_free_memory

pytestmark = pytest.mark.gpu

SENTINEL = -77
GAP_CUT = 0.1                                                                # BF16_GAP_BOUND of tests/test_gpu_prefill_chunk.py


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


# ---------------------------------------------------------------------------------------------------------------- 3 (first)
@pytest.mark.parametrize("pad", [0, 5, 131])
@pytest.mark.parametrize("sk_kind", ["sq+60", "257", "449+sq"])
@pytest.mark.parametrize("sq", [2, 4, 8])
@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (8, 2)])
def test_verify_attention_vs_fp64(hip, Hq, Hkv, sq, sk_kind, pad):
    """A chunk of sq = k + 1 query rows at slots [sk - sq, sk) of the slab; key j is visible to query i iff pad <= j <= i + (sk - sq).
    Criterion of tests/test_gpu_prefill_chunk.py::test_chunk_attention_vs_fp64."""
    sk = {"sq+60": sq + 60, "257": 257, "449+sq": 449 + sq}[sk_kind]
    B, pads = 2, [0, pad]                                                    # (pad 131 over 62 - 68 keys: a row that sees no key at all)
    Smax, qkvw, kvw = sk + 9, (Hq + 2 * Hkv) * HD, 2 * Hkv * HD
    g = torch.Generator().manual_seed(Hq * 1000 + sq * 7 + sk + pad)
    qbuf = torch.randn(B * sq, qkvw, generator=g).bfloat16()
    slab = torch.randn(B, Smax, kvw, generator=g).bfloat16()
    kv = torch.tensor(pads, dtype=torch.int32)
    q = qbuf[:, :Hq * HD].reshape(B, sq, Hq, HD)
    k, v = slab[:, :sk, :Hkv * HD].reshape(B, sk, Hkv, HD), slab[:, :sk, Hkv * HD:].reshape(B, sk, Hkv, HD)
    a = (q, k, v, torch.zeros_like(q), HD ** -0.5, True, kv)
    ref = R.exact(*a)
    emu_ratio = R.worst_ratio(ref, "O", R.emulate(*a, fwd8=False)["O"])
    o = torch.full((B * sq, Hq * HD), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, Hq, sq), 7.0, device="cuda")
    qd, sd = qbuf.cuda(), slab.cuda()
    sd[:, sk:] = float("nan")                                                # slots behind the chunk are never read
    d = hip.attn_desc(qd, sd, sd, o, lse, batch=B, hq=Hq, hkv=Hkv, sq=sq, sk=sk, hd=HD, scale=HD ** -0.5, causal=True, kv_start=kv.cuda(),
                      q_off=0, k_off=0, v_off=Hkv * HD, q_rs=qkvw, k_rs=kvw, v_rs=kvw, o_rs=Hq * HD, k_bs=Smax * kvw, v_bs=Smax * kvw)
    hip.attention_fwd(d)
    torch.cuda.synchronize()
    got, lse = o.cpu().view(B, sq, Hq, HD), lse.cpu()
    ratio = R.worst_ratio(ref, "O", got.double())
    live = ref["live"]
    lse_err = float(((lse.double() - ref["lse"])[live].abs() / (1 + ref["lse"][live].abs())).max())
    dead_rows = int((~live[1, 0]).sum())
    print(f"VERIFY_ATTN Hq {Hq} Hkv {Hkv} sq {sq} sk {sk} pad {pad}: O {ratio:.3f} ({emu_ratio:.3f}) lse {lse_err:.1e} "
          f"rows of the padded sequence without a key {dead_rows}")
    assert dead_rows == min(sq, max(0, pad - (sk - sq))) and bool(live[0].all())
    assert ratio <= min(2.0, 2.0 * emu_ratio), (ratio, emu_ratio)
    assert lse_err <= 1e-4
    assert bool(torch.isinf(lse[~live]).all()) and bool((lse[~live] > 0).all())
    assert bool((got[1, :dead_rows] == 0).all())                            # rows that lie wholly in the padding


# ---------------------------------------------------------------------------------------------------------------- 1
def _draft(hip, rows, hist_len, starts, k, n_max, n_min):
    """Kernel and reference on the same rows -> (kernel [B][k], reference [B][k]); the draft buffer sits between sentinels."""
    B, ld = len(rows), max(len(r) for r in rows) + 3
    hist = torch.full((B, ld), SENTINEL, dtype=torch.int64)
    for b, r in enumerate(rows):
        hist[b, :len(r)] = torch.tensor(r, dtype=torch.int64)
    buf = torch.full((B * k + 16,), SENTINEL, dtype=torch.int64, device="cuda")
    draft = buf[8:8 + B * k].view(B, k)
    hip.spec_ngram_draft(hist.cuda(), hist_len, torch.tensor(starts, dtype=torch.int32).cuda(), k, n_max, n_min, draft)
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert bool((buf[:8] == SENTINEL).all()) and bool((buf[8 + B * k:] == SENTINEL).all())
    return buf[8:8 + B * k].view(B, k).tolist(), [SR.ngram_draft(r, hist_len, s, k, n_max, n_min) for r, s in zip(rows, starts)]


@pytest.mark.parametrize("k", [1, 3, 7])
def test_lookup_kernel_equals_the_reference(hip, k):
    rng = random.Random(k)
    n0 = hip.SPEC_DRAFT_CALLS
    # hand cases (tests/test_speculative_host.py checks the reference on them): two matches, a longer n beats a shorter one,
    # row_start inside the only match, a continuation that runs into hist_len, -1 inside a would-be match: B = 5, five answers
    rows = [[1, 2, 3, 9, 1, 2, 3, 8, 2, 3], [1, 2, 3, 9, 7, 3, 8, 2, 3, 0], [4, 5, 6, 4, 5, 0, 0, 0, 0, 0], [4, 5, 4, 5, 0, 0, 0, 0, 0, 0],
            [4, -1, 6, 4, -1, 0, 0, 0, 0, 0]]
    for hl, starts, n_max, n_min in ((10, [0] * 5, 2, 1), (9, [0] * 5, 2, 1), (5, [0, 0, 1, 0, 0], 2, 2), (5, [0, 0, 1, 0, 0], 2, 1),
                                     (5, [0, 0, 2, 0, 0], 2, 1), (4, [0] * 5, 2, 2), (5, [0] * 5, 4, 1)):
        got, want = _draft(hip, rows, hl, starts, k, n_max, n_min)
        assert got == want, (hl, starts, n_max, n_min)
    got, want = _draft(hip, rows, 10, [0] * 5, k, 2, 1)
    assert len({tuple(r) for r in want}) >= 3                                # different answers per row
    # random histories over a small alphabet (matches at every n), planted repeats, -1 runs (pads in front, placeholders inside)
    for hist_len in (1, 2, 3, 4, 130, 4100):
        for n_max, n_min in ((4, 1), (3, 1), (4, 4), (2, 2), (hist_len if 1 <= hist_len <= 4 else 3, 1)):
            rows, starts = [], []
            for b in range(5):
                r = [rng.randrange(0, 4 + 3 * b) for _ in range(hist_len + 2)]
                pad = rng.randrange(0, max(1, hist_len // 3))
                r[:pad] = [-1] * pad
                if hist_len >= 130:
                    i = rng.randrange(pad, hist_len - 40)
                    r[hist_len - 6:hist_len] = r[i:i + 6]                    # the suffix repeats an earlier stretch
                    j = rng.randrange(pad, hist_len - 20)
                    r[j:j + 3] = [-1] * 3
                rows.append(r)
                starts.append(pad if b % 2 else 0)
            got, want = _draft(hip, rows, hist_len, starts, k, n_max, n_min)
            assert got == want, (hist_len, n_max, n_min)
            if hist_len >= 130 and (n_max, n_min) == (4, 1):
                assert any(t >= 0 for r in want for t in r)
    assert hip.SPEC_DRAFT_CALLS > n0


def test_lookup_kernel_rejections(hip):
    hist = torch.zeros(2, 16, dtype=torch.int64, device="cuda")
    start = torch.zeros(2, dtype=torch.int32, device="cuda")
    draft = torch.full((2, 8), SENTINEL, dtype=torch.int64, device="cuda")
    n0 = hip.SPEC_DRAFT_CALLS
    for name, (hl, k, n_max, n_min) in (("k", (8, 0, 3, 1)), ("k", (8, 8, 3, 1)), ("n-gram", (8, 3, 5, 1)), ("n-gram", (8, 3, 2, 3)),
                                        ("n-gram", (8, 3, 3, 0)), ("hist_len", (0, 3, 3, 1)), ("hist_len", (17, 3, 3, 1))):
        with pytest.raises(RuntimeError, match=name) as ei:
            hip.spec_ngram_draft(hist, hl, start, k, n_max, n_min, draft)
        assert "(-1)" in str(ei.value)                                       # DESTA_EINVAL
    torch.cuda.synchronize()
    assert hip.SPEC_DRAFT_CALLS == n0 and bool((draft == SENTINEL).all())    # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- 2
EOS_A, EOS_B, PAD_ID = 900, 901, 0


def _accept_case(rng, B, k, eos_mode, n_fin):
    """Rows with every m_b in 0..k (cyclic), an EOS planted by `eos_mode` at index 0 / the middle / m_b of some rows."""
    pred, inp, fin = [], [], []
    for b in range(B):
        m = (b + rng.randrange(0, k + 1)) % (k + 1) if B > 1 else rng.randrange(0, k + 1)
        p = [rng.randrange(1, 800) for _ in range(k + 1)]
        e = {"none": None, "first": 0, "middle": m // 2, "last": m}[eos_mode] if b % 2 == 0 else None
        if e is not None:
            p[e] = EOS_B if b % 4 == 0 else EOS_A
        x = [rng.randrange(1, 800)] + [p[j] for j in range(k)]
        if m < k:
            x[m + 1] = -1 if b % 3 == 0 else p[m] + 1                        # the first rejected draft: absent, or wrong
        pred.append(p)
        inp.append(x)
        fin.append(b >= B - n_fin)
    return pred, inp, fin


@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("B", [1, 3, 21])
def test_accept_kernel_equals_the_reference(hip, B, k):
    rng = random.Random(B * 10 + k)
    n, P, ld = 5, 3, 5 + k + 1 + 4
    seen_m, seen_a = set(), set()
    for eos_mode in ("none", "first", "middle", "last"):
        for n_fin in sorted({0, B // 3, B}):
            for max_take in sorted({1, 2, k + 1}):
                for m_all in [None] + (list(range(k + 1)) if eos_mode == "none" and n_fin == 0 else []):
                    pred, inp, fin = _accept_case(rng, B, k, eos_mode, n_fin)
                    if m_all is not None:                                    # every row accepts exactly m_all drafts: a = min(max_take, m_all + 1)
                        for p, x in zip(pred, inp):
                            x[1:] = p[:k]
                            if m_all < k:
                                x[m_all + 1] = -1
                        seen_m.add(m_all)
                    eos = [EOS_A, EOS_B]
                    w_out, w_fin, w_next, w_a = SR.accept(pred, inp, fin, eos, PAD_ID, max_take)
                    out = torch.full((B, ld), SENTINEL, dtype=torch.int64, device="cuda")
                    hist = torch.full((B, P + ld), SENTINEL, dtype=torch.int64, device="cuda")
                    nxt = torch.full((B + 2,), SENTINEL, dtype=torch.int64, device="cuda")
                    taken = torch.full((3,), SENTINEL, dtype=torch.int32, device="cuda")
                    fin_d = torch.tensor(fin + [False, True], dtype=torch.bool).cuda()
                    hip.spec_accept(torch.tensor(pred).cuda(), torch.tensor(inp).cuda(), k, fin_d, torch.tensor(eos).cuda(), PAD_ID, max_take,
                                    out, n, nxt[1:B + 1], taken[1:2], hist=hist, hist_col=P + n)
                    torch.cuda.synchronize()
                    out, hist, nxt, taken, fin_d = out.cpu(), hist.cpu(), nxt.cpu(), taken.cpu(), fin_d.cpu()
                    key = (eos_mode, n_fin, max_take, m_all)
                    assert taken.tolist() == [SENTINEL, w_a, SENTINEL], key
                    assert out[:, n:n + w_a].tolist() == w_out, key
                    assert bool((out[:, :n] == SENTINEL).all()) and bool((out[:, n + w_a:] == SENTINEL).all()), key
                    assert hist[:, P + n:P + n + w_a].tolist() == w_out, key
                    assert bool((hist[:, :P + n] == SENTINEL).all()) and bool((hist[:, P + n + w_a:] == SENTINEL).all()), key
                    assert nxt.tolist() == [SENTINEL] + w_next + [SENTINEL], key
                    assert fin_d.tolist() == w_fin + [False, True], key
                    seen_a.add(w_a)
    assert seen_m == set(range(k + 1)) and seen_a >= {1, min(2, k + 1), k + 1}
    # no history pointer, no EOS list
    pred, inp, fin = _accept_case(rng, B, k, "none", 0)
    w_out, _, w_next, w_a = SR.accept(pred, inp, fin, [], PAD_ID, k + 1)
    out = torch.full((B, ld), SENTINEL, dtype=torch.int64, device="cuda")
    nxt, taken = torch.zeros(B, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.spec_accept(torch.tensor(pred).cuda(), torch.tensor(inp).cuda(), k, torch.tensor(fin).cuda(), None, PAD_ID, k + 1, out, n, nxt, taken)
    torch.cuda.synchronize()
    assert int(taken) == w_a and out[:, n:n + w_a].cpu().tolist() == w_out and nxt.cpu().tolist() == w_next


def test_accept_kernel_rejections(hip):
    B, k = 2, 3
    pred = torch.zeros(B, k + 1, dtype=torch.int64, device="cuda")
    out = torch.full((B, 8), SENTINEL, dtype=torch.int64, device="cuda")
    hist = torch.full((B, 8), SENTINEL, dtype=torch.int64, device="cuda")
    fin = torch.zeros(B, dtype=torch.bool, device="cuda")
    nxt = torch.full((B,), SENTINEL, dtype=torch.int64, device="cuda")
    taken = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    n0 = hip.SPEC_ACCEPT_CALLS
    for name, kw in (("k", dict(k=8)), ("max_take", dict(max_take=0)), ("columns", dict(n=6, max_take=3)), ("columns", dict(n=-1)),
                     ("history columns", dict(hist=hist, hist_col=6, max_take=3))):
        a = dict(k=k, max_take=2, n=0, hist=None, hist_col=0)
        a.update(kw)
        p = torch.zeros(B, a["k"] + 1, dtype=torch.int64, device="cuda")
        with pytest.raises(RuntimeError, match=name) as ei:
            hip.spec_accept(p, p, a["k"], fin, None, PAD_ID, a["max_take"], out, a["n"], nxt, taken, hist=a["hist"], hist_col=a["hist_col"])
        assert "(-1)" in str(ei.value)                                       # DESTA_EINVAL
    torch.cuda.synchronize()
    assert hip.SPEC_ACCEPT_CALLS == n0
    assert all(bool((t == SENTINEL).all()) for t in (out, hist, nxt, taken)) and not bool(fin.any())     # nothing was launched
    hip.spec_accept(pred, pred, k, fin, None, PAD_ID, 2, out, 0, nxt, taken)
    torch.cuda.synchronize()
    assert hip.SPEC_ACCEPT_CALLS == n0 + 1 and int(taken) == 2               # every draft 0 == every prediction 0: limited by max_take


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("k", [3, 7])                                        # B (k + 1) = 12 and 24: both sides of the 16-row threshold
@pytest.mark.parametrize("weights", ["bf16", "fp8"])
@pytest.mark.parametrize("g4", [False, True])
def test_verify_step_vs_single_steps(hip, g4, weights, k):
    d, w, model = _model(g4)
    S, T = 61, k + 2
    inputs, ref, lo = _oracle(g4, S, 12)
    llm, w1 = model.llm, k + 1
    try:
        model.set_decode_weights(weights)
        model.set_speculative(None)
        _, lg = _gen(model, inputs, T, ref[:, :T])                           # prompt pass + k + 1 single steps on the oracle's tokens
        plain = [c[:, S:S + w1].clone() for c in llm.kv_cache]
        nw, n8 = hip.GEMM_WIDE_CALLS, hip.GEMM_W8_CALLS
        kv_start = torch.tensor(PADS[S], dtype=torch.int32, device="cuda")
        vl = llm.verify_step(ref[:, :w1].cuda(), S, kv_start).view(3, w1, -1)[:, :, :d.vocab].clone()
        torch.cuda.synchronize()
        assert (hip.GEMM_WIDE_CALLS > nw) == (3 * w1 > 16) and (hip.GEMM_W8_CALLS > n8) == (weights == "fp8" and 3 * w1 <= 16)
        e_plain = max(rel_err(lg[j + 1].float(), lo[j + 1]) for j in range(w1))
        e_v = max(rel_err(vl[:, j].float(), lg[j + 1].float()) for j in range(w1))
        e_kv = max(rel_err(c[:, S:S + w1].float(), p.float()) for c, p in zip(llm.kv_cache, plain))
        same_l = all(torch.equal(vl[:, j], lg[j + 1]) for j in range(w1))
        same_kv = all(torch.equal(c[:, S:S + w1], p) for c, p in zip(llm.kv_cache, plain))
        print(f"VERIFY_STEP G {d.llm_hq // d.llm_hkv} {weights} weights M {3 * w1}: logits rel-L2 verify vs single steps {e_v:.3e}, single steps vs "
              f"fp32 oracle {e_plain:.3e} (ratio {e_v / e_plain:.3f}); cache slots rel-L2 {e_kv:.3e}; bits equal: logits {same_l}, cache {same_kv}")
        assert bool(torch.isfinite(vl.float()).all())
        assert e_v <= 1.5 * e_plain, (e_v, e_plain)
        assert e_kv <= 1.5 * e_plain, (e_kv, e_plain)
    finally:
        model.set_decode_weights("bf16")
        model.set_speculative(None)


STEP_LAUNCHES = ("embed_gather", "rmsnorm_fwd", "gemm", "gemm_w8", "gemm_wide", "rope_kv_append", "attention_fwd", "attention_decode")


def _record_launches(hip, monkeypatch, step):
    """The launches of one step as a list, in order.  Projections: (name, M, N, K, act, a_rms_weight given, residual given); the
    row-wise kernels: (name, rows, width); the append additionally its rows per sequence; attention: (name, batch, seq_q, seq_k,
    causal)."""
    log = []

    def wrap(name, entry):
        real = getattr(hip, name)

        def f(*a, **kw):
            log.append((name,) + entry(*a, **kw))
            return real(*a, **kw)
        return f

    def proj(*a, act=0, a_rms_weight=None, residual=None, **kw):
        M, N, K = a[-3:]
        return (M, N, K, act, a_rms_weight is not None, residual is not None)

    def attn(d, *a):
        return (d.batch, d.seq_q, d.seq_k, d.causal)
    entries = dict(embed_gather=lambda table, audio, src, rows, hidden, out: (rows, hidden),
                   rmsnorm_fwd=lambda x, w, eps, y, rstd=None: (x.numel() // x.shape[-1], x.shape[-1]),
                   gemm=proj, gemm_w8=proj, gemm_wide=proj, rope_kv_append=lambda buf, ld, rows, seq, *a: (rows, ld, seq),
                   attention_fwd=attn, attention_decode=attn)
    assert sorted(entries) == sorted(STEP_LAUNCHES)
    with monkeypatch.context() as m:
        for name in STEP_LAUNCHES:
            m.setattr(hip, name, wrap(name, entries[name]))
        step()
        torch.cuda.synchronize()
    return log


def _without_what_differs(log):
    """The attention entry and the append's rows per sequence are meant to differ between the two widths."""
    return [("attention",) if e[0].startswith("attention") else e[:3] if e[0] == "rope_kv_append" else e for e in log]


@pytest.mark.parametrize("k", [3, 7])                                        # M = 12 and 24: both sides of the 16-row threshold
@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_verify_step_launches_what_decode_step_launches(hip, monkeypatch, weights, k):
    """`verify_step` at B = 3 with k drafts and `decode_step` at B = 3 (k + 1), each behind a prompt of S = 20, are one body over
    M = 3 (k + 1) rows: the same launches with the same shapes, epilogues and fusions in the same order, the attention apart."""
    d, w, model = _model(False)
    llm, S, w1 = model.llm, 20, k + 1
    M = 3 * w1
    gen = torch.Generator().manual_seed(k)
    toks = torch.randint(3, d.vocab, (M,), generator=gen).cuda()
    try:
        model.set_decode_weights(weights)
        model.set_speculative(None)
        pads = [0, 5, 11]
        _gen(model, _text_inputs(d, S, pads, seed=S)[2], k + 2)              # the prompt pass; the cache has room for slots [S, S + k]
        kv3 = torch.tensor(pads, dtype=torch.int32, device="cuda")
        ver = _record_launches(hip, monkeypatch, lambda: llm.verify_step(toks.view(3, w1), S, kv3))
        pads = [i % 7 for i in range(M)]
        _gen(model, _text_inputs(d, S, pads, seed=S)[2], 2)
        kvm = torch.tensor(pads, dtype=torch.int32, device="cuda")
        dec = _record_launches(hip, monkeypatch, lambda: llm.decode_step(toks, S, kvm))
    finally:
        model.set_decode_weights("bf16")
        model.set_speculative(None)
    L = d.llm_layers
    assert _without_what_differs(ver) == _without_what_differs(dec)
    names = {e[0] for e in ver}
    assert ("gemm_wide" in names) == (M > 16) and ("gemm_w8" in names) == (weights == "fp8" and M <= 16)
    assert [e for e in ver if e[0].startswith("attention")] == [("attention_fwd", 3, w1, S + w1, 1)] * L
    split = d.llm_hd == 128 and d.llm_hq // d.llm_hkv <= 8 and S + 1 >= hip.DECODE_ATTN_MIN_KEYS
    assert [e for e in dec if e[0].startswith("attention")] == [("attention_decode" if split else "attention_fwd", M, 1, S + 1, 0)] * L
    assert [e[3] for e in ver if e[0] == "rope_kv_append"] == [w1] * L and [e[3] for e in dec if e[0] == "rope_kv_append"] == [1] * L


# ---------------------------------------------------------------------------------------------------------------- 5
def _spec_gen(model, inputs, T, drafts=None):
    return model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[],
                                draft_tokens=drafts)


# Prompt seeds of the invariance test, chosen on the CPU with the oracle alone (the search walked seeds 1000, 1001, ... and kept the
# first with no near-tie): over all 3 x 24 (row, step) cases the fp32 oracle's top-2 gap / spread is at least MIN_TOP2.  The bf16
# path's logits sit within 6e-3 rel-L2 of the oracle's (module docstring of tests/test_gpu_prefill_chunk.py), which moves the
# difference of two logits by about sqrt(2) x 6e-3 = 0.009 of the spread: MIN_TOP2 is 2 - 3 times that, so no cut is expected.
SPEC_SEEDS = {(False, 61): 1237, (False, 251): 1038, (True, 61): 2187, (True, 251): 1134}
MIN_TOP2 = 0.03
_SPEC_ORACLE = {}


def _spec_oracle(g4, S, T):
    """(inputs, greedy ids, fp32 logits [T, B, V]) of the oracle on the prompt of SPEC_SEEDS: computed once."""
    if (g4, S) not in _SPEC_ORACLE:
        d, w, _ = _model(g4)
        ids, am, inputs = _text_inputs(d, S, PADS[S], seed=SPEC_SEEDS[(g4, S)])
        with torch.no_grad():
            ref, lo = O.greedy_generate(w, d, O.embed_splice(w, d, ids, None, [], []), am, T, 0)
        _SPEC_ORACLE[(g4, S)] = (inputs, ref, lo)
    return _SPEC_ORACLE[(g4, S)]


def _cut_against_oracle(tokens, ref, lo):
    """A row is compared with the oracle's greedy ids up to its first step where the two differ; the difference is excused, and
    the rest of the row cut, only if the ORACLE itself rates the other token within GAP_CUT of its maximum (gap / spread, the
    BF16_GAP_BOUND sense of tests/test_gpu_kv8_cache.py::_errors).  -> the cut fraction of the (row, step) cases."""
    T, B = lo.shape[0], lo.shape[1]
    cut = 0
    for b in range(B):
        for t in range(T):
            if tokens[b][t] != ref[b][t]:
                gap = float((lo[t, b].max() - lo[t, b, tokens[b][t]]) / lo[t, b].std())
                assert gap < GAP_CUT, (b, t, gap)
                cut += T - t
                break
    return cut / (B * T)


@pytest.mark.parametrize("S", [61, 251])
@pytest.mark.parametrize("g4", [False, True])
def test_output_does_not_depend_on_the_drafts(hip, g4, S):
    d, w, model = _model(g4)
    T, B = 24, 3
    inputs, ref, lo = _spec_oracle(g4, S, T)
    top2 = lo.topk(2, dim=-1).values
    assert float(((top2[..., 0] - top2[..., 1]) / lo.std(-1)).min()) >= MIN_TOP2      # the oracle alone: the chosen seed has no near-tie
    gen = torch.Generator().manual_seed(S)
    corrupt = ref.clone()
    for b in range(B):
        corrupt[b, 3 + 5 * b] = (corrupt[b, 3 + 5 * b] + 1) % d.vocab          # a different position per row
    sources = {"perfect": ref, "none": torch.full_like(ref, -1), "corrupt": corrupt,
               "random": torch.randint(0, d.vocab, ref.shape, generator=gen), "lookup": None}
    try:
        model.set_speculative(None)
        out_p, lg_p = _spec_gen(model, inputs, T)
        assert model.llm.spec_stats == dict(path="plain", reason="off", verify_steps=0, emitted=T, drafts_accepted=0)
        plain = out_p.cpu().tolist()
        removed = _cut_against_oracle(plain, ref.tolist(), lo)
        print(f"SPEC_INVARIANCE G {d.llm_hq // d.llm_hkv} S {S}: plain HIP run against the oracle's greedy ids: {removed:.3f} of the (row, step) cases cut")
        assert removed <= 0.10
        for k in (3, 7):
            model.set_speculative(k)
            _poison_free_memory()                                            # the verify buffers and the longer cache are made by the next run
            runs = {}
            for name, dr in sources.items():
                na, nd = hip.SPEC_ACCEPT_CALLS, hip.SPEC_DRAFT_CALLS
                out, lg = _spec_gen(model, inputs, T, dr)
                st = dict(model.llm.spec_stats)
                runs[name] = (out.cpu().tolist(), lg, st)
                assert bool(torch.isfinite(lg.float()).all()) and lg.shape == lo.shape == lg_p.shape, name
                assert st["path"] == "speculative" and st["reason"] is None and st["emitted"] == T, (name, st)
                assert st["drafts_accepted"] == T - 1 - st["verify_steps"] and hip.SPEC_ACCEPT_CALLS - na == st["verify_steps"], (name, st)
                assert hip.SPEC_DRAFT_CALLS - nd == (st["verify_steps"] if dr is None else 0), name
                assert model.llm.kv_cache[0].shape[1] == S + T + k
                print(f"SPEC_INVARIANCE G {d.llm_hq // d.llm_hkv} S {S} k {k} {name:8s}: {st['verify_steps']} verify steps, "
                      f"{st['drafts_accepted']} drafts accepted")
            first = runs["perfect"][0]
            for name, (toks, lg, st) in runs.items():
                assert toks == first, name                                   # the same tokens from every draft source
            assert first == plain                                            # ... the plain HIP loop's
            assert _cut_against_oracle(first, ref.tolist(), lo) <= 0.10      # ... and the oracle's
            if first == ref.tolist():                                        # (always, unless a cut applies)
                assert runs["perfect"][2]["verify_steps"] == math.ceil((T - 1) / (k + 1))
                for name, (toks, lg, st) in runs.items():
                    _check_against_oracle(lg, lo, T)
            else:
                assert removed > 0
            assert runs["none"][2]["verify_steps"] == T - 1 and runs["none"][2]["drafts_accepted"] == 0
            assert runs["corrupt"][2]["verify_steps"] > runs["perfect"][2]["verify_steps"]
            out2, lg2 = _spec_gen(model, inputs, T, sources["corrupt"])      # two identical runs: the same bits
            assert out2.cpu().tolist() == runs["corrupt"][0] and torch.equal(lg2, runs["corrupt"][1])
    finally:
        model.set_speculative(None)


# ---------------------------------------------------------------------------------------------------------------- 6
def _counters(hip):
    return {n: getattr(hip, n) for n in dir(hip) if n.endswith("_CALLS")}


def test_fallbacks_run_the_plain_loop(hip):
    d, w, model = _model(False)
    S, T = 61, 8
    inputs, ref, _ = _oracle(False, S, 12)
    llm = model.llm

    def run(**kw):
        a = dict(pad_token_id=0, max_new_tokens=T, do_sample=False, eos_token_id=[])
        a.update(kw)
        c0 = _counters(hip)
        res = model._generate_step(inputs, **a)
        res = res if isinstance(res, tuple) else (res,)
        c1 = _counters(hip)
        flat = []
        for r in res:
            flat += [r] if torch.is_tensor(r) else [r.token_logprobs, r.top_ids, r.top_logprobs]
        return [t.clone() for t in flat], {n: c1[n] - c0[n] for n in c0}
    cases = {"do_sample": dict(do_sample=True, temperature=0.8, top_p=0.9, seed=3), "repetition_penalty": dict(repetition_penalty=1.3),
             "logprobs": dict(logprobs=2), "forced_tokens": dict(forced_tokens=ref[:, :T])}
    try:
        model.set_speculative(None)
        base = {name: run(**kw) for name, kw in cases.items()}
        base["plain"] = run()
        model.set_kv_cache("fp8")
        base["fp8 kv cache"] = run()
        model.set_kv_cache("bf16")
        model.set_speculative(3)
        for name, kw in cases.items():
            got, cnt = run(**kw)
            assert llm.spec_stats["path"] == "plain" and llm.spec_stats["reason"] == name, llm.spec_stats
            assert cnt == base[name][1] and cnt["SPEC_ACCEPT_CALLS"] == 0, name
            assert all(torch.equal(a, b) for a, b in zip(got, base[name][0])), name
        model.set_kv_cache("fp8")
        got, cnt = run()
        assert llm.spec_stats["path"] == "plain" and llm.spec_stats["reason"] == "fp8 kv cache"
        assert cnt == base["fp8 kv cache"][1] and torch.equal(got[0], base["fp8 kv cache"][0][0])
        model.set_kv_cache("bf16")
        got, cnt = run()                                                     # no fallback: the speculative path, the plain tokens
        assert llm.spec_stats["path"] == "speculative" and cnt["SPEC_ACCEPT_CALLS"] == llm.spec_stats["verify_steps"] > 0
        assert got[0].cpu().tolist() == base["plain"][0][0].cpu().tolist()
        # B (k + 1) = 17 x 4 = 68 > 64 rows
        wide = _text_inputs(d, 20, list(range(17)), seed=5)[2]
        model.set_speculative(None)
        o0 = model._generate_step(wide, pad_token_id=0, max_new_tokens=4, do_sample=False, eos_token_id=[])
        model.set_speculative(3)
        o1 = model._generate_step(wide, pad_token_id=0, max_new_tokens=4, do_sample=False, eos_token_id=[])
        assert llm.spec_stats["path"] == "plain" and "68 rows" in llm.spec_stats["reason"] and torch.equal(o0, o1)
        model.set_speculative(None)                                          # off again: today's launches, today's bits
        got, cnt = run()
        assert llm._spec is None and llm.spec_stats["reason"] == "off"
        assert cnt == base["plain"][1] and torch.equal(got[0], base["plain"][0][0])
    finally:
        model.set_kv_cache("bf16")
        model.set_speculative(None)


def test_orca_model_falls_back(hip, golden_dir):
    """The inputs of tests/test_gpu_kv8_cache.py::test_fp8_cache_with_orca_injection: the deep injection is a `layer_hook`."""
    import orca_oracle as RO
    from safetensors.torch import load_file
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    g = load_file(os.path.join(golden_dir, "ref_orca_tiny.safetensors"))
    kg, ds, ks, ntr = (int(x) for x in g["orca_dims"])
    d = copy.copy(O.tiny_dims(True))
    d.prompt_size = kg + ntr
    o = RO.OrcaDims(global_num_tokens=kg, local_downsample=ds, local_kernel_size=ks, ortho_diversity_weight=0.05,
                    ortho_weight_qformer_local=0.05, align_weight_local=0.05, global_cross_attn=False, local_enabled=True)
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=ds,
                        orca_local_kernel_size=ks, orca_ortho_diversity_weight=0.05, orca_ortho_weight_qformer_local=0.05,
                        orca_align_weight_local=0.05, orca_rope_theta=float(g["rope_theta_used"]), orca_global_cross_attn=False, orca_local_enabled=True)
    n_ctx, n = int(g["gen_ctx_len"]), g["starts"].shape[0]
    inputs = {"context_input_ids": g["input_ids"][:, :n_ctx], "context_attention_mask": g["attention_mask"][:, :n_ctx],
              "context_batch_start_positions": [(int(b), int(p)) for b, p in g["starts"].tolist()], "batch_features": g["batch_features"],
              "batch_transcription_ids": [g["transcription_ids"][i:i + 1] for i in range(n)]}
    model = DeSTA25AudioModel(cfg, weights=RO.init_weights(d, o, seed=7)).eval()
    ids0, lg0 = _gen(model, inputs, 6)
    model.set_speculative(3)
    na = hip.SPEC_ACCEPT_CALLS
    ids1, lg1 = _gen(model, inputs, 6)
    assert model.llm.spec_stats["path"] == "plain" and model.llm.spec_stats["reason"] == "layer_hook" and hip.SPEC_ACCEPT_CALLS == na
    assert torch.equal(ids0, ids1) and torch.equal(lg0, lg1)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_chat_level_generate_gives_the_same_text(hip):
    from helpers import ToyTokenizer
    d, w, model = _model(False)
    model._setup_generation(tokenizer=ToyTokenizer(vocab_size=d.vocab), processor=object())
    phrase = "the quick brown fox jumps over the lazy dog"
    msgs = [[{"role": "user", "content": f"repeat after me : {phrase} . {phrase} . {phrase} . now you :"}],
            [{"role": "user", "content": f"say {phrase} twice"}]]
    try:
        model.set_speculative(None)
        a = model.generate(msgs, do_sample=False, max_new_tokens=20)
        model.set_speculative(3)
        b = model.generate(msgs, do_sample=False, max_new_tokens=20)
        st = model.llm.spec_stats
        print(f"SPEC_CHAT: {st['emitted']} tokens in {st['verify_steps']} verify steps, {st['drafts_accepted']} lookup drafts accepted "
              "(random weights: the acceptance says nothing about a trained model)")
        assert st["path"] == "speculative" and hip.SPEC_DRAFT_CALLS > 0
        assert a.text == b.text and a.generated_ids == b.generated_ids
        model.generate(msgs, do_sample=True, max_new_tokens=4)               # the default sampling call: the plain loop
        assert model.llm.spec_stats["path"] == "plain" and model.llm.spec_stats["reason"] == "do_sample"
    finally:
        model.set_speculative(None)
