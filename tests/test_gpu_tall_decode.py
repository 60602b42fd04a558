"""GPU: opt-in decode at 65..256 rows — the tall weight-streaming projection (desta_gemm_tall_nt) and the KV-cached step on top of it
after `set_decode_rows`.

Kernel: against bf16(fp64 product) within the wide kernel's bound (1 bf16 ulp at the larger magnitude + 1e-3; the slice loop of
`gemm_wide` on the same operands is held to it in the same test) at the shapes where it can go wrong: one row in the second row
group, ragged N, an odd chunk count cut into K-slices, the first M of the four-group class, and two true widths.  Exact properties:
reruns, persistent grids, row permutations, M inside a row-group class (65..128 and 129..256 each share one summation order), act 4
against the plain GEMM + swiglu kernel, FP8 against bf16 on the dequantised weight; rejections.
Model: text-only Llama / Qwen3 at B = 80 and 136 and the golden audio batch at 72 rows against the fp32 oracles, FP8 weights on the
FP8 grid, guidance at 80 rows, speculation at 96 rows, and the ceilings."""

import pytest
import torch

import desta_oracle as O
from helpers import cfg_from_dims, golden_batch
from test_gpu_wide_decode import _ab, _bf, _check_against_oracle, _grids, _quantize, _repeat_batch, _text_batch

pytestmark = pytest.mark.gpu

PLAIN = [(65, 16, 64), (97, 100, 192), (128, 36, 64 * 37), (129, 1028, 2048), (255, 64, 256), (200, 4096, 4096), (256, 4096, 14336)]
SWIGLU = [(65, 104, 192), (136, 512, 2048), (256, 14336, 4096)]              # the middle one is cut into two K-slices: slab stores + SwiGLU fix-up


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _tall(hip, A, B, M, N, K, fill_rows=0, **kw):
    out = torch.full((M + fill_rows, kw.get("ldc", N)), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.gemm_tall(A, B, out, M, N, K, lda=A.stride(0), **kw)
    return out


def _wide_loop(hip, A, B, M, N, K):
    """The only way the 64-row kernel runs these M: one launch per slice of at most 64 rows (17 at the least)."""
    out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    m0 = 0
    while m0 < M:
        m = min(64, M - m0)
        if m < 17:                                                           # the last slice borrows rows from the one before
            m0, m = M - 17, 17
        hip.gemm_wide(A[m0:], B, out[m0:], m, N, K, lda=A.stride(0))
        m0 += m
    return out


def _worst(got, ref64):
    got = got.double()
    big = torch.maximum(got.abs(), ref64.abs()).clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(big)) - 7)                       # one bf16 step at the larger magnitude
    return float(((got - ref64).abs() / (ulp + 1e-3)).max())


@pytest.mark.parametrize("M,N,K", PLAIN)
def test_tall_vs_fp64(hip, M, N, K):
    A, B, g = _ab(M, N, K, M * 11 + N + K, gain=1.0)
    res = _bf(torch.randn(M, N, generator=g)).cuda()
    ref = A.float() @ B.float().T
    outr = _tall(hip, A, B, M, N, K, fill_rows=1, residual=res, alpha=0.5)
    torch.testing.assert_close(outr[:M].float(), 0.5 * ref + res.float(), rtol=1e-2, atol=1e-2)
    assert bool((outr[M] == 7.0).all())                                      # the guard row beyond M keeps its fill value
    out = _tall(hip, A, B, M, N, K, fill_rows=1)
    assert bool((out[M] == 7.0).all())
    ref64 = (A.double() @ B.double().T).bfloat16().double()                  # bf16(fp64 product)
    worst, worst_wide = _worst(out[:M], ref64), _worst(_wide_loop(hip, A, B, M, N, K), ref64)
    print(f"vs bf16(fp64) M={M} N={N} K={K}: tall {worst:.3f}, gemm_wide slice loop {worst_wide:.3f} of the bound (1 ulp + 1e-3)")
    assert worst <= 1.0 and worst_wide <= 1.0
    ldc = N + 12                                                             # strided output rows (the lm_head writes [B, Vp])
    o2 = _tall(hip, A, B, M, N, K, ldc=ldc)
    assert torch.equal(o2[:, :N], out[:M]) and bool((o2[:, N:] == 7.0).all())


@pytest.mark.parametrize("M,N,K", PLAIN)
def test_tall_exact_properties(hip, M, N, K):
    A, B, g = _ab(M, N, K, M * 7 + N + K)
    res = _bf(torch.randn(M, N, generator=g)).cuda()
    first = _tall(hip, A, B, M, N, K, residual=res)
    for out in _grids(hip, lambda: _tall(hip, A, B, M, N, K, residual=res)):  # rerun + every grid: the same bits
        assert torch.equal(out, first)
    perm = torch.randperm(M, generator=g).cuda()                             # rows are independent of their position
    Ap = A[perm].contiguous()
    outp = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm_tall(Ap, B, outp, M, N, K, residual=res[perm].contiguous())
    assert torch.equal(outp, first[perm])


@pytest.mark.parametrize("N,K", [(100, 192), (1028, 2048), (4096, 4096)])
@pytest.mark.parametrize("m,M", [(100, 128), (65, 128), (200, 256), (129, 256)])
def test_tall_rows_do_not_depend_on_m_inside_a_class(hip, m, M, N, K):
    """65..128 rows run two row groups, 129..256 four: inside a class a row's bits are those of any other M."""
    A, B, g = _ab(M, N, K, N + K + M)
    assert torch.equal(_tall(hip, A, B, m, N, K), _tall(hip, A, B, M, N, K)[:m])


@pytest.mark.parametrize("M,I,K", SWIGLU)
def test_tall_swiglu_equals_plain_then_swiglu_kernel(hip, M, I, K):
    A, W, g = _ab(M, 2 * I, K, M + I)
    gu = _tall(hip, A, W, M, 2 * I, K)
    ref = torch.empty(M, I, dtype=torch.bfloat16, device="cuda")
    hip.swiglu_fwd(gu, ref, M, I)
    for out in _grids(hip, lambda: _tall(hip, A, W, M, I, K, fill_rows=1, act=4)):
        assert torch.equal(out[:M], ref)
        assert bool((out[M] == 7.0).all())


@pytest.mark.parametrize("M,N,K", PLAIN)
def test_tall_fp8_equals_bf16_on_dequantised_weight(hip, M, N, K):
    A, W, g = _ab(M, N, K, M * 13 + N + K)
    q, s, Wd = _quantize(hip, W)
    res = _bf(torch.randn(M, N, generator=g)).cuda()
    ref = _tall(hip, A, Wd, M, N, K, residual=res, alpha=0.5)
    for out in _grids(hip, lambda: _tall(hip, A, q, M, N, K, scale=s, residual=res, alpha=0.5)):
        assert torch.equal(out, ref)


@pytest.mark.parametrize("M,I,K", SWIGLU)
def test_tall_fp8_swiglu_equals_bf16(hip, M, I, K):
    """act 4: gate rows and up rows carry different scales."""
    A, W, g = _ab(M, 2 * I, K, M + 3 * I)
    W[I:] *= 4.0
    q, s, Wd = _quantize(hip, W)
    assert bool((s[I:] != s[:I]).any())
    ref = _tall(hip, A, Wd, M, I, K, act=4)
    for out in _grids(hip, lambda: _tall(hip, A, q, M, I, K, scale=s, act=4)):
        assert torch.equal(out, ref)


def test_tall_rejections(hip):
    K, N = 256, 64
    A = torch.zeros(257, K, dtype=torch.bfloat16, device="cuda")
    B = torch.zeros(2 * N, K, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(257, N, dtype=torch.bfloat16, device="cuda")
    n0 = hip.GEMM_TALL_CALLS
    with pytest.raises(RuntimeError, match="gemm_tall: M=64"):
        hip.gemm_tall(A, B, out, 64, N, K)
    with pytest.raises(RuntimeError, match="gemm_tall: M=257"):
        hip.gemm_tall(A, B, out, 257, N, K)
    with pytest.raises(RuntimeError, match="gemm_tall: act 2"):
        hip.gemm_tall(A, B, out, 128, N, K, act=2)
    with pytest.raises(RuntimeError, match="gemm_tall: fp32 output"):
        hip.gemm_tall(A, B, torch.zeros(128, N, device="cuda"), 128, N, K)
    d = hip.GemmDesc()                                                       # a bias: the binding has no argument for one
    d.A, d.B, d.C, d.M, d.N, d.K, d.batch = hip.p(A), hip.p(B), hip.p(out), 128, N, K, 1
    d.lda, d.ldb, d.ldc, d.ldr, d.ldp, d.alpha = K, K, N, N, N, 1.0
    d.bias = hip.p(torch.zeros(N, device="cuda"))
    with pytest.raises(RuntimeError, match="gemm_tall: bias"):
        hip.check(hip._gemm_tall(d, 0, hip.stream()), "desta_gemm_tall_nt")
    assert hip.GEMM_TALL_CALLS == n0
    with pytest.raises(RuntimeError, match="gemm_wide: M=65"):               # the 64-row entry point keeps its limit
        hip.gemm_wide(A, B, out, 65, N, K)
    hip.gemm_tall(A, B, out, 65, N, K)                                       # ... and M = 65 and 256 are served
    hip.gemm_tall(A, B, out, 256, N, K)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- model level
def _model(d, w, rows=256):
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    model.set_decode_rows(rows)
    return model


@pytest.mark.parametrize("qwen", [False, True])
@pytest.mark.parametrize("B", [80, 136])
def test_tall_decode_text_only_vs_oracle(qwen, B):
    from desta import _hip as H
    from test_gpu_wide_decode import _text_reference
    T = 12
    d, w, inputs, ref, lo = _text_reference(qwen, B, T)
    model = _model(d, w)
    n0, w0 = H.GEMM_TALL_CALLS, H.GEMM_WIDE_CALLS
    out, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref, collect_logits=True,
                                       eos_token_id=[])
    assert H.GEMM_TALL_CALLS - n0 == (T - 1) * (4 * d.llm_layers + 1)        # q|k|v, o, gate|up, down per layer + the lm_head, per decode step
    assert H.GEMM_WIDE_CALLS == w0
    assert out.cpu().tolist() == ref.tolist() and logits.shape == lo.shape
    _check_against_oracle(logits, lo, T)


MIN_TOP2 = 0.03            # top-2 gap / spread under the fp32 oracle from which a bf16 pick has to agree (tests/test_gpu_speculative.py)


def test_tall_decode_golden_audio_at_72_rows(golden_dir):
    """More than 64 audios: the encoder and the connector run in two slices.  The golden batch repeated to 72 rows is decoded as
    the project decodes against a reference's tokens (tests/test_gpu_generate.py (a), test_wide_decode_with_audio_qformer_vs_oracle):
    teacher-forced on the golden's `gen_ids`.  Every copy returns the golden's tokens, every copy of a row has the SAME logits bit
    for bit (36 copies, in both encoder slices and in both row groups), the logits follow the fp32 oracle within the bounds of
    `_check_against_oracle`, and the model's own pick (argmax of its logits) IS the golden's token in every cell where the fp32
    oracle is decisive: top-2 gap / spread >= MIN_TOP2 = 0.03, three times the 0.009 of the spread by which 6e-3 relative L2
    moves a difference of two logits (the reasoning of SPEC_SEEDS there).  Then free running: every copy of a row gives the same
    tokens, those of the default 2-row path, the golden's first token, and near-optimal picks under the oracle on the run's own
    prefix (tests/test_gpu_generate.py (b)).
    Equality of the FREE-RUNNING tokens with `gen_ids` is not asserted: under the fp32 oracle alone golden row 1 has a top-2 gap
    of 0.0019 of the spread at step 2 (qwen3's golden: 0.0015 in row 0), bf16 arithmetic decides it the other way on the
    default 2-row path as well, and the rest of the row
    then differs legitimately.  Both figures are printed."""
    from desta import _hip as H
    from test_gpu_generate import _gen_inputs, _oracle_logits
    T = 10
    d = O.tiny_dims(False)
    g, batch = golden_batch(golden_dir, "llama")
    gold = g["gen_ids"]
    inputs = _repeat_batch(batch, int(g["gen_ctx_len"]), 72)
    Bn, B0 = inputs["context_input_ids"].shape[0], batch["input_ids"].shape[0]
    r = Bn // B0
    assert Bn >= 72 and len(inputs["context_batch_start_positions"]) > 64 and gold.shape == (B0, T)
    w = O.init_weights(d, seed=7)
    model = _model(d, w)
    # teacher-forced on the golden's tokens
    n0 = H.GEMM_TALL_CALLS
    out, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=gold.repeat(r, 1),
                                       collect_logits=True)
    assert H.GEMM_TALL_CALLS - n0 == (T - 1) * (4 * d.llm_layers + 1)
    assert out.cpu().tolist() == gold.repeat(r, 1).tolist()                  # every copy: the golden's tokens
    lg = logits.reshape(T, r, B0, -1)
    for j in range(1, r):
        assert torch.equal(lg[:, j], lg[:, 0]), j                            # every copy of a row: the same logits, bit for bit
    lo = _oracle_logits(w, d, g, batch, gold)                                # [T, B0, V]
    _check_against_oracle(logits, lo.repeat(1, r, 1), T)
    top2 = lo.topk(2, dim=-1).values
    decisive = (top2[..., 0] - top2[..., 1]) / lo.std(-1) >= MIN_TOP2        # [T, B0], from the oracle alone
    pick = lg[:, 0].float().cpu().argmax(-1)
    print(f"teacher-forced: {int(decisive.sum())} of {decisive.numel()} cells decisive under the oracle, "
          f"picks equal to the golden's in {int((pick == gold.t()).sum())} cells")
    assert int(decisive.sum()) >= decisive.numel() // 2
    assert torch.equal(pick[decisive], gold.t()[decisive])                   # the model's own pick is the golden's wherever fp32 decides
    # free running
    ids = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False).cpu()
    lo2 = _oracle_logits(w, d, g, batch, ids[:B0])
    two = _model(d, w, rows=None)._generate_step(_gen_inputs(g, batch), pad_token_id=0, max_new_tokens=T, do_sample=False).cpu()
    for b in range(B0):
        diff = (ids[b] != gold[b]).nonzero()
        t = int(diff[0]) if diff.numel() else None
        gap = None if t is None else float((lo2[t, b].max() - lo2[t, b, ids[b, t]]) / lo2[t, b].std())
        print(f"free running, golden row {b}: first step off the golden's tokens {t}, oracle gap / spread of the pick there {gap}")
    for b in range(Bn):
        assert ids[b].tolist() == ids[b % B0].tolist(), b                   # every copy of a row: the same tokens
    assert ids[:B0].tolist() == two.tolist()                                 # ... those of the default 2-row path
    assert (ids[:B0, 0] == gold[:, 0]).all()
    gap2 = lo2.max(-1).values - lo2.gather(-1, ids[:B0].t().unsqueeze(-1)).squeeze(-1)
    assert float((gap2 / lo2.std(-1)).max()) < 0.1                           # every pick near-optimal under the fp32 oracle on its own prefix


def test_tall_decode_fp8_equals_bf16_on_snapped_weights():
    from desta import _hip as H
    from test_gpu_wide_decode import _text_reference
    T = 12
    d, w, inputs, ref, lo = _text_reference(False, 80, T, snapped=True)
    model = _model(d, w)
    n0, w0 = H.GEMM_TALL_CALLS, H.GEMM_W8_CALLS
    ids_b, lg_b = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[])
    model.set_decode_weights("fp8")
    ids_f, lg_f = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[])
    assert H.GEMM_TALL_CALLS - n0 == 2 * (T - 1) * (4 * d.llm_layers + 1) and H.GEMM_W8_CALLS == w0
    assert all("q8" in ly for ly in model.llm.layers) and model.llm.head8 is not None
    assert torch.equal(ids_b, ids_f)
    for t in range(T):
        assert torch.equal(lg_b[t], lg_f[t]), t


def test_tall_decode_guidance_at_80_rows():
    """Bc = 40: conditional prompts, then 40 other prompts as the unconditional rows.  The picks are the fp64 guided argmax of the
    run's own logits wherever tests/guidance_reference.py's bound decides the cell, and all 80 rows follow the oracle."""
    import guidance_reference as GR
    from desta import _hip as H
    T, Bc, g = 8, 40, 3.0
    d = O.tiny_dims(False)
    w = O.init_weights(d, seed=7)
    ids, am, inputs = _text_batch(d, 2 * Bc, 13, seed=5)
    model = _model(d, w)
    n0, c0 = H.GEMM_TALL_CALLS, H.CFG_SCORES_CALLS
    out, lg = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[], guidance_scale=g)
    assert out.shape == (Bc, T) and lg.shape == (T, 2 * Bc, d.vocab)
    assert H.GEMM_TALL_CALLS - n0 == (T - 1) * (4 * d.llm_layers + 1) and H.CFG_SCORES_CALLS - c0 == T
    want, counts = GR.pick_cells(lg, g)
    got = out.cpu().t()
    print(f"guidance at 80 rows: cells counting {float(counts.float().mean()):.2f}")
    assert torch.equal(got[counts], want[counts]) and float(counts.float().mean()) >= 0.75
    with torch.no_grad():
        forced = torch.cat([out.cpu(), out.cpu()])
        lo = O.greedy_generate(w, d, O.embed_splice(w, d, ids, None, [], []), am, T, 0, forced_tokens=forced)[1]
    _check_against_oracle(lg, lo, T)
    ids2, _, inputs2 = _text_batch(d, 2 * 129, 9, seed=6)                    # 258 rows: over the ceiling of 256
    with pytest.raises(ValueError, match=r"guidance_scale doubles the rows.*129 sequences are 258 rows.*256"):
        model._generate_step(inputs2, pad_token_id=0, max_new_tokens=4, do_sample=False, guidance_scale=g)


def test_tall_decode_speculation_at_96_rows():
    """B = 24, k = 3: verify steps of 96 rows.  Their logits follow the oracle teacher-forced on the run's own tokens (the verify
    step and the plain step run different kernels at these rows, so token equality with the plain loop is not asserted)."""
    from desta import _hip as H
    from test_gpu_wide_decode import _text_reference
    T, B, k = 12, 24, 3
    d, w, inputs, ref, lo = _text_reference(False, B, T)
    model = _model(d, w)
    model.set_speculative(k)
    n0, a0, dr0 = H.GEMM_TALL_CALLS, H.SPEC_ACCEPT_CALLS, H.SPEC_DRAFT_CALLS
    out, lg = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[],
                                   draft_tokens=ref)
    st = dict(model.llm.spec_stats)
    print("speculation at 96 rows:", st)
    assert st["path"] == "speculative" and st["reason"] is None and st["emitted"] == T and st["verify_steps"] > 0
    assert H.SPEC_ACCEPT_CALLS - a0 == st["verify_steps"] and H.SPEC_DRAFT_CALLS == dr0      # the drafts came from `draft_tokens`
    assert H.GEMM_TALL_CALLS - n0 == st["verify_steps"] * (4 * d.llm_layers + 1)
    ids, am = inputs["context_input_ids"], inputs["context_attention_mask"]
    with torch.no_grad():
        lo2 = O.greedy_generate(w, d, O.embed_splice(w, d, ids, None, [], []), am, T, 0, forced_tokens=out.cpu())[1]
    assert lg.shape == lo2.shape
    _check_against_oracle(lg, lo2, T)


def test_tall_decode_ceilings():
    from desta import _hip as H
    d = O.tiny_dims(False)
    model = _model(d, O.init_weights(d, seed=7))
    _, _, inputs = _text_batch(d, H.DECODE_TALL_MAX_ROWS + 1, 9, seed=1)
    model.llm._gen_shape = None
    n0 = H.GEMM_TALL_CALLS
    with pytest.raises(ValueError, match="257 sequences.*256"):
        model._generate_step(inputs, pad_token_id=0, max_new_tokens=4, do_sample=False)
    assert getattr(model.llm, "_gen_shape", None) is None                    # raised before the caches were allocated and the prompt pass ran
    model.set_decode_weights("mxfp4")
    _, _, inputs = _text_batch(d, 65, 9, seed=1)
    with pytest.raises(ValueError, match="MXFP4"):
        model._generate_step(inputs, pad_token_id=0, max_new_tokens=4, do_sample=False)
    assert getattr(model.llm, "_gen_shape", None) is None and H.GEMM_TALL_CALLS == n0
    plain = _model(d, O.init_weights(d, seed=7), rows=None)                  # a default model keeps today's ceiling
    with pytest.raises(ValueError):
        plain._generate_step(inputs, pad_token_id=0, max_new_tokens=4, do_sample=False)


# ------------------------------------------------------------------------------------------ the bf16 route to the tile GEMM
def _lower_route(monkeypatch):
    """The routing rule at the tiny models' widths: the thresholds that sit at 8192 / 6144 weight rows are lowered to 1024 / 512,
    so gate|up (1024 rows) takes `H.gemm` + `swiglu_fwd` at every M, the lm_head (512, ldc = Vp) and a 512-row q|k|v above 128 rows
    (a 1024-row q|k|v at every M), and o / down (256) stay on `gemm_tall`."""
    import desta.models.modeling_desta25 as MD
    monkeypatch.setattr(MD, "TALL_GEMM_ROWS", 1024)
    monkeypatch.setattr(MD, "TALL_GEMM_ROWS_ABOVE_128", 512)
    return MD


def _unrouted(MD, llm, M):
    """Projections of one step of M rows that stay on `gemm_tall` under the rule as it stands."""
    rows = [llm.qkvw, llm.h, 2 * llm.I, llm.h] * llm.L + [llm.V]
    return sum(not MD.tall_rows_to_gemm(M, r) for r in rows)


@pytest.mark.parametrize("qwen", [False, True])
@pytest.mark.parametrize("B", [80, 136])
def test_tall_decode_routed_to_gemm_vs_oracle(monkeypatch, qwen, B):
    from desta import _hip as H
    from test_gpu_wide_decode import _text_reference
    MD = _lower_route(monkeypatch)
    T = 12
    d, w, inputs, ref, lo = _text_reference(qwen, B, T)
    model = _model(d, w)
    per_step = _unrouted(MD, model.llm, B)
    assert 2 * d.llm_layers <= per_step < 4 * d.llm_layers + 1               # o and down stay, gate|up leaves
    n0, w0 = H.GEMM_TALL_CALLS, H.GEMM_WIDE_CALLS
    out, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref, collect_logits=True,
                                       eos_token_id=[])
    assert H.GEMM_TALL_CALLS - n0 == (T - 1) * per_step and H.GEMM_WIDE_CALLS == w0
    assert model.llm._step1["gu"].shape == (B, 2 * d.llm_inter)              # the route's gate|up buffer, made by the first routed step
    assert out.cpu().tolist() == ref.tolist() and logits.shape == lo.shape
    _check_against_oracle(logits, lo, T)
    model.set_decode_weights("fp8")                                          # FP8 weights: nothing is routed, no buffer is made
    model.llm._gen_shape = None
    n1 = H.GEMM_TALL_CALLS
    model._generate_step(inputs, pad_token_id=0, max_new_tokens=3, do_sample=False, eos_token_id=[])
    assert H.GEMM_TALL_CALLS - n1 == 2 * (4 * d.llm_layers + 1) and model.llm._step1.get("gu") is None


@pytest.mark.parametrize("B", [20, 34])
def test_tall_verify_step_routed_to_gemm_vs_oracle(monkeypatch, B):
    """`verify_step` at B (k + 1) = 80 and 136 rows through the route: its logits follow the oracle on the run's own tokens."""
    from desta import _hip as H
    from test_gpu_wide_decode import _text_reference
    MD = _lower_route(monkeypatch)
    T, k = 12, 3
    d, w, inputs, ref, lo = _text_reference(False, B, T)
    model = _model(d, w)
    model.set_speculative(k)
    per_step = _unrouted(MD, model.llm, B * (k + 1))
    n0 = H.GEMM_TALL_CALLS
    out, lg = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[],
                                   draft_tokens=ref)
    st = dict(model.llm.spec_stats)
    print(f"routed verify steps at {B * (k + 1)} rows:", st)
    assert st["path"] == "speculative" and st["reason"] is None and st["verify_steps"] > 0
    assert H.GEMM_TALL_CALLS - n0 == st["verify_steps"] * per_step
    assert model.llm._spec["gu"].shape == (B * (k + 1), 2 * d.llm_inter)
    ids, am = inputs["context_input_ids"], inputs["context_attention_mask"]
    with torch.no_grad():
        lo2 = O.greedy_generate(w, d, O.embed_splice(w, d, ids, None, [], []), am, T, 0, forced_tokens=out.cpu())[1]
    _check_against_oracle(lg, lo2, T)
