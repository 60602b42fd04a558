"""GPU: decode at batch 17..64 — the wide weight-streaming projections (desta_gemm_wide_nt) and the decode step on top of them.

Kernel: against torch fp32 and fp64 at the shapes where it can go wrong (one row in a new 16-row fragment, a full last fragment,
N ragged to 4, one K-chunk, an odd chunk count that is no multiple of the 8 waves, and the two true decode shapes that are cut into
K-slices), exact properties (reruns, persistent-grid sizes, M = 40 against M = 64, row permutations), act 4 against the plain
GEMM + swiglu kernel and the FP8 form against the bf16 form on the dequantised weight, all bit for bit; rejections.
Model: B = 24 / 40 text-only and >= 17 repeated golden rows with audio against the fp32 oracles within the bounds
tests/test_gpu_generate.py holds the 16-row path to; FP8 weights equal bf16 weights on the FP8 grid; B = 65 raises.
Measured (MI355X, this file's shapes): bf16 output against bf16(fp64 product), worst |diff| in units of the bound
(1 bf16 ulp of the larger magnitude + 1e-3) — printed by test_wide_vs_torch, copied into DESIGN.md."""
import math

import pytest
import torch

import desta_oracle as O
from helpers import cfg_from_dims, golden_batch, rel_err

pytestmark = pytest.mark.gpu

PLAIN = [(17, 16, 64), (33, 100, 192), (48, 36, 64 * 37), (64, 1028, 2048), (24, 4096, 4096), (64, 4096, 14336)]
SWIGLU = [(17, 104, 192), (40, 512, 256), (64, 14336, 4096), (40, 512, 2048)]     # the last one is cut into two K-slices: slab stores + SwiGLU fix-up


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _bf(x):
    return x.to(torch.bfloat16)


def _ab(M, N, K, seed, gain=2.0):
    """A [M, K] with rows strided by 3K, weight [N, K] / sqrt(K) (the scaling of test_gemm_skinny), generator."""
    g = torch.Generator().manual_seed(seed)
    Abig = _bf(torch.randn(M, 3, K, generator=g)).cuda()
    B = _bf(torch.randn(N, K, generator=g) / math.sqrt(K) * gain).cuda()
    return Abig[:, 1], B, g


def _wide(hip, A, B, M, N, K, fill_rows=0, **kw):
    out = torch.full((M + fill_rows, kw.get("ldc", N)), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.gemm_wide(A, B, out, M, N, K, lda=A.stride(0), **kw)
    return out


def _grids(hip, fn):
    """fn() at the default persistent grid and at 7 / 64 / 512 blocks (option 3)."""
    outs = [fn()]
    try:
        for blocks in (7, 64, 512):
            hip.gemm_set_option(3, blocks)
            outs.append(fn())
    finally:
        hip.gemm_set_option(3, 512)
    return outs


def _quantize(hip, W):
    """(q, scale, bf16(q * scale)) of a bf16 device weight; the product is exact in bf16 (desta_quantize_rows_e4m3)."""
    q, s = hip.quantize_rows_e4m3(W)
    d = q.view(torch.float8_e4m3fn).float() * s[:, None]
    Wd = d.bfloat16()
    assert torch.equal(Wd.float(), d)
    return q, s, Wd


@pytest.mark.parametrize("M,N,K", PLAIN)
def test_wide_vs_torch(hip, M, N, K):
    A, B, g = _ab(M, N, K, M * 11 + N + K, gain=1.0)
    res = _bf(torch.randn(M, N, generator=g)).cuda()
    ref = A.float() @ B.float().T
    outr = _wide(hip, A, B, M, N, K, fill_rows=1, residual=res, alpha=0.5)
    torch.testing.assert_close(outr[:M].float(), 0.5 * ref + res.float(), rtol=1e-2, atol=1e-2)
    assert bool((outr[M] == 7.0).all())                                      # the guard row beyond M keeps its fill value
    out = _wide(hip, A, B, M, N, K, fill_rows=1)
    assert bool((out[M] == 7.0).all())
    ref64 = (A.double() @ B.double().T).bfloat16().double()                  # bf16(fp64 product)
    got = out[:M].double()
    big = torch.maximum(got.abs(), ref64.abs()).clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(big)) - 7)                       # one bf16 step at the larger magnitude
    worst = float(((got - ref64).abs() / (ulp + 1e-3)).max())
    print(f"wide vs bf16(fp64) M={M} N={N} K={K}: max |diff| {float((got - ref64).abs().max()):.3e} = {worst:.3f} of the bound (1 ulp + 1e-3)")
    assert worst <= 1.0
    ldc = N + 12                                                             # strided output rows (the lm_head writes [B, Vp])
    o2 = _wide(hip, A, B, M, N, K, ldc=ldc)
    assert torch.equal(o2[:, :N], out[:M]) and bool((o2[:, N:] == 7.0).all())


@pytest.mark.parametrize("M,N,K", PLAIN)
def test_wide_exact_properties(hip, M, N, K):
    A, B, g = _ab(M, N, K, M * 7 + N + K)
    res = _bf(torch.randn(M, N, generator=g)).cuda()
    first = _wide(hip, A, B, M, N, K, residual=res)
    for out in _grids(hip, lambda: _wide(hip, A, B, M, N, K, residual=res)):  # rerun + every grid: the same bits
        assert torch.equal(out, first)
    perm = torch.randperm(M, generator=g).cuda()                             # rows are independent of their position
    Ap = A[perm].contiguous()
    outp = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm_wide(Ap, B, outp, M, N, K, residual=res[perm].contiguous())
    assert torch.equal(outp, first[perm])


@pytest.mark.parametrize("N,K", [(100, 192), (1028, 2048), (4096, 4096)])
def test_wide_m40_equals_rows_of_m64(hip, N, K):
    A, B, g = _ab(64, N, K, N + K)
    o64 = _wide(hip, A, B, 64, N, K)
    o40 = _wide(hip, A, B, 40, N, K)
    assert torch.equal(o40, o64[:40])


@pytest.mark.parametrize("M,I,K", SWIGLU)
def test_wide_swiglu_equals_plain_then_swiglu_kernel(hip, M, I, K):
    A, W, g = _ab(M, 2 * I, K, M + I)
    gu = _wide(hip, A, W, M, 2 * I, K)
    ref = torch.empty(M, I, dtype=torch.bfloat16, device="cuda")
    hip.swiglu_fwd(gu, ref, M, I)
    for out in _grids(hip, lambda: _wide(hip, A, W, M, I, K, fill_rows=1, act=4)):
        assert torch.equal(out[:M], ref)
        assert bool((out[M] == 7.0).all())


@pytest.mark.parametrize("M,N,K", PLAIN)
def test_wide_fp8_equals_bf16_on_dequantised_weight(hip, M, N, K):
    A, W, g = _ab(M, N, K, M * 13 + N + K)
    q, s, Wd = _quantize(hip, W)
    res = _bf(torch.randn(M, N, generator=g)).cuda()
    ref = _wide(hip, A, Wd, M, N, K, residual=res, alpha=0.5)
    for out in _grids(hip, lambda: _wide(hip, A, q, M, N, K, scale=s, residual=res, alpha=0.5)):
        assert torch.equal(out, ref)


@pytest.mark.parametrize("M,I,K", SWIGLU)
def test_wide_fp8_swiglu_equals_bf16(hip, M, I, K):
    """act 4: gate rows and up rows carry different scales."""
    A, W, g = _ab(M, 2 * I, K, M + 3 * I)
    W[I:] *= 4.0
    q, s, Wd = _quantize(hip, W)
    assert bool((s[I:] != s[:I]).any())
    ref = _wide(hip, A, Wd, M, I, K, act=4)
    for out in _grids(hip, lambda: _wide(hip, A, q, M, I, K, scale=s, act=4)):
        assert torch.equal(out, ref)


def test_wide_rejections(hip):
    K, N = 256, 64
    A = torch.zeros(80, K, dtype=torch.bfloat16, device="cuda")
    B = torch.zeros(2 * N, K, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(80, N, dtype=torch.bfloat16, device="cuda")
    n0 = hip.GEMM_WIDE_CALLS
    with pytest.raises(RuntimeError, match="M=16"):
        hip.gemm_wide(A, B, out, 16, N, K)
    with pytest.raises(RuntimeError, match="M=65"):
        hip.gemm_wide(A, B, out, 65, N, K)
    with pytest.raises(RuntimeError, match="act"):
        hip.gemm_wide(A, B, out, 32, N, K, act=2)
    with pytest.raises(RuntimeError, match="fp32 output"):
        hip.gemm_wide(A, B, torch.zeros(32, N, device="cuda"), 32, N, K)
    d = hip.GemmDesc()                                                       # a bias: the binding has no argument for one
    d.A, d.B, d.C, d.M, d.N, d.K, d.batch = hip.p(A), hip.p(B), hip.p(out), 32, N, K, 1
    d.lda, d.ldb, d.ldc, d.ldr, d.ldp, d.alpha = K, K, N, N, N, 1.0
    d.bias = hip.p(torch.zeros(N, device="cuda"))
    with pytest.raises(RuntimeError, match="bias"):
        hip.check(hip._gemm_wide(d, 0, hip.stream()), "desta_gemm_wide_nt")
    assert hip.GEMM_WIDE_CALLS == n0
    hip.gemm_wide(A, B, out, 17, N, K)                                       # ... and M = 17 and 64 are served
    hip.gemm_wide(A, B, out, 64, N, K)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- model level
def _text_batch(d, B, S, seed):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, d.vocab, (B, S), generator=gen)
    am = torch.ones(B, S, dtype=torch.long)
    for b in range(0, B, 3):                                                 # left padding on every third row, of varying length
        n = 1 + (b * 5) % 7
        am[b, :n] = 0
        ids[b, :n] = 0
    inputs = {"context_input_ids": ids, "context_attention_mask": am, "context_batch_start_positions": [],
              "batch_features": None, "batch_transcription_ids": []}
    return ids, am, inputs


_TEXT_REF = {}


def _text_reference(qwen, B, T=12, snapped=False):
    """Weights, inputs and the fp32 oracle's greedy tokens + teacher-forced logits, computed once per case."""
    key = (qwen, B, snapped)
    if key not in _TEXT_REF:
        d = O.tiny_dims(qwen)
        w = O.init_weights(d, seed=7)
        if snapped:
            from test_gpu_fp8_decode import snap_llm_weights
            w = snap_llm_weights(w)
        ids, am, inputs = _text_batch(d, B, 13, seed=B)
        with torch.no_grad():
            x = O.embed_splice(w, d, ids, None, [], [])
            ref, ref_logits = O.greedy_generate(w, d, x, am, T, 0)
        _TEXT_REF[key] = (d, w, inputs, ref, ref_logits)
    return _TEXT_REF[key]


def _check_against_oracle(logits, lo, T):
    es = [rel_err(logits[t].float(), lo[t]) for t in range(T)]
    pick = logits.float().cpu().argmax(-1)
    gap = lo.max(-1).values - lo.gather(-1, pick.unsqueeze(-1)).squeeze(-1)
    worst = float((gap / lo.std(-1)).max())
    print("per-step logits rel-L2", [round(e, 4) for e in es], "gap/spread", worst)
    assert max(es) < 3e-2, es
    assert worst < 0.1, worst


@pytest.mark.parametrize("qwen", [False, True])
@pytest.mark.parametrize("B", [24, 40])
def test_wide_decode_text_only_vs_oracle(qwen, B):
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    T = 12
    d, w, inputs, ref, lo = _text_reference(qwen, B, T)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    n0 = H.GEMM_WIDE_CALLS
    out, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref, collect_logits=True,
                                       eos_token_id=[])
    assert H.GEMM_WIDE_CALLS - n0 == (T - 1) * (4 * d.llm_layers + 1)        # q|k|v, o, gate|up, down per layer + the lm_head, per decode step
    assert out.cpu().tolist() == ref.tolist() and logits.shape == lo.shape
    _check_against_oracle(logits, lo, T)
    if B == 24:                                                              # the same run at B = 8 stays on the 16-row kernels
        sub = {k: (v[:8] if torch.is_tensor(v) else v) for k, v in inputs.items()}
        n1 = H.GEMM_WIDE_CALLS
        out8, lg8 = model._generate_step(sub, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref[:8], collect_logits=True,
                                         eos_token_id=[])
        assert H.GEMM_WIDE_CALLS == n1
        _check_against_oracle(lg8, lo[:, :8], T)


def _repeat_batch(batch, n_ctx, rows):
    """The golden batch repeated to >= `rows` rows: generation inputs (audio spans, features and transcriptions follow their rows)."""
    B = batch["input_ids"].shape[0]
    r = -(-rows // B)
    return {"context_input_ids": batch["input_ids"][:, :n_ctx].repeat(r, 1), "context_attention_mask": batch["attention_mask"][:, :n_ctx].repeat(r, 1),
            "context_batch_start_positions": [(b + j * B, s) for j in range(r) for b, s in batch["batch_start_positions"]],
            "batch_features": torch.cat([batch["batch_features"]] * r, 0),
            "batch_transcription_ids": [t for _ in range(r) for t in batch["batch_transcription_ids"]]}


def test_wide_decode_with_audio_qformer_vs_oracle(golden_dir):
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    T = 10
    d = O.tiny_dims(False)
    g, batch = golden_batch(golden_dir, "llama")
    w = O.init_weights(d, seed=7)
    inputs = _repeat_batch(batch, int(g["gen_ctx_len"]), 17)
    Bn = inputs["context_input_ids"].shape[0]
    assert Bn >= 17
    with torch.no_grad():
        af = O.perception(w, d, inputs["batch_features"])
        x = O.embed_splice(w, d, inputs["context_input_ids"], af, inputs["batch_transcription_ids"], inputs["context_batch_start_positions"])
        ref, lo = O.greedy_generate(w, d, x, inputs["context_attention_mask"], T, 0)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    n0 = H.GEMM_WIDE_CALLS
    out, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref, collect_logits=True,
                                       eos_token_id=[])
    assert H.GEMM_WIDE_CALLS > n0
    assert out.cpu().tolist() == ref.tolist() and logits.shape == lo.shape
    _check_against_oracle(logits, lo, T)


def test_wide_decode_with_orca_injection_vs_oracle(golden_dir):
    import orca_oracle as R
    from desta import _hip as H
    from test_gpu_orca import _case, _oracle_with_theta
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    g, d, o, w, batch, cfg = _case(golden_dir, False)
    model = DeSTA25AudioModel(cfg, weights=w).eval()
    orig = _oracle_with_theta(float(g["rope_theta_used"]))
    try:
        inputs = _repeat_batch(batch, int(g["gen_ctx_len"]), 17)
        assert inputs["context_input_ids"].shape[0] >= 17
        T = g["gen_ids"].shape[1]
        with torch.no_grad():
            ref_ids = R.generate(w, d, o, inputs, T, 0)[0]
            lo = R.generate(w, d, o, inputs, T, 0, forced_tokens=ref_ids)[1]
        n0 = H.GEMM_WIDE_CALLS
        ids, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref_ids, collect_logits=True,
                                           eos_token_id=[])
        assert H.GEMM_WIDE_CALLS > n0
        assert ids.cpu().tolist() == ref_ids.tolist()
        _check_against_oracle(logits, lo, T)
    finally:
        R.rope_whole_vector = orig


def test_wide_decode_fp8_equals_bf16_on_snapped_weights():
    """The FP8 whole-run assertion of tests/test_gpu_fp8_decode.py at a wide batch: tokens and per-step logits, exactly."""
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    T = 12
    d, w, inputs, ref, lo = _text_reference(False, 24, T, snapped=True)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    n0, w0 = H.GEMM_WIDE_CALLS, H.GEMM_W8_CALLS
    ids_b, lg_b = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[])
    model.set_decode_weights("fp8")
    ids_f, lg_f = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[])
    assert H.GEMM_WIDE_CALLS - n0 == 2 * (T - 1) * (4 * d.llm_layers + 1) and H.GEMM_W8_CALLS == w0
    assert all("q8" in ly for ly in model.llm.layers) and model.llm.head8 is not None
    assert torch.equal(ids_b, ids_f)
    for t in range(T):
        assert torch.equal(lg_b[t], lg_f[t]), t
    # ... and the FP8 run follows the fp32 oracle on the same snapped weights
    out, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref, collect_logits=True,
                                       eos_token_id=[])
    _check_against_oracle(logits, lo, T)


def test_batch_over_the_limit_raises_before_any_kernel():
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = O.tiny_dims(False)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=O.init_weights(d, seed=7))
    _, _, inputs = _text_batch(d, H.DECODE_MAX_ROWS + 1, 9, seed=1)
    model.llm._gen_shape = None
    with pytest.raises(ValueError, match="64"):
        model._generate_step(inputs, pad_token_id=0, max_new_tokens=4, do_sample=False)
    assert getattr(model.llm, "_gen_shape", None) is None                    # raised before the caches were allocated and the prompt pass ran
