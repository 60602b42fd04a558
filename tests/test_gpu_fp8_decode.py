"""GPU: weight-only FP8 (OCP e4m3fn, one power-of-two scale per output row) decode.

  - desta_quantize_rows_e4m3 against the rule of include/desta_hip.h evaluated with torch on the host, exactly;
  - desta_gemm_w8a16_nt == desta_gemm_bf16_nt on the dequantised weight, bit for bit (a power-of-two scale commutes with every
    fp32 rounding and the skinny kernel's per-wave K order does not depend on its pipeline depth), and against fp64;
  - `set_decode_weights("fp8")`: on weights snapped to the FP8 grid the decode equals the bf16 decode bit for bit and follows the
    fp32 oracle run on the same snapped weights within the bounds tests/test_gpu_generate.py holds the bf16 path to;
  - adapters keep the q|k|v projection in bf16, ORCA's injection keeps working.
Recorded, not asserted (random tiny weights, NOT snapped; prompt pass on the original weights, decode on the quantised ones):
FP8-vs-bf16 logits distance per step, printed by test_fp8_decode_equals_bf16_decode_on_snapped_weights."""
import math
import re

import pytest
import torch

import desta_oracle as O
from helpers import cfg_from_dims, golden_batch, rel_err

pytestmark = pytest.mark.gpu

E4M3_MAX = 448.0


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def quantize_ref(w):
    """The rule on the host: scale = 2^e, e the smallest integer with amax * 2^-e <= 448 (exact: frexp + integer arithmetic;
    448 = 0.875 * 2^9), all-zero row -> 1; q = e4m3fn(w / scale), round to nearest even (torch's CPU cast)."""
    assert w.dtype == torch.bfloat16
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    m, ex = torch.frexp(amax)                                                # amax = m * 2^ex, 0.5 <= m < 1
    e = ex.to(torch.int32) - 9 + (m > 0.875).to(torch.int32)
    e = torch.where(amax == 0, torch.zeros_like(e), e)
    scale = torch.ldexp(torch.ones_like(amax), e)
    scaled = wf / scale[:, None]
    assert float(scaled.abs().max()) <= E4M3_MAX                             # torch's cast gives NaN above the range, not 448
    q = scaled.to(torch.float8_e4m3fn)
    assert bool(torch.isfinite(q.float()).all())
    return q, scale


def dequant_bf16(q, scale):
    d = q.float() * scale[:, None]
    b = d.bfloat16()
    assert torch.equal(b.float(), d)                                         # q * scale is exactly a bf16 value
    return b


def _bf(x):
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("rows,cols", [(6144, 4096), (1024, 4096), (512, 14336), (100, 192)])
def test_quantize_rows_matches_torch_cpu(hip, rows, cols):
    g = torch.Generator().manual_seed(rows + cols)
    ld = cols + 64                                                           # strided rows
    big = torch.zeros(rows, ld, dtype=torch.bfloat16)
    third = rows // 3
    big[:third, :cols] = _bf(torch.randn(third, cols, generator=g) * 0.02)
    big[third:2 * third, :cols] = _bf(torch.randn(third, cols, generator=g))
    big[2 * third:, :cols] = _bf(torch.randn(rows - 2 * third, cols, generator=g) * 3e-4)
    big[:, cols:] = 1e4                                                      # behind the row: must not be read
    big[5, :cols] = 0                                                        # an all-zero row
    big[7, :cols] = _bf(torch.randn(cols, generator=g)).clamp(-1, 1)
    big[7, 3] = -448.0 * 2.0 ** -5                                           # amax exactly 2^k * 448
    big[9, :cols] = big[7, :cols]
    big[9, 3] = 2.0 ** 3 * 1.7578125                                         # one bf16 step above 1.75 * 2^3: the next exponent
    w = big[:, :cols]
    q_ref, s_ref = quantize_ref(w.contiguous())
    assert float(s_ref[5]) == 1.0 and float(s_ref[7]) == 2.0 ** -5 and float(s_ref[9]) == 2.0 ** -4
    wd = big.cuda()
    q, s = hip.quantize_rows_e4m3(wd[:, :cols], rows, cols, ld)
    assert q.dtype == torch.uint8 and q.shape == (rows, cols) and s.shape == (rows,)
    assert torch.equal(s.cpu(), s_ref)
    got = q.cpu().view(torch.float8_e4m3fn).float()
    assert bool(torch.isfinite(got).all())
    assert bool((got == q_ref.float()).all())                                # +-0 compared as values
    q2, s2 = hip.quantize_rows_e4m3(dequant_bf16(q_ref, s_ref).cuda())       # re-quantising a snapped weight reproduces its values
    assert torch.equal(q2.cpu().view(torch.float8_e4m3fn).float() * s2.cpu()[:, None], q_ref.float() * s_ref[:, None])


def _operands(M, N, K, rows, seed, gain_from=None):
    """A [M, K] with strided rows, the CPU quantisation (B8, s) of a random weight [rows, K] and its dequantised bf16 form."""
    g = torch.Generator().manual_seed(seed)
    Abig = _bf(torch.randn(M, 3, K, generator=g)).cuda()
    W = torch.randn(rows, K, generator=g) / math.sqrt(K) * 2
    if gain_from is not None:
        W[gain_from:] *= 4.0                                                 # rows [gain_from, rows) land on other scales
    W = _bf(W)
    q, s = quantize_ref(W)
    Bd = dequant_bf16(q, s)
    return Abig[:, 1], q.view(torch.uint8).cuda(), s.cuda(), Bd.cuda(), g


PLAIN = [(1, 16, 64), (3, 100, 192), (8, 4096, 4096), (16, 1028, 2048), (8, 6144, 14336)]
SWIGLU = [(8, 512, 256), (3, 104, 192), (16, 14336, 4096)]
RMS = [(8, 4096, 4096), (8, 28672, 4096)]


def _grids(hip, fn):
    """fn() at the default persistent grid and at 7 / 64 / 512 blocks."""
    outs = [fn()]
    try:
        for blocks in (7, 64, 512):
            hip.gemm_set_option(3, blocks)
            outs.append(fn())
    finally:
        hip.gemm_set_option(3, 512)
    return outs


@pytest.mark.parametrize("M,N,K", PLAIN)
def test_gemm_w8_equals_bf16_kernel_on_dequantised_weight(hip, M, N, K):
    A, B8, s, Bd, g = _operands(M, N, K, N, M * 11 + N + K)
    res = _bf(torch.randn(M, N, generator=g)).cuda()
    ref = torch.empty(M, N, dtype=torch.float32, device="cuda")
    hip.gemm(A, Bd, ref, M, N, K, lda=3 * K)
    for U in (0, 162, 164):                                                  # automatic choice and both pipeline depths: same bits
        try:
            hip.gemm_set_option(11, U)
            for out in _grids(hip, lambda: hip.gemm_w8(A, B8, s, torch.full((M + 1, N), 7.0, dtype=torch.float32, device="cuda"), M, N, K, lda=3 * K)):
                assert torch.equal(out[:M], ref), U
                assert bool((out[M] == 7.0).all())                           # rows >= M untouched
        finally:
            hip.gemm_set_option(11, 0)
    refb = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm(A, Bd, refb, M, N, K, lda=3 * K, residual=res, alpha=0.5)
    for out in _grids(hip, lambda: hip.gemm_w8(A, B8, s, torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), M, N, K, lda=3 * K, residual=res, alpha=0.5)):
        assert torch.equal(out, refb)
    ldc = N + 12                                                             # strided output rows (the lm_head writes [B, Vp])
    o1 = torch.full((M, ldc), 3.0, dtype=torch.bfloat16, device="cuda")
    o2 = o1.clone()
    hip.gemm(A, Bd, o1, M, N, K, lda=3 * K, ldc=ldc)
    hip.gemm_w8(A, B8, s, o2, M, N, K, lda=3 * K, ldc=ldc)
    assert torch.equal(o1, o2) and bool((o2[:, N:] == 3.0).all())


@pytest.mark.parametrize("M,I,K", SWIGLU)
def test_gemm_w8_fused_swiglu_equals_bf16_kernel(hip, M, I, K):
    """act 4: the gate row and the up row each carry their own scale."""
    A, B8, s, Bd, g = _operands(M, I, K, 2 * I, M + I, gain_from=I)
    assert bool((s[I:] != s[:I]).all())                                      # every up row on another scale than its gate row
    ref = torch.empty(M, I, dtype=torch.bfloat16, device="cuda")
    hip.gemm(A, Bd, ref, M, I, K, lda=3 * K, act=4)
    for out in _grids(hip, lambda: hip.gemm_w8(A, B8, s, torch.empty(M, I, dtype=torch.bfloat16, device="cuda"), M, I, K, lda=3 * K, act=4)):
        assert torch.equal(out, ref)


@pytest.mark.parametrize("M,N,K", RMS)
def test_gemm_w8_fused_rmsnorm_equals_bf16_kernel(hip, M, N, K):
    assert hip.rms_fusable(M, K)
    g = torch.Generator().manual_seed(M * 5 + N)
    x = _bf(torch.randn(M, K, generator=g) * 3).cuda()
    gamma = (1.0 + 0.1 * torch.randn(K, generator=g)).cuda()
    W = _bf(torch.randn(2 * N, K, generator=g) / math.sqrt(K) * 2)
    q, s = quantize_ref(W)
    Bd, B8, s = dequant_bf16(q, s).cuda(), q.view(torch.uint8).cuda(), s.cuda()
    res = _bf(torch.randn(M, N, generator=g)).cuda()
    ref = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm(x, Bd, ref, M, N, K, residual=res, a_rms_weight=gamma, a_rms_eps=1e-5)
    for out in _grids(hip, lambda: hip.gemm_w8(x, B8, s, torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), M, N, K, residual=res,
                                               a_rms_weight=gamma, a_rms_eps=1e-5)):
        assert torch.equal(out, ref)
    ref32 = torch.empty(M, N, dtype=torch.float32, device="cuda")
    hip.gemm(x, Bd, ref32, M, N, K, a_rms_weight=gamma, a_rms_eps=1e-5)
    for U in (162, 164):
        try:
            hip.gemm_set_option(11, U)
            assert torch.equal(hip.gemm_w8(x, B8, s, torch.empty_like(ref32), M, N, K, a_rms_weight=gamma, a_rms_eps=1e-5), ref32)
        finally:
            hip.gemm_set_option(11, 0)
    # gate|up rows [0, N) | [N, 2N) with their own scales, RMSNorm and SwiGLU fused
    ref4 = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    hip.gemm(x, Bd, ref4, M, N, K, act=4, a_rms_weight=gamma, a_rms_eps=1e-5)
    out4 = hip.gemm_w8(x, B8, s, torch.empty_like(ref4), M, N, K, act=4, a_rms_weight=gamma, a_rms_eps=1e-5)
    assert torch.equal(out4, ref4)


@pytest.mark.parametrize("M,N,K", PLAIN + SWIGLU + RMS)
def test_gemm_w8_vs_fp64(hip, M, N, K):
    A, B8, s, Bd, g = _operands(M, N, K, N, M * 13 + N + K)
    out = hip.gemm_w8(A, B8, s, torch.empty(M, N, dtype=torch.float32, device="cuda"), M, N, K, lda=3 * K)
    B64 = B8.cpu().view(torch.float8_e4m3fn).double() * s.cpu().double()[:, None]
    ref = A.cpu().double() @ B64.T
    err = (out.cpu().double() - ref).abs()
    print(f"gemm_w8 vs fp64 M={M} N={N} K={K}: max abs err {float(err.max()):.3e}, max |ref| {float(ref.abs().max()):.3e}")
    torch.testing.assert_close(out.cpu().double(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(hip.gemm_w8(A, B8, s, torch.empty_like(out), M, N, K, lda=3 * K), out)       # a rerun gives identical bits


def test_gemm_w8_argument_checks(hip):
    K, N = 256, 64
    A17 = torch.zeros(17, K, dtype=torch.bfloat16, device="cuda")
    B8 = torch.zeros(N, K, dtype=torch.uint8, device="cuda")
    s = torch.ones(N, device="cuda")
    out = torch.zeros(17, N, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="M"):
        hip.gemm_w8(A17, B8, s, out, 17, N, K)
    with pytest.raises(RuntimeError, match="scale"):
        hip.gemm_w8(A17, B8, None, out, 8, N, K)
    with pytest.raises(RuntimeError, match="act"):
        hip.gemm_w8(A17, B8, s, out, 8, N, K, act=2)
    with pytest.raises(RuntimeError):
        hip.gemm_set_option(11, 322)
    hip.gemm_w8(A17, B8, s, out, 16, N, K)                                   # ... and M = 16 is served
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- model level
LLM_LINEAR = re.compile(r"^llm_model\.(model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)|lm_head)\.weight$")


def snap_llm_weights(w):
    """Every LLM linear weight and the lm_head weight onto the FP8 grid, on the host: w <- bf16(q * s)."""
    out, n = dict(w), 0
    for k, v in w.items():
        if LLM_LINEAR.match(k):
            q, s = quantize_ref(v.bfloat16())
            out[k] = dequant_bf16(q, s).float()
            n += 1
    assert n >= 8
    return out


def _gen_inputs(g, batch):
    n_ctx = int(g["gen_ctx_len"])
    return {"context_input_ids": batch["input_ids"][:, :n_ctx], "context_attention_mask": batch["attention_mask"][:, :n_ctx],
            "context_batch_start_positions": batch["batch_start_positions"], "batch_features": batch["batch_features"],
            "batch_transcription_ids": batch["batch_transcription_ids"]}


def _oracle(w, d, g, batch, T, forced=None):
    n_ctx = int(g["gen_ctx_len"])
    with torch.no_grad():
        af = O.perception(w, d, batch["batch_features"])
        x = O.embed_splice(w, d, batch["input_ids"][:, :n_ctx], af, batch["batch_transcription_ids"], batch["batch_start_positions"])
        return O.greedy_generate(w, d, x, batch["attention_mask"][:, :n_ctx], T, 0, forced_tokens=forced)


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_fp8_decode_equals_bf16_decode_on_snapped_weights(golden_dir, name):
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = O.tiny_dims(name == "qwen3")
    g, batch = golden_batch(golden_dir, name)
    w = snap_llm_weights(O.init_weights(d, seed=7))
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    inputs = _gen_inputs(g, batch)
    with pytest.raises(ValueError):
        model.set_decode_weights("int4")
    assert model.llm.decode_weights == "bf16"
    for kw in (dict(do_sample=False), dict(do_sample=True, top_k=20, seed=3)):
        model.set_decode_weights("bf16")
        n0 = H.GEMM_W8_CALLS
        ids_b, lg_b = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, collect_logits=True, eos_token_id=[], **kw)
        assert H.GEMM_W8_CALLS == n0                                         # the default path never touches the FP8 kernel
        model.set_decode_weights("fp8")
        ids_f, lg_f = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, collect_logits=True, eos_token_id=[], **kw)
        assert H.GEMM_W8_CALLS - n0 == 9 * (4 * d.llm_layers + 1)            # 9 decode steps: q|k|v, o, gate|up, down per layer + the lm_head
        assert torch.equal(ids_b, ids_f)
        for t in range(10):
            assert torch.equal(lg_b[t], lg_f[t]), t
        model.set_decode_weights("bf16")
        assert model.llm.head8 is None and all("q8" not in ly for ly in model.llm.layers)       # the copies are freed
        ids_r, lg_r = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, collect_logits=True, eos_token_id=[], **kw)
        assert torch.equal(ids_r, ids_b) and torch.equal(lg_r, lg_b)
    # recorded, not asserted: the distance the quantisation itself causes on random tiny weights (prompt pass on the original
    # weights, decode steps on the quantised ones), teacher-forced on the bf16 run's tokens
    raw = DeSTA25AudioModel(cfg_from_dims(d), weights=O.init_weights(d, seed=7))
    ids0, lg0 = raw._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True, eos_token_id=[])
    raw.set_decode_weights("fp8")
    ids8, lg8 = raw._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True, eos_token_id=[], forced_tokens=ids0.cpu())
    print(f"{name}: un-snapped FP8-vs-bf16 logits rel-L2 per step", [round(rel_err(lg8[t].float(), lg0[t].float()), 4) for t in range(10)],
          "greedy agreement", float((lg8.float().argmax(-1) == lg0.float().argmax(-1)).float().mean()))


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_fp8_decode_vs_oracle(golden_dir, name):
    """The FP8 path against an fp32 reference that shares no code with it, on the quantised model: the same snapped weights go to the
    product and to the oracle, teacher-forced on the oracle's own greedy tokens."""
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = O.tiny_dims(name == "qwen3")
    g, batch = golden_batch(golden_dir, name)
    w = snap_llm_weights(O.init_weights(d, seed=7))
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    model.set_decode_weights("fp8")
    ref_ids, _ = _oracle(w, d, g, batch, 10)
    lo = _oracle(w, d, g, batch, 10, forced=ref_ids)[1]
    ids, logits = model._generate_step(_gen_inputs(g, batch), pad_token_id=0, max_new_tokens=10, do_sample=False, forced_tokens=ref_ids,
                                       collect_logits=True, eos_token_id=[])
    assert ids.cpu().tolist() == ref_ids.tolist() and logits.shape == lo.shape
    es = [rel_err(logits[t].float(), lo[t]) for t in range(10)]
    pick = logits.float().cpu().argmax(-1)
    gap = lo.max(-1).values - lo.gather(-1, pick.unsqueeze(-1)).squeeze(-1)
    print(f"{name}: fp8 decode vs oracle, per-step logits rel-L2", [round(e, 4) for e in es], "gap/spread", float((gap / lo.std(-1)).max()))
    assert max(es) < 3e-2, es
    assert float((gap / lo.std(-1)).max()) < 0.1, gap / lo.std(-1)


def test_fp8_decode_with_lora_keeps_qkv_in_bf16():
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = O.tiny_dims(False)
    d.lora_r = 16
    w = snap_llm_weights(O.init_weights(d, seed=7))
    model = DeSTA25AudioModel(cfg_from_dims(d, use_lora=True), weights=w)
    for n in model.trainable_parameter_names:
        if ".lora_B." in n:
            model.arena.param(n).zero_()
    model.mark_weights_updated()
    base = DeSTA25AudioModel(cfg_from_dims(O.tiny_dims(False)), weights={k: v for k, v in w.items() if ".lora_" not in k})
    batch = O.synthetic_batch(d, B=2, S_ctx=8, S_tgt=10, seed=2, pad=[2, 0])
    n_ctx = batch["input_ids"].shape[1] - 10 + 3
    ctx = {"context_input_ids": batch["input_ids"][:, :n_ctx], "context_attention_mask": batch["attention_mask"][:, :n_ctx],
           "batch_features": batch["batch_features"], "batch_transcription_ids": batch["batch_transcription_ids"],
           "context_batch_start_positions": batch["batch_start_positions"]}
    model.eval().set_decode_weights("fp8")
    base.eval().set_decode_weights("fp8")
    n0 = H.GEMM_W8_CALLS
    ids = model._generate_step(ctx, pad_token_id=0, max_new_tokens=6, do_sample=False, eos_token_id=[])
    assert H.GEMM_W8_CALLS - n0 == 5 * (3 * d.llm_layers + 1)                # 5 decode steps: o, gate|up, down + the lm_head; q|k|v stayed bf16
    assert all("wqkv" not in ly["q8"] for ly in model.llm.layers)
    n1 = H.GEMM_W8_CALLS
    ids_base = base._generate_step(ctx, pad_token_id=0, max_new_tokens=6, do_sample=False, eos_token_id=[])
    assert H.GEMM_W8_CALLS - n1 == 5 * (4 * d.llm_layers + 1)
    assert ids.shape == (2, 6) and torch.equal(ids, ids_base)                # B = 0: the base model's FP8 tokens


def test_fp8_decode_with_orca_injection(golden_dir):
    """ORCA tiny config: the injection's own (trainable) projections stay bf16, the LLM's stream FP8; per-step logits against the ORCA
    oracle on the same snapped weights within the bound tests/test_gpu_orca.py holds the bf16 decode to."""
    import orca_oracle as R
    from test_gpu_orca import _case, _oracle_with_theta
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    g, d, o, w, batch, cfg = _case(golden_dir, False)
    w = snap_llm_weights(w)
    model = DeSTA25AudioModel(cfg, weights=w).eval()
    model.set_decode_weights("fp8")
    orig = _oracle_with_theta(float(g["rope_theta_used"]))
    try:
        inputs = _gen_inputs(g, batch)
        T = g["gen_ids"].shape[1]
        with torch.no_grad():
            ref_ids = R.generate(w, d, o, inputs, T, 0)[0]
            lo = R.generate(w, d, o, inputs, T, 0, forced_tokens=ref_ids)[1]
        ids, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref_ids, collect_logits=True,
                                           eos_token_id=[])
        assert ids.cpu().tolist() == ref_ids.tolist()
        es = [rel_err(logits[t].float(), lo[t]) for t in range(T)]
        pick = logits.float().cpu().argmax(-1)
        gap = lo.max(-1).values - lo.gather(-1, pick.unsqueeze(-1)).squeeze(-1)
        print("orca fp8 decode: per-step logits rel", [round(e, 4) for e in es], "gap/std", float((gap / lo.std(-1)).max()))
        assert max(es) < 3e-2, es
        assert float((gap / lo.std(-1)).max()) < 0.1
    finally:
        R.rope_whole_vector = orig
