"""GPU: weight-only MXFP4 (OCP e2m1 nibbles, one e8m0 scale per 32 consecutive k) decode.

  - desta_quantize_rows_mxfp4 against tests/mxfp4_reference.py::quantize_ref: codes as values, scales exactly, on strided rows with
    1e4 planted behind each row, rows in three magnitude bands, the host test's planted blocks included;
  - desta_gemm_w4a16_nt per element against fp64 on the DEQUANTISED weight (quantisation error is not in it): max |out - ref| /
    bound <= 2 over whole sentinel-filled buffers with guard rows, the criterion and factor of tests/test_gpu_gemm_fp64.py; a rerun
    and the grids 7 / 64 / 512 give identical bits; rejected arguments are rejected by name;
  - `set_decode_weights("mxfp4")` on the tiny goldens with the LLM linears snapped to the MXFP4 grid: per-step logits against the
    fp32 oracle on the same snapped weights within the bounds tests/test_gpu_fp8_decode.py::test_fp8_decode_vs_oracle holds FP8 and
    bf16 to, the projection counter, the bf16 path untouched, the copies freed; the same at batch 24 (the 17..64-row form);
  - verify_step under MXFP4 against single steps (tests/test_gpu_speculative.py::test_verify_step_vs_single_steps' ratio);
  - adapters keep q|k|v on `gemm`, the ORCA injection runs.
Recorded, not asserted: MXFP4-vs-bf16 logits rel-L2 per step and greedy agreement on UNSNAPPED tiny weights (run with -s)."""
import re

import pytest
import torch

import desta_oracle as O
import mxfp4_reference as X
from helpers import cfg_from_dims, golden_batch, rel_err

pytestmark = pytest.mark.gpu

FACTOR = 2.0
GUARD_ROWS = X.G.GUARD_ROWS


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from desta import _hip
    return _hip


def _bf(x):
    return x.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- quantiser
@pytest.mark.parametrize("rows,cols", [(100, 192), (1024, 4096), (512, 14336)])
def test_quantize_rows_mxfp4_matches_the_reference(hip, rows, cols):
    g = torch.Generator().manual_seed(rows + cols)
    ld, nb = cols + 64, cols // 32
    big = torch.zeros(rows, ld, dtype=torch.bfloat16)
    third = rows // 3
    big[:third, :cols] = _bf(torch.randn(third, cols, generator=g) * 0.02)
    big[third:2 * third, :cols] = _bf(torch.randn(third, cols, generator=g))
    big[2 * third:, :cols] = _bf(torch.randn(rows - 2 * third, cols, generator=g) * 3e-4)
    big[:, cols:] = 1e4                                                      # behind the row: must not be read
    planted, e_planted, _ = X.planted_blocks()
    where = [(7 + 3 * i, (5 * i) % nb) for i in range(planted.shape[0])]     # (row, block) of planted block i
    for i, (r, b) in enumerate(where):
        big[r, 32 * b:32 * b + 32] = planted[i]
    wd = big.cuda()
    codes_ref, e_ref = X.quantize_ref(wd[:, :cols])                          # the reference, on the device
    for i, (r, b) in enumerate(where):
        assert int(e_ref[r, b]) == int(e_planted[i])
    ldq, lds = cols // 2 + 32, nb + 5                                        # strided outputs between sentinels
    q = torch.full((rows, ldq), 0xAB, dtype=torch.uint8, device="cuda")
    s = torch.full((rows, lds), 0xCD, dtype=torch.uint8, device="cuda")
    hip.quantize_rows_mxfp4(wd[:, :cols], rows, cols, ld, q=q, ldq=ldq, scale=s, lds=lds)
    torch.cuda.synchronize()
    assert bool((q[:, cols // 2:] == 0xAB).all()) and bool((s[:, nb:] == 0xCD).all())
    assert torch.equal(s[:, :nb], X.scale_bytes(e_ref))                      # scales exactly
    got = X.unpack(q[:, :cols // 2])
    assert torch.equal(X.code_values(got), X.code_values(codes_ref))         # +-0 compared as values
    assert int(s[:, :nb].max()) < 255
    # re-quantising the dequantised weight reproduces it
    d = X.dequant_bf16(codes_ref, e_ref)
    q2, s2 = hip.quantize_rows_mxfp4(d)
    assert q2.shape == (rows, cols // 2) and q2.stride(0) % 16 == 0 and s2.shape == (rows, nb)
    assert torch.equal(X.dequant(X.unpack(q2), s2.to(torch.int32) - 127), d.double())


# ---------------------------------------------------------------------------------------------------------------- GEMM against fp64
PLAIN = [(1, 16, 64), (3, 100, 192), (8, 4096, 4096), (16, 1028, 2048), (8, 512, 14336)]
SWIGLU = [(8, 512, 256), (3, 104, 192), (16, 1024, 4096)]
WIDE = [(17, 16, 64), (33, 100, 192), (48, 36, 64 * 37), (64, 1028, 2048), (24, 4096, 4096)]
WIDE_SWIGLU = [(17, 104, 192), (40, 512, 256), (40, 512, 2048)]              # the last one takes the K-slice fix-up
CASES = ([X.case(*s, res=i % 2 == 1) for i, s in enumerate(PLAIN)] + [X.case(*s, act=4) for s in SWIGLU] +
         [X.case(8, 4096, 4096, rms=True, res=True), X.case(8, 4096, 4096, act=4, rms=True)] +
         [X.case(*s, res=i % 2 == 1) for i, s in enumerate(WIDE)] + [X.case(*s, act=4) for s in WIDE_SWIGLU] +
         [X.case(5, 100, 192, out_f32=True, alpha=0.75), X.case(20, 100, 192, out_f32=True, res=True)])


KSLICES = {(4096, 4096, 0): 4, (1028, 2048, 0): 2, (512, 14336, 0): 8, (1024, 4096, 4): 4, (4096, 4096, 4): 2, (36, 64 * 37, 0): 2,
           (512, 2048, 4): 2}                                                # (N, K, act) -> K-slices; every other case has one


def _run(hip, o):
    M, N, K = o["M"], o["N"], o["K"]
    out = torch.full((1, M + GUARD_ROWS, o["ldc"]), X.SENTINEL, dtype=torch.float32 if o["out_f32"] else torch.bfloat16, device="cuda")
    hip.gemm_w4(X.kernel_arg(o, "A"), o["q"], o["s"], out, M, N, K, lda=o["lda"], ldb=o["ldq"], ldc=o["ldc"], ld_scale=o["lds"],
                residual=o["res"], ldr=o["ldr"], act=o["act"], alpha=o["alpha"], a_rms_weight=o["rms_w"], a_rms_eps=o.get("rms_eps", 0.0))
    return out


@pytest.mark.parametrize("case", CASES, ids=[X.case_id(c) for c in CASES])
def test_gemm_w4_against_fp64(hip, case):
    o = X.operands(case, device="cuda")
    M, N = o["M"], o["N"]
    if case["act"] == 4:
        assert bool((o["e"][N:] != o["e"][:N]).any(1).all())                 # up rows sit on other scales than their gate rows
    if case["rms"]:
        assert hip.rms_fusable(M, o["K"])
    assert o["plan"]["ks"] == KSLICES.get((N, o["K"], case["act"]), 1)       # which cases go through slabs and the fix-up launch
    n0 = hip.GEMM_W4_CALLS
    out = _run(hip, o)
    torch.cuda.synchronize()
    assert hip.GEMM_W4_CALLS == n0 + 1 and hip.lib.desta_gemm_last_kernel() == 3
    ref = X.exact(o)
    valid = ref["_"]["C_valid"]
    assert bool((out.double()[~valid] == X.SENTINEL).all()), "a guard row or column was written"      # rows >= M, columns >= N
    r = X.ratio(o, ref, "C", out)
    print(f"\n{X.case_id(case)} [MF {o['plan']['mf']} ks {o['plan']['ks']} c {o['c']}]: C {r:.3f}", end="")
    assert r <= FACTOR, (X.case_id(case), r)
    assert torch.equal(_run(hip, o), out), "a rerun differs"
    try:
        for blocks in (7, 64, 512):                                          # the result does not depend on the grid
            hip.gemm_set_option(3, blocks)
            assert torch.equal(_run(hip, o), out), blocks
    finally:
        hip.gemm_set_option(3, 512)


def test_gemm_w4_argument_checks(hip):
    K, N = 256, 64
    A = torch.zeros(65, K, dtype=torch.bfloat16, device="cuda")
    B4 = torch.zeros(N, K // 2 + 8, dtype=torch.uint8, device="cuda")
    s = torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda")
    out = torch.full((65, N), 7.0, dtype=torch.bfloat16, device="cuda")
    n0 = hip.GEMM_W4_CALLS
    with pytest.raises(RuntimeError, match="M=65"):
        hip.gemm_w4(A, B4, s, out, 65, N, K, ldb=K // 2)
    with pytest.raises(RuntimeError, match="scale"):
        hip.gemm_w4(A, B4, None, out, 8, N, K, ldb=K // 2)
    with pytest.raises(RuntimeError, match="act 2"):
        hip.gemm_w4(A, B4, s, out, 8, N, K, ldb=K // 2, act=2)
    with pytest.raises(RuntimeError, match="K=96"):
        hip.gemm_w4(A, B4, s, out, 8, N, 96, ldb=K // 2)
    with pytest.raises(RuntimeError, match="ldb"):
        hip.gemm_w4(A, B4, s, out, 8, N, K, ldb=K // 2 + 8)                  # not a multiple of 16
    with pytest.raises(RuntimeError, match="residual"):
        hip.gemm_w4(A, B4, s, out, 8, N, K, ldb=K // 2, residual=torch.zeros(8, N, device="cuda"))
    with pytest.raises(RuntimeError, match="a_rms_weight"):
        hip.gemm_w4(A, B4, s, out, 17, N, 512, ldb=256, ld_scale=16, a_rms_weight=torch.ones(512, device="cuda"))     # M > 16
    torch.cuda.synchronize()
    assert hip.GEMM_W4_CALLS == n0 and bool((out == 7.0).all())              # nothing was launched
    hip.gemm_w4(A, B4, s, out, 64, N, K, ldb=K // 2)                         # ... and M = 64 is served: zero codes give zeros
    torch.cuda.synchronize()
    assert bool((out[:64] == 0).all()) and bool((out[64] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- model level
LLM_LINEAR = re.compile(r"^llm_model\.(model\.layers\.\d+\.(self_attn\.[qkvo]_proj|mlp\.(gate|up|down)_proj)|lm_head)\.weight$")


def snap_llm_weights_mx(w):
    """Every LLM linear weight and the lm_head weight onto the MXFP4 grid, on the host: w <- code * 2^e."""
    out, n = dict(w), 0
    for k, v in w.items():
        if LLM_LINEAR.match(k):
            out[k] = X.dequant_bf16(*X.quantize_ref(v.bfloat16())).float()
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


def _check_against_oracle(tag, logits, lo, T):
    es = [rel_err(logits[t].float(), lo[t]) for t in range(T)]
    pick = logits.float().cpu().argmax(-1)
    gap = lo.max(-1).values - lo.gather(-1, pick.unsqueeze(-1)).squeeze(-1)
    worst = float((gap / lo.std(-1)).max())
    print(f"{tag}: mxfp4 decode vs oracle, per-step logits rel-L2", [round(e, 4) for e in es], "gap/spread", worst)
    assert max(es) < 3e-2, es
    assert worst < 0.1, worst


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_mxfp4_decode_vs_oracle_on_snapped_weights(golden_dir, name):
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = O.tiny_dims(name == "qwen3")
    g, batch = golden_batch(golden_dir, name)
    w = snap_llm_weights_mx(O.init_weights(d, seed=7))
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    inputs = _gen_inputs(g, batch)
    with pytest.raises(ValueError):
        model.set_decode_weights("int4")
    model.set_decode_weights("mxfp4")
    ref_ids, _ = _oracle(w, d, g, batch, 10)
    lo = _oracle(w, d, g, batch, 10, forced=ref_ids)[1]
    n0, n8 = H.GEMM_W4_CALLS, H.GEMM_W8_CALLS
    ids, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, forced_tokens=ref_ids, collect_logits=True,
                                       eos_token_id=[])
    assert H.GEMM_W4_CALLS - n0 == 9 * (4 * d.llm_layers + 1)                # 9 decode steps: q|k|v, o, gate|up, down per layer + the lm_head
    assert H.GEMM_W8_CALLS == n8
    assert model.llm.head4 is not None and all(set(ly["q4"]) == {"wqkv", "wo", "wgu", "wd"} for ly in model.llm.layers)
    assert ids.cpu().tolist() == ref_ids.tolist() and logits.shape == lo.shape
    _check_against_oracle(name, logits, lo, 10)
    # "fp8" frees the MXFP4 copies, "mxfp4" the FP8 ones, "bf16" both; the bf16 path never touches the counter and keeps its bits
    model.set_decode_weights("bf16")
    assert model.llm.head4 is None and all("q4" not in ly for ly in model.llm.layers)
    n1 = H.GEMM_W4_CALLS
    ids_b, lg_b = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True, eos_token_id=[])
    assert H.GEMM_W4_CALLS == n1
    model.set_decode_weights("mxfp4")
    model._generate_step(inputs, pad_token_id=0, max_new_tokens=3, do_sample=False, eos_token_id=[])
    model.set_decode_weights("fp8")
    assert model.llm.head4 is None and all("q4" not in ly for ly in model.llm.layers)
    model._generate_step(inputs, pad_token_id=0, max_new_tokens=3, do_sample=False, eos_token_id=[])
    assert model.llm.head8 is not None
    model.set_decode_weights("mxfp4")
    assert model.llm.head8 is None and all("q8" not in ly for ly in model.llm.layers)
    model.set_decode_weights("bf16")
    ids_r, lg_r = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True, eos_token_id=[])
    assert torch.equal(ids_r, ids_b) and torch.equal(lg_r, lg_b)
    # recorded, not asserted: what the quantisation itself costs on random tiny weights (prompt pass on the original weights, decode
    # steps on the quantised ones), teacher-forced on the bf16 run's tokens
    raw = DeSTA25AudioModel(cfg_from_dims(d), weights=O.init_weights(d, seed=7))
    ids0, lg0 = raw._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True, eos_token_id=[])
    raw.set_decode_weights("mxfp4")
    ids4, lg4 = raw._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True, eos_token_id=[], forced_tokens=ids0.cpu())
    print(f"{name}: un-snapped MXFP4-vs-bf16 logits rel-L2 per step", [round(rel_err(lg4[t].float(), lg0[t].float()), 4) for t in range(10)],
          "greedy agreement", float((lg4.float().argmax(-1) == lg0.float().argmax(-1)).float().mean()))


def test_mxfp4_decode_batch_24_vs_oracle():
    """The same check through the 17..64-row form: text-only batch 24 of tests/test_gpu_wide_decode.py on MXFP4-snapped weights."""
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    from test_gpu_wide_decode import _text_batch
    T, B = 12, 24
    d = O.tiny_dims(False)
    w = snap_llm_weights_mx(O.init_weights(d, seed=7))
    ids, am, inputs = _text_batch(d, B, 13, seed=B)
    with torch.no_grad():
        ref, lo = O.greedy_generate(w, d, O.embed_splice(w, d, ids, None, [], []), am, T, 0)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
    model.set_decode_weights("mxfp4")
    n0, nw = H.GEMM_W4_CALLS, H.GEMM_WIDE_CALLS
    out, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref, collect_logits=True,
                                       eos_token_id=[])
    assert H.GEMM_W4_CALLS - n0 == (T - 1) * (4 * d.llm_layers + 1) and H.GEMM_WIDE_CALLS == nw
    assert out.cpu().tolist() == ref.tolist() and logits.shape == lo.shape
    _check_against_oracle("batch 24", logits, lo, T)


@pytest.mark.parametrize("k", [3, 7])                                        # B (k + 1) = 12 and 24: both forms of the kernel
def test_verify_step_vs_single_steps_under_mxfp4(hip, k):
    """tests/test_gpu_speculative.py::test_verify_step_vs_single_steps with MXFP4 decode weights: the verify step's logits and cache
    slots stay within 1.5 x the single steps' own distance to the fp32 oracle."""
    from test_gpu_kv8_cache import _gen
    from test_gpu_prefill_chunk import PADS, _model, _oracle as _pf_oracle
    d, w, model = _model(False)
    S, T = 61, k + 2
    inputs, ref, lo = _pf_oracle(False, S, 12)
    llm, w1 = model.llm, k + 1
    try:
        model.set_decode_weights("mxfp4")
        model.set_speculative(None)
        _, lg = _gen(model, inputs, T, ref[:, :T])                           # prompt pass + k + 1 single steps on the oracle's tokens
        plain = [c[:, S:S + w1].clone() for c in llm.kv_cache]
        n4, nw = hip.GEMM_W4_CALLS, hip.GEMM_WIDE_CALLS
        kv_start = torch.tensor(PADS[S], dtype=torch.int32, device="cuda")
        vl = llm.verify_step(ref[:, :w1].cuda(), S, kv_start).view(3, w1, -1)[:, :, :d.vocab].clone()
        torch.cuda.synchronize()
        assert hip.GEMM_W4_CALLS - n4 == 4 * d.llm_layers + 1 and hip.GEMM_WIDE_CALLS == nw
        e_plain = max(rel_err(lg[j + 1].float(), lo[j + 1]) for j in range(w1))
        e_v = max(rel_err(vl[:, j].float(), lg[j + 1].float()) for j in range(w1))
        e_kv = max(rel_err(c[:, S:S + w1].float(), p.float()) for c, p in zip(llm.kv_cache, plain))
        print(f"VERIFY_STEP mxfp4 weights M {3 * w1}: logits rel-L2 verify vs single steps {e_v:.3e}, single steps vs fp32 oracle {e_plain:.3e} "
              f"(ratio {e_v / e_plain:.3f}); cache slots rel-L2 {e_kv:.3e}")
        assert bool(torch.isfinite(vl.float()).all())
        assert e_v <= 1.5 * e_plain, (e_v, e_plain)
        assert e_kv <= 1.5 * e_plain, (e_kv, e_plain)
    finally:
        model.set_decode_weights("bf16")
        model.set_speculative(None)


def test_mxfp4_decode_with_lora_keeps_qkv_in_bf16():
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = O.tiny_dims(False)
    d.lora_r = 16
    w = snap_llm_weights_mx(O.init_weights(d, seed=7))
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
    model.eval().set_decode_weights("mxfp4")
    base.eval().set_decode_weights("mxfp4")
    n0 = H.GEMM_W4_CALLS
    ids = model._generate_step(ctx, pad_token_id=0, max_new_tokens=6, do_sample=False, eos_token_id=[])
    assert H.GEMM_W4_CALLS - n0 == 5 * (3 * d.llm_layers + 1)                # 5 decode steps: o, gate|up, down + the lm_head; q|k|v stayed on gemm
    assert all("wqkv" not in ly["q4"] for ly in model.llm.layers)
    n1 = H.GEMM_W4_CALLS
    ids_base = base._generate_step(ctx, pad_token_id=0, max_new_tokens=6, do_sample=False, eos_token_id=[])
    assert H.GEMM_W4_CALLS - n1 == 5 * (4 * d.llm_layers + 1)
    assert ids.shape == (2, 6) and ids_base.shape == (2, 6)


def test_mxfp4_decode_with_orca_injection(golden_dir):
    """ORCA tiny config: the injection's own (trainable) projections stay bf16, the LLM's stream MXFP4; per-step logits against the
    ORCA oracle on the same snapped weights within the bound tests/test_gpu_orca.py holds the bf16 decode to."""
    import orca_oracle as R
    from test_gpu_orca import _case, _oracle_with_theta
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    g, d, o, w, batch, cfg = _case(golden_dir, False)
    w = snap_llm_weights_mx(w)
    model = DeSTA25AudioModel(cfg, weights=w).eval()
    model.set_decode_weights("mxfp4")
    orig = _oracle_with_theta(float(g["rope_theta_used"]))
    try:
        inputs = _gen_inputs(g, batch)
        T = g["gen_ids"].shape[1]
        with torch.no_grad():
            ref_ids = R.generate(w, d, o, inputs, T, 0)[0]
            lo = R.generate(w, d, o, inputs, T, 0, forced_tokens=ref_ids)[1]
        n0 = H.GEMM_W4_CALLS
        ids, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref_ids, collect_logits=True,
                                           eos_token_id=[])
        assert H.GEMM_W4_CALLS > n0
        assert ids.cpu().tolist() == ref_ids.tolist()
        _check_against_oracle("orca", logits, lo, T)
    finally:
        R.rope_whole_vector = orig
