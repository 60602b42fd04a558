"""GPU: the row-wise training kernels of csrc/norm_act.hip and csrc/embed_ce.hip held PER ELEMENT to a float64 reference.

Reference, bounds with their derivation, the conforming emulation and the rounding points it reproduces: tests/rowwise_reference.py.
The instrument itself is proved on the CPU by tests/test_rowwise_bound_host.py, over the case table this file runs
(rowwise_reference.CASES: the dispatch edges of LN_DISPATCH, the grid caps, the three loss kernels and their scalar tails).

Every output of every kernel is asserted element by element:
    |out - fp64| <= 2 x bound        (`FACTOR`: what the emulation leaves out - fp32 accumulation order, fused multiply-adds,
                                      __expf / __logf / rsqrtf / erff; where the bound is 0 the output must be exact)
and `max |err| / bound` is printed per case (run with -s).  Every output buffer starts as the sentinel 7.0 and is followed by
64 guard elements that must still hold it; the columns a kernel must not touch (V heads and padding of RoPE, [V, ld) of the
logits, the logits under write_grad = 0) are compared bit for bit.  LayerNorm backward, the loss and the prompt gradient are
run twice and must agree bit for bit.

Which new test a kernel error turns red while test_gpu_ops.py stays green (host evidence: test_rowwise_bound_host.py):
`eps` -> 1e-2 or rstd x 1.003 in rmsnorm_fwd_k: test_rmsnorm_fwd (the old rel-L2 6e-3 passes both); non-target gradients
of ce_row_k 2 % high: test_causal_lm_loss[V=50257...rows=randn]; an unwritten scalar tail of ce_row_k: every V % 8 != 0 case
(the old test has none); silu not rounded in swiglu_fwd_k: test_elementwise[swiglu_fwd-*].
Tried by hand on the MI355X with `+ eps` replaced by `+ 1e-2f` in rmsnorm_fwd_k: test_gpu_ops.py::test_rmsnorm_fwd_bwd passed its
3 cases, test_rmsnorm_fwd here failed all 20 (rstd off by 300 ... 5000 bounds).

Measured on the MI355X: profiles/r14_rowwise_fp64_tests.log and the table in DESIGN.md ("Row-wise kernels against fp64")."""
import math

import pytest
import torch

import rowwise_reference as R

pytestmark = pytest.mark.gpu

FACTOR = 2.0
GUARD = 64


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _ids(op):
    return [R.case_id(c) for c in R.CASES[op]]


def _dev(o):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in o.items()}


def guarded(shape, dtype, fill=R.SENTINEL):
    """a sentinel-filled output of `shape` followed by GUARD sentinel elements -> (whole buffer, the output's view)"""
    n = math.prod(shape)
    full = torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")
    return full, full[:n].view(*shape)


def intact(*fulls):
    return all(bool((f[-GUARD:] == R.SENTINEL).all()) for f in fulls)


def check(op, case, o, outs, ref=None):
    """assert every output within FACTOR x bound of the float64 reference; print the ratios -> ratios"""
    ref = R.OPS[op].exact(o) if ref is None else ref
    ratios = {n: R.ratio(op, o, ref, n, outs[n].to(ref[n].device)) for n in R.OPS[op].outputs if n in outs}
    print(f"\n{op} {R.case_id(case)}: " + " ".join(f"{n} {r:.3f}" for n, r in ratios.items()), end="")
    for n, r in ratios.items():
        assert r <= FACTOR, (op, R.case_id(case), n, r)
    return ratios


# ------------------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("case", R.CASES["layernorm_fwd"], ids=_ids("layernorm_fwd"))
def test_layernorm_fwd(hip, case):
    o = R.operands("layernorm_fwd", case)
    rows, cols = o["x"].shape
    f16, y16 = guarded((rows, cols), torch.bfloat16)
    f32, y32 = guarded((rows, cols), torch.float32)
    fst, st = guarded((rows, 2), torch.float32)
    hip.layernorm_fwd(o["x"].cuda(), o["gamma"].cuda(), o["beta"].cuda(), o["eps"], y16=y16, y32=y32, stats=st)
    torch.cuda.synchronize()
    assert intact(f16, f32, fst)
    outs = {"y16": y16.cpu(), "y32": y32.cpu(), "mean": st[:, 0].cpu(), "rstd": st[:, 1].cpu()}
    check("layernorm_fwd", case, o, outs)
    if case["data"] == "edges":                                        # the constant row: variance 0, y = beta exactly
        assert torch.equal(outs["y32"][2], o["beta"]) and torch.equal(outs["y16"][2], o["beta"].bfloat16())
        assert float(outs["mean"][2]) == R.EDGE_CONST
    # one output at a time: the same bits
    f16b, y16b = guarded((rows, cols), torch.bfloat16)
    f32b, y32b = guarded((rows, cols), torch.float32)
    hip.layernorm_fwd(o["x"].cuda(), o["gamma"].cuda(), o["beta"].cuda(), o["eps"], y16=y16b)
    hip.layernorm_fwd(o["x"].cuda(), o["gamma"].cuda(), o["beta"].cuda(), o["eps"], y32=y32b)
    assert torch.equal(f16b, f16) and torch.equal(f32b, f32)


@pytest.mark.parametrize("case", R.CASES["layernorm_bwd"], ids=_ids("layernorm_bwd"))
def test_layernorm_bwd(hip, case):
    o = R.operands("layernorm_bwd", case)
    rows, cols = o["x"].shape
    d = _dev(o)
    runs = []
    for _ in range(2):
        f32, dx32 = guarded((rows, cols), torch.float32)
        f16, dx16 = guarded((rows, cols), torch.bfloat16)
        fg, dg = guarded((cols,), torch.float32)
        fb, db = guarded((cols,), torch.float32)
        if case["accumulate"]:
            dg.copy_(o["prev"][0])
            db.copy_(o["prev"][1])
        hip.layernorm_bwd(d["dy"], d["x"], d["gamma"], d["stats"], dx32=dx32, dx16=dx16, dgamma=dg, dbeta=db,
                          accumulate=case["accumulate"])
        torch.cuda.synchronize()
        assert intact(f32, f16, fg, fb)
        runs.append((f32, f16, fg, fb))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs differ"
    f32, f16, fg, fb = runs[0]
    outs = {"dx32": f32[:-GUARD].view(rows, cols).cpu(), "dx16": f16[:-GUARD].view(rows, cols).cpu(),
            "dgamma": fg[:-GUARD].cpu(), "dbeta": fb[:-GUARD].cpu()}
    check("layernorm_bwd", case, o, outs)
    # dx alone (no partial sums, no reduction): the same bits
    f32b, dx32b = guarded((rows, cols), torch.float32)
    hip.layernorm_bwd(d["dy"], d["x"], d["gamma"], d["stats"], dx32=dx32b)
    assert torch.equal(f32b, f32)


@pytest.mark.parametrize("case", R.CASES["rmsnorm_fwd"], ids=_ids("rmsnorm_fwd"))
def test_rmsnorm_fwd(hip, case):
    o = R.operands("rmsnorm_fwd", case)
    rows, cols = o["x"].shape
    fy, y = guarded((rows, cols), torch.bfloat16)
    fr, rstd = guarded((rows,), torch.float32)
    hip.rmsnorm_fwd(o["x"].cuda(), o["w"].cuda(), o["eps"], y, rstd)
    torch.cuda.synchronize()
    assert intact(fy, fr)
    check("rmsnorm_fwd", case, o, {"y": y.cpu(), "rstd": rstd.cpu()})
    fy2, y2 = guarded((rows, cols), torch.bfloat16)
    hip.rmsnorm_fwd(o["x"].cuda(), o["w"].cuda(), o["eps"], y2)          # without the rstd output
    assert torch.equal(fy2, fy)


@pytest.mark.parametrize("case", R.CASES["rmsnorm_bwd"], ids=_ids("rmsnorm_bwd"))
def test_rmsnorm_bwd(hip, case):
    o = R.operands("rmsnorm_bwd", case)
    rows, cols = o["x"].shape
    d = _dev(o)
    fx, dx = guarded((rows, cols), torch.bfloat16)
    hip.rmsnorm_bwd(d["dy"], d["x"], d["w"], d["rstd"], dx, dres=d["dres"])
    torch.cuda.synchronize()
    assert intact(fx)
    check("rmsnorm_bwd", case, o, {"dx": dx.cpu()})


def test_norm_rejections(hip):
    def bufs(rows, cols):
        return (torch.zeros(rows, cols, dtype=torch.bfloat16, device="cuda"), torch.ones(cols, device="cuda"),
                torch.zeros(rows, cols, dtype=torch.bfloat16, device="cuda"), torch.ones(rows, 2, device="cuda"))
    for cols, ln_fwd_too in ((12, True), (8200, True), (4104, False)):
        x, w, y, st = bufs(2, cols)
        if ln_fwd_too:
            with pytest.raises(RuntimeError):
                hip.layernorm_fwd(x, w, w, 1e-5, y16=y)
            with pytest.raises(RuntimeError):
                hip.rmsnorm_fwd(x, w, 1e-5, y, st[:, 0].contiguous())
            with pytest.raises(RuntimeError):
                hip.rmsnorm_bwd(x, x, w, st[:, 0].contiguous(), y)
        with pytest.raises(RuntimeError):
            hip.layernorm_bwd(x, x, w, st, dx16=y)
        assert float(y.float().abs().max()) == 0.0                     # a rejected call writes nothing


# ------------------------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("case", R.CASES["rope"], ids=_ids("rope"))
def test_rope(hip, case):
    o = R.operands("rope", case)
    rows, ld = o["buf"].shape
    d = _dev(o)
    full, buf = guarded((rows, ld), torch.bfloat16)
    buf.copy_(d["buf"])
    hip.rope(buf, ld, rows, o["seq"], o["n_q"], o["n_kv"], o["hd"], d["cos_sin"], d["wq"], d["wk"], o["eps"],
             pre_norm=d["pre"], ld_pre=o.get("ld_pre", 0), backward=o["backward"], pos_shift=d["pos_shift"],
             s_major_batch=o["s_major_batch"])
    torch.cuda.synchronize()
    assert intact(full)
    nhd = (o["n_q"] + o["n_kv"]) * o["hd"]
    assert torch.equal(buf[:, nhd:].cpu(), o["buf"][:, nhd:])          # V heads and padding: bit for bit
    check("rope", case, o, {"out": buf.cpu()})


# ------------------------------------------------------------------------------------------------------------ SwiGLU / GELU'
@pytest.mark.parametrize("case", R.CASES["swiglu_fwd"], ids=_ids("swiglu_fwd"))
@pytest.mark.parametrize("op", R.ELEMENTWISE)
def test_elementwise(hip, op, case):
    o = _dev(R.operands(op, case))                                     # the reference runs on the device (float64, row chunks)
    rows, I = case["rows"], case["I"]
    name = R.OPS[op].outputs[0]
    full, out = guarded((rows, 2 * I if op == "swiglu_bwd" else I), torch.bfloat16)
    if op == "swiglu_fwd":
        hip.swiglu_fwd(o["gu"], out, rows, I)
    elif op == "swiglu_bwd":
        hip.swiglu_bwd(o["gu"], o["dact"], out, rows, I)
    else:
        hip.gelu_bwd(o["pre"], o["dact"], out, rows * I)
    torch.cuda.synchronize()
    assert intact(full)
    assert bool(torch.isfinite(out.float()).all())                      # +-100 saturate, no NaN
    worst = 0.0
    for sl, oc in R.row_chunks(op, o):
        worst = max(worst, R.ratio(op, oc, R.OPS[op].exact(oc), name, out[sl]))
    print(f"\n{op} {R.case_id(case)}: {name} {worst:.3f}", end="")
    assert worst <= FACTOR, (op, case, worst)


# ------------------------------------------------------------------------------------------------------------ causal-LM loss
@pytest.mark.parametrize("case", R.CASES["causal_lm_loss"], ids=_ids("causal_lm_loss"))
def test_causal_lm_loss(hip, case):
    o = R.operands("causal_lm_loss", case)
    V, ld, M = o["V"], o["ld"], R.CE_B * R.CE_S
    ref = R.OPS["causal_lm_loss"].exact(o)
    labels = o["labels"].cuda()
    runs = []
    for _ in range(2):
        full, buf = guarded((M, ld), torch.bfloat16)
        buf.copy_(o["logits"])                                          # columns [V, ld) hold the sentinel
        floss, loss = guarded((1,), torch.float32)
        hip.causal_lm_loss(buf, ld, labels, R.CE_B, R.CE_S, V, loss, write_grad=case["write_grad"])
        torch.cuda.synchronize()
        assert intact(full, floss)
        runs.append((full, floss))
    assert all(torch.equal(a, b) for a, b in zip(*runs)), "two runs differ"
    got = runs[0][0][:-GUARD].view(M, ld).cpu()
    assert torch.equal(got[:, V:], o["logits"][:, V:])                  # [V, ld) untouched
    if not case["write_grad"]:
        assert torch.equal(got, o["logits"])
    check("causal_lm_loss", case, o, {"loss": runs[0][1][0].cpu(), "dlogits": got}, ref=ref)
    if case["labels"] == "ignored":
        assert float(runs[0][1][0]) == 0.0 and float(got[:, :V].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ tap mix, prompts
@pytest.mark.parametrize("case", R.CASES["tap_mix_fwd"], ids=_ids("tap_mix_fwd"))
def test_tap_mix(hip, case):
    taps, B, K, dd = case["taps"], case["batch"], case["prompt"], case["d"]
    o = R.operands("tap_mix_fwd", case)
    d = _dev(o)
    fo, out = guarded((B * K, dd), torch.float32)
    hip.tap_mix_fwd(d["x"], d["lw"], taps, B, K, dd, out)
    torch.cuda.synchronize()
    assert intact(fo)
    check("tap_mix_fwd", case, o, {"out": out.cpu()})
    o = R.operands("tap_mix_bwd", case)
    d = _dev(o)
    fx, dx = guarded((taps, B * K, dd), torch.float32)
    fl, dlw = guarded((K, taps), torch.float32)
    hip.tap_mix_bwd(d["x"], d["lw"], d["dout"], taps, B, K, dd, dx, dlw)
    torch.cuda.synchronize()
    assert intact(fx, fl)
    check("tap_mix_bwd", case, o, {"dx": dx.cpu(), "dlw": dlw.cpu()})


def test_tap_mix_rejects_33_taps(hip):
    x, lw, out = torch.zeros(33, 2, 8, device="cuda"), torch.zeros(2, 33, device="cuda"), torch.zeros(2, 8, device="cuda")
    with pytest.raises(RuntimeError):
        hip.tap_mix_fwd(x, lw, 33, 1, 2, 8, out)
    with pytest.raises(RuntimeError):
        hip.tap_mix_bwd(x, lw, out, 33, 1, 2, 8, torch.zeros_like(x), torch.zeros_like(lw))


@pytest.mark.parametrize("case", R.CASES["prompt_expand"], ids=_ids("prompt_expand"))
def test_prompt_expand_and_grad(hip, case):
    taps, B, n = case["taps"], case["batch"], case["n"]
    o = R.operands("prompt_expand", case)
    f32, x32 = guarded((taps * B, n), torch.float32)
    f16, x16 = guarded((taps * B, n), torch.bfloat16)
    hip.prompt_expand(o["prompts"].cuda(), taps, B, n, x32, x16)
    torch.cuda.synchronize()
    assert intact(f32, f16)
    check("prompt_expand", case, o, {"x32": x32.cpu(), "x16": x16.cpu()})      # bound 0: the copy and its rounding are exact
    o = R.operands("prompt_grad", case)
    runs = []
    for _ in range(2):
        fg, dp = guarded((taps, n), torch.float32)
        hip.prompt_grad(o["dx"].cuda(), taps, B, n, dp)
        torch.cuda.synchronize()
        assert intact(fg)
        runs.append(fg)
    assert torch.equal(runs[0], runs[1]), "two runs differ"
    check("prompt_grad", case, o, {"dprompts": runs[0][:-GUARD].view(taps, n).cpu()})


def test_cast_and_add_beyond_the_grid_cap(hip):
    """cast_f32_bf16_k and add_f32_k cap their grid at 8192 blocks (nblocks) and stride beyond: one size each that takes a second
    pass, ragged in its last block.  Both are exact: round-to-nearest-even, and one fp32 add."""
    g = torch.Generator().manual_seed(11)
    n = (8192 * 256 + 300) * 8
    x = torch.randn(n, generator=g).cuda()
    full, y = guarded((n,), torch.bfloat16)
    hip.cast_bf16(x, y)
    torch.cuda.synchronize()
    assert intact(full) and torch.equal(y, x.bfloat16())
    n = (8192 * 256 + 300) * 4
    a, b = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    full, acc = guarded((n,), torch.float32)
    acc.copy_(a)
    hip.add_f32(acc, b)
    torch.cuda.synchronize()
    assert intact(full) and torch.equal(acc, a + b)
