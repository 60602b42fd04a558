"""GPU: classifier-free guidance of generate() — `desta_cfg_scores_bf16` against float64 within a derived per-element bound
(tests/guidance_reference.py) and against the spelled-out fp32 formula bit for bit, the guided decode loop against the logits it
collected and against the oracle on the 2 Bc batch, its combinations and refusals, and the chat-level surface."""
import copy
import types

import pytest
import torch

import desta_oracle as O
import guidance_reference as GR
from helpers import GENERATE_MESSAGES, ToyTokenizer, cfg_from_dims, golden_batch, rel_err
from test_gpu_fp8_decode import _gen_inputs
from test_gpu_generate_logprobs import _check_against_logits

pytestmark = pytest.mark.gpu

NEG_INF = GR.NEG_INF
KERNEL_CASES = [(511, 511), (4099, 4104), (128256, 128256), (151936, 151944)]
SCALES = [1.5, 4.0]
SENTINEL = 123.0                                                                    # exact in bf16


# ------------------------------------------------------------------------------------------------ kernel
_ROWS = {}


def _rows(V, ld):
    """Eight crafted bf16 row pairs (cond, uncond) [8, ld]; entries >= V are random, so a kernel that reads them gets a wrong sum."""
    if (V, ld) in _ROWS:
        return _ROWS[(V, ld)]
    g = torch.Generator().manual_seed(31 + V)
    rn = lambda: (3.0 * torch.randn(8, ld, generator=g)).to(torch.bfloat16)
    c, u = rn(), rn()                                                               # row 0: N(0, 3^2) against an independent N(0, 3^2)
    c[1] = (160.0 * torch.rand(ld, generator=g) - 80.0).to(torch.bfloat16)          # row 1: +-80 against +-80
    u[1] = (160.0 * torch.rand(ld, generator=g) - 80.0).to(torch.bfloat16)
    u[2] = c[2]                                                                     # row 2: uncond == cond
    c[3], u[3] = 1.5, -2.0                                                          # row 3: every entry equal
    c[3, V:], u[3, V:] = 9.0, 9.0
    c[4, torch.randperm(V, generator=g)[: V // 3]] = NEG_INF                        # row 4: a third of cond at -inf
    perm = torch.randperm(V, generator=g)                                           # row 5: uncond alone at -inf, both, cond alone
    u[5, perm[: V // 4]] = NEG_INF
    c[5, perm[V // 8: V // 4 + V // 8]] = NEG_INF
    a, b = (int(i) for i in torch.randperm(V, generator=g)[:2])                     # row 6: guidance moves the argmax from a to b
    c[6], u[6] = (c[6].float() / 3.0).to(torch.bfloat16), (u[6].float() / 3.0).to(torch.bfloat16)
    c[6, a], c[6, b], u[6, a], u[6, b] = 12.0, 11.5, 12.0, 0.0
    _ROWS[(V, ld)] = (c, u, a, b)                                                   # row 7: run on its own at scale 1
    return _ROWS[(V, ld)]


def _device_layout(c, u, ld, rows):
    """cond contiguous; uncond 3 elements into its allocation (three pointers, three alignments); out with ld_out = ld + 8, one
    sentinel row behind `rows`, everything preset to SENTINEL."""
    cd = c[:rows].cuda().contiguous()
    flat = torch.zeros(3 + rows * ld + 5, dtype=torch.bfloat16, device="cuda")
    ud = flat[3:3 + rows * ld].view(rows, ld)
    ud.copy_(u[:rows])
    out = torch.full((rows + 1, ld + 8), SENTINEL, dtype=torch.bfloat16, device="cuda")
    assert cd.data_ptr() % 16 == 0 and ud.data_ptr() % 16 == 6 and out.data_ptr() % 16 == 0
    return cd, ud, out


def _run(H, cd, ud, ld, rows, V, g, out):
    H.cfg_scores(cd, ud, ld, rows, V, g, out, out.shape[1])
    torch.cuda.synchronize()
    assert bool((out[rows:] == SENTINEL).all()) and bool((out[:rows, V:] == SENTINEL).all())     # nothing behind rows, nothing behind V
    return out[:rows, :V]


@pytest.mark.parametrize("g", SCALES)
@pytest.mark.parametrize("V,ld", KERNEL_CASES)
def test_kernel_vs_float64(V, ld, g):
    from desta import _hip as H
    c, u, a, b = _rows(V, ld)
    cd, ud, out = _device_layout(c, u, ld, 8)
    c0, u0 = cd.clone(), ud.clone()
    got = _run(H, cd, ud, ld, 8, V, g, out).cpu()
    worst = GR.check_scores(got, c[:, :V], u[:, :V], g)                             # every finite element; -inf exactly; no NaN
    print(f"V={V} ld={ld} g={g}: worst |out - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(cd.view(torch.int16), c0.view(torch.int16)) and torch.equal(ud.view(torch.int16), u0.view(torch.int16))
    # the crafted rows say what they were built to say
    R, Lc, Lu = GR.guided_scores_fp64(c[:, :V], u[:, :V], g)
    dead5 = torch.isinf(c[5, :V].float()) | torch.isinf(u[5, :V].float())
    only_u = torch.isinf(u[5, :V].float()) & ~torch.isinf(c[5, :V].float())
    assert int(only_u.sum()) > 0 and int((torch.isinf(u[5, :V].float()) & torch.isinf(c[5, :V].float())).sum()) > 0
    assert bool((got[5][dead5] == NEG_INF).all()) and bool(torch.isfinite(got[5][~dead5]).all())
    assert int(torch.isinf(got[4]).sum()) == V // 3
    assert int(c[6, :V].float().argmax()) == a and int(R[6].argmax()) == b and int(got[6].float().argmax()) == b
    assert bool((got[3] == got[3, 0]).all()) and abs(float(got[3, 0]) + torch.log(torch.tensor(float(V))).item()) <= 2.0 ** -8 * 12 + 1e-4
    # uncond == cond: g (lc - lu) + lu is lc, so the output is bf16(lc) — lc's bits are known at the ids desta_topk_logprobs ranks
    n = min(32, V)
    ids = torch.zeros(8, n, dtype=torch.int32, device="cuda")
    top = torch.zeros(8, n, dtype=torch.float32, device="cuda")
    H.topk_logprobs(cd, ld, None, 8, V, n, None, ids, top)
    assert torch.equal(got[2][ids[2].cpu().long()].view(torch.int16), top[2].cpu().to(torch.bfloat16).view(torch.int16))
    assert float((got[2].double() - Lc[2]).abs().max()) <= float(GR.guided_bound(Lc[2], Lc[2], Lc[2], g).max())
    # row 7 at scale 1, a call of its own: fl(fl(lc - lu) + lu), the conditional log-softmax to within the same bound
    out1 = torch.full((2, ld + 8), SENTINEL, dtype=torch.bfloat16, device="cuda")
    got1 = _run(H, cd[7:], ud[7:], ld, 1, V, 1.0, out1).cpu()
    worst1 = GR.check_scores(got1, c[7:, :V], u[7:, :V], 1.0)
    print(f"V={V} ld={ld} scale 1: worst / bound = {worst1:.3f}")
    assert worst1 <= 1.0
    assert float(((got1[0].double() - Lc[7]).abs() / GR.guided_bound(Lc[7], Lc[7], Lu[7], 1.0)).max()) <= 1.0


@pytest.mark.parametrize("V,ld", KERNEL_CASES)
def test_kernel_bits(V, ld):
    """At the <= 32 ids per row that desta_topk_logprobs ranks on `cond`: lc from that kernel, lu from desta_token_logprobs on
    `uncond`, the spelled-out fp32 formula on the host, rounded to bf16 — the kernel's bits must be those."""
    from desta import _hip as H
    c, u, _, _ = _rows(V, ld)
    cd, ud, out = _device_layout(c, u, ld, 8)
    c0, u0 = cd.clone(), ud.clone()
    n = min(32, V)
    ids = torch.zeros(8, n, dtype=torch.int32, device="cuda")
    lc = torch.zeros(8, n, dtype=torch.float32, device="cuda")
    H.topk_logprobs(cd, ld, None, 8, V, n, None, ids, lc)
    lu = torch.zeros(8, n, dtype=torch.float32, device="cuda")
    col = torch.zeros(8, dtype=torch.float32, device="cuda")
    for j in range(n):
        H.token_logprobs(ud, ld, ids[:, j].long().contiguous(), 8, V, col)
        lu[:, j] = col
    idx, lc, lu = ids.cpu().long(), lc.cpu(), lu.cpu()
    dead = torch.isinf(c[:, :V].float().gather(1, idx)) | torch.isinf(u[:, :V].float().gather(1, idx))
    assert int(dead.sum()) > 0 and int((~dead).sum()) > 6 * n                       # both kinds of entry are among the ranked ones
    for g in SCALES:
        got = _run(H, cd, ud, ld, 8, V, g, out)
        d = lc - lu                                                                 # three fp32 roundings, one after the other
        t = d * torch.tensor(g, dtype=torch.float32)
        o = t + lu
        want = torch.where(dead, torch.full_like(o, NEG_INF), o).to(torch.bfloat16)
        assert torch.equal(got.cpu().gather(1, idx).view(torch.int16), want.view(torch.int16)), g
        again = _run(H, cd, ud, ld, 8, V, g, torch.full_like(out, SENTINEL))       # a rerun repeats every bit
        assert torch.equal(again.view(torch.int16), got.view(torch.int16))
        alone = _run(H, cd[5:], ud[5:], ld, 1, V, g, torch.full((2, ld + 8), SENTINEL, dtype=torch.bfloat16, device="cuda"))
        assert torch.equal(alone[0].view(torch.int16), got[5].view(torch.int16))   # independent of rows
    assert torch.equal(cd.view(torch.int16), c0.view(torch.int16)) and torch.equal(ud.view(torch.int16), u0.view(torch.int16))


def test_kernel_argument_checks():
    from desta import _hip as H
    V, ld = 511, 511
    c, u, _, _ = _rows(V, ld)
    cd, ud, out = _device_layout(c, u, ld, 8)
    lo = out.shape[1]
    raw, st, p = H._cfg_scores, H.stream(), H.p
    n0 = H.CFG_SCORES_CALLS
    assert raw(0, p(ud), ld, 8, V, 2.0, p(out), lo, st) == -1                       # NULL pointers
    assert raw(p(cd), 0, ld, 8, V, 2.0, p(out), lo, st) == -1
    assert raw(p(cd), p(ud), ld, 8, V, 2.0, 0, lo, st) == -1
    assert raw(p(cd), p(ud), ld, 0, V, 2.0, p(out), lo, st) == -1                   # rows <= 0
    assert raw(p(cd), p(ud), ld, -3, V, 2.0, p(out), lo, st) == -1
    assert raw(p(cd), p(ud), V - 1, 8, V, 2.0, p(out), lo, st) == -1                # ld < vocab
    assert raw(p(cd), p(ud), ld, 8, V, 2.0, p(out), V - 1, st) == -1                # ld_out < vocab
    assert raw(p(cd), p(ud), ld, 8, 0, 2.0, p(out), lo, st) == -1                   # vocab outside 1..262144
    assert raw(p(cd), p(ud), 262152, 8, 262145, 2.0, p(out), 262152, st) == -1
    for bad in (0.0, -1.5, float("inf"), float("-inf"), float("nan")):              # guidance_scale finite and > 0
        assert raw(p(cd), p(ud), ld, 8, V, bad, p(out), lo, st) == -1, bad
    assert raw(p(cd), p(ud), ld, 8, V, 2.0, p(cd), ld, st) == -1                    # out == cond, out == uncond
    assert raw(p(cd), p(ud), ld, 8, V, 2.0, p(ud), ld, st) == -1
    with pytest.raises(RuntimeError, match="desta_cfg_scores_bf16"):
        H.cfg_scores(cd, ud, V - 8, 8, V, 2.0, out, lo)
    torch.cuda.synchronize()
    assert H.CFG_SCORES_CALLS == n0 and bool((out == SENTINEL).all())               # a refused call launched nothing
    assert torch.equal(cd.cpu().view(torch.int16), c[:8].view(torch.int16))


def test_kernel_largest_guided_batch():
    from desta import _hip as H
    rows, V, ld, g = 32, 4099, 4104, 4.0
    gen = torch.Generator().manual_seed(9)
    c = (3.0 * torch.randn(rows, ld, generator=gen)).to(torch.bfloat16)
    u = (3.0 * torch.randn(rows, ld, generator=gen)).to(torch.bfloat16)
    u[17, :V:5] = NEG_INF
    cd, ud, out = _device_layout(c, u, ld, rows)
    got = _run(H, cd, ud, ld, rows, V, g, out).cpu()
    worst = GR.check_scores(got, c[:, :V], u[:, :V], g)
    print(f"rows=32 V={V}: worst |out - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ decode loop
_MODELS = {}
KW = dict(pad_token_id=0, max_new_tokens=10, eos_token_id=[])


def _setup(golden_dir, name):
    """One model per tiny golden, the 2 Bc inputs, the plain greedy run of the conditional rows alone and the guided greedy run
    at g = 3, shared by the tests below (none of them changes any of it)."""
    if name not in _MODELS:
        from desta import _hip as H
        from desta.models.modeling_desta25 import DeSTA25AudioModel
        d = O.tiny_dims(name == "qwen3")
        g, batch = golden_batch(golden_dir, name)
        w = O.init_weights(d, seed=7)
        model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
        inputs2 = GR.guided_inputs(g, batch)
        plain = model._generate_step(_gen_inputs(g, batch), do_sample=False, **KW)
        n0 = H.CFG_SCORES_CALLS
        ids, lg = model._generate_step(inputs2, do_sample=False, collect_logits=True, guidance_scale=3.0, **KW)
        _MODELS[name] = types.SimpleNamespace(model=model, d=d, w=w, g=g, batch=batch, inputs2=inputs2, plain=plain, ids=ids, lg=lg,
                                              launches=H.CFG_SCORES_CALLS - n0)
    return _MODELS[name]


def _picks_follow(ids, lg, g):
    """Every counting (step, row) cell of a guided greedy run equals the fp64 guided argmax of the run's own logits -> share counting."""
    want, counts = GR.pick_cells(lg, g)
    got = ids.cpu().t()
    assert torch.equal(got[counts], want[counts]), (got.tolist(), want.tolist(), counts.tolist())
    return float(counts.float().mean())


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_scale_none_and_one_are_the_plain_call(golden_dir, name):
    from desta import _hip as H
    s = _setup(golden_dir, name)
    n0 = H.CFG_SCORES_CALLS
    ids0, lg0 = s.model._generate_step(s.inputs2, do_sample=False, collect_logits=True, **KW)
    for scale in (None, 1.0, 1):
        ids, lg = s.model._generate_step(s.inputs2, do_sample=False, collect_logits=True, guidance_scale=scale, **KW)
        assert ids.shape == (4, 10) and torch.equal(ids, ids0) and torch.equal(lg.view(torch.int16), lg0.view(torch.int16))
    assert H.CFG_SCORES_CALLS == n0


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_guided_greedy_follows_its_own_logits(golden_dir, name):
    s = _setup(golden_dir, name)
    assert s.launches == 10                                                         # exactly one launch per step
    assert s.ids.shape == (2, 10) and s.ids.dtype == torch.int64 and s.lg.shape == (10, 4, s.d.vocab)
    share = _picks_follow(s.ids, s.lg, 3.0)
    differs = (s.ids != s.plain).sum(dim=1).tolist()
    print(f"{name}: g = 3, cells counting {share:.2f}, picks differing from plain greedy per row {differs}")
    assert share >= 0.75
    assert min(differs) >= 1
    again, lg2 = s.model._generate_step(s.inputs2, do_sample=False, collect_logits=True, guidance_scale=3.0, **KW)
    assert torch.equal(again, s.ids) and torch.equal(lg2.view(torch.int16), s.lg.view(torch.int16))


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_both_halves_match_the_oracle_teacher_forced(golden_dir, name):
    """Teacher-forced on the guided run's tokens, all 2 Bc rows against the fp32 oracle at the bound of the decode-against-oracle
    tests (3e-2 relative L2 per step, tests/test_gpu_generate.py, tests/test_gpu_fp8_decode.py): the second half really is the
    negative prompt, at its own positions (one negative row is 5 tokens shorter)."""
    s = _setup(golden_dir, name)
    forced = s.ids.cpu()
    ids, lg = s.model._generate_step(s.inputs2, do_sample=False, collect_logits=True, guidance_scale=3.0, forced_tokens=forced, **KW)
    assert torch.equal(ids.cpu(), forced) and torch.equal(lg.view(torch.int16), s.lg.view(torch.int16))
    lo = GR.oracle_forced_logits(s.w, s.d, s.inputs2, forced)
    assert lo.shape == lg.shape
    es = [[rel_err(lg[t, rows].float(), lo[t, rows]) for t in range(10)] for rows in (slice(0, 4), slice(0, 2), slice(2, 4))]
    print(f"{name}: per-step logits rel-L2 vs oracle: all rows {max(es[0]):.4f}, conditional {max(es[1]):.4f}, unconditional {max(es[2]):.4f}")
    assert max(max(e) for e in es) < 3e-2, es
    assert rel_err(lg[0, 2:].float(), lo[0, :2]) > 3e-2                              # and the halves do differ: it is not the same prompt twice


def test_guided_sampling_chain(golden_dir):
    from desta import _hip as H
    s = _setup(golden_dir, "llama")
    kw = dict(do_sample=True, top_k=20, seed=3, repetition_penalty=1.3, logprobs=5, collect_logits=True, guidance_scale=3.0, **KW)
    n0 = H.TOPK_LOGPROBS_CALLS
    ids, lg, lp = s.model._generate_step(s.inputs2, **kw)
    assert H.TOPK_LOGPROBS_CALLS - n0 == 10 and ids.shape == (2, 10) and lg.shape == (10, 4, s.d.vocab)
    # the test's own replay: cfg_scores of the collected logits, then the sampler with the loop's seed / step / history
    V, Vp = s.d.vocab, s.model.llm.Vp
    raw = torch.zeros(4, Vp, dtype=torch.bfloat16, device="cuda")
    scores = torch.zeros(2, Vp, dtype=torch.bfloat16, device="cuda")
    hist = torch.zeros(2, 10, dtype=torch.int64, device="cuda")
    nxt = torch.zeros(2, dtype=torch.int64, device="cuda")
    for t in range(10):
        raw[:, :V] = lg[t]
        H.cfg_scores(raw[:2], raw[2:], Vp, 2, V, 3.0, scores, Vp)
        H.sample(scores, Vp, 2, V, nxt, do_sample=True, temperature=0.7, top_k=20, top_p=0.9, min_p=0.0, repetition_penalty=1.3,
                 hist=hist, hist_len=t, seed=3, step=t)
        assert torch.equal(nxt, ids[:, t]), t
        hist[:, t] = nxt
    worst = _check_against_logits(lp, ids, lg[:, :2], 5)                            # the model's own distribution: the raw conditional rows
    print(f"guided sampling: worst |logprob - fp64 of the raw conditional logits| / bound = {worst:.3f}")
    assert worst <= 1.0
    ids2, lg2, lp2 = s.model._generate_step(s.inputs2, **kw)
    assert torch.equal(ids2, ids) and torch.equal(lg2.view(torch.int16), lg.view(torch.int16))
    for a, b in ((lp.token_logprobs, lp2.token_logprobs), (lp.top_ids, lp2.top_ids), (lp.top_logprobs, lp2.top_logprobs)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ combinations and refusals
def test_guided_with_fp8_weights_fp8_cache_and_chunked_prefill(golden_dir):
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = O.tiny_dims(True)                                                           # Qwen3: head_dim 128, which the FP8 cache needs
    g, batch = golden_batch(golden_dir, "qwen3")
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=O.init_weights(d, seed=7))
    model.set_decode_weights("fp8")
    model.set_kv_cache("fp8")
    model.set_prefill_chunk(16)
    n0 = H.CFG_SCORES_CALLS
    ids, lg = model._generate_step(GR.guided_inputs(g, batch), do_sample=False, collect_logits=True, guidance_scale=3.0, **KW)
    assert H.CFG_SCORES_CALLS - n0 == 10 and ids.shape == (2, 10) and lg.shape == (10, 4, d.vocab)
    share = _picks_follow(ids, lg, 3.0)
    print(f"fp8 weights + fp8 cache + chunked prefill: cells counting {share:.2f}")


def test_speculation_steps_aside(golden_dir):
    from desta import _hip as H
    s = _setup(golden_dir, "llama")
    s.model.set_speculative(3, scope="all")
    try:
        n0 = H.SPEC_ACCEPT_CALLS
        ids = s.model._generate_step(s.inputs2, do_sample=False, guidance_scale=3.0, **KW)
        assert H.SPEC_ACCEPT_CALLS == n0
        st = s.model.llm.spec_stats
        assert st["path"] == "plain" and st["reason"] == "guidance_scale"
        assert torch.equal(ids, s.ids)
    finally:
        s.model.set_speculative(None)


def test_orca_with_guidance_is_refused():
    import orca_oracle as R
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = copy.copy(O.tiny_dims(False))
    kg = 6
    o = R.OrcaDims(global_num_tokens=kg, local_downsample=4, local_kernel_size=5, global_cross_attn=True)
    w = R.init_weights(d, o, seed=11)
    d.prompt_size = kg
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=4,
                        orca_local_kernel_size=5, orca_global_cross_attn=True)
    model = DeSTA25AudioModel(cfg, weights=w).eval()
    batch = O.synthetic_batch(d, B=2, S_ctx=9, S_tgt=14, seed=4, pad=[3, 0])
    n_ctx = 9 + 3 + kg
    ids, am = batch["input_ids"][:, :n_ctx], batch["attention_mask"][:, :n_ctx]
    inputs = {"context_input_ids": torch.cat([ids, ids]), "context_attention_mask": torch.cat([am, am]),
              "context_batch_start_positions": batch["batch_start_positions"], "batch_features": batch["batch_features"],
              "batch_transcription_ids": batch["batch_transcription_ids"]}
    n0 = H.CFG_SCORES_CALLS
    with pytest.raises(NotImplementedError, match=r"guidance_scale.*ORCA"):
        model._generate_step(inputs, pad_token_id=0, max_new_tokens=4, do_sample=False, guidance_scale=2.0)
    assert H.CFG_SCORES_CALLS == n0


def test_row_limit_counts_both_halves(golden_dir):
    from desta import _hip as H
    s = _setup(golden_dir, "llama")
    ids = torch.randint(3, s.d.vocab, (66, 12), generator=torch.Generator().manual_seed(1))
    inputs = {"context_input_ids": ids, "context_attention_mask": torch.ones_like(ids), "context_batch_start_positions": [],
              "batch_features": None, "batch_transcription_ids": []}
    n0 = H.CFG_SCORES_CALLS
    with pytest.raises(ValueError, match=r"guidance_scale doubles the rows.*33 sequences are 66 rows"):
        s.model._generate_step(inputs, do_sample=False, guidance_scale=2.0, **KW)
    with pytest.raises(ValueError, match="even|one unconditional row each"):
        s.model._generate_step({**inputs, "context_input_ids": ids[:3], "context_attention_mask": torch.ones_like(ids[:3])}, do_sample=False,
                               guidance_scale=2.0, **KW)
    assert H.CFG_SCORES_CALLS == n0


# ------------------------------------------------------------------------------------------------ chat level
def _chat_model(golden_dir, tmp_path):
    import wave
    import numpy as np
    s = _setup(golden_dir, "llama")
    feats = s.g["batch_features"]

    class Proc:
        def __call__(self, waves, sampling_rate=None, return_tensors=None):
            return types.SimpleNamespace(input_features=feats[[i % feats.shape[0] for i in range(len(waves))]].cuda())
    msgs = copy.deepcopy(GENERATE_MESSAGES)
    for conv in msgs:
        for m in conv:
            for a in m.get("audios", []):
                p = tmp_path / a["audio"]
                with wave.open(str(p), "wb") as wv:
                    wv.setnchannels(1); wv.setsampwidth(2); wv.setframerate(16000)
                    wv.writeframes((0.1 * np.random.default_rng(len(a["audio"])).standard_normal(4000) * 32767).astype("<i2").tobytes())
                a["audio"] = str(p)
    tok = ToyTokenizer(vocab_size=s.d.vocab)
    s.model._setup_generation(tokenizer=tok, processor=Proc(), vad=lambda w: True, asr=lambda ws: ["spoken words"] * len(ws))
    return s, tok, msgs


def _left_pad(x, S, value):
    return torch.cat([torch.full((x.shape[0], S - x.shape[1]), value, dtype=x.dtype), x], dim=1)


def test_chat_generate_with_guidance(golden_dir, tmp_path):
    from desta import _hip as H
    from desta.models.modeling_desta25 import guidance_negative_messages
    s, tok, msgs = _chat_model(golden_dir, tmp_path)
    model = s.model
    before = copy.deepcopy(msgs)
    n0 = H.CFG_SCORES_CALLS
    out = model.generate(msgs, do_sample=False, max_new_tokens=6, guidance_scale=2.0)
    assert H.CFG_SCORES_CALLS - n0 == 6 and msgs == before
    assert len(out.generated_ids) == 2 and len(out.text) == 2 and all(len(r) == 6 for r in out.generated_ids)
    assert [t for _, t in out.audios] == ["hello world", "spoken words", ""] and len(out.audios) == 3      # the conditional conversations' audios
    # the same through _generate_step on inputs built by hand: conditional rows, then the chats without their audio, one left-padded batch
    negs = guidance_negative_messages(msgs, model.audio_locator)
    _, in_c, _, _ = model._chat_inputs(msgs)
    _, in_n, _, _ = model._chat_inputs(negs)
    Sc, Sn = in_c["context_input_ids"].shape[1], in_n["context_input_ids"].shape[1]
    S = max(Sc, Sn)
    hand = {"context_input_ids": torch.cat([_left_pad(in_c["context_input_ids"], S, tok.pad_token_id), _left_pad(in_n["context_input_ids"], S, tok.pad_token_id)]),
            "context_attention_mask": torch.cat([_left_pad(in_c["context_attention_mask"], S, 0), _left_pad(in_n["context_attention_mask"], S, 0)]),
            "context_batch_start_positions": [(r, int(p) + S - Sc) for r, p in in_c["context_batch_start_positions"]],
            "batch_features": in_c["batch_features"], "batch_transcription_ids": in_c["batch_transcription_ids"]}
    ids = model._generate_step(hand, pad_token_id=tok.pad_token_id, do_sample=False, max_new_tokens=6, guidance_scale=2.0)
    assert ids.cpu().tolist() == out.generated_ids
    plain = model.generate(msgs, do_sample=False, max_new_tokens=6)
    assert plain.generated_ids != out.generated_ids                                 # the guidance is not a no-op on this chat
    # explicit negatives equal to the derived ones: the same ids
    out2 = model.generate(msgs, do_sample=False, max_new_tokens=6, guidance_scale=2.0, negative_messages=negs)
    assert out2.generated_ids == out.generated_ids and out2.audios == out.audios
    with pytest.raises(ValueError, match="1 conversations for 2"):
        model.generate(msgs, do_sample=False, max_new_tokens=6, guidance_scale=2.0, negative_messages=negs[:1])


def test_chat_text_only_with_explicit_negatives(golden_dir, tmp_path):
    s, tok, _ = _chat_model(golden_dir, tmp_path)
    model = s.model
    msgs = [[{"role": "user", "content": "hi there"}], [{"role": "user", "content": "a somewhat longer question , please"}]]
    negs = [[{"role": "user", "content": "hello"}], [{"role": "user", "content": "a question"}]]
    with pytest.raises(ValueError, match="no audio"):
        model.generate(msgs, do_sample=False, max_new_tokens=6, guidance_scale=2.0)
    first = model.generate(msgs, do_sample=False, max_new_tokens=6, guidance_scale=2.0, negative_messages=negs, repetition_penalty=1.2)
    assert len(first.generated_ids) == 2 and first.audios == [] and all(2 <= len(r) <= 6 for r in first.generated_ids)
    tok._fixed["<|eot_id|>"] = first.generated_ids[0][1]                            # row 0's second token ends a turn from now on
    eos = {tok.eos_token_id, first.generated_ids[0][1]}
    out = model.generate(msgs, do_sample=False, max_new_tokens=6, guidance_scale=2.0, negative_messages=negs, repetition_penalty=1.2)
    ends = [next((i + 1 for i, t in enumerate(r) if t in eos), len(r)) for r in first.generated_ids]
    assert ends[0] <= 2 and len(out.generated_ids) == 2
    for b, e in enumerate(ends):
        assert out.generated_ids[b][:e] == first.generated_ids[b][:e]
        assert all(t == tok.pad_token_id for t in out.generated_ids[b][e:])         # stopped on the EOS list: padding behind it
