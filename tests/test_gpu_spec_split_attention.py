"""GPU: draft-and-verify decoding with the verify step on the split-KV verify kernels (`set_speculative(k, attention="split")`).

Tiny Qwen3 geometry with head_dim 128 (G = 2 and G = 4), B = 3 with left pads [0, 5, 11], k = 3 (R = 8 and 16 query rows per KV head).
bf16 cache: a prompt of 490 tokens, so that every verify step sits past H.DECODE_ATTN_MIN_KEYS and decoding crosses key 512 (a
chunk boundary): tokens and per-step logits equal the plain loop's with torch.equal for perfect, absent and corrupted drafts, every
verify step attends through `H.attention_verify` once per layer, and a short prompt stays on the forward kernel.  FP8 cache:
speculation no longer falls back; tokens, logits, TokenLogprobs and the cache bytes and scales equal the FP8-cache plain loop's, at
S = 61 and at S = 250 (decoding crosses key 256).  G = 7 (tiny Qwen2-like, q|k|v bias) at k = 3 has 28 query rows per KV head and
runs the plain loop with the reason that says so.  With the default attention everything is as it was."""
import pytest
import torch

from test_gpu_kv8_cache import _text_inputs
from test_gpu_prefill_chunk import _model, _slabs

pytestmark = pytest.mark.gpu

PADS = [0, 5, 11]
K = 3
W = K + 1
ATTENTION = ("attention_fwd", "attention_decode", "attention_decode_kv8", "attention_verify", "attention_verify_kv8")


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _gen(model, inputs, T, drafts=None, **kw):
    a = dict(pad_token_id=0, max_new_tokens=T, do_sample=False, collect_logits=True, eos_token_id=[], draft_tokens=drafts)
    a.update(kw)
    res = model._generate_step(inputs, **a)
    return [r.clone() if torch.is_tensor(r) else [t.clone() for t in (r.token_logprobs, r.top_ids, r.top_logprobs)] for r in res]


def _attention_launches(hip, monkeypatch, run):
    """-> (run's result, [(name, batch, seq_q, seq_k, causal)] of every attention launch, in order)"""
    log = []

    def wrap(name):
        real = getattr(hip, name)

        def f(d, *a, **kw):
            log.append((name, d.batch, d.seq_q, d.seq_k, d.causal))
            return real(d, *a, **kw)
        return f
    with monkeypatch.context() as m:
        for name in ATTENTION:
            m.setattr(hip, name, wrap(name))
        res = run()
        torch.cuda.synchronize()
    return res, log


def _corrupt(ids, vocab):
    bad = ids.clone()
    for b in range(ids.shape[0]):
        bad[b, 3 + 5 * b] = (bad[b, 3 + 5 * b] + 1) % vocab                   # a different position per row
    return bad


def test_the_opt_in_exists(hip):
    """Fails on the parent commit: `attention` is no argument of `set_speculative` and the binding has no verify attention."""
    d, w, model = _model(False)
    assert callable(hip.attention_verify) and callable(hip.attention_verify_kv8) and hip.VERIFY_ATTN_MAX_ROWS == 16
    try:
        model.set_speculative(3, attention="split")
        assert (model.llm.speculative, model.llm.spec_scope, model.llm.spec_attention) == (3, "greedy", "split")
        with pytest.raises(ValueError, match="speculative attention"):
            model.set_speculative(3, attention="splitkv")
        assert model.llm.spec_attention == "split"
    finally:
        model.set_speculative(None)
    assert model.llm.spec_attention == "forward"


@pytest.mark.parametrize("g4", [False, True])
def test_bf16_cache_split_equals_the_plain_loop(hip, monkeypatch, g4):
    d, w, model = _model(g4)
    llm, L, CH, MIN = model.llm, d.llm_layers, hip.DECODE_ATTN_CHUNK, hip.DECODE_ATTN_MIN_KEYS
    S, T = 490, 40
    assert S + 1 >= MIN and S + W < 2 * CH < S + T                            # every verify step past the threshold; keys cross 512
    inputs = _text_inputs(d, S, PADS, seed=S + g4)[2]
    try:
        model.set_speculative(None)
        (ids_p, lg_p), plain_log = _attention_launches(hip, monkeypatch, lambda: _gen(model, inputs, T))
        assert [e for e in plain_log if e[2] == 1] == [("attention_decode", 3, 1, S + 1 + i, 0) for i in range(T - 1) for _ in range(L)]
        sources = {"perfect": ids_p, "none": torch.full_like(ids_p, -1), "corrupt": _corrupt(ids_p, d.vocab)}
        model.set_speculative(K, attention="split")
        steps = {}
        for name, drafts in sources.items():
            (ids, lg), log = _attention_launches(hip, monkeypatch, lambda: _gen(model, inputs, T, drafts))
            st = dict(llm.spec_stats)
            assert st["path"] == "speculative" and st["reason"] is None and st["emitted"] == T, (name, st)
            assert torch.equal(ids, ids_p), name
            assert torch.equal(lg, lg_p), name
            step_log = [e for e in log if e[2] != S]                         # everything behind the prompt pass
            assert len(step_log) == L * st["verify_steps"] and not any(e[0] == "attention_fwd" for e in step_log), name
            assert all(e[0] == "attention_verify" and e[1:3] == (3, W) and e[4] == 1 for e in step_log), name
            steps[name] = st["verify_steps"]
            if name != "corrupt":                                            # the emitted count per step is known: so is every step's cur
                curs = [S + i for i in range(T - 1)] if name == "none" else list(range(S, S + T - 1, W))
                assert step_log == [("attention_verify", 3, W, cur + W, 1) for cur in curs for _ in range(L)], name
        assert steps["perfect"] == -(-(T - 1) // W) and steps["none"] == T - 1 and steps["perfect"] < steps["corrupt"] < T - 1, steps
        assert llm._spec["attn_ws"] is not None and llm._spec["attn_ws"].numel() * 4 == hip.attention_verify_workspace_bytes(3, d.llm_hq, W, S + T + K, 128)
        # the opt-in off: the same long cache on the forward kernel, as before.  Its bits are not the plain loop's split-KV bits,
        # so neither the tokens nor the accepted runs are asserted here
        model.set_speculative(K)
        (ids, lg), log = _attention_launches(hip, monkeypatch, lambda: _gen(model, inputs, T, ids_p))
        step_log = [e for e in log if e[2] != S]
        assert llm.spec_stats["path"] == "speculative" and len(step_log) == L * llm.spec_stats["verify_steps"] > 0
        assert all(e[0] == "attention_fwd" and e[1:3] == (3, W) and e[4] == 1 for e in step_log)
        # below the threshold "split" keeps the forward kernel
        S2, T2 = 61, 12
        short = _text_inputs(d, S2, PADS, seed=S2 + g4)[2]
        model.set_speculative(None)
        ids_s, lg_s = _gen(model, short, T2)
        model.set_speculative(K, attention="split")
        (ids, lg), log = _attention_launches(hip, monkeypatch, lambda: _gen(model, short, T2, ids_s))
        assert llm.spec_stats["path"] == "speculative"
        assert [e for e in log if e[2] != S2] == [("attention_fwd", 3, W, cur + W, 1) for cur in range(S2, S2 + T2 - 1, W) for _ in range(L)]
        assert torch.equal(ids, ids_s) and torch.equal(lg, lg_s)
    finally:
        model.set_speculative(None)


@pytest.mark.parametrize("S", [61, 250])
@pytest.mark.parametrize("g4", [False, True])
def test_fp8_cache_speculates_and_equals_the_plain_loop(hip, monkeypatch, g4, S):
    d, w, model = _model(g4)
    llm, L, CH, T = model.llm, d.llm_layers, hip.DECODE_ATTN_CHUNK, 24
    assert S != 250 or S + 1 < CH < S + T                                     # decoding crosses key 256
    inputs = _text_inputs(d, S, PADS, seed=S + g4)[2]
    try:
        model.set_kv_cache("fp8")
        model.set_speculative(None)
        ids_p, lg_p = _gen(model, inputs, T)
        slabs_p = _slabs(llm, PADS, S + T - 1)
        assert llm.kv_cache[0].dtype == torch.uint8 and len(slabs_p) == 2 * 3 * L
        model.set_speculative(K)                                             # the default attention: today's fallback
        ids, lg = _gen(model, inputs, T, ids_p)
        assert llm.spec_stats["path"] == "plain" and llm.spec_stats["reason"] == "fp8 kv cache" and torch.equal(ids, ids_p) and torch.equal(lg, lg_p)
        model.set_speculative(K, attention="split")
        for name, drafts in (("perfect", ids_p), ("none", torch.full_like(ids_p, -1))):
            (ids, lg), log = _attention_launches(hip, monkeypatch, lambda: _gen(model, inputs, T, drafts))
            st = dict(llm.spec_stats)
            assert st["path"] == "speculative" and st["reason"] is None and st["verify_steps"] > 0 and st["emitted"] == T, (name, st)
            assert st["verify_steps"] == (-(-(T - 1) // W) if name == "perfect" else T - 1), (name, st)
            assert torch.equal(ids, ids_p), name
            assert torch.equal(lg, lg_p), name
            curs = list(range(S, S + T - 1, W)) if name == "perfect" else [S + i for i in range(T - 1)]
            assert [e for e in log if e[2] != S] == [("attention_verify_kv8", 3, W, cur + W, 1) for cur in curs for _ in range(L)], name
            slabs = _slabs(llm, PADS, S + T - 1)                             # bytes and scales of the slots the run trusts
            assert len(slabs) == len(slabs_p) and all(torch.equal(a, b) for a, b in zip(slabs, slabs_p)), name
        # scope "all": sampling at a fixed seed with logprobs = 2
        kw = dict(do_sample=True, temperature=0.8, top_p=0.9, seed=11, logprobs=2)
        model.set_speculative(None)
        ids_s, lg_s, lp_s = _gen(model, inputs, T, **kw)
        assert int((ids_s != lg_s.float().argmax(-1).t()).sum()) > 0         # a real draw
        model.set_speculative(K, scope="all", attention="split")
        for drafts in (ids_s, _corrupt(ids_s, d.vocab)):
            ids, lg, lp = _gen(model, inputs, T, drafts, **kw)
            assert llm.spec_stats["path"] == "speculative" and llm.spec_stats["verify_steps"] > 0
            assert torch.equal(ids, ids_s) and torch.equal(lg, lg_s) and all(torch.equal(a, b) for a, b in zip(lp, lp_s))
    finally:
        model.set_kv_cache("bf16")
        model.set_speculative(None)


def test_fp8_cache_with_too_many_query_rows_runs_the_plain_loop(hip, tmp_path_factory):
    """G = 7 (tiny Qwen2-like, q|k|v bias on) at k = 3: 28 query rows per KV head."""
    from test_gpu_qwen2_model import _inputs, _model as _qwen2, _text
    model = _qwen2(tmp_path_factory, "g7")
    ids, am = _text(3, 21, seed=4)[:2]
    run = lambda: _gen(model, _inputs(ids, am), 8)
    try:
        model.set_kv_cache("fp8")
        model.set_speculative(None)
        ids_p, lg_p = run()
        model.set_speculative(K, attention="split")
        n0 = hip.SPEC_ACCEPT_CALLS
        ids_k, lg_k = run()
        assert model.llm.spec_stats["path"] == "plain" and model.llm.spec_stats["reason"] == "fp8 kv cache: 7 x 4 = 28 query rows per KV head > 16"
        assert hip.SPEC_ACCEPT_CALLS == n0 and torch.equal(ids_k, ids_p) and torch.equal(lg_k, lg_p)
        model.set_speculative(1, attention="split")                          # 7 x 2 = 14 rows: speculates, the plain tokens
        ids_1, lg_1 = run()
        assert model.llm.spec_stats["path"] == "speculative" and model.llm.spec_stats["verify_steps"] > 0
        assert torch.equal(ids_1, ids_p) and torch.equal(lg_1, lg_p)
    finally:
        model.set_kv_cache("bf16")
        model.set_speculative(None)
