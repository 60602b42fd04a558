"""CPU: the host side of draft-and-verify decoding for sampled and penalised calls (`set_speculative(k, scope="all")`) — the
reference loop with a position-dependent pick (tests/spec_sampling_reference.py) against the token-by-token loop on a toy model,
the row rule of the grouped samplers on a hand case, the two C entry points in the header and the library at an unchanged ABI
version, the binding, the `scope` argument of the model and the entry point's `trainer.speculative_scope` key."""
import importlib.util
import math
import os
import random
import re

import numpy as np
import pytest
import torch

import sampling_reference as S
import spec_sampling_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS, PAD, VOCAB = 5, 0, 13


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _toy_logits(model_seed, h):
    """A deterministic toy model: bf16 logits [VOCAB] as a seeded function of the last three tokens and the history's length."""
    x = model_seed
    for t in h[-3:]:
        x = (x * 1000003 + t + 2) % 2147483647
    x = (x * 31 + len(h)) % 2147483647
    g = np.random.default_rng(x)
    return torch.from_numpy((g.standard_normal(VOCAB) * 2.0).astype(np.float32)).to(torch.bfloat16)


def _pick(logits, pen_hist, penalty, T, top_k, top_p, u):
    """sampling_reference's contract on one row: scores (penalty, temperature) -> kept -> the index-order inverse CDF at u / 2^24."""
    hist = torch.tensor([pen_hist], dtype=torch.int64) if pen_hist else None
    _, t = S.scores(logits.unsqueeze(0), hist, penalty, T)
    keep = S.kept(t, top_k, top_p)[0]
    t64 = t[0].astype(np.float64)
    p = np.where(keep, np.exp(t64 - t64[keep].max()), 0.0)
    C = np.cumsum(p / p.sum())
    return int(min(np.searchsorted(C, u / 2.0 ** 24, side="right"), VOCAB - 1))


def _next_token(model_seed, rng_seed, penalty, S_prompt):
    """next_token(history, b, t): the draw u24(seed, t, b) from the toy logits of the history, penalised with the EMITTED part of
    the history (an inputs_embeds prompt: HF's input_ids hold the generated tokens only).  Never PAD: token 0 is masked."""
    memo = {}

    def f(h, b, t):
        key = (tuple(h), b, t)
        if key not in memo:
            logits = _toy_logits(model_seed, [max(x, 0) for x in h]).clone()
            logits[PAD] = float("-inf")
            memo[key] = _pick(logits, list(h[S_prompt:]), penalty, 0.8, 6, 0.9, S.u24(rng_seed, t, b))
        return memo[key]
    return f


@pytest.mark.parametrize("penalty", [1.0, 1.3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("source", ["perfect", "none", "corrupt", "random", "lookup"])
def test_reference_loop_equals_the_token_by_token_loop(source, k, B, penalty):
    T, Sp = 16, 7
    for seed in range(3):
        rng = random.Random(seed * 100 + k * 10 + B)
        nt = _next_token(seed, S.SEEDS[seed % 2], penalty, Sp)
        prompts = [[rng.randrange(1, VOCAB) for _ in range(Sp)] for _ in range(B)]
        eos = [EOS] if seed == 1 else []
        want = R.plain_loop(nt, prompts, T, eos, PAD)

        def drafts(b, n, hist):
            if source in ("perfect", "corrupt"):
                d = (want[b] + [-1] * k)[n:n + k]
                if source == "corrupt" and n <= 3 + 4 * b < n + k:           # one position per row
                    d[3 + 4 * b - n] = 1 + d[3 + 4 * b - n] % (VOCAB - 1)
                return d
            if source == "random":
                return [rng.randrange(-1, VOCAB) for _ in range(k)]
            if source == "lookup":
                return R.ngram_draft(hist, len(hist), 0, k, 3, 1)
            return [-1] * k
        got, steps = R.speculative_loop(nt, prompts, T, k, drafts, eos, PAD)
        assert got == want, (source, k, B, seed)
        if not eos and source == "perfect":
            assert steps == math.ceil((T - 1) / (k + 1))
        if not eos and source == "none":
            assert steps == T - 1
        if not eos:
            assert len({tuple(r) for r in want}) == B and all(len(set(r)) > 3 for r in want)     # a real draw per row


def test_reference_loop_finishes_a_row_inside_an_accepted_run():
    """Row 0 draws its EOS at emitted position 2, inside a fully accepted chunk of perfect drafts; row 1 goes on.  The pick depends
    on (b, t) alone here, so a wrong position or row shows at once."""
    script = {0: [3, 4, EOS, 7, 7, 7, 7, 7], 1: [6, 7, 8, 9, 10, 11, 12, 6]}
    prompts = [[1, 2], [1, 2]]

    def nt(h, b, t):
        assert len(h) == 2 + t                                               # the history of position t holds t emitted tokens
        return script[b][t % 8]                                              # (a chunk's last rows lie past T: picked, never emitted)
    want = R.plain_loop(nt, prompts, 8, [EOS], PAD)
    assert want[0] == [3, 4, EOS] + [PAD] * 5 and want[1] == script[1]
    got, steps = R.speculative_loop(nt, prompts, 8, 3, lambda b, n, hist: (want[b] + [-1] * 3)[n:n + 3], [EOS], PAD)
    assert got == want and steps == 2                                       # 1 + 4 + 3: the finished row limits nobody


def test_row_rule_on_a_hand_case():
    """hist ++ drafts[:j] and the counter (t0 + j, b).  The two mutations a grouped kernel can make — the flat row index r in the
    counter, step0 for every row — change a pick, and so does a history without the drafts in front of the row."""
    hist, tail = [4, 9, 4], [4, 7, -1, 20, 7]                                # column 0 repeats hist[-1]; a -1 and an id >= cols; 7 twice
    assert R.row_history(hist, tail, 0) == [4, 9, 4] and R.row_history(hist, tail, 3) == [4, 9, 4, 7, -1, 20]
    assert R.penalised_ids(hist, tail, 0, VOCAB) == [4, 9] and R.penalised_ids(hist, tail, 4, VOCAB) == [4, 7, 9]
    assert R.row_counter(5, 2, 1) == (7, 1) and R.row_counter(2 ** 32 - 2, 3, 0) == (1, 0)          # the uint32 sum wraps
    batch, width, step0, seed = 2, 4, 2 ** 32 - 2, S.SEEDS[1]
    flat = np.ones(VOCAB, dtype=bool)                                        # a flat row: the pick is kept index (u24 K) >> 24
    right = [[S.flat_pick("chain", flat, S.u24(seed, *R.row_counter(step0, j, b))) for j in range(width)] for b in range(batch)]
    by_r = [[S.flat_pick("chain", flat, S.u24(seed, (step0 + j) & R.M32, b * width + j)) for j in range(width)] for b in range(batch)]
    by_step0 = [[S.flat_pick("chain", flat, S.u24(seed, step0, b)) for j in range(width)] for b in range(batch)]
    no_wrap = [[S.flat_pick("chain", flat, S.u24(seed, step0 + j, b)) for j in range(width)] for b in range(batch)]
    assert right != by_r and right != by_step0
    assert right[0][0] == by_r[0][0] == by_step0[0][0]                       # row (0, 0) is where all three agree
    assert right == no_wrap                                                  # S.rng32 masks the step: a Python int past 2^32 wraps too
    # the penalty: token 7 leads unpenalised; with the draft 7 in front of row 2 it is divided by 1.5 and 3 takes over
    logits = torch.full((VOCAB,), -4.0).to(torch.bfloat16)
    logits[7], logits[3] = 3.0, 2.5
    greedy = [int(np.argmax(S.scores(logits.unsqueeze(0), torch.tensor([R.row_history(hist, tail, j)]), 1.5, 1.0)[0][0])) for j in range(4)]
    assert greedy == [7, 3, 3, 3]
    assert int(np.argmax(S.scores(logits.unsqueeze(0), torch.tensor([hist]), 1.5, 1.0)[0][0])) == 7     # ... and without the drafts: the wrong pick


def test_header_declares_and_library_exports_the_grouped_samplers_at_abi_8():
    from desta import _hip
    txt = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+desta_sample_rows_bf16\s*\(\s*const void\*\s*logits,\s*int64_t ld,\s*int batch,\s*int width,\s*int cols,\s*"
                     r"const int64_t\*\s*hist,\s*int64_t hist_ld,\s*int hist_len,\s*const int64_t\*\s*tail,\s*int64_t tail_ld,\s*"
                     r"float repetition_penalty,\s*int do_sample,\s*float temperature,\s*int top_k,\s*float top_p,\s*float min_p,\s*"
                     r"uint64_t seed,\s*uint32_t step0,\s*int64_t\*\s*out,\s*uint8_t\*\s*keep_mask,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"int\s+desta_sample_top_p_rows_bf16\s*\(\s*const void\*\s*logits,\s*int64_t ld,\s*int batch,\s*int width,\s*int cols,\s*"
                     r"float temperature,\s*float top_p,\s*uint64_t seed,\s*uint32_t step0,\s*int64_t\*\s*out,\s*uint8_t\*\s*keep_mask,\s*"
                     r"void\*\s*stream\s*\)", code)
    # the one-row entry points keep their signatures
    assert re.search(r"int\s+desta_sample_bf16\s*\(\s*const void\*\s*logits,\s*int64_t ld,\s*int rows,\s*int cols,\s*const int64_t\*\s*hist,\s*"
                     r"int64_t hist_ld,\s*int hist_len,\s*float repetition_penalty,\s*int do_sample,\s*float temperature,\s*int top_k,\s*"
                     r"float top_p,\s*float min_p,\s*uint64_t seed,\s*uint32_t step,\s*int64_t\*\s*out,\s*uint8_t\*\s*keep_mask,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"int\s+desta_sample_top_p_bf16\s*\(\s*const void\*\s*logits,\s*int64_t ld,\s*int rows,\s*int cols,\s*float temperature,\s*"
                     r"float top_p,\s*uint64_t seed,\s*uint32_t step,\s*int64_t\*\s*out,\s*uint8_t\*\s*keep_mask,\s*void\*\s*stream\s*\)", code)
    assert int(re.search(r"#define DESTA_ABI_VERSION (\d+)", txt).group(1)) == 8 == _hip.ABI_VERSION == _hip.lib.desta_abi_version()
    assert hasattr(_hip.lib, "desta_sample_rows_bf16") and hasattr(_hip.lib, "desta_sample_top_p_rows_bf16")
    doc = txt[txt.index("The two samplers over the rows of a verify step"):txt.index("int desta_sample_rows_bf16")]
    assert "modeling_desta25.py:1419" in doc and "step0 + j" in doc and "counter row is b" in doc


def test_binding_has_the_grouped_callables_and_counters():
    from desta import _hip
    assert callable(_hip.sample_rows) and callable(_hip.sample_top_p_rows)
    assert isinstance(_hip.SAMPLE_ROWS_CALLS, int) and isinstance(_hip.SAMPLE_TOP_P_ROWS_CALLS, int)


def test_sampler_kernels_are_one_body_each_and_use_no_scratch():
    res = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources()
    for kernel in ("sample_greedy_k", "sample_chain_k", "sample_top_p_k"):
        hits = {n: r for n, r in res.items() if kernel in n}
        assert len(hits) == 1, (kernel, sorted(hits))                       # the grouped entry point launches the same kernel: no twin
        (name, r), = hits.items()
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)


def _bare_model():
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                    # no device state: the checks come first
    llm = model.llm = CausalLMHIP.__new__(CausalLMHIP)
    llm.speculative = llm._spec = None
    llm.spec_scope = "greedy"
    llm.kv_cache_kind = "bf16"
    return model, llm


def test_scope_argument():
    from desta.models.modeling_desta25 import SPECULATIVE_SCOPES, check_speculative_scope
    assert SPECULATIVE_SCOPES == ("greedy", "all")
    for ok in SPECULATIVE_SCOPES:
        check_speculative_scope(ok)
    model, llm = _bare_model()
    model.set_speculative(3, scope="all")
    assert (llm.speculative, llm.spec_scope) == (3, "all")
    for bad in ("sampling", "ALL", "", None, 1, True, ["all"]):
        with pytest.raises(ValueError, match="speculative"):
            check_speculative_scope(bad)
        for target in (model, llm):
            with pytest.raises(ValueError, match="speculative"):
                target.set_speculative(5, scope=bad)
            with pytest.raises(ValueError, match="speculative"):
                target.set_speculative(9, scope="greedy")                    # a bad k with a good scope
            assert (llm.speculative, llm.spec_scope) == (3, "all")           # the setting is untouched
    llm._spec = marker = dict(key=(3, 3))
    llm.set_speculative(3, scope="greedy")                                   # only the scope changes: the verify buffers stay
    assert llm._spec is marker and llm.spec_scope == "greedy"
    llm.set_speculative(3, "all")
    assert llm._spec is marker and llm.spec_scope == "all"
    llm.set_speculative(7, "all")                                            # k changes: they go
    assert llm._spec is None
    model.set_speculative(3)                                                 # the default scope is "greedy"
    assert (llm.speculative, llm.spec_scope) == (3, "greedy")


def test_default_scope_keeps_the_fallback_reasons():
    from desta import _hip
    model, llm = _bare_model()
    calls = dict(do_sample=(True, False, None, None, None), repetition_penalty=(False, True, None, None, None), logprobs=(False, False, 2, None, None),
                 forced_tokens=(False, False, None, object(), None), layer_hook=(False, False, None, None, object()))
    llm.set_speculative(3)
    for reason, a in calls.items():
        assert llm._spec_reason(3, 3, *a) == reason
    assert llm._spec_reason(3, 3, True, True, 2, None, None) == "do_sample"                  # today's order
    assert llm._spec_reason(3, 3, False, False, None, None, None) is None
    llm.set_speculative(3, scope="all")
    for reason, a in calls.items():
        assert llm._spec_reason(3, 3, *a) == (reason if reason in ("forced_tokens", "layer_hook") else None)
    assert llm._spec_reason(3, 3, True, True, 2, None, None) is None
    assert llm._spec_reason(3, 17, True, False, None, None, None) == f"B * (k + 1) = 68 rows > {_hip.DECODE_MAX_ROWS}"
    llm.kv_cache_kind = "fp8"
    assert llm._spec_reason(3, 3, True, False, None, None, None) == "fp8 kv cache"


def _yaml_with(tmp_path, *lines):
    """A copy of the debug config directory whose trainer section carries `lines`."""
    import shutil
    src = os.path.join(ROOT, "examples", "train", "config")
    dst = tmp_path / "config"
    shutil.copytree(src, dst)
    for name in os.listdir(src):
        if name.endswith(".yaml"):
            assert "speculative_scope" not in open(os.path.join(src, name)).read(), name      # the shipped YAMLs do not carry the key
    txt = open(dst / "desta25_debug.yaml").read()
    assert re.search(r"^trainer:\s*$", txt, flags=re.M)
    if lines:
        txt = re.sub(r"^trainer:\s*$", "trainer:\n  " + "\n  ".join(lines), txt, count=1, flags=re.M)
    open(dst / "desta25_debug.yaml", "w").write(txt)
    return str(dst)


@pytest.mark.parametrize("lines,want", [((), (None, "greedy")), (("speculative: 3",), (3, "greedy")),
                                        (("speculative: 3", "speculative_scope: all"), (3, "all")),
                                        (("speculative: 7", "speculative_scope: greedy"), (7, "greedy")), (("speculative_scope: all",), (None, "all"))])
def test_speculative_scope_key_parses(tmp_path, lines, want):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, *lines))
    assert (m.speculative(cfg), m.speculative_scope(cfg)) == want
    assert m.kv_cache_kind(cfg) == "bf16" and cfg.trainer.max_epochs is not None             # the rest of the trainer section is intact


@pytest.mark.parametrize("value", ["sampling", "3", "true", "null"])
def test_bad_speculative_scope_raises_before_create_model(tmp_path, monkeypatch, value):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"],
                        config_dir=_yaml_with(tmp_path, "speculative: 3", f"speculative_scope: {value}"))
    with pytest.raises(ValueError, match="speculative_scope"):
        m.speculative_scope(cfg)
    monkeypatch.setattr(m, "create_model", lambda *a, **k: pytest.fail("create_model reached with a bad trainer.speculative_scope"))
    monkeypatch.setattr(m, "load_config", lambda argv, config_dir=None: cfg)
    with pytest.raises(ValueError, match="speculative_scope"):
        m.main([])


def test_main_hands_the_scope_to_the_model(tmp_path, monkeypatch):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"],
                        config_dir=_yaml_with(tmp_path, "speculative: 3", "speculative_scope: all"))
    seen = {}

    class Stop(Exception):
        pass

    class Model:
        def set_decode_weights(self, kind): pass
        def set_kv_cache(self, kind): pass
        def set_prefill_chunk(self, n): pass

        def set_speculative(self, k, scope="greedy"):
            seen.update(k=k, scope=scope)
            raise Stop
    monkeypatch.setattr(m, "create_model", lambda *a, **k: Model())
    monkeypatch.setattr(m, "load_config", lambda argv, config_dir=None: cfg)
    with pytest.raises(Stop):
        m.main([])
    assert seen == dict(k=3, scope="all")
