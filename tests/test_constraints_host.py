"""Host side of the hard constraints of generate() (`desta_logit_constraints_bf16`): the restatement of tests/constraints_reference.py
against the installed transformers' five processors and against `generate(output_scores=True)` of a tiny local Llama (the order
of the chain), the argument checks, the host tables, the resolver's opt-in, the speculation fallback, the kernel's resources
and the ABI."""
import importlib.util
import os
import re

import pytest
import torch

import constraints_reference as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 50
EOS = [7, 9]


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------ the restatement is HF's
def _hf_mask(history, prompt_len, s):
    """isinf mask after HF's processors, in `_get_logits_processor`'s order, on a finite row."""
    from transformers.generation.logits_process import (LogitsProcessorList, MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor, SuppressTokensAtBeginLogitsProcessor,
                                                        SuppressTokensLogitsProcessor)
    procs = LogitsProcessorList()
    if s.get("no_repeat_ngram_size"):
        procs.append(NoRepeatNGramLogitsProcessor(s["no_repeat_ngram_size"]))
    if s.get("bad_words_ids"):
        procs.append(NoBadWordsLogitsProcessor(s["bad_words_ids"], torch.tensor(EOS)))
    if s.get("min_new_tokens"):
        procs.append(MinNewTokensLengthLogitsProcessor(prompt_len, s["min_new_tokens"], torch.tensor(EOS)))
    if s.get("suppress_tokens"):
        procs.append(SuppressTokensLogitsProcessor(s["suppress_tokens"]))
    if s.get("begin_suppress_tokens"):
        procs.append(SuppressTokensAtBeginLogitsProcessor(s["begin_suppress_tokens"], prompt_len))
    ids = torch.tensor([history], dtype=torch.long).view(1, len(history))
    scores = torch.linspace(-3.0, 3.0, V).view(1, V).clone()
    return torch.isinf(procs(ids, scores))[0].numpy()


def _bad_words(h):
    """Words of 1..4 tokens for the history h (length L): two sharing a last token, one longer than h, one of length exactly L
    and one of length L + 1 (both built to match, so only HF's length rule keeps the latter from firing), an [eos] word."""
    L = len(h)
    words = [[3], [EOS[0]], [11, 12], [13, 12], [1, 2, 3, 4], [5, 6, 7, 8]]
    if L >= 1:
        words.append([h[-1], 20])                                                   # a live two-token word (fires when L >= 2)
    if 2 <= L <= 4:
        words.append(h[1:] + [21])                                                  # length exactly L: matches and fires
    if 1 <= L <= 3:
        words.append(h + [22])                                                      # length L + 1: matches, HF skips it
    if L >= 3:
        words += [h[-2:] + [23], [h[-1], 23]]                                       # two live words sharing their last token
    return words


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_restatement_is_hfs_processors(n):
    gen = torch.Generator().manual_seed(100 + n)
    fired = dict(ngram=0, quirk=0, word=0)
    for L in sorted({0, 1, max(n - 2, 0), n - 1, n, 40}):
        for rep in range(4):
            h = torch.randint(0, 3 if L > 8 else V, (L,), generator=gen).tolist()  # long histories over 3 tokens: repeats are the rule
            words = _bad_words(h)
            for prompt_len in sorted({L, max(L - 2, 0)}):
                t = L - prompt_len
                sets = [dict(no_repeat_ngram_size=n), dict(bad_words_ids=words), dict(suppress_tokens=[4, EOS[1], 49]),
                        dict(begin_suppress_tokens=[0, 5]), dict(min_new_tokens=2)]
                sets.append({k: v for s in sets for k, v in s.items()})
                for s in sets:
                    want = _hf_mask(h, prompt_len, s)
                    got = CR.banned_mask(h, t, V, eos_token_ids=EOS, **s)
                    assert (got == want).all(), (L, t, s, h, sorted(got.nonzero()[0]), sorted(want.nonzero()[0]))
                fired["ngram"] += int(CR.banned_mask(h, t, V, no_repeat_ngram_size=n).sum())
                fired["word"] += int(20 in CR.banned(h, t, V, bad_words_ids=words))
                fired["quirk"] += int(1 <= L <= 3 and 22 not in CR.banned(h, t, V, bad_words_ids=words))
    assert fired["ngram"] > 0 and fired["word"] > 0 and fired["quirk"] > 0, fired


def test_restatement_edge_rules():
    assert CR.banned([], 0, V, no_repeat_ngram_size=1) == set()
    assert CR.banned([4, 4, 8], 3, V, no_repeat_ngram_size=1) == {4, 8}
    assert CR.banned([1, 2, 1], 3, V, no_repeat_ngram_size=2) == {2}
    assert CR.banned([1], 1, V, no_repeat_ngram_size=3) == set()                   # L + 1 < n
    assert CR.banned([5], 1, V, bad_words_ids=[[5, 6]]) == set()                   # the quirk: m = 2 > L = 1
    assert CR.banned([0, 5], 2, V, bad_words_ids=[[5, 6]]) == {6}
    assert CR.banned([], 0, V, bad_words_ids=[[7], [8]], eos_token_ids=[7]) == {8}
    assert CR.banned([], 0, V, suppress_tokens=[7], eos_token_ids=[7]) == {7}      # EOS is not filtered out of suppress_tokens
    assert CR.banned([], 0, V, suppress_tokens=[V, 3]) == {3}                      # only ids below the vocab can be banned
    assert CR.banned([], 0, V, begin_suppress_tokens=[2]) == {2} and CR.banned([2], 1, V, begin_suppress_tokens=[2]) == set()
    assert CR.banned([1], 1, V, min_new_tokens=2, eos_token_ids=EOS) == set(EOS)
    assert CR.banned([1, 1], 2, V, min_new_tokens=2, eos_token_ids=EOS) == set() == CR.banned([], 0, V, min_new_tokens=2)
    assert CR.banned([-1, 60, -1], 3, V, no_repeat_ngram_size=2) == set()          # -1 matches -1, the 60 behind it is no column
    assert CR.banned([-1, 6, -1], 3, V, no_repeat_ngram_size=2) == {6}
    assert CR.grouped_history([1, 2], [2, 8, 9, -1], 2) == [1, 2, 8, 9] and CR.grouped_history([1, 2], None, 0) == [1, 2]


@pytest.mark.parametrize("penalty", [None, 1.3])
def test_chain_order_on_a_tiny_llama(penalty):
    """HF's own generate() on a local random Llama: the -inf of its processed scores sit exactly where the restatement bans, with
    HF's `input_ids` (prompt + emitted) as the history, with and without the repetition penalty in front."""
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(5)
    model = LlamaForCausalLM(LlamaConfig(vocab_size=V, hidden_size=16, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2,
                                         num_key_value_heads=2, max_position_embeddings=64)).eval()
    prompt = torch.tensor([[3, 11, 12, 3, 11], [8, 8, 13, 12, 8]])
    s = dict(no_repeat_ngram_size=2, bad_words_ids=[[11, 12], [EOS[0]], [30]], suppress_tokens=[4, 31], begin_suppress_tokens=[0, 32], min_new_tokens=3)
    kw = {} if penalty is None else {"repetition_penalty": penalty}
    with torch.no_grad():
        out = model.generate(prompt, attention_mask=torch.ones_like(prompt), max_new_tokens=10, do_sample=False, output_scores=True,
                             return_dict_in_generate=True, eos_token_id=EOS, pad_token_id=0, **s, **kw)
    seq, P = out.sequences, prompt.shape[1]
    total = by_ngram = 0
    for t, sc in enumerate(out.scores):
        for b in range(2):
            h = seq[b, :P + t].tolist()
            want = CR.banned_mask(h, t, V, eos_token_ids=EOS, **s)
            assert (torch.isinf(sc[b]).numpy() == want).all(), (t, b, h)
            total += int(want.sum())
            by_ngram += len(CR.banned(h, t, V, no_repeat_ngram_size=2))
    assert total > 0 and by_ngram > 0
    for b in range(2):
        assert CR.violations(seq[b, P:].tolist(), V, prompt=prompt[b].tolist(), eos_token_ids=EOS, **s) == []


# ------------------------------------------------------------------------------------------------ arguments, tables, resolver
def test_check_constraint_args():
    from desta.models.modeling_desta25 import check_constraint_args as chk
    chk()
    chk(3, [[1, 2], [3]], [4], [5], 0, vocab=10)
    chk(no_repeat_ngram_size=1, min_new_tokens=7, suppress_tokens=(1, 2))
    for bad in (0, -1, 2.0, True, "3", [3]):
        with pytest.raises(ValueError, match="ngram_size"):
            chk(no_repeat_ngram_size=bad)
    for bad in ([], [1, 2], "x", ((1,),), [[1], []], [[1], (2,)], [[-1]], [[1.0]], [[True]]):
        with pytest.raises(ValueError, match="bad_words_ids"):
            chk(bad_words_ids=bad)
    for name in ("suppress_tokens", "begin_suppress_tokens"):
        for bad in (3, "3", [-1], [1.5], [[1]], [True]):
            with pytest.raises(ValueError, match=name):
                chk(**{name: bad})
    for bad in (-1, 1.0, True, "2", [2]):
        with pytest.raises(ValueError, match="min_new_tokens"):
            chk(min_new_tokens=bad)
    for kw in (dict(bad_words_ids=[[1, 10]]), dict(suppress_tokens=[10]), dict(begin_suppress_tokens=[3, 11])):
        chk(**kw)                                                                    # vocabulary unknown: nothing to hold the id against
        with pytest.raises(ValueError, match="vocabulary has 10 tokens"):
            chk(**kw, vocab=10)
    chk(bad_words_ids=[[1, 2]], suppress_tokens=list(range(65535)))                  # the caps of the device table: 65 536 words in all
    with pytest.raises(ValueError, match="together hold more than 65536 words"):
        chk(bad_words_ids=[[1, 2]], suppress_tokens=list(range(65536)))


def test_generate_refuses_before_any_work():
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                                 # no device state: the checks come first
    model.llm = CausalLMHIP.__new__(CausalLMHIP)
    model.llm.V = 64
    for kw in (dict(no_repeat_ngram_size=0), dict(bad_words_ids=[]), dict(suppress_tokens=[64]), dict(min_new_tokens=-2), dict(begin_suppress_tokens=7)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            model.generate([{"role": "user", "content": "hi"}], do_sample=False, **kw)
        with pytest.raises(ValueError, match=next(iter(kw))):
            model._generate_step({}, pad_token_id=0, **kw)


def test_constraint_tables_fold_and_drop():
    from desta.models.modeling_desta25 import constraint_tables
    t = constraint_tables([7, 9], 3, [[1, 2, 3], [7], [9], [4], [7, 9]], [9, 5], [0], 2)
    assert t == dict(no_repeat_ngram=3, word_ids=[1, 2, 3, 4, 7, 9, 9, 5], word_off=[0, 3, 4, 6, 7, 8], n_words=5, begin_ids=[0], eos_ids=[7, 9],
                     min_new_tokens=2)
    off = constraint_tables(None, None, None, None, None, 4)                             # min_new_tokens without an EOS: off
    assert off == dict(no_repeat_ngram=0, word_ids=[], word_off=[0], n_words=0, begin_ids=[], eos_ids=[], min_new_tokens=0)
    assert constraint_tables([7], bad_words_ids=[[7]])["n_words"] == 0                   # nothing left once the [eos] word is gone


def test_resolver_opt_in():
    from desta.models.modeling_desta25 import resolve_generation_kwargs as res
    file_cfg = {"no_repeat_ngram_size": 3, "suppress_tokens": [5], "top_k": 20, "begin_suppress_tokens": [], "min_new_tokens": 0}
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size=3"):             # the default contract stands
        res(file_cfg)
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size=3"):
        res({}, no_repeat_ngram_size=3)
    got = res(file_cfg, constraints=True, bad_words_ids=[[1, 2]], max_new_tokens=9)
    assert got == dict(do_sample=False, temperature=1.0, top_k=20, top_p=1.0, min_p=None, repetition_penalty=1.0, max_new_tokens=9,
                       no_repeat_ngram_size=3, bad_words_ids=[[1, 2]], suppress_tokens=[5], begin_suppress_tokens=None, min_new_tokens=None)
    assert res(file_cfg, constraints=True, no_repeat_ngram_size=2)["no_repeat_ngram_size"] == 2          # explicit > file
    assert all(res({}, constraints=True)[k] is None for k in CR.KEYS)                    # nothing set: all off
    for kw in (dict(num_beams=4), dict(typical_p=0.5), dict(epsilon_cutoff=1e-3), dict(top_h=0.4)):
        with pytest.raises(NotImplementedError, match=next(iter(kw))):
            res(file_cfg, constraints=True, **kw)
    with pytest.raises(NotImplementedError, match="num_beams"):
        res({"num_beams": 2}, constraints=True)
    assert "no_repeat_ngram_size" not in res({}, top_k=5)                                # the default output carries none of the keys


def test_spec_reason_for_a_constrained_call():
    from desta.models.modeling_desta25 import CausalLMHIP
    llm = CausalLMHIP.__new__(CausalLMHIP)
    llm.speculative = llm._spec = None
    llm.spec_scope, llm.kv_cache_kind = "greedy", "bf16"
    llm.set_speculative(3)
    assert llm._spec_reason(3, 2, False, False, None, None, None, constrained=True) == "logit_constraints"
    assert llm._spec_reason(3, 2, True, False, None, None, None, constrained=True) == "do_sample"
    assert llm._spec_reason(3, 2, False, False, None, None, None) is None                # the old positional form
    assert llm._spec_reason(3, 2, False, False, None, None, None, guided=True, constrained=True) == "guidance_scale"
    llm.set_speculative(3, scope="all")
    assert llm._spec_reason(3, 2, True, True, 2, None, None, constrained=True) is None


# ------------------------------------------------------------------------------------------------ kernel and ABI
def test_kernel_uses_no_scratch():
    res = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources()
    hits = {n: r for n, r in res.items() if "logit_constraints_k" in n}
    assert len(hits) == 1, sorted(hits)
    (name, r), = hits.items()
    assert r["scratch"] == 0 and r["spill"] == 0, (name, r)


def test_abi_declares_and_binds_the_symbol():
    from desta import _hip
    hdr = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    assert re.search(r"#define DESTA_ABI_VERSION 8\b", hdr) and _hip.ABI_VERSION == 8 and _hip.lib.desta_abi_version() == 8
    m = re.search(r"int desta_logit_constraints_bf16\(([^;]*)\);", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)) == (
        "const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int batch, int width, int cols, const int64_t* hist, int64_t hist_ld, "
        "int hist_len, const int64_t* tail, int64_t tail_ld, uint32_t step0, int no_repeat_ngram, const int32_t* word_ids, "
        "const int32_t* word_off, int n_words, int n_word_ids, const int32_t* begin_ids, int n_begin, const int32_t* eos_ids, int n_eos, "
        "int min_new_tokens, int id_max, void* stream")
    for name in ("NoRepeatNGramLogitsProcessor", "NoBadWordsLogitsProcessor", "SuppressTokensLogitsProcessor", "SuppressTokensAtBeginLogitsProcessor",
                 "MinNewTokensLengthLogitsProcessor", "modeling_desta25.py:1419 / :1703"):
        assert name in hdr, name
    h = _hip
    assert h._logit_constraints.argtypes == [h.vp, h.i64, h.vp, h.i64, h.i32, h.i32, h.i32, h.vp, h.i64, h.i32, h.vp, h.i64, h.C.c_uint32, h.i32,
                                             h.vp, h.vp, h.i32, h.i32, h.vp, h.i32, h.vp, h.i32, h.i32, h.i32, h.vp]
    assert callable(h.logit_constraints) and isinstance(h.CONSTRAINT_CALLS, int)
