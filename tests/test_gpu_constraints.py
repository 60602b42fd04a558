"""GPU: the hard constraints of generate() — `desta_logit_constraints_bf16` against the restatement of
tests/constraints_reference.py (bit equality off the banned set, -inf on it), and the decode loops (plain, penalised, sampled,
guided, scored, draft-and-verify, chat level, trainer) replayed on the host from the logits they collected.  Every comparison
is exact: the pass moves no value other than to -inf."""
import copy
import types

import pytest
import torch

import constraints_reference as CR
import desta_oracle as O
import guidance_reference as GR
import sampling_reference as SR
from helpers import GENERATE_MESSAGES, ToyTokenizer, cfg_from_dims, golden_batch

pytestmark = pytest.mark.gpu

SENTINEL = 123.0                                                                    # exact in bf16
EOS = [0, 5]


# ------------------------------------------------------------------------------------------------ kernel
def _settings(which, n, words):
    s = dict(no_repeat_ngram_size=n, bad_words_ids=words, suppress_tokens=[1, 9], begin_suppress_tokens=[2, 7], min_new_tokens=3)
    return s if which == "all" else {which: s[which]}


_LAST = {}


def _case(cols, ld, offset, batch, width, hist_len, which="all", n=3, step0=0, seed=0):
    """One launch out of place and one in place on crafted rows, both against the restatement -> banned entries in all rows.
    Rows start `offset` elements into their allocation; columns >= cols of src are random, of dst SENTINEL; hist has 5 junk
    columns behind hist_len (the two highest ids, which no row's history holds) and tail a -1."""
    from desta import _hip as H
    from desta.models.modeling_desta25 import ConstraintPlan
    gen = torch.Generator().manual_seed(1000 * cols + 10 * hist_len + width + seed)
    R, A = batch * width, min(cols - 2, 4)                                          # histories over A tokens: n-grams repeat
    flat = (3.0 * torch.randn(offset + R * ld + 8, generator=gen)).to(torch.bfloat16).cuda()
    src = flat[offset:offset + R * ld].view(R, ld)
    before = flat.clone()
    ld_dst = ld + 8
    dflat = torch.full((offset + (R + 1) * ld_dst,), SENTINEL, dtype=torch.bfloat16, device="cuda")
    dst = dflat[offset:].view(R + 1, ld_dst)
    hist = torch.randint(0, A, (batch, hist_len + 5), generator=gen)
    hist[:, hist_len:] = torch.tensor([cols - 1, cols - 2, cols - 1, cols - 1, cols - 2])
    tail = torch.randint(0, A, (batch, width), generator=gen)
    if width > 2:
        tail[0, 2] = -1
    h1 = CR.grouped_history(hist[batch - 1, :hist_len], tail[batch - 1], width - 1)            # live words: they end the last row's history
    words = [[cols - 3], [EOS[0]], [1, 2, 3], [0, 1, 3]] + ([[h1[-1], 6 % cols], h1[-2:] + [8 % cols]] if len(h1) >= 2 and min(h1[-2:]) >= 0 else [])
    _LAST.update(hist=hist, tail=tail)
    s = _settings(which, n, words)
    plan = ConstraintPlan("cuda", EOS, **s)
    hd, td = hist.cuda(), tail.cuda()
    n0 = H.CONSTRAINT_CALLS
    plan.apply(src, ld, dst, ld_dst, batch, width, cols, hd if hist_len else None, hist_len, tail=td if width > 1 else None, step0=step0)
    assert H.CONSTRAINT_CALLS == n0 + 1
    assert torch.equal(flat.view(torch.int16), before.view(torch.int16))            # src and everything around it unchanged
    got = dst.cpu()
    assert bool((got[:R, cols:] == SENTINEL).all()) and bool((got[R] == SENTINEL).all()) and bool((dflat[:offset] == SENTINEL).all())
    sc, total = src.cpu(), 0
    for b in range(batch):
        for j in range(width):
            r = b * width + j
            mask = CR.banned_mask(CR.grouped_history(hist[b, :hist_len], tail[b], j), step0 + j, cols, eos_token_ids=EOS, **s)
            want = CR.apply(sc[r, :cols], mask)
            assert torch.equal(got[r, :cols].view(torch.int16), want.view(torch.int16)), (cols, hist_len, b, j, which)
            total += int(mask.sum())
    plan.apply(src, ld, src, ld, batch, width, cols, hd if hist_len else None, hist_len, tail=td if width > 1 else None, step0=step0)
    inp = src.cpu()
    assert torch.equal(inp[:, :cols].view(torch.int16), got[:R, :cols].view(torch.int16))                # in place == out of place
    after = flat.cpu().view(torch.int16)
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    keep[offset:offset + R * ld].view(R, ld)[:, :cols] = False
    assert torch.equal(after[keep], before.cpu().view(torch.int16)[keep])           # pad columns and surroundings unchanged
    return total


@pytest.mark.parametrize("cols,ld,offset", [(33, 40, 0), (37, 37, 3), (1000, 1000, 0), (1000, 1003, 5), (1032, 1040, 0), (1032, 1032, 8)])
def test_kernel_shapes_and_alignments(cols, ld, offset):
    for width, hist_len in ((1, 12), (4, 12)):
        assert _case(cols, ld, offset, 2, width, hist_len) > 0


@pytest.mark.parametrize("cols,ld", [(128256, 128256), (151936, 151944)])
def test_kernel_real_vocab(cols, ld):
    assert _case(cols, ld, 0, 2, 1, 1027) > 0
    assert _case(cols, ld, 0, 1, 8, 40, step0=1) > 0


@pytest.mark.parametrize("hist_len", [0, 1, 2, 3, 1027])                          # 0, n - 2, n - 1, n and more than one thread stride
def test_kernel_history_lengths(hist_len):
    for width in (1, 8):
        _case(1000, 1000, 0, 2, width, hist_len)
    hits = _case(1000, 1000, 0, 2, 1, hist_len, which="no_repeat_ngram_size")
    assert hits == 0 if hist_len < 3 else (hits > 0 or hist_len == 3)              # L < n: no n-gram yet; a long history has repeats
    hits = _case(1000, 1000, 0, 2, 1, hist_len, which="no_repeat_ngram_size", n=1)
    # n = 1 bans what the history holds: junk behind hist_len read as history would add its two ids to each row
    assert hits == sum(len(set(_LAST["hist"][b, :hist_len].tolist())) for b in range(2))


@pytest.mark.parametrize("which", list(CR.KEYS))
def test_kernel_each_rule_alone(which):
    hits = [_case(1000, 1008, 0, 2, width, 12, which=which, n=2, step0=step0) for width, step0 in ((1, 0), (8, 0), (4, 2))]
    assert hits[0] > 0 and hits[1] > 0
    if which == "begin_suppress_tokens":
        assert hits == [4, 4, 0]                                                    # two ids, row j = 0 of two sequences, step 0 only
    if which == "min_new_tokens":
        assert hits == [4, 12, 4]                                                   # two EOS ids while t < 3


@pytest.mark.parametrize("width", [4, 8])
def test_grouped_row_is_the_one_row_call_on_the_joined_history(width):
    from desta import _hip as H
    from desta.models.modeling_desta25 import ConstraintPlan
    gen = torch.Generator().manual_seed(width)
    cols, ld, batch, hist_len, step0 = 1000, 1008, 3, 9, 1
    src = (3.0 * torch.randn(batch * width, ld, generator=gen)).to(torch.bfloat16).cuda()
    hist, tail = torch.randint(0, 4, (batch, hist_len), generator=gen).cuda(), torch.randint(0, 4, (batch, width), generator=gen).cuda()
    tail[1, 1] = -1
    plan = ConstraintPlan("cuda", EOS, **_settings("all", 2, [[1, 2], [3], [0, 0, 1]]))
    grouped = torch.zeros_like(src)
    plan.apply(src, ld, grouped, ld, batch, width, cols, hist, hist_len, tail=tail, step0=step0)
    one = torch.zeros(1, ld, dtype=torch.bfloat16, device="cuda")
    for b in range(batch):
        for j in range(width):
            r = b * width + j
            joined = torch.cat([hist[b], tail[b, 1:1 + j]]).view(1, -1).contiguous()
            plan.apply(src[r:r + 1], ld, one, ld, 1, 1, cols, joined, hist_len + j, step0=step0 + j)
            assert torch.equal(one[0, :cols].view(torch.int16), grouped[r, :cols].view(torch.int16)), (b, j)


def test_kernel_argument_errors():
    from desta import _hip as H
    from desta.models.modeling_desta25 import ConstraintPlan
    cols, ld = 64, 64
    src = torch.zeros(16, ld, dtype=torch.bfloat16, device="cuda")
    dst = torch.full((16, ld), SENTINEL, dtype=torch.bfloat16, device="cuda")
    hist = torch.zeros(2, 8, dtype=torch.int64, device="cuda")
    tail = torch.zeros(2, 8, dtype=torch.int64, device="cuda")
    ids = torch.tensor([1, 2, 3], dtype=torch.int32, device="cuda")
    off = torch.tensor([0, 2, 3], dtype=torch.int32, device="cuda")
    p, st = H.p, H.stream()
    good = dict(src=p(src), ld_src=ld, dst=p(dst), ld_dst=ld, batch=2, width=2, cols=cols, hist=p(hist), hist_ld=8, hist_len=4, tail=p(tail),
                tail_ld=8, step0=0, ngram=2, word_ids=p(ids), word_off=p(off), n_words=2, n_word_ids=3, begin_ids=p(ids), n_begin=3,
                eos_ids=p(ids), n_eos=3, min_new=2, id_max=3)

    def call(**kw):
        return H._logit_constraints(*{**good, **kw}.values(), st)
    assert call() == 0
    bad = [dict(width=0), dict(width=9), dict(tail=0), dict(tail_ld=1), dict(hist=0), dict(hist_ld=3), dict(hist_len=-1), dict(batch=-1),
           dict(batch=0), dict(cols=-1), dict(cols=0), dict(ngram=-1), dict(n_words=-1), dict(n_word_ids=-1), dict(n_begin=-1), dict(n_eos=-1),
           dict(min_new=-1), dict(ld_src=cols - 1), dict(ld_dst=cols - 1), dict(cols=262145, ld_src=262145, ld_dst=262145), dict(id_max=cols),
           dict(src=0), dict(dst=0), dict(word_ids=0), dict(word_off=0), dict(begin_ids=0), dict(eos_ids=0), dict(n_words=65537, n_word_ids=65537),
           dict(n_word_ids=1048577), dict(n_word_ids=1)]
    dst.fill_(SENTINEL)
    for kw in bad:
        assert call(**kw) == -1, kw                                                 # DESTA_EINVAL
        assert b"logit_constraints" in H.lib.desta_last_error()
    assert call(ngram=0, n_words=0, n_begin=0, min_new=0) == 0 and call(ngram=0, n_words=0, n_begin=0, n_eos=0) == 0      # every rule off
    assert bool((dst == SENTINEL).all())                                            # none of these launched anything
    n0 = H.CONSTRAINT_CALLS
    with pytest.raises(RuntimeError, match="desta_logit_constraints_bf16.*token id 64"):    # a word id >= cols, through the binding
        ConstraintPlan("cuda", [], bad_words_ids=[[3, 64]]).apply(src, ld, dst, ld, 2, 1, cols, hist, 4)
    H.logit_constraints(src, ld, dst, ld, 2, 1, cols)                               # no rule: accepted, not counted
    assert H.CONSTRAINT_CALLS == n0 and bool((dst == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ decode loops
T = 24
KW = dict(pad_token_id=0, max_new_tokens=T)
_S = {}


def _gen_inputs(g, batch):
    n_ctx = int(g["gen_ctx_len"])
    return {"context_input_ids": batch["input_ids"][:, :n_ctx], "context_attention_mask": batch["attention_mask"][:, :n_ctx],
            "context_batch_start_positions": batch["batch_start_positions"], "batch_features": batch["batch_features"],
            "batch_transcription_ids": batch["batch_transcription_ids"]}


def _text_inputs(d):
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(3, d.vocab, (3, 21), generator=gen)
    am = torch.ones(3, 21, dtype=torch.long)
    am[1, :6] = 0
    ids[1, :6] = 0
    return {"context_input_ids": ids, "context_attention_mask": am, "context_batch_start_positions": [], "batch_features": None,
            "batch_transcription_ids": []}


def _setup(golden_dir):
    """One tiny Llama, the audio prompt and the text-only prompt, and the unconstrained greedy run of each (shared, unchanged)."""
    if not _S:
        from desta.models.modeling_desta25 import DeSTA25AudioModel
        d = O.tiny_dims(False)
        g, batch = golden_batch(golden_dir, "llama")
        model = DeSTA25AudioModel(cfg_from_dims(d), weights=O.init_weights(d, seed=7))
        audio, text = _gen_inputs(g, batch), _text_inputs(d)
        kinds = {"audio": (audio, {}, [[] for _ in range(audio["context_input_ids"].shape[0])]),
                 "text": (text, dict(prompt_in_history=True), text["context_input_ids"].tolist())}
        plain = {k: model._generate_step(v[0], do_sample=False, eos_token_id=[], **v[1], **KW).cpu() for k, v in kinds.items()}
        _S.update(model=model, d=d, g=g, batch=batch, kinds=kinds, plain=plain)
    return types.SimpleNamespace(**_S)


def _narrowed(plain, V):
    """suppress_tokens that leave four tokens (the first four of row 0 of `plain`).  The random tiny model repeats no token in T
    steps on its own; over four tokens there are 16 bigrams, so ANY run of more than 17 tokens repeats one: the n-gram rule has
    something to forbid, whatever the model prefers."""
    keep = set(plain[0, :4].tolist())
    return [c for c in range(V) if c not in keep]


def _rules(plain):
    """Settings the unconstrained run `plain` [B, T] violates by construction (the n-gram rule: see `_narrowed`), and the EOS ids
    that go with min_new_tokens: row 0's second token ends a sequence."""
    p = plain.tolist()
    return {"no_repeat_ngram_size": dict(no_repeat_ngram_size=2),
            "bad_words_ids": dict(bad_words_ids=[p[0][2:4], [p[1][1]], p[0][5:8]]),
            "suppress_tokens": dict(suppress_tokens=[p[0][3], p[1][0]]),
            "begin_suppress_tokens": dict(begin_suppress_tokens=[p[0][0], p[1][0]]),
            "min_new_tokens": dict(min_new_tokens=4)}, [p[0][1]]


def _replay(ids, lg, prompts, eos, s, pad=0, penalty=None):
    """Greedy replay on the host: at every step the restatement applied to the collected raw logits (the repetition penalty in
    fp32 in front, as tests/sampling_reference.py spells it) has its first maximum at the emitted token."""
    ids, lg = ids.cpu(), lg.cpu()
    B, n_new = ids.shape
    V = lg.shape[-1]
    done = [False] * B
    banned_total = 0
    for t in range(n_new):
        for b in range(B):
            if done[b]:
                assert int(ids[b, t]) == pad
                continue
            h = list(prompts[b]) + ids[b, :t].tolist()
            mask = CR.banned_mask(h, t, V, eos_token_ids=eos, **s)
            row = lg[t, b:b + 1]
            if penalty is not None:
                row = torch.from_numpy(SR.scores(row, torch.tensor([h], dtype=torch.long).view(1, len(h)), penalty)[0])
            want = int(CR.apply(row[0].float(), mask).argmax())
            assert want == int(ids[b, t]), (t, b, want, int(ids[b, t]))
            banned_total += int(mask.sum())
            done[b] = int(ids[b, t]) in eos
    return banned_total


@pytest.mark.parametrize("kind", ["audio", "text"])
@pytest.mark.parametrize("rule", list(CR.KEYS) + ["all"])
def test_plain_loop_follows_its_own_logits(golden_dir, kind, rule):
    from desta import _hip as H
    S = _setup(golden_dir)
    inputs, extra, prompts = S.kinds[kind]
    plain = S.plain[kind]
    rules, eos = _rules(plain)
    s = {k: v for r in rules.values() for k, v in r.items()} if rule == "all" else rules[rule]
    use_eos = eos if rule in ("min_new_tokens", "all") else []
    # the unconstrained run of the same prompt breaks the rule: the constrained one cannot pass by doing nothing
    kw = dict(KW)
    if rule == "no_repeat_ngram_size":                                              # on four tokens: the run without the rule repeats a bigram
        narrow = _narrowed(plain, S.d.vocab)
        plain = S.model._generate_step(inputs, do_sample=False, eos_token_id=[], suppress_tokens=narrow, **extra, **KW).cpu()
        s = dict(s, suppress_tokens=narrow)
        kw["max_new_tokens"] = 12                                                   # 16 bigrams: the rule leaves room for 17 tokens at most
    cut = [r[:next((i + 1 for i, x in enumerate(r) if x in use_eos), len(r))] for r in plain.tolist()]
    assert any(CR.violations(r, S.d.vocab, prompt=pr, eos_token_ids=use_eos, **s) for r, pr in zip(cut, prompts)), (kind, rule, plain.tolist())
    n0 = H.CONSTRAINT_CALLS
    ids, lg = S.model._generate_step(inputs, do_sample=False, collect_logits=True, eos_token_id=use_eos, **extra, **s, **kw)
    steps = H.CONSTRAINT_CALLS - n0
    assert ids.shape[0] == plain.shape[0] and lg.shape[0] == ids.shape[1]
    assert steps == ids.shape[1] if not use_eos else ids.shape[1] <= steps <= T     # one launch per step (a trimmed tail ran its steps too)
    assert _replay(ids, lg, prompts, use_eos, s) > 0
    for r, pr in zip(ids.tolist(), prompts):
        assert CR.violations(r, S.d.vocab, prompt=pr, eos_token_ids=use_eos, **s) == []
    # the in-place form (nothing reads the logits again) picks the same tokens
    n0 = H.CONSTRAINT_CALLS
    ids2 = S.model._generate_step(inputs, do_sample=False, eos_token_id=use_eos, **extra, **s, **kw)
    assert torch.equal(ids2, ids) and H.CONSTRAINT_CALLS - n0 == steps


def test_without_a_plan_nothing_changes(golden_dir):
    from desta import _hip as H
    S = _setup(golden_dir)
    inputs = S.kinds["audio"][0]
    ref_ids = S.g["gen_ids"]
    off = {k: None for k in CR.KEYS}
    n0 = H.CONSTRAINT_CALLS
    kw = dict(pad_token_id=0, max_new_tokens=10, do_sample=False)
    ids_f = S.model._generate_step(inputs, forced_tokens=ref_ids, **kw)              # the golden-token expectations of test_gpu_generate.py
    assert ids_f.cpu().tolist() == ref_ids.tolist()
    ids_e = S.model._generate_step(inputs, eos_token_id=int(S.g["gen_eos_id"]), forced_tokens=ref_ids, **off, **kw)
    assert ids_e.cpu().tolist() == S.g["gen_ids_eos"].tolist()
    free = S.model._generate_step(inputs, **kw)
    assert bool((free[:, 0].cpu() == ref_ids[:, 0]).all())
    a, la = S.model._generate_step(inputs, collect_logits=True, **kw)
    b, lb = S.model._generate_step(inputs, collect_logits=True, **off, **kw)
    assert torch.equal(a, b) and torch.equal(a, free) and torch.equal(la.view(torch.int16), lb.view(torch.int16))
    assert H.CONSTRAINT_CALLS == n0


def test_with_repetition_penalty_and_sampling(golden_dir):
    S = _setup(golden_dir)
    for kind in ("audio", "text"):
        inputs, extra, prompts = S.kinds[kind]
        rules, eos = _rules(S.plain[kind])
        s = {k: v for r in rules.values() for k, v in r.items()}
        ids, lg = S.model._generate_step(inputs, do_sample=False, collect_logits=True, eos_token_id=eos, repetition_penalty=1.3, **extra, **s, **KW)
        assert _replay(ids, lg, prompts, eos, s, penalty=1.3) > 0
        for sample_kw in (dict(top_k=20, repetition_penalty=1.2), dict(temperature=1.5, top_p=0.95)):
            ids = S.model._generate_step(inputs, do_sample=True, seed=3, eos_token_id=eos, **sample_kw, **extra, **s, **KW)
            for r, pr in zip(ids.tolist(), prompts):
                assert CR.violations(r, S.d.vocab, prompt=pr, eos_token_ids=eos, **s) == [], (kind, sample_kw)


def test_guided(golden_dir):
    from desta import _hip as H
    S = _setup(golden_dir)
    inputs2 = GR.guided_inputs(S.g, S.batch)
    g = 1.5
    kw = dict(do_sample=False, guidance_scale=g, eos_token_id=[], **KW)
    plain = S.model._generate_step(inputs2, **kw).cpu()
    rules, _ = _rules(plain)
    s = {k: v for k, v in {**rules["no_repeat_ngram_size"], **rules["bad_words_ids"], **rules["begin_suppress_tokens"]}.items()}
    assert any(CR.violations(r, S.d.vocab, **s) for r in plain.tolist())
    c0, k0 = H.CFG_SCORES_CALLS, H.CONSTRAINT_CALLS
    ids, lg = S.model._generate_step(inputs2, collect_logits=True, **s, **kw)
    assert H.CFG_SCORES_CALLS - c0 == T == H.CONSTRAINT_CALLS - k0 and ids.shape == (2, T) and lg.shape == (T, 4, S.d.vocab)
    # replay on g (lc - lu) + lu in float64 with the banned set taken out; a cell counts when its lead exceeds the guided
    # scores' derived bound (tests/guidance_reference.py), as for the unconstrained guided loop
    R, Lc, Lu = GR.guided_scores_fp64(lg[:, :2].cpu(), lg[:, 2:].cpu(), g)
    Bd = GR.guided_bound(R, Lc, Lu, g)
    ids_c = ids.cpu()
    for t in range(T):
        for b in range(2):
            R[t, b][torch.from_numpy(CR.banned_mask(ids_c[b, :t].tolist(), t, S.d.vocab, **s))] = GR.NEG_INF
    top2 = R.topk(2, dim=-1)
    b12 = Bd.gather(-1, top2.indices)
    counts = (top2.values[..., 0] - top2.values[..., 1]) > 2 * b12.max(dim=-1).values
    reach = torch.where(torch.isinf(R), R, R + Bd).scatter(-1, top2.indices[..., :1], GR.NEG_INF).max(dim=-1).values
    counts &= top2.values[..., 0] - b12[..., 0] > reach
    assert torch.equal(ids_c.t()[counts], top2.indices[..., 0][counts]) and float(counts.float().mean()) >= 0.75
    for r in ids_c.tolist():
        assert CR.violations(r, S.d.vocab, **s) == []


def _lp_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in
               ((a.token_logprobs, b.token_logprobs), (a.top_ids, b.top_ids), (a.top_logprobs, b.top_logprobs)))


def test_logprobs_stay_the_models_own(golden_dir):
    from desta import _hip as H
    S = _setup(golden_dir)
    inputs, extra, prompts = S.kinds["audio"]
    rules, _ = _rules(S.plain["audio"])
    s = {**rules["no_repeat_ngram_size"], **rules["bad_words_ids"], **rules["suppress_tokens"]}
    ids, lg, lp = S.model._generate_step(inputs, do_sample=False, collect_logits=True, logprobs=3, eos_token_id=[], **s, **KW)
    assert _replay(ids, lg, prompts, [], s) > 0
    B, V, Vp = ids.shape[0], S.d.vocab, S.model.llm.Vp
    raw = torch.zeros(B, Vp, dtype=torch.bfloat16, device="cuda")
    tok, top_i, top_v = (torch.zeros(B, dtype=torch.float32, device="cuda"), torch.zeros(B, 3, dtype=torch.int32, device="cuda"),
                         torch.zeros(B, 3, dtype=torch.float32, device="cuda"))
    for t in range(T):
        raw[:, :V] = lg[t]
        H.topk_logprobs(raw, Vp, ids[:, t].contiguous(), B, V, 3, tok, top_i, top_v)
        assert torch.equal(tok.view(torch.int32), lp.token_logprobs[:, t].view(torch.int32)), t
        assert torch.equal(top_i, lp.top_ids[:, t]) and torch.equal(top_v.view(torch.int32), lp.top_logprobs[:, t].view(torch.int32)), t
    assert bool(torch.isfinite(lp.top_logprobs).all())                              # a banned token still shows its raw probability


@pytest.mark.parametrize("mode", ["greedy", "sampled"])
def test_speculation_emits_the_plain_loops_tokens(golden_dir, mode):
    from desta import _hip as H
    S = _setup(golden_dir)
    inputs, extra, prompts = S.kinds["text"]
    rules, eos = _rules(S.plain["text"])
    s = {k: v for r in rules.values() for k, v in r.items()}
    pick = dict(do_sample=False, repetition_penalty=1.2) if mode == "greedy" else dict(do_sample=True, top_k=20, seed=3)
    kw = dict(logprobs=3, eos_token_id=eos, **pick, **extra, **s, **KW)
    ids, lp = S.model._generate_step(inputs, **kw)
    ids0 = S.model._generate_step(inputs, **{**kw, "logprobs": None, "repetition_penalty": None}) if mode == "greedy" else None
    drafts = torch.full((ids.shape[0], T), -1, dtype=torch.int64)
    drafts[:, :ids.shape[1]] = ids.cpu()
    drafts[:, 3::4] = (drafts[:, 3::4] + 1) % S.d.vocab                             # every fourth proposal is wrong, one is missing
    drafts[0, 6] = -1
    S.model.set_speculative(3, scope="all")
    try:
        k0, a0 = H.CONSTRAINT_CALLS, H.SPEC_ACCEPT_CALLS
        ids_s, lp_s = S.model._generate_step(inputs, draft_tokens=drafts, **kw)
        st = S.model.llm.spec_stats
        assert st["path"] == "speculative" and st["drafts_accepted"] > 0
        assert H.CONSTRAINT_CALLS - k0 == 1 + (H.SPEC_ACCEPT_CALLS - a0)            # the first pick, then one launch per verify step
        assert torch.equal(ids_s, ids) and _lp_equal(lp_s, lp)
        if mode == "greedy":                                                        # no chain at all: the argmax picker behind the pass
            ids_p = S.model._generate_step(inputs, draft_tokens=drafts, **{**kw, "logprobs": None, "repetition_penalty": None})
            assert S.model.llm.spec_stats["path"] == "speculative" and torch.equal(ids_p, ids0)
        S.model.set_speculative(3, scope="greedy")
        ids_g = S.model._generate_step(inputs, draft_tokens=drafts, do_sample=False, eos_token_id=eos, **extra, **s, **KW)
        st = S.model.llm.spec_stats
        assert st["path"] == "plain" and st["reason"] == "logit_constraints"
        for r, pr in zip(ids_g.tolist(), prompts):
            assert CR.violations(r, S.d.vocab, prompt=pr, eos_token_ids=eos, **s) == []
    finally:
        S.model.set_speculative(None)


# ------------------------------------------------------------------------------------------------ chat level and trainer
def test_chat_generate_and_trainer(golden_dir, tmp_path):
    import wave
    import numpy as np
    from desta.trainer.desta_trainer import DeSTA25Trainer, TrainingArguments
    S = _setup(golden_dir)
    feats = S.g["batch_features"]

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
    model, V = S.model, S.d.vocab
    model._setup_generation(tokenizer=ToyTokenizer(vocab_size=V), processor=Proc(), vad=lambda w: True, asr=lambda ws: ["spoken words"] * len(ws))
    eos = model.config.llm_config.eos_token_id
    eos = [eos] if isinstance(eos, int) else list(eos or [])
    plain = model.generate(msgs, do_sample=False, max_new_tokens=12).generated_ids
    p0 = plain[0] + [0] * 12
    s = dict(no_repeat_ngram_size=2, bad_words_ids=[[p0[0]], p0[1:3]], min_new_tokens=4)
    assert any(CR.violations(r, V, eos_token_ids=eos, **s) for r in plain)
    out = model.generate(msgs, do_sample=False, max_new_tokens=12, **s)
    assert len(out.generated_ids) == len(plain) and out.generated_ids != plain
    for r in out.generated_ids:
        assert CR.violations(r, V, eos_token_ids=eos, **s) == []
        assert len(r) >= 4 and not any(x in eos for x in r[:4])
    # text-only: the prompt ids are part of the history
    text = [[{"role": "user", "content": "hi there"}], [{"role": "user", "content": "a somewhat longer question , please"}]]
    tp = model.generate(text, do_sample=False, max_new_tokens=8).generated_ids
    st = dict(no_repeat_ngram_size=1, suppress_tokens=[tp[0][0]], begin_suppress_tokens=[tp[1][0]])
    got = model.generate(text, do_sample=False, max_new_tokens=8, **st).generated_ids
    tok, tin, _, _ = model._chat_inputs(text)
    ends = [tok.eos_token_id, tok.convert_tokens_to_ids("<|eot_id|>")]
    assert got != tp
    for r, pr in zip(got, tin["context_input_ids"].tolist()):
        assert CR.violations(r, V, prompt=pr, eos_token_ids=ends, **st) == []
    # the trainer passes model.generation_kwargs through
    full = dict(S.batch)
    full.update(S.kinds["audio"][0])
    narrow = _narrowed(S.plain["audio"], V)                                         # 20 tokens over four: the run without the rule repeats a bigram
    kw = dict(pad_token_id=0, max_new_tokens=20, do_sample=False, suppress_tokens=narrow)
    base = model._generate_step(full, **kw).cpu()
    gk = {"max_new_tokens": 20, "do_sample": False, "suppress_tokens": narrow, "no_repeat_ngram_size": 2}
    tr = DeSTA25Trainer(model, cfg=types.SimpleNamespace(model=types.SimpleNamespace(generation_kwargs=gk)), args=TrainingArguments(max_steps=10))
    ids = tr._predict_step(full).cpu()
    assert torch.equal(ids, model._generate_step(full, no_repeat_ngram_size=2, **kw).cpu()) and not torch.equal(ids, base)
    assert torch.equal(tr._predict_step(full, {"no_repeat_ngram_size": 3, "begin_suppress_tokens": [int(base[0, 0])]}).cpu(),
                       model._generate_step(full, no_repeat_ngram_size=3, begin_suppress_tokens=[int(base[0, 0])], **kw).cpu())
