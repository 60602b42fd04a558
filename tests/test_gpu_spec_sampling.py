"""GPU: draft-and-verify decoding for sampled, penalised and scored calls (`set_speculative(k, scope="all")`,
desta_sample_rows_bf16, desta_sample_top_p_rows_bf16).

Kernels (tables of tests/sampling_reference.py; 64 rows as batch x width in {64 x 1, 32 x 2, 16 x 4, 8 x 8}):
  1. a grouped launch equals, bit for bit in `out` and `keep_mask`, `width` launches of the one-row entry point with rows = batch,
     step = step0 + j and the history extended by the j tail tokens in front of row j (the rows of sequence b are rows b * width + j
     of the same buffer, so both launches read the same addresses); step0 in {0, 2^32 - 2}: the uint32 sum wraps inside a group;
  2. flat rows: every pick is sampling_reference.flat_pick under u24(seed, step0 + j, b), no tolerance: the counter is
     (position, sequence), not the flat row and not step0 for every row (tests/test_spec_sampling_host.py shows both change a pick);
  3. rejected arguments return DESTA_EINVAL and launch nothing.
Model (the tiny models and prompts of tests/test_gpu_speculative.py, B = 3, T = 24, k in {3, 7}: M = 12 and 24, where
test_verify_step_vs_single_steps finds the verify step's logits bit-equal to the single steps'):
  4. under scope "all" `_generate_step` returns the plain loop's tokens, per-step logits and `TokenLogprobs`, whatever the drafts are;
  5. a row that meets its EOS inside an accepted run; 6. the chat-level call, and the default scope's unchanged fallback.
No (row, step) case is excluded anywhere: the comparisons are `torch.equal`.

Measured (MI355X, profiles/r29_spec_sampling_tests.log): all 37 cases pass in 11 s, the slowest (V = 128256, 160 grouped launches
and their 600 one-row launches) in 1.3 s; perfect drafts 6 (k = 3) and 3 (k = 7) verify steps, all -1 drafts 23, in every setting.
On the parent commit every case fails: the entry points and the `scope` argument do not exist there."""
import math

import numpy as np
import pytest
import torch

import sampling_reference as S
from test_gpu_kv8_cache import _text_inputs
from test_gpu_prefill_chunk import PADS, _model
from test_gpu_speculative import SPEC_SEEDS

pytestmark = pytest.mark.gpu

PAD = 60.0
SENTINEL = -77
LAYOUTS = ((64, 1), (32, 2), (16, 4), (8, 8))
STEP0S = (0, 2 ** 32 - 2)
GREEDY_PENALTY = dict(T=1.0, penalty=1.3, greedy=True)
SETTINGS = ([("chain", n, s) for n, s in S.CHAIN_SETTINGS.items()] + [("top_p", n, s) for n, s in S.TOP_P_SETTINGS.items()]
            + [("chain", "greedy_penalty", GREEDY_PENALTY)])


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _buf(logits, ld):
    rows, V = logits.shape
    buf = torch.full((rows, ld), PAD, dtype=torch.bfloat16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[:, :V] = logits.cuda()
    return buf


def _tails(logits, hist, batch, width, V):
    """The verify input [batch, width]: column 0 the last history token; drafts that matter to a penalty (the row maxima of the
    sequence's own rows), and by sequence b % 4: 1 a repeated token, 2 a -1, 3 an id >= V."""
    top = logits.float().argmax(-1).view(batch, width)
    tail = torch.empty(batch, width, dtype=torch.int64)
    tail[:, 0] = hist[:batch, -1]
    for j in range(1, width):
        tail[:, j] = top[:, j]                                               # the draft in front of row j is row j's own best token
    for b in range(batch):
        if width > 1 and b % 4 == 1:
            tail[b, 1:] = top[b, width - 1]
        if width > 1 and b % 4 == 2:
            tail[b, 1] = -1
        if width > 1 and b % 4 == 3:
            tail[b, 1] = V + 5
    return tail


def _grouped(hip, kernel, s, buf, V, batch, width, hist, tail, seed, step0):
    ld = buf.shape[1]
    guard = torch.full((64 + 16,), SENTINEL, dtype=torch.int64, device="cuda")
    out = guard[8:72]
    mask = torch.full((64, V), 3, dtype=torch.uint8, device="cuda")
    if kernel == "chain":
        pen = s.get("penalty", 1.0)
        hip.sample_rows(buf, ld, batch, width, V, out, do_sample=not s.get("greedy", False), temperature=s["T"], top_k=s.get("top_k", 0),
                        top_p=s.get("top_p", 1.0), min_p=s.get("min_p", 0.0), repetition_penalty=pen, hist=hist if pen != 1.0 else None,
                        hist_len=hist.shape[1] if pen != 1.0 else 0, tail=tail if (pen != 1.0 and width > 1) else None, seed=seed, step0=step0,
                        keep_mask=mask)
    else:
        hip.sample_top_p_rows(buf, ld, batch, width, V, s["T"], s["top_p"], seed, step0, out, keep_mask=mask)
    assert bool((guard[:8] == SENTINEL).all()) and bool((guard[72:] == SENTINEL).all())
    return out.clone(), mask


def _per_step(hip, kernel, s, buf, V, batch, width, hist, tail, seed, step0, j):
    """Row j of every sequence through the one-row entry point: rows b * width + j of `buf` as a [batch] launch of stride width * ld."""
    ld = buf.shape[1]
    rows_j = buf.view(-1)[j * ld:]
    out = torch.full((batch,), SENTINEL, dtype=torch.int64, device="cuda")
    mask = torch.full((batch, V), 3, dtype=torch.uint8, device="cuda")
    step = (step0 + j) & 0xFFFFFFFF
    if kernel == "chain":
        pen = s.get("penalty", 1.0)
        h = torch.cat([hist[:batch], tail[:, 1:1 + j]], dim=1).contiguous() if pen != 1.0 else None
        hip.sample(rows_j, width * ld, batch, V, out, do_sample=not s.get("greedy", False), temperature=s["T"], top_k=s.get("top_k", 0),
                   top_p=s.get("top_p", 1.0), min_p=s.get("min_p", 0.0), repetition_penalty=pen, hist=h, hist_len=0 if h is None else h.shape[1],
                   seed=seed, step=step, keep_mask=mask)
    else:
        hip.sample_top_p(rows_j, width * ld, batch, V, s["T"], s["top_p"], seed, step, out, keep_mask=mask)
    return out, mask


# ------------------------------------------------------------------------------------------------ 1. grouped == per-step launches
@pytest.mark.parametrize("profile", ["randn", "peaked", "suppressed"])
@pytest.mark.parametrize("V,ld", S.VLD[:3])
def test_grouped_launch_equals_per_step_launches(hip, V, ld, profile):
    logits, hist = S.rows_for(V, profile)
    buf, hist_d = _buf(logits, ld), hist.cuda()
    n_rows, n_top_p, differ = hip.SAMPLE_ROWS_CALLS, hip.SAMPLE_TOP_P_ROWS_CALLS, 0
    for batch, width in LAYOUTS:
        tail = _tails(logits, hist, batch, width, V).cuda()
        for kernel, name, s in SETTINGS:
            for step0 in STEP0S:
                for seed in S.SEEDS:
                    got, gmask = _grouped(hip, kernel, s, buf, V, batch, width, hist_d[:batch], tail, seed, step0)
                    for j in range(width):
                        want, wmask = _per_step(hip, kernel, s, buf, V, batch, width, hist_d, tail, seed, step0, j)
                        key = (name, batch, width, step0, seed, j)
                        assert torch.equal(got.view(batch, width)[:, j], want), key
                        assert torch.equal(gmask.view(batch, width, V)[:, j], wmask), key
                    if name == "greedy_penalty" and width > 1 and step0 == 0 and seed == S.SEEDS[0]:
                        # the tail matters: without it (the history of row 0 for every row) some pick differs
                        plain = torch.full((64,), SENTINEL, dtype=torch.int64, device="cuda")
                        hip.sample(buf, ld, 64, V, plain, do_sample=False, repetition_penalty=s["penalty"],
                                   hist=hist_d[:batch].repeat_interleave(width, dim=0).contiguous(), hist_len=hist.shape[1])
                        differ += int((plain != got).sum())
    per_layout = len(S.SEEDS) * len(STEP0S)
    assert hip.SAMPLE_ROWS_CALLS - n_rows == len(LAYOUTS) * per_layout * (len(S.CHAIN_SETTINGS) + 1)
    assert hip.SAMPLE_TOP_P_ROWS_CALLS - n_top_p == len(LAYOUTS) * per_layout * len(S.TOP_P_SETTINGS)
    assert differ > 0 or profile == "peaked"                                 # (a peak of 23 stays the maximum after / 1.3)


# ------------------------------------------------------------------------------------------------ 2. flat rows: the counter
@pytest.mark.parametrize("profile", S.FLAT)
@pytest.mark.parametrize("V,ld", S.VLD[:2])
def test_flat_rows_draw_the_closed_form_at_position_and_sequence(hip, V, ld, profile):
    logits, hist = S.rows_for(V, profile)
    buf, hist_d = _buf(logits, ld), hist.cuda()
    finite = torch.isfinite(logits.float()).numpy()
    for kernel, name, s in SETTINGS:
        if s.get("penalty", 1.0) != 1.0:
            continue                                                         # a penalised flat row is no longer flat
        case = S.CASE_BY_ID[f"{kernel}-V{V}-ld{ld}-{profile}-{name}"]
        kept = S.reference(case).kept
        assert np.array_equal(kept, finite)                                  # a flat row keeps its finite entries
        want_mask = torch.from_numpy(kept.astype(np.uint8)).cuda()
        for batch, width in LAYOUTS:
            for step0 in STEP0S:
                for seed in S.SEEDS:
                    got, gmask = _grouped(hip, kernel, s, buf, V, batch, width, hist_d[:batch], None, seed, step0)
                    want = [S.flat_pick(kernel, kept[b * width + j], S.u24(seed, (step0 + j) & S.M32, b)) for b in range(batch) for j in range(width)]
                    assert got.cpu().tolist() == want, (name, batch, width, step0, seed)
                    assert torch.equal(gmask, want_mask), (name, batch, width)


# ------------------------------------------------------------------------------------------------ 3. rejections
def test_grouped_rejections(hip):
    V, ld = S.VLD[0]
    logits, hist = S.rows_for(V, "randn")
    buf, hist_d = _buf(logits, ld), hist.cuda()
    guard = torch.full((64 + 16,), SENTINEL, dtype=torch.int64, device="cuda")
    out = guard[8:72]
    mask = torch.full((64, V), 3, dtype=torch.uint8, device="cuda")
    tail = torch.zeros(8, 8, dtype=torch.int64, device="cuda")
    n_rows, n_top_p = hip.SAMPLE_ROWS_CALLS, hip.SAMPLE_TOP_P_ROWS_CALLS
    for width in (0, 9, -1):
        with pytest.raises(RuntimeError, match="width") as ei:
            hip.sample_rows(buf, ld, 4, width, V, out, temperature=0.8, tail=None if width < 1 else torch.zeros(4, 9, dtype=torch.int64, device="cuda"),
                            keep_mask=mask)
        assert "(-1)" in str(ei.value)                                       # DESTA_EINVAL
        with pytest.raises(RuntimeError, match="width") as ei:
            hip.sample_top_p_rows(buf, ld, 4, width, V, 0.8, 0.9, 99, 0, out, keep_mask=mask)
        assert "(-1)" in str(ei.value)
    for do_sample in (True, False):
        with pytest.raises(RuntimeError, match="tail") as ei:                # an active penalty over two rows per sequence needs the drafts
            hip.sample_rows(buf, ld, 8, 2, V, out, do_sample=do_sample, repetition_penalty=1.3, hist=hist_d[:8], hist_len=hist.shape[1], tail=None,
                            keep_mask=mask)
        assert "(-1)" in str(ei.value)
    for bad in (dict(temperature=0.0), dict(top_p=0.0), dict(top_k=-1), dict(min_p=1.5), dict(repetition_penalty=0.0),      # the one-row entry point's checks
                dict(repetition_penalty=1.3, hist=None, hist_len=4)):
        with pytest.raises(RuntimeError, match="sample") as ei:
            hip.sample_rows(buf, ld, 8, 2, V, out, tail=tail, keep_mask=mask, **bad)
        assert "(-1)" in str(ei.value), bad
    torch.cuda.synchronize()
    assert hip.SAMPLE_ROWS_CALLS == n_rows and hip.SAMPLE_TOP_P_ROWS_CALLS == n_top_p
    assert bool((guard == SENTINEL).all()) and bool((mask == 3).all())      # nothing was launched
    hip.sample_rows(buf, ld, 8, 2, V, out, repetition_penalty=1.3, hist=hist_d[:8], hist_len=hist.shape[1], tail=tail)       # accepted: tail given
    hip.sample_rows(buf, ld, 8, 2, V, out, repetition_penalty=1.0, tail=None)                                               # ... penalty off: NULL tail
    hip.sample_rows(buf, ld, 8, 1, V, out, repetition_penalty=1.3, hist=hist_d[:8], hist_len=hist.shape[1], tail=None)       # ... width 1: NULL tail
    torch.cuda.synchronize()
    assert hip.SAMPLE_ROWS_CALLS == n_rows + 3 and bool((guard[:8] == SENTINEL).all()) and bool((guard[72:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 4. speculative == plain
T_NEW, B_ROWS = 24, 3
MODEL_SETTINGS = {
    "top_p": dict(do_sample=True, temperature=0.8, top_p=0.9),
    "chain": dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=20, min_p=0.05),
    "chain_penalty": dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=20, min_p=0.05, repetition_penalty=1.3),
    "greedy_penalty": dict(do_sample=False, repetition_penalty=1.3),
    "text_penalty": dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=20, repetition_penalty=1.3, prompt_in_history=True),
}


def _run(model, inputs, drafts=None, eos=(), T=T_NEW, logprobs=2, **kw):
    res = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, collect_logits=True, eos_token_id=list(eos), seed=11, logprobs=logprobs,
                               draft_tokens=drafts, **kw)
    ids, lg = res[0], res[1]
    lp = res[2] if logprobs is not None else None
    return ids.clone(), lg.clone(), None if lp is None else [t.clone() for t in (lp.token_logprobs, lp.top_ids, lp.top_logprobs)]


def _counters(hip):
    return {n: getattr(hip, n) for n in ("SAMPLE_ROWS_CALLS", "SAMPLE_TOP_P_ROWS_CALLS", "TOPK_LOGPROBS_CALLS", "SPEC_ACCEPT_CALLS", "SPEC_DRAFT_CALLS")}


@pytest.mark.parametrize("setting", list(MODEL_SETTINGS))
@pytest.mark.parametrize("S_prompt", [61, 251])
@pytest.mark.parametrize("g4", [False, True])
def test_speculative_equals_plain(hip, g4, S_prompt, setting):
    d, w, model = _model(g4)
    kw, T = MODEL_SETTINGS[setting], T_NEW
    inputs = _text_inputs(d, S_prompt, PADS[S_prompt], seed=SPEC_SEEDS[(g4, S_prompt)])[2]
    try:
        model.set_speculative(None)
        ids_p, lg_p, lp_p = _run(model, inputs, **kw)
        assert model.llm.spec_stats == dict(path="plain", reason="off", verify_steps=0, emitted=T, drafts_accepted=0)
        ids_q, _, _ = _run(model, inputs, logprobs=None, **kw)
        assert torch.equal(ids_p, ids_q) and ids_p.shape == (B_ROWS, T)
        assert bool(torch.isfinite(lp_p[0]).all()) and bool((lp_p[1] >= 0).all())
        if kw["do_sample"]:                                                  # a real draw: not the argmax everywhere
            assert int((ids_p != lg_p.float().argmax(-1).t()).sum()) > 0
        gen = torch.Generator().manual_seed(S_prompt)
        corrupt = ids_p.clone()
        for b in range(B_ROWS):
            corrupt[b, 3 + 5 * b] = (corrupt[b, 3 + 5 * b] + 1) % d.vocab      # a different position per row
        sources = {"perfect": ids_p, "none": torch.full_like(ids_p, -1), "corrupt": corrupt,
                   "random": torch.randint(0, d.vocab, ids_p.shape, generator=gen), "lookup": None}
        for k in (3, 7):
            model.set_speculative(k, scope="all")
            steps = {}
            for name, dr in sources.items():
                c0 = _counters(hip)
                ids, lg, lp = _run(model, inputs, dr, **kw)
                c1 = _counters(hip)
                st = dict(model.llm.spec_stats)
                key = (setting, k, name, st)
                assert torch.equal(ids, ids_p), key
                assert torch.equal(lg, lg_p), key
                assert all(torch.equal(a, b) for a, b in zip(lp, lp_p)), key
                assert st["path"] == "speculative" and st["reason"] is None and st["emitted"] == T, key
                assert st["drafts_accepted"] == T - 1 - st["verify_steps"], key
                n = st["verify_steps"]
                chain = setting != "top_p"
                assert c1["SPEC_ACCEPT_CALLS"] - c0["SPEC_ACCEPT_CALLS"] == n and c1["TOPK_LOGPROBS_CALLS"] - c0["TOPK_LOGPROBS_CALLS"] == n + 1, key
                assert c1["SAMPLE_ROWS_CALLS"] - c0["SAMPLE_ROWS_CALLS"] == (n if chain else 0), key
                assert c1["SAMPLE_TOP_P_ROWS_CALLS"] - c0["SAMPLE_TOP_P_ROWS_CALLS"] == (0 if chain else n), key
                assert c1["SPEC_DRAFT_CALLS"] - c0["SPEC_DRAFT_CALLS"] == (n if dr is None else 0), key
                steps[name] = n
            assert steps["perfect"] == math.ceil((T - 1) / (k + 1)) and steps["none"] == T - 1, steps
            assert steps["perfect"] < steps["corrupt"] < T - 1, steps
            ids, lg, lp = _run(model, inputs, sources["corrupt"], **kw)      # two identical runs: the same bits
            assert torch.equal(ids, ids_p) and torch.equal(lg, lg_p) and all(torch.equal(a, b) for a, b in zip(lp, lp_p))
            ids, _, _ = _run(model, inputs, sources["perfect"], logprobs=None, **kw)
            assert torch.equal(ids, ids_p) and model.llm.spec_stats["verify_steps"] == steps["perfect"]
    finally:
        model.set_speculative(None)


# ------------------------------------------------------------------------------------------------ 5. EOS inside an accepted run
@pytest.mark.parametrize("setting", ["top_p", "chain_penalty"])
def test_a_row_meets_its_eos_inside_an_accepted_run(hip, setting):
    d, w, model = _model(False)
    kw, T, k = MODEL_SETTINGS[setting], T_NEW, 3
    inputs = _text_inputs(d, 61, PADS[61], seed=SPEC_SEEDS[(False, 61)])[2]
    try:
        model.set_speculative(None)
        free, _, _ = _run(model, inputs, **kw)
        free = free.cpu().tolist()
        # perfect drafts, k = 3: the verify chunks hold emitted positions 1-4, 5-8, ...; a token first seen at position 6 or 7 of a row
        b, t = next((b, t) for t in (6, 7) for b in range(B_ROWS) if free[b][t] not in free[b][:t] and free[b][t] != 0)
        eos = [free[b][t]]
        ids_p, _, lp_p = _run(model, inputs, eos=eos, **kw)
        want = ids_p.cpu().tolist()
        assert want[b][:t + 1] == free[b][:t + 1] and want[b][t + 1:] == [0] * (ids_p.shape[1] - t - 1)
        assert any(eos[0] not in row for row in want)                        # another row goes on to the end
        assert ids_p.shape[1] == T
        for src in (ids_p, torch.full_like(ids_p, -1)):
            model.set_speculative(k, scope="all")
            ids, _, lp = _run(model, inputs, src, eos=eos, **kw)
            st = model.llm.spec_stats
            assert st["path"] == "speculative" and st["emitted"] == T
            assert torch.equal(ids, ids_p) and all(torch.equal(x, y) for x, y in zip(lp, lp_p)), st
            tl, ti, tp = (x.cpu() for x in lp)
            assert bool((tl[b, t + 1:] == 0).all()) and bool((ti[b, t + 1:] == -1).all()) and bool((tp[b, t + 1:] == 0).all())
            assert float(tl[b, t]) < 0 and bool((ti[b, t] >= 0).all())        # the EOS itself is scored
        assert model.llm.spec_stats["verify_steps"] == T - 1
        model.set_speculative(k, scope="all")
        _run(model, inputs, ids_p, eos=eos, **kw)
        assert model.llm.spec_stats["verify_steps"] < T - 1                  # accepted runs: the EOS of row b lay inside one
    finally:
        model.set_speculative(None)


# ------------------------------------------------------------------------------------------------ 6. chat level, default scope
def test_chat_level_sampled_generate_and_the_default_scope(hip):
    from helpers import ToyTokenizer
    d, w, model = _model(False)
    model._setup_generation(tokenizer=ToyTokenizer(vocab_size=d.vocab), processor=object())
    phrase = "the quick brown fox jumps over the lazy dog"
    msgs = [[{"role": "user", "content": f"repeat after me : {phrase} . {phrase} . {phrase} . now you :"}],
            [{"role": "user", "content": f"say {phrase} twice"}]]
    try:
        model.set_speculative(None)
        a = model.generate(msgs, do_sample=True, seed=5, max_new_tokens=20)
        a_pen = model.generate(msgs, do_sample=True, seed=5, max_new_tokens=20, top_k=20, repetition_penalty=1.2, logprobs=2)
        model.set_speculative(3, scope="all")
        n0 = hip.SAMPLE_TOP_P_ROWS_CALLS
        b = model.generate(msgs, do_sample=True, seed=5, max_new_tokens=20)
        st = model.llm.spec_stats
        assert st["path"] == "speculative" and st["reason"] is None and hip.SAMPLE_TOP_P_ROWS_CALLS - n0 == st["verify_steps"] > 0
        assert a.text == b.text and a.generated_ids == b.generated_ids
        b_pen = model.generate(msgs, do_sample=True, seed=5, max_new_tokens=20, top_k=20, repetition_penalty=1.2, logprobs=2)
        assert model.llm.spec_stats["path"] == "speculative"
        assert a_pen.generated_ids == b_pen.generated_ids and a_pen.token_logprobs == b_pen.token_logprobs and a_pen.top_logprobs == b_pen.top_logprobs
        assert model.generate(msgs, do_sample=True, seed=6, max_new_tokens=20).generated_ids != a.generated_ids      # the seed matters
        model.set_speculative(3)                                             # the default scope: today's fallback
        c = model.generate(msgs, do_sample=True, seed=5, max_new_tokens=20)
        assert model.llm.spec_stats["path"] == "plain" and model.llm.spec_stats["reason"] == "do_sample"
        assert c.generated_ids == a.generated_ids
    finally:
        model.set_speculative(None)
