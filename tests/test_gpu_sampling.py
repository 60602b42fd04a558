"""GPU: `desta_sample_bf16`, HF's whole logits chain in one kernel (repetition penalty -> greedy, or temperature -> top-k ->
top-p -> min-p -> draw), against transformers' own processors on the CPU in fp32, and the decode loop that uses it.

Kept sets must equal HF's except where fp32 rounding decides: a token whose top-p cumulative mass is within 2e-5 of
1 - top_p, a token whose exp(t - t_max) is within 1e-5 (relative) of min_p, or a token tied with the boundary score
(torch.sort leaves the order of ties unspecified, the kernel keeps every tie).  Top-k and the penalty are exact."""
import types

import pytest
import torch

import desta_oracle as O
from helpers import ToyTokenizer, cfg_from_dims, golden_batch

pytestmark = pytest.mark.gpu


def _hf_stages(logits, hist, penalty, temp, top_k, top_p, min_p):
    """fp32 scores after each HF processor: (penalised, after temperature + top-k, final)."""
    from transformers.generation.logits_process import (MinPLogitsWarper, RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper,
                                                        TopKLogitsWarper, TopPLogitsWarper)
    s = logits.float()
    if penalty != 1.0 and hist is not None and hist.shape[1] > 0:
        s = RepetitionPenaltyLogitsProcessor(float(penalty))(hist, s)
    pen = s
    if temp != 1.0:
        s = TemperatureLogitsWarper(float(temp))(None, s)
    if top_k:
        s = TopKLogitsWarper(int(top_k))(None, s)
    before_p = s
    if top_p < 1.0:
        s = TopPLogitsWarper(float(top_p))(None, s)
    if min_p:
        s = MinPLogitsWarper(float(min_p))(None, s)
    return pen, before_p, s


def _justified(i, row_before_p, ref_row, kept_row, top_p, min_p):
    """Why token i may differ between the kernel's and HF's kept set (module docstring)."""
    t = row_before_p
    fin = torch.isfinite(t)
    if not bool(fin[i]):
        return False
    probs = torch.softmax(t.double(), -1)
    tmax = t[fin].max()
    if min_p and abs(float(torch.exp((t[i] - tmax).double())) - min_p) <= 1e-5 * min_p:
        return True
    if top_p < 1.0:
        c_i = float(probs[probs <= probs[i]].sum())                     # mass of the tokens not more probable than i
        if abs(c_i - (1.0 - top_p)) < 2e-5:
            return True
    tie = (t[ref_row].min() == t[i]) if bool(ref_row.any()) else False
    tie = tie or ((t[kept_row].min() == t[i]) if bool(kept_row.any()) else False)
    return bool(tie)


def _run(logits, hist, *, do_sample=True, temp=1.0, top_k=0, top_p=1.0, min_p=0.0, penalty=1.0, seed=1234, step=0, ld=None):
    from desta import _hip as H
    rows, V = logits.shape
    ld = ld or (V + 8 - V % 8)
    buf = torch.zeros(rows, ld, dtype=torch.bfloat16, device="cuda")
    buf[:, :V] = logits.cuda()
    out = torch.zeros(rows, dtype=torch.int64, device="cuda")
    mask = torch.zeros(rows, V, dtype=torch.uint8, device="cuda")
    h = None if hist is None else hist.cuda().contiguous()
    H.sample(buf, ld, rows, V, out, do_sample=do_sample, temperature=temp, top_k=top_k, top_p=top_p, min_p=min_p, repetition_penalty=penalty,
             hist=h, hist_len=0 if hist is None else hist.shape[1], seed=seed, step=step, keep_mask=mask)
    return out.cpu(), mask.cpu().bool()


def _logits(V, rows=6, seed=0):
    g = torch.Generator().manual_seed(V * 31 + seed)
    x = (torch.randn(rows, V, generator=g) * 3.0)
    x[1, :60] = 30.0                                            # a tie group at the top, wider than k = 20 / 50
    x[2, :10] = 31.0                                            # ten above, thirty tied at the 20th value below them
    x[2, 10:40] = 30.5
    x[3, :V // 2] = -1.0                                        # half the row tied
    return x.to(torch.bfloat16)


def _hist(V, rows, L=40, seed=0):
    g = torch.Generator().manual_seed(seed + 7)
    h = torch.randint(0, V, (rows, L), generator=g)
    h[:, 1] = h[:, 0]                                            # duplicates: penalised once
    h[:, 2] = h[:, 0]
    h[:, 3:8] = torch.arange(5)                                  # ids 0..4 (the tie groups above, positive and negative logits)
    return h


CASES = {
    "topk1": dict(temp=0.7, top_k=1),
    "topk20": dict(temp=0.7, top_k=20),
    "topk50": dict(temp=1.0, top_k=50),
    "topk_over_V": dict(temp=1.3, top_k=10 ** 6),
    "penalty_topk": dict(temp=0.9, top_k=20, penalty=1.3, hist=True),
    "reward_topk": dict(temp=0.9, top_k=50, penalty=0.7, hist=True),
    "min_p": dict(temp=0.9, min_p=0.05),
    "full_chain": dict(temp=0.7, top_k=50, top_p=0.9, min_p=0.02, penalty=1.2, hist=True),
    "top_p_min_p": dict(temp=1.0, top_p=0.5, min_p=0.1),
}


@pytest.mark.parametrize("V", [512, 4099, 128256, 151936])
@pytest.mark.parametrize("case", list(CASES))
def test_kept_set_matches_hf_chain(V, case):
    c = dict(CASES[case])
    use_hist = c.pop("hist", False)
    logits = _logits(V)
    rows = logits.shape[0]
    hist = _hist(V, rows) if use_hist else None
    top_k = c.get("top_k", 0)
    out, kept = _run(logits, hist, **c)
    _, before_p, final = _hf_stages(logits, hist, c.get("penalty", 1.0), c["temp"], top_k, c.get("top_p", 1.0), c.get("min_p", 0.0))
    ref = torch.isfinite(final)
    for r in range(rows):
        diff = (kept[r] != ref[r]).nonzero().flatten().tolist()
        for i in diff:
            assert _justified(i, before_p[r], ref[r], kept[r], c.get("top_p", 1.0), c.get("min_p", 0.0)), (case, V, r, i)
        assert kept[r, int(out[r])]                                          # the draw is one of the kept tokens
        if top_k and c.get("top_p", 1.0) == 1.0 and not c.get("min_p"):
            assert torch.equal(kept[r], ref[r]), (case, V, r)                # top-k (+ penalty) alone: exact
    if case == "topk20":
        assert int(kept[1].sum()) == 60 and int(kept[2].sum()) == 40        # every tie at the k-th value kept


@pytest.mark.parametrize("V", [512, 4099, 151936])
def test_greedy_with_penalty_is_argmax_of_hf_scores(V):
    logits = _logits(V).float()
    logits[4, :] = -3.0                                         # ids 0..4 are in every history (_hist)
    logits[4, 1] = 4.0                                          # ids 1 and 3 tie after the penalty too: the first index wins
    logits[4, 3] = 4.0
    logits[4, 0] = 3.0
    logits[5, :] = -2.0
    logits[5, 2] = -0.75                                        # negative maximum, penalised: -1.5, still the maximum
    logits = logits.to(torch.bfloat16)
    hist = _hist(V, logits.shape[0])
    for penalty in (2.0, 1.0, 0.5):
        out, kept = _run(logits, hist, do_sample=False, penalty=penalty)
        pen, _, _ = _hf_stages(logits, hist, penalty, 1.0, 0, 1.0, 0.0)
        assert out.tolist() == pen.argmax(-1).tolist(), penalty
        assert kept.sum(1).tolist() == [1] * logits.shape[0] and bool(kept[torch.arange(logits.shape[0]), out].all())
    out, _ = _run(logits, hist, do_sample=False, penalty=2.0)
    assert int(out[4]) == 1


def test_full_chain_distribution_and_reproducibility():
    """Frequencies of 20000 draws match the renormalised kept probabilities (5 sigma); the same (seed, step, row) draws the
    same token."""
    V, n, rows = 64, 20000, 8
    g = torch.Generator().manual_seed(2)
    logits = (torch.randn(1, V, generator=g) * 2).to(torch.bfloat16).repeat(rows, 1)
    hist = torch.tensor([[3, 3, 9, 17, 40]]).repeat(rows, 1)
    kw = dict(temp=0.8, top_k=20, top_p=0.95, min_p=0.01, penalty=1.3, seed=99)
    outs = []
    for step in range(n // rows):
        o, kept = _run(logits, hist, step=step, **kw)
        outs.append(o)
    toks = torch.cat(outs)
    counts = torch.bincount(toks, minlength=V).float()
    _, _, final = _hf_stages(logits[:1], hist[:1], 1.3, 0.8, 20, 0.95, 0.01)
    ref = torch.isfinite(final[0])
    assert torch.equal(kept[0], ref)
    assert counts[~ref].sum() == 0
    q = torch.softmax(final[0], -1)
    freq = counts / counts.sum()
    sigma = torch.sqrt(q * (1 - q) / n)
    assert bool(((freq - q).abs() <= 5 * sigma + 1e-4).all()), (freq - q).abs().max()
    o1, _ = _run(logits, hist, step=5, **kw)
    o2, _ = _run(logits, hist, step=5, **kw)
    assert torch.equal(o1, o2) and torch.equal(o1, outs[5])
    assert len(set(toks[:64].tolist())) > 3


def test_bad_arguments():
    from desta import _hip as H
    V, rows = 512, 2
    buf = torch.zeros(rows, V, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(rows, dtype=torch.int64, device="cuda")
    hist = torch.zeros(rows, 4, dtype=torch.int64, device="cuda")
    good = dict(hist=hist.data_ptr(), hist_ld=4, hist_len=4, pen=1.2, do_sample=1, temp=0.7, top_k=20, top_p=0.9, min_p=0.1)

    def call(**kw):
        a = dict(good, **kw)
        return H._sample_chain(buf.data_ptr(), V, rows, V, a["hist"], a["hist_ld"], a["hist_len"], a["pen"], a["do_sample"], a["temp"],
                               a["top_k"], a["top_p"], a["min_p"], 1, 0, out.data_ptr(), None, H.stream())
    assert call() == 0
    for kw in (dict(temp=0.0), dict(temp=-1.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(min_p=-0.1), dict(min_p=1.1),
               dict(pen=0.0), dict(pen=-1.0), dict(hist_len=-1), dict(hist_ld=2), dict(hist=None)):
        assert call(**kw) == -1, kw                                          # DESTA_EINVAL
    with pytest.raises(RuntimeError, match="desta_sample_bf16"):
        H.sample(buf, V, rows, V, out, temperature=0.0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ decode loop
def _model(d, seed=7, **kw):
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    return DeSTA25AudioModel(cfg_from_dims(d, **kw), weights=O.init_weights(d, seed=seed))


def _gen_inputs(g, batch):
    n_ctx = int(g["gen_ctx_len"])
    return {"context_input_ids": batch["input_ids"][:, :n_ctx], "context_attention_mask": batch["attention_mask"][:, :n_ctx],
            "context_batch_start_positions": batch["batch_start_positions"], "batch_features": batch["batch_features"],
            "batch_transcription_ids": batch["batch_transcription_ids"]}


def _check_picks(ids, logits, kw, prompt=None):
    """Every pick of `_generate_step` is what HF's processors allow on the product's own logits, with the product's own
    prefix (after `prompt`, if the prompt is part of HF's input_ids) as history."""
    ids, logits = ids.cpu(), logits.float().cpu()
    T, B, V = logits.shape
    for t in range(T):
        hist = ids[:, :t] if prompt is None else torch.cat([prompt.cpu(), ids[:, :t]], 1)
        pen, before_p, final = _hf_stages(logits[t], hist, kw.get("repetition_penalty") or 1.0, kw.get("temperature", 1.0),
                                          kw.get("top_k") or 0, kw.get("top_p", 1.0), kw.get("min_p") or 0.0)
        for r in range(B):
            i = int(ids[r, t])
            if not kw.get("do_sample", True):
                assert i == int(pen[r].argmax()), (t, r)
            elif not torch.isfinite(final[r, i]):
                assert _justified(i, before_p[r], torch.isfinite(final[r]), torch.isfinite(final[r]) | (torch.arange(V) == i),
                                  kw.get("top_p", 1.0), kw.get("min_p") or 0.0), (t, r, i)


def test_generate_step_chain_end_to_end(golden_dir):
    d = O.tiny_dims(False)
    g, batch = golden_batch(golden_dir, "llama")
    model = _model(d)
    inputs = _gen_inputs(g, batch)
    T = 10
    full = dict(do_sample=True, temperature=0.7, top_p=0.9, top_k=20, min_p=0.02, repetition_penalty=1.3)
    ids, lg = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, eos_token_id=[], seed=3, collect_logits=True, **full)
    _check_picks(ids, lg, full)
    again = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, eos_token_id=[], seed=3, **full)
    assert torch.equal(ids, again)
    greedy_pen = dict(do_sample=False, repetition_penalty=1.5)
    ids_g, lg_g = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, eos_token_id=[], collect_logits=True, **greedy_pen)
    _check_picks(ids_g, lg_g, greedy_pen)
    # top_k = 1 sampling = greedy, up to ties at the maximum (then any tied token may be drawn)
    greedy, lg0 = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, eos_token_id=[], collect_logits=True)
    k1, lg1 = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=True, temperature=0.7, top_p=0.9, top_k=1,
                                   eos_token_id=[], seed=5, collect_logits=True)
    lg1 = lg1.float()
    assert torch.equal(lg1.gather(-1, k1.t().unsqueeze(-1)).squeeze(-1), lg1.max(-1).values)
    ties = bool(((lg0.float() == lg0.float().max(-1, keepdim=True).values).sum(-1) > 1).any())
    assert ties or torch.equal(k1, greedy)
    # none of the new arguments: the same ids as today's call (and the "off" values route to today's kernels)
    for do_sample in (True, False):
        base = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=do_sample, temperature=0.7, top_p=0.9, seed=4)
        off = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=do_sample, temperature=0.7, top_p=0.9, seed=4,
                                   top_k=None, min_p=None, repetition_penalty=None)
        off2 = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=do_sample, temperature=0.7, top_p=0.9, seed=4,
                                    top_k=0, repetition_penalty=1.0)
        assert torch.equal(base, off) and torch.equal(base, off2)
    for bad in (dict(top_k=-2), dict(min_p=2.0), dict(repetition_penalty=0.0)):
        with pytest.raises(ValueError):
            model._generate_step(inputs, pad_token_id=0, max_new_tokens=2, **bad)


def test_text_only_penalty_reaches_prompt_tokens():
    """HF passes a text-only chat as input_ids, so the prompt (left padding included) is part of the penalty's history.  The
    unpenalised first pick is put into the prompt at a masked left-pad slot: the logits do not change, and with the prompt in
    the history a strong penalty moves the pick away from it; with an inputs_embeds prompt (empty history) it does not."""
    d = O.tiny_dims(False)
    model = _model(d)
    B, S = 2, 12
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(8, d.vocab, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    am[1, :3] = 0
    inputs = {"context_input_ids": ids, "context_attention_mask": am, "context_batch_start_positions": [], "batch_transcription_ids": [],
              "batch_features": None}
    plain, lg = model._generate_step(inputs, pad_token_id=0, max_new_tokens=1, do_sample=False, eos_token_id=[], collect_logits=True)
    a = int(plain[1, 0])
    ids2 = ids.clone()
    ids2[1, 0] = a                                              # masked slot: HF's input_ids hold it, the logits do not see it
    inputs2 = dict(inputs, context_input_ids=ids2)
    kw = dict(pad_token_id=0, max_new_tokens=4, do_sample=False, eos_token_id=[], repetition_penalty=50.0)
    no_prompt, lg2 = model._generate_step(inputs2, collect_logits=True, **kw)
    assert torch.equal(lg2[0], lg[0]) and int(no_prompt[1, 0]) == a
    with_prompt, lg3 = model._generate_step(inputs2, collect_logits=True, prompt_in_history=True, **kw)
    assert int(with_prompt[1, 0]) != a
    _check_picks(with_prompt, lg3, dict(do_sample=False, repetition_penalty=50.0), prompt=ids2)
    # the chat-level generate() passes text-only prompts that way
    seen = {}
    real = model._generate_step

    def spy(inputs, **k):
        seen.update(k)
        return real(inputs, **k)
    model._generate_step = spy
    model._setup_generation(tokenizer=ToyTokenizer(d.vocab))
    out = model.generate([{"role": "user", "content": "hello there"}], max_new_tokens=3, do_sample=True, top_k=5, repetition_penalty=1.2)
    assert seen["prompt_in_history"] is True and seen["top_k"] == 5 and seen["repetition_penalty"] == 1.2
    assert len(out.generated_ids) == 1


def test_orca_generate_accepts_chain_arguments():
    import copy
    import orca_oracle as R
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = copy.copy(O.tiny_dims(False))
    kg = 6
    o = R.OrcaDims(global_num_tokens=kg, local_downsample=4, local_kernel_size=5, global_cross_attn=True)
    w = R.init_weights(d, o, seed=11)
    d.prompt_size = kg
    batch = O.synthetic_batch(d, B=2, S_ctx=9, S_tgt=14, seed=4, pad=[3, 0])
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=4,
                        orca_local_kernel_size=5, orca_global_cross_attn=True)
    model = DeSTA25AudioModel(cfg, weights=w).eval()
    n_ctx = 9 + 3 + kg
    inputs = {"context_input_ids": batch["input_ids"][:, :n_ctx], "context_attention_mask": batch["attention_mask"][:, :n_ctx],
              "context_batch_start_positions": batch["batch_start_positions"], "batch_features": batch["batch_features"],
              "batch_transcription_ids": batch["batch_transcription_ids"]}
    kw = dict(pad_token_id=0, max_new_tokens=4, eos_token_id=[], collect_logits=True)
    full = dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=10, min_p=0.05, repetition_penalty=1.3)
    ids, lg = model._generate_step(inputs, seed=2, **full, **kw)
    assert ids.shape == (2, 4)
    _check_picks(ids, lg, full)
    ids_g, lg_g = model._generate_step(inputs, do_sample=False, repetition_penalty=2.0, **kw)
    _check_picks(ids_g, lg_g, dict(do_sample=False, repetition_penalty=2.0))


def test_predict_step_honours_yaml_generation_kwargs(golden_dir):
    from desta.trainer.desta_trainer import DeSTA25Trainer, TrainingArguments
    d = O.tiny_dims(False)
    g, batch = golden_batch(golden_dir, "llama")
    model = _model(d)
    full = dict(batch)
    full.update(_gen_inputs(g, batch))
    gk = {"max_new_tokens": 6, "do_sample": True, "temperature": 0.9, "top_p": 1.0, "top_k": 3, "repetition_penalty": 1.4}
    cfg = types.SimpleNamespace(model=types.SimpleNamespace(generation_kwargs=gk))
    tr = DeSTA25Trainer(model, cfg=cfg, args=TrainingArguments(max_steps=10))
    ids = tr._predict_step(full).cpu()
    want = model._generate_step(full, pad_token_id=0, max_new_tokens=6, do_sample=True, temperature=0.9, top_p=1.0, top_k=3,
                                repetition_penalty=1.4, seed=0).cpu()
    plain = model._generate_step(full, pad_token_id=0, max_new_tokens=6, do_sample=True, temperature=0.9, top_p=1.0, seed=0).cpu()
    assert torch.equal(ids, want) and not torch.equal(ids, plain)
    # the call-time generation_kwargs override the YAML's
    ids2 = tr._predict_step(full, {"top_k": 5, "repetition_penalty": 2.0}).cpu()
    want2 = model._generate_step(full, pad_token_id=0, max_new_tokens=6, do_sample=True, temperature=0.9, top_p=1.0, top_k=5,
                                 repetition_penalty=2.0, seed=0).cpu()
    assert torch.equal(ids2, want2)


def test_model_reads_llm_generation_config(tmp_path, golden_dir):
    import json
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = O.tiny_dims(False)
    (tmp_path / "generation_config.json").write_text(json.dumps({"do_sample": True, "temperature": 0.6, "top_p": 0.9, "top_k": 20}))
    cfg = cfg_from_dims(d)
    cfg.llm_model_id = str(tmp_path)
    model = DeSTA25AudioModel(cfg, weights=O.init_weights(d, seed=7))
    assert model.llm_generation_config["top_k"] == 20
    assert "top_k" not in json.dumps(model.config.to_dict())                # not written into DeSTA's own config.json
    kw = model.hf_generation_kwargs(temperature=0.7)
    assert kw["temperature"] == 0.7 and kw["top_k"] == 20 and kw["top_p"] == 0.9 and kw["do_sample"] is True
    assert _model(d).hf_generation_kwargs()["top_k"] == 50                   # no file: HF's global default
    g, batch = golden_batch(golden_dir, "llama")
    ids = model._generate_step(_gen_inputs(g, batch), pad_token_id=0, max_new_tokens=3, eos_token_id=[], seed=1, **kw)
    assert ids.shape[1] == 3
