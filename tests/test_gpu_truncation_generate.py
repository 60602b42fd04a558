"""GPU: typical_p / epsilon_cutoff / eta_cutoff through the decode loops of the tiny model (tests/helpers.py): every token a
truncated sampling call emits lies inside the float64 reference interval of ITS step's collected logits
(tests/truncation_reference.py on top of tests/sampling_reference.py), draft-and-verify under scope "all" emits the plain loop's
tokens bit for bit, guidance and constraints keep acting in front of the truncated pick, do_sample=False ignores the three, and
calls without them reach the kernels they always reached."""
import types

import numpy as np
import pytest
import torch

import constraints_reference as CR
import desta_oracle as O
import guidance_reference as GR
import sampling_reference as SR
import truncation_reference as TR
from helpers import cfg_from_dims, golden_batch

pytestmark = pytest.mark.gpu

T = 24
KW = dict(pad_token_id=0, max_new_tokens=T, eos_token_id=[])
TRUNC = dict(typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=6e-3)
_S = {}


def _setup(golden_dir):
    if not _S:
        from desta.models.modeling_desta25 import DeSTA25AudioModel
        d = O.tiny_dims(False)
        g, batch = golden_batch(golden_dir, "llama")
        model = DeSTA25AudioModel(cfg_from_dims(d), weights=O.init_weights(d, seed=7))
        n_ctx = int(g["gen_ctx_len"])
        audio = {"context_input_ids": batch["input_ids"][:, :n_ctx], "context_attention_mask": batch["attention_mask"][:, :n_ctx],
                 "context_batch_start_positions": batch["batch_start_positions"], "batch_features": batch["batch_features"],
                 "batch_transcription_ids": batch["batch_transcription_ids"]}
        _S.update(model=model, d=d, g=g, batch=batch, audio=audio)
    return types.SimpleNamespace(**_S)


def _check_steps(ids, lg, seed, case, hist0=None):
    """every emitted token against the reference of its own step's logits -> (steps x rows checked, largest ratio).  A (step, row)
    is judged when the reference holds its margins there (a condition on the logits, evaluated on the reference alone)."""
    ids, lg = ids.cpu(), lg.cpu()
    n_new, B, V = lg.shape
    judged, worst = 0, 0.0
    for t in range(n_new):
        hist = None
        if case.get("penalty", 1.0) != 1.0:
            hist = ids[:, :t] if hist0 is None else torch.cat([hist0, ids[:, :t]], dim=1)
        ref = TR.Reference(dict(case, V=V), lg[t], hist)
        ok = TR.margins_hold(ref.margins) & (ref.margin_top_p >= SR.MARGIN) & (ref.margin_min_p >= SR.MARGIN)
        tok = ids[:, t].numpy()
        u = SR.u24_rows(seed, t, B)
        ratio = ref.ratio(tok, u)
        for b in np.flatnonzero(ok):
            assert bool(ref.kept[b, tok[b]]), (t, b, int(tok[b]), int(ref.kept[b].sum()))
            assert float(ratio[b]) <= 1.0, (t, b, float(ratio[b]))
            worst = max(worst, float(ratio[b]))
        judged += int(ok.sum())
    return judged, worst


@pytest.mark.parametrize("setting", ["tail", "all"])
def test_sampled_tokens_lie_in_the_reference_interval_and_speculation_repeats_them(golden_dir, setting):
    from desta import _hip as H
    S = _setup(golden_dir)
    seed = 11
    extra = dict(temperature=0.9, top_p=1.0) if setting == "tail" else dict(temperature=0.8, top_k=40, top_p=0.95, min_p=0.01, repetition_penalty=1.2)
    case = dict(kernel="chain", T=extra["temperature"], top_k=extra.get("top_k", 0), top_p=extra["top_p"], min_p=extra.get("min_p", 0.0),
                penalty=extra.get("repetition_penalty", 1.0), **TRUNC)
    n0, r0 = H.SAMPLE_TRUNCATED_CALLS, H.SAMPLE_ROWS_CALLS
    ids, lg = S.model._generate_step(S.audio, do_sample=True, seed=seed, collect_logits=True, **extra, **TRUNC, **KW)
    assert H.SAMPLE_TRUNCATED_CALLS - n0 == T and H.SAMPLE_ROWS_CALLS == r0 and ids.shape[1] == T     # one launch per step, the chain's
    judged, worst = _check_steps(ids, lg, seed, case)
    assert judged >= 0.75 * ids.numel(), (judged, ids.numel())
    print(f"\n{setting}: {judged} of {ids.numel()} draws judged, largest ratio {worst:.3g}", end="")
    # the truncation is visible: the same call without it draws other tokens from the same first-step logits onwards
    plain = S.model._generate_step(S.audio, do_sample=True, seed=seed, **extra, **KW)
    assert not torch.equal(plain, ids)
    # draft-and-verify, scope "all": the grouped call carries the three values
    drafts = torch.full((ids.shape[0], T), -1, dtype=torch.int64)
    drafts[:, :] = ids.cpu()
    drafts[:, 3::4] = (drafts[:, 3::4] + 1) % S.d.vocab
    drafts[0, 6] = -1
    S.model.set_speculative(3, scope="all")
    try:
        n0 = H.SAMPLE_TRUNCATED_CALLS
        ids_s, lg_s = S.model._generate_step(S.audio, do_sample=True, seed=seed, collect_logits=True, draft_tokens=drafts, **extra, **TRUNC, **KW)
        st = S.model.llm.spec_stats
        assert st["path"] == "speculative" and st["drafts_accepted"] > 0
        assert H.SAMPLE_TRUNCATED_CALLS - n0 == 1 + st["verify_steps"]
        assert torch.equal(ids_s, ids)
        S.model.set_speculative(3, scope="greedy")                                  # sampled calls keep to the plain loop
        ids_g = S.model._generate_step(S.audio, do_sample=True, seed=seed, draft_tokens=drafts, **extra, **TRUNC, **KW)
        assert S.model.llm.spec_stats["path"] == "plain" and S.model.llm.spec_stats["reason"] == "do_sample" and torch.equal(ids_g, ids)
    finally:
        S.model.set_speculative(None)


def test_guided_constrained_and_truncated(golden_dir):
    from desta import _hip as H
    S = _setup(golden_dir)
    inputs2 = GR.guided_inputs(S.g, S.batch)
    kw = dict(do_sample=True, seed=5, temperature=0.9, top_p=1.0, guidance_scale=1.5, **KW)
    plain = S.model._generate_step(inputs2, **TRUNC, **kw).cpu()
    p = plain.tolist()
    s = dict(bad_words_ids=[p[0][2:4], [p[1][1]]], suppress_tokens=[p[0][3], p[1][0]], begin_suppress_tokens=[p[0][0]], no_repeat_ngram_size=2)
    assert any(CR.violations(r, S.d.vocab, **s) for r in p)
    c0, k0, n0 = H.CFG_SCORES_CALLS, H.CONSTRAINT_CALLS, H.SAMPLE_TRUNCATED_CALLS
    ids = S.model._generate_step(inputs2, **s, **TRUNC, **kw)
    assert H.CFG_SCORES_CALLS - c0 == T == H.CONSTRAINT_CALLS - k0 == H.SAMPLE_TRUNCATED_CALLS - n0 and ids.shape == (2, T)
    for r in ids.cpu().tolist():
        assert CR.violations(r, S.d.vocab, **s) == []


def test_greedy_ignores_them_and_calls_without_them_are_unchanged(golden_dir):
    from desta import _hip as H
    S = _setup(golden_dir)
    n0 = H.SAMPLE_TRUNCATED_CALLS
    a = S.model._generate_step(S.audio, do_sample=False, **KW)
    b = S.model._generate_step(S.audio, do_sample=False, **TRUNC, **KW)
    c = S.model._generate_step(S.audio, do_sample=False, repetition_penalty=1.3, **KW)
    d = S.model._generate_step(S.audio, do_sample=False, repetition_penalty=1.3, **TRUNC, **KW)
    assert torch.equal(a, b) and torch.equal(c, d)
    off = dict(typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    for extra in (dict(temperature=0.7, top_p=0.9), dict(temperature=0.7, top_p=0.9, top_k=20, min_p=0.02)):
        x = S.model._generate_step(S.audio, do_sample=True, seed=3, **extra, **KW)
        y = S.model._generate_step(S.audio, do_sample=True, seed=3, **extra, **off, **KW)
        z = S.model._generate_step(S.audio, do_sample=True, seed=3, **extra, typical_p=None, epsilon_cutoff=None, eta_cutoff=None, **KW)
        assert torch.equal(x, y) and torch.equal(x, z)
    assert H.SAMPLE_TRUNCATED_CALLS == n0
    for bad, name in ((dict(typical_p=1.5), "typical_p"), (dict(epsilon_cutoff=-0.1), "epsilon_cutoff"), (dict(eta_cutoff=1.0), "eta_cutoff")):
        with pytest.raises(ValueError, match=f"`{name}` has to be a float > 0 and < 1"):
            S.model._generate_step(S.audio, do_sample=True, **bad, **KW)
