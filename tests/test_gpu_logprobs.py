"""GPU: token log-probabilities — `desta_token_logprobs` against a float64 log-softmax, `score_batch` against the forward's loss,
the chat-level `score()` against hand-built rows and teacher-forced decode, and the trainer's `eval_token_accuracy`."""
import copy
import types

import pytest
import torch

import desta_oracle as O
from helpers import ToyTokenizer, cfg_from_dims, golden_batch

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


# ------------------------------------------------------------------------------------------------ kernel
def _rows(V, ld, seed=0):
    """Six bf16 rows [6, ld] (stride ld, entries >= V random: a kernel that reads them gets a wrong sum) and their labels."""
    g = torch.Generator().manual_seed(seed + V)
    x = (3.0 * torch.randn(6, ld, generator=g)).to(torch.bfloat16)
    lab = torch.randint(0, V, (6,), generator=g)
    lab[0] = -100                                                   # ignored
    top = float(x[:, :V].float().max()) + 2.0
    a, b, c = sorted(torch.randperm(V, generator=g)[:3].tolist())
    x[1, torch.randperm(V, generator=g)[: V // 7]] = NEG_INF        # -inf entries carry no mass ...
    lab[1] = b
    x[1, b] = top                                                   # ... and the label is the (single) maximum
    x[2, [a, b, c]] = top                                           # tie at the top, label = FIRST tied index -> argmax
    lab[2] = a
    x[3, [a, b, c]] = top                                           # same tie, label = a LATER tied index -> not the argmax
    lab[3] = c
    x[4] = (160.0 * torch.rand(ld, generator=g) - 80.0).to(torch.bfloat16)      # spans +-80: exp(x) without the maximum subtracted overflows
    x[4, a], x[4, c] = 80.0, -80.0
    # label = third largest entry: |logprob| stays O(1), so the fp32 result's own rounding (half an ulp: 4e-6 at |logprob| = 110,
    # which a label at the bottom of the range would give) does not eat the bound meant for the sum
    lab[4] = int(x[4, :V].float().argsort()[-3])
    x[5, torch.randperm(V, generator=g)[: V // 3]] = NEG_INF
    lab[5] = b
    x[5, b] = NEG_INF                                               # the label's own entry is -inf -> logprob -inf, not NaN
    return x, lab


def _reference(x, lab, V):
    """float64 log_softmax of the same bf16 values on the CPU, gathered at the label; first-index argmax."""
    xs = x[:, :V].double()
    ls = torch.log_softmax(xs, dim=-1)
    lp = torch.zeros(x.shape[0], dtype=torch.float64)
    top1 = torch.zeros(x.shape[0], dtype=torch.uint8)
    for r in range(x.shape[0]):
        t = int(lab[r])
        if 0 <= t < V:
            lp[r] = ls[r, t]
            first = int((xs[r] == xs[r].max()).nonzero()[0])
            top1[r] = 1 if first == t else 0
    return lp, top1


# ld padded to the next multiple of 8 (16-byte aligned row starts), and ld = V with V odd (row starts at every 2-byte phase)
KERNEL_CASES = [(V, V + 8 - V % 8) for V in (512, 4099, 128256, 151936)] + [(V, V) for V in (511, 4099, 128255, 151935)]


@pytest.mark.parametrize("V,ld", KERNEL_CASES)
def test_kernel_vs_float64(V, ld):
    from desta import _hip as H
    x, lab = _rows(V, ld)
    want, want_top = _reference(x, lab, V)
    xd, labd = x.cuda().contiguous(), lab.cuda()
    before = xd.clone()
    lp = torch.full((6,), 123.0, dtype=torch.float32, device="cuda")
    top = torch.full((6,), 9, dtype=torch.uint8, device="cuda")
    H.token_logprobs(xd, ld, labd, 6, V, lp, top)
    lp2 = torch.full((6,), 123.0, dtype=torch.float32, device="cuda")
    H.token_logprobs(xd, ld, labd, 6, V, lp2)                       # is_top1 = NULL
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.int16), before.view(torch.int16))          # the logits are read only
    got = lp.double().cpu()
    fin = torch.isfinite(want)
    err = (got[fin] - want[fin]).abs()
    print(f"V={V} ld={ld}: max |logprob - fp64| = {float(err.max()):.3e}  rows {err.tolist()}")
    assert fin.tolist() == [True, True, True, True, True, False]
    assert float(err.max()) <= 1e-5, err.tolist()
    assert float(got[0]) == 0.0 and float(got[5]) == NEG_INF                    # ignored row; -inf label entry (no NaN)
    assert top.cpu().tolist() == want_top.tolist() == [0, 1, 1, 0, 0, 0]
    assert torch.equal(lp, lp2)


def test_kernel_argument_checks():
    from desta import _hip as H
    V, ld = 512, 512
    x, lab = _rows(V, ld)
    xd, labd = x.cuda().contiguous(), lab.cuda()
    lp = torch.zeros(6, dtype=torch.float32, device="cuda")
    top = torch.zeros(6, dtype=torch.uint8, device="cuda")
    raw = H._token_logprobs
    st = H.stream()
    assert raw(0, ld, H.p(labd), 6, V, H.p(lp), H.p(top), st) == -1
    assert raw(H.p(xd), ld, 0, 6, V, H.p(lp), H.p(top), st) == -1
    assert raw(H.p(xd), ld, H.p(labd), 6, V, 0, H.p(top), st) == -1
    assert raw(H.p(xd), ld, H.p(labd), 0, V, H.p(lp), H.p(top), st) == -1
    assert raw(H.p(xd), ld, H.p(labd), -3, V, H.p(lp), H.p(top), st) == -1
    assert raw(H.p(xd), V - 1, H.p(labd), 6, V, H.p(lp), H.p(top), st) == -1
    with pytest.raises(RuntimeError, match="desta_token_logprobs"):
        H.token_logprobs(xd, V - 8, labd, 6, V, lp, top)
    # a label >= vocab cannot be checked on the host: the kernel treats it as ignored
    lab2 = lab.clone()
    lab2[1], lab2[2] = V, 2 ** 40
    lp.fill_(7.0)
    top.fill_(7)
    H.token_logprobs(xd, ld, lab2.cuda(), 6, V, lp, top)
    want, want_top = _reference(x, lab, V)
    assert lp[:3].cpu().tolist() == [0.0, 0.0, 0.0] and top[:3].cpu().tolist() == [0, 0, 0]
    assert abs(float(lp[3]) - float(want[3])) <= 1e-5 and int(top[3]) == int(want_top[3])


# ------------------------------------------------------------------------------------------------ score_batch
def _model(d, seed=7, **kw):
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    return DeSTA25AudioModel(cfg_from_dims(d, **kw), weights=O.init_weights(d, seed=seed))


def _check_score_batch(model, batch, golden_loss=None):
    model.train()                                                   # score_batch switches to eval itself and restores the flag
    sc = model.score_batch(**batch)
    assert model.training
    model.eval()
    ref = model(**batch).loss                                       # the same eval-mode forward, full token grid
    n = (batch["labels"][:, 1:] != -100).sum(dim=1)
    assert sc.n_tokens.cpu().tolist() == n.tolist() and sc.n_tokens.dtype == torch.int64
    assert sc.sum_logprob.dtype == torch.float32 and sc.top1_match.dtype == torch.int64
    mean_nll = -float(sc.sum_logprob.double().sum()) / float(n.sum())
    print(f"score_batch: -sum(logprob)/n = {mean_nll:.8f}, forward loss = {float(ref):.8f}, compact loss = {float(sc.loss):.8f}")
    assert abs(mean_nll - float(ref)) <= 1e-6 * abs(float(ref))     # same bf16 logits, only the fp32 reduction order differs
    assert abs(float(sc.loss) - float(ref)) <= 1e-6 * abs(float(ref))
    if golden_loss is not None:
        assert abs(float(sc.loss) - golden_loss) < 2e-3            # tests/test_gpu_model.py:35
    assert [t.numel() for t in sc.token_logprobs] == n.tolist()
    for b, t in enumerate(sc.token_logprobs):
        assert float(t.double().sum()) == pytest.approx(float(sc.sum_logprob[b]), rel=1e-6)
    assert bool((sc.top1_match <= sc.n_tokens).all()) and bool((sc.top1_match >= 0).all())
    # against the kept full-grid logits of the plain forward: log-softmax at the shifted labels, argmax hits
    lg = model(**batch, keep_logits=True).logits.float().cpu()      # [B, S, V]
    lsm = torch.log_softmax(lg.double(), dim=-1)
    for b in range(lg.shape[0]):
        pos = (batch["labels"][b, 1:] != -100).nonzero().flatten()
        tgt = batch["labels"][b, 1:][pos]
        want = lsm[b, pos, tgt]
        assert float((sc.token_logprobs[b].double().cpu() - want).abs().max()) <= 1e-5
        assert int(sc.top1_match[b]) == int((lg[b, pos].argmax(-1) == tgt).sum())
    again = model.score_batch(**batch)                              # deterministic: bit-identical
    assert torch.equal(again.sum_logprob, sc.sum_logprob) and torch.equal(again.top1_match, sc.top1_match) and torch.equal(again.loss, sc.loss)
    assert all(torch.equal(a, b) for a, b in zip(again.token_logprobs, sc.token_logprobs))
    none = dict(batch, labels=torch.full_like(batch["labels"], -100))
    z = model.score_batch(**none)
    B = batch["labels"].shape[0]
    assert z.sum_logprob.tolist() == [0.0] * B and z.n_tokens.tolist() == [0] * B and z.top1_match.tolist() == [0] * B
    assert float(z.loss) == 0.0 and [t.numel() for t in z.token_logprobs] == [0] * B
    return sc


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_score_batch_vs_forward_loss_golden(golden_dir, name):
    d = O.tiny_dims(name == "qwen3")
    g, batch = golden_batch(golden_dir, name)
    model = _model(d)
    _check_score_batch(model, batch, golden_loss=float(g["loss"]))
    # FP8 decode weights do not touch scoring (prefill kernels, bf16 weights)
    a = model.score_batch(**batch)
    model.set_decode_weights("fp8")
    b = model.score_batch(**batch)
    assert torch.equal(a.sum_logprob, b.sum_logprob)


def _orca_model():
    import orca_oracle as R
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = copy.copy(O.tiny_dims(False))
    kg = 6
    o = R.OrcaDims(global_num_tokens=kg, local_downsample=4, local_kernel_size=5, global_cross_attn=True)
    w = R.init_weights(d, o, seed=11)
    d.prompt_size = kg
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=4,
                        orca_local_kernel_size=5, orca_global_cross_attn=True)
    return DeSTA25AudioModel(cfg, weights=w), d


def test_score_batch_orca_hybrid(tmp_path):
    model, d = _orca_model()
    batch = O.synthetic_batch(d, B=2, S_ctx=9, S_tgt=14, seed=4, pad=[3, 0])
    _check_score_batch(model, batch)
    # score() on the ORCA branch: the one encoded audio's global and local tokens are repeated per answer row
    tok = ToyTokenizer(d.vocab)

    class Proc:
        def __call__(self, waves, sampling_rate=None, return_tensors=None):
            return types.SimpleNamespace(input_features=batch["batch_features"][:len(waves)].cuda())
    model.eval()._setup_generation(tokenizer=tok, processor=Proc(), vad=lambda w: True)
    msgs = [{"role": "user", "content": "Listen to <|AUDIO|> . Which animal barks ?", "audios": [{"audio": _wav(tmp_path), "text": "woof woof"}]}]
    out = model.score(msgs, CHOICES)
    _, inputs, _, _ = model._chat_inputs(msgs)
    tails, rows, index = _hand_rows(tok, inputs, CHOICES)
    sb = model.score_batch(**rows, audio_index=index)
    assert torch.equal(out.scores, sb.sum_logprob) and out.n_tokens.tolist() == [len(t) for t in tails]
    per_row = model.score_batch(**dict(rows, batch_features=inputs["batch_features"].expand(3, -1, -1).contiguous()))
    assert torch.allclose(per_row.sum_logprob, sb.sum_logprob, rtol=2e-2, atol=2e-2), (per_row.sum_logprob, sb.sum_logprob)


# ------------------------------------------------------------------------------------------------ score()
MSG_TEXT = [{"role": "system", "content": "Answer with one option."}, {"role": "user", "content": "Which animal barks ?"}]
CHOICES = ["a dog", "the cat on the mat", "bird"]
# Teacher-forced decode (KV-cached skinny GEMMs, one query row) against the prefill (tiled GEMMs, whole sequence) of the SAME
# tokens: both produce bf16 logits from bf16 activations, with different fp32 summation orders in every layer.  No existing test
# compares the two directly (tests/test_gpu_generate.py:53 compares decode with the fp32 oracle at 3e-2 relative L2, a norm over
# the whole vocabulary, not a per-token log-prob), so the gap was measured on the kernels this feature does not change: max
# |logprob(prefill) - logprob(decode)| over these messages and choices; the bound is twice that ("Token log-probabilities").
DECODE_GAP_MEASURED = 3.8648e-3                                    # profiles/r08_prefill_decode_logprob_gap.log (3.06e-3 with the audio)
DECODE_GAP_BOUND = 2 * DECODE_GAP_MEASURED


def _wav(tmp_path):
    import wave
    import numpy as np
    p = tmp_path / "clip.wav"
    with wave.open(str(p), "wb") as wv:
        wv.setnchannels(1); wv.setsampwidth(2); wv.setframerate(16000)
        wv.writeframes((0.1 * np.random.default_rng(0).standard_normal(16000) * 32767).astype("<i2").tobytes())
    return str(p)


def _hand_rows(tok, inputs, choices):
    """The rows `score()` must build, restated: context ‖ choice ids ‖ EOS, left-padded, labels on choice + EOS only, every
    row's audio span reading audio 0."""
    ctx = inputs["context_input_ids"][0].tolist()
    assert int(inputs["context_attention_mask"].min()) == 1
    tails = [tok.encode(c, add_special_tokens=False) + [tok.eos_token_id] for c in choices]
    S = len(ctx) + max(len(t) for t in tails)
    ids = torch.full((len(tails), S), tok.pad_token_id, dtype=torch.long)
    am = torch.zeros(len(tails), S, dtype=torch.long)
    lab = torch.full((len(tails), S), -100, dtype=torch.long)
    starts, trs, index = [], [], []
    for i, t in enumerate(tails):
        row = ctx + t
        ids[i, S - len(row):] = torch.tensor(row)
        am[i, S - len(row):] = 1
        lab[i, S - len(t):] = torch.tensor(t)
        for a, (_, s0) in enumerate(inputs["context_batch_start_positions"]):
            starts.append((i, int(s0) + S - len(row)))
            trs.append(inputs["batch_transcription_ids"][a])
            index.append(a)
    return tails, dict(input_ids=ids, attention_mask=am, labels=lab, batch_features=inputs["batch_features"], batch_transcription_ids=trs,
                       batch_start_positions=starts), index


@pytest.mark.parametrize("audio", [False, True])
def test_score_choices(golden_dir, tmp_path, audio):
    d = O.tiny_dims(False)
    g, _ = golden_batch(golden_dir, "llama")
    model = _model(d).eval()
    tok = ToyTokenizer(d.vocab)

    class Proc:                                                     # the tiny encoder takes 2 * 96 mel frames: hand over the golden's features
        def __call__(self, waves, sampling_rate=None, return_tensors=None):
            return types.SimpleNamespace(input_features=g["batch_features"][:len(waves)].cuda())
    model._setup_generation(tokenizer=tok, processor=Proc(), vad=lambda w: True)
    msgs = copy.deepcopy(MSG_TEXT)
    if audio:
        msgs[1] = {"role": "user", "content": "Listen to <|AUDIO|> . Which animal barks ?", "audios": [{"audio": _wav(tmp_path), "text": "woof woof"}]}
    calls = []
    real_encode = model._encode

    def spy(feats, n):
        calls.append((tuple(feats.shape), n))
        return real_encode(feats, n)
    model._encode = spy
    out = model.score(msgs, CHOICES)
    model._encode = real_encode
    assert calls == ([((1, d.n_mels, 2 * d.enc_T), 1)] if audio else [])        # one encoder pass for the one audio, not one per choice
    assert len({len(tok.encode(c)) for c in CHOICES}) == 3
    # == score_batch on the hand-built rows, exactly
    _, inputs, _, _ = model._chat_inputs(msgs)
    tails, rows, index = _hand_rows(tok, inputs, CHOICES)
    sb = model.score_batch(**rows, **(dict(audio_index=index) if audio else {}))
    assert torch.equal(out.scores, sb.sum_logprob) and torch.equal(out.n_tokens, sb.n_tokens)
    assert out.n_tokens.tolist() == [len(t) for t in tails]
    assert all(torch.equal(a, b) for a, b in zip(out.token_logprobs, sb.token_logprobs))
    assert out.best == int(out.scores.argmax()) and out.scores.shape == (3,)
    if audio:                                                       # one shared encoded audio == the same audio encoded once per row
        # (not bitwise: the encoder's / connector's GEMMs pick their tiling by row count, and bf16 outputs move in the last bit)
        per_row = model.score_batch(**dict(rows, batch_features=inputs["batch_features"].expand(3, -1, -1).contiguous()))
        assert torch.allclose(per_row.sum_logprob, sb.sum_logprob, rtol=2e-2, atol=2e-2), (per_row.sum_logprob, sb.sum_logprob)
    mean = model.score(msgs, CHOICES, normalize="mean")
    assert torch.equal(mean.scores, sb.sum_logprob / sb.n_tokens.float()) and mean.best == int(mean.scores.argmax())
    # teacher-forced decode of every choice: the KV-cached path gives the same token log-probs
    worst = 0.0
    for i, t in enumerate(tails):
        forced = torch.tensor([t])
        ids, lg = model._generate_step(inputs, pad_token_id=tok.pad_token_id, max_new_tokens=len(t), do_sample=False, eos_token_id=[],
                                       forced_tokens=forced, collect_logits=True)
        assert ids.cpu().tolist() == [t]
        want = torch.log_softmax(lg.float()[:, 0], dim=-1).cpu().gather(-1, forced.t()).squeeze(-1)
        worst = max(worst, float((out.token_logprobs[i].cpu() - want).abs().max()))
    print(f"score() vs teacher-forced decode (audio={audio}): max |d logprob| = {worst:.3e}")
    assert worst <= DECODE_GAP_BOUND, worst
    # generate() after the refactor: the same greedy ids as `_generate_step` on the same inputs
    gen = model.generate(msgs, do_sample=False, max_new_tokens=6)
    kw = {} if audio else dict(eos_token_id=[tok.eos_token_id, tok.convert_tokens_to_ids("<|eot_id|>")], prompt_in_history=True)
    direct = model._generate_step(inputs, pad_token_id=tok.pad_token_id, max_new_tokens=6, do_sample=False, **kw)
    assert gen.generated_ids == direct.cpu().tolist()
    if audio:
        assert [tuple(int(v) for v in s) for s in model._last_generate_inputs["context_batch_start_positions"]] == \
               [tuple(int(v) for v in s) for s in inputs["context_batch_start_positions"]]


# ------------------------------------------------------------------------------------------------ trainer
def test_evaluate_reports_token_accuracy(golden_dir):
    from desta.trainer.desta_trainer import DeSTA25Trainer, TrainingArguments
    d = O.tiny_dims(False)
    g, batch = golden_batch(golden_dir, "llama")
    model = _model(d, dropout=0.1)
    other = O.synthetic_batch(d, B=2, S_ctx=7, S_tgt=11, seed=9, pad=[0, 4])
    tr = DeSTA25Trainer(model, args=TrainingArguments(max_steps=10))
    m = tr.evaluate([batch, {"_empty_batch": True}, other])
    assert model.training
    model.eval()
    sc = [model.score_batch(**b) for b in (batch, other)]
    losses = [float(model(**b).loss) for b in (batch, other)]
    model.train()
    hit = sum(int(s.top1_match.sum()) for s in sc)
    n = sum(int(s.n_tokens.sum()) for s in sc)
    assert 0.0 <= m["eval_token_accuracy"] <= 1.0 and m["eval_token_accuracy"] == hit / n
    assert abs(m["eval_loss"] - sum(losses) / 2) <= 1e-6 * (sum(losses) / 2)
    assert {"eval_loss", "eval_ppl", "eval_token_accuracy"} <= set(m)
