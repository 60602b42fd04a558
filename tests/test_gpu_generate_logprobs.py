"""GPU: per-token log-probabilities and top-n alternatives of generate() — `desta_topk_logprobs` against a float64 log-softmax and a
stable descending sort, the decode loop against the logits it collected, the oracle, `score_batch`, and the chat-level fields."""
import math

import pytest
import torch

import desta_oracle as O
from helpers import ToyTokenizer, cfg_from_dims, golden_batch
from test_gpu_fp8_decode import _gen_inputs, _oracle

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
KERNEL_CASES = [(512, 512), (511, 511), (4099, 4104), (128256, 128256), (151935, 151935), (151936, 151944)]
TOP_NS = [1, 5, 20, 32]


def _bound(want):
    """1e-5 is the project's bound for `desta_token_logprobs`; 2^-23 |logprob| is half an fp32 ulp of the result itself."""
    return 1e-5 + 2.0 ** -23 * want.abs()


# ------------------------------------------------------------------------------------------------ kernel
def _rows(V, ld, n, seed=0):
    """Eight crafted bf16 rows [8, ld] (entries >= V random: a kernel that reads them gets a wrong sum or a wrong rank) + tokens."""
    g = torch.Generator().manual_seed(seed + V + 7 * n)
    x = (3.0 * torch.randn(8, ld, generator=g)).to(torch.bfloat16)                   # row 0: N(0, 3^2)
    tok = torch.randint(0, V, (8,), generator=g)
    x[1] = (160.0 * torch.rand(ld, generator=g) - 80.0).to(torch.bfloat16)          # row 1: +-80, exp overflows without the maximum subtracted
    tok[1] = int(x[1, :V].float().argsort()[-3])
    top = float(x[2, :V].float().max())
    free = max(1, n // 3)                                                           # row 2: n - free entries above a tie of free + 3 entries
    pick = torch.randperm(V, generator=g)[: n + 3]
    x[2, pick[: n - free]] = top + 2.0
    x[2, pick[n - free:]] = top + 1.0
    x[3] = 1.5                                                                      # row 3: every entry equal
    x[3, V:] = 9.0
    x[4] = -(x[4].float().abs() + 1.0).to(torch.bfloat16)                           # row 4: +0.0 and -0.0 are the top values
    zeros = torch.randperm(V, generator=g)[: n + 2].sort().values
    x[4, zeros[0::2]] = -0.0
    x[4, zeros[1::2]] = 0.0
    x[5, torch.randperm(V, generator=g)[: V // 3]] = NEG_INF                        # row 5: one third -inf
    tok[5] = int(x[5, :V].float().argmax())
    tok[6] = -1                                                                     # row 6: ignored
    x[7, torch.randperm(V, generator=g)[: V // 3]] = NEG_INF                        # row 7: the token's own entry is -inf
    x[7, int(tok[7])] = NEG_INF
    return x, tok


def _reference(x, V, n):
    """float64 log_softmax of the same bf16 values on the CPU; rank by a stable descending sort (lower index first among equals)."""
    xs = x[:, :V].double()
    ls = torch.log_softmax(xs, dim=-1)
    ids = torch.sort(xs, dim=-1, descending=True, stable=True).indices[:, :n]
    return ls, ids


def _run(H, xd, ld, tokd, rows, V, n, sentinel=True):
    """Outputs with one row behind `rows` that the kernel must leave alone."""
    lp = torch.full((rows + 1,), 123.0, dtype=torch.float32, device="cuda")
    ids = torch.full((rows + 1, n), 77, dtype=torch.int32, device="cuda")
    top = torch.full((rows + 1, n), 123.0, dtype=torch.float32, device="cuda")
    H.topk_logprobs(xd, ld, tokd, rows, V, n, lp if tokd is not None else None, ids, top)
    torch.cuda.synchronize()
    assert float(lp[rows]) == 123.0 and bool((ids[rows] == 77).all()) and bool((top[rows] == 123.0).all())
    return lp[:rows], ids[:rows], top[:rows]


def _check_rows(got_lp, got_ids, got_top, ls, want_ids, tok, live):
    """Rows `live`: ids exactly, finite log-probs within the bound, -inf where fp64 says -inf, no NaN."""
    got_ids, got_top, got_lp = got_ids.cpu().long(), got_top.double().cpu(), got_lp.double().cpu()
    worst = 0.0
    for r in live:
        assert got_ids[r].tolist() == want_ids[r].tolist(), (r, got_ids[r].tolist(), want_ids[r].tolist())
        for got, want in ((got_top[r], ls[r, want_ids[r]]), (got_lp[r:r + 1], ls[r, int(tok[r]):int(tok[r]) + 1])):
            assert not bool(torch.isnan(got).any())
            fin = torch.isfinite(want)
            assert torch.equal(got[~fin], want[~fin])
            if bool(fin.any()):
                ratio = ((got[fin] - want[fin]).abs() / _bound(want[fin])).max()
                worst = max(worst, float(ratio))
    return worst


@pytest.mark.parametrize("n", TOP_NS)
@pytest.mark.parametrize("V,ld", KERNEL_CASES)
def test_kernel_vs_float64(V, ld, n):
    from desta import _hip as H
    x, tok = _rows(V, ld, n)
    ls, want_ids = _reference(x, V, n)
    xd, tokd = x.cuda().contiguous(), tok.cuda()
    before = xd.clone()
    lp, ids, top = _run(H, xd, ld, tokd, 8, V, n)
    worst = _check_rows(lp, ids, top, ls, want_ids, tok, [0, 1, 2, 3, 4, 5, 7])
    print(f"V={V} ld={ld} n={n}: worst |logprob - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0
    # the crafted rows say what they were built to say
    assert float(x[2, want_ids[2, n - 1]]) == float(x[2, :V].float().sort(descending=True).values[n])      # n-th == (n+1)-th: a boundary tie
    assert want_ids[3].tolist() == list(range(n))
    assert torch.allclose(ls[3, :n], torch.full((n,), -math.log(V), dtype=torch.float64))
    assert bool((x[4, want_ids[4]].float() == 0.0).all()) and want_ids[4].tolist() == sorted(want_ids[4].tolist())
    # ignored row, -inf token entry
    assert float(lp[6]) == 0.0 and ids[6].tolist() == [-1] * n and top[6].tolist() == [0.0] * n
    assert float(lp[7]) == NEG_INF
    # the chosen token's value carries the bits of desta_token_logprobs; a rerun repeats every bit; the logits are read only
    lp_ref = torch.full((8,), 55.0, dtype=torch.float32, device="cuda")
    H.token_logprobs(xd, ld, tokd, 8, V, lp_ref)
    assert torch.equal(lp.view(torch.int32), lp_ref.view(torch.int32))
    lp2, ids2, top2 = _run(H, xd, ld, tokd, 8, V, n)
    assert torch.equal(lp2.view(torch.int32), lp.view(torch.int32)) and torch.equal(ids2, ids) and torch.equal(top2.view(torch.int32), top.view(torch.int32))
    assert torch.equal(xd.view(torch.int16), before.view(torch.int16))
    # independent of rows: row 5 alone, and without tokens (every row ranked, the ignored one too)
    lp1, ids1, top1 = _run(H, xd[5:], ld, tokd[5:6], 1, V, n)
    assert torch.equal(lp1.view(torch.int32), lp[5:6].view(torch.int32)) and torch.equal(ids1, ids[5:6]) and torch.equal(top1.view(torch.int32), top[5:6].view(torch.int32))
    _, ids3, top3 = _run(H, xd, ld, None, 8, V, n)
    live = [0, 1, 2, 3, 4, 5, 7]
    assert torch.equal(ids3[live], ids[live]) and torch.equal(top3[live].view(torch.int32), top[live].view(torch.int32))
    assert ids3[6].cpu().long().tolist() == want_ids[6].tolist()


def test_kernel_fewer_finite_entries_than_top_n():
    from desta import _hip as H
    V, n = 512, 5
    x = torch.full((1, V), NEG_INF, dtype=torch.bfloat16)
    x[0, [300, 17, 411]] = torch.tensor([1.0, 2.5, -3.0], dtype=torch.bfloat16)
    tok = torch.tensor([17])
    ls, want_ids = _reference(x, V, n)
    assert want_ids[0].tolist() == [17, 300, 411, 0, 1]                             # then the two lowest -inf indices
    lp, ids, top = _run(H, x.cuda(), V, tok.cuda(), 1, V, n)
    assert ids[0].tolist() == [17, 300, 411, 0, 1]
    assert top[0, 3:].tolist() == [NEG_INF, NEG_INF] and not bool(torch.isnan(top).any())
    assert _check_rows(lp, ids, top, ls, want_ids, tok, [0]) <= 1.0


def test_kernel_largest_decode_batch():
    from desta import _hip as H
    rows, V, ld, n = 64, 151936, 151944, 32
    g = torch.Generator().manual_seed(5)
    x = (3.0 * torch.randn(rows, ld, generator=g)).to(torch.bfloat16)
    tok = torch.randint(0, V, (rows,), generator=g)
    tok[9] = -1
    x[11, :V] = -2.0                                                                # all equal again, in the middle of the grid
    ls, want_ids = _reference(x, V, n)
    xd, tokd = x.cuda(), tok.cuda()
    lp, ids, top = _run(H, xd, ld, tokd, rows, V, n)
    worst = _check_rows(lp, ids, top, ls, want_ids, tok, [r for r in range(rows) if r != 9])
    print(f"rows=64 V={V} n=32: worst |logprob - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert ids[9].tolist() == [-1] * n and float(lp[9]) == 0.0
    lp_ref = torch.zeros(rows, dtype=torch.float32, device="cuda")
    H.token_logprobs(xd, ld, tokd, rows, V, lp_ref)
    assert torch.equal(lp.view(torch.int32), lp_ref.view(torch.int32))


def test_kernel_argument_checks():
    from desta import _hip as H
    V, ld, n = 512, 512, 5
    x, tok = _rows(V, ld, n)
    xd, tokd = x.cuda().contiguous(), tok.cuda()
    lp = torch.zeros(8, dtype=torch.float32, device="cuda")
    ids = torch.zeros(8, n, dtype=torch.int32, device="cuda")
    top = torch.zeros(8, n, dtype=torch.float32, device="cuda")
    raw, st, p = H._topk_logprobs, H.stream(), H.p
    assert raw(0, ld, p(tokd), 8, V, n, p(lp), p(ids), p(top), st) == -1            # NULL logits
    assert raw(p(xd), ld, p(tokd), 0, V, n, p(lp), p(ids), p(top), st) == -1        # rows <= 0
    assert raw(p(xd), ld, p(tokd), -2, V, n, p(lp), p(ids), p(top), st) == -1
    assert raw(p(xd), V - 1, p(tokd), 8, V, n, p(lp), p(ids), p(top), st) == -1     # ld < vocab
    assert raw(p(xd), ld, p(tokd), 8, V, -1, p(lp), p(ids), p(top), st) == -1       # top_n outside 0..32
    assert raw(p(xd), ld, p(tokd), 8, V, 33, p(lp), p(ids), p(top), st) == -1
    assert raw(p(xd), ld, p(tokd), 8, V, n, 0, p(ids), p(top), st) == -1            # tokens without token_logprob
    assert raw(p(xd), ld, 0, 8, V, n, p(lp), p(ids), p(top), st) == -1              # token_logprob without tokens
    assert raw(p(xd), ld, p(tokd), 8, V, n, p(lp), 0, p(top), st) == -1             # top_n > 0 without top_ids / top_logprobs
    assert raw(p(xd), ld, p(tokd), 8, V, n, p(lp), p(ids), 0, st) == -1
    with pytest.raises(RuntimeError, match="desta_topk_logprobs"):
        H.topk_logprobs(xd, V - 8, tokd, 8, V, n, lp, ids, top)
    torch.cuda.synchronize()
    assert float(lp.abs().sum()) == 0.0 and int(ids.abs().sum()) == 0               # a refused call launched nothing
    ls, want_ids = _reference(x, V, n)
    H.topk_logprobs(xd, ld, None, 8, V, n, None, ids, top)                          # tokens = NULL with top_n = 5
    assert ids.cpu().long().tolist() == want_ids.tolist()
    H.topk_logprobs(xd, ld, tokd, 8, V, 0, lp, None, None)                          # top_n = 0 with NULL top pointers
    lp_ref = torch.zeros(8, dtype=torch.float32, device="cuda")
    H.token_logprobs(xd, ld, tokd, 8, V, lp_ref)
    assert torch.equal(lp.view(torch.int32), lp_ref.view(torch.int32))
    tok2 = tok.clone()                                                              # a token >= vocab: ignored like a negative one
    tok2[0] = V
    H.topk_logprobs(xd, ld, tok2.cuda(), 8, V, n, lp, ids, top)
    assert float(lp[0]) == 0.0 and ids[0].tolist() == [-1] * n and top[0].tolist() == [0.0] * n


# ------------------------------------------------------------------------------------------------ decode loop
_MODELS = {}


def _setup(golden_dir, name):
    """One model, its inputs and one plain greedy run per tiny golden, shared by the tests below (none of them changes it)."""
    if name not in _MODELS:
        from desta.models.modeling_desta25 import DeSTA25AudioModel
        d = O.tiny_dims(name == "qwen3")
        g, batch = golden_batch(golden_dir, name)
        w = O.init_weights(d, seed=7)
        model = DeSTA25AudioModel(cfg_from_dims(d), weights=w)
        inputs = _gen_inputs(g, batch)
        ids0, lg0 = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True, eos_token_id=[])
        _MODELS[name] = (model, d, w, g, batch, inputs, ids0, lg0)
    return _MODELS[name]


def _check_against_logits(lp, ids, logits, n, ranks=True):
    """`lp` against float64 log_softmax of the run's own collected logits [T, B, V]; -> worst error / bound."""
    ls = torch.log_softmax(logits.double().cpu(), dim=-1).permute(1, 0, 2)          # [B, T, V]
    B, T, V = ls.shape
    assert lp.token_logprobs.shape == (B, T) and lp.top_ids.shape == (B, T, n) and lp.top_logprobs.shape == (B, T, n)
    assert lp.token_logprobs.dtype == torch.float32 and lp.top_ids.dtype == torch.int32 and lp.top_logprobs.dtype == torch.float32
    want_tok = ls.gather(-1, ids.cpu().unsqueeze(-1)).squeeze(-1)
    worst = float(((lp.token_logprobs.double().cpu() - want_tok).abs() / _bound(want_tok)).max())
    if ranks:
        want_ids = torch.sort(logits.double().cpu().permute(1, 0, 2), dim=-1, descending=True, stable=True).indices[..., :n]
        assert torch.equal(lp.top_ids.cpu().long(), want_ids)
        want_top = ls.gather(-1, want_ids)
        worst = max(worst, float(((lp.top_logprobs.double().cpu() - want_top).abs() / _bound(want_top)).max()))
    return worst


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_greedy_logprobs_match_collected_logits(golden_dir, name):
    from desta import _hip as H
    from desta.models.modeling_desta25 import TokenLogprobs
    model, d, w, g, batch, inputs, ids0, lg0 = _setup(golden_dir, name)
    c0 = H.TOPK_LOGPROBS_CALLS
    ids_n, lg_n = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True, eos_token_id=[])
    assert H.TOPK_LOGPROBS_CALLS == c0                                              # logprobs=None: not one launch
    ids, lg, lp = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True, eos_token_id=[], logprobs=5)
    assert H.TOPK_LOGPROBS_CALLS - c0 == 10                                         # exactly one per step
    assert isinstance(lp, TokenLogprobs)
    assert torch.equal(ids, ids0) and torch.equal(ids_n, ids0)
    assert torch.equal(lg.view(torch.int16), lg0.view(torch.int16)) and torch.equal(lg_n.view(torch.int16), lg0.view(torch.int16))
    worst = _check_against_logits(lp, ids, lg, 5)
    print(f"{name}: greedy, worst |logprob - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(lp.top_ids[:, :, 0].long(), ids)                            # greedy: the chosen token leads its own ranking
    assert torch.equal(lp.top_logprobs[:, :, 0], lp.token_logprobs)
    only, lp2 = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, eos_token_id=[], logprobs=0)
    assert torch.equal(only, ids0) and lp2.top_ids.shape == (ids0.shape[0], 10, 0) and torch.equal(lp2.token_logprobs, lp.token_logprobs)
    with pytest.raises(ValueError, match="33"):
        model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, eos_token_id=[], logprobs=33)


def test_sampling_logprobs_are_of_the_raw_logits(golden_dir):
    model, d, w, g, batch, inputs, ids0, lg0 = _setup(golden_dir, "llama")
    kw = dict(pad_token_id=0, max_new_tokens=10, do_sample=True, temperature=0.7, top_k=20, repetition_penalty=1.3, seed=3, eos_token_id=[],
              collect_logits=True)
    ids_s, lg_s = model._generate_step(inputs, **kw)
    ids, lg, lp = model._generate_step(inputs, logprobs=5, **kw)
    assert torch.equal(ids, ids_s) and torch.equal(lg.view(torch.int16), lg_s.view(torch.int16))
    assert not torch.equal(ids, ids0)                                               # the draw left the greedy path: ranks and tokens differ
    worst = _check_against_logits(lp, ids, lg, 5)
    print(f"sampling: worst |logprob - fp64 of the raw logits| / bound = {worst:.3f}")
    assert worst <= 1.0


def test_eos_is_scored_and_the_padding_is_not(golden_dir):
    model, d, w, g, batch, inputs, ids0, lg0 = _setup(golden_dir, "llama")
    _, lp0 = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, eos_token_id=[], logprobs=5)
    eos = int(ids0[0, 2])
    ids, lp = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, eos_token_id=[eos], logprobs=5)
    rows0 = ids0.cpu().tolist()
    ends = [row.index(eos) + 1 if eos in row else 10 for row in rows0]             # columns each row scores: up to and including its EOS
    assert ends[0] <= 3
    n_new = max(ends)
    assert ids.shape[1] == n_new and lp.token_logprobs.shape[1] == n_new and lp.top_ids.shape[1] == n_new
    for b, e in enumerate(ends):
        assert ids[b, :e].cpu().tolist() == rows0[b][:e] and ids[b, e:].cpu().tolist() == [0] * (n_new - e)
        assert torch.equal(lp.token_logprobs[b, :e], lp0.token_logprobs[b, :e]) and torch.equal(lp.top_ids[b, :e], lp0.top_ids[b, :e])
        assert torch.equal(lp.top_logprobs[b, :e], lp0.top_logprobs[b, :e])
        assert float(lp.token_logprobs[b, e - 1]) != 0.0                            # the EOS step itself (or the row's last) is scored
        assert bool((lp.token_logprobs[b, e:] == 0.0).all()) and bool((lp.top_ids[b, e:] == -1).all()) and bool((lp.top_logprobs[b, e:] == 0.0).all())


# Measured on the MI355X: max |token_logprob - fp64 log_softmax(oracle logits)[token]| over 10 teacher-forced steps of the golden
# batch; the bound is three times the measurement (the project's convention).
ORACLE_GAP_MEASURED = {"llama": 6.5324e-3, "qwen3": 6.1336e-3}


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_logprobs_vs_oracle(golden_dir, name):
    """Against the fp32 oracle, which shares no code with the library, teacher-forced on the oracle's own greedy tokens."""
    model, d, w, g, batch, inputs, ids0, lg0 = _setup(golden_dir, name)
    ref_ids, _ = _oracle(w, d, g, batch, 10)
    lo = _oracle(w, d, g, batch, 10, forced=ref_ids)[1]                             # [T, B, V]
    ids, lp = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, forced_tokens=ref_ids, eos_token_id=[], logprobs=5)
    assert ids.cpu().tolist() == ref_ids.tolist()
    want = torch.log_softmax(lo.double(), dim=-1).permute(1, 0, 2).gather(-1, ref_ids.unsqueeze(-1)).squeeze(-1)
    gap = float((lp.token_logprobs.double().cpu() - want).abs().max())
    print(f"{name}: max |token_logprob - oracle| = {gap:.4e}")
    assert gap <= 3 * ORACLE_GAP_MEASURED[name], gap


@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_sum_agrees_with_score_batch(golden_dir, name):
    model, d, w, g, batch, inputs, ids0, lg0 = _setup(golden_dir, name)
    ids, lp = model._generate_step(inputs, pad_token_id=0, max_new_tokens=10, do_sample=False, eos_token_id=[], logprobs=0)
    new = ids.cpu()
    ctx, am = inputs["context_input_ids"], inputs["context_attention_mask"]
    rows = dict(input_ids=torch.cat([ctx, new], dim=1), attention_mask=torch.cat([am, torch.ones_like(new)], dim=1),
                labels=torch.cat([torch.full_like(ctx, -100), new], dim=1), batch_features=inputs["batch_features"],
                batch_transcription_ids=inputs["batch_transcription_ids"], batch_start_positions=inputs["context_batch_start_positions"])
    sc = model.score_batch(**rows)
    assert sc.n_tokens.tolist() == [10] * new.shape[0]
    got, want = lp.token_logprobs.sum(dim=1).cpu(), sc.sum_logprob.cpu()
    print(f"{name}: sum of log-probs, generate {got.tolist()} score_batch {want.tolist()}")
    assert torch.allclose(got, want, rtol=2e-2, atol=2e-2), (got, want)


def test_logprobs_with_chunked_prefill_and_fp8_decode(golden_dir):
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = O.tiny_dims(False)
    g, batch = golden_batch(golden_dir, "llama")
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=O.init_weights(d, seed=7))
    model.set_prefill_chunk(16)
    model.set_decode_weights("fp8")
    ids, lg, lp = model._generate_step(_gen_inputs(g, batch), pad_token_id=0, max_new_tokens=10, do_sample=False, collect_logits=True,
                                       eos_token_id=[], logprobs=5)
    worst = _check_against_logits(lp, ids, lg, 5)
    print(f"chunked prefill + fp8 decode: worst |logprob - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert torch.equal(lp.top_ids[:, :, 0].long(), ids)


def test_chat_generate_logprob_fields(golden_dir):
    model, d, w, g, batch, inputs, ids0, lg0 = _setup(golden_dir, "llama")

    class Tok(ToyTokenizer):
        def convert_ids_to_tokens(self, i):
            return f"tok{int(i)}"
    tok = Tok(vocab_size=d.vocab)
    model._setup_generation(tokenizer=tok, processor=object())
    msgs = [[{"role": "user", "content": "hi there"}], [{"role": "user", "content": "a somewhat longer question , please"}]]
    plain = model.generate(msgs, do_sample=False, max_new_tokens=6)
    assert plain.token_logprobs is None and plain.top_logprobs is None and plain.sum_logprob is None
    with pytest.raises(ValueError, match="True"):
        model.generate(msgs, do_sample=False, max_new_tokens=6, logprobs=True)
    tok._fixed["<|eot_id|>"] = plain.generated_ids[0][1]                            # row 0's second token ends a turn from now on
    eos = {tok.eos_token_id, plain.generated_ids[0][1]}
    out = model.generate(msgs, do_sample=False, max_new_tokens=6, logprobs=2)
    ends = [next((i + 1 for i, t in enumerate(r) if t in eos), len(r)) for r in out.generated_ids]
    assert ends[0] <= 2 and out.generated_ids[0][:ends[0]] == plain.generated_ids[0][:ends[0]]
    assert len(out.token_logprobs) == len(out.top_logprobs) == len(out.sum_logprob) == 2
    for b, e in enumerate(ends):
        assert len(out.token_logprobs[b]) == e and len(out.top_logprobs[b]) == e   # cut behind the first EOS, inclusive
        assert all(isinstance(v, float) and v < 0.0 for v in out.token_logprobs[b])
        assert out.sum_logprob[b] == pytest.approx(sum(out.token_logprobs[b]), abs=1e-6)
        for t, alts in enumerate(out.top_logprobs[b]):
            assert len(alts) == 2 and alts[0][2] >= alts[1][2]
            assert all(s == f"tok{i}" for i, s, _ in alts)
            assert alts[0][0] == out.generated_ids[b][t] and alts[0][2] == out.token_logprobs[b][t]     # greedy
    model._setup_generation(tokenizer=ToyTokenizer(vocab_size=d.vocab), processor=object())               # a tokenizer without token strings
    bare = model.generate(msgs[:1], do_sample=False, max_new_tokens=3, logprobs=1)
    assert all(s is None for row in bare.top_logprobs for alts in row for _, s, _ in alts)
