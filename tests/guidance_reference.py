"""Reference side of the classifier-free guidance tests (`desta_cfg_scores_bf16`, `generate(guidance_scale=)`): float64 guided scores of
bf16 rows, the per-element bound the kernel is held to, the negative-message cases, and the teacher-forced oracle of a 2 Bc batch.

The bound (derived, not tuned).  For one element write Lc, Lu for the exact log-probabilities of the bf16 inputs, g for the scale
(1.5, 2, 3, 4 and 1 in the tests: exact in fp32) and R = g (Lc - Lu) + Lu for the exact guided score.  The kernel forms

    lc = Lc + ec,  lu = Lu + eu       |ec| <= bc = 1e-5 + 2^-23 |Lc|,  |eu| <= bu = 1e-5 + 2^-23 |Lu|
                                      (the project's bound for desta_token_logprobs / desta_topk_logprobs,
                                       tests/test_gpu_generate_logprobs.py::_bound; the kernel shares their code)
    d = fl(lc - lu) = (lc - lu)(1 + d1)
    t = fl(g d)     = g d (1 + d2)
    o = fl(t + lu)  = (t + lu)(1 + d3)         |d1|, |d2|, |d3| <= u = 2^-24   (fp32, round to nearest)
    out = bf16(o)   = o (1 + d4)               |d4| <= 2^-8                    (half a bf16 ulp)

With D = |Lc - Lu| and E = bc + bu:  |lc - lu| <= D + E, so
    |t + lu - R|  <=  g E + bu + g (D + E)(2u + u^2)                     =: a
    |o - R|       <=  a + u (|R| + a)                                    =: e32
    |out - R|     <=  e32 + 2^-8 (|R| + e32)
No term is measured.  A -inf entry of either input gives -inf exactly (the kernel's documented rule) and is compared exactly."""
import torch

import desta_oracle as O

NEG_INF = float("-inf")
U32 = 2.0 ** -24


def guided_scores_fp64(cond: torch.Tensor, uncond: torch.Tensor, g: float):
    """-> (R, Lc, Lu) in float64 from bf16-valued rows [..., V]; R is -inf where either input is -inf."""
    c, u = cond.double(), uncond.double()
    Lc, Lu = torch.log_softmax(c, dim=-1), torch.log_softmax(u, dim=-1)
    dead = torch.isinf(c) | torch.isinf(u)
    R = g * (torch.where(dead, torch.zeros_like(Lc), Lc) - torch.where(dead, torch.zeros_like(Lu), Lu)) + torch.where(dead, torch.zeros_like(Lu), Lu)
    return torch.where(dead, torch.full_like(R, NEG_INF), R), Lc, Lu


def guided_bound(R, Lc, Lu, g: float):
    """The module docstring's bound, element by element (meaningful where R is finite)."""
    dead = torch.isinf(R)
    Lc, Lu, R = (torch.where(dead, torch.zeros_like(x), x) for x in (Lc, Lu, R))
    bc, bu = 1e-5 + 2.0 ** -23 * Lc.abs(), 1e-5 + 2.0 ** -23 * Lu.abs()
    D, E = (Lc - Lu).abs(), bc + bu
    a = g * E + bu + g * (D + E) * (2 * U32 + U32 * U32)
    e32 = a + U32 * (R.abs() + a)
    return e32 + 2.0 ** -8 * (R.abs() + e32)


def check_scores(got_bf16: torch.Tensor, cond: torch.Tensor, uncond: torch.Tensor, g: float) -> float:
    """Kernel output against the fp64 reference: -inf exactly where the rule says so, no NaN, every finite element within the
    bound.  -> worst |got - R| / bound."""
    R, Lc, Lu = guided_scores_fp64(cond, uncond, g)
    got = got_bf16.double().cpu()
    assert not bool(torch.isnan(got).any())
    dead = torch.isinf(R)
    assert bool((got[dead] == NEG_INF).all()) and bool(torch.isfinite(got[~dead]).all())
    ratio = (got - R).abs()[~dead] / guided_bound(R, Lc, Lu, g)[~dead]
    return float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------ negative messages
LOC = "<|AUDIO|>"
NEGATIVE_CASES = {
    # name: (messages, expected negative)
    "single conversation": (
        [{"role": "system", "content": "Listen."},
         {"role": "user", "content": f"What is said in {LOC}?", "audios": [{"audio": "a.wav", "text": "hi"}]}],
        [{"role": "system", "content": "Listen."}, {"role": "user", "content": "What is said in ?"}]),
    "list of conversations": (
        [[{"role": "user", "content": f"{LOC} first", "audios": [{"audio": "a.wav", "text": None}]}],
         [{"role": "user", "content": f"second {LOC}", "audios": [{"audio": "b.wav", "text": ""}]}]],
        [[{"role": "user", "content": " first"}], [{"role": "user", "content": "second "}]]),
    "two audios in one message": (
        [[{"role": "user", "content": f"Compare {LOC} with {LOC} please", "audios": [{"audio": "a.wav"}, {"audio": "b.wav"}]}]],
        [[{"role": "user", "content": "Compare  with  please"}]]),
    "a message without audios": (
        [[{"role": "user", "content": "no clip here"}, {"role": "assistant", "content": "ok", "note": 7},
          {"role": "user", "content": f"now {LOC}", "audios": [{"audio": "c.wav", "text": "x"}]}]],
        [[{"role": "user", "content": "no clip here"}, {"role": "assistant", "content": "ok", "note": 7}, {"role": "user", "content": "now "}]]),
}


# ------------------------------------------------------------------------------------------------ 2 Bc batch and its oracle
def guided_inputs(g, batch, shorten_row: int = 0, shorten_by: int = 5):
    """`_generate_step` inputs of 2 Bc rows from a tiny golden: the golden's context rows (with their audio spans) are the
    conditional rows; the negatives are the same context ids WITHOUT spans (the placeholders embed as plain tokens), and negative
    `shorten_row` loses its first `shorten_by` tokens and is left-padded, so the kv_start values of the two halves differ."""
    n_ctx = int(g["gen_ctx_len"])
    ids, am = batch["input_ids"][:, :n_ctx], batch["attention_mask"][:, :n_ctx]
    neg_ids, neg_am = ids.clone(), am.clone()
    live = ids[shorten_row][am[shorten_row] == 1][shorten_by:]
    neg_ids[shorten_row], neg_am[shorten_row] = 0, 0
    neg_ids[shorten_row, n_ctx - live.numel():] = live
    neg_am[shorten_row, n_ctx - live.numel():] = 1
    return {"context_input_ids": torch.cat([ids, neg_ids]), "context_attention_mask": torch.cat([am, neg_am]),
            "context_batch_start_positions": batch["batch_start_positions"], "batch_features": batch["batch_features"],
            "batch_transcription_ids": batch["batch_transcription_ids"]}


def oracle_embeds(w, d, inputs):
    with torch.no_grad():
        af = O.perception(w, d, inputs["batch_features"])
        return O.embed_splice(w, d, inputs["context_input_ids"], af, inputs["batch_transcription_ids"], inputs["context_batch_start_positions"])


def oracle_forced_logits(w, d, inputs, tokens, x=None):
    """The oracle's per-step logits [T, 2 Bc, V] of the 2 Bc batch, both rows of a sequence teacher-forced on `tokens` [Bc, T]."""
    x = oracle_embeds(w, d, inputs) if x is None else x
    with torch.no_grad():
        return O.greedy_generate(w, d, x, inputs["context_attention_mask"], tokens.shape[1], 0, forced_tokens=torch.cat([tokens, tokens]))[1]


def oracle_guided_greedy(w, d, inputs, g: float, T: int):
    """Free-running guided greedy decoding on the oracle (no cache: step t re-runs the prefix) -> (tokens [Bc, T], logits [T, 2 Bc, V])."""
    x = oracle_embeds(w, d, inputs)
    Bc = x.shape[0] // 2
    toks = torch.zeros(Bc, 0, dtype=torch.long)
    for t in range(T):
        lo = oracle_forced_logits(w, d, inputs, torch.cat([toks, torch.zeros(Bc, 1, dtype=torch.long)], dim=1), x=x)
        R, _, _ = guided_scores_fp64(lo[t, :Bc], lo[t, Bc:], g)
        toks = torch.cat([toks, R.argmax(-1, keepdim=True)], dim=1)
    return toks, lo


def pick_cells(logits, g: float):
    """From collected raw logits [T, 2 Bc, V]: the fp64 guided argmax [T, Bc] and which (step, row) cells count — the top-2 gap of
    the guided scores exceeds twice the derived bound (the larger of the two leading entries'), and no entry further down, whose
    own bound grows with its magnitude, can reach the leader either; a kernel within the bound then picks the same token."""
    Bc = logits.shape[1] // 2
    R, Lc, Lu = guided_scores_fp64(logits[:, :Bc].cpu(), logits[:, Bc:].cpu(), g)
    B = guided_bound(R, Lc, Lu, g)
    top2 = R.topk(2, dim=-1)
    b12 = B.gather(-1, top2.indices)
    counts = (top2.values[..., 0] - top2.values[..., 1]) > 2 * b12.max(dim=-1).values
    reach = torch.where(torch.isinf(R), R, R + B).scatter(-1, top2.indices[..., :1], NEG_INF).max(dim=-1).values
    return top2.indices[..., 0], counts & (top2.values[..., 0] - b12[..., 0] > reach)
