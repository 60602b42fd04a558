"""Plain-Python statement of draft-and-verify decoding with a pick that depends on the position (`set_speculative(k, scope="all")`):
the loop of tests/speculative_reference.py around `next_token(history, b, t) -> id`, t the emitted position and b the sequence, and
the row rule of desta_sample_rows_bf16 / desta_sample_top_p_rows_bf16 (include/desta_hip.h).

Row (b, j) of a verify step at step0 = n emitted tokens is emitted position n + j of sequence b:
    counter ........... (step, row) = ((step0 + j) mod 2^32, b)         `row_counter`
    penalty history ... hist[b][:hist_len] ++ tail[b][1:1 + j]          `row_history`   (tail = the verify input: last token, drafts)
    penalised ids ..... the distinct ids of that history in [0, cols)   `penalised_ids`
The accept and lookup rules are imported, not restated."""
from speculative_reference import accept, ngram_draft  # noqa: F401  (ngram_draft: the drafts of the callers' lookup source)

M32 = 0xFFFFFFFF


def row_counter(step0, j, b):
    """(step, row) of the RNG counter of row (b, j): the position, which wraps as a uint32, and the SEQUENCE (not the flat row)."""
    return (step0 + j) & M32, b


def row_history(hist, tail, j):
    """The token history row j of a sequence is penalised with: what was emitted, then the j drafts in front of the row."""
    return list(hist) + list(tail[1:1 + j])


def penalised_ids(hist, tail, j, cols):
    return sorted({t for t in row_history(hist, tail, j) if 0 <= t < cols})


def plain_loop(next_token, prompts, T, eos, pad):
    """Token by token: -> [B][T], `pad` behind a row's EOS."""
    out = []
    for b, pr in enumerate(prompts):
        h, row, done = list(pr), [], False
        for t in range(T):
            tok = pad if done else next_token(h, b, t)
            done = done or tok in eos
            row.append(tok)
            h.append(tok)
        out.append(row)
    return out


def speculative_loop(next_token, prompts, T, k, drafts, eos, pad):
    """drafts(b, n, hist) -> k proposals for emitted positions n .. n + k - 1 of row b.  Row j of a chunk is picked at position
    n + j from the history prompt ++ emitted ++ drafts[:j] (`row_history`; a -1 draft sits there as -1, which a penalty ignores and
    acceptance never passes).  -> ([B][T], verify steps)"""
    B = len(prompts)
    out = [[next_token(list(pr), b, 0)] for b, pr in enumerate(prompts)]
    finished = [r[0] in eos for r in out]
    nxt, n, steps = [r[0] for r in out], 1, 0
    while n < T:
        inp = [[nxt[b]] + list(drafts(b, n, list(prompts[b]) + out[b])) for b in range(B)]
        pred = [[next_token(row_history(list(prompts[b]) + out[b], inp[b], j), b, n + j) for j in range(k + 1)] for b in range(B)]
        new, finished, nxt, a = accept(pred, inp, finished, eos, pad, T - n)
        for b in range(B):
            out[b] += new[b]
        n, steps = n + a, steps + 1
    return out, steps
