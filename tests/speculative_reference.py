"""Plain-Python statement of draft-and-verify greedy decoding: the lookup rule (desta_spec_ngram_draft), the lockstep accept rule
(desta_spec_accept) and the loop around an arbitrary `next_token(history) -> id` (`CausalLMHIP._speculative_loop`)."""


def ngram_draft(hist, hist_len, row_start, k, n_max, n_min):
    """hist: one row's ids.  -> k ids: the tokens behind the latest earlier occurrence of the row's last n tokens, longest n first."""
    for n in range(n_max, n_min - 1, -1):
        suf = hist[hist_len - n:hist_len]
        if hist_len < n or min(suf) < 0:
            continue
        for i in range(hist_len - 1 - n, max(row_start, 0) - 1, -1):
            if hist[i:i + n] == suf:
                return [hist[i + n + j] if i + n + j < hist_len else -1 for j in range(k)]
    return [-1] * k


def accept(pred, inp, finished, eos, pad, max_take):
    """pred, inp: [B][k + 1].  -> (emitted [B][a], finished [B], next [B], a)"""
    k, rows, lims = len(inp[0]) - 1, [], []
    for p, x, f in zip(pred, inp, finished):
        m = 0
        while m < k and x[m + 1] >= 0 and x[m + 1] == p[m]:
            m += 1
        e = next((j for j in range(m + 1) if p[j] in eos), -1)
        rows.append((m, e))
        if not f and e < 0:
            lims.append(m + 1)
    a = min([max_take] + lims)
    out = [[pad if f or (e >= 0 and j > e) else p[j] for j in range(a)] for p, f, (m, e) in zip(pred, finished, rows)]
    fin = [bool(f or (0 <= e < a)) for f, (m, e) in zip(finished, rows)]
    return out, fin, [r[-1] for r in out], a


def greedy_loop(next_token, prompts, T, eos, pad):
    """Token-by-token greedy: -> [B][T], `pad` behind a row's EOS."""
    out = []
    for pr in prompts:
        h, row, done = list(pr), [], False
        for _ in range(T):
            t = pad if done else next_token(h)
            done = done or t in eos
            row.append(t)
            h.append(t)
        out.append(row)
    return out


def speculative_loop(next_token, prompts, T, k, drafts, eos, pad):
    """drafts(b, n, hist) -> k proposals for emitted positions n .. n + k - 1 of row b.  The cache is a dict slot -> token per row;
    a verify row reads slots [0, cur + j] and asserts each was written and holds the token greedy decoding put there.
    -> ([B][T], verify steps)"""
    B, S = len(prompts), len(prompts[0])
    cache = [dict(enumerate(pr)) for pr in prompts]
    out = [[next_token(list(pr))] for pr in prompts]
    finished = [r[0] in eos for r in out]
    nxt, n, steps = [r[0] for r in out], 1, 0
    while n < T:
        cur = S + n - 1
        inp = [[nxt[b]] + list(drafts(b, n, list(prompts[b]) + out[b])) for b in range(B)]
        pred = []
        for b in range(B):
            row = []
            for j in range(k + 1):
                cache[b][cur + j] = max(inp[b][j], 0)                       # the chunk's append: slots [cur, cur + k]
            if not finished[b]:                                             # everything up to the last emitted token is greedy's own history
                assert [cache[b].get(s) for s in range(cur + 1)] == list(prompts[b]) + out[b], "a stale draft survived in the cache"
            for j in range(k + 1):
                assert all(s in cache[b] for s in range(cur + j + 1)), "read of a slot that was never written"
                row.append(next_token([cache[b][s] for s in range(cur + j + 1)]))
            pred.append(row)
        new, finished, nxt, a = accept(pred, inp, finished, eos, pad, T - n)
        for b in range(B):
            out[b] += new[b]
        n, steps = n + a, steps + 1
    return out, steps
