"""Reference side of the hard-constraint tests (`desta_logit_constraints_bf16`, `generate(no_repeat_ngram_size=, bad_words_ids=,
suppress_tokens=, begin_suppress_tokens=, min_new_tokens=)`): a plain Python restatement of HF's five banning processors on ONE
row, (history, t, settings, vocab) -> banned set.  tests/test_constraints_host.py pins it to the installed transformers'
classes; the GPU tests hold the kernel and the decode loops to it.

`history` is HF's `input_ids` of the row (any ints; a -1 or an id >= vocab matches like any other value and is never banned), `t`
the emitted position the row picks (HF: input_ids.shape[-1] - prompt length).  Settings, None = off:
  no_repeat_ngram_size = n   nothing while L + 1 < n; else history[i + n - 1] for every 0 <= i <= L - n whose n - 1 predecessors
                             equal the last n - 1 tokens of the history (n = 1: every token seen)
  bad_words_ids              [e] words of an EOS id e are dropped; a one-token word is always banned; a word w of m > 1 tokens
                             bans w[-1] iff m <= L and history[L - m + 1:] == w[:-1]  (m <= L, not m - 1 <= L: HF skips a word
                             longer than the context)
  suppress_tokens            always banned (EOS not filtered)
  begin_suppress_tokens      banned iff t == 0
  min_new_tokens = m         every EOS id banned while t < m; off without EOS ids"""
import numpy as np
import torch

NEG_INF = float("-inf")
KEYS = ("no_repeat_ngram_size", "bad_words_ids", "suppress_tokens", "begin_suppress_tokens", "min_new_tokens")


def grouped_history(hist, tail=None, j=0):
    """The history of row (b, j) of a grouped launch: hist[b, :hist_len] followed by tail[b, 1:1 + j]."""
    return [int(x) for x in hist] + ([int(x) for x in tail[1:1 + j]] if j else [])


def banned(history, t, vocab, *, no_repeat_ngram_size=None, bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None,
           min_new_tokens=None, eos_token_ids=None):
    h = [int(x) for x in history]
    L = len(h)
    eos = [int(e) for e in (eos_token_ids or [])]
    out = set()
    n = no_repeat_ngram_size
    if n and L + 1 >= n:
        ctx = h[L - (n - 1):] if n > 1 else []
        for i in range(L - n + 1):
            if h[i:i + n - 1] == ctx:
                out.add(h[i + n - 1])
    for w in bad_words_ids or []:
        w = [int(x) for x in w]
        if len(w) == 1 and w[0] in eos:
            continue
        m = len(w)
        if m == 1:
            out.add(w[0])
        elif m <= L and h[L - (m - 1):] == w[:-1]:
            out.add(w[-1])
    out.update(int(x) for x in suppress_tokens or [])
    if t == 0:
        out.update(int(x) for x in begin_suppress_tokens or [])
    if min_new_tokens and t < min_new_tokens:
        out.update(eos)
    return {c for c in out if 0 <= c < vocab}


def banned_mask(history, t, vocab, **settings):
    m = np.zeros(vocab, dtype=bool)
    m[sorted(banned(history, t, vocab, **settings))] = True
    return m


def apply(row: torch.Tensor, mask) -> torch.Tensor:
    """A copy of `row` [V] with -inf on the banned set; everything else keeps its bits."""
    out = row.clone()
    out[torch.as_tensor(mask, device=row.device)] = NEG_INF
    return out


def violations(ids, vocab, prompt=(), eos_token_ids=None, **settings):
    """[(t, token)] of the emitted tokens `ids` (one row) that lie in their step's banned set, the history being `prompt` + ids[:t];
    the row ends with its first EOS (what follows is padding, which nothing constrains).  A step whose every token is banned
    yields token 0 by the pickers' rule and is no violation."""
    ids = [int(x) for x in ids]
    eos = [int(e) for e in (eos_token_ids or [])]
    end = next((t + 1 for t, tok in enumerate(ids) if tok in eos), len(ids))
    out = []
    for t, tok in enumerate(ids[:end]):
        b = banned(list(prompt) + ids[:t], t, vocab, eos_token_ids=eos, **settings)
        if tok in b and not (len(b) == vocab and tok == 0):                         # every token banned: the pickers yield token 0
            out.append((t, tok))
    return out
