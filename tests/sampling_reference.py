"""Float64 inverse-CDF reference, allowance and conforming emulation for the kernels that pick the next token:
`desta_sample_bf16` (csrc/sampling.hip, sample_chain_k / sample_greedy_k), `desta_sample_top_p_bf16` (csrc/norm_act.hip,
sample_top_p_k) and `desta_argmax_bf16`.  Plain numpy / torch on the CPU; imported by the host test
(test_sampling_draw_host.py) and the GPU test (test_gpu_sampling_draw.py), which share the case table `CASES` and the row
generator `rows_for()` below.

What a draw must satisfy.  Both samplers invert the prefix sum of the kept masses in INDEX order with one uniform per
(seed, step, row): u = u24 / 2^24, u24 = rng32(seed, step, row) >> 8.  With p_i the exact (float64) normalised mass of kept
token i and C the exact cumulative sum in index order, the pick `tok` is right iff  C_lo <= u < C_hi,  [C_lo, C_hi) =
[C(tok) - p_tok, C(tok)).  A kernel works in fp32 or fixed point, so its boundaries sit within `eps` of the exact ones:
    ratio = max(C_lo - u, u - C_hi, 0) / eps          must be <= 1 for every draw, and is 0 for most.

The contract restated (include/desta_hip.h, desta_sample_bf16 steps 1-7):
    rng32(seed, step, row)   common.h desta_rng32 with idx = (step << 32) | row, seed_lo = seed & 0xffffffff, seed_hi = seed >> 32
    scores(logits, hist, p, T)   steps 1 and 3 in fp32, bit for bit (IEEE multiply / divide): one penalty per DISTINCT history
                             token, ids outside [0, cols) ignored, s < 0 ? s * p : s / p, t = s / T
    kept(t, top_k, top_p, min_p)  steps 4-6 in float64 on t: ties with the k-th value kept, ties with the top-p boundary kept,
                             exp(t - t_max) >= min_p, non-finite scores never kept.  top_p and min_p are the fp32 values the
                             kernel receives, widened.
    margin(...)              how far the inputs are from a decision float64 and fp32 could take differently: the distance of
                             1 - top_p from the nearest cumulative-mass boundary F(v) / Z and the relative distance of min_p
                             from the nearest exp(t - t_max).  `rows_for()` only hands out rows with both >= MARGIN = 1e-4
                             (rows that miss it are drawn again from the next salt), so kept() is unambiguous.
For the top-p kernel the contract is p = softmax(logit / T): its reference scores are float64 x / T (no fp32 division).

eps, with F = 2^-24 and r(x) = (2 |x| + 8) F the relative error of __expf(x) (rowwise_reference.py, swiglu).  If every mass
carries a relative error r_i, a numerator sum_{i<=j} p_i moves by at most sum p_i r_i and so does the normalisation: 2 sum p r.
    chain (sampling.hip:194-196 mass = floor(__expf(t - tmax) 2^40); :261-295 integer prefix sums, target truncated :279):
        eps = 2 (sum_kept p_i r(t_i - tmax) + (K + 1) 2^-40)        K kept tokens lose < 2^-40 each to the floor (Z >= 2^40 units),
                                                                    the target's truncation one more; no other rounding exists
    top-p kernel (norm_act.hip:662 and :681-718: argument (x - mx) * inv_temp, one more rounded product with inv_temp = fl(1 / T)
    itself rounded: 2 |a| F more in the exponent; a thread adds ceil(V / 1024) masses, lane 0 adds 1024 partial sums, target
    and remainder are 4 more roundings, all of sums <= Z):
        eps = 2 (sum_kept p_i (4 |a_i| + 8) F + (ceil(V / 1024) + 1024 + 4) F)
Both are derived from the code; the conforming emulation below must stay inside them on the CPU (test_sampling_draw_host.py).

`emulate()` restates what a conforming kernel computes: the chain kernel's chunk = ceil(V / 1024) rounded up to 8 and its
integer sums, the top-p kernel's chunk = ceil(V / 1024), its sequential fp32 sums per thread (np.cumsum in float32 is
sequential) and lane 0's serial scan; fp32 `exp` stands in for __expf.  The kept set of the emulation is kept() on the
emulation's own scores: the chain kernel's selection sums integers, whose order cannot matter, and MARGIN keeps both
kernels' cut-offs away from every boundary.  Seeded mutations (`MUTATIONS`: name -> kernels it applies to), each an error
these kernels can actually make:
    wave_prefix_dropped     select_bin's cross-wave `before` taken as 0 (a wave's prefix starts at 0)            chain
    strided_order           prefix in the order of row_strided (element c on thread c / 8 % 1024) instead of row_chunk   both
    chunk_unrounded         chain chunk not rounded up to 8: the 16-byte loop starts off alignment and reads the aligned
                            group below it, so columns are counted twice or skipped                             chain
    tail_dropped            columns [V - V % 8, V) carry no mass                                                chain
    u_low_bits              rng32 & 0xffffff instead of >> 8                                                    both
    row_ignored             counter without the row                                                             both
    step_low_word           step added to the low word instead of shifted to the high word                      both
    seed_hi_dropped         high seed word lost                                                                 both
    penalty_per_occurrence  a repeated history token penalised once per occurrence                              chain
    unpenalised_mass        the draw's masses taken from unpenalised scores                                     chain

Flat rows (every finite entry equal) have closed forms with no tolerance (`flat_pick`): a tie with the maximum has mass exactly
2^40 (chain) or 1.0f (top-p kernel), so the chain picks kept index (u24 K) >> 24 and the top-p kernel kept index
min(floor(fl32(fl32(u24) 2^-24 K)), K - 1) (the fp32 product may round up to K: the kernel then takes the last kept token)."""
import concurrent.futures
import functools
import math

import numpy as np
import torch

F = 2.0 ** -24
MARGIN = 1e-4
ROWS = 64
SNT = 1024
STEPS = (0, 1, 2 ** 31, 2 ** 32 - 1)
SEEDS = (99, (7 << 32) | 5)
M32 = 0xFFFFFFFF

MUTATIONS = {
    "wave_prefix_dropped": ("chain",), "strided_order": ("chain", "top_p"), "chunk_unrounded": ("chain",), "tail_dropped": ("chain",),
    "u_low_bits": ("chain", "top_p"), "row_ignored": ("chain", "top_p"), "step_low_word": ("chain", "top_p"),
    "seed_hi_dropped": ("chain", "top_p"), "penalty_per_occurrence": ("chain",), "unpenalised_mass": ("chain",),
}
_RNG_MUTATIONS = ("u_low_bits", "row_ignored", "step_low_word", "seed_hi_dropped")


# ---------------------------------------------------------------------------------------------------------------- rng
def rng32(seed, step, row, mutation=None):
    """common.h desta_rng32 as the samplers call it (Python integers)."""
    seed_lo, seed_hi = seed & M32, (seed >> 32) & M32
    lo, hi = row & M32, step & M32
    if mutation == "row_ignored":
        lo = 0
    if mutation == "step_low_word":
        lo, hi = (row + step) & M32, 0
    if mutation == "seed_hi_dropped":
        seed_hi = 0
    key = ((seed_lo ^ ((seed_hi * 0x632BE5AB) & M32)) * 0xC2B2AE35) & M32
    x = (lo + seed_lo * 0x9E3779B9 + (hi + seed_hi) * 0x85EBCA6B) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= (x >> 15) ^ key
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def u24(seed, step, row, mutation=None):
    x = rng32(seed, step, row, mutation)
    return (x & 0xFFFFFF) if mutation == "u_low_bits" else (x >> 8)


def u24_rows(seed, step, rows=ROWS, mutation=None):
    return np.array([u24(seed, step, r, mutation) for r in range(rows)], dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------ contract
def scores(logits_bf16, hist=None, penalty=1.0, T=1.0, per_occurrence=False):
    """Steps 1 and 3 in fp32 -> (s, t) float32 numpy arrays [rows, V]."""
    s = logits_bf16.float().clone()
    rows, V = s.shape
    if penalty != 1.0 and hist is not None and hist.shape[1] > 0:
        p = torch.tensor(float(penalty), dtype=torch.float32)
        count = torch.zeros(rows, V, dtype=torch.int32)
        ok = (hist >= 0) & (hist < V)
        for r in range(rows):
            count[r] = torch.bincount(hist[r][ok[r]], minlength=V).to(torch.int32)
        for n in range(1, int(count.max()) + 1 if per_occurrence else 2):
            s = torch.where(count >= n, torch.where(s < 0, s * p, s / p), s)
    t = s / torch.tensor(float(T), dtype=torch.float32)
    return s.numpy(), t.numpy()


def _tmax(t):
    return np.where(np.isfinite(t), t, -np.inf).max(axis=1)


def _ascending_mass(key, e):
    """F_i = sum of e_j over key_j <= key_i, per row, and F at every sorted position (the end of its tie group)."""
    rows, V = key.shape
    flat = (np.argsort(key, axis=1) + np.arange(rows)[:, None] * V).ravel()
    ks = key.ravel()[flat].reshape(rows, V)
    cum = np.cumsum(e.ravel()[flat].reshape(rows, V), axis=1)
    end = np.full((rows, V), V - 1, dtype=np.int64)              # index of the last member of the tie group, by position
    end[:, :-1] = np.where(ks[:, 1:] != ks[:, :-1], np.arange(V - 1)[None, :], V - 1)
    end = np.minimum.accumulate(end[:, ::-1], axis=1)[:, ::-1]
    Fs = np.take_along_axis(cum, end, 1)
    Fi = np.empty(rows * V)
    Fi[flat] = Fs.ravel()
    return Fi.reshape(rows, V), Fs


def kept(t, top_k=0, top_p=1.0, min_p=0.0, want_margin=False, key=None):
    """Steps 4-6 in float64 -> bool [rows, V] (and, with want_margin, the per-row (top-p, min-p) margins).  `key` (optional,
    float32) orders the tokens exactly as t does (t itself when it is fp32, the bf16 logits for x / T): comparisons only."""
    key = np.asarray(t) if key is None else key
    t = np.asarray(t, dtype=np.float64)
    rows, V = t.shape
    fin = np.isfinite(t)
    keep = fin.copy()
    tmax = _tmax(t)
    m_p = np.full(rows, np.inf)
    m_min = np.full(rows, np.inf)
    if 0 < top_k < V:
        kth = np.partition(key, V - top_k, axis=1)[:, V - top_k]
        keep &= key >= kth[:, None]
    if float(np.float32(top_p)) < 1.0 or float(np.float32(min_p)) > 0.0:
        with np.errstate(invalid="ignore", over="ignore"):
            e = np.where(fin, np.exp(t - tmax[:, None]), 0.0)
    if float(np.float32(top_p)) < 1.0:
        cutf = 1.0 - float(np.float32(top_p))
        es = np.where(keep, e, 0.0)
        Z = es.sum(axis=1)
        Fi, Fs = _ascending_mass(np.where(keep, key, key.dtype.type(-np.inf)), es)
        with np.errstate(invalid="ignore", divide="ignore"):
            keep &= Fi > cutf * Z[:, None]
            m_p = np.where(Z > 0, np.abs(Fs / Z[:, None] - cutf).min(axis=1), np.inf)
    if float(np.float32(min_p)) > 0.0:
        mp = float(np.float32(min_p))
        m_min = np.where(keep, np.abs(e - mp) / mp, np.inf).min(axis=1)
        keep &= e >= mp
    return (keep, m_p, m_min) if want_margin else keep


def case_scores(case, logits, hist, mutation=None):
    """-> (t, key): the scores the contract defines for the case's kernel (chain: fp32 t = s / T; top-p kernel: float64 x / T)
    and a float32 array that orders the tokens as t does."""
    if case["kernel"] == "chain":
        pen = case.get("penalty", 1.0)
        _, t = scores(logits, hist if pen != 1.0 else None, pen, case["T"], per_occurrence=mutation == "penalty_per_occurrence")
        return t, t
    x = logits.float().numpy()
    return x.astype(np.float64) / float(np.float32(case["T"])), x


def case_kept(case, t, key, want_margin=False):
    return kept(t, case.get("top_k", 0), case.get("top_p", 1.0), case.get("min_p", 0.0), want_margin, key)


_KEPT = {}          # (V, profile, kernel, setting) -> (packed kept [rows, V], top-p margins, min-p margins), filled by rows_for()


class Reference:
    """The float64 side of one case: kept set, margins, normalised masses p, cumulative C (index order), eps per row."""

    def __init__(self, case, logits=None, hist=None):
        V = case["V"]
        stored = None
        if logits is None:
            logits, hist = rows_for(case["V"], case["profile"])
            stored = _KEPT[(V, case["profile"], case["kernel"], case["setting"])]
        self.case = case
        t, key = case_scores(case, logits, hist)
        t = np.asarray(t, dtype=np.float64)
        if stored is not None:
            self.kept = np.unpackbits(stored[0], axis=1, count=V).astype(bool)
            self.margin_top_p, self.margin_min_p = stored[1], stored[2]
        else:
            self.kept, self.margin_top_p, self.margin_min_p = case_kept(case, t, key, True)
        tmax = _tmax(t)
        with np.errstate(invalid="ignore"):
            a = np.where(self.kept, t - tmax[:, None], 0.0)
            p = np.where(self.kept, np.exp(a), 0.0)
        Z = p.sum(axis=1, keepdims=True)
        self.finite_rows = Z[:, 0] > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            p = np.where(Z > 0, p / Z, 0.0)
        self.p = p
        self.C = np.cumsum(p, axis=1)
        K = self.kept.sum(axis=1)
        if case["kernel"] == "chain":
            self.eps = 2.0 * ((p * (2.0 * np.abs(a) + 8.0)).sum(axis=1) * F + (K + 1) * 2.0 ** -40)
        else:
            self.eps = 2.0 * ((p * (4.0 * np.abs(a) + 8.0)).sum(axis=1) * F + (math.ceil(V / SNT) + SNT + 4) * F)

    def interval(self, tok):
        r = np.arange(len(tok))
        hi = self.C[r, tok]
        lo = np.where(tok > 0, self.C[r, np.maximum(tok - 1, 0)], 0.0)
        return lo, hi

    def ratio(self, tok, u):
        """max(C_lo - u, u - C_hi, 0) / eps per row for the picks `tok` under the 24-bit uniforms `u` (int arrays [rows])."""
        tok = np.asarray(tok, dtype=np.int64)
        lo, hi = self.interval(tok)
        uu = np.asarray(u, dtype=np.float64) / 2.0 ** 24
        return np.maximum(np.maximum(lo - uu, uu - hi), 0.0) / self.eps


def margin(case):
    ref = reference(case)
    return ref.margin_top_p, ref.margin_min_p


def interval(case, tok):
    return reference(case).interval(np.asarray(tok))


def eps(case):
    return reference(case).eps


def ratio(case, tok, u):
    return reference(case).ratio(tok, u)


@functools.lru_cache(maxsize=1)
def _reference(key):
    return Reference(CASE_BY_ID[key])


def reference(case):
    """The Reference of a table case (the last one is cached; (V, ld) pairs with one V share rows, so run them back to back)."""
    return _reference(ref_id(case))


# ------------------------------------------------------------------------------------------------------------ emulation
def chain_chunk(V):
    return ((V + SNT - 1) // SNT + 7) & ~7


def top_p_chunk(V):
    return (V + SNT - 1) // SNT


def row_aligned(ld, rows=ROWS):
    """per row: does a row of a 16-byte aligned [rows, ld] bf16 buffer start on a 16-byte boundary"""
    return (np.arange(rows) * ld * 2) % 16 == 0


def _thread_order(V, chunk, strided, vec):
    """columns of each thread in the order it walks them -> int [1024, L], -1 padded"""
    if not strided:
        L = chunk
        idx = np.arange(SNT)[:, None] * chunk + np.arange(L)[None, :]
        return np.where(idx < V, idx, -1)
    cols = [[] for _ in range(SNT)]
    n8 = V >> 3 if vec else 0
    for g in range(n8):
        cols[g % SNT].extend(range(g * 8, g * 8 + 8))
    for c in range(n8 * 8, V):
        cols[(c - n8 * 8) % SNT].append(c)
    L = max(len(c) for c in cols)
    return np.array([c + [-1] * (L - len(c)) for c in cols], dtype=np.int64)


class Emulation:
    """What a conforming kernel holds for one case (with an optional seeded error); draw(u24[rows]) -> picks [rows]."""

    def __init__(self, case, mutation=None, logits=None, hist=None):
        kernel, V, ld = case["kernel"], case["V"], case["ld"]
        stored = None
        if logits is None:
            logits, hist = rows_for(case["V"], case["profile"])
            stored = _KEPT[(V, case["profile"], kernel, case["setting"])]
        assert mutation is None or kernel in MUTATIONS[mutation], (mutation, kernel)
        self.case, self.kernel, self.mutation, self.V = case, kernel, mutation, V
        rows = logits.shape[0]
        self.rows = rows
        vec_rows = row_aligned(ld, rows)
        t64, key = case_scores(case, logits, hist, mutation)
        if mutation != "penalty_per_occurrence" and stored is not None:
            self.kept = np.unpackbits(stored[0], axis=1, count=V).astype(bool)
        else:
            self.kept = case_kept(case, t64, key)
        if kernel == "chain":
            chunk = (V + SNT - 1) // SNT if mutation == "chunk_unrounded" else chain_chunk(V)
            t = t64
            tmass = case_scores(dict(case, penalty=1.0), logits, None)[0] if mutation == "unpenalised_mass" else t
            tmax = _tmax(t).astype(np.float32)
            with np.errstate(invalid="ignore", over="ignore"):
                e = np.exp((tmass - tmax[:, None]).astype(np.float32)).astype(np.float32)
            e = np.minimum(e, np.float32(2.0 ** 20))                                # (only the unpenalised masses can pass 1)
            mass = np.where(np.isfinite(tmass), e * np.float32(2.0 ** 40), 0).astype(np.int64)
            mass = np.where(self.kept, mass, 0)
            if mutation == "tail_dropped":
                mass[:, V - V % 8:] = 0
        else:
            chunk = top_p_chunk(V)
            x = logits.float().numpy()
            mx = _tmax(x).astype(np.float32)
            inv_temp = np.float32(1.0) / np.float32(case["T"])
            with np.errstate(invalid="ignore", over="ignore"):
                mass = np.exp(((x - mx[:, None]).astype(np.float32) * inv_temp).astype(np.float32)).astype(np.float32)
            mass = np.where(self.kept, mass, np.float32(0.0)).astype(np.float32)
        strided = mutation == "strided_order"
        if not strided and mutation != "chunk_unrounded":           # every row walks [tid * chunk, tid * chunk + chunk)
            self.order = _thread_order(V, chunk, False, False)
            pad = np.zeros((rows, SNT * chunk - V), dtype=mass.dtype)
            self.m = np.concatenate([mass[:, :SNT * chunk], pad], axis=1).reshape(rows, SNT, chunk)
        else:
            # row_strided's order depends on the row's alignment (16-byte groups or single columns); the top-p kernel has no vector path
            variant = vec_rows & strided & (kernel == "chain")
            orders = {v: _thread_order(V, chunk, strided, v) for v in set(variant.tolist())}
            L = max(o.shape[1] for o in orders.values())
            self.order = np.full((rows, SNT, L), -1, dtype=np.int64)
            for r in range(rows):
                o = orders[bool(variant[r])]
                self.order[r, :, :o.shape[1]] = o
            src = np.maximum(self.order, 0)
            if mutation == "chunk_unrounded":                       # the misaligned 16-byte loop of aligned rows reads the group below
                c0 = np.arange(SNT)[:, None] * chunk
                c1 = np.minimum(V, c0 + chunk)
                invec = np.arange(L)[None, :] < np.maximum(c1 - c0, 0) // 8 * 8
                shifted = np.where(invec, src[0] - c0 % 8, src[0])
                src = np.where(vec_rows[:, None, None], shifted[None], src)
            m = np.take_along_axis(mass, src.reshape(rows, -1), 1).reshape(rows, SNT, L)
            self.m = np.where(self.order >= 0, m, 0).astype(mass.dtype)
        self.cs = np.cumsum(self.m, axis=2, dtype=self.m.dtype)     # a thread's running sum, in its walk order (fp32: sequential)
        self.mine = self.cs[:, :, -1]

    def draw(self, u):
        u = np.asarray(u, dtype=np.int64)
        rows = self.rows
        rr = np.arange(rows)
        if self.kernel == "chain":
            tot = self.mine.sum(axis=1)
            # sampling.hip:279: (u64)((double)u24 * 2^-24 * (double)total); Python floats are the same IEEE doubles
            target = np.array([int(float(int(a)) * (1.0 / 16777216.0) * float(int(b))) for a, b in zip(u, tot)], dtype=np.int64)
            if self.mutation == "wave_prefix_dropped":
                incl = np.cumsum(self.mine.reshape(rows, SNT // 64, 64), axis=2).reshape(rows, SNT)
            else:
                incl = np.cumsum(self.mine, axis=1)
            excl = incl - self.mine
            hit = (excl <= target[:, None]) & (target[:, None] < incl)
            found = hit.any(axis=1)                                 # no thread claims the target: sel stays (0, 0)
            tid = np.where(found, hit.argmax(axis=1), 0)
            rem = target - np.where(found, excl[rr, tid], 0)
        else:
            pc = np.cumsum(self.mine, axis=1, dtype=np.float32)     # lane 0's serial scan (norm_act.hip:692-702)
            tot = pc[:, -1]
            target = ((u.astype(np.float32) * np.float32(1.0 / 16777216.0)).astype(np.float32) * tot).astype(np.float32)
            over_t = pc[:, :SNT - 1] > target[:, None]
            stop = np.where(over_t.any(axis=1), over_t.argmax(axis=1), SNT - 1)
            run_before = np.where(stop > 0, pc[rr, np.maximum(stop - 1, 0)], np.float32(0.0)).astype(np.float32)
            rem = (target - run_before).astype(np.float32)
            tid = stop.copy()
            for r in range(rows):                                   # :704 walk back over threads that hold no mass
                while tid[r] > 0 and self.mine[r, tid[r]] == 0:
                    tid[r] -= 1
        over = self.cs[rr, tid] > rem[:, None]
        order = self.order[tid] if self.order.ndim == 2 else self.order[rr, tid]
        tok = np.where(over.any(axis=1), order[rr, over.argmax(axis=1)], -1)
        if self.kernel == "chain":
            return np.where(tok >= 0, tok, 0)
        held = self.kept[rr[:, None], np.maximum(order, 0)] & (order >= 0)
        lastj = held.shape[1] - 1 - held[:, ::-1].argmax(axis=1)
        last = np.where(held.any(axis=1), order[rr, lastj], 0)      # :720 the last kept column of the chunk (token 0 if none)
        return np.where(tok >= 0, tok, last)


@functools.lru_cache(maxsize=2)
def _emulation(key, mutation):
    return Emulation(CASE_BY_ID[key], mutation)


def emulate(case, kernel, seed, step, row=None, mutation=None):
    """The pick of a conforming kernel (or of one with the seeded error) -> token of `row`, or of every row when row is None."""
    assert kernel == case["kernel"]
    state_mut = None if mutation in _RNG_MUTATIONS else mutation
    em = _emulation(case_id(case), state_mut)
    tok = em.draw(u24_rows(seed, step, em.rows, mutation if mutation in _RNG_MUTATIONS else None))
    return tok if row is None else int(tok[row])


def flat_pick(kernel, kept_row, u):
    """Closed form of the pick on a flat row: kept_row bool [V], u a 24-bit integer."""
    idx = np.flatnonzero(kept_row)
    K = len(idx)
    if kernel == "chain":
        j = (int(u) * K) >> 24
    else:
        target = np.float32(np.float32(u) * np.float32(1.0 / 16777216.0)) * np.float32(K)
        j = min(int(math.floor(float(np.float32(target)))), K - 1)
    return int(idx[j])


# ---------------------------------------------------------------------------------------------------------- case table
VLD = ((4099, 4101), (4099, 4104), (128256, 128256), (151936, 151944))
PROFILES = ("randn", "two_spike", "peaked", "suppressed", "flat", "flat_suppressed")
CHAIN_SETTINGS = {
    "T": dict(T=0.8),
    "top_k": dict(T=1.0, top_k=50),
    "top_p": dict(T=0.7, top_p=0.9),
    "min_p": dict(T=0.9, min_p=0.05),
    "full": dict(T=0.7, top_k=50, top_p=0.9, min_p=0.05, penalty=1.3),
}
TOP_P_SETTINGS = {"T0.7_p0.9": dict(T=0.7, top_p=0.9), "T1.3_p0.5": dict(T=1.3, top_p=0.5), "T1.0_p1.0": dict(T=1.0, top_p=1.0)}
HIST_LEN = 40

CASES = []
for _V, _ld in VLD:
    for _prof in PROFILES:
        for _name, _s in CHAIN_SETTINGS.items():
            CASES.append(dict(kernel="chain", V=_V, ld=_ld, profile=_prof, setting=_name, **_s))
        for _name, _s in TOP_P_SETTINGS.items():
            CASES.append(dict(kernel="top_p", V=_V, ld=_ld, profile=_prof, setting=_name, **_s))


def case_id(c):
    return f"{c['kernel']}-V{c['V']}-ld{c['ld']}-{c['profile']}-{c['setting']}"


def ref_id(c):
    """cases that differ only in ld share their reference; the id of the first of them"""
    return case_id(dict(c, ld=next(ld for V, ld in VLD if V == c["V"])))


CASE_BY_ID = {case_id(c): c for c in CASES}
FLAT = ("flat", "flat_suppressed")


def _suppress_mask(g, V):
    m = g.random(V) < 0.25
    run = V // 12                                                # longer than any thread's chunk (<= 152 columns)
    a = int(g.integers(0, V - run))
    m[a:a + run] = True
    return m


def _make_row(V, profile, r, salt):
    g = np.random.default_rng([V, PROFILES.index(profile), r, salt])
    if profile in ("randn", "suppressed"):
        x = g.standard_normal(V, dtype=np.float32) * 3.0
    elif profile == "two_spike":
        x = g.standard_normal(V, dtype=np.float32) * 0.5
        i0 = 3 * chain_chunk(V) + r % 5
        i1 = min(1000 * chain_chunk(V) + r % 5, V - 1 - r % 3)   # thread 1000's chunk, or the last populated one
        hi, lo = (i0, i1) if r % 2 else (i1, i0)
        x[hi], x[lo] = 40.0, 39.75
    elif profile == "peaked":
        x = g.standard_normal(V, dtype=np.float32)
        x[int(g.integers(0, V))] = float(round(math.log(V) + 14.3))
    else:
        x = np.full(V, (2.0, -1.5, 0.0, 0.75)[r % 4], dtype=np.float32)
    if profile in ("suppressed", "flat_suppressed"):
        x[_suppress_mask(g, V)] = -np.inf
    h = g.integers(0, V, HIST_LEN)
    h[0] = int(np.argmax(x)) if r % 2 == 0 else h[0]             # a heavy token in the history of the even rows ...
    h[1] = h[2] = h[0]                                           # ... three times: penalised once
    h[3:8] = np.arange(5)
    h[8:12] = (-1, V, V + 5, 2 ** 40)                            # outside [0, V): ignored
    return x, h


@functools.lru_cache(maxsize=None)
def rows_for(V, profile, rows=ROWS):
    """(bf16 logits [rows, V], int64 history [rows, HIST_LEN]) of a (V, profile).  Row r is drawn from salt 0, 1, ... until its
    margins under every setting of both kernels are >= MARGIN (a condition on the inputs, evaluated on the reference alone).
    The kept sets and margins computed on the way are stored per setting (`_KEPT`) and reused by Reference / Emulation."""
    x = np.empty((rows, V), dtype=np.float32)
    h = np.empty((rows, HIST_LEN), dtype=np.int64)
    todo = np.arange(rows)
    settings = [dict(kernel="chain", V=V, ld=V, profile=profile, setting=n, **s) for n, s in CHAIN_SETTINGS.items()]
    settings += [dict(kernel="top_p", V=V, ld=V, profile=profile, setting=n, **s) for n, s in TOP_P_SETTINGS.items()]
    store = {}
    for salt in range(64):
        for r in todo:
            x[r], h[r] = _make_row(V, profile, int(r), salt)
        lg = torch.from_numpy(x[todo]).to(torch.bfloat16)
        hh = torch.from_numpy(h[todo])
        bad = np.zeros(len(todo), dtype=bool)
        with concurrent.futures.ThreadPoolExecutor(4) as pool:   # numpy releases the GIL: the settings are independent
            results = list(pool.map(lambda c: case_kept(c, *case_scores(c, lg, hh), True), settings))
        for c, (k, m_p, m_min) in zip(settings, results):
            bad |= (m_p < MARGIN) | (m_min < MARGIN)
            st = store.setdefault(c["setting"] + c["kernel"], [np.zeros((rows, (V + 7) // 8), dtype=np.uint8), np.zeros(rows), np.zeros(rows)])
            st[0][todo], st[1][todo], st[2][todo] = np.packbits(k, axis=1), m_p, m_min
        todo = todo[bad]
        if len(todo) == 0:
            break
    assert len(todo) == 0, (V, profile, todo)
    for c in settings:
        _KEPT[(V, profile, c["kernel"], c["setting"])] = tuple(store[c["setting"] + c["kernel"]])
    return torch.from_numpy(x).to(torch.bfloat16), torch.from_numpy(h)
