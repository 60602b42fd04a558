"""Float64 reference for steps 7-9 of `desta_sample_truncated_rows_bf16` (csrc/sampling.hip, sample_truncated_k): HF's
TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper behind min-p, in front of the draw.  Plain numpy on the CPU, on top
of tests/sampling_reference.py (`S`): its row profiles (`S._make_row`), `S.scores()`, `S.kept()` for steps 4-6, the RNG, the
interval check `Reference.ratio` and the chain `eps` are reused as they are.  Given a kept set the draw and its allowance are
the chain's, so no new draw tolerance exists here; what is new is the kept set, and that is compared EXACTLY.

The contract restated (include/desta_hip.h), all on the fp32 scores t of one row, S0 = the survivors of steps 4-6,
a_i = t_i - t_max, e_i = exp(a_i); every step renormalises over its own input set (p_i = e_i / sum of e over that set):
    7. typical_p = m < 1    c = sum p_i a_i, d_i = |a_i - c|, D = the smallest d with sum_{d_i <= D} p_i >= m, keep d_i <= D
    8. epsilon_cutoff > 0   keep p_i >= epsilon, or t_i == the largest t of step 8's input set
    9. eta_cutoff > 0       H = -sum p_i log p_i, theta = min(eta, sqrt(eta) exp(-H)), keep p_i >= theta, or t_i == that largest t
m, epsilon and eta are the fp32 values the kernel receives, widened.

Margins: how far a row is from a decision that float64 and the kernel could take differently, evaluated on the reference alone.
`rows_for()` redraws a row from the next salt until all of them hold under every setting, so no case is left out:
    (a) |m - F / Z| over the cumulative mass F at the end of every distinct-d group            >= MARGIN = 1e-4
    (b) |d_i - D| over every surviving-set token with d_i != D                                  >= max(MARGIN, 4 err_d)
    (c) |p_i - epsilon| / epsilon over step 8's input set                                       >= MARGIN
    (d) |p_i - theta| / theta over step 9's input set                                           >= MARGIN
and, for settings with top-p / min-p in front, the two margins of S.kept().

err_d, the kernel's worst error on d, from its code (F = 2^-24, r(x) = (2 |x| + 8) F the relative error of __expf(x), as in
sampling_reference.py).  The kernel holds Z = sum floor(__expf(a_i) 2^40) and EA = sum floor(fl(__expf(a_i) * -a_i) 2^40) as
integers (`stats` in sample_truncated_k, csrc/sampling_chain.h: no rounding in the sums), a_i = fl(t_i - t_max), and c = -fl32(EA / Z) (a double division).
Every term of EA carries r(a_i) from __expf, F from fl(a_i) and F from the product, and loses < 1 unit to the floor; every term
of Z carries r(a_i) and the floor.  With K survivors in S0 and Z their mass in units of the row maximum's (steps 4-6 never
remove the row maximum, so Z >= 1):
    delta_c <= sum p_i ((|a_i| + |c|) r(a_i) + 2 F |a_i|) + (1 + |c|) K 2^-40 / Z
Then d_i = fl(|fl(a_i) - fl32(c)|): F |a_i| + F |c| + F d_i more, and |a_i| <= |c| + d_i.  Only tokens with d_i < D + 1 can miss
margin (b) (MARGIN and 4 err_d are far below 1), so for those
    err_d = delta_c + 2 F (|c| + D + 1)
About 1e-6 on the table's rows (c is a few units, D below 10), so 4 err_d stays below MARGIN there and (b) is 1e-4 in effect;
the max() keeps the bound honest on rows where it would not.  The comparisons of steps 8 and 9 carry r(a) <= 30 F on the token
(p >= 1e-4 Z means |a| <= 10), F on the threshold and sum p r on Z and H: below 4e-6 relative, 25 times inside MARGIN.

Seeded mutations of the reference (`MUTATIONS`), each a way to get these steps wrong that the table must tell apart
(test_truncation_host.py):
    exempt_row_max            steps 8 / 9 exempt ties with t_max instead of ties with the survivors' maximum
    entropy_not_renormalised  step 9's H from p_i = e_i / Z(S0) over the survivors, not renormalised over them
    entropy_before_epsilon    step 9's H over step 8's input set
    boundary_dropped          step 7 keeps d < D (the token closest to c still stays)
    typical_by_neglogp        step 7 orders by -log p (a plain "least probable first" nucleus) instead of d"""
import functools

import numpy as np
import torch

import sampling_reference as S

F = S.F
MARGIN = S.MARGIN
ROWS = 32
MUTATIONS = ("exempt_row_max", "entropy_not_renormalised", "entropy_before_epsilon", "boundary_dropped", "typical_by_neglogp")

SETTINGS = {
    "typical": dict(T=0.8, typical_p=0.9),
    "typical_lo": dict(T=1.0, typical_p=0.2),
    "eps": dict(T=1.0, epsilon_cutoff=3e-4),
    "eta": dict(T=1.0, eta_cutoff=2e-3),
    "typical_lo_eps": dict(T=1.0, typical_p=0.2, epsilon_cutoff=3e-4),        # step 7 removes the row maximum in front of step 8
    "typical_lo_eps_hi": dict(T=1.0, typical_p=0.2, epsilon_cutoff=0.25),     # ... and step 8 leaves only the ties with ITS maximum
    "tail3": dict(T=0.9, typical_p=0.95, epsilon_cutoff=3e-4, eta_cutoff=6e-4),
    "all": dict(T=0.7, top_k=50, top_p=0.9, min_p=0.05, typical_p=0.9, epsilon_cutoff=9e-4, eta_cutoff=2e-3, penalty=1.3),
}
CASES = []
for _V, _ld in S.VLD:
    for _prof in S.PROFILES:
        for _name, _s in SETTINGS.items():
            CASES.append(dict(kernel="chain", V=_V, ld=_ld, profile=_prof, setting=_name, **_s))


def case_id(c):
    return f"V{c['V']}-ld{c['ld']}-{c['profile']}-{c['setting']}"


def truncation_args(case):
    return dict(typical_p=case.get("typical_p", 1.0), epsilon_cutoff=case.get("epsilon_cutoff", 0.0), eta_cutoff=case.get("eta_cutoff", 0.0))


def _f32(v):
    return float(np.float32(v))


def kept_truncated(t, kept0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, want_margin=False, mutation=None):
    """Steps 7-9 in float64 on the scores t [rows, V] and the survivors kept0 of steps 4-6 -> bool [rows, V]; with want_margin
    also {"a", "b", "c", "d": per-row margins, "err_d", "b_need": max(MARGIN, 4 err_d) per row}."""
    t = np.asarray(t, dtype=np.float64)
    rows, V = t.shape
    fin = np.isfinite(t)
    keep = np.asarray(kept0, dtype=bool) & fin
    tmax = S._tmax(t)
    with np.errstate(invalid="ignore", over="ignore"):
        a = np.where(fin, t - tmax[:, None], 0.0)
        e = np.where(fin, np.exp(a), 0.0)
    inf = np.full(rows, np.inf)
    mg = {"a": inf.copy(), "b": inf.copy(), "c": inf.copy(), "d": inf.copy(), "b_need": np.full(rows, MARGIN), "err_d": np.zeros(rows)}

    def probs(k):
        es = np.where(k, e, 0.0)
        Z = es.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return es, Z, np.where(Z[:, None] > 0, es / Z[:, None], 0.0)

    def entropy(p):
        with np.errstate(invalid="ignore", divide="ignore"):
            return -np.where(p > 0, p * np.log(p), 0.0).sum(axis=1)

    es0, Z0, p0 = probs(keep)
    m = _f32(typical_p)
    if m < 1.0:
        es, Z, p = es0, Z0, p0
        c = (p * a).sum(axis=1)
        d = np.where(keep, np.abs(a - c[:, None]), np.inf)
        order = np.where(keep, -a, np.inf) if mutation == "typical_by_neglogp" else d
        Fi, Fs = S._ascending_mass(order, es)
        with np.errstate(invalid="ignore", divide="ignore"):
            reach = keep & (Fi >= m * Z[:, None])
            D = np.where(reach, order, np.inf).min(axis=1)
            D = np.where(np.isfinite(D), D, np.where(keep, order, -np.inf).max(axis=1))          # (rounding: the whole set misses m)
            mg["a"] = np.where(Z > 0, np.abs(Fs / Z[:, None] - m).min(axis=1), np.inf)
            mg["b"] = np.where(keep & (order != D[:, None]), np.abs(order - D[:, None]), np.inf).min(axis=1)
        r = (2.0 * np.abs(a) + 8.0) * F
        K = keep.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            delta_c = (p * ((np.abs(a) + np.abs(c)[:, None]) * r + 2.0 * F * np.abs(a))).sum(axis=1) \
                + np.where(Z > 0, (1.0 + np.abs(c)) * K * 2.0 ** -40 / Z, 0.0)
        err_d = delta_c + 2.0 * F * (np.abs(c) + np.where(np.isfinite(D), D, 0.0) + 1.0)
        mg["err_d"] = err_d
        mg["b_need"] = np.maximum(MARGIN, 4.0 * err_d)
        if mutation == "boundary_dropped":
            keep = keep & ((order < D[:, None]) | (order == order.min(axis=1)[:, None]))
        else:
            keep = keep & (order <= D[:, None])
    before_eps = keep
    top = np.where(keep, t, -np.inf).max(axis=1)                              # the survivors' maximum: steps 8 and 9 never remove it
    if mutation == "exempt_row_max":
        top = tmax
    eps = _f32(epsilon_cutoff)
    if eps > 0.0:
        _, _, p = probs(keep)
        mg["c"] = np.where(keep, np.abs(p - eps) / eps, np.inf).min(axis=1)
        keep = keep & ((p >= eps) | (t == top[:, None]))
    eta = _f32(eta_cutoff)
    if eta > 0.0:
        _, _, p = probs(keep)
        if mutation == "entropy_not_renormalised":
            H = entropy(np.where(keep, p0, 0.0))
        elif mutation == "entropy_before_epsilon":
            H = entropy(probs(before_eps)[2])
        else:
            H = entropy(p)
        theta = np.minimum(eta, np.sqrt(eta) * np.exp(-H))
        mg["d"] = np.where(keep, np.abs(p - theta[:, None]) / theta[:, None], np.inf).min(axis=1)
        keep = keep & ((p >= theta[:, None]) | (t == top[:, None]))
    return (keep, mg) if want_margin else keep


def margins_hold(mg):
    """per row: do the four margins of kept_truncated hold"""
    return (mg["a"] >= MARGIN) & (mg["b"] >= mg["b_need"]) & (mg["c"] >= MARGIN) & (mg["d"] >= MARGIN)


def case_kept(case, logits, hist, want_margin=False, mutation=None):
    """steps 1-9 of a case on bf16 logits -> (t fp32, kept0, kept) (+ the step 4-6 margins and the margins of steps 7-9)"""
    t, key = S.case_scores(case, logits, hist)
    k0, m_p, m_min = S.case_kept(case, t, key, True)
    out = kept_truncated(t, k0, want_margin=want_margin, mutation=mutation, **truncation_args(case))
    return (t, k0, out[0], m_p, m_min, out[1]) if want_margin else (t, k0, out)


class Reference(S.Reference):
    """S.Reference of a case (steps 1-6: kept set `kept0`, its margins, eps) moved onto the truncated kept set: p, C and eps are
    S.Reference's own expressions evaluated on `kept`, with a still measured from the row maximum t_max, as the kernel's masses are."""

    def __init__(self, case, logits, hist):
        super().__init__(case, logits, hist)
        t = np.asarray(S.case_scores(case, logits, hist)[0], dtype=np.float64)
        self.kept0 = self.kept
        self.kept, self.margins = kept_truncated(t, self.kept0, want_margin=True, **truncation_args(case))
        tmax = S._tmax(t)
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
        self.eps = 2.0 * ((p * (2.0 * np.abs(a) + 8.0)).sum(axis=1) * F + (K + 1) * 2.0 ** -40)      # S.Reference's chain eps, unchanged


@functools.lru_cache(maxsize=None)
def rows_for(V, profile, rows=ROWS):
    """(bf16 logits [rows, V], int64 history [rows, S.HIST_LEN]) of a (V, profile): S._make_row(V, profile, r, salt) with salt
    0, 1, ... per row until every margin holds under every setting of SETTINGS (at most 64 salts; none may be left)."""
    x = np.empty((rows, V), dtype=np.float32)
    h = np.empty((rows, S.HIST_LEN), dtype=np.int64)
    todo = np.arange(rows)
    settings = [dict(kernel="chain", V=V, ld=V, profile=profile, setting=n, **s) for n, s in SETTINGS.items()]
    for salt in range(64):
        for r in todo:
            x[r], h[r] = S._make_row(V, profile, int(r), salt)
        lg = torch.from_numpy(x[todo]).to(torch.bfloat16)
        hh = torch.from_numpy(h[todo])
        bad = np.zeros(len(todo), dtype=bool)
        for c in settings:
            _, _, _, m_p, m_min, mg = case_kept(c, lg, hh, True)
            bad |= (m_p < MARGIN) | (m_min < MARGIN) | ~margins_hold(mg)
        REDRAWN[(V, profile, salt)] = int(bad.sum())
        todo = todo[bad]
        if len(todo) == 0:
            break
    assert len(todo) == 0, (V, profile, todo)
    return torch.from_numpy(x).to(torch.bfloat16), torch.from_numpy(h)


REDRAWN = {}        # (V, profile, salt) -> rows that missed a margin at that salt


@functools.lru_cache(maxsize=1)
def _reference(V, profile, setting):
    case = next(c for c in CASES if (c["V"], c["profile"], c["setting"]) == (V, profile, setting))
    return Reference(case, *rows_for(V, profile))


def reference(case):
    """The Reference of a table case (the last one is cached; the ld variants of one V share it, so run them back to back)."""
    return _reference(case["V"], case["profile"], case["setting"])
