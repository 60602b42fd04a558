"""CPU: the instrument of test_gpu_sampling_draw.py proved on the host (tests/sampling_reference.py: the float64 inverse-CDF
reference, its allowance `eps`, the conforming emulation of both samplers and the seeded mutations).

  * the inputs: over the whole case table every row keeps MARGIN = 1e-4 from the top-p cut-off and 1e-4 (relative) from min_p,
    so the reference kept set is unambiguous;
  * the check passes a correct kernel: the conforming emulation picks a kept token with ratio <= 1 on every draw of every case
    (64 rows x 4 steps x 2 seeds), and on flat rows it equals the closed forms bit for bit;
  * the check has power: every mutation is caught in at least one case of the table, by the interval check with a ratio of
    at least 10, or by the exact flat-row prediction (run with -s for the case that caught each);
  * why it exists: at V = 64, the shape of test_gpu_sampling.py::test_full_chain_distribution_and_reproducibility, a sampler whose
    waves each start their prefix at 0, or whose prefix runs in row_strided's order, draws exactly the tokens of a correct one.

`rng32` has no second restatement on the host (no host test of this suite compiles a C program); it is pinned to the device
by the flat rows of test_gpu_sampling_draw.py, where every pick is an exact function of u24."""
import concurrent.futures

import numpy as np
import pytest
import torch

import sampling_reference as S

VS = sorted({V for V, _ in S.VLD})
DRAWS = [(seed, step) for seed in S.SEEDS for step in S.STEPS]


def _cases(V, profile):
    return [c for c in S.CASES if c["V"] == V and c["profile"] == profile]


def _is_flat(case):
    return case["profile"] in S.FLAT and case.get("penalty", 1.0) == 1.0


def _flat_picks(case, ref, u):
    return np.array([S.flat_pick(case["kernel"], ref.kept[r], int(u[r])) for r in range(S.ROWS)])


def _check_conforming(case):
    """margins, then every draw of the conforming emulation against the reference -> largest ratio"""
    rr = np.arange(S.ROWS)
    ref, em = S.Reference(case), S.Emulation(case)
    m_p, m_min = ref.margin_top_p, ref.margin_min_p
    assert float(m_p.min()) >= S.MARGIN and float(m_min.min()) >= S.MARGIN, (S.case_id(case), float(m_p.min()), float(m_min.min()))
    assert bool(ref.finite_rows.all())
    worst = 0.0
    for seed, step in DRAWS:
        u = S.u24_rows(seed, step)
        tok = em.draw(u)
        assert bool(ref.kept[rr, tok].all()), (S.case_id(case), seed, step)
        ratio = ref.ratio(tok, u)
        worst = max(worst, float(ratio.max()))
        assert float(ratio.max()) <= 1.0, (S.case_id(case), seed, step, int(ratio.argmax()), float(ratio.max()))
        if _is_flat(case):
            assert tok.tolist() == _flat_picks(case, ref, u).tolist(), (S.case_id(case), seed, step)
    return worst


@pytest.mark.parametrize("profile", S.PROFILES)
@pytest.mark.parametrize("V", VS)
def test_margins_and_conforming_emulation(V, profile):
    S.rows_for(V, profile)
    cases = _cases(V, profile)
    with concurrent.futures.ThreadPoolExecutor(4) as pool:                # numpy releases the GIL: the cases are independent
        worst = list(pool.map(_check_conforming, cases))
    by_kernel = {k: max(w for c, w in zip(cases, worst) if c["kernel"] == k) for k in ("chain", "top_p")}
    print(f"\nconforming emulation V={V} {profile}: largest ratio " + " ".join(f"{k} {v:.3g}" for k, v in sorted(by_kernel.items())), end="")


def _caught(case, mutation):
    """-> (detector, figure) if the mutation shows in this case, else None"""
    ref = S.reference(case)
    worst, wrong = 0.0, 0
    for seed, step in DRAWS:
        u = S.u24_rows(seed, step)                                        # the contract's uniform, whatever the mutated kernel used
        tok = S.emulate(case, case["kernel"], seed, step, mutation=mutation)
        if _is_flat(case):
            wrong += int((tok != _flat_picks(case, ref, u)).sum())
        else:
            worst = max(worst, float(S.ratio(case, tok, u).max()))
    if wrong:
        return "flat-row prediction", wrong
    if worst >= 10.0:                                                     # a condition on the choice of inputs, not a tolerance
        return "interval check", worst
    return None


@pytest.mark.parametrize("mutation", list(S.MUTATIONS))
def test_every_mutation_is_caught(mutation):
    small = [c for c in S.CASES if c["V"] == VS[0]]
    large = [c for c in S.CASES if c["V"] == VS[1] and c["profile"] == "randn"]
    order = {"randn": 0, "peaked": 1, "two_spike": 2, "suppressed": 3, "flat": 4, "flat_suppressed": 5}
    pref = "full" if mutation in ("penalty_per_occurrence", "unpenalised_mass") else "T"
    cands = sorted(small, key=lambda c: (c["setting"] != pref, order[c["profile"]])) + large
    for case in cands:
        if case["kernel"] not in S.MUTATIONS[mutation]:
            continue
        hit = _caught(case, mutation)
        if hit:
            print(f"\n{mutation}: caught in {S.case_id(case)} by the {hit[0]} ({hit[1]:.3g})", end="")
            return
    raise AssertionError(f"{mutation} is caught by no case of the table")


def test_rng_restatement_is_sensitive_to_every_input():
    """row, step (both halves of the counter), both seed words and the bit selection all reach u24"""
    base = [S.u24(99, 5, r) for r in range(64)]
    assert len(set(base)) == 64 and all(0 <= u < 1 << 24 for u in base)
    assert [S.u24(99, 6, r) for r in range(64)] != base
    assert [S.u24(99 | (1 << 32), 5, r) for r in range(64)] != base
    assert [S.u24(98, 5, r) for r in range(64)] != base
    assert S.u24(99, 1, 0) != S.u24(99, 0, 1)                             # step is not added to the row
    for m in ("u_low_bits", "row_ignored", "step_low_word", "seed_hi_dropped"):
        got = [S.u24((7 << 32) | 5, 2 ** 32 - 1, r, m) for r in range(64)]
        assert got != [S.u24((7 << 32) | 5, 2 ** 32 - 1, r) for r in range(64)], m
    # the counter's high word enters through an odd multiplier, so step 2^31 alone lands where the low word would put it
    assert S.u24(99, 2 ** 31, 3, "step_low_word") == S.u24(99, 2 ** 31, 3)
    assert S.u24(99, 0, 0, "seed_hi_dropped") == S.u24(99, 0, 0)          # seed 99 has no high word: only the second seed sees it


def test_v64_statistics_cannot_see_the_prefix_mutations():
    """The inputs and the criterion of test_gpu_sampling.py::test_full_chain_distribution_and_reproducibility (V = 64, 20000 draws,
    5 sigma per token), on the emulation: threads 0..7 of wave 0 hold the whole row, so both prefix mutations draw the
    conforming tokens, draw for draw, and the criterion passes them."""
    V, n, rows = 64, 20000, 8
    g = torch.Generator().manual_seed(2)
    logits = (torch.randn(1, V, generator=g) * 2).to(torch.bfloat16).repeat(rows, 1)
    hist = torch.tensor([[3, 3, 9, 17, 40]]).repeat(rows, 1)
    case = dict(kernel="chain", V=V, ld=V + 8 - V % 8, T=0.8, top_k=20, top_p=0.95, min_p=0.01, penalty=1.3)
    ref = S.Reference(case, logits, hist)
    us = [S.u24_rows(99, step, rows) for step in range(n // rows)]
    picks = {}
    for mutation in (None, "wave_prefix_dropped", "strided_order"):
        em = S.Emulation(case, mutation, logits, hist)
        picks[mutation] = np.concatenate([em.draw(u) for u in us])
    q = torch.from_numpy(ref.p[0])
    for mutation in ("wave_prefix_dropped", "strided_order"):
        assert picks[mutation].tolist() == picks[None].tolist(), mutation
        counts = torch.bincount(torch.from_numpy(picks[mutation]), minlength=V).double()
        assert counts[~torch.from_numpy(ref.kept[0])].sum() == 0
        freq = counts / counts.sum()
        sigma = torch.sqrt(q * (1 - q) / n)
        assert bool(((freq - q).abs() <= 5 * sigma + 1e-4).all()), mutation      # the V = 64 test is green on both
    assert float(max(ref.ratio(picks[None][i * rows:(i + 1) * rows], us[i]).max() for i in range(0, n // rows, 50))) <= 1.0
