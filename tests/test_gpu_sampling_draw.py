"""GPU: the token the decoding kernels pick, held to a float64 inverse-CDF reference at real vocabulary sizes.

`desta_sample_bf16` (sample_chain_k / sample_greedy_k), `desta_sample_top_p_bf16` (sample_top_p_k) and `desta_argmax_bf16`.
Reference, allowance `eps` with its derivation, conforming emulation, mutations and the shared case table: tests/sampling_reference.py;
the instrument is proved on the CPU by tests/test_sampling_draw_host.py.  Table: (V, ld) = (4099, 4101) (rows off 16-byte
alignment: the scalar paths), (4099, 4104) (vector body + scalar tail), (128256, 128256), (151936, 151944); profiles randn,
two_spike, peaked, suppressed, flat, flat_suppressed; five chain settings and three (T, top_p) of the top-p kernel; 64 rows per
launch x steps {0, 1, 2^31, 2^32 - 1} x seeds {99, (7 << 32) | 5}.  Columns [V, ld) hold +60, above every logit.

  1. flat rows: every pick equals the closed form (sampling_reference.flat_pick) bit for bit: no tolerance.  This pins rng32 on the
     host to the device, the counter (step << 32) | row, both seed words through the binding, the 24-bit uniform, the
     index-order prefix over all 16 waves and the chunk geometry.
  2. every other case: keep_mask == kept() exactly (the rows keep 1e-4 from every cut-off) and every draw has
     ratio = max(C_lo - u, u - C_hi, 0) / eps <= 1.  For the top-p kernel's cases the chain kernel, given the same (T, top_p), has the
     same keep_mask.
  3. a -inf entry is never kept and never drawn; 4. a row of -inf alone gives a token in [0, V) (0 from the chain kernel);
  5. desta_argmax_bf16 == torch.argmax == greedy desta_sample_bf16 at every (V, ld), 1 and 64 rows; 6. signed zeros at the top-p
     boundary.

Measured on the MI355X (largest ratio per kernel and vocabulary; profiles/r23_sampling_draw_fp64_tests.log, DESIGN.md "Token picks
against fp64"):
    chain kernel   V = 4099: 0          V = 128256: 0        V = 151936: 0        (eps about 2e-6: no draw came that close to a boundary)
    top-p kernel   V = 4099: 0.00029    V = 128256: 0.0022   V = 151936: 0.0060   (eps 1.3e-4 ... 1.4e-4; the emulation: 0, 0.0022, 0.0060)

Predictions of the issue, checked against the library of the parent commit (same log):
    held      desta_argmax_bf16 ordered -0.0 below +0.0 and returned the later index (test 5, every (V, ld));
    held      the top-p kernel's bf16_key did the same: the two -0.0 logits at the boundary were dropped (test 6, 16 entries);
    held      with every filter off the chain kernel marked -inf entries as kept (tests 2, 3), and so did the top-p kernel at top_p = 1;
    held      a row of -inf alone gave -1 from the top-p kernel at top_p < 1 (V - 1 at top_p = 1, inside [0, V)); the chain kernel
              and argmax gave 0 as documented (test 4), the chain kernel's mask held all of the row.
All four are fixed in this change (zero fold in both keys, -inf never kept, token 0 for a row without a finite score)."""
import numpy as np
import pytest
import torch

import sampling_reference as S

pytestmark = pytest.mark.gpu

PAD = 60.0
DRAWS = [(seed, step) for seed in S.SEEDS for step in S.STEPS]
WORST = {}


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _buf(logits, ld):
    """bf16 [rows, ld] on the device (16-byte aligned base), columns [V, ld) above every logit"""
    rows, V = logits.shape
    buf = torch.full((rows, ld), PAD, dtype=torch.bfloat16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[:, :V] = logits.cuda()
    return buf


def _launch(hip, case, buf, hist, seed, step, mask=True, kernel=None):
    rows, V, ld = buf.shape[0], case["V"], buf.shape[1]
    out = torch.full((rows,), -7, dtype=torch.int64, device="cuda")
    m = torch.full((rows, V), 3, dtype=torch.uint8, device="cuda") if mask else None
    if (kernel or case["kernel"]) == "chain":
        pen = case.get("penalty", 1.0)
        hip.sample(buf, ld, rows, V, out, temperature=case["T"], top_k=case.get("top_k", 0), top_p=case.get("top_p", 1.0),
                   min_p=case.get("min_p", 0.0), repetition_penalty=pen, hist=hist if pen != 1.0 else None,
                   hist_len=hist.shape[1] if pen != 1.0 else 0, seed=seed, step=step, keep_mask=m)
    else:
        hip.sample_top_p(buf, ld, rows, V, case["T"], case["top_p"], seed, step, out, keep_mask=m)
    return out.cpu().numpy(), m


def _is_flat(case):
    return case["profile"] in S.FLAT and case.get("penalty", 1.0) == 1.0


_ORDERED = sorted(S.CASES, key=lambda c: (c["V"], c["profile"], S.ref_id(c), c["ld"]))      # one reference per pair of ld variants
FLAT_CASES = [c for c in _ORDERED if _is_flat(c)]
OTHER_CASES = [c for c in _ORDERED if not _is_flat(c)]


# ------------------------------------------------------------------------------------------------ 1. exact draws
@pytest.mark.parametrize("case", FLAT_CASES, ids=S.case_id)
def test_flat_rows_draw_the_closed_form(hip, case):
    logits, hist = S.rows_for(case["V"], case["profile"])
    ref = S.reference(case)
    buf = _buf(logits, case["ld"])
    want_mask = torch.from_numpy(ref.kept.astype(np.uint8)).cuda()
    idx = [np.flatnonzero(ref.kept[r]) for r in range(S.ROWS)]
    assert all(len(i) == int(torch.isfinite(logits[r].float()).sum()) for r, i in enumerate(idx))      # a flat row keeps its finite entries
    for seed, step in DRAWS:
        tok, mask = _launch(hip, case, buf, hist.cuda(), seed, step)
        assert torch.equal(mask, want_mask), (S.case_id(case), seed, step)
        u = S.u24_rows(seed, step)
        want = [S.flat_pick(case["kernel"], ref.kept[r], int(u[r])) for r in range(S.ROWS)]
        assert tok.tolist() == want, (S.case_id(case), seed, step)


# ------------------------------------------------------------------------------------------------ 2. interval check
@pytest.mark.parametrize("case", OTHER_CASES, ids=S.case_id)
def test_every_draw_inverts_the_fp64_cdf(hip, case):
    logits, hist = S.rows_for(case["V"], case["profile"])
    ref = S.reference(case)
    buf = _buf(logits, case["ld"])
    hist_d = hist.cuda()
    want_mask = torch.from_numpy(ref.kept.astype(np.uint8)).cuda()
    rr = np.arange(S.ROWS)
    worst = 0.0
    for seed, step in DRAWS:
        tok, mask = _launch(hip, case, buf, hist_d, seed, step)
        assert torch.equal(mask, want_mask), (S.case_id(case), seed, step, int((mask != want_mask).sum()))
        assert bool(((tok >= 0) & (tok < case["V"])).all())
        assert bool(ref.kept[rr, tok].all()), (S.case_id(case), seed, step)
        ratio = S.ratio(case, tok, S.u24_rows(seed, step))
        worst = max(worst, float(ratio.max()))
        assert float(ratio.max()) <= 1.0, (S.case_id(case), seed, step, int(ratio.argmax()), float(ratio.max()))
    key = (case["kernel"], case["V"])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"\n{S.case_id(case)}: largest ratio {worst:.3g} (eps {float(ref.eps.max()):.3g})", end="")
    if case["kernel"] == "top_p":                                            # 6. the chain kernel keeps the same set
        _, mask = _launch(hip, case, buf, hist_d, 99, 0, kernel="chain")
        assert torch.equal(mask, want_mask), S.case_id(case)


def test_report_largest_ratios():
    for (kernel, V), w in sorted(WORST.items()):
        print(f"\nlargest ratio {kernel} V={V}: {w:.3g}", end="")


# ------------------------------------------------------------------------------------------------ 3. suppressed entries
@pytest.mark.parametrize("kernel,setting", [("chain", "T"), ("top_p", "T1.0_p1.0")])
def test_suppressed_entries_are_neither_kept_nor_drawn(hip, kernel, setting):
    """every filter off: the kept set is the finite entries (the tokens that can be drawn), as the header says"""
    V, ld = S.VLD[0]
    case = S.CASE_BY_ID[f"{kernel}-V{V}-ld{ld}-suppressed-{setting}"]
    logits, hist = S.rows_for(V, "suppressed")
    finite = torch.isfinite(logits.float())
    assert bool((~finite).any(1).all()) and np.array_equal(S.reference(case).kept, finite.numpy())
    buf = _buf(logits, ld)
    for seed, step in DRAWS:
        tok, mask = _launch(hip, case, buf, hist.cuda(), seed, step)
        assert torch.equal(mask.cpu().bool(), finite), (kernel, int((mask.cpu().bool() != finite).sum()))
        assert bool(finite[torch.arange(S.ROWS), torch.from_numpy(tok)].all())


# ------------------------------------------------------------------------------------------------ 4. no finite score
@pytest.mark.parametrize("V,ld", [S.VLD[0], S.VLD[2]])
def test_rows_without_a_finite_score(hip, V, ld):
    rows = 4
    logits = torch.full((rows, V), float("-inf"), dtype=torch.bfloat16)
    buf = _buf(logits, ld)
    hist = torch.zeros(rows, 4, dtype=torch.int64, device="cuda")
    for s in list(S.CHAIN_SETTINGS.values()):
        tok, mask = _launch(hip, dict(kernel="chain", V=V, **s), buf, hist, 99, 1)
        assert tok.tolist() == [0] * rows, s
        assert int(mask.sum()) == 0, s
    for s in S.TOP_P_SETTINGS.values():
        tok, mask = _launch(hip, dict(kernel="top_p", V=V, **s), buf, hist, 99, 1)
        assert bool(((tok >= 0) & (tok < V)).all()), (s, tok)
        assert int(mask.sum()) == 0, s
    out = torch.full((rows,), -7, dtype=torch.int64, device="cuda")
    hip.argmax_bf16(buf, ld, rows, V, out)
    assert out.cpu().tolist() == [0] * rows
    out.fill_(-7)
    hip.sample(buf, ld, rows, V, out, do_sample=False)
    assert bool(((out >= 0) & (out < V)).all())


# ------------------------------------------------------------------------------------------------ 5. argmax at real shapes
ARGMAX_KINDS = ("tie_5_40", "last_column", "first_column", "plain", "all_negative", "suppressed", "neg_zero_first", "pos_zero_first")


def _argmax_rows(V, rows):
    """row r is of kind r % 8; slices are the 64 column slices of argmax_part_k (ceil(V / 64) wide)"""
    per = (V + 63) // 64
    g = torch.Generator().manual_seed(V)
    x = torch.randn(rows, V, generator=g)
    for r in range(rows):
        kind = ARGMAX_KINDS[r % len(ARGMAX_KINDS)]
        a, b = 5 * per + 3 + r % 7, 40 * per + 7 + r % 5
        if kind == "tie_5_40":
            x[r, a] = x[r, b] = 9.0
        elif kind == "last_column":
            x[r, V - 1] = 9.0
        elif kind == "first_column":
            x[r, 0] = 9.0
        elif kind == "all_negative":
            x[r] = -x[r].abs() - 0.5
        elif kind == "suppressed":
            x[r, torch.from_numpy(S._suppress_mask(np.random.default_rng(r), V))] = float("-inf")
            x[r, int(x[r].argmax())] = float("-inf")
        elif kind in ("neg_zero_first", "pos_zero_first"):
            x[r] = -x[r].abs() - 0.5
            x[r, a], x[r, b] = (-0.0, 0.0) if kind == "neg_zero_first" else (0.0, -0.0)
    return x.to(torch.bfloat16)


@pytest.mark.parametrize("V,ld", S.VLD)
def test_argmax_and_greedy_sample_at_real_shapes(hip, V, ld):
    x = _argmax_rows(V, S.ROWS)
    want = x.float().argmax(-1)
    per = (V + 63) // 64
    assert int(want[0]) == 5 * per + 3 and int(want[1]) == V - 1 and int(want[2]) == 0
    assert bool(torch.signbit(x[6, want[6]].float())) and not bool(torch.signbit(x[7, want[7]].float()))     # the earlier zero, whatever its sign
    for rows, sel in [(S.ROWS, slice(None))] + [(1, slice(k, k + 1)) for k in range(len(ARGMAX_KINDS))]:
        buf = _buf(x[sel], ld)
        out = torch.full((rows,), -7, dtype=torch.int64, device="cuda")
        hip.argmax_bf16(buf, ld, rows, V, out)
        assert out.cpu().tolist() == want[sel].tolist(), ("argmax", V, ld, rows, sel)
        out.fill_(-7)
        hip.sample(buf, ld, rows, V, out, do_sample=False, repetition_penalty=1.0)
        assert out.cpu().tolist() == want[sel].tolist(), ("greedy sample", V, ld, rows, sel)


# ------------------------------------------------------------------------------------------------ 6. signed zeros at the boundary
def test_signed_zeros_tie_at_the_top_p_boundary(hip):
    """One token at 2.0, twenty at zero (two of them -0.0, the rest +0.0), the rest at -20; T = 1, top_p = 0.9.  The cut-off
    0.1 Z = 2.74 lies above the mass of the two -0.0 tokens (2) and below that of the zeros together (20): a key that orders -0.0
    below +0.0 drops the two, although they tie with the boundary logit."""
    V, ld, rows = 4099, 4104, 8
    x = torch.full((rows, V), -20.0)
    for r in range(rows):
        z = torch.arange(20) * 200 + 10 + r
        x[r, z] = 0.0
        x[r, z[[3, 11]]] = -0.0
        x[r, 4000 + r] = 2.0
    x = x.to(torch.bfloat16)
    case = dict(kernel="top_p", V=V, ld=ld, T=1.0, top_p=0.9)
    ref = S.Reference(case, x, None)
    assert float(ref.margin_top_p.min()) >= S.MARGIN and ref.kept.sum(1).tolist() == [21] * rows
    buf = _buf(x, ld)
    want = torch.from_numpy(ref.kept.astype(np.uint8)).cuda()
    for kernel in ("top_p", "chain"):
        kref = S.Reference(dict(case, kernel=kernel), x, None)
        assert np.array_equal(kref.kept, ref.kept)
        for seed, step in DRAWS:
            tok, mask = _launch(hip, case, buf, None, seed, step, kernel=kernel)
            assert torch.equal(mask, want), (kernel, int((mask != want).sum()))
            ratio = kref.ratio(tok, S.u24_rows(seed, step, rows))
            assert float(ratio.max()) <= 1.0, (kernel, seed, step, float(ratio.max()))
