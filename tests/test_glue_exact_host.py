"""Host (no GPU): the instrument of tests/test_gpu_glue_exact.py is proved before it is pointed at a kernel.

Over the SAME case table the GPU test runs (glue_reference.CASES) and under the SAME comparison rule (glue_reference.mismatch):
  (a) every kernel-shaped emulation equals its plainly written reference on every case (the random-data colsum cases: inside
      1 x the bound, worst ratio printed with -s);
  (b) every seeded mutation of an emulation (glue_reference.MUTANTS) is rejected by at least one case of each operation it
      applies to; the cases are printed.  `lane_stride_256` is the exception and is asserted as such: with a lane stride of 256
      every vector is copied twice, which changes no output, so no case can (or should) catch it;
  (c) for every mutation, whether the shapes tests/test_gpu_ops.py runs these kernels at would have shown it.  Those shapes and
      criteria are rebuilt here (`_old_cases`; the GPU test is not imported): the old tests look at the output alone (no guard),
      at rtol / atol for the column sums, and have no direct test of mask_tokens.  `OLD_SEES` pins the outcome per operation;
      nothing is forced: `per = M / 1024` IS seen at the old 5 x 37 grid (per = 0 there, nothing is found), the late reduce tail
      IS seen at 1000 x 136 (125 partial rows: wave groups 13-15 have a tail), a lane stride of 1024 is NOT seen by embed_gather
      at hidden = 256 but IS by the gather / scatter of the 1000-wide logits rows, and the dropped shift guard is NOT seen,
      although per = 1 there: the old labels start every sequence with -100, so labels[b + 1, 0] is never a target.  What an
      operation's old shapes let through, a case of the new table catches (asserted);
  (d) the integer-data condition of the exact colsum rule, from the table: rows * 8 + 64 < 2^24; and the rounding count of the
      random-data bound: colsum_roundings (walked) <= colsum_chain (the formula) for every case."""
import math

import pytest
import torch

import glue_reference as R

_CACHE = {}


def _case(op, i):
    """(operands, reference, emulation) of case i of op, computed once and left unchanged"""
    if (op, i) not in _CACHE:
        o = R.operands(op, R.CASES[op][i])
        _CACHE[(op, i)] = (o, R.reference(op, o), R.emulate(op, o))
    return _CACHE[(op, i)]


@pytest.mark.parametrize("op", R.OPS)
def test_emulation_equals_reference(op):
    worst = (-1.0, "")
    for i, case in enumerate(R.CASES[op]):
        o, ref, emu = _case(op, i)
        assert R.mismatch(op, o, ref, emu) is None, (op, R.case_id(case), R.mismatch(op, o, ref, emu))
        if op == "colsum" and case["data"] == "randn":
            worst = max(worst, (R.colsum_ratio(o, ref, emu), R.case_id(case)))
    print(f"\n{op}: {len(R.CASES[op])} cases, emulation == reference" +
          (f"; worst |err| / bound {worst[0]:.4f} at {worst[1]}" if op == "colsum" else ""))


def test_colsum_conditions_from_the_table():
    for case in R.CASES["colsum"]:
        rows, cols = case["rows"], case["cols"]
        assert rows * 8 + 64 < 2 ** 24, case                      # |partial sum| <= 8 rows, |prev| <= 50: integers fp32 holds
        assert R.colsum_roundings(rows, cols) <= R.colsum_chain(rows, cols), case
    nrs = sorted({R.colsum_splits(c["rows"], c["cols"]) for c in R.CASES["colsum"]})
    print(f"\ncolsum splits in the table: {nrs}; chains L: {sorted({R.colsum_chain(c['rows'], c['cols']) for c in R.CASES['colsum']})}")
    assert set(nrs) >= {1, 2, 15, 16, 17, 48, 49, 63, 64, 65, 112, 113, 512}
    # both vector widths, and V = 4 for each of its three reasons
    v = {(c["cols"] % 8 == 0, c["ld"] % 8 == 0, c["off"] % 8 == 0) for c in R.CASES["colsum"]}
    assert {(True, True, True), (False, True, True), (True, False, True), (True, True, False)} <= v


def _catchers(mut, op):
    hits = []
    for i, case in enumerate(R.CASES[op]):
        o, ref, _ = _case(op, i)
        if R.mismatch(op, o, ref, R.emulate(op, o, mut)) is not None:
            hits.append(R.case_id(case))
    return hits


@pytest.mark.parametrize("mut", list(R.MUTANTS))
def test_mutant_is_caught(mut):
    ops, what = R.MUTANTS[mut]
    for op in ops:
        hits = _catchers(mut, op)
        print(f"\n{mut} ({what}) on {op}: caught by {len(hits)} of {len(R.CASES[op])} cases: {' '.join(hits) if hits else '-'}")
        if mut in R.EQUIVALENT:
            assert not hits, (mut, op, hits)                       # an equivalent mutant: every output is the reference's
        else:
            assert hits, (mut, op)


# ------------------------------------------------------------------------------------- the shapes of tests/test_gpu_ops.py
def _old_cases(op):
    """operands at the shapes (and label / index patterns) test_gpu_ops.py runs `op` at today"""
    if op == "embed_gather":                                        # test_embed_gather_and_rows
        g = torch.Generator().manual_seed(5)
        return [dict(rows=7, hidden=256, table=R._rows16(g, 50, 256), audio=R._rows16(g, 6, 256),
                     src=torch.tensor([3, 49, -1, -2, -6, 0, 7], dtype=torch.int32))]
    if op == "gather_rows":
        g = torch.Generator().manual_seed(6)
        old = [dict(rows=3, hidden=256, x=R._rows16(g, 7, 256), src=torch.tensor([6, 0, 2], dtype=torch.int32))]
        s = _old_cases("scatter_rows")[0]                           # and the target rows of the 1000-wide logits
        return old + [dict(rows=s["rows"], hidden=1000, x=R._rows16(g, 5 * 37, 1000), src=s["src"])]
    if op == "scatter_rows":                                        # test_target_rows_and_scatter: the target rows, V = 1000
        t = R.operands("target_rows", dict(B=5, S=37, labels="old", s_major=0))
        ref = R.reference("target_rows", t)
        n = int(ref["count"][0])
        g = torch.Generator().manual_seed(7)
        return [dict(rows=n, hidden=1000, x=R._rows16(g, n, 1000), src=ref["idx"][:n].clone(), out_rows=5 * 37)]
    if op == "target_rows":
        return [R.operands(op, dict(B=5, S=37, labels=p, s_major=sm)) for p, sm in (("old", 0), ("old", 1), ("none", 0))]
    if op == "colsum":                                              # test_colsum_transpose_cast_add, without 48000 x 2560
        shapes = [(1000, 136, 136, 0), (1000, 136, 136, 1), (2048, 3840, 3840, 0), (4097, 132, 140, 0), (5, 8, 8, 0),
                  (33, 1280, 2560, 0)]
        return [R.operands(op, dict(rows=r, cols=c, ld=ld, off=0, accumulate=a, data="randn")) for r, c, ld, a in shapes]
    if op == "transpose":                                           # the same test, without 48000 x 256
        shapes = [(1000, 136, 136, 1024, 0), (70, 200, 200, 128, 1), (2048, 1280, 3840, 2048, 0)]
        return [R.operands(op, dict(rows=r, cols=c, ld_out=lo, ld_in=li, f32=f)) for r, c, li, lo, f in shapes]
    if op == "cast":
        return [R.operands(op, dict(n=70 * 200))]
    return []                                                       # mask_tokens: no direct test


def _old_sees(op, o, ref, got):
    """would the criterion of test_gpu_ops.py notice `got`?  It looks at the output alone: no guard, no sentinel behind it."""
    if op == "colsum":                                              # assert_close(rtol, atol) of the old test
        a, b = got["out"][:o["cols"]].double(), ref["out"][:o["cols"]].double()
        rtol, atol = (1e-4, 2e-3 if o["accumulate"] else 1e-3) if o["rows"] == 1000 else (2e-4, 2e-3 * math.sqrt(o["rows"] / 1000))
        return bool(((a - b).abs() > atol + rtol * b.abs()).any())
    if op == "target_rows":
        n = int(ref["count"][0])
        return not (torch.equal(got["count"][:2], ref["count"][:2]) and torch.equal(got["idx"][:n], ref["idx"][:n])
                    and torch.equal(got["lab"][:n + 2], ref["lab"][:n + 2]))
    cut = {k: v[:v.numel() - R.GUARD - (2 * o["ld_out"] if op == "transpose" else 0)] for k, v in got.items()}
    exp = {k: v[:v.numel() - R.GUARD - (2 * o["ld_out"] if op == "transpose" else 0)] for k, v in ref.items()}
    return R.mismatch(op, o, exp, cut) is not None


# mutation -> the operations whose old shapes show it (None: the kernel has no direct test in test_gpu_ops.py)
_ALL = R.MOVERS
OLD_SEES = {
    "lane_stride_256": (), "lane_stride_1024": ("gather_rows", "scatter_rows"),      # the 1000-wide logits rows, not hidden = 256
    "last_chunk_skipped": _ALL, "no_row_test": (), "audio_minus_s": ("embed_gather",), "scatter_to_row": ("scatter_rows",),
    "no_shift_guard": (), "per_floor": ("target_rows",), "first_from_row": (), "s_major_swapped": ("target_rows",),
    "no_trailing_label": ("target_rows",),
    "mask_div_mod_swapped": None, "mask_bound_ld": None, "mask_plus_inf": None,
    "reduce_tail_late": ("colsum",), "reduce_64_no_tail": ("colsum",), "last_partial_dropped": ("colsum",), "v8_on_4": (),
    "accumulate_ignored": ("colsum",),
    "no_tail_tiles": (), "vec_tail_rows": ("transpose",), "f32_truncated": ("transpose", "cast"),
}
_OLD = {}


def _old(op):
    if op not in _OLD:
        _OLD[op] = [(o, R.reference(op, o)) for o in _old_cases(op)]
    return _OLD[op]


@pytest.mark.parametrize("mut", list(R.MUTANTS))
def test_what_the_old_shapes_see(mut):
    ops, what = R.MUTANTS[mut]
    seen, tested = {}, False
    for op in ops:
        for o, ref in _old(op):
            tested = True
            if op == "colsum" and _old_sees(op, o, ref, R.emulate(op, o)):
                pytest.fail(f"the emulation itself misses the old criterion at {o['rows']} x {o['cols']}")
            if _old_sees(op, o, ref, R.emulate(op, o, mut)):
                seen.setdefault(op, []).append(" x ".join(str(o[k]) for k in ("B", "S", "rows", "hidden", "cols", "n") if k in o))
    blind = [op for op in ops if op not in seen]
    verdict = "no direct test" if not tested else "; ".join(
        [f"SEEN by {op} at {', '.join(v)}" for op, v in seen.items()] + ([f"not seen by {' '.join(blind)}"] if blind else []))
    print(f"\n{mut} ({what}): old shapes: {verdict}")
    assert (tuple(op for op in ops if op in seen) if tested else None) == OLD_SEES[mut], (mut, verdict)
    if mut not in R.EQUIVALENT:                                     # what the old shapes let through, a new case catches
        assert all(_catchers(mut, op) for op in blind)
