"""Host (no GPU): the per-element fp64 criterion of tests/adafactor_reference.py is proved before it is pointed at the kernel.

Over the SAME case table the GPU test runs (adafactor_reference.CASES; three steps each, step k + 1 from the emulation's own fp32
results of step k, every element of every output):
  (a) the conforming emulation stays inside the bound (worst |err| / bound <= 1; printed per case with -s);
  (b) every seeded mutation (adafactor_reference.MUTATIONS) exceeds TWICE the bound (the GPU test's `FACTOR`) on some output of
      some case; the kinds of output that catch it are printed, and whether a parameters-only comparison at the limits of
      tests/test_gpu_kernels.py (rtol 2e-6, atol 3e-7) would have passed on that case;
  (c) the blind spot on record: the column mean over `cols` instead of `rows` on the `growing` case (gradients growing 4 x per
      step, no clip) PASSES the parameters-only comparison on all three steps while the column state is far outside its bound;
  (d) the case table reaches every kernel form, every stats_rows instantiation and every edge the issue names.
Measured figures: the table in DESIGN.md ("Adafactor against fp64")."""
import math

import pytest
import torch

import adafactor_reference as A

FACTOR = 2.0                # of test_gpu_adafactor_fp64.py: a mutation counts as rejected only beyond it
_REF = {}
# what must catch each mutation (kinds of output); a subset of what does
EXPECT = {"col_mean_over_cols": "col", "eps_inside_c2": "row", "rfac_all_batches": "p", "rms_one_chunk": "p",
          "c_not_squared": "row", "decay_after_update": "p", "decay_on_no_decay": "p", "last_unit_dropped": "col",
          "vec_unclipped": "sq", "beta2t_previous": "row", "coef_no_min": "coef"}


def _reference(ci):
    """[(operands, exact, bound, emulation)] of the three steps of case ci, computed once"""
    if ci not in _REF:
        case = A.CASES[ci]
        params, state = A.initial(case)
        steps = []
        for k in range(1, A.STEPS + 1):
            o = A.operands(case, k, params, state)
            ref = A.exact(o)
            emu = A.emulate(o)
            steps.append((o, ref, A.bound(o, ref), emu))
            params, state = A.carry(case, emu)
        if case["big"]:
            return steps                                                # 5 M elements in float64: not cached
        _REF[ci] = steps
    return _REF[ci]


@pytest.mark.parametrize("ci", range(len(A.CASES)), ids=A.CASE_IDS)
def test_emulation_is_inside_the_bound(ci):
    case = A.CASES[ci]
    worst = {}
    for k, (o, ref, bnd, emu) in enumerate(_reference(ci), 1):
        for key in A.outputs(o):
            assert bool(torch.isfinite(ref[key]).all()) and bool(torch.isfinite(emu[key]).all()), (case["name"], k, key)
        kinds = A.by_kind(A.ratios(o, ref, emu, bnd))
        for kind, r in kinds.items():
            worst[kind] = max(worst.get(kind, 0.0), r)
        c = float(ref["coef"])
        if case["max_grad_norm"] > 0 and case["gnorm"] is not None:      # the regime the case names
            assert (c < 1.0) == (case["gnorm"][k - 1] > case["max_grad_norm"]), (case["name"], k, c)
        if case["max_grad_norm"] <= 0:
            assert c == 1.0
    print(f"\n{case['name']}: " + " ".join(f"{kind} {r:.3f}" for kind, r in worst.items()), end="")
    for kind, r in worst.items():
        assert r <= 1.0, (case["name"], kind, r)


def _outcome(mut):
    """[(case, step, kinds of output beyond FACTOR x bound, worst ratio, parameters-only comparison passes)]"""
    res = []
    for ci, case in enumerate(A.CASES):
        if case["big"]:
            continue
        for k, (o, ref, bnd, emu) in enumerate(_reference(ci), 1):
            out = A.emulate(o, mutation=mut)
            if all(torch.equal(out[key], emu[key]) for key in A.outputs(o)):
                continue
            kinds = A.by_kind(A.ratios(o, ref, out, bnd))
            res.append((case["name"], k, tuple(sorted(kd for kd, r in kinds.items() if r > FACTOR)), max(kinds.values()),
                        A.old_params_pass(o, ref, out)))
    return res


@pytest.mark.parametrize("mut", A.MUTATIONS)
def test_mutation_exceeds_the_bound(mut):
    res = _outcome(mut)
    assert res, f"{mut} changed no output of any case"
    hits = [r for r in res if r[2]]
    gaps = [r for r in hits if r[4]]
    caught = sorted({kd for r in hits for kd in r[2]})
    print(f"\n{mut}: changes {len(res)} (case, step) pairs, exceeds the bound at {len(hits)} on {','.join(caught)}; "
          f"{len(gaps)} of them pass the parameters-only comparison")
    for name, k, kinds, worst, old_ok in (gaps + hits)[:4]:
        print(f"    {name} step {k}: worst |err| / bound {worst:.3g} on {','.join(kinds)}; parameters only: {'PASSES' if old_ok else 'rejects too'}")
    assert hits, f"the per-element criterion does not reject {mut} at any case"
    assert EXPECT[mut] in caught, (mut, caught)


def test_column_mean_mutation_passes_a_parameters_only_comparison():
    """The blind spot: rms(u) >= 1 divides a constant factor on a tensor's second moments out of the update."""
    ci = A.CASE_IDS.index("growing")
    assert A.CASES[ci]["max_grad_norm"] == 0.0
    case = A.CASES[ci]
    params, state = A.initial(case)
    for k, (o, ref, bnd, emu) in enumerate(_reference(ci), 1):
        # the wrong kernel runs on from its OWN state and parameters (a constant factor on the column state, step after step),
        # and is compared with the conforming chain as the old test compared the kernel with the oracle
        out = A.emulate(A.operands(case, k, params, state), mutation="col_mean_over_cols")
        params, state = A.carry(case, out)
        rt = A.ratios(o, ref, out, bnd)
        col_err = float(((out[("col", 0)] - ref[("col", 0)]).abs() / ref[("col", 0)]).max())
        dp = max(float((out[("p", i)] - ref[("p", i)]).abs().max()) for i in range(len(o["shapes"])))
        print(f"\nstep {k}: column state off by {100 * col_err:.0f} % ({rt[('col', 0)]:.3g} bounds), max |dp| {dp:.2g}", end="")
        assert A.old_params_pass(o, ref, out), (k, dp)
        assert rt[("col", 0)] > FACTOR and col_err > 0.3


def test_case_table_reaches_every_form_and_edge():
    forms, stats_rows, seen = set(), set(), {}
    for case in A.CASES:
        pl = A.plan(case["shapes"], case["group_floats"] or A.GROUP_FLOATS)
        forms |= set(pl["forms"])
        stats_rows |= {ln.get("stats_rows") for ln in pl["lens"]} - {None}
        seen[case["name"]] = pl
        assert any(A.decay_of(case["shapes"])) and not all(A.decay_of(case["shapes"]))
    assert forms == set(A.FORMS) and stats_rows == {4, 2, 1}
    shapes = {s for c in A.CASES for s in c["shapes"]}
    assert {(1, 4), (3, 24), (64, 256), (65, 260), (130, 260), (4097, 4), (300, 8), (2, 3, 8, 24), (5, 1284), (3, 3072),
            (16, 4096), (70, 3076), (33, 7), (5, 3, 9), (2, 300, 5), (6600, 5), (300, 64, 5), (40, 1), (20, 30), (3, 70, 259),
            (200, 259), (70, 4095), (1,), (7,), (256,), (257,), (3072,), (4100, 1280)} <= shapes
    # the edges behind those shapes
    pl = A.plan([(4097, 4)])
    assert [c[3] for c in pl["chunks"]] == [16384, 4]
    assert A.plan([(64, 256)])["chunks"] == [[0, 0, 0, 16384]]
    pl = A.plan([(6600, 5)])
    assert [u[2:] for u in pl["units"]] == [[0, 6553], [6553, 47]]
    assert [u[3] for u in A.plan([(200, 259)])["units"]] == [126, 74]
    assert A.plan([(2, 300, 5)])["lens"][0]["rows_per_wave"] == 2           # the second trip of rr += 256
    assert A.plan([(300, 64, 5)])["lens"][0]["units"] == 300
    assert A.plan([(4100, 1280)])["lens"][0]["chunks"] == 321
    g = seen["groups"]
    assert g["n_groups"] == 3 and g["group_bounds"] == [0, 3, 6, 7]
    first = [g["chunks"][b][0] for b in g["group_bounds"][:-1]]                        # the tensor that opens each group
    assert math.prod(g["tensors"][first[1]][1:4]) > A.SMALL_GROUP_FLOATS and g["ragged_units"] and len(g["vecs"]) == 2
    assert A.plan(A.GROUP_SHAPES)["n_groups"] == 1
    assert seen["all-ragged"]["chunks"] == [] and seen["all-ragged"]["vecs"]
    assert seen["no-1d"]["vecs"] == []
    assert {c["max_grad_norm"] for c in A.CASES} == {0.0, 1.0} and {c["clip_threshold"] for c in A.CASES} == {1.0, 0.5}
    assert {c["eps1"] for c in A.CASES} == {1e-30, 1e-3} and {c["weight_decay"] for c in A.CASES} == {0.01, 0.1}
    assert {c["grad"] for c in A.CASES} == {"gauss", "scaled", "zeros", "allzero"}


def test_zero_gradients_are_defined():
    """zero rows, columns, tensors and a zero arena: every output finite, and the reference says what each is"""
    ci = A.CASE_IDS.index("all-zero")
    for o, ref, bnd, emu in _reference(ci):
        assert float(ref["grad_norm"]) == 0.0 and float(ref["coef"]) == 1.0 and float(bnd["coef"]) == 0.0
        assert float(emu["grad_norm"]) == 0.0 and float(emu["coef"]) == 1.0
        for i, s in enumerate(o["shapes"]):
            wd = A.f32(o["weight_decay"]) if o["decay"][i] else 0.0
            assert torch.allclose(ref[("p", i)], o["params"][i].double() * (1.0 - wd * A.f32(o["lr"])), rtol=1e-15, atol=0)
    ci = A.CASE_IDS.index("zeros")
    o, ref, bnd, emu = _reference(ci)[0]
    assert float(ref[("row", 0)].max()) == A.f32(1e-30) and float(ref[("sq", 5)].max()) == A.f32(1e-30)     # beta2t = 0: eps1 alone
    assert torch.equal(ref[("p", 0)], o["params"][0].double() * ref["aux"]["decay"][0])
    assert float(ref[("row", 1)][1, 0]) == A.f32(1e-30) and float(ref[("row", 1)][1, 1]) > 1e-6             # a zero row beside a live one
