"""Host (no GPU): the per-element fp64 criterion of tests/rowwise_reference.py is proved before it is pointed at a kernel.

Over the SAME case table the GPU test runs (rowwise_reference.CASES, every case, every element):
  (a) the conforming emulation stays inside the bound on every output of every operation (worst |err| / bound <= 1; printed per
      operation and output with -s);
  (b) every seeded mutation (rowwise_reference.MUTATIONS) exceeds TWICE the bound (the GPU test's criterion, `FACTOR`) at some
      element of some case; the cases that catch it
      are printed, and with them whether the mutated result passes the whole-tensor criterion of tests/test_gpu_ops.py
      (rowwise_reference.OLD_LIMIT) on the same case.  The mutations named in `GAP` must be caught per element at a case where
      they pass the old criterion: that is the gap this suite closes;
  (c) the exact-zero regions hold: ignored rows of dlogits, the columns [V, ld), write_grad = 0, the all-ignored loss, the V and
      padding columns of RoPE, the prompt copies; and "exactly" means exactly (one element off by 2^-100 is an infinite ratio).
Measured (seed 0), worst ratio of the emulation per operation: see the table in DESIGN.md ("Row-wise kernels against fp64")."""
import pytest
import torch

import rowwise_reference as R

# mutations that today's whole-tensor criteria let through (the others are caught by both, or only have a per-element meaning)
GAP = ("rstd_scaled", "eps_1e-2", "ce_offtarget_2pct", "silu_unrounded")
FACTOR = 2.0                # of test_gpu_rowwise_fp64.py: a mutation counts as rejected only beyond it
_REF = {}


def _reference(op, i):
    """(operands, [(row slice, operands of the slice, exact, emulation)]) of case i of op, computed once"""
    if (op, i) not in _REF:
        o = R.operands(op, R.CASES[op][i])
        keep = op not in R.ELEMENTWISE or o[next(k for k in R._ROW_KEYS if k in o)].shape[0] <= 128
        parts = []
        for sl, oc in R.row_chunks(op, o):
            ref, emu = R.OPS[op].exact(oc), R.OPS[op].emulate(oc)
            parts.append((sl, oc, ref, emu))
        if not keep:
            return o, parts                                             # the large element-wise case: not cached (float64 of 17 M elements)
        _REF[(op, i)] = (o, parts)
    return _REF[(op, i)]


@pytest.mark.parametrize("op", list(R.OPS))
def test_emulation_is_inside_the_bound(op):
    worst = {n: (0.0, None) for n in R.OPS[op].outputs}
    for i, case in enumerate(R.CASES[op]):
        o, parts = _reference(op, i)
        for sl, oc, ref, emu in parts:
            for n in R.OPS[op].outputs:
                r = R.ratio(op, oc, ref, n, emu[n])
                if r > worst[n][0]:
                    worst[n] = (r, R.case_id(case))
    print(f"\n{op} ({len(R.CASES[op])} cases): " + "; ".join(f"{n} {r:.3f} at {c}" for n, (r, c) in worst.items()))
    for n, (r, c) in worst.items():
        assert r <= 1.0, (op, n, r, c)


def _outcome(mut):
    """[(op, case id, outputs caught per element, mutated result passes the old whole-tensor criterion on every output, worst ratio)]"""
    res = []
    for op in R.MUTATIONS[mut]:
        for i, case in enumerate(R.CASES[op]):
            o, parts = _reference(op, i)
            caught, changed, old_ok, worst = set(), False, True, 0.0
            for sl, oc, ref, emu in parts:
                out = R.OPS[op].emulate(oc, mutation=mut)
                for n in R.OPS[op].outputs:
                    if torch.equal(out[n], emu[n]):
                        continue
                    changed = True
                    r = R.ratio(op, oc, ref, n, out[n])
                    worst = max(worst, r)
                    if r > FACTOR:
                        caught.add(n)
                    lim = R.OLD_LIMIT.get(op, {}).get(n)
                    if lim is not None:
                        a, b = out[n], ref[n]
                        if op == "causal_lm_loss" and n == "dlogits":
                            a, b = a[:, :oc["V"]], b[:, :oc["V"]]      # the old test compares the first V columns
                        old_ok = old_ok and R.old_passes(lim, a, b)
            if changed:
                res.append((op, R.case_id(case), tuple(sorted(caught)), old_ok, worst))
    return res


@pytest.mark.parametrize("mut", list(R.MUTATIONS))
def test_mutation_exceeds_the_bound(mut):
    res = _outcome(mut)
    assert res, f"{mut} changed no output of any case"
    hits = [r for r in res if r[2]]
    gaps = [r for r in hits if r[3]]
    print(f"\n{mut}: changes {len(res)} cases, exceeds the bound at {len(hits)}, of which {len(gaps)} pass the whole-tensor criterion")
    for op, cid, caught, old_ok, worst in list(dict.fromkeys(gaps + hits))[:6]:
        print(f"    {op} {cid}: worst |err| / bound {worst:.1f}, REJECTED on {','.join(caught)}; old criterion {'PASSES' if old_ok else 'rejects too'}")
    print(f"    smallest worst ratio among the rejecting cases: {min(r[4] for r in hits):.2f}" if hits else "")
    assert hits, f"the per-element criterion does not reject {mut} at any case"
    if mut in GAP:
        assert gaps, f"{mut} was expected to pass the whole-tensor criterion where the bound rejects it"


def test_exact_zero_regions():
    op = "causal_lm_loss"
    for i, case in enumerate(R.CASES[op]):
        o, parts = _reference(op, i)
        _, _, ref, emu = parts[0]
        V, ld, logits = o["V"], o["ld"], o["logits"].double()
        bnd = R.OPS[op].bound(o, ref, "dlogits", emu["dlogits"])
        valid = ref["aux"]["valid"]
        assert torch.equal(ref["dlogits"][:, V:], logits[:, V:]) and float(bnd[:, V:].abs().max() if ld > V else 0.0) == 0.0
        assert torch.equal(emu["dlogits"][:, V:], logits[:, V:])
        assert not bool(valid.view(R.CE_B, R.CE_S)[:, -1].any())                          # the shift by one
        if case["write_grad"]:
            assert float(ref["dlogits"][~valid][:, :V].abs().max()) == 0.0 and float(bnd[~valid].abs().max()) == 0.0
            assert bool((bnd[valid][:, :V] > 0).all())
            bad = emu["dlogits"].clone()
            bad[int(torch.nonzero(~valid)[0]), 0] = 2.0 ** -100
            assert R.ratio(op, o, ref, "dlogits", bad) == float("inf")
        else:
            assert torch.equal(ref["dlogits"], logits) and float(bnd.abs().max()) == 0.0
        if case["labels"] == "ignored":
            assert float(ref["loss"]) == 0.0 and float(emu["loss"]) == 0.0 and float(ref["dlogits"][:, :V].abs().max()) == 0.0
        else:
            assert int(valid.sum()) == 6 and float(ref["loss"]) > 0.0
    op = "rope"
    for i, case in enumerate(R.CASES[op]):
        o, parts = _reference(op, i)
        _, _, ref, emu = parts[0]
        nhd = (o["n_q"] + o["n_kv"]) * o["hd"]
        bnd = R.OPS[op].bound(o, ref, "out", emu["out"])
        assert o["ld"] > nhd and float(bnd[:, nhd:].abs().max()) == 0.0 and bool((bnd[:, :nhd] > 0).all())
        assert torch.equal(ref["out"][:, nhd:], o["buf"].double()[:, nhd:]) and torch.equal(emu["out"][:, nhd:], o["buf"].double()[:, nhd:])
        bad = emu["out"].clone()
        bad[0, nhd] = torch.nextafter(bad[0, nhd], torch.tensor(float("inf"), dtype=torch.float64))
        assert R.ratio(op, o, ref, "out", bad) == float("inf")
    for i, case in enumerate(R.CASES["prompt_expand"]):
        o, parts = _reference("prompt_expand", i)
        _, _, ref, emu = parts[0]
        assert torch.equal(ref["x16"], o["prompts"].bfloat16().double().repeat_interleave(o["batch"], 0))
        assert R.ratio("prompt_expand", o, ref, "x32", emu["x32"]) == 0.0
    # LayerNorm's constant row: y = beta exactly, rstd = eps^-1/2
    for i, case in enumerate(R.CASES["layernorm_fwd"]):
        if case["data"] != "edges":
            continue
        o, parts = _reference("layernorm_fwd", i)
        _, _, ref, emu = parts[0]
        assert torch.equal(ref["y32"][2], o["beta"].double()) and torch.equal(emu["y32"][2], o["beta"].double())
        assert float(ref["mean"][2]) == R.EDGE_CONST and abs(float(ref["rstd"][2]) * R.f32(case["eps"]) ** 0.5 - 1) < 1e-12


def test_case_table_reaches_every_path():
    """the shapes the dispatchers switch on (norm_act.hip LN_DISPATCH, nblocks' cap, layernorm_bwd's 512 blocks; embed_ce.hip:467-473)"""
    cols = {c["cols"] for c in R.CASES["rmsnorm_fwd"]}
    assert {8, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104, 8192} <= cols
    assert any(c["rows"] > 512 * 4 and c["rows"] % 4 for c in R.CASES["layernorm_bwd"])
    assert any(R.ln_bwd_blocks(c["rows"]) >= 65 and R.ln_bwd_blocks(c["rows"]) % 16 for c in R.CASES["layernorm_bwd"])
    for op in R.ELEMENTWISE:
        assert any(c["rows"] * (c["I"] // 8) > 8192 * 256 for c in R.CASES[op])

    def kernel(V):
        nv8 = V // 8
        return "reg16" if V % 8 == 0 and 2048 < nv8 <= 16384 else "reg20" if V % 8 == 0 and 2048 < nv8 <= 20480 else "row"
    by = {}
    for c in R.CASES["causal_lm_loss"]:
        by.setdefault(kernel(c["V"]), set()).add(c["V"])
    assert by["row"] >= {7, 1003, 16384, 50257, 163848} and by["reg16"] >= {16392, 131072} and by["reg20"] >= {131080, 163840}
