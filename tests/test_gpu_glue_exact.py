"""GPU: the glue kernels of csrc/embed_ce.hip and csrc/norm_act.hip held to EXACT references at their loops, tails and branches:
embed_gather_k, gather_rows_k, scatter_rows_k, target_rows_k, mask_tokens_k, colsum_partial_k<8|4> + reduce_partials_k,
transpose_k / transpose_vec_k (bf16 and fp32 input), cast_f32_bf16_k, add_f32_k.

References, the case table (`CASES`) and the comparison rule (`mismatch`): tests/glue_reference.py.  The instrument is proved on the
CPU by tests/test_glue_exact_host.py over the table this file runs: every kernel-shaped emulation equals its reference, every
seeded mutation of an emulation is rejected by a case named there, and which of them today's shapes of test_gpu_ops.py let through.

Comparison rules (one per kind of result; every case prints a line with -s):
    copies (embed_gather, gather_rows, scatter_rows, transpose of bf16 input): torch.equal on int16 views, so quiet and
        signalling NaN payloads, -0.0 and denormals must arrive bit for bit
    fp32 -> bf16 (cast, transpose of fp32 input): equal bits to x.bfloat16() on the CPU; NaN positions are compared as "is NaN"
    add_f32: equal bits to the CPU fp32 add
    target_rows: count == [n, first position] ([0, S] without a target), idx[:n] and lab[:n + 2] equal to the reference,
        idx[n:] and lab[n + 2:] still the sentinel
    mask_tokens: masked positions == 0xff80, every other element of the [rows, ld] buffer bit-identical, columns [cols, ld) included
    colsum, integer data in [-8, 8]: out == the int64 column sum exactly, with and without accumulate (rows * 8 + 64 < 2^24, so
        every partial sum of any order is exact in fp32): a dropped or doubled row, partial or column cannot hide
    colsum, random normal data: per column |out - fp64| <= gamma_L sum_r |x[r, c]| (+ half an fp32 ulp of |out| for the
        accumulate add), gamma_L = L 2^-24 / (1 - L 2^-24), L = ceil(rows / nr) + ceil(nr / 64) + 8 (glue_reference.colsum_chain
        says why).  A worst-case bound: the limit is 1 x the bound, `max |err| / bound` is printed, two launches agree bit for bit.
Every buffer a kernel writes starts as the sentinel (or as what the operation updates in place) and is followed by 64 guard
elements that must survive; the transpose also has two whole rows behind row `cols`; rows the scatter does not own and the
tails of idx / lab keep the sentinel: `mismatch` compares the WHOLE buffer.  Inputs are compared with a clone after the call.
Scalar against vector: every vector-eligible transpose case runs again through the scalar kernel (an output view that starts 4
elements into its buffer) and every V = 8 colsum case on integer data again through V = 4 (x 8-byte aligned only); the results
are torch.equal.  Rejected arguments raise RuntimeError and leave the sentinel-filled outputs untouched.

Measured on the MI355X: profiles/r30_glue_exact_tests.log and DESIGN.md ("Glue kernels against exact references")."""
import pytest
import torch

import glue_reference as R

pytestmark = pytest.mark.gpu

WORST = {}                       # colsum case id -> |err| / bound


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _ids(op):
    return [R.case_id(c) for c in R.CASES[op]]


def _dev(o):
    return {k: v.cuda() for k, v in o.items() if torch.is_tensor(v)}


def _unchanged(d, o):
    return all(torch.equal(d[k].cpu().view(torch.int8), o[k].contiguous().view(torch.int8)) for k in d)


def launch(hip, op, o, d, bufs):
    """one call of the kernel of `op`: operands `d` (device), the guarded device buffers `bufs` of glue_reference.fresh()"""
    if op == "embed_gather":
        hip.embed_gather(d["table"], d.get("audio"), d["src"], o["rows"], o["hidden"], bufs["out"])
    elif op == "gather_rows":
        hip.gather_rows(d["x"], d["src"], o["rows"], o["hidden"], bufs["out"])
    elif op == "scatter_rows":
        hip.scatter_rows(d["x"], d["src"], o["rows"], o["hidden"], bufs["out"])
    elif op == "target_rows":
        hip.target_rows(d["lab_in"], o["B"], o["S"], bufs["idx"], bufs["lab"], bufs["count"], s_major=bool(o["s_major"]))
    elif op == "mask_tokens":
        hip.mask_tokens_bf16(bufs["x"], o["ld"], o["rows"], o["cols"], d["ids"])
    elif op == "colsum":
        hip.colsum(d["xbuf"][o["off"]:], o["rows"], o["cols"], o["ld"], bufs["out"], accumulate=bool(o["accumulate"]))
    elif op == "transpose":
        hip.transpose_to_bf16(d["x"], o["rows"], o["cols"], bufs["out"][o["off"]:], o["ld_out"], ld_in=o["ld_in"])
    elif op == "cast":
        hip.cast_bf16(d["x"], bufs["y"], o["n"])
    elif op == "add":
        hip.add_f32(bufs["y"], d["b"], o["n"])
    else:
        raise KeyError(op)


def run(hip, op, o, d=None):
    """fresh buffers -> the kernel -> the buffers on the CPU; the operands must come out as they went in"""
    d = _dev(o) if d is None else d
    bufs = {k: v.cuda() for k, v in R.fresh(op, o).items()}
    launch(hip, op, o, d, bufs)
    torch.cuda.synchronize()
    assert _unchanged(d, o), (op, "an operand was written")
    return {k: v.cpu() for k, v in bufs.items()}


def held(hip, op, case, o=None, note=""):
    """one case against its reference under the rule -> (operands, reference, result)"""
    o = R.operands(op, case) if o is None else o
    ref, got = R.reference(op, o), run(hip, op, o)
    bad = R.mismatch(op, o, ref, got)
    print(f"\n{op} {R.case_id(case)}{note}: {'ok' if bad is None else bad}", end="")
    assert bad is None, (op, R.case_id(case), note, bad)
    return o, ref, got


def _table(ops):
    return dict(argnames="op,case", argvalues=[(op, c) for op in ops for c in R.CASES[op]],
                ids=[f"{op}-{R.case_id(c)}" for op in ops for c in R.CASES[op]])


@pytest.mark.parametrize(**_table(R.MOVERS))
def test_row_movers(hip, op, case):
    held(hip, op, case)


@pytest.mark.parametrize("case", R.CASES["target_rows"], ids=_ids("target_rows"))
def test_target_rows(hip, case):
    o, ref, got = held(hip, "target_rows", case)
    n = int(ref["count"][0])
    assert got["count"][:2].tolist() == [n, int(ref["count"][1])] and (n > 0 or int(got["count"][1]) == case["S"])
    assert bool((got["idx"][n:] == 7).all()) and bool((got["lab"][n + 2:] == 7).all())
    if case["labels"] in ("none", "first") or case["S"] == 1:
        assert n == 0


@pytest.mark.parametrize("case", R.CASES["mask_tokens"], ids=_ids("mask_tokens"))
def test_mask_tokens(hip, case):
    o, ref, got = held(hip, "mask_tokens", case)
    view = got["x"][:case["rows"] * case["ld"]].view(case["rows"], case["ld"])
    assert bool((view[:, case["cols"] - 1] == R._i16([0xFF80])[0]).all())                     # over the NaN that stood in row 0
    assert torch.equal(view[:, case["cols"]:], o["x"].view(case["rows"], case["ld"])[:, case["cols"]:])


@pytest.mark.parametrize("case", R.CASES["colsum"], ids=_ids("colsum"))
def test_colsum(hip, case):
    o, ref, got = held(hip, "colsum", case)
    again = run(hip, "colsum", o)
    assert torch.equal(again["out"].view(torch.int32), got["out"].view(torch.int32)), "two launches differ"
    if case["data"] == "randn":
        WORST[R.case_id(case)] = r = R.colsum_ratio(o, ref, got)
        print(f" |err| / bound {r:.4f} (L = {R.colsum_chain(case['rows'], case['cols'])}, V = {R.colsum_vector_width(o)})", end="")
        assert r <= 1.0
    elif R.colsum_vector_width(o) == 8:                                 # the same matrix 8-byte aligned only: the V = 4 kernel
        o4 = dict(o, off=4, xbuf=torch.cat([o["xbuf"][:4], o["xbuf"][o["off"]:]]))
        assert R.colsum_vector_width(o4) == 4
        _, _, got4 = held(hip, "colsum", dict(case, off=4), o=o4, note=" [V = 4 twin]")
        assert torch.equal(got4["out"], got["out"])


def test_colsum_worst_ratio():
    """the worst random-data ratio of this run, for DESIGN.md (the cases above assert each one <= 1)"""
    if WORST:
        worst = max(WORST, key=WORST.get)
        print(f"\ncolsum, random normal data: worst |err| / bound {WORST[worst]:.4f} at {worst} over {len(WORST)} cases", end="")
        assert WORST[worst] <= 1.0


@pytest.mark.parametrize("case", R.CASES["transpose"], ids=_ids("transpose"))
def test_transpose(hip, case):
    o, ref, got = held(hip, "transpose", case)
    if R.transpose_is_vector(o):                                        # the same case through transpose_k
        o4 = dict(o, off=4)
        assert not R.transpose_is_vector(o4)
        _, _, got4 = held(hip, "transpose", dict(case, off=4), o=o4, note=" [scalar twin]")
        n = (case["cols"] + 2) * case["ld_out"]
        assert torch.equal(got4["out"][4:4 + n], got["out"][:n])


@pytest.mark.parametrize(**_table(("cast", "add")))
def test_cast_add(hip, op, case):
    held(hip, op, case)


REJECTED = [
    ("embed_gather", dict(rows=5, hidden=520, idx="mixed"), dict(hidden=516)),
    ("gather_rows", dict(rows=5, hidden=520, idx="mixed"), dict(hidden=516)),
    ("scatter_rows", dict(rows=5, hidden=520, idx="mixed"), dict(hidden=516)),
    ("embed_gather", dict(rows=5, hidden=520, idx="mixed"), dict(rows=0)),
    ("gather_rows", dict(rows=5, hidden=520, idx="mixed"), dict(rows=0)),
    ("scatter_rows", dict(rows=5, hidden=520, idx="mixed"), dict(rows=0)),
    ("colsum", dict(rows=19, cols=72, ld=72, off=0, accumulate=0, data="int"), dict(rows=0)),
    ("colsum", dict(rows=19, cols=72, ld=72, off=0, accumulate=0, data="int"), dict(cols=70)),
    ("colsum", dict(rows=19, cols=72, ld=80, off=0, accumulate=0, data="int"), dict(ld=78)),
    ("transpose", dict(rows=65, cols=8, ld_out=72, ld_in=8, f32=0), dict(ld_out=64)),
    ("transpose", dict(rows=65, cols=8, ld_out=72, ld_in=8, f32=0), dict(rows=0)),
    ("mask_tokens", dict(rows=3, n=88, cols=504, ld=512), dict(ld=496)),
    ("mask_tokens", dict(rows=3, n=88, cols=504, ld=512), dict(n=0)),
    ("mask_tokens", dict(rows=3, n=88, cols=504, ld=512), dict(rows=0)),
    ("cast", dict(n=2056), dict(n=2052)),
    ("add", dict(n=1028), dict(n=1026)),
]


@pytest.mark.parametrize("op,case,bad", REJECTED, ids=[f"{op}-{R.case_id(bad)}" for op, _, bad in REJECTED])
def test_rejected_arguments_leave_the_outputs_alone(hip, op, case, bad):
    """the buffers are sized for the valid case; the call gets one argument the entry point must refuse"""
    o = R.operands(op, case)
    d = _dev(o)
    before = R.fresh(op, o)
    bufs = {k: v.cuda() for k, v in before.items()}
    with pytest.raises(RuntimeError):
        launch(hip, op, dict(o, **bad), dict(d, ids=d["ids"][:0]) if bad.get("n") == 0 else d, bufs)
    torch.cuda.synchronize()
    assert all(torch.equal(bufs[k].cpu().view(torch.int8), before[k].view(torch.int8)) for k in before)
    assert _unchanged(d, o)
