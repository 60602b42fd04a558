"""GPU: every GEMM path and epilogue of csrc/gemm_bf16.hip held PER ELEMENT to a float64 reference of the operation.

Reference, bounds with their derivation, the emulation, the case table (path x epilogue x shape), the restated dispatch `plan()`
and the path selection `select()`: tests/gemm_reference.py.  The instrument is proved on the CPU by tests/test_gemm_bound_host.py
over the case table this file runs.  The bit-identity tests between paths stay where they are (tests/test_gpu_kernels.py,
tests/test_gpu_gemm_persistent.py): they cannot see an error two paths share, this file can.

Per case: every output (C, the pre-activation copy, the SwiGLU side output) is a sentinel-filled buffer with GUARD_ROWS rows
below row M and ldc - N columns right of column N; the path is selected with desta_gemm_force_variant / desta_gemm_set_option
(restored in `finally`), the call runs twice, and
    desta_gemm_last_kernel() is the family plan() names;
    the two runs are bit-identical;
    max |out - fp64| / bound <= 2 (`FACTOR`) over ALL elements of every output, guards included (their bound is 0: they must
        still hold the sentinel bit for bit; asserted on its own as well) - no element is masked out;
    dyadic cases: an fp32 output EQUALS float64, a bf16 output RNE(float64), bit for bit;
    the head of the stream's workspace, zeroed before the call, is non-zero afterwards exactly when plan() says the case goes
        through K-slice slabs, and its last 4 KiB (arrival tickets, queue counters) are all zero after every call.
desta_gemm_last_kernel() reports the FAMILY only (1 = 128x128, 2 = 256x256, 3 = skinny / wide): that a case ran the ring and not the
double-buffered kernel, the persistent and not the one-tile-per-block kernel, the in-kernel reduce and not the fix-up launch, is
taken from the dispatch code as `plan()` restates it (gemm_bf16.hip:1812-1935), not observed; the workspace check confirms the
split, and the kernel names and split counts in the printed lines are plan()'s.
Every split case under option 5 = 1 shares its operands with its option 5 = 0 twin, and `test_inkernel_reduce_equals_the_fixup_launch`
asserts that the two give the same bits for real and dyadic operands alike.
The dropout mask of the reference is desta_dropout_mask's at index (z M + m) N + n.  The float64 reference of the two large
shapes is computed on the device.  Ratios are printed per case (run with -s).

A kernel edit this file catches while tests/test_gpu_kernels.py stays green (host evidence: the mutations of
test_gemm_bound_host.py): `f2bf` in front of the residual add of epilogue4 / epilogue_pair_bf16, rounding in front of rope4,
act 2 formed from the unrounded accumulator.

Measured on the MI355X: profiles/r15_gemm_fp64_tests.log and the table in DESIGN.md ("GEMM paths against fp64")."""
import pytest
import torch

import gemm_reference as G

pytestmark = pytest.mark.gpu

FACTOR = 2.0
ON_DEVICE = 1 << 20                     # outputs: above this the float64 reference is computed on the device
IDS = [G.case_id(c) for c in G.CASES]


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from desta import _hip
    return _hip


def _buffers(o):
    """sentinel-filled outputs -> {name: [batch, M + GUARD_ROWS, ld]}"""
    rows = o["M"] + G.GUARD_ROWS
    out = {"C": torch.full((o["batch"], rows, o["ldc"]), G.SENTINEL, dtype=torch.float32 if o["out_f32"] else torch.bfloat16, device="cuda")}
    if o["ldp_on"]:
        out["preact"] = torch.full((o["batch"], rows, o["ldp"]), G.SENTINEL, dtype=torch.bfloat16, device="cuda")
    if o["act"] == 2:
        out["aux"] = torch.full((1, rows, o["ld_aux"]), G.SENTINEL, dtype=torch.bfloat16, device="cuda")
    return out


def _call(hip, case, o, d, out):
    M, N, K = o["M"], o["N"], o["K"]
    A, B = G.kernel_arg(d, "A"), G.kernel_arg(d, "B")
    rows = M + G.GUARD_ROWS
    if case["entry"] == "w8":
        return hip.gemm_w8(A, B, d["scale"], out["C"], M, N, K, lda=o["lda"], ldc=o["ldc"], residual=d["res"], ldr=o["ldr"],
                           act=o["act"], alpha=o["alpha"])
    if case["entry"] in ("wide", "wide8"):
        return hip.gemm_wide(A, B, out["C"], M, N, K, scale=d["scale"], lda=o["lda"], ldc=o["ldc"], residual=d["res"], ldr=o["ldr"],
                             act=o["act"], alpha=o["alpha"])
    aux, ld_aux = (out["aux"], o["ld_aux"]) if o["act"] == 2 else (d["gu_store"], o["ld_aux"]) if o["act"] == 3 else (None, 0)
    return hip.gemm(A, B, out["C"], M, N, K, lda=o["lda"], ldb=o["ldb"], ldc=o["ldc"], bias=d["bias"], residual=d["res"], ldr=o["ldr"],
                    act=o["act"], preact=out.get("preact"), ldp=o["ldp"], alpha=o["alpha"], batch=o["batch"], stride_a=o["sA"],
                    stride_b=o["sB"], stride_c=rows * o["ldc"], stride_r=o.get("sR", 0), stride_p=rows * o["ldp"], aux=aux, ld_aux=ld_aux,
                    dropout_p=o["drop"], dropout_seed=o.get("seed", 0), a_rms_weight=d["rms_w"], a_rms_eps=o.get("rms_eps", 0.0),
                    trans_a=o["trans_a"], trans_b=o["trans_b"],
                    rope=(d["cs"], d["pos"], o["rope_cols"], o["rope"]) if o["rope"] else None)


def _slab_floats(case, o, p):
    """floats at the head of the workspace that the case's K-slice slabs cover (one slab's worth where it has none)"""
    if p["kernel"] == "wide":
        return p["ks"] * o["M"] * (2 * o["N"] if o["act"] == 4 else o["N"]) if p["ks"] > 1 else 65536
    return (p["tilesM"] * p["tilesN"] - p["full"]) * p["split"] * 65536 if p["split"] > 1 else 65536


def _run_twice(hip, case):
    """the case's call, twice, on its selected path -> (plan, host operands, device operands, the first run's outputs)"""
    p, e = G.plan(case), G.epi(case)
    mask = None
    if e["drop"]:
        mask = hip.dropout_mask(G.dropout_seed(case), e["batch"] * case["M"] * case["N"], e["drop"]).cpu()
    o = G.operands(case, mask=mask)
    d = G.to_device(o, "cuda")
    ws = hip._workspace(torch.device("cuda", torch.cuda.current_device()), hip.stream())
    head, tail = ws[:_slab_floats(case, o, p)], ws[-1024:].view(torch.int32)
    variant, opts = G.select(case)
    runs = []
    try:
        hip.gemm_force_variant(variant)
        for k, v in opts.items():
            hip.gemm_set_option(k, v)
        for _ in range(2):
            out = _buffers(o)
            head.zero_()
            _call(hip, case, o, d, out)
            torch.cuda.synchronize()
            assert hip.lib.desta_gemm_last_kernel() == p["family"], (hip.lib.desta_gemm_last_kernel(), p)
            assert bool(head.any()) == p["uses_ws"], "K-slice slabs " + ("missing" if p["uses_ws"] else "written by a case that does not split")
            assert not bool(tail.any()), "tickets / queue counters not reset"
            runs.append(out)
    finally:
        hip.gemm_force_variant(0)
        for k, v in G.DEFAULT_OPTIONS.items():
            hip.gemm_set_option(k, v)
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), f"two runs differ in {name}"
    return p, o, d, runs[0]


@pytest.mark.parametrize("case", G.CASES, ids=IDS)
def test_gemm_against_fp64(hip, case):
    p, o, d, out = _run_twice(hip, case)
    dev = "cuda" if case["M"] * case["N"] > ON_DEVICE else "cpu"
    oo = d if dev == "cuda" else o
    got = {n: x.to(dev) for n, x in out.items()}
    ref = G.exact(oo, stored=got["C"] if o["act"] == 2 else None)
    assert set(got) == set(G.outputs(o))
    ratios = {}
    for name, x in got.items():
        valid = ref["_"][name + "_valid"]
        assert bool((x.double()[~valid] == G.SENTINEL).all()), f"{name}: a guard row or column was written"
        ratios[name] = G.ratio(oo, ref, name, x)
    print(f"\n{G.case_id(case)} [{p['kernel']} split {p['split']} ks {p['ks']} c {p['c']}]: " + " ".join(f"{n} {r:.3f}" for n, r in ratios.items()), end="")
    for name, r in ratios.items():
        assert r <= FACTOR, (G.case_id(case), name, r)
    if case["kind"] == "dyadic":
        for name, x in got.items():
            want = ref[name] if G.is_f32(o, name) else G.rbf(ref[name])
            assert torch.equal(x.double(), want), f"{name}: a dyadic case must be exact"


TWINS = [c for c in G.CASES if c["opts"].get(5) == 1]


@pytest.mark.parametrize("case", TWINS, ids=[G.case_id(c) for c in TWINS])
def test_inkernel_reduce_equals_the_fixup_launch(hip, case):
    """option 5 = 1 (K-slices summed inside the GEMM launch, rows 256 s / split .. of slice s) against option 5 = 0 (the fix-up
    launch) on the SAME operands: both add the slabs in slice order and run epilogue4<true>, so every output has the same bits."""
    twin = {**case, "opts": {**case["opts"], 5: 0}}
    assert G.case_id(twin) in IDS and G.plan(case)["inkernel"] and not G.plan(twin)["inkernel"]
    _, o1, _, out1 = _run_twice(hip, case)
    _, o0, _, out0 = _run_twice(hip, twin)
    assert torch.equal(o1["A_store"], o0["A_store"]) and torch.equal(o1["B_store"], o0["B_store"])
    for name in out1:
        assert torch.equal(out1[name], out0[name]), name
