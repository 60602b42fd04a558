"""Host (no GPU): the per-element fp64 criterion of tests/gemm_reference.py is proved before it is pointed at a kernel.

Over the SAME case table the GPU test runs (gemm_reference.CASES):
  (a) the conforming emulation stays inside 1 x bound at every element of every output (guard rows and columns included) of
      every case; the worst ratio per path is printed with -s;
  (b) every seeded mutation (gemm_reference.MUTATIONS) exceeds TWICE the bound (the GPU test's `FACTOR`) somewhere at EVERY case
      it applies to (`applies()`: double_rounding_residual and kslice_row_missing are seeded into real-operand cases); with it, whether the
      mutated result passes the whole-tensor limits of tests/test_gpu_kernels.py.  double_rounding_residual must pass the
      assert_close limits of test_gemm_plain and test_gemm_epilogues_and_batch, rope_double_rounding the rotary test's rel-L2 <
      6e-3, where the bound rejects them: that is the gap this suite closes.  The others are reported only;
  (c) every dyadic case satisfies its exactness precondition (K a b < 2^24, integer operands inside [-a, a] / [-b, b] 2^-s, an
      fp32 matmul in two K permutations equal to float64), its float64 result is an fp32 value, and the emulation equals it;
  (d) `plan()` reproduces the hand-computed split counts, tile maps and row partitions of the dispatch edges the table is built on.
Measured here (seed 0): see the table in DESIGN.md ("GEMM paths against fp64")."""
import pytest
import torch

import gemm_reference as G

FACTOR = 2.0                # of test_gpu_gemm_fp64.py: a mutation counts as rejected only beyond it
PATHS = sorted({c["path"] for c in G.CASES})
_REF = {}


def _reference(i):
    """(operands, exact, emulation) of case i, computed once (the two largest cases are not kept)"""
    if i in _REF:
        return _REF[i]
    o = G.operands(G.CASES[i])
    r = (o, G.exact(o), G.emulate(o))
    if G.CASES[i]["M"] * G.CASES[i]["N"] <= G.HOST_MAX_ELEMENTS:
        _REF[i] = r
    return r


@pytest.mark.parametrize("path", PATHS)
def test_emulation_is_inside_the_bound(path):
    worst = (0.0, None)
    n = 0
    for i, case in enumerate(G.CASES):
        if case["path"] != path:
            continue
        o, ref, emu = _reference(i)
        n += 1
        assert set(G.outputs(o)) == set(emu) == set(ref) - {"_"}
        for name in G.outputs(o):
            r = G.ratio(o, ref, name, emu[name])
            assert r <= 1.0, (G.case_id(case), name, r)
            if r > worst[0]:
                worst = (r, f"{G.case_id(case)}:{name}")
    print(f"\n{path} ({n} cases): worst emulation ratio {worst[0]:.3f} at {worst[1]}")


def _old_limits(case, o, ref, out):
    """does the mutated C pass the old whole-tensor limits on the region the old tests compare?  -> {limit: passed}"""
    M, N = o["M"], G.layout(case)["Nc"]
    a, b = out["C"][:, :M, :N], ref["C"][:, :M, :N]
    res = {"plain": G.old_plain_bf16(a, b, o["K"]), "epilogue": G.old_epilogue_bf16(a, b)}
    if o["rope"]:
        res["rope"] = G.old_rope(a, b)
    return res


@pytest.mark.parametrize("mut", G.MUTATIONS)
def test_mutation_exceeds_the_bound(mut):
    rows = []
    for i, case in enumerate(G.CASES):
        if not G.applies(mut, case):
            continue
        o, ref, emu = _reference(i)
        out = G.emulate(o, mutation=mut)
        if mut == "swiglu_unrounded_proj" and o["act"] == 2:
            assert torch.equal(out["C"], emu["C"])                       # the projection itself is unchanged: only aux is off
        r = max(G.ratio(o, ref, name, out[name]) for name in G.outputs(o))
        rows.append((G.case_id(case), r, _old_limits(case, o, ref, out)))
        assert r > FACTOR, f"{mut} stays within {FACTOR} x bound at {G.case_id(case)}: worst ratio {r:.3f}"
    assert rows, f"{mut} applies to no case"
    passed = {k: sum(1 for _, _, lim in rows if lim.get(k)) for k in ("plain", "epilogue", "rope")}
    print(f"\n{mut}: {len(rows)} cases, smallest worst ratio {min(r for _, r, _ in rows):.1f}; passes the old limits at "
          f"{passed['plain']} (test_gemm_plain) / {passed['epilogue']} (epilogues_and_batch) / {passed['rope']} (rotary rel-L2) of them")
    if mut == "double_rounding_residual":
        both = [cid for cid, _, lim in rows if lim["plain"] and lim["epilogue"]]
        assert any(c.startswith("db128-200x136x192-res8") for c in both) and any(c.startswith("k256-257x288x256-res8") for c in both), both
    if mut == "rope_double_rounding":
        assert all(lim["rope"] for _, _, lim in rows), [(c, lim) for c, _, lim in rows]


def test_mutations_cover_every_kind_of_case():
    for mut in G.MUTATIONS:
        assert any(G.applies(mut, c) for c in G.CASES), mut
    paths = {m: {c["path"] for c in G.CASES if G.applies(m, c)} for m in G.MUTATIONS}
    assert paths["double_rounding_residual"] >= {"db128", "ring128", "k256", "split", "persist", "skinny", "w8", "wide"}
    assert paths["rope_double_rounding"] >= {"db128", "ring128", "k256", "split", "persist"}      # generic, wide-store MODE 4, fix-up, reduce
    assert paths["swiglu_unrounded_proj"] >= {"db128", "ring128", "k256", "persist", "skinny", "w8", "wide"}
    assert {c["opts"].get(5, 0) for c in G.CASES if G.applies("kslice_row_missing", c)} == {0, 1}
    assert {c["opts"].get(5, 0) for c in G.CASES if G.applies("group_tail_tile_swapped", c)} == {0, 1}


def test_guard_region_is_exact():
    """a stray store that moves a guard element by one float64 step, past row M or past column N inside a row, is an infinite ratio"""
    i = next(k for k, c in enumerate(G.CASES) if G.case_id(c).startswith("k256-257x288x256-f32-real"))
    o, ref, emu = _reference(i)
    for m, n in ((o["M"], 0), (0, o["N"]), (o["M"] + G.GUARD_ROWS - 1, o["ldc"] - 1)):
        bad = emu["C"].clone()
        bad[0, m, n] *= 1 + 2.0 ** -52
        assert G.ratio(o, ref, "C", bad) == float("inf")
    assert G.ratio(o, ref, "C", emu["C"]) <= 1.0


def test_dyadic_cases_are_exact():
    n = 0
    for i, case in enumerate(G.CASES):
        if case["kind"] != "dyadic":
            continue
        assert G.epi(case)["exact"], G.case_id(case)
        o, ref, emu = _reference(i)
        a, b, s = o["dyadic"]
        K = o["K"]
        assert K * a * b < 2 ** 24, G.case_id(case)
        A, B = G.logical(o, "A"), G.logical(o, "B")
        Bi = B * 2.0 ** s
        assert torch.equal(A, A.round()) and torch.equal(Bi, Bi.round()) and float(A.abs().max()) <= a and float(Bi.abs().max()) <= b
        if K <= 256 and o["alpha"] == 1.0:
            assert (a, b, s) == (255, 255, 0) and float(A.abs().max()) > 127 and float(B.abs().max()) > 127   # full 8-bit significands
        # (bf16 storage holds exactly these integers: logical() reads the bf16 tensors)
        ref64 = A @ B.transpose(1, 2)
        perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
        for Ap, Bp in ((A, B), (A[:, :, perm], B[:, :, perm])):
            got = Ap.float() @ Bp.float().transpose(1, 2)
            assert torch.equal(got.double(), ref64), G.case_id(case)
        for name in G.outputs(o):
            want = ref[name] if G.is_f32(o, name) else G.rbf(ref[name])
            assert torch.equal(G.r32(ref[name]), ref[name]), (G.case_id(case), name)        # every intermediate sum fits fp32
            assert torch.equal(emu[name], want), (G.case_id(case), name)
        n += 1
    assert n >= 60
    print(f"\n{n} dyadic cases exact")


def _case(prefix):
    hits = [c for c in G.CASES if G.case_id(c).startswith(prefix)]
    assert hits, prefix
    return hits[0]


def test_plan_reproduces_the_dispatch_edges():
    # split counts of the (257, 288, K) tail: 4 tiles, min(256 / 4, 8, nk / 16)
    for o5 in (0, 1):
        for K, split in ((2048, 2), (3072, 3), (4096, 4), (5120, 5), (7168, 7), (8192, 8)):
            p = G.plan(_case(f"split-257x288x{K}-f32-dyadic-o5={o5}"))
            assert (p["family"], p["kernel"], p["split"], p["full"], p["tilesM"], p["tilesN"]) == (2, "256", split, 0, 2, 2)
            assert p["inkernel"] == bool(o5) and p["uses_ws"] and not p["persistent"]
            assert 4 * split <= 64                                       # every block co-resident: a timeout of the bounded spin shows as the sentinel
            assert p["c"] == 2 * -(-(K // 64) // split) + 32 + split - 1
        p = G.plan(_case(f"split-2305x520x2048-f32-dyadic-o5={o5}"))
        assert (p["split"], p["full"], p["tilesM"], p["tilesN"]) == (2, 0, 10, 3) and 30 * 2 <= 64
        # L -> tile: a whole group of 8 tile rows, then the short last group of 2 (gemm_bf16.hip:931-936)
        assert [G.tile_of(p, L) for L in (0, 1, 7, 8, 23)] == [(0, 0), (1, 0), (7, 0), (0, 1), (7, 2)]
        assert [G.tile_of(p, L) for L in range(24, 30)] == [(8, 0), (9, 0), (8, 1), (9, 1), (8, 2), (9, 2)]
        assert sorted(G.tile_of(p, L) for L in range(30)) == [(m, n) for m in range(10) for n in range(3)]
    # the in-kernel reduce's uneven row partitions
    assert G.reduce_rows(3) == [(0, 85), (85, 170), (170, 256)]
    assert [b - a for a, b in G.reduce_rows(7)] == [36, 37, 36, 37, 36, 37, 37]
    assert [b - a for a, b in G.reduce_rows(5)] == [51, 51, 51, 51, 52]
    # persistent kernel: 4 tiles, a split tail through the queues, 272 tiles
    p = G.plan(_case("persist-257x288x512-plain-real"))
    assert (p["kernel"], p["persistent"], p["split"], p["tilesM"] * p["tilesN"], p["wide_store"]) == ("256p", True, 1, 4, True)
    p = G.plan(_case("persist-257x288x4096-f32"))
    assert (p["kernel"], p["split"], p["inkernel"], p["uses_ws"]) == ("256p", 4, False, True)
    p = G.plan(_case("persist-4352x4096x64-plain"))
    assert (p["kernel"], p["split"], p["tilesM"] * p["tilesN"]) == ("256p", 1, 272)   # 34 tiles per queue for its 32 blocks
    assert not G.plan(G._c("persist", 257, 288, 512, "batch3", variant=8))["persistent"]   # batch > 1: the one-tile-per-block kernel
    # wide store: N % 32 == 0, ldc % 8 == 0, bf16, no dropout; the preact copy only alone
    assert not G.plan(_case("k256-257x260x256-plain-real"))["wide_store"]
    assert not G.plan(_case("k256-257x288x256-ldc12-real"))["wide_store"]
    assert G.plan(_case("k256-257x288x256-pre-real"))["wide_store"] and not G.plan(_case("k256-257x288x256-rich-real"))["wide_store"]
    assert not G.plan(_case("k256-257x288x256-drop-real"))["wide_store"] and G.plan(_case("k256-257x288x256-rope128"))["wide_store"]
    # 128x128: double-buffered below four K-tiles or with option 6 = 0, ring with option 6 = 2
    assert {G.plan(c)["kernel"] for c in G.CASES if c["path"] == "db128"} == {"db128"}
    assert {G.plan(c)["kernel"] for c in G.CASES if c["path"] == "ring128"} == {"ring128"}
    assert {c["K"] for c in G.CASES if c["path"] == "ring128"} >= {256, 320, 576}
    assert G.plan(G._c("db128", 200, 136, 192, "plain", variant=1, opts={6: 2}))["kernel"] == "db128"     # nk = 3 < 4
    assert G.plan(G._c("x", 200, 136, 256, "plain", variant=1))["kernel"] == "ring128"                    # default: <= 256 blocks
    assert G.plan(G._c("x", 4352, 4096, 256, "plain", variant=1))["kernel"] == "db128"                    # 1088 blocks
    # SwiGLU epilogues never fall to the skinny kernel, the decode paths are family 3
    assert G.plan(_case("db128-8x128x192-act2"))["family"] == 1 and G.plan(_case("k256-8x320x256-act3"))["family"] == 2
    for c in G.CASES:
        if c["path"] in ("skinny", "w8", "wide"):
            assert G.plan(c)["family"] == 3, G.case_id(c)
    assert G.plan(_case("wide-64x1028x2048-plain"))["ks"] == 2 and G.plan(_case("wide-40x512x2048-act4"))["ks"] == 2
    assert G.plan(_case("wide-33x100x192-res8"))["ks"] == 1 and G.plan(_case("wide-48x36x2368-res4"))["ks"] == 2
    # automatic choice (no forced variant): the flagship shapes still land where the comments of the dispatch say
    assert G.plan(G._c("x", 5120, 4096, 4096, "plain"))["split"] == 4 and G.plan(G._c("x", 5120, 4096, 4096, "plain"))["full"] == 256
    assert G.plan(G._c("x", 200, 136, 512, "plain"))["family"] == 1


def test_case_table_reaches_every_path():
    ids = [G.case_id(c) for c in G.CASES]
    assert len(set(ids)) == len(ids)
    assert {c["variant"] for c in G.CASES if c["path"] == "k256"} == {2, 3, 6, 7}
    assert {c["K"] for c in G.CASES if c["path"] == "k256"} >= {64, 128, 192, 256, 512}
    assert {c["opts"].get(2, 0) for c in G.CASES if c["path"] == "skinny"} == {0, 164, 322, 641}
    assert {c["M"] for c in G.CASES if c["path"] == "skinny"} >= {1, 3, 16}
    assert any(c["opts"].get(3) == 7 for c in G.CASES) and any(c["opts"].get(10) == 0 for c in G.CASES)
    assert {(c["ta"], c["tb"]) for c in G.CASES if c["ta"] or c["tb"]} == {(True, False), (False, True), (True, True)}
    # every epilogue instance on every path that admits it; what a path does not admit is listed with the check that refuses it
    for path, refused in G.INADMISSIBLE.items():
        have = {c["epi"] for c in G.CASES if c["path"] == path}
        assert have >= set(G.ALL_EPIS) - set(refused), (path, set(G.ALL_EPIS) - set(refused) - have)
        assert not have & set(refused), (path, have & set(refused))
        for e in ("act2", "act3"):
            if e not in refused:
                assert {c["M"] for c in G.CASES if c["epi"] == e and c["path"] == path} == {8, 200, 257}, (path, e)
        real = {c["epi"] for c in G.CASES if c["path"] == path and c["kind"] == "real"}
        assert real >= set(G.ALL_EPIS) - set(refused), (path, "real operands", set(G.ALL_EPIS) - set(refused) - real)
    # every shape of a path with `plain` (real operands) and the richest instance
    for path in ("db128", "ring128", "k256", "split", "persist", "skinny"):
        shapes = {(c["M"], c["N"], c["K"]) for c in G.CASES if c["path"] == path and not (c["ta"] or c["tb"] or c["im2col"])
                  and c["epi"] in G.TILE_EPIS and c["N"] >= 16}
        for sh in shapes:
            epis = {(c["epi"], c["kind"]) for c in G.CASES if c["path"] == path and (c["M"], c["N"], c["K"]) == sh}
            assert ("plain", "real") in epis and ("rich", "real") in epis, (path, sh)
    for v in (2, 3, 6, 7):
        assert {c["K"] for c in G.CASES if c["path"] == "k256" and c["variant"] == v} >= {64, 128, 192, 256, 512}
