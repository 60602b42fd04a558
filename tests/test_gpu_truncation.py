"""GPU: typical-p, epsilon and eta cut-offs of `desta_sample_truncated_rows_bf16` (sample_truncated_k) held to the float64
reference of tests/truncation_reference.py (`T`; proved on the CPU against HF's warper classes by test_truncation_host.py).

Table: (V, ld) of sampling_reference.VLD, its six row profiles, the eight settings of T.SETTINGS, 32 rows per launch, draws over
sampling_reference.SEEDS x STEPS.  Columns [V, ld) hold +60, above every logit.
  1. every case: keep_mask == T.kept_truncated exactly (the rows keep their margins from every cut-off), every pick lies in the
     kept set, and every draw has ratio = max(C_lo - u, u - C_hi, 0) / eps <= 1 under the chain's eps;
  2. with all three off the new entry point returns the picks and masks of desta_sample_rows_bf16, bit for bit;
  3. rows (b, j) of a width > 1 launch equal row b of one-row calls at step0 + j whose history carries the tail;
  4. rows without a finite score give token 0 and an empty mask; bad arguments are rejected.
The model-level checks (generate, draft-and-verify, guidance + constraints) are in test_gpu_truncation_generate.py."""
import numpy as np
import pytest
import torch

import sampling_reference as S
import truncation_reference as T

pytestmark = pytest.mark.gpu

PAD = 60.0
DRAWS = [(seed, step) for seed in S.SEEDS for step in S.STEPS]


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _buf(logits, ld):
    rows, V = logits.shape
    buf = torch.full((rows, ld), PAD, dtype=torch.bfloat16, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[:, :V] = logits.cuda()
    return buf


def _chain_args(case, hist):
    pen = case.get("penalty", 1.0)
    return dict(temperature=case["T"], top_k=case.get("top_k", 0), top_p=case.get("top_p", 1.0), min_p=case.get("min_p", 0.0),
                repetition_penalty=pen, hist=hist if pen != 1.0 else None, hist_len=hist.shape[1] if pen != 1.0 else 0)


def _launch(hip, case, buf, hist, seed, step):
    rows, V, ld = buf.shape[0], case["V"], buf.shape[1]
    out = torch.full((rows,), -7, dtype=torch.int64, device="cuda")
    m = torch.full((rows, V), 3, dtype=torch.uint8, device="cuda")
    hip.sample(buf, ld, rows, V, out, seed=seed, step=step, keep_mask=m, **_chain_args(case, hist), **T.truncation_args(case))
    return out.cpu().numpy(), m


_ORDERED = sorted(T.CASES, key=lambda c: (c["V"], c["profile"], c["setting"], c["ld"]))        # one reference per pair of ld variants


# ------------------------------------------------------------------------------------------------ 1. kept set and draw
@pytest.mark.parametrize("case", _ORDERED, ids=T.case_id)
def test_kept_set_is_exact_and_every_draw_inverts_the_fp64_cdf(hip, case):
    logits, hist = T.rows_for(case["V"], case["profile"])
    ref = T.reference(case)
    assert bool(T.margins_hold(ref.margins).all()) and bool(ref.finite_rows.all())
    buf = _buf(logits, case["ld"])
    hist_d = hist.cuda()
    want_mask = torch.from_numpy(ref.kept.astype(np.uint8)).cuda()
    rr = np.arange(T.ROWS)
    worst = 0.0
    calls = hip.SAMPLE_TRUNCATED_CALLS
    for seed, step in DRAWS:
        tok, mask = _launch(hip, case, buf, hist_d, seed, step)
        wrong = int((mask != want_mask).sum())
        assert wrong == 0, (T.case_id(case), seed, step, wrong, (mask != want_mask).any(1).nonzero().flatten().tolist())
        assert bool(((tok >= 0) & (tok < case["V"])).all())
        assert bool(ref.kept[rr, tok].all()), (T.case_id(case), seed, step)
        ratio = ref.ratio(tok, S.u24_rows(seed, step, T.ROWS))
        worst = max(worst, float(ratio.max()))
        assert float(ratio.max()) <= 1.0, (T.case_id(case), seed, step, int(ratio.argmax()), float(ratio.max()))
    assert hip.SAMPLE_TRUNCATED_CALLS == calls + len(DRAWS)
    print(f"\n{T.case_id(case)}: kept {int(ref.kept.sum(1).min())}..{int(ref.kept.sum(1).max())} of {int(ref.kept0.sum(1).min())}.."
          f"{int(ref.kept0.sum(1).max())}, largest ratio {worst:.3g} (eps {float(ref.eps.max()):.3g})", end="")


def test_step_7_can_remove_the_row_maximum_in_front_of_step_8(hip):
    """The table holds the case the survivors'-maximum rule exists for: under typical_lo_eps_hi step 7 removes the most probable
    token of most randn rows and step 8 (epsilon above every survivor's share) leaves exactly the ties with THEIR maximum."""
    V, ld = S.VLD[0]
    case = next(c for c in T.CASES if (c["V"], c["ld"], c["profile"], c["setting"]) == (V, ld, "randn", "typical_lo_eps_hi"))
    logits, hist = T.rows_for(V, "randn")
    ref = T.reference(case)
    t = S.case_scores(case, logits, hist)[0]
    top = t.argmax(1)
    gone = ~ref.kept[np.arange(T.ROWS), top]
    assert int(gone.sum()) >= T.ROWS // 2
    _, mask = _launch(hip, case, _buf(logits, ld), hist.cuda(), 99, 0)
    mask = mask.cpu().numpy().astype(bool)
    assert np.array_equal(mask, ref.kept)
    for r in np.flatnonzero(gone):
        assert len(set(t[r, mask[r]].tolist())) == 1 and float(t[r, mask[r]][0]) < float(t[r, top[r]])


# ------------------------------------------------------------------------------------------------ 2. all three off
@pytest.mark.parametrize("V,ld", [S.VLD[0], S.VLD[3]])
@pytest.mark.parametrize("setting", ["T", "full"])
def test_all_three_off_is_sample_rows_bit_for_bit(hip, V, ld, setting):
    case = S.CASE_BY_ID[f"chain-V{V}-ld{ld}-randn-{setting}"]
    logits, hist = T.rows_for(V, "randn")
    batch, width = 4, 3
    buf, hist_d = _buf(logits[:batch * width], ld), hist[:batch].cuda()
    tail = torch.randint(0, V, (batch, width), generator=torch.Generator().manual_seed(V), dtype=torch.int64).cuda()
    args = dict(_chain_args(case, hist_d), tail=tail, seed=S.SEEDS[1], step0=2 ** 32 - 2)
    got = []
    for which in ("rows", "truncated"):
        out = torch.full((batch * width,), -7, dtype=torch.int64, device="cuda")
        m = torch.full((batch * width, V), 3, dtype=torch.uint8, device="cuda")
        if which == "rows":
            hip.sample_rows(buf, ld, batch, width, V, out, keep_mask=m, **args)
        else:                                                              # the new symbol itself, with the off values
            hip.check(hip._sample_truncated_rows(hip.p(buf), ld, batch, width, V, hip.p(args["hist"]),
                                                 0 if args["hist"] is None else args["hist"].stride(0), args["hist_len"], hip.p(tail),
                                                 tail.stride(0), args["repetition_penalty"], 1, args["temperature"], args["top_k"],
                                                 args["top_p"], args["min_p"], 1.0, 0.0, 0.0, args["seed"], args["step0"] & 0xFFFFFFFF,
                                                 hip.p(out), hip.p(m), hip.stream()), "desta_sample_truncated_rows_bf16")
        got.append((out.cpu(), m.cpu()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert bool(((got[0][0] >= 0) & (got[0][0] < V)).all())


# ------------------------------------------------------------------------------------------------ 3. grouped rows
@pytest.mark.parametrize("V,ld", [S.VLD[1], S.VLD[2]])
def test_grouped_rows_equal_one_row_calls(hip, V, ld):
    """row (b, j) of a (batch, width) launch == row b of a batch-row call at step0 + j with the history hist[b] + tail[b, 1:1 + j]"""
    case = next(c for c in T.CASES if (c["V"], c["ld"], c["profile"], c["setting"]) == (V, ld, "randn", "all"))
    logits, hist = T.rows_for(V, "randn")
    batch, width = 5, 4
    buf = _buf(logits[:batch * width], ld)
    hist_d = hist[:batch].cuda()
    t = S.case_scores(dict(case, penalty=1.0), logits[:batch * width], None)[0]
    top2 = torch.from_numpy(np.argsort(-t, axis=1)[:, :2].copy())           # heavy tokens: a penalty on them moves the kept set
    tail = torch.empty(batch, width, dtype=torch.int64)
    for b in range(batch):
        tail[b, 0] = hist[b, -1]
        for j in range(1, width):
            tail[b, j] = top2[b * width + j, j % 2] if j < width - 1 else -1     # the next row's heavy token; a -1 draft is ignored
    tail = tail.cuda()
    step0 = 2 ** 32 - 2                                                     # step0 + j wraps
    out = torch.full((batch * width,), -7, dtype=torch.int64, device="cuda")
    m = torch.full((batch * width, V), 3, dtype=torch.uint8, device="cuda")
    hip.sample_rows(buf, ld, batch, width, V, out, keep_mask=m, tail=tail, seed=S.SEEDS[1], step0=step0, **_chain_args(case, hist_d),
                    **T.truncation_args(case))
    moved = 0
    for j in range(width):
        rows_j = buf.view(batch, width, ld)[:, j].contiguous()
        h = torch.cat([hist_d, tail[:, 1:1 + j]], dim=1).contiguous()
        o1 = torch.full((batch,), -7, dtype=torch.int64, device="cuda")
        m1 = torch.full((batch, V), 3, dtype=torch.uint8, device="cuda")
        hip.sample(rows_j, ld, batch, V, o1, keep_mask=m1, seed=S.SEEDS[1], step=(step0 + j) & 0xFFFFFFFF,
                   **dict(_chain_args(case, h), hist_len=h.shape[1]), **T.truncation_args(case))
        assert torch.equal(out.view(batch, width)[:, j], o1), j
        assert torch.equal(m.view(batch, width, V)[:, j], m1), j
        if j:
            m0 = torch.full((batch, V), 3, dtype=torch.uint8, device="cuda")
            hip.sample(rows_j, ld, batch, V, o1, keep_mask=m0, seed=S.SEEDS[1], step=(step0 + j) & 0xFFFFFFFF,
                       **_chain_args(case, hist_d), **T.truncation_args(case))
            moved += int((m0 != m1).any(1).sum())
    assert moved > 0                                                        # the tail history is visible in the kept sets


# ------------------------------------------------------------------------------------------------ 4. edges
@pytest.mark.parametrize("V,ld", [S.VLD[0], S.VLD[2]])
def test_rows_without_a_finite_score(hip, V, ld):
    rows = 4
    buf = _buf(torch.full((rows, V), float("-inf"), dtype=torch.bfloat16), ld)
    hist = torch.zeros(rows, 4, dtype=torch.int64, device="cuda")
    for name, s in T.SETTINGS.items():
        tok, mask = _launch(hip, dict(kernel="chain", V=V, **s), buf, hist, 99, 1)
        assert tok.tolist() == [0] * rows, name
        assert int(mask.sum()) == 0, name


def test_suppressed_entries_are_never_kept(hip):
    V, ld = S.VLD[1]
    logits, hist = T.rows_for(V, "suppressed")
    finite = torch.isfinite(logits.float())
    buf = _buf(logits, ld)
    for name, s in T.SETTINGS.items():
        tok, mask = _launch(hip, dict(kernel="chain", V=V, **s), buf, hist.cuda(), 99, 3)
        assert not bool((mask.cpu().bool() & ~finite).any()), name
        assert bool(finite[torch.arange(T.ROWS), torch.from_numpy(tok)].all()), name


@pytest.mark.parametrize("bad", [dict(typical_p=0.0), dict(typical_p=1.5), dict(typical_p=-0.1), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=-1e-3),
                                 dict(eta_cutoff=1.0), dict(eta_cutoff=-1e-3), dict(typical_p=float("nan"))])
def test_bad_arguments_are_rejected(hip, bad):
    V, ld = S.VLD[0]
    buf = _buf(torch.zeros(2, V, dtype=torch.bfloat16), ld)
    out = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="desta_sample_truncated_rows_bf16"):
        hip.sample(buf, ld, 2, V, out, **bad)
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [-7, -7]                                   # nothing launched
