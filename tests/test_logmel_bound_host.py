"""Host (no GPU): the per-element fp64 criterion of tests/logmel_reference.py is proved before it is pointed at the kernel.

Over the SAME case table the GPU test runs (logmel_reference.CASES, every element of every output, none excluded):
  (a) the conforming emulation stays inside the bound (worst |err| / bound <= 1; printed per case with -s, with the median bound
      and the share of elements whose bound exceeds the old whole-tensor tolerance 2e-4);
  (b) that share stays at or under 1 % on the noise cases and on every case of family h, so that a later, looser bound cannot pass
      unnoticed (the shares of the leakage cases c are elements near the floor, ill-conditioned; they are printed, not asserted);
  (c) every seeded mutation (logmel_reference.MUTATIONS) exceeds TWICE the bound (the GPU test's `FACTOR`) on its named case;
  (d) every array of the table blob - window, cos, sin, filter bank, ranges - equals its float64 formula rounded once to fp32,
      for n_mels 1, 3, 80, 128 and 256 (the twiddles to half an fp32 ulp; the ranges exactly; an empty filter gives (0, 0));
  (e) desta_logmel_fill_tables rejects n_mels 0 and 257 and writes nothing.
Measured figures: the table in DESIGN.md ("Log-mel against fp64")."""
import pytest
import torch

import logmel_reference as R

FACTOR = 2.0                # of test_gpu_logmel_fp64.py: a mutation counts as rejected only beyond it
OLD_INPUT = "a-noise-128"    # the waveform of tests/test_gpu_kernels.py::test_logmel_matches_oracle
_KEEP = {c for _, c in R.MUTATIONS.values()} | {OLD_INPUT}
_REF = {}


def _reference(name):
    """(operands, exact output, bound, the emulation's mel sums) of a case; kept for the cases the mutations name"""
    if name in _REF:
        return _REF[name]
    o = R.operands(R.CASES[R.CASE_IDS.index(name)])
    ref = R.exact(o)
    res = (o, ref["out"], R.bound(o, ref), R.mel_sums(o))
    if name in _KEEP:
        _REF[name] = res
    return res


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_emulation_is_inside_the_bound(name):
    o, out, bnd, acc = _reference(name)
    emu = R.emulate(o, acc=acc)
    assert out.shape == bnd.shape == emu.shape == (o["wave"].shape[0], o["n_mels"], R.N_FRAMES)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(bnd).all()) and bool((bnd >= 0).all())
    ratio = R.worst_ratio((emu - out).abs(), bnd)
    share = R.share_above_old_tolerance(bnd)
    print(f"\n{name}: emulation worst |err| / bound {ratio:.3f}; median bound {float(bnd.median()):.2e}, "
          f"{100 * share:.2f} % of elements with bound > {R.OLD_ATOL:g}", end="")
    assert ratio <= 1.0, (name, ratio)
    if name in R.SHARE_CASES:
        assert share <= R.SHARE_LIMIT, (name, share)
    if name == "f-all-zero":
        assert bool((bnd == 0).all()) and bool((out == -1.5).all()) and bool((emu == -1.5).all())
    if name == "g-gains":
        assert bool((bnd[2] == 0).all()) and bool((out[2] == -1.5).all()) and bool((bnd[:2] > 0).all())


def test_share_condition_covers_noise_and_family_h():
    assert {c["name"] for c in R.CASES if c["family"] == "h"} | {"a-noise-80", "a-noise-128"} == set(R.SHARE_CASES)


@pytest.mark.parametrize("mut", list(R.MUTATIONS))
def test_mutation_exceeds_the_bound(mut):
    what, name = R.MUTATIONS[mut]
    o, out, bnd, acc = _reference(name)
    emu, wrong = R.emulate(o, acc=acc), R.emulate(o, mut, acc=acc)
    err = (wrong - out).abs()
    ratio = R.worst_ratio(err, bnd)
    beyond = float((err > FACTOR * bnd).double().mean())
    old = bool((err <= R.OLD_ATOL).all())
    print(f"\n{mut} ({what}) on {name}: worst |err| / bound {ratio:.3g}, {100 * beyond:.2f} % of elements beyond {FACTOR:g} x bound; "
          f"max |err| {float(err.max()):.2g}: the old tolerance {R.OLD_ATOL:g} {'PASSES it' if old else 'rejects it too'}", end="")
    # the same mutation as the old test saw it: its input (a-noise-128), its one whole-tensor tolerance
    o2, out2, _, acc2 = _reference(OLD_INPUT)
    err2 = float((R.emulate(o2, mut, acc=acc2) - out2).abs().max())
    print(f"; on the old test's input max |err| {err2:.2g}: {'PASSES' if err2 <= R.OLD_ATOL else 'rejected'}", end="")
    assert not torch.equal(wrong, emu)
    assert ratio > FACTOR, (mut, name, ratio)


def _half_ulp(tab, f64, rel=2.0 ** -45, tiny=0.0):
    """|fp32 table - float64 formula| <= half an fp32 ulp of the formula's value (+ the slack of the two float64 evaluations)"""
    err = (tab.double() - f64).abs()
    lim = 0.5 * R.ulp32(f64) + rel * f64.abs() + tiny
    return bool((err <= lim).all()), float((err / (0.5 * R.ulp32(f64))).max())


@pytest.mark.parametrize("n_mels", [1, 3, 80, 128, 256])
def test_table_blob_against_fp64_formulas(n_mels):
    blob = R.table_blob(n_mels)
    assert blob.numel() == 3 * R.N_FFT + R.N_BINS * n_mels + 2 * n_mels
    t, f = R.split_blob(blob, n_mels), R.tables_fp64(n_mels)
    worst = {}
    for key in ("win", "cos", "sin"):
        # 2^-52: cos(pi / 2) and sin(pi) of a double argument are 6e-17 and 1e-16, not 0, on either side
        ok, worst[key] = _half_ulp(t[key], f[key], tiny=2.0 ** -52)
        assert ok, (key, worst[key])
    assert float(t["win"][0]) == 0.0 and float(t["win"][200]) == 1.0 and torch.equal(t["win"][1:], t["win"][1:].flip(0))   # periodic
    assert float(t["cos"][0]) == 1.0 and float(t["cos"][200]) == -1.0 and float(t["sin"][100]) == 1.0 and float(t["sin"][300]) == -1.0
    ok, worst["fb"] = _half_ulp(t["fb"], f["fb"], tiny=1e-15)
    assert ok, worst["fb"]
    assert bool((t["fb"] >= 0).all()) and float(t["fb"][0].max()) == 0.0 and float(t["fb"][200].max()) == 0.0        # DC and Nyquist weigh nothing
    empty = 0
    for m in range(n_mels):
        nz = torch.nonzero(t["fb"][:, m])[:, 0]
        want = (int(nz[0]), int(nz[-1]) + 1) if nz.numel() else (0, 0)
        empty += nz.numel() == 0
        assert (int(t["klo"][m]), int(t["khi"][m])) == want, (m, want)
        assert bool((t["fb"][want[0]:want[1], m] > 0).all())                   # a triangle: no zero inside its range
    rng = blob[3 * R.N_FFT + R.N_BINS * n_mels:]
    assert torch.equal(rng, rng.round()) and bool((rng >= 0).all()) and bool((rng <= R.N_BINS).all())
    print(f"\nn_mels {n_mels}: worst error in half ulps " + " ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; {empty} empty filters, longest range {int((t['khi'] - t['klo']).max())}", end="")
    assert (empty > 0) == (n_mels == 256)                                       # the lo = hi = 0 branch runs at 256 only


def test_fill_tables_rejects_bad_n_mels():
    from desta import _hip
    host = torch.full((4096,), 7.0)
    for n_mels in (0, 257, -1):
        assert _hip._logmel_fill(n_mels, host.data_ptr()) == -1
        assert b"n_mels" in _hip.lib.desta_last_error()
    assert _hip._logmel_fill(128, None) == -1
    assert bool((host == 7.0).all())
    big = torch.empty(_hip.lib.desta_logmel_table_floats(256))
    assert _hip._logmel_fill(1, host.data_ptr()) == 0 and _hip._logmel_fill(256, big.data_ptr()) == 0


def test_case_table_reaches_what_it_names():
    """the inputs do what their names say: the frames and blocks they land in, the floor and the clamp they reach"""
    idx = R._sample_index("cpu")
    assert int(idx[0, 0]) == 200 and int(idx[0, 200]) == 0 and int(idx[2999, 399]) == 2 * 479999 - 480039
    assert [int(t) for t in torch.nonzero((idx == 479900).any(1))[:, 0]] == [2999]          # e-impulse-frame-2999: that frame only
    assert int(torch.nonzero((idx == 5120).any(1))[0, 0]) == 31 and (5120 + 200) // R.HOP + 1 > R.FT  # 5120 reaches into block 1
    assert (R.NBLK - 1) * R.FT == 2976
    by = {c["name"]: c for c in R.CASES}
    assert {c["family"] for c in R.CASES} == set("abcdefghi") and len(R.CASES) == len(set(R.CASE_IDS))
    assert {c["n_mels"] for c in R.CASES} == {3, 80, 128, 256}
    assert [by[n]["wave"]().shape[1] for n in ("f-len-1", "f-len-100", "f-len-201", "f-len-48017", "f-len-485000")] == \
        [1, 100, 201, 48017, 485000]
    assert all(by[n]["wave"]().shape[0] == 3 for n in ("a-noise-80", "a-noise-128", "g-gains"))
    # the quiet clips: the maximum is below -2, so max - 8 is below the floor's -10 and the floor itself is what comes out
    for name, clip in (("g-gains", 1), ("h-noise-3e-5", 0)):
        o = R.operands(by[name])
        lv = R.exact(o)["lv"][clip]
        assert float(lv.max()) < -2.0, (name, float(lv.max()))
    # the loud ones: the clamp at max - 8 is active on values above the floor (not only on exact zeros)
    o = R.operands(by["c-two-tones-60dB"])
    ref = R.exact(o)
    lv = ref["lv"][0]
    assert bool(((lv > -10.0) & (lv < lv.max() - 8.0)).any())
