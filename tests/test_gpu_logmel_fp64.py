"""GPU: the log-mel front end (csrc/logmel.hip through desta_logmel_f32) held PER ELEMENT to a float64 reference, and
desta_mel_to_rows (mel_rows_k, csrc/norm_act.hip) held bit for bit to its header contract.

Reference, bounds in interval form with their derivation, the conforming emulation and the mutations: tests/logmel_reference.py.
The instrument is proved on the CPU by tests/test_logmel_bound_host.py over the case table this file runs (logmel_reference.CASES).

Per case  |out - fp64| <= 2 x bound  on every element (`FACTOR`: what the emulation leaves out - the device's log10f against a
correctly rounded one, the contraction the compiler chose in r r + i i; where the bound is 0 the output must be exactly -1.5),
and `max |err| / bound` is printed per case (run with -s).  Every launch goes through the C entry point with
    * the output buffer filled with a sentinel and 64 guard floats behind it,
    * a workspace of exactly batch * 94 floats with guards behind it,
    * wave_stride = n + 24 with NaN in the gap (and NaN past sample 480000 of the clip that is truncated):
the guards must be untouched, every output element written and finite.  Each case is run twice (bit-identical).

What a kernel error turns red here while the white-noise tests of test_gpu_kernels.py stay green: test_logmel_bound_host.py (host
evidence) and DESIGN.md, "Log-mel against fp64" (one hand-mutated kernel run on the MI355X).
Measured on the MI355X: profiles/r18_logmel_fp64_tests.log."""
import numpy as np
import pytest
import torch

import logmel_reference as R

pytestmark = pytest.mark.gpu

FACTOR = 2.0
GUARD = 64
SENTINEL = 12345.0
EINVAL = -1


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(hip, wave, n_mels, gap=24):
    """wave [B, n] fp32 (cpu) -> [B, n_mels, 3000] through desta_logmel_f32 with guarded buffers and a strided, NaN-padded waveform"""
    B, n = wave.shape
    wbuf = torch.full((B, n + gap), float("nan"), device="cuda")
    wbuf[:, :n] = wave.cuda()
    per = n_mels * R.N_FRAMES
    obuf = torch.full((B * per + GUARD,), SENTINEL, device="cuda")
    assert hip.lib.desta_logmel_workspace_floats(B) == B * R.NBLK
    ws = torch.full((B * R.NBLK + GUARD,), SENTINEL, device="cuda")
    tb = hip.logmel_tables(n_mels, wbuf.device)
    assert tb.numel() == hip.lib.desta_logmel_table_floats(n_mels)
    hip.check(hip._logmel(wbuf.data_ptr(), B, n, n + gap, tb.data_ptr(), n_mels, obuf.data_ptr(), ws.data_ptr(), hip.stream()),
              "desta_logmel_f32")
    torch.cuda.synchronize()
    assert bool((obuf[B * per:] == SENTINEL).all()), "guard behind the output written"
    assert bool((ws[B * R.NBLK:] == SENTINEL).all()), "guard behind the workspace written"
    out = obuf[:B * per].view(B, n_mels, R.N_FRAMES)
    assert bool(torch.isfinite(out).all()) and not bool((out == SENTINEL).any()), "an output element not written, or NaN read"
    assert bool(torch.isfinite(ws[:B * R.NBLK]).all()) and not bool((ws[:B * R.NBLK] == SENTINEL).any())
    return out


def _wave_for_device(case):
    w = case["wave"]()
    if w.shape[1] > R.N_SAMPLES:
        w[:, R.N_SAMPLES:] = float("nan")                   # truncated: never read
    return w


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_logmel_against_fp64(hip, case):
    o = R.operands(case)
    ref = R.exact(o)
    bnd = R.bound(o, ref)
    wave = _wave_for_device(case)
    out = _launch(hip, wave, case["n_mels"])
    assert torch.equal(_bits(out), _bits(_launch(hip, wave, case["n_mels"]))), "two runs differ"
    err = (out.cpu().double() - ref["out"]).abs()
    ratio = R.worst_ratio(err, bnd)
    print(f"\n{case['name']}: kernel worst |err| / bound {ratio:.3f}, max |err| {float(err.max()):.2e}; median bound "
          f"{float(bnd.median()):.2e}, {100 * R.share_above_old_tolerance(bnd):.2f} % of elements with bound > {R.OLD_ATOL:g}", end="")
    assert ratio <= FACTOR, (case["name"], ratio)
    for b, w in enumerate(o["wave"]):
        if not bool((w[:R.N_SAMPLES] != 0).any()):
            assert bool((out[b] == -1.5).all())


def test_each_clip_alone_gives_its_rows_of_the_batch(hip):
    """the clip max is per clip: gains 1, 1e-3 and 0 in one batch, and each clip at B = 1"""
    case = R.CASES[R.CASE_IDS.index("g-gains")]
    wave = case["wave"]()
    batched = _launch(hip, wave, 128)
    for b in range(wave.shape[0]):
        alone = _launch(hip, wave[b:b + 1], 128)
        assert torch.equal(_bits(alone[0]), _bits(batched[b])), b
    assert float(batched[0].max()) > float(batched[1].max()) + 0.5 > float(batched[2].max()) + 0.5


def test_binding_with_and_without_out_equals_the_strided_call(hip):
    case = R.CASES[R.CASE_IDS.index("a-noise-80")]
    wave = case["wave"]()
    strided = _launch(hip, wave, 80)
    dev = wave.cuda()
    fresh = hip.logmel(dev, 80)
    pre = torch.full((3, 80, R.N_FRAMES), SENTINEL, device="cuda")
    assert hip.logmel(dev, 80, out=pre) is pre
    torch.cuda.synchronize()
    assert torch.equal(_bits(fresh), _bits(strided)) and torch.equal(_bits(pre), _bits(strided))


def test_entry_point_rejects_bad_arguments_and_launches_nothing(hip):
    wave = torch.zeros(1, 1600, device="cuda")
    tb = hip.logmel_tables(128, wave.device)
    obuf = torch.full((128 * R.N_FRAMES + GUARD,), SENTINEL, device="cuda")
    ws = torch.full((R.NBLK,), SENTINEL, device="cuda")
    w, t, o, s, st = wave.data_ptr(), tb.data_ptr(), obuf.data_ptr(), ws.data_ptr(), hip.stream()
    bad = {"n_mels 0": (w, 1, 1600, 1600, t, 0, o, s, st), "n_mels 257": (w, 1, 1600, 1600, t, 257, o, s, st),
           "batch 0": (w, 0, 1600, 1600, t, 128, o, s, st), "no samples": (w, 1, 0, 1600, t, 128, o, s, st),
           "misaligned out": (w, 1, 1600, 1600, t, 128, o + 4, s, st),
           "null wave": (None, 1, 1600, 1600, t, 128, o, s, st), "null tables": (w, 1, 1600, 1600, None, 128, o, s, st),
           "null out": (w, 1, 1600, 1600, t, 128, None, s, st), "null workspace": (w, 1, 1600, 1600, t, 128, o, None, st)}
    for what, args in bad.items():
        assert hip._logmel(*args) == EINVAL, what
        assert b"logmel" in hip.lib.desta_last_error()
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((ws == SENTINEL).all())


@pytest.mark.parametrize("C,T,Cp", [(128, 3000, 128), (80, 3000, 128), (3, 65, 64), (128, 64, 192)])
def test_mel_to_rows_writes_what_the_header_says(hip, C, T, Cp):
    """rows 0 and T + 1 stay as the caller left them (a sentinel here, not zeros), channels [C, Cp) of rows 1 .. T are written
    as zero, everything else is RNE-bf16 of the input, bit for bit; nothing behind the buffer is touched"""
    B = 2
    g = torch.Generator().manual_seed(1000 * C + T)
    mel = torch.randn(B, C, T, generator=g) * 2.0 ** torch.randint(-8, 4, (B, C, T), generator=g).float()
    mel[0, 0, :8] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, -0.0, 3.0e38, -1.5, 1 + 2.0 ** -8 + 2.0 ** -20])
    sent = torch.tensor(-1234.0, dtype=torch.bfloat16)
    n = B * (T + 2) * Cp
    buf = torch.full((n + GUARD,), float(sent), dtype=torch.bfloat16, device="cuda")
    hip.mel_to_rows(mel.cuda(), Cp, buf)
    torch.cuda.synchronize()
    want = torch.full((B, T + 2, Cp), float(sent), dtype=torch.bfloat16)
    want[:, 1:T + 1, :C] = mel.permute(0, 2, 1).to(torch.bfloat16)
    want[:, 1:T + 1, C:] = 0.0
    got = buf.cpu()
    assert bool((got[n:] == sent).all()), "guard behind the rows written"
    got = got[:n].view(B, T + 2, Cp)
    assert bool((got[:, 0] == sent).all()) and bool((got[:, T + 1] == sent).all()), "a pad row written"
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_processor_on_ragged_numpy_clips(hip):
    from desta.utils.audio import HipLogMelProcessor, pad_or_trim
    rng = np.random.default_rng(5)
    clips = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (1, 16000, 48017, 480000, 485000)]
    feats = HipLogMelProcessor(128, "cuda:0")(clips, sampling_rate=16000).input_features
    ref = hip.logmel(pad_or_trim(clips).cuda(), 128)
    assert feats.shape == (5, 128, R.N_FRAMES) and feats.is_cuda
    assert torch.equal(_bits(feats), _bits(ref))
