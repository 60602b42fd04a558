"""Float64 reference, per-element error bounds in interval form, a conforming emulation and seeded mutations of the Whisper
log-mel front end (csrc/logmel.hip).  Plain torch, float64, device-agnostic (`operands(case, device)`); the only thing taken
from the library is the table blob of desta_logmel_fill_tables, which is pure host code.  Imported by the host test
(test_logmel_bound_host.py) and the GPU test (test_gpu_logmel_fp64.py), which share `CASES`.

Operands are what the kernel receives: the fp32 waveform [B, n], the fp32 window [400] and the fp32 filter bank [201, n_mels]
of the blob (taken as given) and the per-filter bin ranges.  The cos / sin twiddles of the blob are NOT operands: exact() uses
float64 trigonometry, and the fp32 rounding of the twiddles is part of the kernel's error.

    exact(o)   1 zero-pad / truncate to 480000 samples  2 reflect-pad by 200  3 3000 frames at hop 160  4 times the fp32 window
               5 400-point DFT in float64  6 |.|^2  7 the fp32 filter bank  8 log10(max(., 1e-10))
               9 per-clip max, clamp at max - 8, (x + 4) / 4                                       -> {"out": [B, n_mels, 3000], ...}
    bound(o, ref)          -> [B, n_mels, 3000], derivation below; no element is masked
    emulate(o, mutation)   -> [B, n_mels, 3000] float64 holding fp32 values: float64 arithmetic with one rounding to fp32 wherever
                              the kernel rounds, in the kernel's order (fold in place; n = 0 and n = 200 first with sign (-1)^k;
                              odd and even n accumulated apart; the twiddle index (k n) mod 400 kept incrementally; the pair
                              (k, 200 - k) from one pass; bin 100 written twice; the mel sum over [klo, khi) only; the block max
                              over t < 3000, then the clip max).  Not emulated: the device's log10f (float64 log10 rounded once)
                              and the compiler's choice of contraction in r r + i i (the fused form is used).

Bounds.  F = 2^-24, one fp32 rounding.  logmel.hip lines in brackets.  a[n] = |x[n] win[n]| (the exact product of two fp32
values), A[n] = a[n] + a[400 - n] for n = 1 .. 199, A[0] = a[0], A[200] = a[200]; c_kn = cos(2 pi k n / 400), s_kn likewise.
  window product [:52]      |xw^ - xw| <= F a[n]
  fold u +- v [:64-66]      one more rounding of a value of magnitude <= A[n]:  |e^[n] - e[n]|, |o^[n] - o[n]| <= 2 F A[n]
  fp32 twiddle [:44, :83]   |c^ - c| <= F |c| + 2^-52 (the table is (float) of a double cos; the 2^-52 covers cos(pi / 2) = 6e-17
                            instead of 0 and the double's own error)
  FMA chains [:88, :96-106] ee (n = 0, 200, then even n), eo (odd n), oe (even n), oo (odd n): the products are exact inside the
                            FMA; the term of sample n rides through d[n] = 100 - floor(n / 2) roundings of its accumulator
                            (d[0] = d[200] = 100: [:96] then 99 steps), each relative to a partial sum of magnitude <= sum |terms|
  final +- [:112]           one rounding, <= F sum |terms|
      dRe[k] = 1.001 (F sum_{n=0..200} (2 + 1 + d[n] + 1) A[n] |c_kn| + 2^-52 sum A),   dIm[k] likewise with |s_kn|, n = 1 .. 199
      (the shape c 2^-24 sum_n |xw[n] tw|, c <= 104; 1.001 swallows the second-order terms, which are below 1e-5 of the first)
  power [:113-114]          r r + i i as two products and an add, or one product and an FMA (-ffp-contract=fast: the compiler's
                            choice): either way each non-negative term passes at most 2 roundings
      dP = (1 + 2F)(2 |Re| dRe + dRe^2 + 2 |Im| dIm + dIm^2) + 2F P
  mel FMA chain [:126]      L = khi - klo terms, all >= 0:   dM = (1 + L F) fb . dP + L F M
  log [:127]                lv in [log10(max(M - dM, floor_lo)), log10(max(M + dM, floor_hi))] with floor_lo / floor_hi the smaller /
                            larger of 1e-10 and (float) 1e-10 (a kernel may apply the floor before the log, to the fp32 constant,
                            or after it, as fmaxf(log10f(.), -10); :127 does the latter), each end moved outwards by the
                            device's log10f error: 2 ulp (ROCm documentation, "HIP math API", single-precision table: log10f,
                            maximum error 2 ulp).  An element whose whole interval lies under the floor keeps only that: the
                            floor constant's and log10f's error.
  max, clamp [:131-140, :148-155]  fmaxf is exact and 1-Lipschitz: the clip max over the lower ends and over the upper ends;
                            floor_v = mx - 8 [:150] one rounding; max(lv, floor_v) on the interval ends
  (x + 4) 0.25 [:155]       one rounding (as x + 4 then an exact scaling, or fused)
  bound = the larger distance from exact to the two interval ends.  An all-zero clip: every mel sum is exactly 0, the floor applied
  after the log gives exactly -10, so the output is exactly -1.5 and the bound is 0.  (The floor applied BEFORE the log, as the
  kernel did until this was measured, gave log10f((float) 1e-10) = -10 + 1 ulp on the MI355X: silence came out as -1.4999998.)

`MUTATIONS`: seeded wrong variants of emulate(), each with the case that must catch it (test_logmel_bound_host.py)."""
import math

import torch

F = 2.0 ** -24
N_FFT, HOP, N_BINS, N_FRAMES, N_SAMPLES, FT, NBLK = 400, 160, 201, 3000, 480000, 32, 94
SR = 16000
TW_ABS = 2.0 ** -52
SLACK = 1.001
LOG10F_ULP = 2.0
OLD_ATOL = 2e-4                     # the whole-tensor tolerance of tests/test_gpu_kernels.py::test_logmel_matches_oracle
FLOOR32 = float(torch.tensor(1e-10, dtype=torch.float32))
FLOOR_LO, FLOOR_HI = min(1e-10, FLOOR32), max(1e-10, FLOOR32)

# name -> (what is wrong, the case that must show it beyond twice the bound)
MUTATIONS = {
    "hann_symmetric": ("symmetric instead of periodic Hann window", "b-tone-1000"),
    "n200_no_sign": ("the n = 200 term without its (-1)^k sign", "c-tone-1010"),
    "twiddle_unreduced": ("twiddle index not reduced mod 400 at n = 57: cos reads the sine table, sin reads past it (0)", "a-noise-128"),
    "pair_im_plus": ("oe - oo replaced by oe + oo for bin 200 - k", "b-tone-7960"),
    "left_reflect": ("left reflect s = -s - 1", "e-impulse-0"),
    "right_reflect": ("right reflect s = 2 * 480000 - 1 - s", "e-impulse-479999"),
    "khi_short": ("khi short by one", "a-noise-128"),
    "floor_1e-9": ("log floor 1e-9", "e-impulse-5120"),
    "clamp_7.99": ("clamp at max - 7.99", "a-noise-128"),
    "max_misses_last_block": ("clip max without the last block (frames 2976 .. 2999)", "e-impulse-frame-2999"),
    "max_over_batch": ("one max over the whole batch", "g-gains"),
}


def r32(x):
    """float64 -> nearest fp32 value, as float64"""
    return x.float().double()


def ulp32(v):
    """spacing of fp32 at |v| (2^-24 at 0)"""
    _, e = torch.frexp(v.abs())
    return torch.ldexp(torch.ones_like(v), e - 24)


def worst_ratio(err, bnd):
    """max |err| / bound; where the bound is 0 the error must be 0 (inf otherwise, and for a result that is not finite)."""
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    zero = bnd == 0
    if bool((zero & (err != 0)).any()):
        return float("inf")
    return float((err / torch.where(zero, torch.ones_like(bnd), bnd)).max())


# ------------------------------------------------------------------------------------------------------------ tables
def table_blob(n_mels):
    """the blob exactly as the kernel receives it: window | cos | sin | filter bank [201][n_mels] | ranges [n_mels][2], fp32"""
    from desta import _hip
    host = torch.empty(_hip.lib.desta_logmel_table_floats(n_mels), dtype=torch.float32)
    assert _hip._logmel_fill(n_mels, host.data_ptr()) == 0
    return host


def split_blob(blob, n_mels):
    fb0 = 3 * N_FFT
    rng = blob[fb0 + N_BINS * n_mels:].view(n_mels, 2)
    return {"win": blob[:N_FFT], "cos": blob[N_FFT:2 * N_FFT], "sin": blob[2 * N_FFT:fb0],
            "fb": blob[fb0:fb0 + N_BINS * n_mels].view(N_BINS, n_mels), "klo": rng[:, 0].long(), "khi": rng[:, 1].long()}


def hz_to_mel(f):
    return 15.0 + math.log(f / 1000.0) * (27.0 / math.log(6.4)) if f >= 1000.0 else 3.0 * f / 200.0


def mel_to_hz(m):
    return 1000.0 * math.exp((math.log(6.4) / 27.0) * (m - 15.0)) if m >= 15.0 else 200.0 * m / 3.0


def tables_fp64(n_mels):
    """the float64 formulas of every array of the blob (slaney scale and norm, 0 .. 8000 Hz; periodic Hann)"""
    n = torch.arange(N_FFT, dtype=torch.float64)
    ff = [mel_to_hz(hz_to_mel(8000.0) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    f = 8000.0 * torch.arange(N_BINS, dtype=torch.float64) / (N_BINS - 1)
    fb = torch.zeros(N_BINS, n_mels, dtype=torch.float64)
    for m in range(n_mels):
        down, up = (f - ff[m]) / (ff[m + 1] - ff[m]), (ff[m + 2] - f) / (ff[m + 2] - ff[m + 1])
        fb[:, m] = torch.minimum(down, up).clamp(min=0.0) * 2.0 / (ff[m + 2] - ff[m])
    return {"win": 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / N_FFT), "cos": torch.cos(2.0 * math.pi * n / N_FFT),
            "sin": torch.sin(2.0 * math.pi * n / N_FFT), "fb": fb}


# ------------------------------------------------------------------------------------------------------------ cases
def _noise(seed, B, n, amp):
    return amp * torch.randn(B, n, generator=torch.Generator().manual_seed(seed))


def _tones(*fa, n=N_SAMPLES):
    t = torch.arange(n, dtype=torch.float64) / SR
    return sum(a * torch.sin(2.0 * math.pi * f * t) for f, a in fa).float()[None]


def _impulse(i):
    w = torch.zeros(1, N_SAMPLES)
    w[0, i] = 1.0
    return w


def _a_noise():
    w = (0.1 * torch.randn(3, N_SAMPLES, generator=torch.Generator().manual_seed(1234))).clamp(-1, 1)
    w[1, 200000:] = 0.0
    w[2] *= torch.linspace(0, 1, N_SAMPLES)
    return w


def _chirp():
    t = torch.arange(N_SAMPLES, dtype=torch.float64) / SR
    return (0.5 * torch.sin(2.0 * math.pi * (20.0 * t + (7900.0 - 20.0) * t * t / (2 * 30.0)))).float()[None]


def _frame_2999():
    w = _noise(31, 1, N_SAMPLES, 1e-3)
    w[0, 479900] = 1.0                                   # frame 2999 spans 479640 ..; frame 2998 ends at 479879
    return w


def _burst():
    w = _noise(41, 1, N_SAMPLES, 1e-4)
    w[0, :SR] = _tones((440.0, 0.9), n=SR)[0]
    return w


def _case(name, wave, n_mels=128):
    return {"name": name, "wave": wave, "n_mels": n_mels, "family": name[0]}


CASES = [
    _case("a-noise-80", _a_noise, 80), _case("a-noise-128", _a_noise),
    _case("b-tone-40", lambda: _tones((40.0, 0.5))), _case("b-tone-1000", lambda: _tones((1000.0, 0.5))),
    _case("b-tone-4000", lambda: _tones((4000.0, 0.5))), _case("b-tone-7960", lambda: _tones((7960.0, 0.5))),
    _case("c-tone-1010", lambda: _tones((1010.0, 0.5))), _case("c-two-tones-60dB", lambda: _tones((1013.0, 0.9), (5017.0, 0.9e-3))),
    _case("c-chirp", _chirp),
    _case("d-dc", lambda: torch.full((1, N_SAMPLES), 0.25)),
    _case("d-nyquist", lambda: (0.5 * (1.0 - 2.0 * (torch.arange(N_SAMPLES) % 2).float()))[None]),
    _case("e-impulse-0", lambda: _impulse(0)), _case("e-impulse-199", lambda: _impulse(199)),
    _case("e-impulse-200", lambda: _impulse(200)), _case("e-impulse-5120", lambda: _impulse(5120)),
    _case("e-impulse-479999", lambda: _impulse(479999)), _case("e-impulse-frame-2999", _frame_2999),
    _case("f-len-1", lambda: _noise(51, 1, 1, 0.1)), _case("f-len-100", lambda: _noise(52, 1, 100, 0.1)),
    _case("f-len-201", lambda: _noise(53, 1, 201, 0.1)), _case("f-len-48017", lambda: _noise(54, 1, 48017, 0.1)),
    _case("f-len-485000", lambda: _noise(55, 1, 485000, 0.1)), _case("f-all-zero", lambda: torch.zeros(1, SR)),
    _case("g-gains", lambda: _noise(61, 3, N_SAMPLES, 0.1) * torch.tensor([1.0, 1e-3, 0.0])[:, None]),
    _case("h-burst-then-1e-4", _burst), _case("h-noise-3e-5", lambda: _noise(42, 1, N_SAMPLES, 3e-5)),
    _case("i-mels-3", lambda: _noise(71, 1, N_SAMPLES, 0.1), 3), _case("i-mels-256", lambda: _noise(71, 1, N_SAMPLES, 0.1), 256),
]
CASE_IDS = [c["name"] for c in CASES]
SHARE_LIMIT = 0.01                   # of elements with bound > OLD_ATOL, asserted for these:
SHARE_CASES = ("a-noise-80", "a-noise-128", "h-burst-then-1e-4", "h-noise-3e-5")
_BLOBS = {}


def operands(case, device="cpu"):
    """the seeded fp32 waveform [B, n] and the table blob as the kernel receives it, split into its arrays"""
    nm = case["n_mels"]
    if nm not in _BLOBS:
        _BLOBS[nm] = table_blob(nm)
    o = {"name": case["name"], "n_mels": nm, "wave": case["wave"]().to(device), "blob": _BLOBS[nm].to(device)}
    o.update(split_blob(o["blob"], nm))
    return o


# ------------------------------------------------------------------------------------------------------------ the front end
def _sample_index(device, mutation=None):
    """[3000, 400] index into the clip padded to 480000 samples: reflect padding by 200 (logmel.hip:48-50)"""
    s = (torch.arange(N_FRAMES, device=device) * HOP - N_FFT // 2)[:, None] + torch.arange(N_FFT, device=device)[None]
    s = torch.where(s < 0, -s - 1 if mutation == "left_reflect" else -s, s)
    return torch.where(s >= N_SAMPLES, (2 * N_SAMPLES - 1 if mutation == "right_reflect" else 2 * (N_SAMPLES - 1)) - s, s)


def _padded(w):
    """one clip, zero-padded / truncated to 480000 samples, float64"""
    p = torch.zeros(N_SAMPLES, dtype=torch.float64, device=w.device)
    m = min(N_SAMPLES, w.numel())
    p[:m] = w[:m].double()
    return p


def _trig(device):
    j = torch.arange(N_FFT, dtype=torch.float64, device=device)
    return torch.cos(2.0 * math.pi * j / N_FFT), torch.sin(2.0 * math.pi * j / N_FFT)


def _finish(lv, mutation=None, rnd=lambda v: v):
    """[B, T, n_mels] log values -> [B, n_mels, T]: the per-clip max, the clamp and the affine map (logmel.hip:131-155)"""
    B = lv.shape[0]
    if mutation == "max_misses_last_block":
        mx = lv[:, :(NBLK - 1) * FT].reshape(B, -1).max(1).values
    else:
        mx = lv.reshape(B, -1).max(1).values
    if mutation == "max_over_batch":
        mx = mx.max().expand(B)
    floor_v = rnd(mx - (7.99 if mutation == "clamp_7.99" else 8.0))
    return rnd(rnd(torch.maximum(lv, floor_v[:, None, None]) + 4.0) * 0.25).permute(0, 2, 1).contiguous()


def exact(o):
    dev = o["wave"].device
    idx, win, fb = _sample_index(dev), o["win"].double(), o["fb"].double()
    xs, Xs, Ms = [], [], []
    for w in o["wave"]:
        x = _padded(w)[idx] * win
        X = torch.fft.rfft(x, dim=-1)
        xs.append(x)
        Xs.append(X)
        Ms.append((X.real ** 2 + X.imag ** 2) @ fb)
    M = torch.stack(Ms)
    lv = torch.log10(M.clamp(min=1e-10))
    return {"out": _finish(lv), "x": xs, "X": Xs, "M": M, "lv": lv}


def bound(o, ref):
    """[B, n_mels, 3000]: the per-element bound of exact()'s result (the derivation is in the module docstring)."""
    dev = o["wave"].device
    fb = o["fb"].double()
    L = (o["khi"] - o["klo"]).double()
    n = torch.arange(N_BINS, device=dev)
    depth = torch.where((n == 0) | (n == 200), torch.full_like(n, 100), 100 - n // 2).double()
    wgt = (2.0 + 1.0 + depth + 1.0) * F
    c, s = _trig(dev)
    kn = (n[:, None] * n[None, :]) % N_FFT                                                 # [n, k]
    absc, abss = c[kn].abs(), s[kn].abs()
    abss[0], abss[200] = 0.0, 0.0
    lo, hi = [], []
    for b in range(o["wave"].shape[0]):
        a, X, M = ref["x"][b].abs(), ref["X"][b], ref["M"][b]
        A = a[:, :N_BINS].clone()
        A[:, 1:200] += a[:, 201:].flip(-1)                                                  # a[400 - n]
        tw = TW_ABS * A.sum(-1, keepdim=True)
        dre = SLACK * ((A * wgt) @ absc + tw)
        dim = SLACK * ((A * wgt) @ abss + tw)
        P = X.real ** 2 + X.imag ** 2
        dP = (1 + 2 * F) * (2 * X.real.abs() * dre + dre * dre + 2 * X.imag.abs() * dim + dim * dim) + 2 * F * P
        dM = (1 + L * F) * (dP @ fb) + L * F * M
        l = torch.log10((M - dM).clamp(min=FLOOR_LO))
        h = torch.log10((M + dM).clamp(min=FLOOR_HI))
        lo.append(l - LOG10F_ULP * ulp32(l))
        hi.append(h + LOG10F_ULP * ulp32(h))
    ends = []
    for lv in (torch.stack(lo), torch.stack(hi)):
        sgn = -1.0 if not ends else 1.0
        mx = lv.reshape(lv.shape[0], -1).max(1).values - 8.0
        floor_v = mx + sgn * F * mx.abs()
        z = (torch.maximum(lv, floor_v[:, None, None]) + 4.0) * 0.25
        ends.append((z + sgn * F * z.abs()).permute(0, 2, 1))
    bnd = torch.maximum(ref["out"] - ends[0], ends[1] - ref["out"]).clamp(min=0.0)
    for b, w in enumerate(o["wave"]):
        if not bool((w[:N_SAMPLES] != 0).any()):
            bnd[b] = 0.0
    return bnd


def _mel_acc(o, w, mutation):
    """one clip -> [3000, n_mels] mel sums as the kernel holds them (logmel.hip:44-126)"""
    dev = w.device
    win = o["win"].double()
    if mutation == "hann_symmetric":
        win = r32(0.5 - 0.5 * torch.cos(2.0 * math.pi * torch.arange(N_FFT, dtype=torch.float64, device=dev) / (N_FFT - 1)))
    xs = r32(_padded(w)[_sample_index(dev, mutation)] * win)                               # :52
    E, O = xs[:, :N_BINS].clone(), torch.zeros_like(xs[:, :N_BINS])
    rev = xs[:, 201:].flip(-1)                                                              # xs[400 - n], n = 1 .. 199
    E[:, 1:200] = r32(xs[:, 1:200] + rev)                                                   # :65
    O[:, 1:200] = r32(xs[:, 1:200] - rev)                                                   # :66
    cos, sin = o["cos"].double(), o["sin"].double()
    flat = torch.cat([cos, sin, torch.zeros_like(cos)])                                     # cos | sin | what the emulation reads past them
    k = torch.arange(101, device=dev)
    sg = torch.where(k % 2 == 1, -1.0, 1.0).double()
    if mutation == "n200_no_sign":
        sg = torch.ones_like(sg)
    ee = r32(E[:, 200:201] * sg + E[:, 0:1])                                                # :96
    eo, oe, oo = torch.zeros_like(ee), torch.zeros_like(ee), torch.zeros_like(ee)
    ti = torch.zeros_like(k)
    for n in range(1, 200):                                                                 # :99-106
        ti = ti + k
        over = ti >= N_FFT
        if mutation == "twiddle_unreduced" and n == 57:
            cc, ss = flat[ti], flat[N_FFT + ti]
        else:
            cc = ss = None
        ti = torch.where(over, ti - N_FFT, ti)
        if cc is None:
            cc, ss = cos[ti], sin[ti]
        if n % 2:
            eo = r32(torch.addcmul(eo, E[:, n:n + 1], cc))                                  # :88
            oo = r32(torch.addcmul(oo, O[:, n:n + 1], ss))
        else:
            ee = r32(torch.addcmul(ee, E[:, n:n + 1], cc))
            oe = r32(torch.addcmul(oe, O[:, n:n + 1], ss))
    r1, i1, r2 = r32(ee + eo), r32(oe + oo), r32(ee - eo)                                   # :112
    i2 = r32(oe + oo) if mutation == "pair_im_plus" else r32(oe - oo)
    pw = torch.zeros(xs.shape[0], N_BINS, dtype=torch.float64, device=dev)
    pw[:, :101] = r32(r1 * r1 + r32(i1 * i1))                                               # :113
    pw[:, 100:] = r32(r2 * r2 + r32(i2 * i2)).flip(-1)                                      # :114, bin 100 written a second time
    fb, klo, khi = o["fb"].double(), o["klo"], o["khi"]
    if mutation == "khi_short":
        khi = torch.maximum(khi - 1, klo)
    acc = torch.zeros(xs.shape[0], o["n_mels"], dtype=torch.float64, device=dev)
    m = torch.arange(o["n_mels"], device=dev)
    for j in range(int((khi - klo).max())):                                                 # :126
        kk = (klo + j).clamp(max=N_BINS - 1)
        acc = torch.where((klo + j < khi)[None], r32(torch.addcmul(acc, pw[:, kk], fb[kk, m][None])), acc)
    return acc


def mel_sums(o, mutation=None):
    """[B, 3000, n_mels]: the mel sums of every clip; pass them back to emulate() for mutations past the mel product"""
    return torch.stack([_mel_acc(o, w, mutation) for w in o["wave"]])


POST_MEL = ("floor_1e-9", "clamp_7.99", "max_misses_last_block", "max_over_batch")


def emulate(o, mutation=None, acc=None):
    assert mutation is None or mutation in MUTATIONS
    if acc is None or mutation not in POST_MEL:
        acc = mel_sums(o, mutation)
    lv = r32(torch.log10(acc)).clamp(min=-9.0 if mutation == "floor_1e-9" else -10.0)       # :127, the floor after the log
    return _finish(lv, mutation, r32)


def share_above_old_tolerance(bnd):
    return float((bnd > OLD_ATOL).double().mean())
