"""GPU: the training attention kernels (desta_attention_fwd / desta_attention_bwd) held PER ELEMENT to a float64 reference.

Reference, bounds, their derivation, the conforming emulation and the rounding points of csrc/attention.hip it reproduces:
tests/attention_reference.py.  The instrument itself is proved on the CPU by tests/test_attention_bound_host.py.

Every entry of test_gpu_ops.ATTN_CASES (same operands: attention_reference.operands repeats that test's draws) runs forward,
backward (dQ, dK, dV) and the dQ-only backward once.  Asserted for O, dQ, dK, dV and the dQ-only dQ:
    worst |out - fp64| / bound  <=  min(2, 2 x the emulation's worst ratio on the same case and tensor)
(the emulation's ratio comes from the emulation and the fp64 reference alone; the emulation is the one of the forward that ran,
`fwd8` for the 8-wave kernel: it rounds P against its deferred reference, attention.hip:668-677, i.e. other values than the
4-wave kernel; the factor 2 is for what the emulation leaves out: fp32 accumulation order, exp2, lse in fp32).  Where the reference is exactly 0
(padded query rows, keys in front of kv_start) the output must be exactly 0; every output buffer starts as 7.0, so a region a
kernel does not write fails too.  lse (log2 domain): |lse - fp64| <= 1e-4 (1 + |fp64|) on rows with a visible key, +inf elsewhere.
Further cases: O_f32 feeding delta (bound with Ed = 0); dkv_transposed + dkv_bias_grad; dropout (p = 0.1, the DROP kernels, with the
mask of tests/dropout_reference.py planted in reference and emulation: test_attention_dropout_fp64, whose kernels sit on the
emulation too: O 0.171-0.604, dQ 0.179-0.379, dK 0.351-0.720, dV 0.390-0.779, profiles/r24_dropout_mask_tests.log); and, in
test_gpu_ops.py, the spike operands of test_attention_deferred_rescale_threshold.

Switches.  desta_attention_set_option / desta_attention_set_concurrent_bwd select kernel instantiations and launch orders; each
setting is run on the ATTN_CASES whose dispatch it changes (worked out from desta_attention_fwd / desta_attention_bwd,
`_switch_cases` below), held to the same assertion, and compared with the default run (`_agree`): bit for bit where the setting
leaves the arithmetic alone (`BIT_IDENTICAL`, argued from the code there), to ONE bound elsewhere:
    setting                reaches                                                                 on
    option 0 = 0           attn_fwd_k<D,false,4>; attn_delta_k + attn_bwd_dq_k<D,false,4> +        seq_q >= 128
                           attn_bwd_dkdv_k<D,false> (D = 128: dQ on the side stream)
    option 1 = 1           attn_fwd8_k<64,false,1,4,false> (two blocks per CU)                     D = 64, not causal, seq_q >= 128
    option 2 = 1           attn_fwd8_k<128,true,4,2,true>, attn_fwd8_k<64,false,1,2,true>          D = 128 causal with 4 | group size;
                           (waves 4-7 half a tile behind, three-slot ring)                         D = 64 not causal; seq_q >= 128
    option 3 = 1           forward unchanged; backward as under option 0 = 0                       seq_q >= 128
    option 4 = 0           attn_delta_k + attn_bwd_dq_k<64,false,2> + attn_bwd_dkdv_k<64,false>    D = 64, seq_q <= 64, seq_k >= 256,
                           instead of attn_bwd_q64_k + attn_dq_sum_k                               not causal, no GQA
    option 5 = 1           attn_bwd_dkdv_k<128,false,2> (64-key blocks)                            D = 128 causal, seq_q >= 128
    concurrent_bwd(False)  attn_bwd_dq_k<128> and attn_bwd_dkdv_k<128> on ONE stream               D = 128 on the 4-wave backward
With default options no entry of ATTN_CASES reaches the 4-wave D = 128 backward (all have seq_q >= 128), so concurrent_bwd(False)
changes no default dispatch there; it is run together with option 3 = 1 on the D = 128 cases and on the O_f32 case (O_f32 sends
the backward to the 4-wave path), where the header promises identical results: asserted bit for bit.
Preconditions, by reading: option 2's header note ("LLM / Whisper shapes only") is a statement about speed.  The staggered
instantiation takes the same ragged / padded / empty-range paths as the lockstep one (row-clamped loads, wave_on, wave_kmax,
the same number of barriers in both wave halves for any t_hi - t_lo >= 0), its ring of three slots is written for tile t + 3
only after the barrier behind the last read of tile t, and 3 x 32 KB (D = 128) fits the CU's LDS; MINW = 4 (option 1) and the
2-wave dK / dV blocks (option 5: tile_load with 128 threads, LDS_EPI = 2 x 8 KB) change no index arithmetic.  The dispatcher
needs no further check.

Measured (MI355X; profiles/r12_attention_fp64_tests.log), worst |err| / bound over the cases that reach the path, the emulation's
ratio on the same case and tensor in brackets.  The kernels sit ON their emulation: the figures agree to the three digits printed
on every path, case and tensor, except dQ 0.189 (0.195) of the one-pass backward at 64 x 600.
    forward, 4 waves (seq_q < 128, or option 0 = 0)       O 0.780 (0.780)
    forward, 8 waves (default, options 1 and 2)            O 0.780 (0.780); where the deferred reference shows: 0.533 (0.533; 4-wave
                                                           emulation 0.363) 333 x 333, 0.459 (0.459; 0.431) 200 x 260, 0.226 (0.226;
                                                           0.188) 1500 x 1500, 0.234 (0.234; 0.194) 130 x 700
    dQ, 8 waves (default)                                  dQ 0.369 (0.369)
    dQ, 4 waves (seq_q < 128, options 0 = 0, 3 = 1, O_f32) dQ 0.369 (0.369); 0.861 (0.861) with O_f32 (Ed = 0 in the bound)
    dK / dV, 128-key blocks (default)                      dK 0.688 (0.688); dV 0.880 (0.880)
    dK / dV, 64-key blocks (option 5 = 1)                  the default's bits (asserted)
    one query tile (default; option 4 = 0 beside it)       dQ 0.324 (0.324), dK 0.688 (0.688), dV 0.751 (0.751)
    transposed dK | dV + bias sums                         the row-major bits; bias 0.0095 (0.0096) dK, 0.0075 (0.0074) dV of the summed
                                                           bound, 0.042 (0.043) / 0.039 (0.039) of the half-ulp sum of the stored elements
    spike operands (test_gpu_ops.py)                       8 waves 0.221 / 0.293 at spike 3.0 (4-wave emulation 0.193 / 0.229), 0.417-0.479
                                                           at 6.5 and 40; 4 waves 0.193-0.479, equal to its emulation
    lse                                                    |lse - fp64| / (1 + |fp64|) <= 1.9e-7 on every path (limit 1e-4)
    default against switched run, of ONE bound             option 0 = 0 (8- against 4-wave forward, independent roundings of P): O 0.841
                                                           at 333 x 333 (limit 1.066), 0.402 at 1500 x 1500 (0.452), dK 1.099 at 640 x 640
                                                           (1.124: one ulp apart where the bound is the store's half ulp); option 3 = 1
                                                           dQ <= 0.333 (0.598); option 4 = 0 dQ <= 0.266; everything else bit for bit
"""
import pytest
import torch

import attention_reference as R
import dropout_reference as DR
from test_attention_bound_host import DROPOUT_CASES, DROPOUT_P, DROPOUT_SEED
from test_gpu_ops import ATTN_CASES

pytestmark = pytest.mark.gpu

DEFAULTS = {0: 1, 1: 0, 2: 0, 3: 0, 4: 1, 5: 0}
O_F32_CASE = (2, 4, 2, 160, 160, 128, True, [0, 37])
O_F32_FLAT = (2, 3, 3, 64, 1500, 64, False, None)          # the regime O_f32 exists for: flat softmax over 1500 keys, one-pass backward
TRANSPOSED_CASE = (2, 3, 3, 64, 1500, 64, False, None)


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


class Prepared:
    """Operands, fp64 reference, emulation ratios and device copies of one case: built once per module."""

    def __init__(self, case, o_f32, reference=True, dropout=None):
        self.case, self.o_f32, self.dropout = case, o_f32, dropout
        self.ops = R.operands(case)
        if reference:                                      # (tools/attention_bits.py digests the outputs: no reference)
            keep = drop_scale = None
            if dropout is not None:                        # (p, seed): the mask of tests/dropout_reference.py, not the kernels'
                B, Hq, Hkv, Sq, Sk = case[:5]
                keep, drop_scale = torch.from_numpy(DR.attn_keep(dropout[1], B, Hq, Sq, Sk, dropout[0])), DR.drop_scale(dropout[0])
            self.ref, self.emu, self.emu_ratio = R.reference(self.ops, o_f32=o_f32, keep=keep, drop_scale=drop_scale)
        self.dev = None
        self.default = None                                # outputs of the default switches (test_attention_fwd_bwd_fp64 or first use)

    def device(self):
        if self.dev is None:
            o = self.ops
            qd = o["qb"].cuda()
            kvd = qd if o["fused"] else o["kvb"].cuda()
            self.dev = (qd, kvd, o["do_b"].cuda(), o["kv_start"].cuda() if o["kv_start"] is not None else None)
        return self.dev


_CASES = {}


def _prepared(case, o_f32=False, dropout=None):
    key = (repr(case), o_f32, dropout)
    if key not in _CASES:
        _CASES[key] = Prepared(case, o_f32, dropout=dropout)
    return _CASES[key]


def _run(hip, P):
    """forward, backward, dQ-only backward -> {"O", "dQ", "dK", "dV", "dQ_only"} bf16 [B, S, H, D] and "lse" [B, Hq, Sq] on the CPU"""
    B, Hq, Hkv, Sq, Sk, D, causal, pad = P.case
    o_ = P.ops
    qd, kvd, dod, kvs = P.device()
    wq, wkv = Hq * D, Hkv * D
    o = torch.full((B * Sq, wq), 7.0, dtype=torch.bfloat16, device="cuda")
    o32 = torch.full((B * Sq, wq), 7.0, dtype=torch.float32, device="cuda") if P.o_f32 else None
    lse = torch.full((B, Hq, Sq), 7.0, device="cuda")
    d = hip.attn_desc(qd, kvd, kvd, o, lse, batch=B, hq=Hq, hkv=Hkv, sq=Sq, sk=Sk, hd=D, scale=o_["scale"], causal=causal,
                      kv_start=kvs, q_off=o_["q_off"], k_off=o_["k_off"], v_off=o_["v_off"], o_f32=o32,
                      dropout_p=P.dropout[0] if P.dropout else 0.0, dropout_seed=P.dropout[1] if P.dropout else 0)
    hip.attention_fwd(d)
    if o_["fused"]:
        dqkv = torch.full((B * Sq, wq + 2 * wkv), 7.0, dtype=torch.bfloat16, device="cuda")
        hip.attention_bwd(d, dod, dqkv, dqkv, dqkv, dq_off=0, dk_off=wq, dv_off=wq + wkv)
        gq, gk, gv = dqkv[:, :wq], dqkv[:, wq:wq + wkv], dqkv[:, wq + wkv:]
    else:
        gq = torch.full((B * Sq, wq), 7.0, dtype=torch.bfloat16, device="cuda")
        dkv = torch.full((B * Sk, 2 * wkv), 7.0, dtype=torch.bfloat16, device="cuda")
        hip.attention_bwd(d, dod, gq, dkv, dkv, dk_off=0, dv_off=wkv)
        gk, gv = dkv[:, :wkv], dkv[:, wkv:]
    dq2 = torch.full((B * Sq, wq), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.attention_bwd(d, dod, dq2)
    torch.cuda.synchronize()
    out = {"O": o.cpu().view(B, Sq, Hq, D), "lse": lse.cpu(), "dQ": gq.cpu().reshape(B, Sq, Hq, D), "dK": gk.cpu().reshape(B, Sk, Hkv, D),
           "dV": gv.cpu().reshape(B, Sk, Hkv, D), "dQ_only": dq2.cpu().view(B, Sq, Hq, D)}
    if o32 is not None:
        out["O_f32"] = o32.cpu().view(B, Sq, Hq, D)
    return out


def _fwd8(case, setting="default"):
    """Which forward runs (desta_attention_fwd): the 8-wave kernel for seq_q >= 128 unless option 0 = 0; it picks the emulation."""
    return case[3] >= 128 and setting != "opt0=0"


def _limit(P, name, fwd8):
    return min(2.0, 2.0 * P.emu_ratio[fwd8][name])


def _check(P, got, label, fwd8):
    """The per-element assertion of the module docstring on one run; prints every figure before it asserts."""
    ref, emu = P.ref, P.emu_ratio[fwd8]
    ratios = {n: R.worst_ratio(ref, "dQ" if n == "dQ_only" else n, got[n].double()) for n in R.TENSORS + ("dQ_only",)}
    live = ref["live"]
    lse_err = float(((got["lse"].double() - ref["lse"])[live].abs() / (1 + ref["lse"][live].abs())).max())
    print(f"ATTN_FP64 {label} {P.case}" + (" O_f32" if P.o_f32 else "") + f" fwd{8 if fwd8 else 4}: "
          + " ".join(f"{n} {ratios[n]:.3f} ({emu['dQ' if n == 'dQ_only' else n]:.3f})" for n in ratios)
          + f" lse {lse_err:.1e}")
    for n, r in ratios.items():
        lim = _limit(P, "dQ" if n == "dQ_only" else n, fwd8)
        assert r <= lim, f"{label} {P.case} {n}: worst |err| / bound {r:.3f} > {lim:.3f} (emulation {emu['dQ' if n == 'dQ_only' else n]:.3f})"
    assert lse_err <= 1e-4, (label, P.case, lse_err)
    assert bool(torch.isinf(got["lse"][~live]).all()) and bool((got["lse"][~live] > 0).all())     # rows without a visible key: +inf (csrc/attention.hip:18)


ALL = ("O", "lse", "dQ", "dK", "dV", "dQ_only")
# What a setting leaves bit for bit, from the code: options 1 and 2 are attn_fwd8_k's own text under another register budget / wave
# schedule and option 5 is attn_bwd_dkdv_k's with two waves per block: every wave does the same arithmetic in the same order.
# Option 3 keeps the forward, and dV (attn_bwd_dkdv_k either way) takes P from lse and dO only, not delta.  Option 4 keeps the
# forward and the dQ-only backward, and attn_bwd_q64_k forms P and dS by attn_bwd_dkdv_k's expressions from the same attn_delta_k
# values and feeds the dV / dK MFMAs in its order (two 32-row query slices, two k-steps each).  The rest is another summation
# order (dQ under options 3 and 4; dK under option 3 through delta) or another kernel altogether (option 0 = 0).
BIT_IDENTICAL = {"opt0=0": (), "opt1=1": ALL, "opt2=1": ALL, "opt5=1": ALL, "opt3=1": ("O", "lse", "dV"), "opt3=1,serial": ("O", "lse", "dV"),
                 "opt4=0": ("O", "lse", "dK", "dV", "dQ_only")}


def _agree(P, base, got, setting):
    """Default against switched run.  Tensors whose arithmetic the setting leaves alone: bit for bit.  The others: to ONE bound,
    |default - switched| <= limit x bound, with the limit of the looser-held of the two runs (they differ only where option 0 = 0
    swaps the forward: each run is held to its own forward's emulation, the pair to the larger of the two ratios)."""
    live = P.ref["live"]
    for n in ALL:
        if n in BIT_IDENTICAL[setting]:
            assert torch.equal(base[n], got[n]), (setting, P.case, n, "not the default's bits")
            continue
        if n == "lse":
            assert float(((base[n].double() - got[n].double())[live].abs() / (1 + P.ref["lse"][live].abs())).max()) <= 1e-4
            continue
        t = "dQ" if n == "dQ_only" else n
        x, y = base[n].double(), got[n].double()
        big = torch.where(x.abs() >= y.abs(), x, y)
        r = float(((x - y).abs() / R.bounds(P.ref, t, big)).nan_to_num(nan=0.0, posinf=float("inf")).max())
        lim = max(_limit(P, t, _fwd8(P.case)), _limit(P, t, _fwd8(P.case, setting)))
        print(f"ATTN_FP64 {setting} {P.case} default vs switched {n}: {r:.3f} of one bound (limit {lim:.3f})")
        assert r <= lim, (setting, P.case, n, r, lim)
    print(f"ATTN_FP64 {setting} {P.case} default vs switched, bit for bit: {' '.join(BIT_IDENTICAL[setting]) or '-'}")


def _default_run(hip, P):
    if P.default is None:
        P.default = _run(hip, P)
    return P.default


@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_fwd_bwd_fp64(hip, case):
    P = _prepared(case)
    _check(P, _default_run(hip, P), "default", _fwd8(case))


@pytest.mark.parametrize("case", DROPOUT_CASES)
def test_attention_dropout_fp64(hip, case):
    """The DROP kernels under the same assertion, FACTOR and all: random operands, p = 0.1, the mask planted in the fp64 reference
    and the emulation is tests/dropout_reference.py's restatement, not desta_dropout_mask.  No dropout case reaches an 8-wave
    kernel (desta_attention_fwd / _bwd send dropout to the 4- and 2-wave kernels at any seq_q), so the emulation is the 4-wave
    one.  Paths: 64 x 1500 and 40 x 520 attn_fwd_k<64,true,2> + attn_bwd_q64_k<true,false>; 64 x 64 (fused q|k|v buffer)
    attn_fwd_k<64,true,2> + attn_bwd_dq_k<64,true,2> + attn_bwd_dkdv_k<64,true>; 160 x 200 attn_fwd_k<64,true> +
    attn_bwd_dq_k<64,true> (4 waves) + attn_bwd_dkdv_k<64,true>; the dQ-only backward takes attn_bwd_dq_k in every case."""
    P = _prepared(case, dropout=(DROPOUT_P, DROPOUT_SEED))
    _check(P, _run(hip, P), f"dropout p={DROPOUT_P}", False)


def _switch_cases(which):
    """The ATTN_CASES whose dispatch the setting changes (desta_attention_fwd / desta_attention_bwd; table in the module docstring)."""
    out = []
    for c in ATTN_CASES:
        B, Hq, Hkv, Sq, Sk, D, causal, pad = c
        G = Hq // Hkv
        hit = {
            "opt0=0": Sq >= 128,
            "opt1=1": Sq >= 128 and D == 64 and not causal,
            "opt2=1": Sq >= 128 and ((D == 128 and causal and G % 4 == 0) or (D == 64 and not causal)),
            "opt3=1": Sq >= 128,
            "opt4=0": D == 64 and Sq <= 64 and Sk >= 256 and not causal and Hq == Hkv,
            "opt5=1": Sq >= 128 and D == 128 and causal,
            "opt3=1,serial": Sq >= 128 and D == 128,
        }[which]
        if hit:
            out.append(c)
    return out


SETTINGS = {"opt0=0": (0, 0), "opt1=1": (1, 1), "opt2=1": (2, 1), "opt3=1": (3, 1), "opt4=0": (4, 0), "opt5=1": (5, 1), "opt3=1,serial": (3, 1)}
SWITCH_PARAMS = [(s, c) for s in SETTINGS for c in _switch_cases(s)]


def test_switch_case_lists():
    n = {s: len(_switch_cases(s)) for s in SETTINGS}
    assert n == {"opt0=0": 9, "opt1=1": 2, "opt2=1": 4, "opt3=1": 9, "opt4=0": 4, "opt5=1": 5, "opt3=1,serial": 6}, n


@pytest.mark.parametrize("setting,case", SWITCH_PARAMS, ids=[f"{s}-{i}" for i, (s, c) in enumerate(SWITCH_PARAMS)])
def test_attention_switches_fp64(hip, setting, case):
    P = _prepared(case)
    base = _default_run(hip, P)
    which, value = SETTINGS[setting]
    serial = setting.endswith("serial")
    try:
        hip.attention_set_option(which, value)
        if serial:
            concurrent = _run(hip, P)                      # option 3 = 1 with the dQ kernel on the side stream
            hip.attention_set_concurrent_bwd(False)
        got = _run(hip, P)
    finally:
        hip.attention_set_option(which, DEFAULTS[which])
        hip.attention_set_concurrent_bwd(True)
    _check(P, got, setting, _fwd8(case, setting))
    _agree(P, base, got, setting)
    if serial:
        for n in ("O", "dQ", "dK", "dV", "dQ_only", "lse"):
            assert torch.equal(concurrent[n], got[n]), (n, "desta_attention_set_concurrent_bwd: results are identical either way")


@pytest.mark.parametrize("case", [O_F32_CASE, O_F32_FLAT])
def test_attention_o_f32_feeds_delta_fp64(hip, case):
    """O_f32 set: delta comes from the unrounded output, so the bound has Ed = 0.  D = 128: the backward leaves the 8-wave dQ kernel
    for attn_delta_k + attn_bwd_dq_k<128> beside attn_bwd_dkdv_k<128> (the default dispatch concurrent_bwd(False) serialises)."""
    P = _prepared(case, o_f32=True)
    got = _run(hip, P)
    _check(P, got, "o_f32", _fwd8(case))
    assert torch.equal(got["O_f32"].to(torch.bfloat16), got["O"])
    r32 = R.worst_ratio({"O": P.ref["O"], "M_O": P.ref["M_O"]}, "O", got["O_f32"].double())
    print(f"ATTN_FP64 o_f32 {case}: O_f32 {r32:.3f}")
    assert r32 <= _limit(P, "O", _fwd8(case))
    if case[5] == 128:
        try:
            hip.attention_set_concurrent_bwd(False)
            serial = _run(hip, P)
        finally:
            hip.attention_set_concurrent_bwd(True)
        for n in ("O", "dQ", "dK", "dV", "dQ_only", "lse"):
            assert torch.equal(serial[n], got[n]), n


def test_attention_transposed_dkv_and_bias_fp64(hip):
    """dkv_transposed + dkv_bias_grad: the transposed dK | dV per element against fp64, the bias sums against the fp64 column sums.
    The sums are taken from the unrounded accumulators (attention.hip:1385), so their bound is the sum of the elements' bounds
    without the store term, plus n 2^-24 sum |x| for an fp32 sum of n = batch * seq_k terms; and the sum of the kernel's own
    stored elements, each its accumulator within half an ulp.  Sums of worst cases are loose for 3000 independent roundings, so
    both are calibrated like everything else here: within twice the emulation's ratio (its unrounded dK / dV sums against fp64,
    and against its own rounded elements)."""
    case = TRANSPOSED_CASE
    B, Hq, Hkv, Sq, Sk, D, causal, pad = case
    P = _prepared(case)
    qd, kvd, dod, kvs = P.device()
    o = torch.full((B * Sq, Hq * D), 7.0, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, Hq, Sq), 7.0, device="cuda")
    d = hip.attn_desc(qd, kvd, kvd, o, lse, batch=B, hq=Hq, hkv=Hkv, sq=Sq, sk=Sk, hd=D, scale=P.ops["scale"], k_off=0, v_off=Hkv * D)
    hip.attention_fwd(d)
    ld = (B * Sk + 63) // 64 * 64 + 64
    t = torch.full((2 * Hq * D, ld), 7.0, dtype=torch.bfloat16, device="cuda")
    bias = torch.full((2 * Hq * D,), -1.0, device="cuda")
    dq = torch.full((B * Sq, Hq * D), 7.0, dtype=torch.bfloat16, device="cuda")
    hip.attention_bwd(d, dod, dq, dkv_t=(t, ld, bias))
    torch.cuda.synchronize()
    assert float((t[:, B * Sk:].float() - 7.0).abs().max()) == 0.0                 # the pad columns are not touched
    tt = t[:, :B * Sk].cpu().view(2, Hq, D, B, Sk).permute(0, 3, 4, 1, 2)           # -> [K | V][B, Sk, H, D]
    got = {"dK": tt[0], "dV": tt[1], "dQ": dq.cpu().view(B, Sq, Hq, D)}
    for n in ("dQ", "dK", "dV"):
        r = R.worst_ratio(P.ref, n, got[n].double())
        print(f"ATTN_FP64 transposed {case} {n} {r:.3f} ({P.emu_ratio[False][n]:.3f})")
        assert r <= _limit(P, n, False), (n, r)
    base = _default_run(hip, P)
    assert torch.equal(got["dK"], base["dK"]) and torch.equal(got["dV"], base["dV"]) and torch.equal(got["dQ"], base["dQ"])
    bsum = bias.cpu().double().view(2, Hq, D)
    sum_eps = B * Sk * 2.0 ** -24                                                   # an fp32 sum of n = batch * seq_k terms: n 2^-24 sum |x|
    emu = P.emu[False]
    for i, n in enumerate(("dK", "dV")):
        ref = P.ref[n].sum((0, 1))
        bound = (P.ref["M_" + n] * (1.0 if n == "dK" else 2.0 ** -8)).sum((0, 1)) + sum_eps * P.ref[n].abs().sum((0, 1))
        r, r_emu = (float(((x - ref).abs() / bound).max()) for x in (bsum[i], emu[n + "_unrounded"].sum((0, 1))))
        # and against the sum of the kernel's own stored elements, each within half an ulp of the accumulator that was summed
        own, own_emu = got[n].double(), emu[n]
        r_own, r_own_emu = (float(((b_ - o_.sum((0, 1))).abs() / ((0.5 * R.bf16_ulp(o_.abs())).sum((0, 1)) + sum_eps * o_.abs().sum((0, 1)))).max())
                            for b_, o_ in ((bsum[i], own), (emu[n + "_unrounded"].sum((0, 1)), own_emu)))
        print(f"ATTN_FP64 transposed {case} bias {n}: vs fp64 {r:.4f} of the summed bound (emulation {r_emu:.4f}); "
              f"vs the stored elements {r_own:.4f} of the half-ulp sum (emulation {r_own_emu:.4f})")
        assert r <= min(1.0, 2.0 * r_emu) and r_own <= min(1.0, 2.0 * r_own_emu), (n, r, r_emu, r_own, r_own_emu)
