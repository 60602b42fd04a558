"""GPU: the dropout mask read back out of every kernel that draws one, against the independent restatement of
tests/dropout_reference.py (proved on the CPU by tests/test_dropout_mask_host.py; constructions and tolerances in that module's
docstring).  Nothing here takes a mask from desta_dropout_mask except the test of that kernel itself.

  1. dropout_mask_k            == keep(seed, n, p) bit for bit; thresholds 1 and 0xffff; an element with bits == thresh; the known
                               answers of the host test pinned to their 16 bits by two thresholds each (kept at thresh = bits,
                               dropped at bits + 1).  Known answers at idx >= 2^33 would need an 8 GiB mask and stay with the host
                               test (the hash's high index word is what the sampler kernels use, test_gpu_sampling_draw.py).
  2. dropout_bf16_k            y == bf16(x * fp32(1 / (1 - p))) where kept, +0 where dropped, pad columns and guard untouched
  3. GEMM epilogue             A = identity, B small integers: out == keep * B^T * c (+ residual) exactly, fp32 and bf16 outputs,
                               128 x 128, 256 x 256 (lockstep, staggered, two-phase, persistent) and skinny kernels, batch, the
                               transposed-B / residual == out form of the LoRA backward, and one shape the automatic choice sends
                               to the 256 x 256 kernel
  4. attention forward         readout `fwd`: 2-wave and 4-wave kernels, one GQA case (the backward readouts have two)
  5. attention backward        readouts `dV`, `dQ`, `dK` on every path that draws a mask (`_kernels` restates the dispatch of
                               desta_attention_fwd / desta_attention_bwd; test_every_drop_kernel_is_read asserts the case tables
                               reach all seven DROP instantiations)
  6. determinism               two runs, same bits
Each decoded mask must equal attn_keep everywhere, so forward and backward agree pair for pair; a mismatch names the kernels, the
first (b, h, q, k) and where that pair sits in the tiles.  Measured (MI355X; profiles/r24_dropout_mask_tests.log): every mask
exact on every path, no kernel had to change; worst value error, in units of the tolerance, fwd 0.200 and dV 0.362 (of 2^-7
relative), dQ and dK 0.476 (of gap / 64); where it was tried on the host the bf16-rounding emulation of
tests/attention_reference.py gives the same figures for the same operands; bias sums within 0.38 of the half-ulp sum; the whole
file takes 5 s."""
import numpy as np
import pytest
import torch

import dropout_reference as R
from test_dropout_mask_host import KNOWN

pytestmark = pytest.mark.gpu

P, SEED, SCALE = 0.1, (3 << 40) | 77, 0.125
B, H = 2, 3
DEV = "cuda"
PAD = 8                                                                    # sentinel columns behind every output row


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


# ------------------------------------------------------------------------------------------------------ 1. dropout_mask_k
def test_dropout_mask_kernel_is_the_restatement(hip):
    big = (1 << 20) + 3
    cache = {}

    def bits_of(seed):
        if seed not in cache:
            cache[seed] = R.bits16(seed, np.arange(big, dtype=np.uint64))
        return cache[seed]

    for p in (1e-6, 0.1, 0.5, 0.99999):
        t = R.drop_thresh(p)
        edge_seed = next(s for s in range(1000, 2000) if bool((bits_of(s) == np.uint64(t)).any()))
        at = int(np.flatnonzero(bits_of(edge_seed) == np.uint64(t))[0])
        for seed in (0, 12345, (7 << 40) | 12345, (1 << 64) - 1, edge_seed):
            bits = bits_of(seed)
            ref = torch.from_numpy(bits >= np.uint64(t))
            for n in (1, 2, 255, 257, big) if seed != edge_seed else (big,):
                got = hip.dropout_mask(seed, n, p).cpu().bool()
                assert torch.equal(got, ref[:n]), (p, hex(seed), n, int((got != ref[:n]).nonzero()[0]))
        assert int(bits[at]) == t and bool(ref[at])                        # bits == thresh: kept (>=)
        print(f"DROPOUT_MASK p = {p}: thresh {t:#x}, kept {float(ref.float().mean()):.5f}; seed {edge_seed} element {at} sits on the threshold, kept")
    assert R.drop_thresh(1e-6) == 1 and R.drop_thresh(0.99999) == 0xFFFF


def test_known_answers_on_the_device(hip):
    seen = 0
    for seed, idx, bits in KNOWN:
        if idx >= 1 << 21:
            continue
        seen += 1
        if bits >= 1:
            assert int(hip.dropout_mask(seed, idx + 1, bits / 65536.0)[idx]) == 1, (hex(seed), idx, hex(bits))
        if bits + 1 <= 0xFFFF:
            assert int(hip.dropout_mask(seed, idx + 1, (bits + 1) / 65536.0)[idx]) == 0, (hex(seed), idx, hex(bits))
    assert seen >= 8


# ------------------------------------------------------------------------------------------------------ 2. dropout_bf16_k
@pytest.mark.parametrize("rows,cols,ld", [(1, 4, 4), (5, 260, 264), (320, 256, 256)])
def test_dropout_bf16_exact(hip, rows, cols, ld):
    g = torch.Generator().manual_seed(rows + cols)
    for p, seed in ((0.1, SEED), (0.5, 12345)):
        x = torch.randn(rows * ld + 64, generator=g).bfloat16()
        y = torch.full((rows * ld + 64,), 7.0, dtype=torch.bfloat16, device=DEV)
        hip.dropout_bf16(x.cuda(), y, rows, cols, ld, p, seed)
        y = y.cpu()
        keep = torch.from_numpy(R.keep(seed, rows * cols, p)).view(rows, cols)
        xv, yv = x[:rows * ld].view(rows, ld), y[:rows * ld].view(rows, ld)
        want = torch.where(keep, (xv[:, :cols].float() * torch.tensor(R.drop_scale(p), dtype=torch.float32)).bfloat16(), torch.zeros(1, dtype=torch.bfloat16))
        assert torch.equal(yv[:, :cols].view(torch.int16), want.view(torch.int16))          # bits: a dropped element is +0
        assert bool((yv[:, cols:] == 7.0).all()) and bool((y[rows * ld:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------- 3. GEMM epilogue
GEMM_CASES = [
    # M, N, K, ldc, batch, trans_b, variants (gemm_force_variant; 0 = automatic)
    (192, 260, 192, 264, 1, False, (0, 1)),                                # 128 x 128 tiles, M and N off the tile
    (320, 260, 320, 264, 1, False, (0, 1, 2, 3, 4, 6)),                    # 256 x 256: lockstep, staggered, persistent, two-phase
    (192, 260, 192, 264, 2, False, (0, 1, 2)),                             # element index (z M + m) N + n
    (8, 68, 64, 72, 1, False, (0,)),                                       # M <= 16: the weight-streaming kernel (A = the first 8 rows of I)
    (192, 264, 192, 272, 1, True, (0,)),                                   # B stored [K, N], residual == out: the LoRA backward's call
]


@pytest.mark.parametrize("case", GEMM_CASES, ids=[f"{c[0]}x{c[1]}b{c[4]}{'t' if c[5] else ''}" for c in GEMM_CASES])
def test_gemm_epilogue_mask_by_identity(hip, case):
    M, N, K, ldc, batch, trans_b, variants = case
    g = torch.Generator().manual_seed(M + N)
    A = torch.eye(M, K).bfloat16().cuda()
    Bt = torch.randint(-8, 9, (batch, M, N), generator=g).float()           # the product: out[z, m, n] = B[z, n, m]
    Bfull = torch.zeros(batch, N, K)
    Bfull[:, :, :M] = Bt.transpose(1, 2)
    Bdev = (Bfull.transpose(1, 2) if trans_b else Bfull).contiguous().bfloat16().cuda()
    res = torch.randint(-4, 5, (batch, M, ldc), generator=g).float()
    keep = torch.from_numpy(R.gemm_keep(SEED, batch, M, N, P))
    c = torch.tensor(R.drop_scale(P), dtype=torch.float32)
    for variant in variants:
        for dtype in (torch.float32, torch.bfloat16):
            for with_res in (False, True):
                out = torch.full((batch * M + 1, ldc), 7.0, dtype=dtype, device=DEV)
                r = None
                if with_res and trans_b:
                    out[:batch * M] = res.view(batch * M, ldc).to(dtype)
                    r = out
                elif with_res:
                    r = res.view(batch * M, ldc).to(dtype).cuda()
                try:
                    hip.gemm_force_variant(variant)
                    hip.gemm(A, Bdev, out, M, N, K, ldc=ldc, residual=r, ldr=ldc, batch=batch, stride_b=N * K, stride_c=M * ldc,
                             stride_r=M * ldc, trans_b=trans_b, dropout_p=P, dropout_seed=SEED)
                    kernel = hip.lib.desta_gemm_last_kernel()
                finally:
                    hip.gemm_force_variant(0)
                want = torch.where(keep, Bt * c, torch.zeros(()))
                if with_res:
                    want = want + res[:, :, :N].to(dtype).float()
                got = out[:batch * M].cpu().view(batch, M, ldc)
                tag = (variant, str(dtype), with_res, kernel)
                assert torch.equal(got[:, :, :N], want.to(dtype)), (tag, (got[:, :, :N] != want.to(dtype)).nonzero()[0].tolist())
                if not (with_res and trans_b):
                    assert bool((got[:, :, N:] == 7.0).all()), tag
                assert bool((out[batch * M:] == 7.0).all()), tag
                assert kernel == (3 if M <= 16 else (2 if variant >= 2 else 1)), tag


def test_gemm_epilogue_mask_automatic_256(hip):
    """A shape the automatic choice sends to the 256 x 256 kernel (200 tiles of one round): reference on the device."""
    M = K = 2048
    N = 6400
    g = torch.Generator().manual_seed(5)
    A = torch.eye(M, K).bfloat16().cuda()
    Bm = torch.randint(-8, 9, (N, K), generator=g).bfloat16().cuda()
    out = torch.empty(M, N, dtype=torch.float32, device=DEV)
    hip.gemm(A, Bm, out, M, N, K, dropout_p=P, dropout_seed=SEED)
    assert hip.lib.desta_gemm_last_kernel() == 2
    keep = torch.from_numpy(R.gemm_keep(SEED, 1, M, N, P)[0]).cuda()
    want = torch.where(keep, Bm.float().t() * torch.tensor(R.drop_scale(P), dtype=torch.float32, device=DEV), torch.zeros((), device=DEV))
    assert torch.equal(out, want), (out != want).nonzero()[0].tolist()


# ------------------------------------------------------------------------------------------------- 4. / 5. attention readouts
def _kernels(Sq, Sk, Hq, Hkv, opt4=1, transposed=False):
    """The DROP kernels desta_attention_fwd / desta_attention_bwd launch for a head-dim-64 dropout call with dK / dV wanted and
    this file's aligned buffers (attention.hip: forward `two`; backward `q64`, option 4, `two_q`)."""
    nw = 2 if Sq <= 64 else 4
    fwd = f"attn_fwd_k<64,true,{nw}>"
    if (opt4 or transposed) and Sq <= 64 and Sk >= 256 and Hq == Hkv:
        return fwd, (f"attn_bwd_q64_k<true,{'true' if transposed else 'false'}>",)
    assert not transposed
    return fwd, (f"attn_bwd_dq_k<64,true,{nw}>", "attn_bwd_dkdv_k<64,true>")


class Runner:
    """run(q, k, v, do) on the kernels: operands [B, S, H, 64] bf16 on the device -> {"O", "dQ", "dK", "dV"} views of buffers that
    start as 7.0 with PAD sentinel columns per row and two guard rows, all checked after every call."""

    def __init__(self, hip, seed, backward=True, transposed=False):
        self.hip, self.seed, self.backward, self.transposed, self.bias = hip, seed, backward, transposed, []

    def _buf(self, rows, width):
        return torch.full((rows + 2, width + PAD), 7.0, dtype=torch.bfloat16, device=DEV)

    @staticmethod
    def _untouched(buf, rows, width):
        return bool((buf[:, width:] == 7.0).all()) and bool((buf[rows:] == 7.0).all())

    def __call__(self, q, k, v, do):
        hip = self.hip
        Bn, Sq, Hq, _ = q.shape
        Sk, Hkv = k.shape[1], k.shape[2]
        wq, wk = Hq * 64, Hkv * 64
        o = self._buf(Bn * Sq, wq)
        lse = torch.full((Bn, Hq, Sq), 7.0, device=DEV)
        d = hip.attn_desc(q.view(Bn * Sq, wq), k.view(Bn * Sk, wk), v.view(Bn * Sk, wk), o, lse, batch=Bn, hq=Hq, hkv=Hkv, sq=Sq, sk=Sk,
                          hd=64, scale=SCALE, dropout_p=P, dropout_seed=self.seed)
        hip.attention_fwd(d)
        assert self._untouched(o, Bn * Sq, wq), "attention_fwd wrote outside O"
        out = {"O": o[:Bn * Sq, :wq].view(Bn, Sq, Hq, 64)}
        if not self.backward:
            return out
        dq = self._buf(Bn * Sq, wq)
        if self.transposed:
            ld = (Bn * Sk + 63) // 64 * 64 + 64
            t = torch.full((2 * wq, ld), 7.0, dtype=torch.bfloat16, device=DEV)
            bias = torch.full((2 * wq,), -1.0, device=DEV)
            hip.attention_bwd(d, do.view(Bn * Sq, wq), dq, dkv_t=(t, ld, bias))
            assert bool((t[:, Bn * Sk:] == 7.0).all()), "attention_bwd wrote the pad columns of the transposed dK | dV"
            tt = t[:, :Bn * Sk].view(2, Hq, 64, Bn, Sk).permute(0, 3, 4, 1, 2)        # -> [K | V][B, Sk, H, 64]
            out["dK"], out["dV"] = tt[0], tt[1]
            self.bias.append((bias.view(2, Hq, 64), tt))
        else:
            dk, dv = self._buf(Bn * Sk, wk), self._buf(Bn * Sk, wk)
            hip.attention_bwd(d, do.view(Bn * Sq, wq), dq, dk, dv)
            assert self._untouched(dk, Bn * Sk, wk) and self._untouched(dv, Bn * Sk, wk), "attention_bwd wrote outside dK / dV"
            out["dK"], out["dV"] = (x[:Bn * Sk, :wk].view(Bn, Sk, Hkv, 64) for x in (dk, dv))
        assert self._untouched(dq, Bn * Sq, wq), "attention_bwd wrote outside dQ"
        out["dQ"] = dq[:Bn * Sq, :wq].view(Bn, Sq, Hq, 64)
        return out


def _read(hip, kinds, Sq, Sk, Hq=H, Hkv=H, seed=SEED, opt4=1, transposed=False):
    ref = torch.from_numpy(R.attn_keep(seed, B, Hq, Sq, Sk, P))
    fwd, bwd = _kernels(Sq, Sk, Hq, Hkv, opt4, transposed)
    runner, worst = Runner(hip, seed, backward=kinds != ("fwd",), transposed=transposed), {}
    for kind in kinds:
        mask, worst[kind] = R.read_mask(kind, runner, ref, Hkv, P, SCALE, device=DEV, dtype=torch.bfloat16)
        names = fwd if kind == "fwd" else " + ".join(bwd)
        assert torch.equal(mask, ref), f"{names}, readout {kind} at B {B} Hq {Hq} Hkv {Hkv} Sq {Sq} Sk {Sk}: {R.first_mismatch(mask, ref)}"
    print(f"DROPOUT_READOUT {Sq} x {Sk} Hq {Hq} Hkv {Hkv} [{fwd if kinds == ('fwd',) else ' + '.join(bwd)}]: mask exact on {' '.join(kinds)}; "
          "worst value error / tolerance " + " ".join(f"{k} {w:.3f}" for k, w in worst.items()))
    for kind, w in worst.items():
        assert w <= 1.0, (kind, Sq, Sk, w)
    return runner


FWD_SHAPES = [(1, 2), (40, 62), (64, 64), (40, 520), (64, 1500), (65, 66), (128, 200), (160, 1500)]
Q64_SHAPES = [(Sq, Sk) for Sq in (40, 64) for Sk in (256, 384, 386, 520, 896, 898, 1500)]      # chunk counts 1 | 2 | 4: nkb >= 4, nkb >= 8
Q64_T_SHAPES = [(64, 256), (40, 520), (64, 1500)]
TWO_KERNEL_SHAPES = [(64, 64), (40, 200), (64, 2)]
FOUR_WAVE_SHAPES = [(65, 66), (160, 200), (130, 1500)]
BWD = ("dV", "dQ", "dK")


@pytest.mark.parametrize("Sq,Sk", FWD_SHAPES)
def test_forward_readout(hip, Sq, Sk):
    _read(hip, ("fwd",), Sq, Sk)


def test_forward_readout_gqa(hip):
    """Dropout with a GQA group is accepted (fill_args has no such check): the mask's head is the QUERY head."""
    _read(hip, ("fwd",), 40, 200, Hq=4, Hkv=2)


@pytest.mark.parametrize("Sq,Sk", Q64_SHAPES)
def test_backward_readout_one_pass(hip, Sq, Sk):
    _read(hip, BWD, Sq, Sk)


@pytest.mark.parametrize("Sq,Sk", Q64_T_SHAPES)
def test_backward_readout_one_pass_transposed_with_bias_sums(hip, Sq, Sk):
    runner = _read(hip, BWD, Sq, Sk, transposed=True)
    # the bias sums are the column sums of the gradients that were just decoded: taken from the unrounded accumulators, so within
    # the stored elements' half ulps plus an fp32 sum of n = batch * seq_k terms (test_attention_transposed_dkv_and_bias_fp64)
    import attention_reference as AR
    worst = 0.0
    for bias, tt in runner.bias:
        x = tt.double()
        lim = (0.5 * AR.bf16_ulp(x.abs())).sum((1, 2)) + B * Sk * 2.0 ** -24 * x.abs().sum((1, 2))
        err = (bias.double() - x.sum((1, 2))).abs()
        assert bool((err <= lim).all()), float((err / lim.clamp_min(1e-300)).max())
        worst = max(worst, float((err / lim.clamp_min(1e-300)).max()))
    print(f"DROPOUT_READOUT {Sq} x {Sk} transposed: bias sums within {worst:.3f} of the half-ulp sum of the decoded elements ({len(runner.bias)} passes)")


@pytest.mark.parametrize("Sq,Sk", TWO_KERNEL_SHAPES + FOUR_WAVE_SHAPES)
def test_backward_readout_two_kernels(hip, Sq, Sk):
    _read(hip, BWD, Sq, Sk)


@pytest.mark.parametrize("Sq,Sk", [(40, 200), (130, 200)])
def test_backward_readout_gqa(hip, Sq, Sk):
    """4 query heads on 2 kv heads (two-kernel path; the one-pass kernel wants Hq == Hkv): dV / dK read one head of each group per
    pass (dropout_reference.py), so the head index hk * group + it / nq of attn_bwd_dkdv_k is held too."""
    _read(hip, BWD, Sq, Sk, Hq=4, Hkv=2)


def test_backward_readout_two_kernels_at_the_cross_attention_shape(hip):
    """64 x 1500 with the one-pass backward switched off (attention option 4 = 0)."""
    try:
        hip.attention_set_option(4, 0)
        _read(hip, BWD, 64, 1500, opt4=0)
    finally:
        hip.attention_set_option(4, 1)


def test_backward_readout_other_seeds(hip):
    """Seed 0, a seed with only a high word and the all-ones seed through both backward paths at one shape each."""
    for seed in (0, 5 << 32, (1 << 64) - 1):
        _read(hip, BWD, 40, 520, seed=seed)
        _read(hip, ("fwd",) + BWD, 65, 66, seed=seed)


def test_every_drop_kernel_is_read():
    seen = set()
    for shapes, kw in ((FWD_SHAPES, {}), (Q64_SHAPES, {}), (Q64_T_SHAPES, {"transposed": True}), (TWO_KERNEL_SHAPES + FOUR_WAVE_SHAPES, {}),
                       ([(64, 1500)], {"opt4": 0})):
        for Sq, Sk in shapes:
            fwd, bwd = _kernels(Sq, Sk, H, H, **kw)
            seen.add(fwd)
            if shapes is not FWD_SHAPES:
                seen.update(bwd)
    assert seen == {"attn_fwd_k<64,true,2>", "attn_fwd_k<64,true,4>", "attn_bwd_dq_k<64,true,2>", "attn_bwd_dq_k<64,true,4>",
                    "attn_bwd_dkdv_k<64,true>", "attn_bwd_q64_k<true,false>", "attn_bwd_q64_k<true,true>"}, seen
    assert all(_kernels(Sq, Sk, H, H)[1] == ("attn_bwd_q64_k<true,false>",) for Sq, Sk in Q64_SHAPES)
    assert all(len(_kernels(Sq, Sk, H, H)[1]) == 2 for Sq, Sk in TWO_KERNEL_SHAPES + FOUR_WAVE_SHAPES)


# ----------------------------------------------------------------------------------------------------------- 6. determinism
@pytest.mark.parametrize("Sq,Sk", [(64, 1500), (160, 200)])
def test_dropout_forward_backward_is_deterministic(hip, Sq, Sk):
    g = torch.Generator().manual_seed(Sq + Sk)
    q, do = (torch.randn(B, Sq, H, 64, generator=g).bfloat16().cuda() for _ in range(2))
    k, v = (torch.randn(B, Sk, H, 64, generator=g).bfloat16().cuda() for _ in range(2))
    runs = [{n: x.clone() for n, x in Runner(hip, SEED)(q, k, v, do).items()} for _ in range(2)]
    for n in ("O", "dQ", "dK", "dV"):
        assert torch.equal(runs[0][n].view(torch.int16), runs[1][n].view(torch.int16)), n
    other = Runner(hip, SEED + 1)(q, k, v, do)
    assert not torch.equal(other["O"], runs[0]["O"])                        # and the seed matters
