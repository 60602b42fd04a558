"""sha256 digests of what the decode GEMMs write, for the library named by DESTA_HIP_LIB (default: the in-tree build).
The 16-row, the wide and the MXFP4 kernel share their RMS prologue, item walk, reduce / finish and SwiGLU epilogue, and the tests
hold one form to another's bits (FP8 to bf16 on the dequantised weight, act 4 to the plain GEMM + swiglu kernel), so they cannot
see a change made to all of them: run this under the library of the commit before a change and under the new one, every line
must be equal.  One line per case and persistent grid (option 3 = 7 and 512) over the raw bytes of the sentinel-filled output,
guard row and guard columns included, and, for the 64-row kernels, of the head of the GEMM workspace: 8 * M * weight-rows floats,
NaN-filled before the call, which holds the K-slice slab [ks][M][weight rows] of a cut case and must stay NaN behind it.
The cases are those of the test modules: PLAIN / SWIGLU / RMS of tests/test_gpu_fp8_decode.py through `gemm` and `gemm_w8`,
PLAIN / SWIGLU of tests/test_gpu_wide_decode.py through `gemm_wide` on bf16 and e4m3 weights, CASES of
tests/test_gpu_mxfp4_decode.py through `gemm_w4`.
  python tools/decode_gemm_bits.py"""
import hashlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("desta2.5-audio_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
from desta import _hip as H
import test_gpu_fp8_decode as T8
import test_gpu_wide_decode as TW
import test_gpu_mxfp4_decode as T4

X = T4.X
GRIDS = (7, 512)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def filled(M, N, dtype=torch.bfloat16):
    """[M + 1, N + 12]: a guard row and twelve guard columns around the output"""
    return torch.full((M + 1, N + 12), 7.0, dtype=dtype, device="cuda")


def slab_head(M, ntot):
    """the first 8 * M * ntot floats of the stream's GEMM workspace (8 = the most K-slices a plan has), NaN-filled"""
    ws = H._workspace(torch.device("cuda", torch.cuda.current_device()), H.stream())[:8 * M * ntot]
    ws.fill_(float("nan"))
    return ws


def report(tag, fn):
    """fn() -> tensors to hash, at every grid"""
    try:
        for blocks in GRIDS:
            H.gemm_set_option(3, blocks)
            out = fn()
            torch.cuda.synchronize()
            print(f"{tag} grid {blocks:3d}  {sha(*out)}", flush=True)
    finally:
        H.gemm_set_option(3, 512)


def sixteen_rows():
    """tests/test_gpu_fp8_decode.py: `gemm` on the dequantised weight and `gemm_w8` on the bytes"""
    for M, N, K in T8.PLAIN:
        A, B8, s, Bd, g = T8._operands(M, N, K, N, M * 11 + N + K)
        res = T8._bf(torch.randn(M, N, generator=g)).cuda()
        kw = dict(lda=3 * K, ldc=N + 12)
        report(f"gemm    plain  M {M:2d} N {N:5d} K {K:5d}", lambda: (H.gemm(A, Bd, filled(M, N), M, N, K, residual=res, alpha=0.5, **kw),
                                                                      H.gemm(A, Bd, filled(M, N, torch.float32), M, N, K, **kw)))
        report(f"gemm_w8 plain  M {M:2d} N {N:5d} K {K:5d}", lambda: (H.gemm_w8(A, B8, s, filled(M, N), M, N, K, residual=res, alpha=0.5, **kw),
                                                                      H.gemm_w8(A, B8, s, filled(M, N, torch.float32), M, N, K, **kw)))
    for M, I, K in T8.SWIGLU:
        A, B8, s, Bd, g = T8._operands(M, I, K, 2 * I, M + I, gain_from=I)
        kw = dict(lda=3 * K, ldc=I + 12, act=4)
        report(f"gemm    swiglu M {M:2d} N {I:5d} K {K:5d}", lambda: (H.gemm(A, Bd, filled(M, I), M, I, K, **kw),))
        report(f"gemm_w8 swiglu M {M:2d} N {I:5d} K {K:5d}", lambda: (H.gemm_w8(A, B8, s, filled(M, I), M, I, K, **kw),))
    for M, N, K in T8.RMS:
        assert H.rms_fusable(M, K)
        g = torch.Generator().manual_seed(M * 5 + N)
        x = T8._bf(torch.randn(M, K, generator=g) * 3).cuda()
        gamma = (1.0 + 0.1 * torch.randn(K, generator=g)).cuda()
        q, s = T8.quantize_ref(T8._bf(torch.randn(2 * N, K, generator=g) / math.sqrt(K) * 2))
        Bd, B8, s = T8.dequant_bf16(q, s).cuda(), q.view(torch.uint8).cuda(), s.cuda()
        res = T8._bf(torch.randn(M, N, generator=g)).cuda()
        kw = dict(ldc=N + 12, a_rms_weight=gamma, a_rms_eps=1e-5)
        report(f"gemm    rms    M {M:2d} N {N:5d} K {K:5d}", lambda: (H.gemm(x, Bd, filled(M, N), M, N, K, residual=res, **kw),
                                                                      H.gemm(x, Bd, filled(M, N, torch.float32), M, N, K, **kw),
                                                                      H.gemm(x, Bd, filled(M, N), M, N, K, act=4, **kw)))
        report(f"gemm_w8 rms    M {M:2d} N {N:5d} K {K:5d}", lambda: (H.gemm_w8(x, B8, s, filled(M, N), M, N, K, residual=res, **kw),
                                                                      H.gemm_w8(x, B8, s, filled(M, N, torch.float32), M, N, K, **kw),
                                                                      H.gemm_w8(x, B8, s, filled(M, N), M, N, K, act=4, **kw)))


def wide():
    """tests/test_gpu_wide_decode.py: `gemm_wide` on bf16 weights and on their e4m3 quantisation"""
    for act, cases in ((0, TW.PLAIN), (4, TW.SWIGLU)):
        for M, N, K in cases:
            rows = 2 * N if act == 4 else N
            A, W, g = TW._ab(M, rows, K, M * 7 + N + K)
            if act == 4:
                W[N:] *= 4.0                                                 # gate rows and up rows on different scales
            q, s, _ = TW._quantize(H, W)
            kw = dict(fill_rows=1, ldc=N + 12, act=act)
            if act == 0:
                kw.update(residual=TW._bf(torch.randn(M, N, generator=g)).cuda(), alpha=0.5)

            def run(B, **scale):
                ws = slab_head(M, rows)
                return TW._wide(H, A, B, M, N, K, **scale, **kw), ws
            form = "swiglu" if act == 4 else "plain "
            report(f"gemm_wide bf16 {form} M {M:2d} N {N:5d} K {K:5d}", lambda: run(W))
            report(f"gemm_wide e4m3 {form} M {M:2d} N {N:5d} K {K:5d}", lambda: run(q, scale=s))


def mxfp4():
    """tests/test_gpu_mxfp4_decode.py: `gemm_w4` on every case, into the test's own sentinel-filled buffer"""
    for case in T4.CASES:
        o = X.operands(case, device="cuda")

        def run():
            ws = slab_head(o["M"], (2 if case["act"] == 4 else 1) * o["N"])
            return T4._run(H, o), ws
        report(f"gemm_w4 {X.case_id(case)} ks {o['plan']['ks']}", run)


if __name__ == "__main__":
    sixteen_rows()
    wide()
    mxfp4()
