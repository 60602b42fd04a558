"""Per-launch time of the decode projections on bf16 weights, their weight-only FP8 (e4m3) copies and their MXFP4 copies, per
projection shape of Llama-3.1-8B with the epilogue the decode step uses (fused RMSNorm / residual / SwiGLU), at M = 1, 8, 32.
Each timed launch reads a DIFFERENT weight buffer (rotating set > 1 GiB of the form that runs) so neither L2 nor the 256 MB MALL
can serve the weights.  TB/s counts the bytes of the form that ran (MXFP4: nibbles + scale bytes); x = bf16 time / that form's time.
M <= 16: `gemm` / `gemm_w8` / `gemm_w4`; M = 32: `gemm_wide` (bf16, fp8) / `gemm_w4`, with the separate RMSNorm launch the wide
batch pays left out of all three.
  python tools/skinny_mxfp4_bench.py [--rows 1,8,32]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch  # noqa: E402
from desta import _hip as H  # noqa: E402

SHAPES = [("qkv", 6144, 4096, "rms"), ("o", 4096, 4096, "res"), ("gate_up", 14336, 4096, "swiglu_rms"), ("down", 4096, 14336, "res"),
          ("lm_head", 128256, 4096, "rms")]


def timeit(fn, nbuf):
    for i in range(nbuf):
        fn(i)
    reps = max(2 * nbuf, 20)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i % nbuf)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1,8,32")
    a = ap.parse_args()
    for M in [int(x) for x in a.rows.split(",")]:
        for name, N, K, kind in SHAPES:
            rows = 2 * N if kind.startswith("swiglu") else N
            nbuf = max(2, int(1.2 * 2 ** 30 / (rows * K * 2)) + 1)          # the bf16 set is > 1 GiB; the copies rotate over 2x / 4x as many
            x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            res = torch.randn(M, N, device="cuda").to(torch.bfloat16)
            gamma = torch.ones(K, device="cuda")
            out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
            kw = {}
            if "rms" in kind and H.rms_fusable(M, K):
                kw.update(a_rms_weight=gamma, a_rms_eps=1e-5)
            if kind == "res":
                kw.update(residual=res)
            if kind.startswith("swiglu"):
                kw.update(act=4)
            line = [f"M={M:2d} {name:8s} N={N:6d} K={K:5d} {kind:10s}"]
            Ws = [(torch.randn(rows, K, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(nbuf)]
            if M <= 16:
                us = timeit(lambda i: H.gemm(x, Ws[i], out, M, N, K, **kw), nbuf)
            else:
                us = timeit(lambda i: H.gemm_wide(x, Ws[i], out, M, N, K, **kw), nbuf)
            line.append(f"bf16 {us:7.1f}us {rows * K * 2 / us / 1e6:5.2f}TB/s")
            Q8 = [H.quantize_rows_e4m3(Ws[i % nbuf]) for i in range(2 * nbuf)]
            if M <= 16:
                us8 = timeit(lambda i: H.gemm_w8(x, Q8[i][0], Q8[i][1], out, M, N, K, **kw), 2 * nbuf)
            else:
                us8 = timeit(lambda i: H.gemm_wide(x, Q8[i][0], out, M, N, K, scale=Q8[i][1], **kw), 2 * nbuf)
            line.append(f"fp8 {us8:7.1f}us {rows * K / us8 / 1e6:5.2f}TB/s x{us / us8:4.2f}")
            del Q8
            Q4 = [H.quantize_rows_mxfp4(Ws[i % nbuf]) for i in range(4 * nbuf)]
            del Ws
            us4 = timeit(lambda i: H.gemm_w4(x, Q4[i][0], Q4[i][1], out, M, N, K, **kw), 4 * nbuf)
            line.append(f"mxfp4 {us4:7.1f}us {rows * K * 17 / 32 / us4 / 1e6:5.2f}TB/s x{us / us4:4.2f} (vs fp8 x{us8 / us4:4.2f})")
            print("  ".join(line), flush=True)
            del Q4


if __name__ == "__main__":
    main()
