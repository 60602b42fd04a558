"""Skinny (M <= 16) GEMM of the decode step, bf16 weights against their weight-only FP8 (e4m3) copies, per projection shape of
Llama-3.1-8B with the epilogue the decode step uses (fused RMSNorm / residual / SwiGLU).  Each timed launch reads a DIFFERENT
weight buffer (rotating set > 1 GiB) so neither L2 nor the 256 MB MALL can serve the weights.  TB/s counts the bytes of the
form that ran; x = bf16 time / FP8 time.  v162 / v164 = pipeline depth U of the FP8 form (gemm_set_option(11, .)).
  python tools/skinny_fp8_bench.py"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch
from desta import _hip as H

def timeit(fn, nbuf):
    for i in range(nbuf): fn(i)
    reps = max(2 * nbuf, 20)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps): fn(i % nbuf)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps

for M in (8, 1):
    for N, K, kind in [(6144, 4096, "rms"), (4096, 4096, "res"), (14336, 4096, "swiglu_rms"), (4096, 14336, "res"), (128256, 4096, "rms")]:
        rows = 2 * N if kind.startswith("swiglu") else N
        nbuf = max(2, int(1.2 * 2**30 / (rows * K * 2)) + 1)
        Ws = [(torch.randn(rows, K, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(nbuf)]
        Q = [H.quantize_rows_e4m3(w) for w in Ws]
        x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
        res = torch.randn(M, N, device="cuda").to(torch.bfloat16)
        gamma = torch.ones(K, device="cuda")
        out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        kw = {}
        if "rms" in kind and H.rms_fusable(M, K): kw.update(a_rms_weight=gamma, a_rms_eps=1e-5)
        if kind == "res": kw.update(residual=res)
        if kind.startswith("swiglu"): kw.update(act=4)
        line = [f"M={M} N={N:6d} K={K:5d} {kind:10s}"]
        us = timeit(lambda i: H.gemm(x, Ws[i], out, M, N, K, **kw), nbuf)
        line.append(f"bf16 {us:7.1f}us {rows*K*2/us/1e6:5.2f}TB/s")
        for v in ((0,) if kind.startswith("swiglu") else (162, 164)):
            H.gemm_set_option(11, v)
            us8 = timeit(lambda i: H.gemm_w8(x, Q[i][0], Q[i][1], out, M, N, K, **kw), nbuf)
            line.append(f"fp8 v{v} {us8:7.1f}us {rows*K/us8/1e6:5.2f}TB/s x{us/us8:4.2f}")
        H.gemm_set_option(11, 0)
        print("  ".join(line), flush=True)
        del Ws, Q
