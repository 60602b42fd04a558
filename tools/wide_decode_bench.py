"""Wide (17 <= M <= 64) weight-streaming GEMM of the decode step (desta_gemm_wide_nt) per projection shape of Llama-3.1-8B, bf16
and weight-only FP8, with the epilogue the decode step uses (residual / SwiGLU).  Baseline: ceil(M/16) launches of the 16-row
kernel on 16-row slices (the only way the parent's kernels run these M: the weights are streamed once per slice).  Both legs
alternate in one process (--rounds alternations); every timed launch reads a DIFFERENT weight copy (rotating set larger than the
256 MiB Infinity Cache), so the weights come from HBM.  Per leg: median us over the rounds and the spread (max - min); GB/s counts
the weight bytes of the form that ran, once; x = baseline median / wide median.  us = HIP events around a run of back-to-back
calls from Python, so it is kernel time only while the host enqueues faster than the device runs: `enqueue` is the host time per
iteration to issue the calls (no synchronise), and a line whose enqueue time reaches 90 % of a leg's us is marked HOST-BOUND
(that leg's figure is then an upper bound of its kernel time, and the ratio says nothing about the kernels).
  python tools/wide_decode_bench.py [--rows 17,32,48,64] [--rounds 3] [--shapes qkv,o,gate_up,down,lm_head]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch
from desta import _hip as H

SHAPES = {"qkv": (6144, 4096, "plain"), "o": (4096, 4096, "res"), "gate_up": (14336, 4096, "swiglu"), "down": (4096, 14336, "res"),
          "lm_head": (128256, 4096, "plain")}


def timeit(fn, nbuf):
    reps = max(2 * nbuf, 12)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i % nbuf)
    enq = (time.perf_counter() - t0) * 1e6 / reps                            # host time to ENQUEUE one iteration
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, enq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="17,32,48,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    assert a.rounds >= 3, "at least three alternations"
    for name in a.shapes.split(","):
        N, K, kind = SHAPES[name]
        rows = 2 * N if kind == "swiglu" else N
        nbuf = max(2, int(320 * 2**20 / (rows * K)) + 1)                     # the FP8 copies alone exceed the Infinity Cache
        Ws = [(torch.randn(rows, K, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(nbuf)]
        Q = [H.quantize_rows_e4m3(w) for w in Ws]
        for M in (int(m) for m in a.rows.split(",")):
            x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
            res = torch.randn(M, N, device="cuda").to(torch.bfloat16)
            out = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
            act = 4 if kind == "swiglu" else 0
            slices = [(r0, min(16, M - r0)) for r0 in range(0, M, 16)]

            def kw(r0=None):
                if kind != "res":
                    return dict(act=act)
                return dict(residual=res if r0 is None else res[r0:])

            def wide16(i):
                H.gemm_wide(x, Ws[i], out, M, N, K, **kw())

            def base16(i):
                for r0, n in slices:
                    H.gemm(x[r0:], Ws[i], out[r0:], n, N, K, **kw(r0))

            def wide8(i):
                H.gemm_wide(x, Q[i][0], out, M, N, K, scale=Q[i][1], **kw())

            def base8(i):
                for r0, n in slices:
                    H.gemm_w8(x[r0:], Q[i][0], Q[i][1], out[r0:], n, N, K, **kw(r0))

            for tag, wide, base, wbytes in (("bf16", wide16, base16, rows * K * 2), ("fp8 ", wide8, base8, rows * K)):
                for fn in (wide, base):                                      # warm up both legs on every copy
                    for i in range(nbuf):
                        fn(i)
                tw, tb, ew, eb = [], [], [], []
                for _ in range(a.rounds):
                    t, e = timeit(wide, nbuf)
                    tw.append(t), ew.append(e)
                    t, e = timeit(base, nbuf)
                    tb.append(t), eb.append(e)
                mw, mb = sorted(tw)[len(tw) // 2], sorted(tb)[len(tb) // 2]
                hb = " HOST-BOUND" if min(ew) > 0.9 * mw or min(eb) > 0.9 * mb else ""
                print(f"{name:8s} M={M:2d} N={N:6d} K={K:5d} {tag}  wide {mw:8.1f}us (spread {max(tw) - min(tw):5.1f}, enqueue {min(ew):5.1f}) {wbytes / mw / 1e3:7.1f} GB/s   "
                      f"{len(slices)} x 16-row {mb:8.1f}us (spread {max(tb) - min(tb):5.1f}, enqueue {min(eb):5.1f}) {wbytes / mb / 1e3:7.1f} GB/s   x{mb / mw:4.2f}{hb}", flush=True)
        del Ws, Q


if __name__ == "__main__":
    main()
