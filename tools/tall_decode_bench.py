"""Tall (65 <= M <= 256) weight-streaming GEMM of the decode step (desta_gemm_tall_nt) per projection shape of Llama-3.1-8B, bf16
and weight-only FP8, with the epilogue the decode step uses (residual / SwiGLU).  Baselines, the two ways the kernels that
existed before it run these M:
  (a) ceil(M/64) launches of `gemm_wide` on near-equal row slices (the weights are streamed once per slice), bf16 and FP8;
  (b) bf16 only: `gemm`, the tile GEMM of the prompt pass, with the same epilogue (gate|up: the plain 2N-row GEMM + `swiglu_fwd`).
All legs alternate in one process (--rounds alternations); every timed launch reads a DIFFERENT weight copy (rotating set larger
than the 256 MiB Infinity Cache), so the weights come from HBM.  Per leg: median us over the rounds and the spread (max - min);
GB/s counts the weight bytes of the form that ran, once; x = baseline median / tall median.  us = HIP events around a run of
back-to-back calls from Python, so it is kernel time only while the host enqueues faster than the device runs: `enq` is the host
time per iteration to issue the calls (no synchronise), and a line where it reaches 90 % of a leg's us is marked HOST-BOUND (that
leg's figure is then an upper bound of its kernel time).  For those lines take kernel times from a kernel trace of a run of its own
(--trace-loop runs every leg a fixed number of times without timing, for a tracer's per-kernel statistics).
  python tools/tall_decode_bench.py [--rows 65,128,192,256] [--rounds 3] [--shapes qkv,o,gate_up,down,lm_head] [--trace-loop N]"""
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


def row_slices(M):
    """ceil(M/64) near-equal slices: every one inside gemm_wide's 17..64 rows."""
    n = -(-M // 64)
    cuts = [M * i // n for i in range(n + 1)]
    return [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="65,128,192,256")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--trace-loop", type=int, default=0, help="no timing: every leg N times on rotating copies, for a kernel trace")
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
            gu = torch.empty(M, rows, dtype=torch.bfloat16, device="cuda") if kind == "swiglu" else None
            act = 4 if kind == "swiglu" else 0
            slices = row_slices(M)

            def kw(r0=None):
                if kind != "res":
                    return dict(act=act)
                return dict(residual=res if r0 is None else res[r0:])

            def tall16(i):
                H.gemm_tall(x, Ws[i], out, M, N, K, **kw())

            def wide16(i):
                for r0, n in slices:
                    H.gemm_wide(x[r0:], Ws[i], out[r0:], n, N, K, **kw(r0))

            def tile16(i):
                if kind == "swiglu":
                    H.gemm(x, Ws[i], gu, M, rows, K)
                    H.swiglu_fwd(gu, out, M, N)
                else:
                    H.gemm(x, Ws[i], out, M, N, K, **({"residual": res} if kind == "res" else {}))

            def tall8(i):
                H.gemm_tall(x, Q[i][0], out, M, N, K, scale=Q[i][1], **kw())

            def wide8(i):
                for r0, n in slices:
                    H.gemm_wide(x[r0:], Q[i][0], out[r0:], n, N, K, scale=Q[i][1], **kw(r0))

            for tag, legs, wbytes in (("bf16", (("tall", tall16), (f"{len(slices)}xwide", wide16), ("gemm", tile16)), rows * K * 2),
                                      ("fp8 ", (("tall", tall8), (f"{len(slices)}xwide", wide8)), rows * K)):
                for _, fn in legs:                                           # warm up every leg on every copy
                    for i in range(nbuf):
                        fn(i)
                if a.trace_loop:
                    for _, fn in legs:
                        for i in range(a.trace_loop):
                            fn(i % nbuf)
                    torch.cuda.synchronize()
                    continue
                ts = {n: [] for n, _ in legs}
                es = {n: [] for n, _ in legs}
                for _ in range(a.rounds):
                    for n, fn in legs:
                        t, e = timeit(fn, nbuf)
                        ts[n].append(t), es[n].append(e)
                med = {n: sorted(v)[len(v) // 2] for n, v in ts.items()}
                hb = " HOST-BOUND" if any(min(es[n]) > 0.9 * med[n] for n in med) else ""
                line = f"{name:8s} M={M:3d} N={N:6d} K={K:5d} {tag}"
                for n, _ in legs:
                    line += f"  {n} {med[n]:8.1f}us (spread {max(ts[n]) - min(ts[n]):5.1f}, enq {min(es[n]):5.1f}) {wbytes / med[n] / 1e3:7.1f} GB/s"
                    if n != "tall":
                        line += f" x{med[n] / med['tall']:4.2f}"
                print(line + hb, flush=True)
        del Ws, Q


if __name__ == "__main__":
    main()
