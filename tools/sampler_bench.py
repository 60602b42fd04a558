"""Per-call time of the decode-step samplers on [rows, vocab] bf16 logits: today's `sample_top_p_k` (temperature + top-p),
`sample_chain_k` (desta_sample_bf16: top-p only, and the full chain penalty + temperature + top-k + top-p + min-p) and
`sample_greedy_k` (greedy with a repetition penalty), `argmax_bf16` for scale, and `topk_logprob_k` (desta_topk_logprobs, the token's
log-probability + top 5 of generate(logprobs=5)) beside the chain sampler it follows in a decode step.  Device-event timing over `--iters`
back-to-back calls; for kernel times run it under `rocprofv3 --kernel-trace --stats`.

--grouped adds the entry points of a verify step (`sample_rows`, `sample_top_p_rows`) at batch x width = 4, 8, 32 and 64 rows against
the one-row entry points at the same row count (`grouped()` below).

  python tools/sampler_bench.py [--rows 8] [--vocab 128256 151936] [--iters 200] [--hist 256] [--grouped] [--rounds 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--vocab", type=int, nargs="+", default=[128256, 151936])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--hist", type=int, default=256, help="history length of the penalised cases")
    ap.add_argument("--grouped", action="store_true", help="also time the grouped entry points at 4, 8, 32 and 64 rows against the one-row ones")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of the --grouped comparison")
    a = ap.parse_args()
    from desta import _hip as H
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for V in a.vocab:
        ld = (V + 63) // 64 * 64
        B = a.rows
        logits = (torch.randn(B, ld, device=dev, generator=g) * 3).to(torch.bfloat16)
        hist = torch.randint(0, V, (B, a.hist), device=dev, generator=g)
        out = torch.zeros(B, dtype=torch.int64, device=dev)
        tok = torch.randint(0, V, (B,), device=dev, generator=g)
        lp, top_ids, top_lp = torch.zeros(B, device=dev), torch.zeros(B, 5, dtype=torch.int32, device=dev), torch.zeros(B, 5, device=dev)
        cases = {
            "argmax_bf16": lambda: H.argmax_bf16(logits, ld, B, V, out),
            "sample_top_p (old)": lambda: H.sample_top_p(logits, ld, B, V, 0.7, 0.9, 1, 0, out),
            "sample chain top_p": lambda: H.sample(logits, ld, B, V, out, temperature=0.7, top_p=0.9, seed=1),
            "sample chain full": lambda: H.sample(logits, ld, B, V, out, temperature=0.7, top_k=50, top_p=0.9, min_p=0.05,
                                                  repetition_penalty=1.2, hist=hist, hist_len=a.hist, seed=1),
            "sample greedy + penalty": lambda: H.sample(logits, ld, B, V, out, do_sample=False, repetition_penalty=1.2, hist=hist,
                                                        hist_len=a.hist),
            "topk_logprobs n=5": lambda: H.topk_logprobs(logits, ld, tok, B, V, 5, lp, top_ids, top_lp),
        }
        for name, fn in cases.items():
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            print(json.dumps({"shape": [B, V], "case": name, "us_per_call": round(e0.elapsed_time(e1) * 1e3 / a.iters, 2)}), flush=True)
        if a.grouped:
            grouped(H, a, V, ld, dev, g)


def grouped(H, a, V, ld, dev, g):
    """The grouped entry points (`sample_rows`, `sample_top_p_rows`: batch x width rows of a verify step) against the one-row entry
    points at the same row count, alternating in one process for --rounds rounds: medians, spreads (max - min over the rounds) and
    the fold rule, grouped median <= one-row median + both spreads."""
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.iters

    for rows in (4, 8, 32, 64):
        for width in sorted({min(rows, 4), min(rows, 8)}):
            batch = rows // width
            logits = (torch.randn(rows, ld, device=dev, generator=g) * 3).to(torch.bfloat16)
            hist = torch.randint(0, V, (rows, a.hist), device=dev, generator=g)
            tail = torch.randint(0, V, (batch, width), device=dev, generator=g)
            out = torch.zeros(rows, dtype=torch.int64, device=dev)
            full = dict(temperature=0.7, top_k=50, top_p=0.9, min_p=0.05, repetition_penalty=1.2, hist_len=a.hist, seed=1)
            pairs = {
                "top_p": (lambda: H.sample_top_p(logits, ld, rows, V, 0.7, 0.9, 1, 0, out),
                          lambda: H.sample_top_p_rows(logits, ld, batch, width, V, 0.7, 0.9, 1, 0, out)),
                "chain top_p": (lambda: H.sample(logits, ld, rows, V, out, temperature=0.7, top_p=0.9, seed=1),
                                lambda: H.sample_rows(logits, ld, batch, width, V, out, temperature=0.7, top_p=0.9, seed=1)),
                "chain full": (lambda: H.sample(logits, ld, rows, V, out, hist=hist, **full),
                               lambda: H.sample_rows(logits, ld, batch, width, V, out, hist=hist, tail=tail, **full)),
                "greedy + penalty": (lambda: H.sample(logits, ld, rows, V, out, do_sample=False, repetition_penalty=1.2, hist=hist, hist_len=a.hist),
                                     lambda: H.sample_rows(logits, ld, batch, width, V, out, do_sample=False, repetition_penalty=1.2, hist=hist,
                                                           hist_len=a.hist, tail=tail)),
            }
            for name, (one, grp) in pairs.items():
                for fn in (one, grp):
                    for _ in range(10):
                        fn()
                torch.cuda.synchronize()
                t1, tg = [], []
                for _ in range(a.rounds):
                    t1.append(timed(one))
                    tg.append(timed(grp))
                m1, mg = sorted(t1)[len(t1) // 2], sorted(tg)[len(tg) // 2]
                s1, sg = max(t1) - min(t1), max(tg) - min(tg)
                print(json.dumps({"rows": rows, "batch": batch, "width": width, "vocab": V, "case": name, "one_row_us": round(m1, 2),
                                  "one_row_spread": round(s1, 2), "grouped_us": round(mg, 2), "grouped_spread": round(sg, 2),
                                  "grouped_within_spreads": bool(mg - m1 <= s1 + sg)}), flush=True)


if __name__ == "__main__":
    main()
