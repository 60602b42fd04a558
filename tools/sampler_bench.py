"""Per-call time of the decode-step samplers on [rows, vocab] bf16 logits: today's `sample_top_p_k` (temperature + top-p),
`sample_chain_k` (desta_sample_bf16: top-p only, and the full chain penalty + temperature + top-k + top-p + min-p) and
`sample_greedy_k` (greedy with a repetition penalty), `argmax_bf16` for scale, and `topk_logprob_k` (desta_topk_logprobs, the token's
log-probability + top 5 of generate(logprobs=5)) beside the chain sampler it follows in a decode step.  Device-event timing over `--iters`
back-to-back calls; for kernel times run it under `rocprofv3 --kernel-trace --stats`.

  python tools/sampler_bench.py [--rows 8] [--vocab 128256 151936] [--iters 200] [--hist 256]
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


if __name__ == "__main__":
    main()
