"""Time of `desta_token_logprobs` beside `desta_causal_lm_loss(write_grad=0)` on the same [rows, vocab] bf16 logits in one process:
both read every logit once.  One HIP-event pair per launch, the two calls alternating, median over `--iters` launches after a
warm-up; bytes = rows x vocab x 2 (the algorithm's reads), share of the HBM peak taken as 6.3 TB/s unless `--peak-tbs` says otherwise.

  python tools/logprob_bench.py [--rows 1024 5120] [--vocab 128256] [--iters 30]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 5120])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--peak-tbs", type=float, default=6.3)
    a = ap.parse_args()
    from desta import _hip as H
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    V = a.vocab
    ld = (V + 63) // 64 * 64
    for rows in a.rows:
        logits = torch.empty(rows + 1, ld, dtype=torch.bfloat16, device=dev)
        for r0 in range(0, rows + 1, 512):                                         # filled in slices: no fp32 copy of the whole grid
            n = min(512, rows + 1 - r0)
            logits[r0:r0 + n] = (torch.randn(n, ld, device=dev, generator=g) * 3).to(torch.bfloat16)
        labels = torch.randint(0, V, (rows,), device=dev, generator=g)
        lab_ce = torch.cat([torch.full((1,), -100, device=dev), labels, torch.full((1,), -100, device=dev)])   # row i predicts lab_ce[1 + i]
        lp = torch.zeros(rows, dtype=torch.float32, device=dev)
        top = torch.zeros(rows, dtype=torch.uint8, device=dev)
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        cases = {"token_logprobs": lambda: H.token_logprobs(logits, ld, labels, rows, V, lp, top),
                 "causal_lm_loss(write_grad=0)": lambda: H.causal_lm_loss(logits, ld, lab_ce, 1, rows + 1, V, loss, write_grad=False)}
        for fn in cases.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in cases}
        for _ in range(a.iters):
            for name, fn in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
        agree = abs(float(-lp.double().sum() / rows) - float(loss)) / abs(float(loss))
        for name, ts in times.items():
            med = statistics.median(ts)
            tbs = rows * V * 2 / med / 1e6
            print(json.dumps({"rows": rows, "vocab": V, "case": name, "us_median": round(med, 1), "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                              "launches": len(ts), "TB_per_s": round(tbs, 3), "hbm_peak_share": round(tbs / a.peak_tbs, 3)}), flush=True)
        print(json.dumps({"rows": rows, "mean_nll_vs_loss_rel_diff": agree,
                          "ratio_logprobs_over_loss": round(statistics.median(times["token_logprobs"]) / statistics.median(times["causal_lm_loss(write_grad=0)"]), 3)}), flush=True)


if __name__ == "__main__":
    main()
