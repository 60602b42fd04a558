"""Time of `desta_token_logprobs` beside `desta_causal_lm_loss(write_grad=0)` on the same [rows, vocab] bf16 logits in one process:
both read every logit once.  One HIP-event pair per launch, the two calls alternating, median over `--iters` launches after a
warm-up; bytes = rows x vocab x 2 (the algorithm's reads), share of the HBM peak taken as 6.3 TB/s unless `--peak-tbs` says otherwise.

  python tools/logprob_bench.py [--rows 1024 5120] [--vocab 128256] [--iters 30]

--generate: what `generate(logprobs=5)` adds to a decode step.  One full-size model, B = 8 and B = 64 (--batch), greedy decode with
`logprobs=None` and `logprobs=5` alternating in ONE process (--rounds alternations after a warm-up of both); ms per decode step =
(time of --new tokens - time of 1 token) / (--new - 1), best of --repeat, so the prompt pass drops out.  Nothing else runs in the
timed region.

  python tools/logprob_bench.py --generate [--config desta25_llama31-8B_Qformer6L] [--batch 8 64] [--new 33] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch  # noqa: E402


def generate_leg(a):
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    from desta.synthetic import FULL_CONFIGS, RandomWeights, synthetic_inputs, synthetic_waveform
    dev = torch.device("cuda:0")
    cfg = DeSTA25Config(**FULL_CONFIGS[a.config])
    model = DeSTA25AudioModel(cfg, weights=RandomWeights(cfg, dev, seed=0), device=dev).eval()
    for B in a.batch:
        t = synthetic_inputs(cfg, B, 64, 16, dev, seed=5)
        mel = H.logmel(synthetic_waveform(B, dev, seed=6), cfg.encoder_config.num_mel_bins)
        inputs = {"context_input_ids": t["input_ids"], "context_attention_mask": t["attention_mask"],
                  "context_batch_start_positions": t["batch_start_positions"], "batch_features": mel,
                  "batch_transcription_ids": t["batch_transcription_ids"]}

        def step_ms(n):
            res = []
            for new in (1, a.new):
                best = None
                for _ in range(a.repeat):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model._generate_step(inputs, pad_token_id=0, max_new_tokens=new, do_sample=False, eos_token_id=[], logprobs=n)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                res.append(best)
            return (res[1] - res[0]) * 1e3 / (a.new - 1)
        legs = {"logprobs=None": None, "logprobs=5": 5}
        for n in legs.values():                                                        # warm-up of both legs
            step_ms(n)
        runs = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, n in legs.items():
                c0 = H.TOPK_LOGPROBS_CALLS
                runs[k].append(round(step_ms(n), 4))
                assert (H.TOPK_LOGPROBS_CALLS - c0) == (0 if n is None else a.repeat * (1 + a.new))
        med = {k: statistics.median(v) for k, v in runs.items()}
        print(json.dumps({"generate": f"{a.config} B={B} prompt={t['input_ids'].shape[1]} new={a.new} greedy", "rounds": a.rounds,
                          "ms_per_step": runs, "median_ms_per_step": med, "spread_ms": {k: round(max(v) - min(v), 4) for k, v in runs.items()},
                          "overhead_us_per_step": round((med["logprobs=5"] - med["logprobs=None"]) * 1e3, 1),
                          "overhead_share": round(med["logprobs=5"] / med["logprobs=None"] - 1, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--generate", action="store_true", help="decode-step overhead of generate(logprobs=5) instead of the kernel timing")
    ap.add_argument("--config", default="desta25_llama31-8B_Qformer6L")
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--new", type=int, default=33)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 5120])
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--peak-tbs", type=float, default=6.3)
    a = ap.parse_args()
    if a.generate:
        return generate_leg(a)
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
