"""What classifier-free guidance (`generate(guidance_scale=)`, `desta_cfg_scores_bf16`) costs, in one process on one GPU.

(a) The kernel beside `desta_topk_logprobs(top_n = 0)` on the same rows: that kernel reads every conditional logit once; the
guidance kernel reads the conditional and the unconditional row twice each and writes one row (10 bytes per column against 2).
One HIP-event pair per launch, the two calls alternating, median over --iters launches after a warm-up.  The buffers are the
same in every launch, so they come from the caches, as the logits of a decode step do (the lm_head has just written them); GB/s
counts the algorithm's bytes and is no HBM figure.

(b) ms per decode step on a full-size LLM with synthetic weights (--config, Llama-3.1-8B geometry by default), text-only prompts
of --prompt tokens (a decode step does not depend on where the prompt came from, and the audio encoder would only lengthen the
untimed part): the guided loop at Bc sequences (2 Bc rows) against the plain loop at Bc rows and at 2 Bc rows, the three legs
alternating (--rounds alternations after a warm-up of all three).  ms per step = (HIP-event time of --new tokens - time of 1
token) / (--new - 1), best of --repeat, so the prompt pass drops out.  "guided - plain(2Bc)" is what the guidance itself adds
to the rows it doubles: the kernel, the picked tokens copied for both halves, and the pick running on Bc instead of 2 Bc rows.

  python tools/guidance_bench.py [--vocab 128256 151936] [--rows 1 8 32] [--iters 30] [--no-kernel]
                                 [--config desta25_llama31-8B_Qformer6L] [--batch 1 8 32] [--new 33] [--rounds 3] [--no-generate]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch  # noqa: E402


def kernel_leg(a):
    from desta import _hip as H
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    for V in a.vocab:
        ld = (V + 63) // 64 * 64
        for rows in a.rows:
            x = (torch.randn(2 * rows, ld, device=dev, generator=g) * 3).to(torch.bfloat16)
            out = torch.zeros(rows, ld, dtype=torch.bfloat16, device=dev)
            tok = torch.randint(0, V, (rows,), device=dev, generator=g)
            lp = torch.zeros(rows, dtype=torch.float32, device=dev)
            cases = {"cfg_scores": lambda: H.cfg_scores(x[:rows], x[rows:], ld, rows, V, 3.0, out, ld),
                     "topk_logprobs(top_n=0)": lambda: H.topk_logprobs(x, ld, tok, rows, V, 0, lp, None, None)}
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
            med = {k: statistics.median(v) for k, v in times.items()}
            nbytes = {"cfg_scores": 10 * rows * V, "topk_logprobs(top_n=0)": 2 * rows * V}
            for name, ts in times.items():
                print(json.dumps({"kernel": name, "rows": rows, "vocab": V, "us_median": round(med[name], 1), "us_min": round(min(ts), 1),
                                  "us_max": round(max(ts), 1), "launches": len(ts), "algorithm_GB_per_s": round(nbytes[name] / med[name] / 1e3, 1)}), flush=True)
            print(json.dumps({"rows": rows, "vocab": V, "ratio_cfg_over_topk": round(med["cfg_scores"] / med["topk_logprobs(top_n=0)"], 2)}), flush=True)


def generate_leg(a):
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    from desta.synthetic import FULL_CONFIGS, RandomWeights
    dev = torch.device("cuda:0")
    cfg = DeSTA25Config(**FULL_CONFIGS[a.config])
    model = DeSTA25AudioModel(cfg, weights=RandomWeights(cfg, dev, seed=0), device=dev).eval()
    V = cfg.llm_config.vocab_size

    def inputs(rows):
        ids = torch.randint(3, V, (rows, a.prompt), generator=torch.Generator().manual_seed(5 + rows))
        return {"context_input_ids": ids, "context_attention_mask": torch.ones_like(ids), "context_batch_start_positions": [],
                "batch_features": None, "batch_transcription_ids": []}

    def step_ms(inp, scale):
        res = []
        for new in (1, a.new):
            best = None
            for _ in range(a.repeat):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                model._generate_step(inp, pad_token_id=0, max_new_tokens=new, do_sample=False, eos_token_id=[], guidance_scale=scale)
                e1.record()
                e1.synchronize()
                dt = e0.elapsed_time(e1)
                best = dt if best is None else min(best, dt)
            res.append(best)
        return (res[1] - res[0]) / (a.new - 1)

    for Bc in a.batch:
        one, two = inputs(Bc), inputs(2 * Bc)
        legs = {f"guided(Bc={Bc})": (two, a.scale), f"plain({Bc} rows)": (one, None), f"plain({2 * Bc} rows)": (two, None)}
        for inp, scale in legs.values():                                               # warm-up of every leg
            step_ms(inp, scale)
        runs = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, (inp, scale) in legs.items():
                c0 = H.CFG_SCORES_CALLS
                runs[k].append(round(step_ms(inp, scale), 4))
                assert H.CFG_SCORES_CALLS - c0 == (0 if scale is None else a.repeat * (1 + a.new))
        med = {k: statistics.median(v) for k, v in runs.items()}
        gk, pk, p2k = list(legs)
        print(json.dumps({"generate": f"{a.config} Bc={Bc} prompt={a.prompt} new={a.new} greedy g={a.scale}", "rounds": a.rounds, "ms_per_step": runs,
                          "median_ms_per_step": med, "spread_ms": {k: round(max(v) - min(v), 4) for k, v in runs.items()},
                          "guided_minus_plain_2Bc_us": round((med[gk] - med[p2k]) * 1e3, 1),
                          "guided_over_plain_Bc": round(med[gk] / med[pk], 4), "guided_over_plain_2Bc": round(med[gk] / med[p2k], 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, nargs="+", default=[128256, 151936])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--config", default="desta25_llama31-8B_Qformer6L")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--new", type=int, default=33)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=3.0)
    ap.add_argument("--no-generate", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("guidance_bench: needs the GPU (no timing without one)")
    if not a.no_kernel:
        kernel_leg(a)
    if not a.no_generate:
        generate_leg(a)


if __name__ == "__main__":
    main()
