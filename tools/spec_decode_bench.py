"""Draft-and-verify greedy decoding (`set_speculative`) against the plain loop at the full model size, on one MI355X.

  python tools/spec_decode_bench.py [--config desta25_llama31-8B_Qformer6L] [--batch 1,4,8,16] [--k 3,7] [--ctx 64] [--prompt-tail 16]
                                    [--new 64] [--weights {bf16,fp8}] [--prefill-chunk N] [--rounds 3] [--sample] [--penalty 1.05]
                                    [--no-greedy] [--attention {forward,split,ab}] [--kv {bf16,fp8}]
The workload flags are those of tools/decode_bench.py (--batch and --k take comma-separated lists).  For every batch size the plain
loop and, per k, three speculative legs alternate in ONE process for --rounds rounds after a warm-up of every leg; each run is
timed with HIP events around `_generate_step`, and the time of a prompt-only run (one new token, same leg, same round) is taken
off, so a figure is the decode loop alone, the host wait of every verify step included.  The drafts go in through `draft_tokens`:
  accepted  the greedy output of the verify path itself at this row count (the `rejected` leg's ids): every draft is right, the
            upper bound (ceil((new - 1) / (k + 1)) verify steps).  The PLAIN run's ids are not used: with synthetic weights the
            logits are nearly flat, and from 17 rows on the verify pass runs the wide projections, whose other summation order
            flips some near-ties (`tokens_equal_to_plain` reports the agreement); under lockstep acceptance one such row ends the
            accepted run of every row, which would measure the synthetic weights, not the step;
  rejected  all -1: no draft is ever right, one token per verify step, the pure overhead of verifying k + 1 rows;
  lookup    the prompt-lookup kernel on the prompt and the output.  THE WEIGHTS ARE SYNTHETIC: the acceptance of this leg says
            nothing about a trained checkpoint; it shows the cost of the lookup launch and that the path runs.
One JSON line per (batch, leg, round), one summary line per (batch, k) with medians, the spread over the rounds and the
break-even: a verify step costs `step_ms` (median over the accepted and rejected legs) and pays for itself once it emits
step_ms / plain_ms_per_token tokens, i.e. that many minus one accepted drafts per step.  B * (k + 1) > H.DECODE_MAX_ROWS runs the plain
loop (`spec_stats["reason"]`): the summary says so and reports no speculative figure.
--sample and --penalty P add, per batch size, the same plain / accepted / rejected / lookup legs under `set_speculative(k, scope="all")`
for sampled calls (temperature 0.7, top_p 0.9, the reference's defaults: `sample_top_p_rows` picks the verify rows) and for greedy
calls with a repetition penalty (`sample_rows`); every line carries its `mode`.  `accepted` again takes the path's own output (the
`rejected` leg's ids under the same mode) as drafts, and the plain leg of a mode is the plain loop with the same settings.
--attention picks the attention of the verify step (`set_speculative(k, attention=...)`): forward (default), split (the split-KV
verify kernels; on the bf16 cache from H.DECODE_ATTN_MIN_KEYS keys on, so give a --ctx that reaches them), or ab: the speculative
legs of both, alternating in the same rounds, one summary line per (k, attention).  --kv fp8 runs everything on the FP8 KV cache:
with attention forward the speculative legs report the plain loop (`"speculative": "not run: fp8 kv cache"`, today's fallback), with
split they speculate.  Every line carries `attention` and `kv`.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch  # noqa: E402


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="desta25_llama31-8B_Qformer6L")
    ap.add_argument("--batch", default="1,4,8,16")
    ap.add_argument("--k", default="3,7")
    ap.add_argument("--ctx", type=int, default=64)
    ap.add_argument("--prompt-tail", type=int, default=16, help="text tokens after the audio span")
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--weights", choices=("bf16", "fp8"), default="bf16")
    ap.add_argument("--prefill-chunk", type=int, default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sample", action="store_true", help="add the sampled legs (temperature 0.7, top_p 0.9: the reference's defaults), scope \"all\"")
    ap.add_argument("--penalty", type=float, default=None, help="add greedy legs with this repetition penalty (e.g. 1.05), scope \"all\"")
    ap.add_argument("--no-greedy", action="store_true", help="leave the plain greedy legs out")
    ap.add_argument("--attention", choices=("forward", "split", "ab"), default="forward", help="attention of the verify step; ab: both, alternating")
    ap.add_argument("--kv", choices=("bf16", "fp8"), default="bf16", help="what the KV cache holds (`set_kv_cache`)")
    a = ap.parse_args()
    batches, ks = [int(x) for x in a.batch.split(",")], [int(x) for x in a.k.split(",")]
    assert a.new >= 2 and a.rounds >= 1
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU path"
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    from desta.synthetic import FULL_CONFIGS, RandomWeights, synthetic_inputs, synthetic_waveform
    from desta import _hip as H
    dev = torch.device("cuda:0")
    cfg = DeSTA25Config(**FULL_CONFIGS[a.config])
    model = DeSTA25AudioModel(cfg, weights=RandomWeights(cfg, dev, seed=0), device=dev).eval()
    model.set_decode_weights(a.weights)
    model.set_prefill_chunk(a.prefill_chunk)
    model.set_kv_cache(a.kv)
    llm = model.llm
    attentions = ["forward", "split"] if a.attention == "ab" else [a.attention]
    modes = [] if a.no_greedy else [("greedy", dict(do_sample=False), "greedy")]
    if a.sample:
        modes.append(("sample", dict(do_sample=True, temperature=0.7, top_p=0.9, seed=1), "all"))
    if a.penalty is not None:
        modes.append((f"penalty {a.penalty}", dict(do_sample=False, repetition_penalty=a.penalty), "all"))
    assert modes, "nothing to run"

    for B in batches:
        t = synthetic_inputs(cfg, B, a.ctx, a.prompt_tail, dev, seed=5)
        mel = H.logmel(synthetic_waveform(B, dev, seed=6), cfg.encoder_config.num_mel_bins)
        inputs = {"context_input_ids": t["input_ids"], "context_attention_mask": t["attention_mask"],
                  "context_batch_start_positions": t["batch_start_positions"], "batch_features": mel,
                  "batch_transcription_ids": t["batch_transcription_ids"]}
        S = t["input_ids"].shape[1]

        for mode, gen_kw, scope in modes:
            def timed(k, att, drafts, new):
                """-> (ms of one `_generate_step` by HIP events, ids, spec_stats)"""
                model.set_speculative(k, scope=scope, attention=att)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                ids = model._generate_step(inputs, pad_token_id=0, max_new_tokens=new, eos_token_id=[], draft_tokens=drafts, **gen_kw)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1), ids, dict(llm.spec_stats)

            def leg(name, k, att, drafts):
                prompt_ms, _, _ = timed(k, att, None if drafts is None else drafts[:, :1], 1)
                ms, ids, st = timed(k, att, drafts, a.new)
                assert ids.shape == (B, a.new)
                steps = st["verify_steps"]
                r = {"mode": mode, "B": B, "prompt": S, "new": a.new, "weights": a.weights, "kv": a.kv, "leg": name, "k": k, "attention": att if k else None, "path": st["path"], "reason": st["reason"],
                     "prompt_ms": round(prompt_ms, 3), "decode_ms": round(ms - prompt_ms, 3),
                     "ms_per_emitted_token": round((ms - prompt_ms) / (a.new - 1), 4), "verify_steps": steps,
                     "tokens_per_verify_step": round((a.new - 1) / steps, 3) if steps else None,
                     "ms_per_verify_step": round((ms - prompt_ms) / steps, 4) if steps else None}
                print(json.dumps(r), flush=True)
                return r, ids

            _, plain_ids = leg("plain", None, "forward", None)                  # warm-up
            none = torch.full_like(plain_ids, -1)
            legs = [("plain", None, "forward", None)]
            for k, att in ((k, att) for k in ks for att in attentions):          # warm-up of every leg: buffers, workspaces, code objects
                _, own = leg("rejected", k, att, none)                           # the verify path's own greedy output at this row count
                legs += [("accepted", k, att, own), ("rejected", k, att, none), ("lookup", k, att, None)]
                for name, _, _, dr in legs[-3:]:
                    r, ids = leg(name, k, att, dr)
                    if r["path"] == "speculative":
                        print(json.dumps({"mode": mode, "B": B, "k": k, "attention": att, "leg": name,
                                          "tokens_equal_to_rejected_leg": float((ids == own).float().mean()),
                                          "tokens_equal_to_plain": float((ids == plain_ids).float().mean())}), flush=True)
            runs = {(name, k, att): [] for name, k, att, _ in legs}
            for _ in range(a.rounds):
                for name, k, att, dr in legs:
                    runs[(name, k, att)].append(leg(name, k, att, dr)[0])
            plain = [r["ms_per_emitted_token"] for r in runs[("plain", None, "forward")]]
            for k, att in ((k, att) for k in ks for att in attentions):
                acc, rej, look = runs[("accepted", k, att)], runs[("rejected", k, att)], runs[("lookup", k, att)]
                s = {"summary": f"{a.config} {mode} B={B} prompt={S} new={a.new} weights={a.weights} kv={a.kv} k={k} attention={att}", "mode": mode,
                     "attention": att, "kv": a.kv, "rounds": a.rounds,
                     "plain_ms_per_token": plain, "plain_median": _median(plain), "plain_spread": round(max(plain) - min(plain), 4)}
                if acc[0]["path"] != "speculative":
                    s["speculative"] = f"not run: {acc[0]['reason']}"
                    print(json.dumps(s), flush=True)
                    continue
                for name, rs in (("accepted", acc), ("rejected", rej), ("lookup", look)):
                    v = [r["ms_per_emitted_token"] for r in rs]
                    s[name] = {"ms_per_emitted_token": v, "median": _median(v), "spread": round(max(v) - min(v), 4),
                               "tokens_per_verify_step": rs[0]["tokens_per_verify_step"], "ms_per_verify_step": _median([r["ms_per_verify_step"] for r in rs])}
                step_ms = _median([r["ms_per_verify_step"] for r in acc + rej])
                s["verify_step_ms"] = step_ms
                s["verify_step_over_plain_step"] = round(step_ms / s["plain_median"], 3)
                s["break_even_tokens_per_verify_step"] = round(step_ms / s["plain_median"], 3)
                s["break_even_accepted_drafts_per_step"] = round(step_ms / s["plain_median"] - 1, 3)
                s["break_even_acceptance_of_k"] = round((step_ms / s["plain_median"] - 1) / k, 3)
                s["accepted_speedup_median"] = round(s["plain_median"] / s["accepted"]["median"], 3)
                s["accepted_faster_beyond_spread"] = bool(s["plain_median"] - s["accepted"]["median"] > s["plain_spread"] + s["accepted"]["spread"])
                s["rejected_slowdown_median"] = round(s["rejected"]["median"] / s["plain_median"], 3)
                s["lookup_note"] = "synthetic weights: the lookup leg's acceptance says nothing about a trained checkpoint"
                print(json.dumps(s), flush=True)
        model.set_speculative(None)


if __name__ == "__main__":
    main()
