"""Decode-side measurement of `_generate_step` at the full model size: prompt pass + KV-cached greedy
decode on one MI355X.  Reports prompt ms, ms per generated token (whole batch), tokens/s, and the weight-streaming
rate of the decode GEMMs (bytes of frozen LLM weights read per token / token time; HBM peak ~8 TB/s).

  python tools/decode_bench.py [--config desta25_llama31-8B_Qformer6L] [--batch 8] [--ctx 64] [--prompt-tail 16] [--new 64]
                               [--do-sample --temperature T --top-p P --top-k K --min-p M --repetition-penalty R]
                               [--weights {bf16,fp8,mxfp4}] [--ab [--rounds R]] [--attn-ab [--rounds R]] [--kv {bf16,fp8}] [--kv-ab [--rounds R]]
                               [--prefill-chunk N[,N...]] [--prefill-ab [--rounds R]] [--rows-ab B1,B2,... [--rounds R]]
Without --do-sample the decode is greedy (with --repetition-penalty, through the full-chain sampler kernel).
--weights: what the decode steps stream (`set_decode_weights`; fp8 = weight-only OCP e4m3, half the bytes; mxfp4 = OCP MXFP4,
0.266 of the bytes).  --ab alternates bf16, fp8 and mxfp4 in ONE process on one model (R rounds of bf16, fp8, mxfp4) and prints one
line per leg and round plus a summary with the spread over the rounds: the legs of the same process are the yardstick, never a
number from another box.  "X faster than Y beyond the spread": the worst pairing's margin (min of Y - max of X) exceeds the two
legs' summed spreads.
--kv: what the LLM's KV cache holds (`set_kv_cache`; fp8 = e4m3 bytes + per-head scales, 0.516 of the bytes).  --kv-ab alternates
the two cache kinds for the chosen --weights in ONE process, R rounds, same report, plus the bytes each kind's slabs allocate
(`torch.cuda.memory_allocated` deltas around the first allocation).
--attn-ab alternates, for the chosen --weights, the decode step's attention dispatch (split-KV kernel from
H.DECODE_ATTN_MIN_KEYS keys on) with the forward kernel at every length (H.DECODE_ATTN_MIN_KEYS = 1 << 30, the path before the
split-KV kernel) in ONE process, R rounds, same report.
--batch above 64 runs with `set_decode_rows(256)` (the tall projections, the lean prompt pass, the sliced encoder).  --rows-ab
B1,B2,...: alternates the batch sizes (the first rows of the --batch inputs, so --batch is the largest) on bf16 and fp8 decode
weights in ONE process, R rounds: ms per step, tokens/s and weight GB/s per (rows, weights) with the spread over the rounds, and
whether each size's tokens/s exceed the first size's beyond the spread.
--prefill-chunk N: the prompt pass is the lean chunked one (`set_prefill_chunk(N)`) in every leg above.  --prefill-ab alternates
today's prompt pass (the training forward) and the chunked pass, one leg per N of a comma-separated --prefill-chunk, in ONE
process for the chosen --kv: prompt ms (one generated token) and `torch.cuda.max_memory_allocated` of each leg, one leg at a time
with the other legs' buffers dropped and `reset_peak_memory_stats` in between; a leg that does not fit reports "oom".  Under
--kv fp8 one more chunked prompt per N runs with the kernel profile open: the share of desta_kv8_dequant in the prompt pass.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="desta25_llama31-8B_Qformer6L")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=64)
    ap.add_argument("--prompt-tail", type=int, default=16, help="text tokens after the audio span")
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--do-sample", action="store_true")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--min-p", type=float, default=None)
    ap.add_argument("--repetition-penalty", type=float, default=None)
    ap.add_argument("--weights", choices=("bf16", "fp8", "mxfp4"), default="bf16")
    ap.add_argument("--ab", action="store_true", help="alternate bf16 / fp8 / mxfp4 decode weights in this process")
    ap.add_argument("--attn-ab", action="store_true", help="alternate split-KV / forward-kernel decode attention in this process")
    ap.add_argument("--kv", choices=("bf16", "fp8"), default="bf16")
    ap.add_argument("--kv-ab", action="store_true", help="alternate bf16 / fp8 KV cache in this process")
    ap.add_argument("--prefill-chunk", default=None, help="positions per chunk of the lean prompt pass (--prefill-ab: a comma-separated list)")
    ap.add_argument("--prefill-ab", action="store_true", help="alternate today's prompt pass / the chunked pass in this process")
    ap.add_argument("--rows-ab", default=None, help="comma-separated batch sizes (<= --batch) alternated on bf16 / fp8 decode weights in this process")
    ap.add_argument("--rounds", type=int, default=3, help="--ab / --attn-ab / --kv-ab / --prefill-ab / --rows-ab: alternations")
    a = ap.parse_args()
    chunks = [int(x) for x in a.prefill_chunk.split(",")] if a.prefill_chunk else []
    if a.prefill_ab and not chunks:
        ap.error("--prefill-ab needs --prefill-chunk N[,N...]")
    if not a.prefill_ab and len(chunks) > 1:
        ap.error("several --prefill-chunk values need --prefill-ab")
    gen = dict(do_sample=a.do_sample, temperature=a.temperature, top_p=a.top_p, top_k=a.top_k, min_p=a.min_p,
               repetition_penalty=a.repetition_penalty)
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    from desta.synthetic import FULL_CONFIGS, RandomWeights, synthetic_inputs, synthetic_waveform
    from desta import _hip as H
    dev = torch.device("cuda:0")
    cfg = DeSTA25Config(**FULL_CONFIGS[a.config])
    model = DeSTA25AudioModel(cfg, weights=RandomWeights(cfg, dev, seed=0), device=dev).eval()
    B = a.batch
    t = synthetic_inputs(cfg, B, a.ctx, a.prompt_tail, dev, seed=5)
    mel = H.logmel(synthetic_waveform(B, dev, seed=6), cfg.encoder_config.num_mel_bins)
    inputs = {"context_input_ids": t["input_ids"], "context_attention_mask": t["attention_mask"],
              "context_batch_start_positions": t["batch_start_positions"], "batch_features": mel,
              "batch_transcription_ids": t["batch_transcription_ids"]}
    S = t["input_ids"].shape[1]
    c = cfg.llm_config
    per_layer = (c.num_attention_heads + 2 * c.num_key_value_heads) * c.head_dim * c.hidden_size + c.num_attention_heads * c.head_dim * c.hidden_size \
        + 3 * c.hidden_size * c.intermediate_size
    welems = c.num_hidden_layers * per_layer + c.vocab_size * c.hidden_size
    mode = "sample " + " ".join(f"{k}={v}" for k, v in gen.items() if k != "do_sample" and v is not None) if a.do_sample else \
        ("greedy" + (f" repetition_penalty={a.repetition_penalty}" if a.repetition_penalty is not None else ""))

    model.set_kv_cache(a.kv)
    if B > H.DECODE_MAX_ROWS:                                                # opt in: a KV-cached step of up to 256 rows
        model.set_decode_rows(H.DECODE_TALL_MAX_ROWS)
    if chunks and not a.prefill_ab:
        model.set_prefill_chunk(chunks[0])

    if a.prefill_ab:
        llm = model.llm
        model.set_decode_weights(a.weights)
        fwd_bufs = ("cos_sin", "cos_sin_il", "pos_rows", "xs", "sv", "rf", "hb", "hbc", "act", "logits", "dxa", "dxb", "dgu", "dqkv", "datt")

        def drop():                                                          # every leg starts without the other legs' activations
            for n in fwd_bufs:
                setattr(llm, n, None)
            llm.B = llm.S = 0
            llm._pf = llm.kv_cache = llm.kv_scale = llm.kv_scale_v = llm.kv_stage = None
            llm._gen_shape = None
            torch.cuda.synchronize()
            torch.cuda.empty_cache()

        def forward_bytes():                                                 # what `CausalLMHIP._alloc(B, S)` asks for: the training step's save set
            M, L, h, I = B * S, llm.L, llm.h, llm.I
            aw = llm.hq * llm.hd
            per_layer = 2 * M * (llm.qkvw + aw + h + 2 * I) + 4 * (2 * M + B * llm.hq * S)
            return 2 * M * ((L + 1) * h + 4 * h + I + llm.Vp + 2 * I + llm.qkvw + aw) + L * per_layer

        def prompt(C):
            model.set_prefill_chunk(C)
            drop()
            if C is None and forward_bytes() > torch.cuda.mem_get_info()[0]:  # do not walk into the allocator's limit on purpose
                r = {"prompt_ms": "oom", "peak_GiB": "oom", "peak_above_start_GiB": "oom", "needs_GiB": round(forward_bytes() / 2 ** 30, 1)}
                print(json.dumps({"leg": "forward", "B": B, "prompt": S, "kv_cache": a.kv, **r}), flush=True)
                return r
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            try:
                times = []
                for _ in range(a.repeat + 1):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    model._generate_step(inputs, pad_token_id=0, max_new_tokens=1, eos_token_id=[], **gen)
                    torch.cuda.synchronize()
                    times.append(time.perf_counter() - t0)
                best = min(times[1:])                                        # the first run allocates: not timed
                r = {"prompt_ms": round(best * 1e3, 2), "peak_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3),
                     "peak_above_start_GiB": round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3)}
            except torch.cuda.OutOfMemoryError:
                r = {"prompt_ms": "oom", "peak_GiB": "oom", "peak_above_start_GiB": "oom"}
            print(json.dumps({"leg": "forward" if C is None else f"chunk{C}", "B": B, "prompt": S, "kv_cache": a.kv, **r}), flush=True)
            return r
        legs = [None] + chunks
        runs = {C: [] for C in legs}
        for C in legs:                                                       # warm-up: workspaces, merged / transposed weights
            prompt(C)
        for _ in range(a.rounds):
            for C in legs:
                runs[C].append(prompt(C))
        summary = {"prefill_ab": f"{a.config} B={B} prompt={S} kv={a.kv}", "rounds": a.rounds, "weights_GiB": None}
        for C in legs:
            name = "forward" if C is None else f"chunk{C}"
            ms = [r["prompt_ms"] for r in runs[C] if r["prompt_ms"] != "oom"]
            summary[name] = {"prompt_ms": [r["prompt_ms"] for r in runs[C]], "median_ms": sorted(ms)[len(ms) // 2] if ms else "oom",
                             "spread_ms": round(max(ms) - min(ms), 2) if ms else "oom", "peak_GiB": runs[C][-1]["peak_GiB"],
                             "peak_above_start_GiB": runs[C][-1]["peak_above_start_GiB"]}
            if "needs_GiB" in runs[C][-1]:
                summary[name]["needs_GiB"] = runs[C][-1]["needs_GiB"]
        if a.kv == "fp8":                                                    # share of the staging-slab dequantisation in the chunked prompt pass
            for C in chunks:
                model.set_prefill_chunk(C)
                drop()
                model._generate_step(inputs, pad_token_id=0, max_new_tokens=1, eos_token_id=[], **gen)
                H.kernel_profile_start()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model._generate_step(inputs, pad_token_id=0, max_new_tokens=1, eos_token_id=[], **gen)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                prof = H.kernel_profile_stop()
                dq = prof.get("kv8_dequant", (0, 0.0, 0.0))
                attn = sum(v[2] for k, v in prof.items() if k.startswith("attn_fwd"))
                med = summary[f"chunk{C}"]["median_ms"]
                summary[f"chunk{C}"].update(dequant_calls=dq[0], dequant_ms=round(dq[2], 3), attention_fwd_ms=round(attn, 3), profiled_prompt_ms=round(wall, 2),
                                            dequant_share_of_prompt=round(dq[2] / med, 4) if med != "oom" else None)
        drop()
        summary["weights_GiB"] = round(torch.cuda.memory_allocated() / 2 ** 30, 3)
        print(json.dumps(summary), flush=True)
        return

    full_inputs = inputs

    def first_rows(b):                                                       # the first b rows of the batch with their audios
        keep = [i for i, (r, _) in enumerate(full_inputs["context_batch_start_positions"]) if r < b]
        return {"context_input_ids": full_inputs["context_input_ids"][:b], "context_attention_mask": full_inputs["context_attention_mask"][:b],
                "context_batch_start_positions": [full_inputs["context_batch_start_positions"][i] for i in keep],
                "batch_features": full_inputs["batch_features"][keep], "batch_transcription_ids": [full_inputs["batch_transcription_ids"][i] for i in keep]}

    def leg(kind, rows=None):
        nonlocal B, inputs
        if rows is not None:
            B, inputs = rows, first_rows(rows)
        model.set_decode_weights(kind)
        res = []
        for new in (1, a.new):
            best = None
            for _ in range(a.repeat):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ids = model._generate_step(inputs, pad_token_id=0, max_new_tokens=new, eos_token_id=[], **gen)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            assert ids.shape == (B, new)
            res.append(best)
        prompt_ms = res[0] * 1e3
        tok_ms = (res[1] - res[0]) * 1e3 / (a.new - 1)
        wbytes = welems * 17 // 32 if kind == "mxfp4" else welems * (1 if kind == "fp8" else 2)     # mxfp4: 4 bits + one scale byte per 32
        r = {"workload": f"{a.config} generate B={B} prompt={S} new={a.new} {mode}", "decode_weights": kind, "kv_cache": model.llm.kv_cache_kind, "prefill_chunk": model.llm.prefill_chunk,
             "prompt_ms": round(prompt_ms, 2),
             "ms_per_token_step": round(tok_ms, 3), "tokens_per_s": round(B / tok_ms * 1e3, 1),
             "weight_bytes_per_step": wbytes, "weight_stream_GBps": round(wbytes / tok_ms / 1e6, 1), "hbm_peak_GBps": 8000}
        print(json.dumps(r), flush=True)
        return r

    if a.rows_ab:
        sizes = [int(x) for x in a.rows_ab.split(",")]
        assert max(sizes) <= a.batch, "--batch is the largest size of --rows-ab"
        legs = [(b, kind) for b in sizes for kind in ("bf16", "fp8")]
        for b, kind in legs:                                                 # warm-up: quantise once, every buffer set once
            leg(kind, b)
        runs = {lg: [] for lg in legs}
        for _ in range(a.rounds):
            for lg in legs:
                r = leg(lg[1], lg[0])
                runs[lg].append((r["ms_per_token_step"], r["tokens_per_s"], r["weight_stream_GBps"], r["prompt_ms"]))
        model.set_decode_weights("bf16")
        out = {"rows_ab": f"{a.config} prompt={S} new={a.new} {mode} kv={a.kv}", "rounds": a.rounds, "legs": {}}
        for (b, kind), v in runs.items():
            ms, tps = sorted(x[0] for x in v), sorted(x[1] for x in v)
            out["legs"][f"B{b}_{kind}"] = {"ms_per_step": [x[0] for x in v], "median_ms_per_step": ms[len(ms) // 2], "spread_ms": round(ms[-1] - ms[0], 3),
                                           "tokens_per_s": [x[1] for x in v], "median_tokens_per_s": tps[len(tps) // 2],
                                           "spread_tokens_per_s": round(tps[-1] - tps[0], 1), "median_weight_GBps": sorted(x[2] for x in v)[len(v) // 2],
                                           "median_prompt_ms": sorted(x[3] for x in v)[len(v) // 2]}
        for kind in ("bf16", "fp8"):
            base = out["legs"][f"B{sizes[0]}_{kind}"]
            for b in sizes[1:]:
                lg = out["legs"][f"B{b}_{kind}"]
                lg[f"tokens_per_s_vs_B{sizes[0]}"] = round(lg["median_tokens_per_s"] / base["median_tokens_per_s"], 3)
                lg[f"more_tokens_per_s_than_B{sizes[0]}_beyond_spread"] = bool(
                    min(lg["tokens_per_s"]) - max(base["tokens_per_s"]) > lg["spread_tokens_per_s"] + base["spread_tokens_per_s"])
        print(json.dumps(out), flush=True)
        return
    if a.attn_ab:
        min_keys = H.DECODE_ATTN_MIN_KEYS
        legs = {"split_kv": min_keys, "forward": 1 << 30}
        runs = {k: [] for k in legs}
        try:
            H.DECODE_ATTN_MIN_KEYS = min_keys
            leg(a.weights)                                                   # warm-up
            for _ in range(a.rounds):
                for name, thr in legs.items():
                    H.DECODE_ATTN_MIN_KEYS = thr
                    n0 = H.ATTN_DECODE_CALLS
                    runs[name].append(leg(a.weights)["ms_per_token_step"])
                    assert (H.ATTN_DECODE_CALLS > n0) == (name == "split_kv" and S + a.new >= min_keys)
        finally:
            H.DECODE_ATTN_MIN_KEYS = min_keys
        lo = {k: min(v) for k, v in runs.items()}
        hi = {k: max(v) for k, v in runs.items()}
        med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
        print(json.dumps({"attn_ab": f"{a.config} B={B} prompt={S} new={a.new} {mode} weights={a.weights}", "rounds": a.rounds,
                          "min_keys": min_keys, "chunk": H.DECODE_ATTN_CHUNK,
                          "split_kv_ms_per_step": runs["split_kv"], "forward_ms_per_step": runs["forward"],
                          "tokens_per_s": {k: round(B / med[k] * 1e3, 1) for k in runs},
                          "spread_ms": {k: round(hi[k] - lo[k], 3) for k in runs},
                          "median_speedup": round(med["forward"] / med["split_kv"], 3),
                          "margin_ms_worst_case": round(lo["forward"] - hi["split_kv"], 3),
                          "split_kv_faster_beyond_spread": bool(med["forward"] - med["split_kv"] > sum(hi[k] - lo[k] for k in runs))}))
        return
    if a.kv_ab:
        runs = {"bf16": [], "fp8": []}
        prompt = {"bf16": [], "fp8": []}
        alloc = {}
        for kind in ("bf16", "fp8"):                                         # warm-up; the slabs of a kind are made by its first run
            model.set_kv_cache(kind)
            torch.cuda.synchronize()
            m0 = torch.cuda.memory_allocated()
            model.llm._gen_alloc(B, S + a.new)
            nb = sum(x.numel() * x.element_size() for x in model.llm.kv_cache + (model.llm.kv_scale or []))
            alloc[kind] = {"slab_bytes": nb, "memory_allocated_delta": torch.cuda.memory_allocated() - m0}
            model.llm._gen_shape = None
            leg(a.weights)
        for _ in range(a.rounds):
            for kind in runs:
                model.set_kv_cache(kind)
                n8, n16 = H.ATTN_KV8_CALLS, H.ATTN_DECODE_CALLS
                r = leg(a.weights)
                assert (H.ATTN_KV8_CALLS > n8) == (kind == "fp8") and (kind == "bf16" or H.ATTN_DECODE_CALLS == n16)
                runs[kind].append(r["ms_per_token_step"]), prompt[kind].append(r["prompt_ms"])
        model.set_kv_cache(a.kv)
        lo = {k: min(v) for k, v in runs.items()}
        hi = {k: max(v) for k, v in runs.items()}
        med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
        print(json.dumps({"kv_ab": f"{a.config} B={B} prompt={S} new={a.new} {mode} weights={a.weights}", "rounds": a.rounds,
                          "bf16_ms_per_step": runs["bf16"], "fp8_ms_per_step": runs["fp8"], "prompt_ms": prompt,
                          "spread_ms": {k: round(hi[k] - lo[k], 3) for k in runs},
                          "median_speedup": round(med["bf16"] / med["fp8"], 3),
                          "margin_ms_worst_case": round(lo["bf16"] - hi["fp8"], 3),
                          "fp8_faster_beyond_spread": bool(med["bf16"] - med["fp8"] > sum(hi[k] - lo[k] for k in runs)),
                          "cache_bytes": alloc, "cache_bytes_ratio": round(alloc["fp8"]["slab_bytes"] / alloc["bf16"]["slab_bytes"], 4)}))
        return
    if not a.ab:
        leg(a.weights)
        return
    leg("fp8")                                                               # warm-up: quantise once, touch every path
    leg("mxfp4")
    runs = {"bf16": [], "fp8": [], "mxfp4": []}
    for _ in range(a.rounds):
        for kind in runs:
            model.set_decode_weights(kind)                                   # (the copies another leg freed are re-made outside the timed region)
            if kind == "fp8":
                model.llm._fp8_decode_weights()
            elif kind == "mxfp4":
                model.llm._mxfp4_decode_weights()
            runs[kind].append(leg(kind)["ms_per_token_step"])
    model.set_decode_weights("bf16")
    lo = {k: min(v) for k, v in runs.items()}
    hi = {k: max(v) for k, v in runs.items()}
    med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}

    def faster(x, y):                                                        # x beats y in the worst pairing by more than both spreads
        return bool(lo[y] - hi[x] > (hi[x] - lo[x]) + (hi[y] - lo[y]))
    print(json.dumps({"ab": f"{a.config} B={B} prompt={S} new={a.new} {mode}", "rounds": a.rounds,
                      "bf16_ms_per_step": runs["bf16"], "fp8_ms_per_step": runs["fp8"], "mxfp4_ms_per_step": runs["mxfp4"],
                      "spread_ms": {k: round(hi[k] - lo[k], 3) for k in runs},
                      "tokens_per_s": {k: round(B / med[k] * 1e3, 1) for k in runs},
                      "median_speedup": round(med["bf16"] / med["fp8"], 3),
                      "median_speedup_mxfp4_vs_bf16": round(med["bf16"] / med["mxfp4"], 3),
                      "median_speedup_mxfp4_vs_fp8": round(med["fp8"] / med["mxfp4"], 3),
                      "margin_ms_worst_case": round(lo["bf16"] - hi["fp8"], 3),
                      "margin_ms_worst_case_mxfp4_vs_bf16": round(lo["bf16"] - hi["mxfp4"], 3),
                      "margin_ms_worst_case_mxfp4_vs_fp8": round(lo["fp8"] - hi["mxfp4"], 3),
                      "fp8_faster_beyond_spread": bool(lo["bf16"] - hi["fp8"] > max(hi[k] - lo[k] for k in ("bf16", "fp8"))),
                      "mxfp4_faster_than_bf16_beyond_spread": faster("mxfp4", "bf16"),
                      "mxfp4_faster_than_fp8_beyond_spread": faster("mxfp4", "fp8")}))

if __name__ == "__main__":
    main()
