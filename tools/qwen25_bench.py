"""Qwen2.5-7B geometry (q|k|v projection bias, rotary kernel adds it) next to Qwen3-8B (q/k-norm in the same kernel) in ONE
process on one MI355X, synthetic weights: ms per training step and ms per KV-cached decode step at B = 1, 8, 64 with bf16 and
FP8 decode weights.  One model at a time (the first is freed before the second is built).

  python tools/qwen25_bench.py [--configs qwen2.5-7B,desta25_qwen3-8B_Qformer6L] [--batch 8] [--ctx 64] [--tgt 512]
                               [--steps 5] [--warmup 3] [--rounds 3] [--new 32] [--decode-batches 1,8,64] [--skip-train]
One JSON line per figure: median and spread (max - min) over `rounds`.  Training: `DeSTA25Trainer.training_step` on two
alternating synthetic batches, `steps` steps per round (bench.py's workload; bench.py stays the yardstick for the flagship).
Decode: (time of 1 + new tokens - time of 1 token) / new, greedy, prompt = ctx + audio tokens + 16."""
import argparse
import gc
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch  # noqa: E402


def _stat(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "spread": round(v[-1] - v[0], 3), "values": [round(x, 3) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="qwen2.5-7B,desta25_qwen3-8B_Qformer6L")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ctx", type=int, default=64)
    ap.add_argument("--tgt", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=32)
    ap.add_argument("--decode-batches", default="1,8,64")
    ap.add_argument("--skip-train", action="store_true")
    a = ap.parse_args()
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    from desta.synthetic import FULL_CONFIGS, RandomWeights, synthetic_inputs, synthetic_waveform
    from desta.trainer.desta_trainer import DeSTA25Trainer, TrainingArguments
    dev = torch.device("cuda:0")
    for name in a.configs.split(","):
        cfg = DeSTA25Config(**FULL_CONFIGS[name])
        c = cfg.llm_config
        model = DeSTA25AudioModel(cfg, weights=RandomWeights(cfg, dev, seed=0), device=dev)
        tag = {"config": name, "model_type": c.model_type, "attention_bias": c.attention_bias, "qk_norm": c.qk_norm}
        n_mels = cfg.encoder_config.num_mel_bins
        if not a.skip_train:
            B = a.batch
            trainer = DeSTA25Trainer(model, args=TrainingArguments(learning_rate=1e-4, weight_decay=0.01, warmup_steps=5000, max_steps=10 ** 6,
                                                                  logging_steps=10 ** 9))
            waves = [synthetic_waveform(B, dev, seed=1234 + 97 * i) for i in range(2)]
            toks = [synthetic_inputs(cfg, B, a.ctx, a.tgt, dev, seed=1234 + 97 * i) for i in range(2)]

            def step(i):
                b = dict(toks[i % 2])
                b["batch_features"] = H.logmel(waves[i % 2], n_mels)
                return trainer.training_step(b)
            for i in range(a.warmup):
                step(i)
            ms = []
            for _ in range(a.rounds):
                trainer.wait_update()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(a.steps):
                    step(i)
                trainer.wait_update()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
            print(json.dumps({**tag, "figure": "train_ms_per_step", "B": B, "S": a.ctx + cfg.audio_tokens + a.tgt, "rope_fused": bool(model.llm._rope_fused),
                              **_stat(ms)}), flush=True)
            del trainer, waves, toks
            for n in ("xs", "sv", "rf", "hb", "hbc", "act", "logits", "dxa", "dxb", "dgu", "dqkv", "datt"):   # the training save set
                setattr(model.llm, n, None)
            model.llm.B = model.llm.S = 0
            gc.collect()
            torch.cuda.empty_cache()
        model.eval()
        for B in (int(x) for x in a.decode_batches.split(",")):
            t = synthetic_inputs(cfg, B, a.ctx, 16, dev, seed=5)
            mel = H.logmel(synthetic_waveform(B, dev, seed=6), n_mels)
            inputs = {"context_input_ids": t["input_ids"], "context_attention_mask": t["attention_mask"],
                      "context_batch_start_positions": t["batch_start_positions"], "batch_features": mel,
                      "batch_transcription_ids": t["batch_transcription_ids"]}

            def gen(n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model._generate_step(inputs, pad_token_id=0, max_new_tokens=n, do_sample=False, eos_token_id=[])
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3
            for weights in ("bf16", "fp8"):
                model.set_decode_weights(weights)
                gen(1 + a.new)                                               # allocations, the FP8 copies
                ms = [(gen(1 + a.new) - gen(1)) / a.new for _ in range(a.rounds)]
                print(json.dumps({**tag, "figure": "decode_ms_per_step", "B": B, "prompt": int(t["input_ids"].shape[1]), "new": a.new, "weights": weights,
                                  **_stat(ms)}), flush=True)
            model.set_decode_weights("bf16")
        del model
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
