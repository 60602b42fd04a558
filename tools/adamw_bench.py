"""Fused clip + AdamW on the real connector arena (131.54 M fp32): HIP-event time per call, cold (Infinity Cache flushed) and
warm, and the byte rates: algorithmic 8 words per element (g read twice; p, m, v read and written) = 32 N bytes.
  python tools/adamw_bench.py [--iters 50]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "desta2.5-audio_amd"))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    from desta.models.modeling_desta25 import DeSTA25Config, connector_param_shapes
    from desta.optim import FusedAdamW, ParamArena
    from desta.synthetic import FULL_CONFIGS
    cfg = DeSTA25Config(**FULL_CONFIGS["desta25_llama31-8B_Qformer6L"])
    arena = ParamArena(list(connector_param_shapes(cfg).items()), "cuda")
    arena.params.normal_(0, 0.02)
    opt = FusedAdamW(arena, weight_decay=0.01, betas=(0.9, 0.98))
    N = arena.numel
    flush = torch.empty(1 << 28, dtype=torch.float32, device="cuda")      # 1 GiB: evicts the Infinity Cache between calls
    times = {"cold": [], "warm": []}
    for mode in ("cold", "warm"):
        for i in range(a.iters):
            arena.grads.normal_(0, 1e-3 * (1 + i % 3))
            if mode == "cold":
                flush.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.step(1e-4)
            e1.record()
            torch.cuda.synchronize()
            times[mode].append(e0.elapsed_time(e1))
    print(f"arena N = {N / 1e6:.2f} M floats ({arena.true_numel() / 1e6:.2f} M trainable), {opt.plan.n_items} work items, "
          f"grad norm of the last call {float(opt.grad_norm()):.4f}")
    for mode, ts in times.items():
        ts = sorted(ts[5:])
        med = ts[len(ts) // 2]
        print(f"{mode}: median {1e3 * med:.0f} us (min {1e3 * ts[0]:.0f}, max {1e3 * ts[-1]:.0f}) over {len(ts)} calls | "
              f"algorithmic 32 N = {32 * N / 1e9:.3f} GB -> {32 * N / med / 1e6:.0f} GB/s ({32 * N / med / 1e6 / 8000:.3f} of 8 TB/s)")


if __name__ == "__main__":
    main()
