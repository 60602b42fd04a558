"""Per-call time of the decode-step samplers on [rows, vocab] bf16 logits: today's `sample_top_p_k` (temperature + top-p),
`sample_chain_k` (desta_sample_bf16: top-p only, and the full chain penalty + temperature + top-k + top-p + min-p) and
`sample_greedy_k` (greedy with a repetition penalty), `argmax_bf16` for scale, and `topk_logprob_k` (desta_topk_logprobs, the token's
log-probability + top 5 of generate(logprobs=5)) beside the chain sampler it follows in a decode step.  Device-event timing over `--iters`
back-to-back calls; for kernel times run it under `rocprofv3 --kernel-trace --stats`.

--grouped adds the entry points of a verify step (`sample_rows`, `sample_top_p_rows`) at batch x width = 4, 8, 32 and 64 rows against
the one-row entry points at the same row count (`grouped()` below).

--truncation times the chain with HF's typical-p / epsilon / eta steps (`desta_sample_truncated_rows_bf16`) beside today's chain at
1, 8 and 32 rows (`truncation()`); with --parent-lib PATH it also alternates today's entry points between this build and the library
at PATH (`parent_ab()`), and with --generate CONFIG it reports ms per decode step on a synthetic full-size model (`generate_step()`).

  python tools/sampler_bench.py [--rows 8] [--vocab 128256 151936] [--iters 200] [--hist 256] [--grouped] [--rounds 5]
  python tools/sampler_bench.py --truncation [--parent-lib PATH/libdesta_hip.so] [--generate desta25_llama31-8B_Qformer6L]
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
    ap.add_argument("--truncation", action="store_true", help="time the chain with typical-p / epsilon / eta steps at 1, 8 and 32 rows (and nothing else)")
    ap.add_argument("--parent-lib", default=None, help="--truncation: also A/B today's entry points against this libdesta_hip.so (the parent commit's)")
    ap.add_argument("--generate", default=None, metavar="CONFIG", help="--truncation: also ms per decode step on this synthetic full-size config")
    a = ap.parse_args()
    from desta import _hip as H
    dev = torch.device("cuda:0")
    if a.truncation:
        truncation(H, a, dev)
        if a.parent_lib:
            parent_ab(H, a, dev)
        if a.generate:
            generate_step(a, dev)
        return
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


TRUNCATION_SETTINGS = {
    "full (no truncation)": dict(temperature=0.7, top_k=50, top_p=0.9, min_p=0.05, repetition_penalty=1.2),
    "temperature only (no truncation)": dict(temperature=0.8),
    "typical": dict(temperature=0.8, typical_p=0.9),
    "typical_lo": dict(temperature=1.0, typical_p=0.2),
    "eps": dict(temperature=1.0, epsilon_cutoff=3e-4),
    "eta": dict(temperature=1.0, eta_cutoff=2e-3),
    "tail3": dict(temperature=0.9, typical_p=0.95, epsilon_cutoff=3e-4, eta_cutoff=6e-4),
    "all": dict(temperature=0.7, top_k=50, top_p=0.9, min_p=0.05, repetition_penalty=1.2, typical_p=0.9, epsilon_cutoff=9e-4, eta_cutoff=2e-3),
}


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def truncation(H, a, dev):
    """--truncation: the chain sampler with typical-p / epsilon / eta steps (`desta_sample_truncated_rows_bf16`), each setting alone
    and `all`, beside today's chain, at 1, 8 and 32 rows: median and spread of --rounds rounds, us per launch."""
    g = torch.Generator(device=dev).manual_seed(0)
    for V in a.vocab:
        ld = (V + 63) // 64 * 64
        for B in (1, 8, 32):
            logits = (torch.randn(B, ld, device=dev, generator=g) * 3).to(torch.bfloat16)
            hist = torch.randint(0, V, (B, a.hist), device=dev, generator=g)
            out = torch.zeros(B, dtype=torch.int64, device=dev)
            fns = {}
            for name, s in TRUNCATION_SETTINGS.items():
                kw = dict(s, seed=1, **(dict(hist=hist, hist_len=a.hist) if "repetition_penalty" in s else {}))
                fns[name] = (lambda kw=kw: H.sample(logits, ld, B, V, out, **kw))
            runs = {k: [] for k in fns}
            for fn in fns.values():
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    runs[k].append(_timed(fn, a.iters))
            for k, v in runs.items():
                print(json.dumps({"truncation": k, "shape": [B, V], "median_us": round(sorted(v)[len(v) // 2], 2), "spread_us": round(max(v) - min(v), 2)}),
                      flush=True)


def parent_ab(H, a, dev):
    """--parent-lib PATH: today's entry points (`desta_sample_bf16`: top-p only and the full chain; `desta_sample_rows_bf16`: the full
    chain over 8 x 4 rows) through this build and through the library at PATH (the parent commit's), alternating in one process
    for --rounds rounds.  Reports medians, spreads (max - min over the rounds) and whether the difference of the medians lies
    inside the two spreads."""
    import ctypes as C
    old = C.CDLL(os.path.abspath(a.parent_lib))
    assert not hasattr(old, "desta_sample_truncated_rows_bf16"), "--parent-lib: that library already has the truncated entry point"
    one_old, rows_old = old.desta_sample_bf16, old.desta_sample_rows_bf16
    one_old.argtypes, one_old.restype = H._sample_chain.argtypes, C.c_int
    rows_old.argtypes, rows_old.restype = H._sample_rows.argtypes, C.c_int
    g = torch.Generator(device=dev).manual_seed(0)
    p, st = H.p, H.stream
    for V in a.vocab:
        ld = (V + 63) // 64 * 64
        for B in (1, 8, 32):
            logits = (torch.randn(B, ld, device=dev, generator=g) * 3).to(torch.bfloat16)
            hist = torch.randint(0, V, (B, a.hist), device=dev, generator=g)
            width = min(B, 4)
            tail = torch.randint(0, V, (B // width, width), device=dev, generator=g)
            outs = [torch.zeros(B, dtype=torch.int64, device=dev) for _ in range(2)]

            def one(fn, o, full):
                return lambda: fn(p(logits), ld, B, V, p(hist) if full else None, hist.stride(0) if full else 0, a.hist if full else 0,
                                  1.2 if full else 1.0, 1, 0.7, 50 if full else 0, 0.9, 0.05 if full else 0.0, 1, 0, p(o), None, st())

            def rows(fn, o):
                return lambda: fn(p(logits), ld, B // width, width, V, p(hist), hist.stride(0), a.hist, p(tail), tail.stride(0), 1.2, 1, 0.7, 50,
                                  0.9, 0.05, 1, 0, p(o), None, st())
            pairs = {"sample chain top_p": (one(H._sample_chain, outs[0], False), one(one_old, outs[1], False)),
                     "sample chain full": (one(H._sample_chain, outs[0], True), one(one_old, outs[1], True)),
                     f"sample_rows chain full {B // width}x{width}": (rows(H._sample_rows, outs[0]), rows(rows_old, outs[1]))}
            for name, (new_fn, old_fn) in pairs.items():
                for fn in (new_fn, old_fn):
                    for _ in range(10):
                        assert fn() == 0
                torch.cuda.synchronize()
                assert torch.equal(outs[0], outs[1]), name                          # the same picks from both libraries
                tn, to = [], []
                for _ in range(a.rounds):
                    tn.append(_timed(new_fn, a.iters))
                    to.append(_timed(old_fn, a.iters))
                mn, mo = sorted(tn)[len(tn) // 2], sorted(to)[len(to) // 2]
                sn, so = max(tn) - min(tn), max(to) - min(to)
                print(json.dumps({"ab": name, "shape": [B, V], "rounds": a.rounds, "this_us": round(mn, 2), "this_spread": round(sn, 2),
                                  "parent_us": round(mo, 2), "parent_spread": round(so, 2), "this_minus_parent_us": round(mn - mo, 2),
                                  "within_spreads": bool(abs(mn - mo) <= sn + so)}), flush=True)


def generate_step(a, dev):
    """--generate CONFIG: ms per decode step of `_generate_step` on a full-size synthetic model (text prompt of 64 tokens, 33 new
    tokens minus 1, best of 3, --rounds alternations) at B = 1 / 8 / 32: top-p sampling, today's full chain, and the full chain
    with all three truncation steps.  Reported, not gated; synthetic weights, so nothing here speaks about answer quality."""
    import statistics
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    from desta.synthetic import FULL_CONFIGS, RandomWeights
    cfg = DeSTA25Config(**FULL_CONFIGS[a.generate])
    model = DeSTA25AudioModel(cfg, weights=RandomWeights(cfg, dev, seed=0), device=dev).eval()
    V, new = cfg.llm_config.vocab_size, 33
    full = dict(temperature=0.7, top_k=50, top_p=0.9, min_p=0.05, repetition_penalty=1.2)
    legs = {"top_p": dict(temperature=0.7, top_p=0.9), "chain full": full,
            "chain full + typical/eps/eta": dict(full, typical_p=0.9, epsilon_cutoff=9e-4, eta_cutoff=2e-3)}

    def step_ms(inp, kw):
        res = []
        for n in (1, new):
            best = None
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                model._generate_step(inp, pad_token_id=0, max_new_tokens=n, do_sample=True, eos_token_id=[], seed=1, **kw)
                e1.record()
                e1.synchronize()
                dt = e0.elapsed_time(e1)
                best = dt if best is None else min(best, dt)
            res.append(best)
        return (res[1] - res[0]) / (new - 1)

    for B in (1, 8, 32):
        ids = torch.randint(3, V, (B, 64), generator=torch.Generator().manual_seed(5 + B))
        inp = {"context_input_ids": ids, "context_attention_mask": torch.ones_like(ids), "context_batch_start_positions": [],
               "batch_features": None, "batch_transcription_ids": []}
        for kw in legs.values():
            step_ms(inp, kw)
        runs = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, kw in legs.items():
                runs[k].append(round(step_ms(inp, kw), 4))
        med = {k: statistics.median(v) for k, v in runs.items()}
        print(json.dumps({"generate": f"{a.generate} B={B} prompt=64 new={new} do_sample", "rounds": a.rounds, "median_ms_per_step": med,
                          "spread_ms": {k: round(max(v) - min(v), 4) for k, v in runs.items()},
                          "truncation_minus_full_us": round((med["chain full + typical/eps/eta"] - med["chain full"]) * 1e3, 1)}), flush=True)


if __name__ == "__main__":
    main()
