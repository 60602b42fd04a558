"""What the hard constraints of generate() (`no_repeat_ngram_size`, `bad_words_ids`, `suppress_tokens`, `begin_suppress_tokens`,
`min_new_tokens`; `desta_logit_constraints_bf16`) cost, on one GPU.

(a) The kernel, in place and out of place, beside `desta_cfg_scores_bf16` on the same rows as a yardstick: rows x vocab bf16
scores, a history of --hist tokens per row over a 64-token alphabet (so the n-gram scan finds matches), n = --ngram, --words bad
words of two or three tokens, two begin ids and two EOS ids under min_new_tokens.  One HIP-event pair per launch, the cases
alternating, median / min / max over --iters launches after a warm-up.  The buffers are the same in every launch, so they come
from the caches, as the logits of a decode step do (the lm_head has just written them).  In place the kernel stores the banned
entries only; out of place it copies the row (4 bytes per column).

(b) ms per decode step on a full-size LLM with synthetic weights (--config, Llama-3.1-8B geometry by default), text-only prompts
of --prompt tokens: the constrained greedy loop (n-gram + bad words + suppress + min_new_tokens, in place) against the plain
greedy loop of the same build, the legs alternating (--rounds alternations after a warm-up of both).  ms per step = (HIP-event
time of --new tokens - time of 1 token) / (--new - 1), best of --repeat, so the prompt pass drops out.  --parent DIR adds the
plain loop of another checkout (the parent commit, built in DIR) as a third leg: once per round a fresh child process runs this
file against DIR's package, in front of this build's legs, and reports the same figure.

  python tools/constraints_bench.py [--vocab 128256 151936] [--rows 1 8 32] [--hist 0 512 2048] [--iters 30] [--no-kernel]
                                    [--config desta25_llama31-8B_Qformer6L] [--batch 1 8 32] [--new 33] [--rounds 3] [--parent DIR]
                                    [--no-generate]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = "desta2.5-audio_amd"


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, nargs="+", default=[128256, 151936])
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--hist", type=int, nargs="+", default=[0, 512, 2048])
    ap.add_argument("--ngram", type=int, default=3)
    ap.add_argument("--words", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--config", default="desta25_llama31-8B_Qformer6L")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--new", type=int, default=33)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None, help="another checkout of the repository, built: its plain loop becomes a third leg")
    ap.add_argument("--no-generate", action="store_true")
    ap.add_argument("--plain-only", default=None, metavar="PKG_DIR", help="(child of --parent) time the plain loop of the package in PKG_DIR, print one JSON line")
    return ap.parse_args()


a = _args() if __name__ == "__main__" else None
sys.path.insert(0, a.plain_only if a is not None and a.plain_only else os.path.join(HERE, "..", PKG))
import torch  # noqa: E402


def kernel_leg(a):
    from desta import _hip as H
    from desta.models.modeling_desta25 import ConstraintPlan
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    cg = torch.Generator().manual_seed(1)
    for V in a.vocab:
        ld = (V + 63) // 64 * 64
        words = [torch.randint(0, 64, (2 + i % 2,), generator=cg).tolist() for i in range(a.words)]
        plan = ConstraintPlan(dev, [V - 1, V - 2], no_repeat_ngram_size=a.ngram, bad_words_ids=words or None, begin_suppress_tokens=[5, 6],
                              min_new_tokens=4)
        for rows in a.rows:
            x = (torch.randn(2 * rows, ld, device=dev, generator=g) * 3).to(torch.bfloat16)
            y = x[:rows].clone()
            out = torch.zeros(rows, ld, dtype=torch.bfloat16, device=dev)
            for hist_len in a.hist:
                hist = torch.randint(0, 64, (rows, max(hist_len, 1)), device=dev, generator=g)
                cases = {"constraints(in place)": lambda: plan.apply(y, ld, y, ld, rows, 1, V, hist, hist_len, step0=1),
                         "constraints(out of place)": lambda: plan.apply(x, ld, out, ld, rows, 1, V, hist, hist_len, step0=1),
                         "cfg_scores": lambda: H.cfg_scores(x[:rows], x[rows:], ld, rows, V, 3.0, out, ld)}
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
                banned = int(torch.isinf(y[:, :V]).sum())
                for name, ts in times.items():
                    print(json.dumps({"kernel": name, "rows": rows, "vocab": V, "hist_len": hist_len, "ngram": a.ngram, "words": a.words,
                                      "us_median": round(statistics.median(ts), 1), "us_min": round(min(ts), 1), "us_max": round(max(ts), 1),
                                      "launches": len(ts), "banned_entries": banned}), flush=True)


def _model(a):
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    from desta.synthetic import FULL_CONFIGS, RandomWeights
    dev = torch.device("cuda:0")
    cfg = DeSTA25Config(**FULL_CONFIGS[a.config])
    return DeSTA25AudioModel(cfg, weights=RandomWeights(cfg, dev, seed=0), device=dev).eval(), cfg.llm_config.vocab_size


def _inputs(a, V, rows):
    ids = torch.randint(3, V, (rows, a.prompt), generator=torch.Generator().manual_seed(5 + rows))
    return {"context_input_ids": ids, "context_attention_mask": torch.ones_like(ids), "context_batch_start_positions": [],
            "batch_features": None, "batch_transcription_ids": []}


def _step_ms(a, model, inp, **kw):
    res = []
    for new in (1, a.new):
        best = None
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            model._generate_step(inp, pad_token_id=0, max_new_tokens=new, do_sample=False, **kw)
            e1.record()
            e1.synchronize()
            dt = e0.elapsed_time(e1)
            best = dt if best is None else min(best, dt)
        res.append(best)
    return (res[1] - res[0]) / (a.new - 1)


def plain_only(a):
    """The child of --parent: the plain greedy loop of the package this process imported, every --batch once after a warm-up."""
    model, V = _model(a)
    out = {}
    for B in a.batch:
        inp = _inputs(a, V, B)
        _step_ms(a, model, inp, eos_token_id=[])
        out[str(B)] = round(_step_ms(a, model, inp, eos_token_id=[]), 4)
    print("PLAIN_ONLY " + json.dumps(out), flush=True)


def _parent_round(a):
    pkg = os.path.join(os.path.abspath(a.parent), PKG)
    cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", pkg, "--config", a.config, "--prompt", str(a.prompt), "--new", str(a.new),
           "--repeat", str(a.repeat), "--batch", *[str(b) for b in a.batch]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)             # a fresh process: it opens the GPU itself
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("PLAIN_ONLY ")), None)
    if r.returncode != 0 or line is None:
        sys.exit(f"constraints_bench: the --parent leg failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(line[len("PLAIN_ONLY "):])


def generate_leg(a):
    from desta import _hip as H
    model, V = _model(a)
    cg = torch.Generator().manual_seed(1)
    words = [torch.randint(3, V, (2 + i % 2,), generator=cg).tolist() for i in range(a.words)]
    eos = [V - 1]
    con = dict(no_repeat_ngram_size=a.ngram, bad_words_ids=words, suppress_tokens=[5, 6, 7], min_new_tokens=a.new + 1, eos_token_id=eos)
    legs = {"constrained": con, "plain": dict(eos_token_id=[])}
    inputs = {B: _inputs(a, V, B) for B in a.batch}
    for B in a.batch:                                                                  # warm-up of every leg
        for kw in legs.values():
            _step_ms(a, model, inputs[B], **kw)
    runs = {B: {k: [] for k in list(legs) + (["plain(parent)"] if a.parent else [])} for B in a.batch}
    for _ in range(a.rounds):
        if a.parent:
            for B, ms in _parent_round(a).items():
                runs[int(B)]["plain(parent)"].append(ms)
        for B in a.batch:
            for k, kw in legs.items():
                c0 = H.CONSTRAINT_CALLS
                runs[B][k].append(round(_step_ms(a, model, inputs[B], **kw), 4))
                assert H.CONSTRAINT_CALLS - c0 == (a.repeat * (1 + a.new) if k == "constrained" else 0)
    for B in a.batch:
        med = {k: statistics.median(v) for k, v in runs[B].items()}
        line = {"generate": f"{a.config} B={B} prompt={a.prompt} new={a.new} greedy n={a.ngram} words={a.words}", "rounds": a.rounds,
                "ms_per_step": runs[B], "median_ms_per_step": med, "spread_ms": {k: round(max(v) - min(v), 4) for k, v in runs[B].items()},
                "constrained_minus_plain_us": round((med["constrained"] - med["plain"]) * 1e3, 1),
                "constrained_over_plain": round(med["constrained"] / med["plain"], 4)}
        if a.parent:
            line["plain_over_plain_parent"] = round(med["plain"] / med["plain(parent)"], 4)
        print(json.dumps(line), flush=True)


def main():
    if not torch.cuda.is_available():
        sys.exit("constraints_bench: needs the GPU (no timing without one)")
    if a.plain_only:
        return plain_only(a)
    if not a.no_kernel:
        kernel_leg(a)
    if not a.no_generate:
        generate_leg(a)


if __name__ == "__main__":
    main()
