"""sha256 digests of everything generate() writes, for the tree this file sits in and the library named by DESTA_HIP_LIB (default: the
in-tree build).  The host side of the KV-cached decode path (`CausalLMHIP.decode_step`, `verify_step`, `prefill`, the two decode
loops) chooses kernels, weight forms, buffers and descriptors; a change there that is meant to keep behaviour is checked by
running this file in a checkout of the commit before the change (copied in) and in the new tree, against the same library: every
line must be equal.  One line per case over the raw bytes of the emitted tokens, the per-step logits, every layer's cache slab
(and its scales under the FP8 cache) over slots [0, S + emitted - 1), `spec_stats`, and the `TokenLogprobs` fields where asked for.
Tiny models and prompts of tests/test_gpu_speculative.py (`_model(False)` / `_model(True)`, S = 61 and 251 with their PADS, 12 new
tokens, no EOS):
  * plain greedy: decode weights {bf16, fp8} x KV cache {bf16, fp8} x prefill chunk {None, 128};
  * one case each: the sampling chain (top_k, min_p, repetition penalty, fixed seed), logprobs = 4, forced tokens;
  * a batch of 20 rows (S = 20): the wide projections;
  * the ORCA-hybrid model of tests/test_gpu_speculative.py::test_orca_model_falls_back (a `layer_hook`) and the LoRA model of
    tests/test_gpu_lora.py (merged q|k|v weights);
  * speculative: k in {3, 7} x drafts {none (all -1), perfect (the plain run's tokens), lookup} x decode weights {bf16, fp8};
  * `verify_step` called directly after a prompt pass, per k, on the plain run's tokens: its logits and the cache over [0, S + k];
  * speculative under scope "all" (`spec-all` lines, printed only by a tree whose `set_speculative` has the argument): {top-p,
    chain, chain + penalty, greedy + penalty, logprobs} x k in {3, 7} x drafts {none, perfect (the plain loop's tokens under the same
    settings), lookup}.
Apart from the `spec-all` lines only entry points that both trees have are used.
  python tools/generate_bits.py"""
import copy
import hashlib
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("desta2.5-audio_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
import desta_oracle as O
import test_gpu_lora as TL
from helpers import cfg_from_dims
from test_gpu_kv8_cache import _text_inputs
from test_gpu_prefill_chunk import PADS, _model

T = 12
SCOPE_ALL_CASES = (("top_p", dict(do_sample=True, temperature=0.8, top_p=0.9, seed=3)),
                   ("chain", dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=40, min_p=0.02, seed=3)),
                   ("penalty", dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=40, min_p=0.02, repetition_penalty=1.3, seed=3)),
                   ("greedy+penalty", dict(repetition_penalty=1.3)),
                   ("logprobs", dict(logprobs=4)))


def sha(*items):
    h = hashlib.sha256()
    for t in items:
        if torch.is_tensor(t):
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
        elif t is not None:
            h.update(repr(t).encode())
    return h.hexdigest()


def digest(model, S, res):
    """Everything a `_generate_step` call left behind: its result (ids[, logits][, TokenLogprobs]) and the cache it filled."""
    llm = model.llm
    res = res if isinstance(res, tuple) else (res,)
    parts = []
    for r in res:
        parts += [r] if torch.is_tensor(r) else [r.token_logprobs, r.top_ids, r.top_logprobs]
    n = S + res[0].shape[1] - 1                                              # the last emitted token was never appended
    parts += [c[:, :n] for c in llm.kv_cache]
    if llm.kv_scale is not None:
        parts += [s[:, :n] for s in llm.kv_scale]
    torch.cuda.synchronize()
    return sha(*parts, sorted(llm.spec_stats.items()))


def gen(model, inputs, n=T, **kw):
    a = dict(pad_token_id=0, max_new_tokens=n, do_sample=False, collect_logits=True, eos_token_id=[])
    a.update(kw)
    return model._generate_step(inputs, **a)


def tiny_cases(g4):
    d, w, model = _model(g4)
    G = d.llm_hq // d.llm_hkv
    llm = model.llm
    for S in (61, 251):
        inputs = _text_inputs(d, S, PADS[S], seed=S)[2]
        tag = f"G {G} S {S:3d}"
        plain = {}
        for weights in ("bf16", "fp8"):
            model.set_decode_weights(weights)
            for kv in ("bf16", "fp8"):
                model.set_kv_cache(kv)
                for chunk in (None, 128):
                    model.set_prefill_chunk(chunk)
                    res = gen(model, inputs)
                    if kv == "bf16" and chunk is None:
                        plain[weights] = res[0].clone()
                    print(f"plain    {tag} weights {weights:4s} kv {kv:4s} chunk {chunk!s:4s}  {digest(model, S, res)}", flush=True)
            model.set_kv_cache("bf16")
            model.set_prefill_chunk(None)
            for k in (3, 7):
                model.set_speculative(k)
                for name, dr in (("none", torch.full_like(plain[weights], -1)), ("perfect", plain[weights]), ("lookup", None)):
                    res = gen(model, inputs, draft_tokens=dr)
                    print(f"spec     {tag} weights {weights:4s} k {k} drafts {name:7s}  {digest(model, S, res)}", flush=True)
                model.set_speculative(None)
                # `verify_step` directly, as tests/test_gpu_speculative.py::test_verify_step_vs_single_steps calls it: a prompt pass
                # (and one step) first, then the chunk of the plain run's first k + 1 tokens at slots [S, S + k]
                gen(model, inputs, n=k + 2, forced_tokens=plain[weights][:, :k + 2])
                kv_start = torch.tensor(PADS[S], dtype=torch.int32, device="cuda")
                vl = llm.verify_step(plain[weights][:, :k + 1].cuda(), S, kv_start)
                torch.cuda.synchronize()
                print(f"verify   {tag} weights {weights:4s} k {k}  {sha(vl, *[c[:, :S + k + 1] for c in llm.kv_cache])}", flush=True)
        model.set_decode_weights("bf16")
        if "scope" in inspect.signature(model.set_speculative).parameters:  # a tree without the scope argument prints the lines above only
            for name, kw in SCOPE_ALL_CASES:
                own = gen(model, inputs, **kw)[0].clone()                    # the plain loop's tokens under these settings: the perfect drafts
                for k in (3, 7):
                    model.set_speculative(k, scope="all")
                    for src, dr in (("none", torch.full_like(own, -1)), ("perfect", own), ("lookup", None)):
                        res = gen(model, inputs, draft_tokens=dr, **kw)
                        print(f"spec-all {tag} {name:14s} k {k} drafts {src:7s}  {digest(model, S, res)}", flush=True)
                    model.set_speculative(None)
        if g4 or S != 61:
            continue
        forced = (plain["bf16"] + 1) % d.vocab                               # never the model's own pick
        for name, kw in (("chain", dict(do_sample=True, temperature=0.8, top_p=0.9, top_k=40, min_p=0.02, repetition_penalty=1.3, seed=3)),
                         ("logprobs", dict(logprobs=4)), ("forced", dict(forced_tokens=forced))):
            print(f"{name:8s} {tag}  {digest(model, S, gen(model, inputs, **kw))}", flush=True)
        wide = _text_inputs(d, 20, [i % 7 for i in range(20)], seed=5)[2]
        for weights in ("bf16", "fp8"):
            model.set_decode_weights(weights)
            print(f"wide     G {G} S  20 B 20 weights {weights:4s}  {digest(model, 20, gen(model, wide))}", flush=True)
        model.set_decode_weights("bf16")


def orca_case():
    import orca_oracle as RO
    from safetensors.torch import load_file
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    g = load_file(os.path.join(ROOT, "tests", "golden", "ref_orca_tiny.safetensors"))
    kg, ds, ks, ntr = (int(x) for x in g["orca_dims"])
    d = copy.copy(O.tiny_dims(True))
    d.prompt_size = kg + ntr
    o = RO.OrcaDims(global_num_tokens=kg, local_downsample=ds, local_kernel_size=ks, ortho_diversity_weight=0.05,
                    ortho_weight_qformer_local=0.05, align_weight_local=0.05, global_cross_attn=False, local_enabled=True)
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=ds,
                        orca_local_kernel_size=ks, orca_ortho_diversity_weight=0.05, orca_ortho_weight_qformer_local=0.05,
                        orca_align_weight_local=0.05, orca_rope_theta=float(g["rope_theta_used"]), orca_global_cross_attn=False, orca_local_enabled=True)
    n_ctx, n = int(g["gen_ctx_len"]), g["starts"].shape[0]
    inputs = {"context_input_ids": g["input_ids"][:, :n_ctx], "context_attention_mask": g["attention_mask"][:, :n_ctx],
              "context_batch_start_positions": [(int(b), int(p)) for b, p in g["starts"].tolist()], "batch_features": g["batch_features"],
              "batch_transcription_ids": [g["transcription_ids"][i:i + 1] for i in range(n)]}
    model = DeSTA25AudioModel(cfg, weights=RO.init_weights(d, o, seed=7)).eval()
    for kv in ("bf16", "fp8"):
        model.set_kv_cache(kv)
        print(f"orca     kv {kv:4s}  {digest(model, n_ctx, gen(model, inputs, n=6))}", flush=True)


def lora_case():
    d = TL._dims()
    model, w = TL._model(d, dropout=0.1)
    model.eval()
    batch = O.synthetic_batch(d, B=2, S_ctx=8, S_tgt=10, seed=2, pad=[2, 0])
    n_ctx = batch["input_ids"].shape[1] - 10 + 3
    ctx = {"context_input_ids": batch["input_ids"][:, :n_ctx], "context_attention_mask": batch["attention_mask"][:, :n_ctx],
           "batch_features": batch["batch_features"], "batch_transcription_ids": batch["batch_transcription_ids"],
           "context_batch_start_positions": batch["batch_start_positions"]}
    for weights in ("bf16", "fp8"):
        model.set_decode_weights(weights)
        print(f"lora     weights {weights:4s}  {digest(model, n_ctx, gen(model, ctx, n=6))}", flush=True)


def main():
    with torch.no_grad():
        tiny_cases(False)
        tiny_cases(True)
        orca_case()
        lora_case()


if __name__ == "__main__":
    main()
