"""GPU: Qwen2 / Qwen2.5 decoders (q|k|v projection bias) against transformers' `Qwen2ForCausalLM` in fp32 on the CPU.

Two tiny directories as `save_pretrained` writes them (hidden 256, 2 layers, I 256, V 320): heads 7 / 1 x 128 (Qwen2.5-7B's group
of 7, hidden != heads x head_dim) and heads 4 / 2 x 64.  transformers initialises the biases to zero, which today's bias-free
code would pass; they are overwritten with N(0, 1) plus +-30 outliers in k_proj (what real Qwen2.5 k-biases look like) before
saving.  The reference gets `position_ids = index - left pad` explicitly.  The oracle knows no bias and is not involved.

Bounds.  Training: those of tests/test_gpu_model.py::test_local_hf_checkpoint_directories_* (|d loss| < 2e-2, relative L2 of the
logits < 3e-2 over the attended positions), the same relative L2 for dL/d inputs_embeds.  Decode: per-step relative L2 <= 3e-2
and argmax gap / spread <= 0.1, the decode path's bounds of DESIGN §3.  Everything else is bit equality."""
import json
import os

import pytest
import torch

from helpers import rel_err

pytestmark = pytest.mark.gpu

H_, L_, I_, V_ = 256, 2, 256, 320
GEOM = {"g7": (7, 1, 128), "g4": (4, 2, 64)}
THETA = 10000.0
T_NEW = 12
S_PROMPT = 21                                                                 # two chunks under set_prefill_chunk(16)
_DIRS, _MODELS, _HF, _DECODE_REF = {}, {}, {}, {}


def _root(tmp_path_factory):
    if "root" not in _DIRS:
        from transformers import WhisperConfig, WhisperForConditionalGeneration
        import desta_oracle as O
        d = O.tiny_dims(False)
        root = tmp_path_factory.mktemp("qwen2")
        wcfg = WhisperConfig(num_mel_bins=d.n_mels, d_model=d.enc_d, encoder_layers=d.enc_layers, encoder_attention_heads=d.enc_heads,
                             encoder_ffn_dim=d.enc_ffn, max_source_positions=d.enc_T, decoder_layers=1, decoder_attention_heads=2, decoder_ffn_dim=64,
                             vocab_size=64, max_target_positions=8, pad_token_id=0, bos_token_id=1, eos_token_id=2, decoder_start_token_id=1)
        torch.manual_seed(1)
        WhisperForConditionalGeneration(wcfg).save_pretrained(root / "enc", safe_serialization=True)
        _DIRS["root"], _DIRS["dims"] = root, d
    return _DIRS["root"]


def _llm_dir(tmp_path_factory, name):
    """name = geometry, optionally + "-zero" (biases left at zero) or + "-zero-llama" (the SAME tensors without the biases, as a Llama
    directory) or + "-snap" (linear weights on the e4m3 grid)."""
    root = _root(tmp_path_factory)
    if name in _DIRS:
        return _DIRS[name]
    from transformers import Qwen2Config, Qwen2ForCausalLM
    geom = name.split("-")[0]
    hq, hkv, hd = GEOM[geom]
    kw = dict(hidden_size=H_, num_hidden_layers=L_, num_attention_heads=hq, num_key_value_heads=hkv, head_dim=hd, intermediate_size=I_,
              vocab_size=V_, rms_norm_eps=1e-6, rope_theta=THETA, tie_word_embeddings=False, max_position_embeddings=512)
    torch.manual_seed(11 + hq)
    llm = Qwen2ForCausalLM(Qwen2Config(**kw, use_sliding_window=False))
    g = torch.Generator().manual_seed(5 + hq)
    with torch.no_grad():
        for layer in llm.model.layers:
            a = layer.self_attn
            assert a.q_proj.bias is not None and a.o_proj.bias is None and float(a.k_proj.bias.abs().max()) == 0.0
            if "-zero" not in name:
                for proj in (a.q_proj, a.k_proj, a.v_proj):
                    proj.bias.copy_(torch.randn(proj.bias.shape, generator=g))
                idx = torch.randperm(hkv * hd, generator=g)[:4]
                a.k_proj.bias[idx] = torch.tensor([30.0, -30.0, 30.0, -30.0])
    llm = llm.to(torch.bfloat16)
    if name.endswith("-snap"):
        from test_gpu_fp8_decode import dequant_bf16, quantize_ref
        with torch.no_grad():
            for n, p in llm.named_parameters():
                if n.endswith("proj.weight") or n == "lm_head.weight":
                    p.copy_(dequant_bf16(*quantize_ref(p.data)))
    path = root / name
    if name.endswith("-llama"):
        # (written by hand: transformers' LlamaConfig refuses a hidden size that is no multiple of the head count)
        from safetensors.torch import save_file
        os.makedirs(path)
        save_file({k: v.contiguous() for k, v in llm.state_dict().items() if not k.endswith(".bias")}, str(path / "model.safetensors"))
        with open(path / "config.json", "w") as fh:
            json.dump(dict(kw, model_type="llama", architectures=["LlamaForCausalLM"], attention_bias=False, mlp_bias=False), fh)
    else:
        llm.save_pretrained(path, safe_serialization=True)
    _DIRS[name] = str(path)
    return _DIRS[name]


def _model(tmp_path_factory, name, **cfg_kw):
    key = (name, tuple(sorted(cfg_kw.items())))
    if key not in _MODELS:
        from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
        root = _root(tmp_path_factory)
        d = _DIRS["dims"]
        cfg = DeSTA25Config(llm_model_id=_llm_dir(tmp_path_factory, name), encoder_model_id=str(root / "enc"),
                            qformer_num_hidden_layers=d.qf_layers, prompt_size=d.prompt_size, qformer_intermediate_size=d.qf_inter, qformer_dropout=0.0, **cfg_kw)
        lc = cfg.llm_config
        assert lc.model_type == ("llama" if name.endswith("-llama") else "qwen2") and lc.attention_bias == (not name.endswith("-llama"))
        assert (lc.num_attention_heads, lc.num_key_value_heads, lc.head_dim) == GEOM[name.split("-")[0]] and not lc.qk_norm
        m = DeSTA25AudioModel(cfg)
        assert ("bqkv" in m.llm.layers[0]) == lc.attention_bias
        assert ("wqkv_il" in m.llm.layers[0]) == (name.endswith("-llama") and not cfg.use_lora)      # no fused-rope weight copy for a bias model
        assert m.llm.fuse_rope == name.endswith("-llama")
        _MODELS[key] = m
    return _MODELS[key]


def _hf(tmp_path_factory, name):
    if name not in _HF:
        from transformers import Qwen2ForCausalLM
        _HF[name] = Qwen2ForCausalLM.from_pretrained(_llm_dir(tmp_path_factory, name), dtype=torch.float32, attn_implementation="eager").eval()
    return _HF[name]


def _text(B, S, seed):
    """left-padded ids / mask: every third row padded by a varying amount"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V_, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.long)
    for b in range(0, B, 3):
        n = 1 + (b * 5 + 2) % 7
        am[b, :n] = 0
        ids[b, :n] = 0
    return ids, am


def _labels(ids, am):
    """Targets = the attended tokens whose predecessor is attended too.  The first token of a left-padded row would be predicted from
    the last padding row, a query with every key masked: what such a row attends is undefined in the reference (eager softmax over
    an all-masked row is uniform over EVERY key, future ones included) and never a target in a collated batch."""
    prev = torch.cat([torch.zeros_like(am[:, :1]), am[:, :-1]], 1)
    return torch.where((am * prev).bool(), ids, torch.full_like(ids, -100))


def _positions(am):
    return (torch.cumsum(am, 1) - 1).clamp_min(0)                            # index - left pad (0 on the padding)


def _train_llm(llm, ids, am):
    """Text-only training pass through the decoder alone -> (loss, logits [B, S, V] fp32, dL/d inputs_embeds [B, S, h] fp32, embeds)"""
    B, S = ids.shape
    dev = llm.dev
    emb = llm.embed[ids.to(dev)].contiguous()                                # bf16 [B, S, h]
    labels = _labels(ids, am).to(dev).contiguous()
    kv_start = (am == 0).sum(1).to(torch.int32).to(dev).contiguous()

    def fill(buf):
        buf[:B * S].copy_(emb.view(B * S, -1))
    logits = llm.forward(fill, B, S, kv_start, labels, True)
    lg = logits.view(B, S, llm.Vp)[:, :, :llm.V].float().cpu()
    loss = float(llm.loss_and_grad(labels, write_grad=True))
    dx = llm.backward().view(B, S, -1).float().cpu()
    torch.cuda.synchronize()
    return loss, lg, dx, emb.float().cpu()


@pytest.mark.parametrize("S", [40, 136])
@pytest.mark.parametrize("name", ["g7", "g4"])
def test_training_forward_backward_vs_hf_autograd(tmp_path_factory, name, S):
    """Fails on a tree that drops the biases: with them at N(0, 1) and +-30 in k the bias-free logits are nowhere near."""
    B = 4
    model, hf = _model(tmp_path_factory, name), _hf(tmp_path_factory, name)
    ids, am = _text(B, S, seed=S)
    loss, lg, dx, emb = _train_llm(model.llm, ids, am)
    x = emb.clone().requires_grad_(True)
    labels = _labels(ids, am)
    out = hf(inputs_embeds=x, attention_mask=am, position_ids=_positions(am), labels=labels)
    out.loss.backward()
    m = am.bool()
    e_lg, e_dx = rel_err(lg[m], out.logits[m]), rel_err(dx[m], x.grad[m])
    print(f"\n{name} S={S}: loss {loss:.5f} vs {float(out.loss.detach()):.5f}, logits rel-L2 {e_lg:.4f}, dX rel-L2 {e_dx:.4f}")
    assert abs(loss - float(out.loss)) < 2e-2, (loss, float(out.loss))
    assert e_lg < 3e-2, e_lg
    assert e_dx < 3e-2, e_dx


def _inputs(ids, am):
    return {"context_input_ids": ids, "context_attention_mask": am, "context_batch_start_positions": [], "batch_features": None,
            "batch_transcription_ids": []}


def _gen(model, ids, am, T=T_NEW, forced=None):
    return model._generate_step(_inputs(ids, am), pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=forced, collect_logits=True,
                                eos_token_id=[])


def _decode_reference(tmp_path_factory, name, B):
    """HF's own greedy tokens and the fp32 logits of every step (cache-free: the whole sequence again per step), once per case."""
    key = (name, B)
    if key not in _DECODE_REF:
        hf = _hf(tmp_path_factory, name)
        ids, am = _text(B, S_PROMPT, seed=B)
        cur_ids, cur_am, toks, lgs = ids, am, [], []
        with torch.no_grad():
            for _ in range(T_NEW):
                lo = hf(input_ids=cur_ids, attention_mask=cur_am, position_ids=_positions(cur_am)).logits[:, -1]
                nxt = lo.argmax(-1)
                toks.append(nxt)
                lgs.append(lo)
                cur_ids = torch.cat([cur_ids, nxt[:, None]], 1)
                cur_am = torch.cat([cur_am, torch.ones(B, 1, dtype=torch.long)], 1)
        _DECODE_REF[key] = (ids, am, torch.stack(toks, 1), torch.stack(lgs))
    return _DECODE_REF[key]


DECODE_CASES = [(n, B, kv, ch) for n in ("g7", "g4") for B in (3, 20) for kv in ("bf16", "fp8") for ch in (None, 16) if not (n == "g4" and kv == "fp8")]


@pytest.mark.parametrize("name,B,kv,chunk", DECODE_CASES)
def test_decode_teacher_forced_vs_hf(tmp_path_factory, name, B, kv, chunk):
    """12 steps on HF's own tokens: unchunked and chunked prompt pass, the 16-row (B = 3) and the wide (B = 20) step kernels, the
    bf16 and the FP8 cache (head_dim 128 only, as `set_kv_cache` says)."""
    model = _model(tmp_path_factory, name)
    ids, am, ref, lo = _decode_reference(tmp_path_factory, name, B)
    model.set_kv_cache(kv)
    model.set_prefill_chunk(chunk)
    try:
        out, logits = _gen(model, ids, am, forced=ref)
    finally:
        model.set_kv_cache("bf16")
        model.set_prefill_chunk(None)
    assert out.cpu().tolist() == ref.tolist() and logits.shape[:2] == lo.shape[:2]
    lg = logits.float().cpu()[:, :, :V_]
    es = [rel_err(lg[t], lo[t]) for t in range(T_NEW)]
    gap = lo.max(-1).values - lo.gather(-1, lg.argmax(-1).unsqueeze(-1)).squeeze(-1)
    worst = float((gap / lo.std(-1)).max())
    print(f"\n{name} B={B} kv={kv} chunk={chunk}: per-step rel-L2 max {max(es):.4f}, gap/spread {worst:.4f}")
    assert max(es) <= 3e-2, es
    assert worst <= 0.1, worst


def test_zero_bias_qwen2_equals_llama_directory_bit_for_bit(tmp_path_factory):
    """A Qwen2 directory whose biases are zero and the same tensors saved as a Llama directory (rope as its own kernel) compute
    the same bits: training logits, loss and dX, decode logits, bf16 and FP8 cache slabs."""
    a = _model(tmp_path_factory, "g7-zero")
    b = _model(tmp_path_factory, "g7-zero-llama")
    b.llm.fuse_rope = False
    assert all(float(ly["bqkv"].abs().max()) == 0.0 for ly in a.llm.layers) and "bqkv" not in b.llm.layers[0]
    ids, am = _text(4, 136, seed=3)
    ra, rb = _train_llm(a.llm, ids, am), _train_llm(b.llm, ids, am)
    assert not b.llm._rope_fused
    assert ra[0] == rb[0] and torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2])
    assert float(ra[2].abs().max()) > 0
    ids, am = _text(3, S_PROMPT, seed=4)
    for kv in ("bf16", "fp8"):
        for m in (a, b):
            m.set_kv_cache(kv)
        (ta, la), (tb, lb) = _gen(a, ids, am), _gen(b, ids, am)
        assert torch.equal(ta, tb) and torch.equal(la, lb), kv
        n = S_PROMPT + T_NEW - 1                                             # slots the run wrote
        for ca, cb in zip(a.llm.kv_cache, b.llm.kv_cache):
            assert ca.dtype == (torch.uint8 if kv == "fp8" else torch.bfloat16)
            assert torch.equal(ca[:, :n].view(torch.uint8), cb[:, :n].view(torch.uint8)), kv
            assert not torch.equal(ca[:, 0], ca[:, n - 1])
        if kv == "fp8":
            for sa, sb in zip(a.llm.kv_scale, b.llm.kv_scale):
                assert torch.equal(sa[:, :n], sb[:, :n])
    for m in (a, b):
        m.set_kv_cache("bf16")


def test_fp8_weights_equal_bf16_weights_on_snapped_weights(tmp_path_factory):
    """Linear weights on the e4m3 grid: the FP8 decode copies hold them exactly, so the run's tokens and logits are the bf16 run's
    (the bias is not quantised: it is added by the rotary kernel on both sides).  B = 3: gemm_w8, B = 20: gemm_wide."""
    model = _model(tmp_path_factory, "g7-snap")
    for B in (3, 20):
        ids, am = _text(B, S_PROMPT, seed=40 + B)
        model.set_decode_weights("bf16")
        tb, lb = _gen(model, ids, am)
        model.set_decode_weights("fp8")
        try:
            tf, lf = _gen(model, ids, am)
            assert all("q8" in ly and "wqkv" in ly["q8"] for ly in model.llm.layers)
        finally:
            model.set_decode_weights("bf16")
        assert torch.equal(tb, tf) and torch.equal(lb, lf), B


def test_speculative_gives_the_plain_runs_tokens(tmp_path_factory):
    model = _model(tmp_path_factory, "g7")
    ids, am = _text(3, S_PROMPT, seed=9)
    ids[:, 8:14] = ids[:, 2:8]                                               # a repeated span: something for the prompt lookup to find
    ids[am == 0] = 0
    plain, _ = _gen(model, ids, am, T=16)
    assert model.llm.spec_stats["path"] == "plain"
    model.set_speculative(3)
    try:
        spec, _ = _gen(model, ids, am, T=16)
        assert model.llm.spec_stats["path"] == "speculative", model.llm.spec_stats
    finally:
        model.set_speculative(None)
    assert torch.equal(plain, spec)


def test_lora_with_b_zero_equals_the_base_model_bit_for_bit(tmp_path_factory):
    """Adapters at their initial B = 0: the adapter sum adds exact zeros in front of the rotary kernel (which adds the bias on both
    sides), and the merged decode weight W + 0 keeps the same bias."""
    base = _model(tmp_path_factory, "g7")
    lora = _model(tmp_path_factory, "g7", use_lora=True)
    assert lora.llm.lora is not None and "bqkv" in lora.llm.layers[0]
    assert all(float(lora.arena.param(n).abs().max()) == 0.0 for n in lora.trainable_parameter_names if ".lora_B." in n)
    lora.eval()                                                              # no adapter dropout
    ids, am = _text(4, 40, seed=6)
    B, S = ids.shape
    outs = []
    for m in (base, lora):
        dev = m.llm.dev
        emb = m.llm.embed[ids.to(dev)].contiguous()
        labels = _labels(ids, am).to(dev).contiguous()
        kv_start = (am == 0).sum(1).to(torch.int32).to(dev).contiguous()
        lg = m.llm.forward(lambda buf: buf[:B * S].copy_(emb.view(B * S, -1)), B, S, kv_start, labels, False)
        lg = lg.view(B, S, -1).clone()
        outs.append((lg, float(m.llm.loss_and_grad(labels, write_grad=False))))
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][1] == outs[1][1]
    ids, am = _text(3, S_PROMPT, seed=7)
    (tb, lb), (tl, ll) = _gen(base, ids, am), _gen(lora, ids, am)
    assert torch.equal(tb, tl) and torch.equal(lb, ll)
