"""CPU: Qwen2 / Qwen2.5 decoders at the config and loader level: `LLMConfig.attention_bias` is detected and survives a round
trip, and every bias (or mask) no kernel consumes raises a NotImplementedError that names it, at load, instead of being dropped."""
import json

import pytest

from desta.models.modeling_desta25 import LLM, DeSTA25Config, LLMConfig, check_llm_bias_tensors

ENC = dict(num_mel_bins=8, d_model=32, encoder_layers=4, encoder_attention_heads=2, encoder_ffn_dim=64, max_source_positions=16)


def _llm(**kw):
    c = dict(model_type="qwen2", hidden_size=256, num_hidden_layers=2, num_attention_heads=7, num_key_value_heads=1, head_dim=128,
             intermediate_size=256, vocab_size=320, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False)
    c.update(kw)
    return c


def _cfg(**kw):
    return DeSTA25Config(llm_model_id="local-llm", encoder_model_id="local-whisper", llm_config=_llm(**kw), encoder_config=ENC,
                         target_layer_ids=[0, 1, 2, 3])


def _names(c: LLMConfig, extra=(), drop=()):
    n = [f"{LLM}model.layers.{i}.self_attn.{m}_proj.{t}" for i in range(c.num_hidden_layers) for m in "qkvo" for t in ("weight",)]
    if c.attention_bias:
        n += [f"{LLM}model.layers.{i}.self_attn.{m}_proj.bias" for i in range(c.num_hidden_layers) for m in "qkv"]
    n += ["perception.whisper.model.encoder.layers.0.self_attn.q_proj.bias", "perception.whisper.model.encoder.conv1.bias"]   # not the decoder's business
    return [x for x in n if x not in drop] + list(extra)


def test_attention_bias_detection_and_round_trip(tmp_path):
    assert LLMConfig().attention_bias is False
    assert _cfg().llm_config.attention_bias and not _cfg().llm_config.qk_norm                  # qwen2: always, whatever the file says
    assert _cfg(attention_bias=False).llm_config.attention_bias
    assert not _cfg(model_type="llama").llm_config.attention_bias
    assert not _cfg(model_type="qwen3").llm_config.attention_bias
    assert _cfg(model_type="llama", attention_bias=True).llm_config.attention_bias            # config.json's own flag
    assert not _cfg(model_type="llama", attention_bias=False, mlp_bias=False, use_sliding_window=False).llm_config.attention_bias
    # what Qwen2.5's config.json carries besides: an inactive sliding window is fine
    cfg = _cfg(use_sliding_window=False, sliding_window=131072, max_window_layers=28)
    d = cfg.to_dict()
    assert d["llm_config"]["attention_bias"] is True and d["llm_config"]["model_type"] == "qwen2"
    json.dumps(d)
    cfg.save_pretrained(str(tmp_path))
    back = DeSTA25Config.from_pretrained(str(tmp_path))
    assert back.llm_config == cfg.llm_config and back.llm_config.attention_bias
    # the flag alone round-trips too (a Llama-type config that sets it)
    ll = _cfg(model_type="llama", attention_bias=True)
    assert DeSTA25Config(llm_model_id="x", encoder_model_id="y", llm_config=ll.to_dict()["llm_config"], encoder_config=ENC,
                         target_layer_ids=[0, 1, 2, 3]).llm_config.attention_bias


def test_full_config_qwen25_7b():
    from desta.synthetic import FULL_CONFIGS
    c = DeSTA25Config(**FULL_CONFIGS["qwen2.5-7B"]).llm_config
    assert FULL_CONFIGS["qwen2.5-7B"] is FULL_CONFIGS["desta25_qwen25-7B_Qformer6L"] and "qwen2.5-7B" not in set(FULL_CONFIGS)
    assert (c.model_type, c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads, c.head_dim) == ("qwen2", 3584, 28, 28, 4, 128)
    assert (c.intermediate_size, c.vocab_size, c.rope_theta, c.tie_word_embeddings, c.attention_bias, c.qk_norm) == (18944, 152064, 1e6, False, True, False)
    with pytest.raises(KeyError):
        FULL_CONFIGS["qwen2.5-70B"]


def test_config_flags_without_a_kernel_raise_by_name():
    with pytest.raises(NotImplementedError, match="mlp_bias"):
        _cfg(model_type="llama", mlp_bias=True)
    with pytest.raises(NotImplementedError, match="use_sliding_window"):
        _cfg(use_sliding_window=True, sliding_window=4096)


def test_unconsumed_bias_tensors_raise_by_name():
    q2 = _cfg().llm_config
    check_llm_bias_tensors(q2, _names(q2))                                                     # a Qwen2 checkpoint as it is: fine
    ll = _cfg(model_type="llama").llm_config
    check_llm_bias_tensors(ll, _names(ll))
    check_llm_bias_tensors(q2, None)                                                           # a lazy weight source: nothing to list
    # Llama's attention_bias: q, k, v AND o carry a bias
    la = _cfg(model_type="llama", attention_bias=True).llm_config
    with pytest.raises(NotImplementedError, match=r"model\.layers\.0\.self_attn\.o_proj\.bias.*o_proj\.bias \(Llama-style attention_bias\)"):
        check_llm_bias_tensors(la, _names(la, extra=[f"{LLM}model.layers.{i}.self_attn.o_proj.bias" for i in range(2)]))
    # mlp_bias tensors in a checkpoint whose config does not say so
    with pytest.raises(NotImplementedError, match=r"model\.layers\.1\.mlp\.down_proj\.bias.*mlp_bias"):
        check_llm_bias_tensors(q2, _names(q2, extra=[f"{LLM}model.layers.1.mlp.down_proj.bias"]))
    # q|k|v biases in a checkpoint whose config has no attention_bias: today's silent drop
    with pytest.raises(NotImplementedError, match=r"model\.layers\.0\.self_attn\.k_proj\.bias.*without attention_bias"):
        check_llm_bias_tensors(ll, _names(q2))
    # any other *.bias
    with pytest.raises(NotImplementedError, match=r"lm_head\.bias.*an unused bias"):
        check_llm_bias_tensors(q2, _names(q2, extra=[f"{LLM}lm_head.bias"]))
    # a bias together with the q/k-norm: no kernel adds one in front of the norm
    with pytest.raises(NotImplementedError, match="q/k-norm"):
        check_llm_bias_tensors(_cfg(model_type="qwen3", attention_bias=True).llm_config, [])
    # and a checkpoint that lacks a bias its config promises
    with pytest.raises(KeyError, match=r"model\.layers\.1\.self_attn\.v_proj\.bias"):
        check_llm_bias_tensors(q2, _names(q2, drop=[f"{LLM}model.layers.1.self_attn.v_proj.bias"]))


def test_binding_declares_the_bias_forms_and_rejects_a_bias_in_the_backward():
    from desta import _hip as H
    for fn in (H._rope_bias, H._rope_kv_bias, H._rope_kv8_bias):
        assert fn.restype is not None and len(fn.argtypes) >= 14
    with pytest.raises(ValueError, match="backward"):
        H.rope(None, 0, 1, 1, 1, 1, 128, None, backward=True, bias=object())
    assert H.ABI_VERSION == 8


def test_new_rotary_kernels_use_no_scratch():
    import importlib.util
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # the BIAS = true instantiations of rope_k<HD, NORM, BWD, BIAS> and rope_kv8_k<NORM, BIAS> (the last template argument, "Lb1E")
    res = {n: r for n, r in mod.kernel_resources().items() if re.search(r"\d(rope_k|rope_kv8_k)I(Li\d+E)+(Lb[01]E)*Lb1EE", n)}
    assert len(res) == 3, sorted(res)                                                          # head_dim 64 and 128, and the e4m3 form
    for n, r in res.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (n, r)
