"""CPU checks of the opt-in generation defaults and of the full-chain sampler's build.

`resolve_generation_kwargs` must pick the same sampling settings as transformers' own `_prepare_generation_config`
(explicit argument > checkpoint generation_config.json > HF global defaults, TF:generation/utils.py:1806-1808) on a tiny
locally built LlamaForCausalLM; the new sampler kernels must keep everything in registers."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("do_sample", "temperature", "top_k", "top_p", "min_p", "repetition_penalty")


def _hf_resolved(file_cfg, explicit):
    import torch
    from transformers import GenerationConfig, LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    m = LlamaForCausalLM(LlamaConfig(vocab_size=64, hidden_size=16, intermediate_size=32, num_hidden_layers=1,
                                     num_attention_heads=2, num_key_value_heads=1))
    m.generation_config = GenerationConfig(**file_cfg)
    gc, _ = m._prepare_generation_config(None, **explicit)
    return {k: getattr(gc, k) for k in KEYS}


CASES = [
    ({}, {}),
    ({}, dict(temperature=0.7, top_p=0.9, do_sample=True)),
    ({"top_k": 20, "top_p": 0.95, "temperature": 0.6, "do_sample": True}, {}),
    ({"top_k": 20, "top_p": 0.95, "temperature": 0.6, "do_sample": True}, dict(top_k=5, temperature=0.9, top_p=0.5)),
    ({"repetition_penalty": 1.1, "min_p": 0.05}, dict(do_sample=True)),
    ({"repetition_penalty": 1.1, "min_p": 0.05, "top_k": 0}, dict(repetition_penalty=1.3, min_p=0.2)),
    ({"bos_token_id": 1, "eos_token_id": [2, 3], "do_sample": True, "temperature": 0.6, "top_p": 0.9}, {}),
]


@pytest.mark.parametrize("file_cfg,explicit", CASES)
def test_resolve_generation_kwargs_matches_transformers(file_cfg, explicit):
    from desta.models.modeling_desta25 import resolve_generation_kwargs
    got = resolve_generation_kwargs(file_cfg, **explicit)
    want = _hf_resolved(file_cfg, explicit)
    assert {k: got[k] for k in KEYS} == want


def test_resolve_generation_kwargs_defaults_and_passthrough():
    from desta.models.modeling_desta25 import resolve_generation_kwargs
    r = resolve_generation_kwargs({}, max_new_tokens=7, seed=3, top_p=None)
    assert r["top_k"] == 50 and r["top_p"] == 1.0 and r["min_p"] is None and r["do_sample"] is False
    assert r["max_new_tokens"] == 7 and r["seed"] == 3
    assert resolve_generation_kwargs({"top_k": 20}, top_k=0)["top_k"] == 0            # an explicit 0 switches top-k off


@pytest.mark.parametrize("file_cfg,explicit,name", [
    ({"num_beams": 4}, {}, "num_beams"),
    ({}, dict(num_beams=2), "num_beams"),
    ({"typical_p": 0.5}, {}, "typical_p"),
    ({}, dict(no_repeat_ngram_size=3), "no_repeat_ngram_size"),
    ({"suppress_tokens": [5]}, {}, "suppress_tokens"),
    ({"epsilon_cutoff": 3e-4}, {}, "epsilon_cutoff"),
])
def test_resolve_generation_kwargs_rejects_unsupported(file_cfg, explicit, name):
    from desta.models.modeling_desta25 import resolve_generation_kwargs
    with pytest.raises(NotImplementedError, match=name):
        resolve_generation_kwargs(file_cfg, **explicit)
    # the same settings at HF's "off" value are accepted
    resolve_generation_kwargs({"num_beams": 1, "typical_p": 1.0, "suppress_tokens": None, "no_repeat_ngram_size": 0})


def test_check_sampling_args_messages():
    from desta.models.modeling_desta25 import check_sampling_args
    check_sampling_args(None, None, None)
    check_sampling_args(0, 0.0, 1.0)
    check_sampling_args(50, 1.0, 1.2)
    for kw, msg in ((dict(top_k=-1), "`top_k` has to be a strictly positive integer"), (dict(top_k=2.5), "`top_k`"),
                    (dict(min_p=1.5), "`min_p` has to be a float in the \\[0, 1\\] interval"), (dict(min_p=-0.1), "`min_p`"),
                    (dict(repetition_penalty=0.0), "`penalty` has to be a strictly positive float"),
                    (dict(repetition_penalty=-1.0), "`penalty`")):
        with pytest.raises(ValueError, match=msg):
            check_sampling_args(**kw)


def test_sampler_kernels_use_no_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.kernel_resources()
    seen = [n for n in res if "sample_chain_k" in n or "sample_greedy_k" in n]
    assert len(seen) == 2, seen
    for n in seen:
        assert res[n]["scratch"] == 0 and res[n]["spill"] == 0, (n, res[n])


def test_model_reads_llm_generation_config(tmp_path):
    """The model keeps <llm_model_id>/generation_config.json as read (not merged into DeSTA's config.json); the file is
    read with plain json, checked here on the host side of the constructor's logic."""
    from desta.models.modeling_desta25 import DeSTA25AudioModel, resolve_generation_kwargs
    (tmp_path / "generation_config.json").write_text(json.dumps({"top_k": 20, "temperature": 0.6, "do_sample": True}))

    class Stub:                                     # hf_generation_kwargs needs only the attribute
        llm_generation_config = json.loads((tmp_path / "generation_config.json").read_text())
    r = DeSTA25AudioModel.hf_generation_kwargs(Stub(), top_p=0.9)
    assert r == resolve_generation_kwargs(Stub.llm_generation_config, top_p=0.9)
    assert r["top_k"] == 20 and r["temperature"] == 0.6 and r["top_p"] == 0.9 and r["do_sample"] is True
