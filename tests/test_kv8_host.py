"""CPU: the host side of the FP8 KV cache — the two C entry points in the header and the library at an unchanged ABI version,
the binding's callables and counter, the entry point's `trainer.kv_cache` key, the model's check of the kind, and the register
budget of the new kernels."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _yaml_with(tmp_path, line):
    """A copy of the debug config directory whose trainer section carries `line` (or nothing)."""
    import shutil
    src = os.path.join(ROOT, "examples", "train", "config")
    dst = tmp_path / "config"
    shutil.copytree(src, dst)
    txt = open(dst / "desta25_debug.yaml").read()
    assert re.search(r"^trainer:\s*$", txt, flags=re.M) and "kv_cache" not in txt          # the shipped YAMLs do not carry the key
    if line:
        txt = re.sub(r"^trainer:\s*$", "trainer:\n  " + line, txt, count=1, flags=re.M)
    open(dst / "desta25_debug.yaml", "w").write(txt)
    return str(dst)


def test_header_declares_and_library_exports_the_kv8_entry_points_at_abi_8():
    import torch  # noqa: F401  (same load order as the product path)
    from desta import _hip
    txt = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+desta_attention_decode_kv8\s*\(\s*const desta_attn_desc\*\s*d,\s*const float\*\s*k_scale,\s*const float\*\s*v_scale,\s*"
                     r"int64_t scale_batch_stride,\s*int64_t scale_row_stride,\s*void\*\s*workspace,\s*size_t workspace_bytes,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"int\s+desta_rope_kv_append_e4m3\s*\(\s*void\*\s*qkv,.*?uint8_t\*\s*kv_cache,\s*int64_t kv_batch_stride,\s*int64_t kv_row_stride,\s*"
                     r"float\*\s*kv_scale,\s*int64_t scale_batch_stride,\s*int64_t scale_row_stride,\s*int slot0,\s*void\*\s*stream\s*\)", code, flags=re.S)
    assert int(re.search(r"#define DESTA_ABI_VERSION (\d+)", txt).group(1)) == 8 == _hip.ABI_VERSION == _hip.lib.desta_abi_version()
    assert hasattr(_hip.lib, "desta_attention_decode_kv8") and hasattr(_hip.lib, "desta_rope_kv_append_e4m3")
    doc = txt[txt.index("Decode attention on the opt-in FP8 KV cache"):txt.index("int    desta_attention_decode_kv8")]
    assert "modeling_desta25.py:1419" in doc and "e4m3fn" in doc


def test_binding_has_the_kv8_callables_and_counter():
    from desta import _hip
    assert callable(_hip.attention_decode_kv8) and callable(_hip.rope_kv_append_e4m3)
    assert isinstance(_hip.ATTN_KV8_CALLS, int) and isinstance(_hip.ATTN_DECODE_CALLS, int)


@pytest.mark.parametrize("line,want", [(None, "bf16"), ("kv_cache: bf16", "bf16"), ("kv_cache: fp8", "fp8")])
def test_kv_cache_key_parses(tmp_path, line, want):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, line))
    assert m.kv_cache_kind(cfg) == want
    assert m.decode_weights_kind(cfg) == "bf16" and cfg.trainer.max_epochs is not None      # the rest of the trainer section is intact


def test_unknown_kv_cache_raises_before_any_gpu_work(tmp_path, monkeypatch):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, "kv_cache: int4"))
    with pytest.raises(ValueError, match="kv_cache"):
        m.kv_cache_kind(cfg)
    monkeypatch.setattr(m, "create_model", lambda *a, **k: pytest.fail("create_model reached with a bad trainer.kv_cache"))
    monkeypatch.setattr(m, "load_config", lambda argv, config_dir=None: cfg)
    with pytest.raises(ValueError, match="kv_cache"):
        m.main([])
    cfg2 = _load("train_desta_cli", "examples", "train", "train_desta.py").load_config(
        ["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}", "+trainer.kv_cache=int8"])
    with pytest.raises(ValueError, match="int8"):                           # the command-line override takes the same route
        m.kv_cache_kind(cfg2)


def test_model_rejects_unknown_kv_cache_without_gpu():
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    assert CausalLMHIP.KV_CACHE_KINDS == ("bf16", "fp8")
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                    # no device state: the check comes first
    with pytest.raises(ValueError, match="int4"):
        model.set_kv_cache("int4")
    llm = CausalLMHIP.__new__(CausalLMHIP)
    llm.kv_cache_kind, llm.hd, llm.hq, llm.hkv = "bf16", 64, 4, 2
    with pytest.raises(ValueError, match="int4"):
        llm.set_kv_cache("int4")
    with pytest.raises(ValueError, match="head_dim"):                        # a geometry the split-KV kernel does not take
        llm.set_kv_cache("fp8")
    llm.hd, llm.hq, llm.hkv = 128, 32, 2
    with pytest.raises(ValueError, match="16 per KV head"):
        llm.set_kv_cache("fp8")
    assert llm.kv_cache_kind == "bf16"


def test_kv8_kernels_use_no_scratch():
    res = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources()
    attn = {n: r for n, r in res.items() if "attn_kv8_k" in n}
    rope = {n: r for n, r in res.items() if "rope_kv8_k" in n}
    assert len(attn) == 4 and len(rope) >= 1, (sorted(attn), sorted(rope))  # groups padded to 1, 2, 4, 8 query rows; the append with / without q/k-norm
    for name, r in sorted({**attn, **rope}.items()):
        print(f"{name[:80]:80s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} lds {r['lds']:6d} scratch {r['scratch']} spilled {r['spill']}")
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["vgpr"] <= 256 and r["lds"] <= 64 * 1024, (name, r)
