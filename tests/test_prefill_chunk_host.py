"""CPU: the host side of the chunked prompt pass — `check_prefill_chunk`, the chunk ranges of `prefill_chunks`, the setters'
checks without device state, the entry point's `trainer.prefill_chunk` key, the new C entry point in the header and the library
at an unchanged ABI version, and the register budget of the dequantising kernel."""
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
    assert re.search(r"^trainer:\s*$", txt, flags=re.M) and "prefill_chunk" not in txt     # the shipped YAMLs do not carry the key
    if line:
        txt = re.sub(r"^trainer:\s*$", "trainer:\n  " + line, txt, count=1, flags=re.M)
    open(dst / "desta25_debug.yaml", "w").write(txt)
    return str(dst)


BAD = [0, 15, -128, True, 128.0, "128"]


def test_check_prefill_chunk():
    from desta.models.modeling_desta25 import check_prefill_chunk
    for n in (None, 16, 128, 4096):
        assert check_prefill_chunk(n) is None
    for n in BAD:
        with pytest.raises(ValueError, match="prefill_chunk"):
            check_prefill_chunk(n)


@pytest.mark.parametrize("C", [16, 128, 512])
@pytest.mark.parametrize("S", [1, 16, 127, 128, 129, 251, 300, 1024])
def test_prefill_chunks_cover_the_prompt(S, C):
    from desta.models.modeling_desta25 import prefill_chunks
    ch = prefill_chunks(S, C)
    assert ch[0][0] == 0 and ch[-1][1] == S
    assert all(a[1] == b[0] for a, b in zip(ch, ch[1:]))                     # contiguous, in order
    assert all(c1 - c0 == C for c0, c1 in ch[:-1])
    assert 1 <= ch[-1][1] - ch[-1][0] <= C
    assert len(ch) == (S + C - 1) // C
    assert sorted(set(p for c0, c1 in ch for p in range(c0, c1))) == list(range(S)) and sum(c1 - c0 for c0, c1 in ch) == S


def test_setters_check_before_any_device_state():
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                    # no device state: the check comes first
    llm = CausalLMHIP.__new__(CausalLMHIP)
    llm.prefill_chunk = None
    for n in BAD:
        with pytest.raises(ValueError, match="prefill_chunk"):
            model.set_prefill_chunk(n)
        with pytest.raises(ValueError, match="prefill_chunk"):
            llm.set_prefill_chunk(n)
    assert llm.prefill_chunk is None
    llm.set_prefill_chunk(128)
    assert llm.prefill_chunk == 128 and llm._gen_shape is None              # generate() re-allocates for the new setting
    llm.set_prefill_chunk(None)
    assert llm.prefill_chunk is None


@pytest.mark.parametrize("line,want", [(None, None), ("prefill_chunk: 16", 16), ("prefill_chunk: 512", 512)])
def test_prefill_chunk_key_parses(tmp_path, line, want):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, line))
    assert m.prefill_chunk(cfg) == want
    assert m.kv_cache_kind(cfg) == "bf16" and m.decode_weights_kind(cfg) == "bf16" and cfg.trainer.max_epochs is not None


@pytest.mark.parametrize("line", ["prefill_chunk: 8", "prefill_chunk: true", "prefill_chunk: 128.0", "prefill_chunk: '128'"])
def test_bad_prefill_chunk_raises_before_any_gpu_work(tmp_path, monkeypatch, line):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, line))
    with pytest.raises(ValueError, match="trainer.prefill_chunk"):
        m.prefill_chunk(cfg)
    monkeypatch.setattr(m, "create_model", lambda *a, **k: pytest.fail("create_model reached with a bad trainer.prefill_chunk"))
    monkeypatch.setattr(m, "load_config", lambda argv, config_dir=None: cfg)
    with pytest.raises(ValueError, match="trainer.prefill_chunk"):
        m.main([])


def test_header_declares_and_library_exports_the_dequant_entry_point_at_abi_8():
    import torch  # noqa: F401  (same load order as the product path)
    from desta import _hip
    txt = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+desta_kv8_dequant\s*\(\s*const uint8_t\*\s*kv_cache,\s*int64_t kv_batch_stride,\s*int64_t kv_row_stride,\s*"
                     r"const float\*\s*kv_scale,\s*int64_t scale_batch_stride,\s*int64_t scale_row_stride,\s*const int32_t\*\s*kv_start,\s*"
                     r"int batch,\s*int n_heads,\s*int head_dim,\s*int slot1,\s*void\*\s*out_bf16,\s*int64_t out_batch_stride,\s*"
                     r"int64_t out_row_stride,\s*void\*\s*stream\s*\)", code)
    assert int(re.search(r"#define DESTA_ABI_VERSION (\d+)", txt).group(1)) == 8 == _hip.ABI_VERSION == _hip.lib.desta_abi_version()
    assert hasattr(_hip.lib, "desta_kv8_dequant")
    assert callable(_hip.kv8_dequant) and isinstance(_hip.KV8_DEQUANT_CALLS, int)


def test_dequant_kernel_uses_no_scratch_and_no_lds():
    res = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources()
    k = {n: r for n, r in res.items() if "kv8_dequant_k" in n}
    assert len(k) == 1, sorted(k)
    for name, r in k.items():
        print(f"{name[:80]:80s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} lds {r['lds']:6d} scratch {r['scratch']} spilled {r['spill']}")
        assert r["scratch"] == 0 and r["spill"] == 0 and r["lds"] == 0, (name, r)
        assert r["vgpr"] <= 64, (name, r)                                    # eight waves per SIMD: the kernel only moves bytes
