"""CPU: the host side of weight-only FP8 decode — the entry point's `trainer.decode_weights` key, the two C entry points in the
header at an unchanged ABI version, and the register budget of the new kernel instantiations."""
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
    assert re.search(r"^trainer:\s*$", txt, flags=re.M) and "decode_weights" not in txt
    if line:
        txt = re.sub(r"^trainer:\s*$", "trainer:\n  " + line, txt, count=1, flags=re.M)
    open(dst / "desta25_debug.yaml", "w").write(txt)
    return str(dst)


@pytest.mark.parametrize("line,want", [(None, "bf16"), ("decode_weights: bf16", "bf16"), ("decode_weights: fp8", "fp8")])
def test_decode_weights_key_parses(tmp_path, line, want):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, line))
    assert m.decode_weights_kind(cfg) == want
    assert cfg.trainer.max_epochs is not None                               # the rest of the trainer section is intact


def test_unknown_decode_weights_raises_before_any_gpu_work(tmp_path, monkeypatch):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg_dir = _yaml_with(tmp_path, "decode_weights: int4")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"], config_dir=cfg_dir)
    with pytest.raises(ValueError, match="decode_weights"):
        m.decode_weights_kind(cfg)
    # through main(): the model is never built
    monkeypatch.setattr(m, "create_model", lambda *a, **k: pytest.fail("create_model reached with a bad trainer.decode_weights"))
    monkeypatch.setattr(m, "load_config", lambda argv, config_dir=None: cfg)
    with pytest.raises(ValueError, match="decode_weights"):
        m.main([])
    cfg2 = _load("train_desta_cli", "examples", "train", "train_desta.py").load_config(
        ["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}", "+trainer.decode_weights=int8"])
    with pytest.raises(ValueError, match="int8"):                           # the command-line override takes the same route
        m.decode_weights_kind(cfg2)


def test_header_declares_the_fp8_entry_points_at_abi_8():
    txt = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+desta_quantize_rows_e4m3\s*\(\s*const void\*\s*w_bf16,\s*int rows,\s*int cols,\s*int64_t ld,\s*uint8_t\*\s*q,\s*float\*\s*scale,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"int\s+desta_gemm_w8a16_nt\s*\(\s*const desta_gemm_desc\*\s*d,\s*const float\*\s*b_scale,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"#define DESTA_ABI_VERSION (\d+)", txt).group(1) == "8"
    assert "modeling_desta25.py:1419-1427" in txt and "modeling_llama.py:163-176" in txt
    from desta import _hip
    assert _hip.ABI_VERSION == 8 and _hip.lib.desta_abi_version() == 8
    assert hasattr(_hip.lib, "desta_quantize_rows_e4m3") and hasattr(_hip.lib, "desta_gemm_w8a16_nt")
    assert callable(_hip.quantize_rows_e4m3) and callable(_hip.gemm_w8)


def test_model_rejects_unknown_decode_weights_without_gpu():
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    assert CausalLMHIP.DECODE_WEIGHT_KINDS == ("bf16", "fp8")
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                    # no device state: the check comes first
    with pytest.raises(ValueError, match="int4"):
        model.set_decode_weights("int4")


def test_fp8_skinny_kernels_use_no_scratch():
    """The W8 instantiations of the skinny kernel (last template argument true) and the quantiser: no scratch, no spills."""
    res = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources()
    w8 = {n: r for n, r in res.items() if re.search(r"gemm_bf16_nt_skinny_kernelILi\d+ELi\d+ELb[01]ELb[01]ELb1EEE", n)}
    assert len(w8) >= 4, sorted(w8)                                          # plain / SwiGLU x with / without the fused RMSNorm
    quant = {n: r for n, r in res.items() if "quantize_rows_e4m3" in n}
    assert len(quant) == 1
    for n, r in {**w8, **quant}.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (n, r)
