"""CPU-only: the split-KV verify attention (desta_attention_verify{,_kv8}) is declared, exported and bound at ABI 8, its kernels
keep everything in registers, `set_speculative(attention=...)` and the entry point's `trainer.speculative_attention` key check their
values before anything changes, `_spec_reason` answers as documented under attention = "split", and the float64 reference of the
GPU tests reproduces the one-row reference of tests/test_gpu_decode_attention.py."""
import importlib.util
import os
import re
import shutil

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_header_declares_and_library_exports_verify_attention_at_abi_8():
    from desta import _hip
    hdr = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    assert re.search(r"\bsize_t\s+desta_attention_verify_workspace_bytes\(int batch, int n_q_heads, int seq_q, int seq_k, int head_dim\);", hdr)
    assert re.search(r"\bint\s+desta_attention_verify\(const desta_attn_desc\* d, void\* workspace, size_t workspace_bytes, void\* stream\);", hdr)
    assert re.search(r"\bint\s+desta_attention_verify_kv8\(const desta_attn_desc\* d, const float\* k_scale, const float\* v_scale, int64_t scale_batch_stride,\s*"
                     r"int64_t scale_row_stride, void\* workspace, size_t workspace_bytes, void\* stream\);", hdr)
    assert int(re.search(r"#define DESTA_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _hip.ABI_VERSION == _hip.lib.desta_abi_version()
    for sym in ("desta_attention_verify", "desta_attention_verify_kv8", "desta_attention_verify_workspace_bytes"):
        assert hasattr(_hip.lib, sym), sym
    doc = hdr[hdr.index("Split-KV attention of a verify step"):hdr.index("size_t desta_attention_verify_workspace_bytes")]
    assert "modeling_desta25.py:1419" in doc and "bit for bit" in doc
    assert int(re.search(r"#define DESTA_ATTN_VERIFY_MAX_ROWS (\d+)", hdr).group(1)) == 16 == _hip.VERIFY_ATTN_MAX_ROWS


def test_binding_and_workspace_size():
    from desta import _hip
    assert callable(_hip.attention_verify) and callable(_hip.attention_verify_kv8) and callable(_hip.attention_verify_workspace_bytes)
    CH = _hip.DECODE_ATTN_CHUNK
    assert _hip.attention_verify_workspace_bytes(3, 8, 4, CH) == 0           # one chunk: the main kernel finishes every row
    for w in (2, 3, 8):
        for n in (2, 3, 7):
            items = 3 * 8 * w * n                                            # one partial per (row, head, query row, chunk)
            want = 4 * ((2 * items + 3) // 4 * 4 + 128 * items)
            assert _hip.attention_verify_workspace_bytes(3, 8, w, (n - 1) * CH + 1) == want == _hip.attention_verify_workspace_bytes(3, 8, w, n * CH)
            assert want == _hip.attention_decode_workspace_bytes(3, 8 * w, n * CH)


def test_verify_attention_kernels_use_no_scratch_and_leave_the_one_row_kernels_alone():
    res = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources()
    new = {n: r for n, r in res.items() if "attn_verify" in n}
    main16 = sorted(n for n in new if re.search(r"attn_verify_kILi(\d+)E", n))
    main8 = sorted(n for n in new if re.search(r"attn_verify_kv8_kILi(\d+)E", n))
    rows = lambda names, pat: sorted(int(re.search(pat, n).group(1)) for n in names)
    assert rows(main16, r"attn_verify_kILi(\d+)E") == [2, 4, 8, 16] == rows(main8, r"attn_verify_kv8_kILi(\d+)E")
    assert sorted(new) == sorted(main16 + main8 + [n for n in new if "attn_verify_combine_k" in n]) and len(new) == 9
    for name in sorted(new):
        r = new[name]
        print(f"{name[:80]:80s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} lds {r['lds']:6d} scratch {r['scratch']} spilled {r['spill']}")
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["vgpr"] <= 256 and r["lds"] <= 64 * 1024, (name, r)         # two blocks per CU by registers, three by LDS at 16 rows
    assert sum("attn_decode" in n for n in res) == 5 and sum("attn_kv8_k" in n for n in res) == 4
    assert not any("attn_decode" in n or "attn_kv8_k" in n for n in new)


def _bare_llm(hq=8, hkv=2, hd=128):
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                    # no device state: the checks come first
    llm = model.llm = CausalLMHIP.__new__(CausalLMHIP)
    llm.speculative = llm._spec = None
    llm.spec_scope, llm.spec_attention, llm.kv_cache_kind = "greedy", "forward", "bf16"
    llm.hq, llm.hkv, llm.hd = hq, hkv, hd
    return model, llm


def test_attention_argument():
    from desta.models.modeling_desta25 import SPECULATIVE_ATTENTIONS, check_speculative_attention
    assert SPECULATIVE_ATTENTIONS == ("forward", "split")
    for ok in SPECULATIVE_ATTENTIONS:
        check_speculative_attention(ok)
    model, llm = _bare_llm()
    model.set_speculative(3, "all", attention="split")
    assert (llm.speculative, llm.spec_scope, llm.spec_attention) == (3, "all", "split")
    for bad in ("Split", "fwd", "", None, 1, True, ["split"]):
        with pytest.raises(ValueError, match="speculative attention"):
            check_speculative_attention(bad)
        for target in (model, llm):
            with pytest.raises(ValueError, match="speculative"):
                target.set_speculative(5, "greedy", attention=bad)
            with pytest.raises(ValueError, match="speculative"):
                target.set_speculative(9, attention="forward")               # a bad k with a good attention
            with pytest.raises(ValueError, match="speculative"):
                target.set_speculative(5, "some", attention="forward")       # a bad scope with a good attention
            assert (llm.speculative, llm.spec_scope, llm.spec_attention) == (3, "all", "split")      # the setting is untouched
    llm._spec = marker = dict(key=(3, 3))
    llm.set_speculative(3, "all", attention="forward")                       # only the attention changes: the verify buffers stay
    assert llm._spec is marker and llm.spec_attention == "forward"
    llm.set_speculative(3, "all", "split")                                   # positional
    assert llm._spec is marker and llm.spec_attention == "split"
    llm.set_speculative(7, "all", "split")                                   # k changes: they go
    assert llm._spec is None
    model.set_speculative(3)                                                 # the positional (k) and (k, scope) forms: today's defaults
    assert (llm.speculative, llm.spec_scope, llm.spec_attention) == (3, "greedy", "forward")
    model.set_speculative(3, "all")
    assert (llm.speculative, llm.spec_scope, llm.spec_attention) == (3, "all", "forward")


def test_spec_reason_table_under_split():
    from desta import _hip
    model, llm = _bare_llm(8, 2)                                             # G = 4
    none = (False, False, None, None, None)
    llm.set_speculative(3, attention="split")
    assert llm._spec_reason(3, 3, *none) is None
    llm.kv_cache_kind = "fp8"
    assert llm._spec_reason(3, 3, *none) is None                             # 4 x 4 = 16 rows: speculates
    assert llm._spec_reason(1, 3, *none) is None
    assert llm._spec_reason(4, 3, *none) == "fp8 kv cache: 4 x 5 = 20 query rows per KV head > 16"
    assert llm._spec_reason(3, 3, False, False, None, object(), None) == "forced_tokens"
    assert llm._spec_reason(3, 3, False, False, None, None, object()) == "layer_hook"
    assert llm._spec_reason(3, 3, True, False, None, None, None) == "do_sample"
    llm.kv_cache_kind = "bf16"
    assert llm._spec_reason(3, 17, *none) == f"B * (k + 1) = 68 rows > {_hip.DECODE_MAX_ROWS}"
    assert llm._spec_reason(7, 3, *none) is None                             # bf16 cache: the forward kernel takes what the verify kernel does not
    llm.kv_cache_kind = "fp8"
    assert llm._spec_reason(3, 17, *none) == f"B * (k + 1) = 68 rows > {_hip.DECODE_MAX_ROWS}"
    _, q7 = _bare_llm(28, 4)                                                 # Qwen2.5-7B: G = 7
    q7.set_speculative(3, "all", attention="split")
    q7.kv_cache_kind = "fp8"
    assert q7._spec_reason(3, 3, True, True, 2, None, None) == "fp8 kv cache: 7 x 4 = 28 query rows per KV head > 16"
    assert q7._spec_reason(1, 3, True, True, 2, None, None) is None          # 7 x 2 = 14
    for scope in ("greedy", "all"):                                          # the default attention: today's answer
        llm.set_speculative(3, scope)
        assert llm._spec_reason(3, 3, *none) == "fp8 kv cache"
        q7.set_speculative(3, scope)
        assert q7._spec_reason(3, 3, *none) == "fp8 kv cache"


def _yaml_with(tmp_path, *lines):
    """A copy of the debug config directory whose trainer section carries `lines`."""
    src = os.path.join(ROOT, "examples", "train", "config")
    dst = tmp_path / "config"
    shutil.copytree(src, dst)
    for name in os.listdir(src):
        if name.endswith(".yaml"):
            assert "speculative_attention" not in open(os.path.join(src, name)).read(), name     # no shipped YAML carries the key
    txt = open(dst / "desta25_debug.yaml").read()
    assert re.search(r"^trainer:\s*$", txt, flags=re.M)
    if lines:
        txt = re.sub(r"^trainer:\s*$", "trainer:\n  " + "\n  ".join(lines), txt, count=1, flags=re.M)
    open(dst / "desta25_debug.yaml", "w").write(txt)
    return str(dst)


ARGV = ["--config-name", "desta25_debug", "+dataset=debug"]


@pytest.mark.parametrize("lines,want", [((), "forward"), (("speculative: 3",), "forward"), (("speculative: 3", "speculative_attention: split"), "split"),
                                        (("speculative_attention: forward",), "forward")])
def test_speculative_attention_key_parses(tmp_path, lines, want):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(ARGV + [f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, *lines))
    assert m.speculative_attention(cfg) == want
    assert m.speculative_scope(cfg) == "greedy" and cfg.trainer.max_epochs is not None          # the rest of the trainer section is intact


def test_speculative_attention_command_line_override(tmp_path):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(ARGV + [f"exp_dir={tmp_path}", "+trainer.speculative_attention=split"], config_dir=_yaml_with(tmp_path, "speculative: 3"))
    assert (m.speculative(cfg), m.speculative_attention(cfg)) == (3, "split")
    cfg = m.load_config(ARGV + [f"exp_dir={tmp_path}", "trainer.speculative_attention=forward"],
                        config_dir=_yaml_with(tmp_path / "b", "speculative_attention: split"))
    assert m.speculative_attention(cfg) == "forward"


@pytest.mark.parametrize("value", ["splitkv", "3", "true", "null"])
def test_bad_speculative_attention_raises_before_create_model(tmp_path, monkeypatch, value):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(ARGV + [f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, "speculative: 3", f"speculative_attention: {value}"))
    with pytest.raises(ValueError, match="speculative_attention"):
        m.speculative_attention(cfg)
    monkeypatch.setattr(m, "create_model", lambda *a, **k: pytest.fail("create_model reached with a bad trainer.speculative_attention"))
    monkeypatch.setattr(m, "load_config", lambda argv, config_dir=None: cfg)
    with pytest.raises(ValueError, match="speculative_attention"):
        m.main([])


def test_main_hands_the_attention_to_the_model(tmp_path, monkeypatch):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(ARGV + [f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, "speculative: 3", "kv_cache: fp8", "speculative_attention: split"))
    seen = {}

    class Stop(Exception):
        pass

    class Model:
        def set_decode_weights(self, kind): pass
        def set_kv_cache(self, kind): pass
        def set_prefill_chunk(self, n): pass

        def set_speculative(self, k, scope="greedy", attention="forward"):
            seen.update(k=k, scope=scope, attention=attention)
            raise Stop
    monkeypatch.setattr(m, "create_model", lambda *a, **k: Model())
    monkeypatch.setattr(m, "load_config", lambda argv, config_dir=None: cfg)
    with pytest.raises(Stop):
        m.main([])
    assert seen == dict(k=3, scope="greedy", attention="split")


def test_reference_reproduces_the_one_row_reference():
    """At seq_q = 1 with the causal rule off, the verify reference is `Case.reference()` of tests/test_gpu_decode_attention.py."""
    from test_gpu_decode_attention import Case
    from verify_attention_reference import verify_reference, visible
    c = Case(3, 8, 2, 2 * 256 + 37, [5, 256 + 9, 0], seed=8 * 1000 + 2 * 100 + 2 * 256 + 37 + 3)
    out, absv, lse = c.reference()
    got, gabs, glse = verify_reference(c.q().unsqueeze(1), c.k(), c.v(), c.kv, c.scale, causal=False)
    assert got.shape == (3, 1, 8, 128) and glse.shape == (3, 8, 1)
    assert float((got[:, 0] - out).abs().max()) <= 1e-13 and float((gabs[:, 0] - absv).abs().max()) <= 1e-13
    assert float((glse[:, :, 0] - lse).abs().max()) <= 1e-12
    # the causal rule: row j of seq_q = 4 is the one-row reference on the first seq_k - (3 - j) keys; a row in front of kv_start sees nothing
    w, sk = 4, 40
    g = torch.Generator().manual_seed(1)
    q = torch.randn(2, w, 4, 128, generator=g).bfloat16()
    k, v = torch.randn(2, sk, 2, 128, generator=g).bfloat16(), torch.randn(2, sk, 2, 128, generator=g).bfloat16()
    kv = torch.tensor([3, sk - 2], dtype=torch.int32)
    vis = visible(w, sk, kv)
    assert vis[0, 0].sum() == sk - 3 - 3 and vis[0, 3].sum() == sk - 3 and vis[1].sum(-1).tolist() == [0, 0, 1, 2]
    out, absv, lse = verify_reference(q, k, v, kv, 128 ** -0.5)
    for j in range(w):
        n = sk - (w - 1 - j)
        o1, a1, l1 = verify_reference(q[:, j:j + 1], k[:, :n], v[:, :n], kv.clamp_max(n), 128 ** -0.5, causal=False)
        assert float((out[:, j] - o1[:, 0]).abs().max()) <= 1e-13 and float((absv[:, j] - a1[:, 0]).abs().max()) <= 1e-13, j
        same_inf = torch.isinf(lse[:, :, j]) == torch.isinf(l1[:, :, 0])
        assert bool(same_inf.all()) and float((lse[:, :, j] - l1[:, :, 0]).nan_to_num(0.0, 0.0, 0.0).abs().max()) <= 1e-12, j
    assert bool((out[1, :2] == 0).all()) and bool(torch.isinf(lse[1, :, :2]).all()) and bool(torch.isfinite(lse[1, :, 2:]).all())
