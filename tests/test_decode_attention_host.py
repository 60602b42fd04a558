"""CPU-only: the split-KV decode attention is declared, exported and bound at ABI 8, its dispatch constants are sane, and every
instantiation of its kernels keeps the streamed K / V, the scores and the accumulators in registers."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_decode_attention_at_abi_8():
    import torch  # noqa: F401  (same load order as the product path)
    from desta import _hip
    hdr = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    assert re.search(r"\bsize_t\s+desta_attention_decode_workspace_bytes\(int batch, int n_q_heads, int seq_k, int head_dim\);", hdr)
    assert re.search(r"\bint\s+desta_attention_decode\(const desta_attn_desc\* d, void\* workspace, size_t workspace_bytes, void\* stream\);", hdr)
    chunk = int(re.search(r"#define DESTA_ATTN_DECODE_CHUNK (\d+)", hdr).group(1))
    assert chunk == _hip.DECODE_ATTN_CHUNK == _hip.lib.desta_attention_decode_chunk()
    assert int(re.search(r"#define DESTA_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _hip.ABI_VERSION == _hip.lib.desta_abi_version()
    assert hasattr(_hip.lib, "desta_attention_decode") and hasattr(_hip.lib, "desta_attention_decode_workspace_bytes")
    assert "modeling_desta25.py:1419" in hdr[hdr.index("Split-KV GQA decode attention"):hdr.index("#define DESTA_ATTN_DECODE_CHUNK")]


def test_binding_has_decode_attention_and_its_constants():
    from desta import _hip
    assert callable(_hip.attention_decode) and callable(_hip.attention_decode_workspace_bytes)
    assert _hip.DECODE_ATTN_CHUNK % 64 == 0 and _hip.DECODE_ATTN_CHUNK in (128, 256)
    assert _hip.DECODE_ATTN_MIN_KEYS >= 256 and _hip.DECODE_ATTN_MIN_KEYS % 64 == 0
    assert isinstance(_hip.ATTN_DECODE_CALLS, int)


def test_workspace_size_is_host_arithmetic():
    from desta import _hip
    CH = _hip.DECODE_ATTN_CHUNK
    assert _hip.attention_decode_workspace_bytes(3, 8, CH) == 0              # one chunk: the main kernel finishes the row
    for n in (2, 3, 7):
        items = 3 * 8 * n
        want = 4 * ((2 * items + 3) // 4 * 4 + 128 * items)                  # (max, sum) pairs padded to 16 bytes + fp32 O per item
        assert _hip.attention_decode_workspace_bytes(3, 8, (n - 1) * CH + 1) == want == _hip.attention_decode_workspace_bytes(3, 8, n * CH)


def test_decode_attention_kernels_use_no_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources().items() if "attn_decode" in n}
    main = {n: r for n, r in res.items() if "combine" not in n}
    assert len(main) == 4 and len(res) == 5                                  # groups padded to 1, 2, 4, 8 query rows, and the combine
    for name in sorted(res):
        r = res[name]
        print(f"{name[:80]:80s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} lds {r['lds']:6d} scratch {r['scratch']} spilled {r['spill']}")
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["vgpr"] <= 256 and r["lds"] <= 64 * 1024, (name, r)
