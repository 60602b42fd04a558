"""CPU-only: the opt-in row ceiling of a KV-cached step (`set_decode_rows`), the limits derived from it, the prompt-chunk rule above
64 sequences, the trainer's config key, and the resources of every instantiation of the tall (65 <= M <= 256) projection kernel."""
import importlib.util
import os
import re
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _llm():
    from desta.models.modeling_desta25 import CausalLMHIP
    llm = CausalLMHIP.__new__(CausalLMHIP)                                   # the settings alone: no weights, no device
    llm.decode_rows, llm.decode_weights, llm.kv_cache_kind, llm.prefill_chunk = None, "bf16", "bf16", None
    llm.hq = llm.hkv = 4
    return llm


def test_header_declares_and_library_exports_gemm_tall_at_abi_8():
    import torch  # noqa: F401  (same load order as the product path)
    from desta import _hip
    hdr = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    assert re.search(r"\bint desta_gemm_tall_nt\(const desta_gemm_desc\* d, const float\* b_scale, void\* stream\);", hdr)
    assert int(re.search(r"#define DESTA_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _hip.ABI_VERSION == _hip.lib.desta_abi_version()
    assert hasattr(_hip.lib, "desta_gemm_tall_nt") and callable(_hip.gemm_tall) and isinstance(_hip.GEMM_TALL_CALLS, int)
    assert _hip.DECODE_MAX_ROWS == 64 and _hip.DECODE_TALL_MAX_ROWS == 256


def test_set_decode_rows_accepts_and_rejects():
    llm = _llm()
    for n, limit in ((None, 64), (64, 64), (65, 65), (256, 256)):
        llm.set_decode_rows(n)
        assert llm.row_limit == limit
    for bad in (63, 257, 100.5, True, 0, "128"):
        with pytest.raises(ValueError, match="decode_rows"):
            llm.set_decode_rows(bad)
        assert llm.row_limit == 256                                          # a refused value leaves the setting as it was
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)
    model.llm = llm
    model.set_decode_rows(128)
    assert llm.row_limit == 128
    with pytest.raises(ValueError, match="decode_rows"):
        model.set_decode_rows(300)
    assert llm.row_limit == 128


def test_check_decode_rows_takes_the_ceiling():
    from desta.models.modeling_desta25 import check_decode_rows
    check_decode_rows(200, limit=256)
    check_decode_rows(256, guided=True, limit=256)
    with pytest.raises(ValueError, match="a batch of 257 sequences.*at most 256"):
        check_decode_rows(257, limit=256)
    with pytest.raises(ValueError, match="129 sequences are 258 rows.*at most 256"):
        check_decode_rows(258, guided=True, limit=256)
    llm = _llm()
    llm.set_decode_rows(256)
    llm.check_rows(200)
    with pytest.raises(ValueError, match="256"):
        llm.check_rows(257)
    llm.decode_weights = "mxfp4"
    llm.check_rows(64)
    with pytest.raises(ValueError, match="MXFP4"):
        llm.check_rows(65)
    llm.set_decode_rows(None)
    with pytest.raises(ValueError, match="at most 64"):                      # a default model: today's message, whatever the weights
        llm.check_rows(65)


def test_spec_reason_takes_the_ceiling():
    llm = _llm()
    args = (False, False, None, None, None)
    assert llm._spec_reason(3, 17, *args) == "B * (k + 1) = 68 rows > 64"
    llm.set_decode_rows(256)
    assert llm._spec_reason(3, 17, *args) is None
    assert llm._spec_reason(3, 64, *args) is None
    assert llm._spec_reason(3, 65, *args) == "B * (k + 1) = 260 rows > 256"
    llm.decode_weights = "mxfp4"                                             # no MXFP4 kernel above 64 rows: the plain loop
    assert llm._spec_reason(3, 17, *args) == "B * (k + 1) = 68 rows > 64"


def test_prefill_chunk_rule():
    from desta.models.modeling_desta25 import TALL_PREFILL_ROWS, tall_prefill_chunk
    assert TALL_PREFILL_ROWS == 16384
    assert [tall_prefill_chunk(B) for B in (65, 128, 256)] == [240, 128, 64]
    for B in (65, 72, 100, 128, 200, 256):
        c = tall_prefill_chunk(B)
        assert c % 16 == 0 and B * c <= TALL_PREFILL_ROWS < B * (c + 16)
    assert all(tall_prefill_chunk(B) is None for B in (1, 16, 17, 63, 64))
    llm = _llm()
    assert llm._prompt_chunk(64) is None and llm._prompt_chunk(128) == 128
    llm.prefill_chunk = 32                                                   # an explicit `set_prefill_chunk` wins
    assert llm._prompt_chunk(64) == 32 and llm._prompt_chunk(128) == 32


def test_trainer_reads_decode_rows():
    from desta.trainer.desta_trainer import DeSTA25Trainer
    seen = []
    model = types.SimpleNamespace(set_decode_rows=seen.append)
    ns = types.SimpleNamespace
    assert DeSTA25Trainer._apply_decode_rows(model, ns(trainer=ns(decode_rows=128))) == 128
    assert DeSTA25Trainer._apply_decode_rows(model, {"trainer": {"decode_rows": 256}}) == 256
    assert seen == [128, 256]
    for cfg in (None, ns(), ns(trainer=ns()), {"trainer": {}}, ns(trainer=ns(decode_rows=None))):
        assert DeSTA25Trainer._apply_decode_rows(model, cfg) is None
    assert seen == [128, 256]


def test_tall_kernel_uses_no_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources().items() if "gemm_bf16_nt_skinny_tall" in n}
    assert len(res) == 8                                                     # 2 / 4 row groups x SwiGLU x FP8
    for name in sorted(res):
        r = res[name]
        print(f"{name[:80]:80s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} lds {r['lds']:6d} scratch {r['scratch']} spilled {r['spill']}")
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["vgpr"] <= 256 and r["lds"] <= 160 * 1024, (name, r)        # one 512-thread block per CU


def test_bf16_routing_rule_is_of_the_shape_alone():
    """The measured routing of DESIGN "Decode at batch 65–256": which bf16 projections of a tall step take the tile GEMM."""
    from desta.models.modeling_desta25 import tall_rows_to_gemm
    for M in (65, 128, 192, 256):
        assert tall_rows_to_gemm(M, 2 * 14336) and tall_rows_to_gemm(M, 128256)          # gate|up, lm_head
        assert not tall_rows_to_gemm(M, 4096)                                            # o, down
        assert tall_rows_to_gemm(M, 6144) == (M > 128)                                   # q|k|v
    assert not tall_rows_to_gemm(256, 512)                                               # the tiny test models stay on gemm_tall
