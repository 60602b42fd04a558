"""CPU-only: the wide (17 <= M <= 64) decode projection is declared, exported and bound, and every instantiation of its kernel keeps
its accumulators and both load stages in registers."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_gemm_wide_at_abi_8():
    import torch  # noqa: F401  (same load order as the product path)
    from desta import _hip
    hdr = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    assert re.search(r"\bint desta_gemm_wide_nt\(const desta_gemm_desc\* d, const float\* b_scale, void\* stream\);", hdr)
    assert int(re.search(r"#define DESTA_ABI_VERSION (\d+)", hdr).group(1)) == 8 == _hip.ABI_VERSION == _hip.lib.desta_abi_version()
    assert hasattr(_hip.lib, "desta_gemm_wide_nt")


def test_binding_has_gemm_wide_and_the_row_limit():
    from desta import _hip
    assert callable(_hip.gemm_wide) and _hip.DECODE_MAX_ROWS == 64 and isinstance(_hip.GEMM_WIDE_CALLS, int)
    from desta.models.modeling_desta25 import check_decode_rows
    check_decode_rows(64)
    try:
        check_decode_rows(65)
    except ValueError as e:
        assert "64" in str(e)
    else:
        raise AssertionError("65 rows accepted")


def test_wide_kernel_uses_no_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources().items() if "gemm_bf16_nt_skinny_wide" in n}
    main = {n: r for n, r in res.items() if "fixup" not in n}
    assert len(main) == 12 and len(res) == 14                                # MF 2..4 x SwiGLU x FP8, and the two fix-up forms
    for name in sorted(res):
        r = res[name]
        print(f"{name[:80]:80s} vgpr {r['vgpr']:3d} sgpr {r['sgpr']:3d} lds {r['lds']:6d} scratch {r['scratch']} spilled {r['spill']}")
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)
        assert r["vgpr"] <= 256 and r["lds"] <= 160 * 1024, (name, r)        # one 512-thread block per CU
