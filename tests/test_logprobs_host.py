"""CPU: the host side of token log-probabilities — `desta_token_logprobs` in the header at an unchanged ABI version, its
binding, `score()`'s argument checks (before any device work) and the register budget of the kernel."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_token_logprobs_at_abi_8():
    txt = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+desta_token_logprobs\s*\(\s*const void\*\s*logits_bf16,\s*int64_t ld,\s*const int64_t\*\s*labels,\s*int rows,\s*int vocab,"
                     r"\s*float\*\s*logprob,\s*uint8_t\*\s*is_top1\s*,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"#define DESTA_ABI_VERSION (\d+)", txt).group(1) == "8"
    assert "TF:loss/loss_utils.py:49-71" in txt and "READ ONLY" in txt and "compact_labels + 1" in txt


def test_binding_exports_token_logprobs():
    import ctypes as C
    from desta import _hip
    assert _hip.ABI_VERSION == 8 and _hip.lib.desta_abi_version() == 8
    fn = _hip.lib.desta_token_logprobs
    assert fn.argtypes == [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] and fn.restype == C.c_int
    assert callable(_hip.token_logprobs)


@pytest.mark.parametrize("choices,normalize,match", [(["a", "b"], "max", "normalize"), ([], "sum", "non-empty"), (["a", ""], "mean", "non-empty string"),
                                                     ("ab", "sum", "list"), (["a", 3], "sum", "non-empty string")])
def test_score_rejects_bad_arguments_without_gpu(choices, normalize, match):
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                    # no device state, no tokenizer: the checks come first
    with pytest.raises(ValueError, match=match):
        model.score([{"role": "user", "content": "which one?"}], choices, normalize=normalize)


def test_token_logprob_kernel_uses_no_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources().items() if "token_logprob_k" in n}
    assert len(res) == 1, sorted(res)
    for n, r in res.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (n, r)
        assert r["vgpr"] <= 64, (n, r)                                      # two 1024-thread blocks per CU
