"""CPU: the host side of generate()'s log-probabilities — `desta_topk_logprobs` in the header at an unchanged ABI version, its binding,
the `logprobs=` argument check (before any device work), `GenerationOutput`'s new fields, the kernel's register budget, and the
trainer's prediction rows with a stub model."""
import importlib.util
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_topk_logprobs_at_abi_8():
    txt = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+desta_topk_logprobs\s*\(\s*const void\*\s*logits_bf16,\s*int64_t ld,\s*const int64_t\*\s*tokens\s*,\s*int rows,\s*int vocab,"
                     r"\s*int top_n,\s*float\*\s*token_logprob\s*,\s*int32_t\*\s*top_ids\s*,\s*float\*\s*top_logprobs\s*,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"#define DESTA_ABI_VERSION (\d+)", txt).group(1) == "8"
    assert "modeling_desta25.py:1419-1427" in txt and "compute_transition_scores" in txt and "output_logits" in txt


def test_binding_exports_topk_logprobs():
    import ctypes as C
    from desta import _hip
    assert _hip.ABI_VERSION == 8 and _hip.lib.desta_abi_version() == 8
    fn = _hip.lib.desta_topk_logprobs
    assert fn.argtypes == [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn.restype == C.c_int and fn is _hip._topk_logprobs
    assert callable(_hip.topk_logprobs) and _hip.TOPK_LOGPROBS_MAX == 32 and isinstance(_hip.TOPK_LOGPROBS_CALLS, int)


def test_check_logprobs_arg():
    from desta.models.modeling_desta25 import DeSTA25AudioModel, check_logprobs_arg
    for ok in (None, 0, 5, 32):
        check_logprobs_arg(ok)
        DeSTA25AudioModel.check_logprobs_arg(ok)
    for bad in (-1, 33, 2.5, True, "5"):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            check_logprobs_arg(bad)
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                    # no device state, no tokenizer: the check comes first
    for bad in (33, True):
        with pytest.raises(ValueError, match="logprobs"):
            model.generate([{"role": "user", "content": "hi"}], logprobs=bad)
        with pytest.raises(ValueError, match="logprobs"):
            model._generate_step({}, pad_token_id=0, logprobs=bad)


def test_generation_output_keeps_its_constructor():
    from desta.models.modeling_desta25 import GenerationOutput, TokenLogprobs
    out = GenerationOutput(audios=[], generated_ids=[], text=[])
    assert out.token_logprobs is None and out.top_logprobs is None and out.sum_logprob is None
    assert [f for f in GenerationOutput.__dataclass_fields__] == ["audios", "generated_ids", "text", "token_logprobs", "top_logprobs", "sum_logprob"]
    assert GenerationOutput(["a"], [[1]], ["t"]).text == ["t"]                # positional order unchanged
    assert [f for f in TokenLogprobs.__dataclass_fields__] == ["token_logprobs", "top_ids", "top_logprobs"]


def test_topk_logprob_kernel_uses_no_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = {n: r for n, r in mod.kernel_resources().items() if "topk_logprob_k" in n}
    assert len(res) == 1, sorted(res)
    for n, r in res.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (n, r)
        assert r["vgpr"] <= 64, (n, r)                                      # two 1024-thread blocks per CU


class _StubModel:
    """`_generate_step` of a model that emits fixed rows: row 0 ends with EOS (7) at its second token."""
    class config:
        class llm_config:
            eos_token_id = 7

    def __init__(self):
        self.calls = []

    def _generate_step(self, batch, **kw):
        from desta.models.modeling_desta25 import TokenLogprobs
        self.calls.append(kw)
        ids = torch.tensor([[11, 7, 0, 0], [12, 13, 14, 15]])
        if kw.get("logprobs") is None:
            return ids
        n = kw["logprobs"]
        lp = torch.tensor([[-0.5, -1.5, 0.0, 0.0], [-1.0, -2.0, -3.0, -4.0]])
        return ids, TokenLogprobs(token_logprobs=lp, top_ids=torch.zeros(2, 4, n, dtype=torch.int32), top_logprobs=torch.zeros(2, 4, n))


class _Tok:
    eos_token_id = 2

    def batch_decode(self, x, skip_special_tokens=False):
        return [" ".join(str(int(t)) for t in row) for row in x]


def _trainer(model, tok):
    from desta.trainer import desta_trainer as T
    tr = T.DeSTA25Trainer.__new__(T.DeSTA25Trainer)
    tr.model, tr.cfg, tr.processing_class, tr.global_step, tr.prediction_step_outputs = model, None, tok, 0, []
    return tr


def test_predict_step_rows_with_and_without_logprobs():
    batch = {"context_input_ids": torch.tensor([[3, 4], [5, 6]]), "labels": torch.tensor([[-100, 8], [9, 10]]), "metadata": [{"id": "a"}, {"id": "b"}]}
    model = _StubModel()
    tr = _trainer(model, _Tok())
    ids = tr._predict_step(batch, dict(max_new_tokens=4, do_sample=False))
    assert torch.is_tensor(ids) and ids.shape == (2, 4) and "logprobs" not in model.calls[0]
    assert [set(o) for o in tr.prediction_step_outputs] == [{"context", "prediction", "label", "id"}] * 2
    tr.prediction_step_outputs = []
    ids = tr._predict_step(batch, dict(max_new_tokens=4, do_sample=False, logprobs=2))
    assert torch.is_tensor(ids) and ids.shape == (2, 4) and model.calls[1]["logprobs"] == 2
    a, b = tr.prediction_step_outputs
    assert set(a) == set(b) == {"context", "prediction", "label", "id", "avg_logprob", "token_logprobs"}
    assert a["token_logprobs"] == [-0.5, -1.5] and a["avg_logprob"] == -1.0           # cut behind the EOS, which is scored
    assert b["token_logprobs"] == [-1.0, -2.0, -3.0, -4.0] and b["avg_logprob"] == -2.5
    assert a["id"] == "a" and a["prediction"] == "11 7 0 0"
    # without a tokenizer the id rows carry the same two keys
    tr2 = _trainer(model, None)
    tr2._predict_step(batch, dict(logprobs=0))
    assert set(tr2.prediction_step_outputs[0]) == {"id", "prediction_ids", "avg_logprob", "token_logprobs"}
