"""Host side of classifier-free guidance (`generate(guidance_scale=)`, `desta_cfg_scores_bf16`): the reference formula against the
installed transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor, the argument checks, the derived negative prompt, the
speculation fallback, the new kernel's resources and the ABI."""
import copy
import importlib.util
import os
import re
import types

import pytest
import torch

import guidance_reference as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------ the formula is HF's
class _StubLM:
    """Stands where HF expects the model: returns fixed unconditional logits [B, S, V] for whatever it is called with."""

    def __init__(self, logits):
        self.logits, self.calls = logits, 0

    def __call__(self, input_ids, attention_mask=None, use_cache=True, past_key_values=None):
        self.calls += 1
        return types.SimpleNamespace(logits=self.logits, get=lambda key, default=None: default)


@pytest.mark.parametrize("g", [1.5, 3.0])
def test_reference_formula_is_hfs_processor(g):
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    gen = torch.Generator().manual_seed(11)
    B, V = 3, 1000
    cond = (3.0 * torch.randn(B, V, generator=gen)).to(torch.bfloat16)
    uncond = (3.0 * torch.randn(B, 4, V, generator=gen)).to(torch.bfloat16)                 # the processor reads the last position
    cond[1, ::7] = GR.NEG_INF                                                                # conditional -inf: HF gives -inf as well
    stub = _StubLM(uncond.float())
    proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(g, stub, unconditional_ids=torch.zeros(B, 4, dtype=torch.long))
    got = proc(torch.zeros(B, 1, dtype=torch.long), cond.float()).double()
    assert stub.calls == 1
    R, Lc, Lu = GR.guided_scores_fp64(cond, uncond[:, -1], g)
    dead = torch.isinf(R)
    assert bool(dead[1, ::7].all()) and int(dead.sum()) == len(range(0, V, 7))
    assert torch.equal(got[dead], R[dead])
    # HF works in fp32: two log-softmaxes (a few ulp of |lp| each, the sum over V = 1000 entries included) and the three
    # roundings of the combination; 1e-5 + 2^-20 |.| per log-softmax is generous for that and far below any modelling difference
    lp = lambda L: 1e-5 + 2.0 ** -20 * L.abs()
    tol = (g * (lp(Lc) + lp(Lu)) + lp(Lu) + 2.0 ** -22 * (g * (Lc - Lu).abs() + R.abs()))[~dead]
    assert bool(((got - R).abs()[~dead] <= tol).all()), float(((got - R).abs()[~dead] / tol).max())
    # scale 1: HF returns the conditional log-softmax and never runs the model; the formula gives the same
    stub1 = _StubLM(uncond.float())
    one = UnbatchedClassifierFreeGuidanceLogitsProcessor(1.0, stub1)(torch.zeros(B, 1, dtype=torch.long), cond.float()).double()
    R1, Lc1, _ = GR.guided_scores_fp64(cond, uncond[:, -1], 1.0)
    assert stub1.calls == 0 and bool(((one - R1).abs()[~dead] <= 3 * lp(Lc1)[~dead]).all())


def test_reference_minus_inf_rule_and_bound():
    cond = torch.tensor([[1.0, GR.NEG_INF, 0.5, GR.NEG_INF, 2.0]]).to(torch.bfloat16)
    uncond = torch.tensor([[0.5, 1.0, GR.NEG_INF, GR.NEG_INF, 2.0]]).to(torch.bfloat16)
    R, Lc, Lu = GR.guided_scores_fp64(cond, uncond, 3.0)
    assert R[0, 1:4].tolist() == [GR.NEG_INF] * 3 and bool(torch.isfinite(R[0, [0, 4]]).all()) and not bool(torch.isnan(R).any())
    b = GR.guided_bound(R, Lc, Lu, 3.0)
    assert bool(torch.isfinite(b).all()) and bool((b > 0).all())
    # the bf16 term dominates: just above 2^-8 |R| for an ordinary entry
    assert float(b[0, 0]) < 2.0 ** -8 * abs(float(R[0, 0])) + 2e-4


# ------------------------------------------------------------------------------------------------ arguments
def test_check_guidance_arg():
    from desta.models.modeling_desta25 import check_guidance_arg
    for ok in (None, 1, 1.0, 1.5, 3, 0.25, 1e-3, 100.0):
        check_guidance_arg(ok)
    for bad in (0, 0.0, -1.5, float("inf"), float("nan"), True, False, "2", [2.0], (1.5,)):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            check_guidance_arg(bad)


@pytest.mark.parametrize("case", sorted(GR.NEGATIVE_CASES))
def test_guidance_negative_messages(case):
    from desta.models.modeling_desta25 import guidance_negative_messages
    messages, want = GR.NEGATIVE_CASES[case]
    before = copy.deepcopy(messages)
    got = guidance_negative_messages(messages, GR.LOC)
    assert got == want
    assert messages == before                                                                # the input is left as it was
    flat = lambda ms: [m for c in ([ms] if isinstance(ms[0], dict) else ms) for m in c]
    assert all(a is not b for a, b in zip(flat(got), flat(messages)))                        # copies, not the caller's dicts
    assert all("audios" not in m and GR.LOC not in m["content"] for m in flat(got))


def _bare_model():
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                                     # no device state: the checks come first
    llm = model.llm = CausalLMHIP.__new__(CausalLMHIP)
    llm.speculative = llm._spec = None
    llm.spec_scope = "greedy"
    llm.kv_cache_kind = "bf16"
    model.audio_locator = GR.LOC
    return model, llm


def test_generate_refuses_before_any_work():
    model, _ = _bare_model()
    audio_chat = [[{"role": "user", "content": f"hear {GR.LOC}", "audios": [{"audio": "a.wav", "text": "x"}]}],
                  [{"role": "user", "content": f"and {GR.LOC}", "audios": [{"audio": "b.wav", "text": "y"}]}]]
    text_chat = [[{"role": "user", "content": "hi there"}]]
    with pytest.raises(ValueError, match="1 conversations for 2"):                           # count mismatch
        model.generate(audio_chat, do_sample=False, guidance_scale=2.0, negative_messages=[[{"role": "user", "content": "hear"}]])
    with pytest.raises(ValueError, match="no audio"):                                        # the derived negative would be the prompt
        model.generate(text_chat, do_sample=False, guidance_scale=2.0)
    with pytest.raises(ValueError, match="no audio"):
        model.generate(text_chat[0], do_sample=False, guidance_scale=2.0)
    for bad in (0.0, -2.0, True, float("nan")):
        with pytest.raises(ValueError, match="guidance_scale"):
            model.generate(audio_chat, do_sample=False, guidance_scale=bad)
        with pytest.raises(ValueError, match="guidance_scale"):
            model._generate_step({}, pad_token_id=0, guidance_scale=bad)


def test_row_limit_message_names_the_doubling():
    from desta import _hip
    from desta.models.modeling_desta25 import check_decode_rows
    check_decode_rows(_hip.DECODE_MAX_ROWS, guided=True)
    with pytest.raises(ValueError, match=r"guidance_scale doubles the rows.*33 sequences are 66 rows"):
        check_decode_rows(66, guided=True)
    with pytest.raises(ValueError, match="a batch of 66 sequences"):                         # the plain message is unchanged
        check_decode_rows(66)


def test_spec_reason_for_a_guided_call():
    model, llm = _bare_model()
    for scope in ("greedy", "all"):
        llm.set_speculative(3, scope=scope)
        assert llm._spec_reason(3, 4, False, False, None, None, None, guided=True) == "guidance_scale"
        assert llm._spec_reason(3, 4, True, True, 2, object(), object(), guided=True) == "guidance_scale"    # in front of every other reason
        assert llm._spec_reason(3, 4, False, False, None, None, None, guided=False) is None
    llm.set_speculative(3)
    assert llm._spec_reason(3, 3, False, False, None, None, None) is None                    # the five-argument positional form
    assert llm._spec_reason(3, 3, True, False, None, None, None) == "do_sample"


# ------------------------------------------------------------------------------------------------ kernel and ABI
def test_kernel_uses_no_scratch():
    res = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources()
    hits = {n: r for n, r in res.items() if "cfg_scores_k" in n}
    assert len(hits) == 1, sorted(hits)
    (name, r), = hits.items()
    assert r["scratch"] == 0 and r["spill"] == 0, (name, r)


def test_abi_declares_and_binds_the_symbol():
    from desta import _hip
    hdr = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    assert re.search(r"#define DESTA_ABI_VERSION 8\b", hdr) and _hip.ABI_VERSION == 8 and _hip.lib.desta_abi_version() == 8
    m = re.search(r"int desta_cfg_scores_bf16\(([^;]*)\);", hdr)
    assert m and re.sub(r"\s+", " ", m.group(1)) == ("const void* cond_bf16, const void* uncond_bf16, int64_t ld, int rows, int vocab, "
                                                     "float guidance_scale, void* out_bf16, int64_t ld_out, void* stream")
    assert "UnbatchedClassifierFreeGuidanceLogitsProcessor" in hdr and "_get_logits_processor" in hdr
    assert _hip._cfg_scores.argtypes == [_hip.vp, _hip.vp, _hip.i64, _hip.i32, _hip.i32, _hip.f32, _hip.vp, _hip.i64, _hip.vp]
    assert callable(_hip.cfg_scores) and isinstance(_hip.CFG_SCORES_CALLS, int)
