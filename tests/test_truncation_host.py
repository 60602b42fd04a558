"""CPU: the instrument of test_gpu_truncation.py proved on the host, and the host side of typical_p / epsilon_cutoff / eta_cutoff.

  * tests/truncation_reference.py equals HF's TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper (float64, fed the
    post-min-p scores with -inf on removed tokens) on every case of the table: exact set equality;
  * every row of the table holds its four margins, so that kept set is unambiguous, and no row is left out;
  * the table has power: each seeded mutation of the reference changes the kept set on at least one of its rows;
  * the resolver's opt-in, HF's messages from check_truncation_args, the checks in front of any work, the chain decision, the
    trainer's forwarding, the binding and the header."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import sampling_reference as S
import truncation_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS = sorted({V for V, _ in S.VLD})


def _cases(V, profile):
    return [c for c in T.CASES if c["V"] == V and c["ld"] == next(ld for v, ld in S.VLD if v == V) and c["profile"] == profile]


def _hf_kept(case, t, kept0):
    from transformers.generation.logits_process import EpsilonLogitsWarper, EtaLogitsWarper, TypicalLogitsWarper
    sc = torch.from_numpy(np.where(kept0, np.asarray(t, dtype=np.float64), -np.inf))
    a = T.truncation_args(case)
    f32 = lambda v: float(np.float32(v))                                   # noqa: E731  (the value the kernel receives, widened)
    if a["typical_p"] < 1.0:
        sc = TypicalLogitsWarper(mass=f32(a["typical_p"]))(None, sc)
    if a["epsilon_cutoff"] > 0.0:
        sc = EpsilonLogitsWarper(epsilon=f32(a["epsilon_cutoff"]))(None, sc)
    if a["eta_cutoff"] > 0.0:
        sc = EtaLogitsWarper(epsilon=f32(a["eta_cutoff"]))(None, sc)
    return torch.isfinite(sc).numpy()


@pytest.mark.parametrize("profile", S.PROFILES)
@pytest.mark.parametrize("V", VS)
def test_reference_is_hfs_warpers_and_rows_hold_their_margins(V, profile):
    logits, hist = T.rows_for(V, profile)
    redrawn = {s: n for (v, p, s), n in T.REDRAWN.items() if (v, p) == (V, profile)}
    assert redrawn[max(redrawn)] == 0
    line, err = [], 0.0
    for case in _cases(V, profile):
        t, k0, k, m_p, m_min, mg = T.case_kept(case, logits, hist, True)
        assert float(m_p.min()) >= S.MARGIN and float(m_min.min()) >= S.MARGIN and bool(T.margins_hold(mg).all()), T.case_id(case)
        assert float(mg["b_need"].max()) < 1.0                             # the derivation's "d < D + 1" covers every row
        assert bool(k.any(1).all()) and not bool((k & ~k0).any())
        assert np.array_equal(_hf_kept(case, t, k0), k), T.case_id(case)
        if profile in S.FLAT and case.get("penalty", 1.0) == 1.0:          # all d equal: a flat row keeps every finite entry
            assert np.array_equal(k, np.isfinite(t))
        line.append(f"{case['setting']} {int(k.sum(1).min())}..{int(k.sum(1).max())}")
        err = max(err, float(mg["err_d"].max()))
    # margin (b) is max(MARGIN, 4 err_d): on the table's rows 4 err_d stays below MARGIN, so (b) is 1e-4 in effect
    assert 0.0 < 4.0 * err < S.MARGIN
    print(f"\nV={V} {profile}: redrawn per salt {redrawn}, largest err_d {err:.3g}; kept " + ", ".join(line), end="")


def test_step_7_removes_the_row_maximum_in_front_of_step_8():
    logits, hist = T.rows_for(VS[0], "randn")
    case = next(c for c in _cases(VS[0], "randn") if c["setting"] == "typical_lo_eps")
    t, k0, k = T.case_kept(case, logits, hist)
    gone = ~k[np.arange(T.ROWS), t.argmax(1)]
    assert int(gone.sum()) >= T.ROWS // 2


@pytest.mark.parametrize("mutation", T.MUTATIONS)
def test_every_mutation_changes_a_kept_set(mutation):
    for profile in ("randn", "suppressed", "two_spike", "peaked"):
        logits, hist = T.rows_for(VS[0], profile)
        for case in _cases(VS[0], profile):
            good = T.case_kept(case, logits, hist)[2]
            bad = T.case_kept(case, logits, hist, mutation=mutation)[2]
            n = int((good != bad).any(1).sum())
            if n:
                print(f"\n{mutation}: {n} of {T.ROWS} rows of {T.case_id(case)} change", end="")
                return
    raise AssertionError(f"{mutation} changes no kept set of the table")


# ------------------------------------------------------------------------------------------------ host side of the feature
def test_resolver_opt_in():
    from desta.models.modeling_desta25 import resolve_generation_kwargs as res
    file_cfg = {"typical_p": 0.9, "eta_cutoff": 0.0, "top_k": 20}
    with pytest.raises(NotImplementedError, match="typical_p=0.9"):                      # the default contract stands
        res(file_cfg)
    with pytest.raises(NotImplementedError, match="typical_p=0.9"):
        res(file_cfg, constraints=True)
    with pytest.raises(NotImplementedError, match="epsilon_cutoff"):
        res({}, epsilon_cutoff=1e-3)
    got = res(file_cfg, truncation=True, epsilon_cutoff=3e-4, max_new_tokens=9)
    assert got == dict(do_sample=False, temperature=1.0, top_k=20, top_p=1.0, min_p=None, repetition_penalty=1.0, max_new_tokens=9,
                       typical_p=0.9, epsilon_cutoff=3e-4, eta_cutoff=None)
    assert res(file_cfg, truncation=True, typical_p=0.5)["typical_p"] == 0.5             # explicit > file
    assert all(res({}, truncation=True)[k] is None for k in ("typical_p", "epsilon_cutoff", "eta_cutoff"))
    assert all(res({"typical_p": 1.0, "epsilon_cutoff": 0.0}, truncation=True, eta_cutoff=0.0)[k] is None
               for k in ("typical_p", "epsilon_cutoff", "eta_cutoff"))                   # the off values
    for combo in (dict(truncation=True), dict(truncation=True, constraints=True), dict(constraints=True), {}):
        for kw in (dict(num_beams=4), dict(top_h=0.4)):
            with pytest.raises(NotImplementedError, match=next(iter(kw))):
                res(file_cfg if combo.get("truncation") else {}, **combo, **kw)
        with pytest.raises(NotImplementedError, match="num_beams"):
            res({"num_beams": 2}, **combo)
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):               # truncation alone does not open the constraints
        res({"no_repeat_ngram_size": 3}, truncation=True)
    both = res({"no_repeat_ngram_size": 3, "eta_cutoff": 2e-3}, truncation=True, constraints=True)
    assert both["no_repeat_ngram_size"] == 3 and both["eta_cutoff"] == 2e-3
    assert "typical_p" not in res({}, top_k=5)                                           # the default output carries none of the keys


def test_check_truncation_args_speaks_hf():
    from transformers.generation.logits_process import EpsilonLogitsWarper, EtaLogitsWarper, TypicalLogitsWarper
    from desta.models.modeling_desta25 import check_truncation_args as chk, truncation_kwargs
    chk()
    chk(None, None, None)
    chk(1.0, 0.0, 0.0)
    chk(0.9, 3e-4, 2e-3)
    chk(np.float32(0.9), np.float64(3e-4), np.float32(2e-3))                             # HF takes float(v): any real scalar
    chk(np.float32(1.0), 0, np.float64(0.0))
    assert truncation_kwargs(True, np.float32(0.5), None, None)["typical_p"] == 0.5
    with pytest.raises(ValueError, match="`typical_p` has to be a float > 0 and < 1, but is 1.5"):
        chk(typical_p=np.float32(1.5))
    for name, cls, arg in (("typical_p", TypicalLogitsWarper, "mass"), ("epsilon_cutoff", EpsilonLogitsWarper, "epsilon"),
                           ("eta_cutoff", EtaLogitsWarper, "epsilon")):
        for bad in (-0.1, 1.5, 2) + ((0.0,) if name == "typical_p" else (1.0,)):
            with pytest.raises(ValueError) as hf:
                cls(**{arg: bad})
            with pytest.raises(ValueError) as ours:
                chk(**{name: bad})
            assert str(ours.value) == str(hf.value), (name, bad)
        for bad in ("0.5", True):
            with pytest.raises(ValueError, match=f"`{name}` has to be a float > 0 and < 1"):
                chk(**{name: bad})
    assert truncation_kwargs(True, 0.9, None, 2e-3) == dict(typical_p=0.9, epsilon_cutoff=0.0, eta_cutoff=2e-3)
    assert truncation_kwargs(False, 0.9, 3e-4, 2e-3) == {}                               # HF's warpers run under do_sample only
    assert truncation_kwargs(True, None, None, None) == {} == truncation_kwargs(True, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="eta_cutoff"):
        truncation_kwargs(False, eta_cutoff=1.0)                                         # ignored, but still checked


def test_generate_refuses_before_any_work_and_signatures():
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                                 # no device state: the checks come first
    for kw in (dict(typical_p=0.0), dict(epsilon_cutoff=1.0), dict(eta_cutoff=-1e-3)):
        with pytest.raises(ValueError, match=f"`{next(iter(kw))}` has to be a float > 0 and < 1"):
            model.generate([{"role": "user", "content": "hi"}], **kw)
        with pytest.raises(ValueError, match=f"`{next(iter(kw))}` has to be a float > 0 and < 1"):
            model._generate_step({}, pad_token_id=0, **kw)
    for fn in (DeSTA25AudioModel.generate, DeSTA25AudioModel._generate_step, CausalLMHIP.generate_greedy):
        sig = inspect.signature(fn).parameters
        assert all(sig[k].default is None for k in ("typical_p", "epsilon_cutoff", "eta_cutoff")), fn
    pos = [p.name for p in inspect.signature(CausalLMHIP._spec_reason).parameters.values() if p.default is inspect.Parameter.empty]
    assert pos == ["self", "k", "B", "do_sample", "use_pen", "logprobs", "forced_tokens", "layer_hook"]


class _StubModel:
    def __init__(self):
        self.calls = []

    def _generate_step(self, batch, **kw):
        self.calls.append(kw)
        return torch.tensor([[11, 7, 0, 0], [12, 13, 14, 15]])


def test_predict_step_forwards_the_three_keys_when_set():
    from desta.trainer import desta_trainer as DT
    tr = DT.DeSTA25Trainer.__new__(DT.DeSTA25Trainer)
    model = _StubModel()
    tr.model, tr.cfg, tr.processing_class, tr.global_step, tr.prediction_step_outputs = model, None, None, 0, []
    batch = {"context_input_ids": torch.tensor([[3, 4], [5, 6]]), "labels": torch.tensor([[-100, 8], [9, 10]]), "metadata": [{"id": "a"}, {"id": "b"}]}
    tr._predict_step(batch, dict(max_new_tokens=4, do_sample=True))
    assert not {"typical_p", "epsilon_cutoff", "eta_cutoff"} & set(model.calls[0])       # not set: not passed
    tr._predict_step(batch, dict(max_new_tokens=4, do_sample=True, typical_p=0.9, eta_cutoff=2e-3))
    assert model.calls[1]["typical_p"] == 0.9 and model.calls[1]["eta_cutoff"] == 2e-3 and "epsilon_cutoff" not in model.calls[1]
    tr._predict_step(batch, dict(epsilon_cutoff=3e-4))
    assert model.calls[2]["epsilon_cutoff"] == 3e-4


# ------------------------------------------------------------------------------------------------ kernel, binding and header
def test_chain_kernels_use_no_scratch():
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    hits = {n: r for n, r in mod.kernel_resources().items() if "sample_chain_k" in n or "sample_truncated_k" in n}
    assert len(hits) == 2, sorted(hits)                                                  # the chain, without and with steps 7-9
    for n, r in hits.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (n, r)


def test_abi_declares_and_binds_the_symbol():
    from desta import _hip as h
    hdr = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    assert re.search(r"#define DESTA_ABI_VERSION 8\b", hdr) and h.ABI_VERSION == 8 and h.lib.desta_abi_version() == 8
    rows = re.search(r"int desta_sample_rows_bf16\(([^;]*)\);", hdr)
    m = re.search(r"int desta_sample_truncated_rows_bf16\(([^;]*)\);", hdr)
    norm = lambda s: re.sub(r"\s+", " ", s)                                              # noqa: E731
    assert m and norm(m.group(1)) == norm(rows.group(1)).replace("float min_p,", "float min_p, float typical_p, float epsilon_cutoff, float eta_cutoff,")
    doc = hdr[hdr.index("desta_sample_rows_bf16 with HF's truncation warpers"):hdr.index("int desta_sample_truncated_rows_bf16")]
    doc = norm(doc.replace("\n *", " "))
    for word in ("TypicalLogitsWarper", "EpsilonLogitsWarper", "EtaLogitsWarper", "|a_i - c|", "tied with D", "OF THOSE SURVIVORS",
                 "bit-identical", "DESTA_EINVAL"):
        assert word in doc, word
    assert h._sample_truncated_rows.argtypes == h._sample_rows.argtypes[:16] + [h.f32] * 3 + h._sample_rows.argtypes[16:]
    for fn in (h.sample, h.sample_rows):
        sig = inspect.signature(fn).parameters
        assert (sig["typical_p"].default, sig["epsilon_cutoff"].default, sig["eta_cutoff"].default) == (1.0, 0.0, 0.0)
    assert isinstance(h.SAMPLE_TRUNCATED_CALLS, int)
