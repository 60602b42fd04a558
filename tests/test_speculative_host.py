"""CPU: the host side of draft-and-verify decoding — the reference loop (tests/speculative_reference.py) against token-by-token
greedy on a toy model, the two C entry points in the header and the library at an unchanged ABI version, the binding, the
`speculative` argument check of the model and of the entry point's `trainer.speculative` key."""
import importlib.util
import os
import random
import re

import pytest

import speculative_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS, PAD, VOCAB = 5, 0, 11


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _next_token(seed):
    """A deterministic toy model: the next id is a hash of the last three tokens and the history's length; never PAD."""
    def f(h):
        x = seed
        for t in h[-3:]:
            x = (x * 1000003 + t + 1) % 2147483647
        x = (x * 31 + len(h)) % 2147483647
        return 1 + x % (VOCAB - 1)
    return f


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("source", ["random", "perfect", "none", "mixed", "lookup"])
def test_reference_loop_equals_token_by_token_greedy(source, k, B):
    T, S = 24, 9
    for seed in range(6):
        rng = random.Random(seed * 100 + k * 10 + B)
        nt = _next_token(seed)
        prompts = [[rng.randrange(1, VOCAB) for _ in range(S)] for _ in range(B)]
        eos = [EOS] if seed % 2 else []                                      # odd seeds: rows finish, some inside an accepted run
        want = SR.greedy_loop(nt, prompts, T, eos, PAD)

        def drafts(b, n, hist):
            if source == "perfect" or (source == "mixed" and b % 2 == 0):
                return (want[b] + [-1] * k)[n:n + k]
            if source == "random" or source == "mixed":
                return [rng.randrange(-1, VOCAB) for _ in range(k)]
            if source == "lookup":
                return SR.ngram_draft(hist, len(hist), 0, k, 3, 1)
            return [-1] * k
        got, steps = SR.speculative_loop(nt, prompts, T, k, drafts, eos, PAD)
        assert got == want, (source, k, B, seed)
        if not eos and source == "perfect":
            assert steps == -(-(T - 1) // (k + 1))
        if not eos and source == "none":
            assert steps == T - 1


def test_reference_loop_finishes_a_row_inside_an_accepted_run():
    """Row 0 meets its EOS at emitted position 2, inside a fully accepted chunk of perfect drafts; row 1 goes on."""
    script = {0: [3, 4, EOS], 1: [6, 7, 8, 9, 6, 7, 8, 9]}
    prompts = [[1, 0], [1, 1]]

    def nt(h):
        row = h[1]
        return script[row][(len(h) - 2) % len(script[row])]
    want = SR.greedy_loop(nt, prompts, 8, [EOS], PAD)
    assert want[0] == [3, 4, EOS] + [PAD] * 5 and PAD not in want[1]
    got, steps = SR.speculative_loop(nt, prompts, 8, 3, lambda b, n, hist: (want[b] + [-1] * 3)[n:n + 3], [EOS], PAD)
    assert got == want and steps == 2                                       # 1 + 4 + 3: the finished row limits nobody


def test_reference_rules_on_hand_cases():
    assert SR.ngram_draft([1, 2, 3, 9, 1, 2, 3, 8, 2, 3], 10, 0, 3, 2, 1) == [8, 2, 3]       # two matches of (2, 3): the later one wins
    assert SR.ngram_draft([1, 2, 3, 9, 7, 3, 8, 2, 3], 9, 0, 2, 2, 1) == [9, 7]              # n = 2 at i = 1 beats the later n = 1 match
    assert SR.ngram_draft([4, 5, 6, 4, 5], 5, 1, 3, 2, 2) == [-1, -1, -1]                    # row_start inside the only n = 2 match
    assert SR.ngram_draft([4, 5, 6, 4, 5], 5, 1, 3, 2, 1) == [6, 4, 5]                       # ... n = 1 then finds the 5 at 1
    assert SR.ngram_draft([4, 5, 6, 4, 5], 5, 0, 3, 2, 1) == [6, 4, 5]
    assert SR.ngram_draft([4, 5, 4, 5], 4, 0, 3, 2, 2) == [4, 5, -1]                         # the continuation runs into hist_len
    assert SR.ngram_draft([4, -1, 6, 4, -1], 5, 0, 2, 2, 1) == [-1, -1]                      # negative ids never match
    assert SR.ngram_draft([7], 1, 0, 2, 3, 1) == [-1, -1]
    out, fin, nxt, a = SR.accept([[1, 2, 3, 4], [5, 6, 7, 8]], [[9, 1, 2, 0], [9, 5, -1, 7]], [False, False], [], PAD, 4)
    assert (out, fin, nxt, a) == ([[1, 2], [5, 6]], [False, False], [2, 6], 2)               # m = 2 and m = 1
    out, fin, nxt, a = SR.accept([[1, EOS, 3, 4], [6, 7, 8, 9]], [[9, 1, EOS, 3], [9, 6, 7, 8]], [False, False], [EOS], PAD, 4)
    assert (out, fin, nxt, a) == ([[1, EOS, PAD, PAD], [6, 7, 8, 9]], [True, False], [PAD, 9], 4)


def test_reference_draft_row_start_case():
    assert SR.ngram_draft([4, 5, 6, 4, 5], 5, 2, 3, 2, 1) == [-1, -1, -1]


def test_header_declares_and_library_exports_the_speculative_entry_points_at_abi_8():
    import torch  # noqa: F401  (same load order as the product path)
    from desta import _hip
    txt = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+desta_spec_ngram_draft\s*\(\s*const int64_t\*\s*hist,\s*int64_t hist_ld,\s*int batch,\s*int hist_len,\s*"
                     r"const int32_t\*\s*row_start,\s*int k,\s*int n_max,\s*int n_min,\s*int64_t\*\s*draft,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"int\s+desta_spec_accept\s*\(\s*const int64_t\*\s*pred,\s*const int64_t\*\s*inp,\s*int batch,\s*int k,\s*uint8_t\*\s*finished,\s*"
                     r"const int64_t\*\s*eos,\s*int n_eos,\s*int64_t pad,\s*int max_take,\s*int64_t\*\s*out,\s*int64_t ld_out,\s*int n,\s*"
                     r"int64_t\*\s*next,\s*int32_t\*\s*taken,\s*int64_t\*\s*hist,\s*int64_t hist_ld,\s*int hist_col,\s*void\*\s*stream\s*\)", code)
    assert int(re.search(r"#define DESTA_ABI_VERSION (\d+)", txt).group(1)) == 8 == _hip.ABI_VERSION == _hip.lib.desta_abi_version()
    assert hasattr(_hip.lib, "desta_spec_ngram_draft") and hasattr(_hip.lib, "desta_spec_accept")
    doc = txt[txt.index("Draft-and-verify greedy decoding"):txt.index("int desta_spec_accept")]
    assert "modeling_desta25.py:1419" in doc and ":1703" in doc and "PromptLookupCandidateGenerator" in doc


def test_binding_has_the_speculative_callables_and_counters():
    from desta import _hip
    assert callable(_hip.spec_ngram_draft) and callable(_hip.spec_accept)
    assert isinstance(_hip.SPEC_DRAFT_CALLS, int) and isinstance(_hip.SPEC_ACCEPT_CALLS, int)


def test_speculative_kernels_are_named_and_use_no_scratch():
    res = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources()
    spec = {n: r for n, r in res.items() if "spec_" in n}
    assert sum("spec_ngram_draft_k" in n for n in spec) == 1 and sum("spec_accept_k" in n for n in spec) == 1, sorted(spec)
    for name, r in spec.items():
        assert not any(s in name for s in ("swiglu", "rmsnorm", "layernorm", "sample_chain_k", "sample_greedy_k")), name
        assert r["scratch"] == 0 and r["spill"] == 0, (name, r)


def test_check_speculative_arg():
    from desta.models.modeling_desta25 import SPECULATIVE_MAX, check_speculative_arg
    assert SPECULATIVE_MAX == 7
    for ok in (None, 0, 1, 3, 7):
        check_speculative_arg(ok)
    for bad in (-1, 8, 9, 2.0, "3", True, False, [3]):
        with pytest.raises(ValueError, match="speculative"):
            check_speculative_arg(bad)


def test_model_keeps_speculative_off_after_a_rejected_value():
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                    # no device state: the check comes first
    llm = model.llm = CausalLMHIP.__new__(CausalLMHIP)
    llm.speculative = llm._spec = None
    for bad in (9, -1, "3", True):
        with pytest.raises(ValueError, match="speculative"):
            model.set_speculative(bad)
        with pytest.raises(ValueError, match="speculative"):
            llm.set_speculative(bad)
        assert llm.speculative is None
    model.set_speculative(3)
    assert llm.speculative == 3
    model.set_speculative(0)                                                # 0 and None both mean off
    assert llm.speculative is None
    model.set_speculative(7)
    model.set_speculative(None)
    assert llm.speculative is None


def _yaml_with(tmp_path, line):
    """A copy of the debug config directory whose trainer section carries `line` (or nothing)."""
    import shutil
    src = os.path.join(ROOT, "examples", "train", "config")
    dst = tmp_path / "config"
    shutil.copytree(src, dst)
    txt = open(dst / "desta25_debug.yaml").read()
    assert re.search(r"^trainer:\s*$", txt, flags=re.M) and "speculative" not in txt        # the shipped YAMLs do not carry the key
    if line:
        txt = re.sub(r"^trainer:\s*$", "trainer:\n  " + line, txt, count=1, flags=re.M)
    open(dst / "desta25_debug.yaml", "w").write(txt)
    return str(dst)


@pytest.mark.parametrize("line,want", [(None, None), ("speculative: 0", None), ("speculative: null", None), ("speculative: 3", 3), ("speculative: 7", 7)])
def test_speculative_key_parses(tmp_path, line, want):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, line))
    assert m.speculative(cfg) == want
    assert m.kv_cache_kind(cfg) == "bf16" and cfg.trainer.max_epochs is not None             # the rest of the trainer section is intact


def test_bad_speculative_raises_before_create_model(tmp_path, monkeypatch):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"], config_dir=_yaml_with(tmp_path, "speculative: 9"))
    with pytest.raises(ValueError, match="speculative"):
        m.speculative(cfg)
    monkeypatch.setattr(m, "create_model", lambda *a, **k: pytest.fail("create_model reached with a bad trainer.speculative"))
    monkeypatch.setattr(m, "load_config", lambda argv, config_dir=None: cfg)
    with pytest.raises(ValueError, match="speculative"):
        m.main([])
    cfg2 = _load("train_desta_cli", "examples", "train", "train_desta.py").load_config(
        ["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}", "+trainer.speculative=-1"])
    with pytest.raises(ValueError, match="-1"):                             # the command-line override takes the same route
        m.speculative(cfg2)
