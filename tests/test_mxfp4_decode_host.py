"""CPU: the host side of weight-only MXFP4 decode - the format's reference (tests/mxfp4_reference.py) on planted blocks, its round
trip and the choice of the scale rule; the `trainer.decode_weights` key and the model's validation; the two C entry points in the
header at an unchanged ABI version; the resources of the new kernel instantiations; and the instrument of the GPU test: a
conforming emulation of the kernel's K order stays inside 1 x bound, two seeded mutations exceed the GPU test's 2 x bound."""
import importlib.util
import os
import re

import pytest
import torch

import mxfp4_reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 2.0                # of test_gpu_mxfp4_decode.py / test_gpu_gemm_fp64.py


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *parts))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------------------------------------------------------- format
def test_scale_rule_and_ties_on_planted_blocks():
    w, e_want, checks = X.planted_blocks()
    codes, e = X.quantize_ref(w)
    assert torch.equal(e.view(-1), e_want), (e.view(-1), e_want)
    vals = X.code_values(codes)
    for blk, el, want in checks:
        assert float(vals[blk, el]) == want, (blk, el, float(w[blk, el]), float(vals[blk, el]), want)
    zero = int((w.double().abs().amax(1) == 0).nonzero()[0])                 # the all-zero block: byte 127, every code 0
    assert int(X.scale_bytes(e)[zero, 0]) == 127 and not bool((codes[zero] & 7).any())
    assert int(X.scale_bytes(e).max()) < 255
    # amax 2^-e <= 7 < amax 2^-(e - 1) at every non-zero block
    amax = w.double().abs().amax(1)
    nz = amax > 0
    sc = torch.ldexp(torch.ones_like(amax), e.view(-1))
    assert bool((amax[nz] / sc[nz] <= 7).all()) and bool((amax[nz] / sc[nz] * 2 > 7).all())


def test_round_trip_is_exact_bf16_and_idempotent():
    g = torch.Generator().manual_seed(5)
    band = torch.tensor([1.0, 0.02, 3e-4])[torch.arange(96) % 3]
    w = (torch.randn(96, 256, generator=g) * band[:, None]).to(torch.bfloat16)
    w = torch.cat([w, X.planted_blocks()[0].repeat(1, 8)[:, :256]])
    codes, e = X.quantize_ref(w)
    d = X.dequant_bf16(codes, e)                                             # asserts exactness
    codes2, e2 = X.quantize_ref(d)
    nz = (d.double().view(d.shape[0], -1, 32).abs().amax(2) > 0)
    assert torch.equal(e2[nz], e[nz])
    assert torch.equal(X.code_values(codes2), X.code_values(codes))
    assert torch.equal(codes2, codes)                                        # -0 keeps its sign bit through bf16
    assert torch.equal(X.unpack(X.pack(codes)), codes)
    q = X.pack(codes)
    assert torch.equal(q[:, 0] & 15, codes[:, 0]) and torch.equal(q[:, 0] >> 4, codes[:, 1])      # element 2j low, 2j + 1 high


def test_le7_rule_beats_both_neighbouring_rules():
    """200 000 seeded Gaussian 32-blocks: the relative squared weight error of the three candidate scale rules."""
    g = torch.Generator().manual_seed(0)
    w = torch.randn(200_000, 32, generator=g).to(torch.bfloat16)
    err = {r: X.rel_sq_error(w, r) for r in X.RULES}
    print("\nrelative squared error: " + "  ".join(f"{r} {v:.5f}" for r, v in err.items()))
    assert err["le7"] < err["ocp_floor"] and err["le7"] < err["le6"], err
    assert err["le7"] < 0.0135, err


# ---------------------------------------------------------------------------------------------------------------- config
def _yaml_with(tmp_path, line):
    import shutil
    src = os.path.join(ROOT, "examples", "train", "config")
    dst = tmp_path / "config"
    shutil.copytree(src, dst)
    txt = open(dst / "desta25_debug.yaml").read()
    assert re.search(r"^trainer:\s*$", txt, flags=re.M) and "decode_weights" not in txt
    txt = re.sub(r"^trainer:\s*$", "trainer:\n  " + line, txt, count=1, flags=re.M)
    open(dst / "desta25_debug.yaml", "w").write(txt)
    return str(dst)


def test_decode_weights_mxfp4_parses_and_int4_still_raises(tmp_path, monkeypatch):
    m = _load("train_desta", "examples", "train", "train_desta.py")
    cfg = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"],
                        config_dir=_yaml_with(tmp_path / "a", "decode_weights: mxfp4"))
    assert m.decode_weights_kind(cfg) == "mxfp4"
    assert cfg.trainer.max_epochs is not None
    bad = m.load_config(["--config-name", "desta25_debug", "+dataset=debug", f"exp_dir={tmp_path}"],
                        config_dir=_yaml_with(tmp_path / "b", "decode_weights: int4"))
    with pytest.raises(ValueError, match="decode_weights"):
        m.decode_weights_kind(bad)
    monkeypatch.setattr(m, "create_model", lambda *a, **k: pytest.fail("create_model reached with a bad trainer.decode_weights"))
    monkeypatch.setattr(m, "load_config", lambda argv, config_dir=None: bad)
    with pytest.raises(ValueError, match="decode_weights"):
        m.main([])


def test_model_kinds_and_validation_without_gpu():
    from desta.models.modeling_desta25 import CausalLMHIP, DeSTA25AudioModel
    assert CausalLMHIP.DECODE_WEIGHT_KINDS == ("bf16", "fp8")
    assert CausalLMHIP.DECODE_WEIGHT_KINDS_MX == ("mxfp4",)
    model = DeSTA25AudioModel.__new__(DeSTA25AudioModel)                     # no device state: the check comes first
    for bad in ("int4", "int8", "mxfp8"):
        with pytest.raises(ValueError, match=bad) as ei:
            model.set_decode_weights(bad)
        assert "mxfp4" in str(ei.value) and "fp8" in str(ei.value)           # the message lists the union
    llm = CausalLMHIP.__new__(CausalLMHIP)
    with pytest.raises(ValueError, match="int4"):
        llm.set_decode_weights("int4")


def test_header_declares_the_mxfp4_entry_points_at_abi_8():
    txt = open(os.path.join(ROOT, "include", "desta_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"int\s+desta_quantize_rows_mxfp4\s*\(\s*const void\*\s*w_bf16,\s*int rows,\s*int cols,\s*int64_t ld,\s*uint8_t\*\s*q,\s*int64_t ldq,"
                     r"\s*uint8_t\*\s*scale_e8m0,\s*int64_t lds,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"int\s+desta_gemm_w4a16_nt\s*\(\s*const desta_gemm_desc\*\s*d,\s*const uint8_t\*\s*b_scale_e8m0,\s*int64_t ld_scale,\s*void\*\s*stream\s*\)", code)
    assert re.search(r"#define DESTA_ABI_VERSION (\d+)", txt).group(1) == "8"
    block = txt[txt.index("Weight-only MXFP4 (W4A16) decode"):txt.index("int desta_gemm_w4a16_nt")]
    assert "modeling_desta25.py:1419-1427" in block and "modeling_llama.py:163-176" in block
    from desta import _hip
    assert _hip.ABI_VERSION == 8 and _hip.lib.desta_abi_version() == 8
    assert hasattr(_hip.lib, "desta_quantize_rows_mxfp4") and hasattr(_hip.lib, "desta_gemm_w4a16_nt")
    assert callable(_hip.quantize_rows_mxfp4) and callable(_hip.gemm_w4) and _hip.GEMM_W4_CALLS == 0


def test_mxfp4_kernels_fit_their_budgets():
    """Every instantiation the model dispatches exists; none uses scratch or spills; VGPR <= 256, LDS <= 160 KiB."""
    res = _load("kernel_resources", "tools", "kernel_resources.py").kernel_resources()
    w4 = {}
    for n, r in res.items():
        m = re.search(r"gemm_w4a16_nt_kernelILi(\d)ELb([01])ELb([01])EEE", n)
        if m:
            w4[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = r
    want = {(1, sw, rms) for sw in (0, 1) for rms in (0, 1)} | {(mf, sw, 0) for mf in (2, 3, 4) for sw in (0, 1)}
    assert set(w4) == want, sorted(w4)
    quant = {n: r for n, r in res.items() if "quantize_rows_mxfp4" in n}
    assert len(quant) == 1
    for n, r in {**w4, **quant}.items():
        assert r["scratch"] == 0 and r["spill"] == 0, (n, r)
    for n, r in w4.items():
        assert r["vgpr"] <= 256 and r["lds"] <= 160 * 1024, (n, r)
        print(f"\ngemm_w4a16_nt_kernel<MF {n[0]}, SWIGLU {n[1]}, RMS {n[2]}>: vgpr {r['vgpr']} lds {r['lds']}", end="")


# ---------------------------------------------------------------------------------------------------------------- the instrument
HOST_CASES = [X.case(1, 16, 64), X.case(3, 100, 192, res=True), X.case(16, 1028, 2048), X.case(5, 64, 64 * 37, out_f32=True, alpha=0.75),
              X.case(8, 512, 256, act=4), X.case(3, 104, 192, act=4), X.case(8, 128, 4096, rms=True, res=True),
              X.case(8, 64, 4096, act=4, rms=True), X.case(33, 100, 192, res=True), X.case(48, 36, 64 * 37), X.case(17, 104, 192, act=4),
              X.case(40, 512, 2048, act=4), X.case(24, 256, 4096)]
_REF = {}


def _reference(i):
    if i not in _REF:
        o = X.operands(HOST_CASES[i])
        _REF[i] = (o, X.exact(o))
    return _REF[i]


def test_plan_matches_hand_computed_edges():
    assert X.plan(8, 4096, 4096, 0) == dict(ntiles=64, nc=32, ks=4, cps=8, mf=1, c=4 + 32 + 7 + 3)
    assert X.plan(24, 4096, 4096, 0)["c"] == X.plan(8, 4096, 4096, 0)["c"]                     # M enters neither ks nor c
    assert X.plan(40, 512, 2048, 4) == dict(ntiles=16, nc=16, ks=2, cps=8, mf=3, c=4 + 32 + 7 + 1)
    assert X.plan(8, 512, 14336, 0) == dict(ntiles=8, nc=112, ks=8, cps=14, mf=1, c=8 + 32 + 7 + 7)
    assert X.plan(48, 36, 64 * 37, 0) == dict(ntiles=1, nc=19, ks=2, cps=10, mf=3, c=8 + 32 + 7 + 1)
    assert X.plan(3, 100, 192, 0)["ks"] == 1 and X.plan(3, 100, 192, 0)["nc"] == 2            # 64-element tail chunk


@pytest.mark.parametrize("i", range(len(HOST_CASES)), ids=[X.case_id(c) for c in HOST_CASES])
def test_emulation_of_the_k_order_is_inside_the_bound(i):
    o, ref = _reference(i)
    emu = X.emulate(o)
    r = X.ratio(o, ref, "C", emu["C"])
    print(f"\n{X.case_id(HOST_CASES[i])} [ks {o['plan']['ks']} c {o['c']}]: emulation ratio {r:.3f}", end="")
    assert r <= 1.0, r


@pytest.mark.parametrize("mut", X.MUTATIONS)
@pytest.mark.parametrize("i", range(len(HOST_CASES)), ids=[X.case_id(c) for c in HOST_CASES])
def test_mutation_exceeds_the_bound(i, mut):
    o, ref = _reference(i)
    r = X.ratio(o, ref, "C", X.emulate(o, mutation=mut)["C"])
    assert r > FACTOR, f"{mut} stays within {FACTOR} x bound at {X.case_id(HOST_CASES[i])}: worst ratio {r:.3f}"
