"""CPU: the clip + AdamW optimizer's host side — the library exports its entry points, the entry point maps `optim.name` /
`optim.betas` / `optim.eps` onto TrainingArguments, the HF `optimizer.pt` layout is torch.optim.AdamW's own, and an Adafactor
state cannot be loaded into AdamW (or the reverse) without a ValueError naming both."""
import ctypes
import importlib.util
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _entry():
    spec = importlib.util.spec_from_file_location("train_desta", os.path.join(ROOT, "examples", "train", "train_desta.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _arena():
    from desta.optim import ParamArena
    a = ParamArena([("con.layer.0.weight", (5, 8)), ("con.layer.0.bias", (5,)), ("con.LayerNorm.weight", (7,))], "cpu")
    return a


def test_library_exports_the_adamw_entry_points():
    from desta import _hip
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for s in ("desta_adamw_workspace_floats", "desta_clip_adamw_step"):
        assert hasattr(lib, s), s
    assert _hip.lib.desta_sizeof_desc(3) == ctypes.sizeof(_hip.AdamWPlan)
    pl = _hip.AdamWPlan()
    pl.numel = 1 << 20
    assert _hip.lib.desta_adamw_workspace_floats(ctypes.byref(pl)) >= 8 + 1


def test_entry_point_maps_optim_name_betas_and_eps(tmp_path):
    m = _entry()
    base = ["--config-name", "desta25_llama31-8B_Qformer6L", "+dataset=synthetic", f"exp_dir={tmp_path}"]
    args = m.create_training_args(m.load_config(base))
    assert args.optim == "adafactor"                                  # no optim.name: today's mapping
    args = m.create_training_args(m.load_config(base + ["optim.name=adamw_torch"]))
    assert args.optim == "adamw_torch" and (args.adam_beta1, args.adam_beta2) == (0.9, 0.98) and args.adam_epsilon == 1e-8
    args = m.create_training_args(m.load_config(base + ["optim.name=adamw_torch_fused", "optim.eps=1e-6"]))
    assert args.optim == "adamw_torch_fused" and args.adam_epsilon == 1e-6 and args.adam_beta2 == 0.98
    with pytest.raises(ValueError, match="optim.name"):
        m.create_training_args(m.load_config(base + ["optim.name=adamw_8bit"]))


def test_training_arguments_defaults_and_unknown_optim():
    from desta.trainer.desta_trainer import DeSTA25Trainer, TrainingArguments
    a = TrainingArguments()
    assert a.optim == "adafactor" and (a.adam_beta1, a.adam_beta2, a.adam_epsilon) == (0.9, 0.999, 1e-8)

    class _M:                                                         # the check runs before the model is touched
        arena = None
    with pytest.raises(NotImplementedError, match="sgd"):
        DeSTA25Trainer(_M(), args=TrainingArguments(optim="sgd"))


def test_work_items_cover_every_tensor_inside_its_slot():
    from desta.optim import FusedAdamW, decay_mask
    from desta import _hip
    a = _arena()
    opt = FusedAdamW(a, weight_decay=0.05)
    items, wd = opt._items.tolist(), opt._wd.tolist()
    assert [o for o, _ in items] == sorted(o for o, _ in items)
    covered = {}
    for (off, n), w in zip(items, wd):
        assert off % 4 == 0 and n % 4 == 0 and 0 < n <= _hip.ADAMW_ITEM_FLOATS and off + n <= a.numel
        name = max((nm for nm in a.names if a.offsets[nm] <= off), key=lambda nm: a.offsets[nm])
        assert off + n <= a.offsets[name] + ((a.param(name).numel() + 63) // 64) * 64
        covered[name] = covered.get(name, 0) + n
        assert w == pytest.approx(0.05 if decay_mask([name])[0] else 0.0, rel=1e-7)
    assert all(covered[nm] >= a.param(nm).numel() for nm in a.names)
    # a tensor larger than one work item is cut into several
    from desta.optim import ParamArena
    big = FusedAdamW(ParamArena([("w", (3, 4100))], "cpu"))
    assert big.plan.n_items == 4 and sum(n for _, n in big._items.tolist()) == 12300


def test_hf_state_dict_has_torch_adamw_layout():
    from desta.optim import FusedAdamW, decay_mask
    a = _arena()
    opt = FusedAdamW(a, weight_decay=0.01, betas=(0.9, 0.98), eps=1e-6)
    names = list(a.names)
    sd = opt.hf_state_dict(names, lr=1e-4, weight_decay=0.01)
    dm = decay_mask(names)
    ps = {n: torch.nn.Parameter(torch.zeros(a.shapes[n])) for n in names}
    ref = torch.optim.AdamW([{"params": [ps[n] for n, d in zip(names, dm) if d], "weight_decay": 0.01},
                             {"params": [ps[n] for n, d in zip(names, dm) if not d], "weight_decay": 0.0}],
                            lr=1e-4, betas=(0.9, 0.98), eps=1e-6)
    want = ref.state_dict()
    assert sd["state"] == {} and len(sd["param_groups"]) == 2
    for g, w in zip(sd["param_groups"], want["param_groups"]):
        assert g == w
    ref.load_state_dict(sd)
    # with moments: per-param {step: float32 scalar tensor, exp_avg, exp_avg_sq} in the parameter's shape
    opt.step_count = 2
    opt.exp_avg.normal_()
    opt.exp_avg_sq.uniform_()
    sd = opt.hf_state_dict(names, lr=1e-4)
    order = [n for n, d in zip(names, dm) if d] + [n for n, d in zip(names, dm) if not d]
    for i, n in enumerate(order):
        e = sd["state"][i]
        assert set(e) == {"step", "exp_avg", "exp_avg_sq"} and e["step"].dtype == torch.float32 and float(e["step"]) == 2
        assert torch.equal(e["exp_avg"], a._view(opt.exp_avg, n)) and e["exp_avg_sq"].shape == a.shapes[n]
    ref.load_state_dict(sd)
    back = FusedAdamW(a, betas=(0.9, 0.98), eps=1e-6)
    back.load_hf_state_dict(sd, names)
    assert back.step_count == 2
    for n in names:
        assert torch.equal(a._view(back.exp_avg, n), a._view(opt.exp_avg, n))
        assert torch.equal(a._view(back.exp_avg_sq, n), a._view(opt.exp_avg_sq, n))
    local = FusedAdamW(a)
    local.load_state_dict(opt.state_dict())
    assert local.step_count == 2 and torch.equal(local.exp_avg[:5 * 8], opt.exp_avg[:5 * 8])


def test_mismatched_optimizer_state_raises_value_error():
    from desta.optim import FusedAdafactor, FusedAdamW
    a = _arena()
    names = list(a.names)
    af, aw = FusedAdafactor(a), FusedAdamW(a)
    af.step_count = aw.step_count = 1
    with pytest.raises(ValueError, match="Adafactor.*AdamW"):
        aw.load_hf_state_dict(af.hf_state_dict(names, lr=1e-4), names)
    with pytest.raises(ValueError, match="AdamW.*Adafactor"):
        af.load_hf_state_dict(aw.hf_state_dict(names, lr=1e-4), names)
    with pytest.raises(ValueError, match="Adafactor.*AdamW"):
        aw.load_state_dict(af.state_dict())
    with pytest.raises(ValueError, match="AdamW.*Adafactor"):
        af.load_state_dict(aw.state_dict())
