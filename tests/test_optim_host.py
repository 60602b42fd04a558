"""CPU: the state-dict codec both fused optimizers share (desta/optim.py), on a CPU arena.  Adafactor's `optimizer.pt` loads into
transformers' own Adafactor built with HF Trainer's two groups and round-trips exactly; the local form round-trips and carries
its tag; a parameter without an entry in an HF dict starts from zeros in both optimizers."""
import copy

import pytest
import torch

OTHER = {"adafactor": "adamw", "adamw": "adafactor"}


def _arena():
    from desta.optim import ParamArena
    a = ParamArena([("con.layer.0.weight", (5, 8)), ("con.layer.0.bias", (5,)), ("con.prompts", (2, 3, 4)),
                    ("con.LayerNorm.weight", (7,))], "cpu")
    g = torch.Generator().manual_seed(0)
    for n in a.names:
        a.param(n).copy_(torch.randn(a.shapes[n], generator=g))
    return a


def _make(which, a):
    from desta.optim import FusedAdafactor, FusedAdamW
    return FusedAdafactor(a, weight_decay=0.01) if which == "adafactor" else FusedAdamW(a, weight_decay=0.01)


def _fill(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for sl in opt.slots.values():
        for v in sl.values():
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)


def test_adafactor_hf_state_dict_loads_into_transformers_and_round_trips():
    from transformers.optimization import Adafactor
    from desta.optim import FusedAdafactor, _hf_order
    a = _arena()
    names = list(a.names)
    order, n_decay = _hf_order(names)
    ps = {n: torch.nn.Parameter(a.param(n).clone()) for n in names}
    hf = Adafactor([{"params": [ps[n] for n in order[:n_decay]], "weight_decay": 0.01},
                    {"params": [ps[n] for n in order[n_decay:]], "weight_decay": 0.0}],
                   lr=1e-3, scale_parameter=False, relative_step=False)
    opt = FusedAdafactor(a, weight_decay=0.01)
    assert opt.hf_state_dict(names, lr=1e-3, weight_decay=0.01) == {"state": {}, "param_groups": hf.state_dict()["param_groups"]}
    _fill(opt, 1)
    opt.step_count = 3
    sd = opt.hf_state_dict(names, lr=1e-3, weight_decay=0.01)
    for i, n in enumerate(order):
        e, shape = sd["state"][i], a.shapes[n]
        keys = ["exp_avg_sq_row", "exp_avg_sq_col"] if len(shape) >= 2 else ["exp_avg_sq"]
        assert list(e) == ["step", "RMS"] + keys and type(e["step"]) is int and e["step"] == 3
        torch.testing.assert_close(e["RMS"], a.param(n).norm(2) / a.param(n).numel() ** 0.5, rtol=0, atol=0)
        for k in keys:
            assert e[k].device.type == "cpu" and e[k].dtype == torch.float32 and torch.equal(e[k], opt.slots[n][k])
        if len(shape) >= 2:
            assert e["exp_avg_sq_row"].shape == shape[:-1] and e["exp_avg_sq_col"].shape == shape[:-2] + shape[-1:]
    hf.load_state_dict(copy.deepcopy(sd))                            # transformers' step below updates what it loaded in place
    got = hf.state_dict()
    for i in sd["state"]:
        for k, v in sd["state"][i].items():
            assert torch.equal(torch.as_tensor(got["state"][i][k]), torch.as_tensor(v)), (i, k)
    for n in names:                                                  # transformers steps on the loaded state (shapes agree)
        ps[n].grad = torch.full_like(ps[n], 1e-2)
    hf.step()
    back = FusedAdafactor(a, weight_decay=0.01)
    back.load_hf_state_dict(sd, names)
    assert back.step_count == 3 and torch.equal(back.state, opt.state)


@pytest.mark.parametrize("which", ["adafactor", "adamw"])
def test_local_state_dict_round_trips_with_its_tag(which):
    a = _arena()
    opt = _make(which, a)
    _fill(opt, 2)
    opt.step_count = 4
    sd = opt.state_dict()
    assert sd["optimizer"] == which and sd["names"] == list(a.names) and sd["step"] == 4
    back = _make(which, a)
    back.load_state_dict(sd)
    assert back.step_count == 4
    for n in a.names:
        for k, v in opt.slots[n].items():
            assert torch.equal(back.slots[n][k], v), (n, k)
    del sd["optimizer"]                                              # an untagged dict is still identified by its keys
    with pytest.raises(ValueError):
        _make(OTHER[which], a).load_state_dict(sd)


@pytest.mark.parametrize("which", ["adafactor", "adamw"])
def test_hf_load_starts_parameters_without_an_entry_from_zeros(which):
    from desta.optim import _hf_order
    a = _arena()
    names = list(a.names)
    order, _ = _hf_order(names)
    src = _make(which, a)
    _fill(src, 3)
    src.step_count = 2
    sd = src.hf_state_dict(names, lr=1e-4)
    dropped = {0, len(order) - 1}
    for i in dropped:
        del sd["state"][i]
    dst = _make(which, a)
    _fill(dst, 4)                                                    # state from before the load must not survive it
    dst.load_hf_state_dict(sd, names)
    assert dst.step_count == 2
    for i, n in enumerate(order):
        for k, v in dst.slots[n].items():
            assert torch.equal(v, torch.zeros_like(v) if i in dropped else src.slots[n][k]), (n, k)
