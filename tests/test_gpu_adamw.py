"""GPU: fused clip + AdamW (csrc/adamw.hip) against `torch.nn.utils.clip_grad_norm_` + `torch.optim.AdamW(foreach=False)` on CPU
fp32 copies — the kernel, its determinism and padding, the trainer with optim="adamw_torch" (side-stream overlap, gradient
accumulation, empty batch) and `optimizer.pt` interoperability with a real torch.optim.AdamW."""
import importlib.util
import math
import os

import pytest
import torch
from safetensors.torch import load_file

import desta_oracle as O
from helpers import cfg_from_dims

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("a.weight", (1, 16, 24)), ("b.bias", (33, 7)), ("c.weight", (5, 3, 9)), ("d.LayerNorm.weight", (7,)),
          ("e.weight", (4100, 1280)), ("f.weight", (257, 516))]


WORST = {"dp_rel_bound": 0.0, "norm_rel": 0.0}          # measured errors, printed at the end of each test (pytest -s)


def _p_close(got, want, lr, what):
    """|p_hip - p_ref| <= 4e-6 lr + 2.4e-7 |p|.  2.4e-7 |p| is two fp32 ulps of p (ulp(p) <= 2^-23 |p|): the step size and the
    clip coefficient reach p rounded differently on the two sides (float vs double lr / bc1, the norm's summation order, torch's
    scalar tail loops vs its vector body), and p itself was measured 1-2 ulp off at |p| just above a power of two."""
    err = (got.double() - want.double()).abs()
    bound = 4e-6 * lr + 2.4e-7 * want.double().abs()
    WORST["dp_rel_bound"] = max(WORST["dp_rel_bound"], float((err / bound).max()))
    worst = float((err - bound).max())
    assert worst <= 0, f"{what}: max |dp| {float(err.max()):.3e} exceeds the bound by {worst:.3e}"


def _moments_close(got_m, got_v, st, g, what, m_prev=0.0, v_prev=0.0):
    """rtol 1e-6 on exp_avg / exp_avg_sq, plus an absolute floor of two ulps of the step's operands (the previous moment and
    g, resp. g^2): m = m + 0.1 (g - m) can cancel to far below its operands, where fp32 keeps only their absolute rounding and
    torch's lerp rounds once (vector body, fmadd) or twice (scalar tail) (measured: one element of 256, 5.8e-12 absolute,
    5.6e-5 relative)."""
    gmax = float(g.abs().max())
    torch.testing.assert_close(got_m, st["exp_avg"], rtol=1e-6, atol=1e-12 + 2.4e-7 * max(gmax, m_prev), msg=f"exp_avg {what}")
    torch.testing.assert_close(got_v, st["exp_avg_sq"], rtol=1e-6, atol=1e-12 + 2.4e-7 * max(gmax * gmax, v_prev),
                               msg=f"exp_avg_sq {what}")


def _clip_(params, max_norm):
    """clip_grad_norm_ semantics (coef = min(1, max_norm / (total + 1e-6)) in fp32, grads scaled in place) with the total norm
    summed in float64: torch's own fp32 CPU norm reduction is the less accurate side (1.4e-4 relative low on a 5.4 M-element
    arena, where the kernel's fixed-order tree agrees with float64 to 1e-8).  Returns the float64 norm."""
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in params))
    coef = torch.clamp(max_norm / (total.float() + 1e-6), max=1.0)
    for p in params:
        p.grad.mul_(coef)
    return float(total)


def _check_norm(hip, ref):
    WORST["norm_rel"] = max(WORST["norm_rel"], abs(hip - ref) / ref)
    assert hip == pytest.approx(ref, rel=1e-6)


def _with_grad(p):
    q = torch.nn.Parameter(p.detach().clone())
    q.grad = p.grad.clone()
    return q


def _torch_ref(named, decay, lr, betas, eps, wd):
    ps = {n: torch.nn.Parameter(t.detach().cpu().clone()) for n, t in named.items()}
    names = list(named)
    groups = [{"params": [ps[n] for n, d in zip(names, decay) if d], "weight_decay": wd},
              {"params": [ps[n] for n, d in zip(names, decay) if not d], "weight_decay": 0.0}]
    return ps, torch.optim.AdamW(groups, lr=lr, betas=betas, eps=eps, foreach=False)


@pytest.mark.parametrize("betas,eps", [((0.9, 0.98), 1e-8), ((0.9, 0.999), 1e-6)])
def test_kernel_matches_torch_adamw_with_clip(betas, eps):
    from desta.optim import FusedAdamW, ParamArena, decay_mask
    torch.manual_seed(0)
    arena = ParamArena(SHAPES, "cuda")
    names = list(arena.names)
    decay = decay_mask(names)
    assert any(decay) and not all(decay)
    for n in names:
        arena.param(n).normal_(0, 0.02)
    wd, lr = 0.01, 1e-3
    opt = FusedAdamW(arena, weight_decay=wd, betas=betas, eps=eps, max_grad_norm=1.0)
    ps, ref = _torch_ref({n: arena.param(n) for n in names}, decay, lr, betas, eps, wd)
    scales = [1e-3, 1.0, 1e-4, 3e-2, 1e-5]                             # total norm ~ 2.3 x scale: clip active at 1.0 and 3e-2 only
    clipped = []
    for step, s in enumerate(scales):
        lr_t = lr * (1 + step) / len(scales)
        for n in names:
            g = torch.randn(arena.shapes[n]) * s
            arena.grad(n).copy_(g)
            ps[n].grad = g.clone()
        torch_norm = float(torch.nn.utils.clip_grad_norm_([_with_grad(ps[n]) for n in names], 1.0))   # torch's fp32 norm, on copies
        norm = _clip_(list(ps.values()), 1.0)
        assert torch_norm == pytest.approx(norm, rel=5e-4)
        clipped.append(norm > 1.0)
        for gr in ref.param_groups:
            gr["lr"] = lr_t
        prev = {n: (float(ref.state[ps[n]]["exp_avg"].abs().max()), float(ref.state[ps[n]]["exp_avg_sq"].max()))
                if ps[n] in ref.state else (0.0, 0.0) for n in names}
        ref.step()
        g0 = arena.grads.clone()
        opt.step(lr_t)
        torch.cuda.synchronize()
        assert torch.equal(arena.grads, g0)                            # the gradient arena is read only
        _check_norm(float(opt.grad_norm()), norm)
        for n in names:
            _moments_close(arena._view(opt.exp_avg, n).cpu(), arena._view(opt.exp_avg_sq, n).cpu(), ref.state[ps[n]], ps[n].grad,
                           f"{n} step {step}", *prev[n])
            _p_close(arena.param(n).cpu(), ps[n].detach(), lr_t, f"{n} step {step}")
        with torch.no_grad():                                           # every step checked on its own: no drift in p, m, v
            for n in names:
                ps[n].copy_(arena.param(n).cpu())
                ref.state[ps[n]]["exp_avg"].copy_(arena._view(opt.exp_avg, n).cpu())
                ref.state[ps[n]]["exp_avg_sq"].copy_(arena._view(opt.exp_avg_sq, n).cpu())
    assert any(clipped) and not all(clipped)
    print(f"\n[adamw] betas {betas} eps {eps}: worst |p_hip - p_ref| / bound {WORST['dp_rel_bound']:.3f}, norm rel err {WORST['norm_rel']:.2e}")


def test_gradients_untouched_deterministic_and_padding_stays_zero():
    from desta.optim import FusedAdamW, ParamArena
    torch.manual_seed(1)
    runs = []
    for _ in range(2):
        arena = ParamArena(SHAPES, "cuda")
        gen = torch.Generator(device="cuda").manual_seed(5)
        for n in arena.names:
            arena.param(n).copy_(torch.randn(arena.shapes[n], device="cuda", generator=gen) * 0.02)
        opt = FusedAdamW(arena, weight_decay=0.1, betas=(0.9, 0.98))
        for step in range(3):
            for n in arena.names:
                arena.grad(n).copy_(torch.randn(arena.shapes[n], device="cuda", generator=gen) * (0.5 if step == 1 else 1e-3))
            g0 = arena.grads.clone()
            opt.step(1e-3)
            torch.cuda.synchronize()
            assert torch.equal(arena.grads, g0)
        runs.append((arena, opt))
    (a0, o0), (a1, o1) = runs
    assert torch.equal(a0.params, a1.params) and torch.equal(o0.exp_avg, o1.exp_avg) and torch.equal(o0.exp_avg_sq, o1.exp_avg_sq)
    assert torch.equal(o0.workspace[:2], o1.workspace[:2])
    live = torch.zeros(a0.numel, dtype=torch.bool)
    for n in a0.names:
        live[a0.offsets[n]:a0.offsets[n] + math.prod(a0.shapes[n])] = True
    assert (~live).sum() > 0
    for buf in (a0.params, o0.exp_avg, o0.exp_avg_sq):
        assert torch.count_nonzero(buf.cpu()[~live]) == 0


def _tiny_trainer(ga=1, overlap=True, lr=1e-3):
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    from desta.trainer.desta_trainer import DeSTA25Trainer, TrainingArguments
    d = O.tiny_dims(False)
    w = O.init_weights(d, seed=7)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=w, device="cuda:0")
    args = TrainingArguments(learning_rate=lr, warmup_steps=0, max_steps=10, logging_steps=1, overlap_comm=overlap,
                             gradient_accumulation_steps=ga, optim="adamw_torch", adam_beta2=0.98, weight_decay=0.01)
    return d, model, DeSTA25Trainer(model, args=args)


def test_trainer_adamw_steps_match_torch_on_the_hip_gradients():
    from desta.optim import FusedAdamW, decay_mask, linear_warmup_lr
    d, model, tr = _tiny_trainer()
    assert isinstance(tr.optimizer, FusedAdamW) and tr._side is not None
    arena = model.arena
    names = list(arena.names)
    ps, ref = _torch_ref({n: arena.param(n) for n in names}, decay_mask(names), 1e-3, (0.9, 0.98), 1e-8, 0.01)
    batches = [O.synthetic_batch(d, B=2, S_ctx=5, S_tgt=24, seed=10 + i) for i in range(4)]
    for i in range(3):
        before = arena.params.clone()
        tr.training_step(batches[i], next_inputs=batches[i + 1])
        tr.wait_update()
        torch.cuda.synchronize()
        lr = linear_warmup_lr(tr.global_step - 1, 1e-3, 0, 10)
        with torch.no_grad():
            for n in names:
                ps[n].copy_(arena._view(before, n).cpu())
                ps[n].grad = arena.grad(n).cpu().clone()
        norm = _clip_(list(ps.values()), 1.0)
        for g in ref.param_groups:
            g["lr"] = lr
        ref.step()
        _check_norm(float(tr.optimizer.grad_norm()), norm)
        for n in names:
            _p_close(arena.param(n).cpu(), ps[n].detach(), lr, f"{n} step {i}")
        assert not torch.equal(before, arena.params)
    assert tr.optimizer.step_count == 3
    # a single-device empty batch: torch AdamW skips every parameter (grads None) — parameters and moments unchanged, the
    # scheduler and global_step advance
    p0, m0, v0 = arena.params.clone(), tr.optimizer.exp_avg.clone(), tr.optimizer.exp_avg_sq.clone()
    loss = tr.training_step({"_empty_batch": True})
    tr.wait_update()
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and tr.global_step == 4 and tr.optimizer.step_count == 3
    assert torch.equal(p0, arena.params) and torch.equal(m0, tr.optimizer.exp_avg) and torch.equal(v0, tr.optimizer.exp_avg_sq)
    print(f"\n[adamw] trainer: worst |p_hip - p_ref| / bound {WORST['dp_rel_bound']:.3f}, norm rel err {WORST['norm_rel']:.2e}")


def test_trainer_adamw_gradient_accumulation():
    from desta.optim import decay_mask, linear_warmup_lr
    d, model, tr = _tiny_trainer(ga=2)
    arena = model.arena
    names = list(arena.names)
    ps, ref = _torch_ref({n: arena.param(n) for n in names}, decay_mask(names), 1e-3, (0.9, 0.98), 1e-8, 0.01)
    for i in range(2):
        before = arena.params.clone()
        tr.training_step(O.synthetic_batch(d, B=2, S_ctx=5, S_tgt=24, seed=20 + 2 * i))
        assert tr.global_step == i and torch.equal(before, arena.params)          # first micro-batch: no update yet
        tr.training_step(O.synthetic_batch(d, B=2, S_ctx=5, S_tgt=24, seed=21 + 2 * i))
        tr.wait_update()
        torch.cuda.synchronize()
        assert tr.global_step == i + 1
        with torch.no_grad():
            for n in names:
                ps[n].copy_(arena._view(before, n).cpu())
                ps[n].grad = arena.grad(n).cpu().clone()                           # the window's summed gradient
        _clip_(list(ps.values()), 1.0)
        lr = linear_warmup_lr(i, 1e-3, 0, 10)
        for g in ref.param_groups:
            g["lr"] = lr
        ref.step()
        for n in names:
            _p_close(arena.param(n).cpu(), ps[n].detach(), lr, f"{n} window {i}")


def _entry():
    spec = importlib.util.spec_from_file_location("train_desta", os.path.join(ROOT, "examples", "train", "train_desta.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_checkpoint_interop_with_torch_adamw_and_resume(tmp_path):
    from desta.models.modeling_desta25 import reference_parameter_names
    from desta.optim import decay_mask, linear_warmup_lr
    m = _entry()
    common = ["--config-name", "desta25_debug", "+dataset=debug", "trainer.max_steps=-1", "trainer.max_epochs=2",
              "dataset.train_ds.num_samples=6", "optim.sched.warmup_steps=2", "optim.lr=1e-3", "optim.name=adamw_torch"]   # 3 steps per epoch
    a = m.main(common + [f"exp_dir={tmp_path}/a"])
    assert a.global_step == 6 and a.args.optim == "adamw_torch" and (a.args.adam_beta1, a.args.adam_beta2) == (0.9, 0.98)
    ck3 = tmp_path / "a" / "checkpoint-3"
    sd = torch.load(ck3 / "optimizer.pt", weights_only=True)
    names = reference_parameter_names(a.model.config)
    dm = decay_mask(names)
    # strict load into a real torch.optim.AdamW over CPU tensors in reference_parameter_names order, two groups
    w3 = load_file(ck3 / "model.safetensors")
    ps = {n: torch.nn.Parameter(w3[n].float().clone()) for n in names}
    ref = torch.optim.AdamW([{"params": [ps[n] for n, d in zip(names, dm) if d], "weight_decay": 0.01},
                             {"params": [ps[n] for n, d in zip(names, dm) if not d], "weight_decay": 0.0}],
                            lr=1e-3, betas=(0.9, 0.98), eps=1e-8)
    ref.load_state_dict(sd)
    assert float(ref.state[ps[names[0]]]["step"]) == 3
    # one further HIP step from the checkpoint (resume + 1 step) vs one further torch step on the HIP gradients
    c = m.main(common + [f"exp_dir={tmp_path}/c", f"resume_from_checkpoint={ck3}", "trainer.max_steps=4"])
    assert c.global_step == 4 and c.optimizer.step_count == 4
    lr = linear_warmup_lr(3, 1e-3, 2, c.total_steps)
    for n in names:
        ps[n].grad = c.model.arena.grad(n).cpu().clone()
    _clip_(list(ps.values()), 1.0)
    for g in ref.param_groups:
        g["lr"] = lr
    ref.step()
    for n in names:
        _p_close(c.model.arena.param(n).cpu(), ps[n].detach(), lr, n)
        _moments_close(c.model.arena._view(c.optimizer.exp_avg, n).cpu(), c.model.arena._view(c.optimizer.exp_avg_sq, n).cpu(),
                       ref.state[ps[n]], ps[n].grad, n)
    # 3 + 3 through main() == 6 straight, bit for bit
    b = m.main(common + [f"exp_dir={tmp_path}/b", f"resume_from_checkpoint={ck3}"])
    assert b.global_step == 6
    pa, pb = load_file(tmp_path / "a" / "checkpoint-6" / "model.safetensors"), load_file(tmp_path / "b" / "checkpoint-6" / "model.safetensors")
    assert pa.keys() == pb.keys() and all(torch.equal(pa[k], pb[k]) for k in pa)
    oa = torch.load(tmp_path / "a" / "checkpoint-6" / "optimizer.pt", weights_only=True)
    ob = torch.load(tmp_path / "b" / "checkpoint-6" / "optimizer.pt", weights_only=True)
    assert oa["param_groups"] == ob["param_groups"] and oa["state"].keys() == ob["state"].keys()
    for i in oa["state"]:
        for k, v in oa["state"][i].items():
            assert torch.equal(v, ob["state"][i][k]), (i, k)
    assert any(not torch.equal(w3[k], pa[k]) for k in pa)
    # an Adafactor checkpoint cannot resume an AdamW run (nor the reverse): ValueError naming both
    af = [t for t in common if not t.startswith("optim.name")] + ["trainer.max_epochs=1"]
    m.main(af + [f"exp_dir={tmp_path}/af"])
    with pytest.raises(ValueError, match="Adafactor.*AdamW"):
        m.main(common + [f"exp_dir={tmp_path}/x", f"resume_from_checkpoint={tmp_path}/af/checkpoint-3"])
    with pytest.raises(ValueError, match="AdamW.*Adafactor"):
        m.main(af + [f"exp_dir={tmp_path}/y", f"resume_from_checkpoint={ck3}"])
