"""GPU: ORCA hybrid — the product's forward AND backward for `connector_mode="orca_hybrid"` against the golden made by
the reference's own ORCAHybridConnector / ORCAGatedCrossAttention / compute_orca_losses / forward (tests/golden/ref_orca_tiny.safetensors,
tests/golden/make_golden_from_reference.py::make_orca_case; the CPU oracle restatement is pinned to the same file in
tests/test_oracle_pin.py).  Tolerances: the product computes in bf16 with fp32 accumulation / statistics like the reference under
autocast, the golden is fp32 — the bounds of the qformer_1 tiny goldens (tests/test_gpu_model.py)."""
import copy
import os

import pytest
import torch
from safetensors.torch import load_file

import desta_oracle as O
import orca_oracle as R
from helpers import cfg_from_dims, rel_err

pytestmark = pytest.mark.gpu


def _case(golden_dir, gca=False):
    """gca: False = the base golden, True = `orca_global_cross_attn`, "nolocal" = that plus `orca_local_enabled: false`."""
    local = gca != "nolocal"
    gca = bool(gca)
    g = load_file(os.path.join(golden_dir, "ref_orca_tiny.safetensors"))
    if gca:                                   # the small files of the variants do not repeat the inputs
        g = {**load_file(os.path.join(golden_dir, "ref_orca_tiny_gca.safetensors" if local else "ref_orca_tiny_nolocal.safetensors")), "batch_features": g["batch_features"]}
    kg, ds, ks, ntr = (int(x) for x in g["orca_dims"])
    d = O.tiny_dims(False)
    o = R.OrcaDims(global_num_tokens=kg, local_downsample=ds, local_kernel_size=ks, ortho_diversity_weight=0.05,
                   ortho_weight_qformer_local=0.05, align_weight_local=0.05, global_cross_attn=gca, local_enabled=local)
    w = R.init_weights(d, o, seed=7)
    d = copy.copy(d)
    d.prompt_size = kg + ntr
    n = g["starts"].shape[0]
    batch = {"input_ids": g["input_ids"], "attention_mask": g["attention_mask"], "labels": g["labels"], "batch_features": g["batch_features"],
             "batch_start_positions": [(int(b), int(s)) for b, s in g["starts"].tolist()],
             "batch_transcription_ids": [g["transcription_ids"][i:i + 1] for i in range(n)]}
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=ds,
                        orca_local_kernel_size=ks, orca_ortho_diversity_weight=0.05, orca_ortho_weight_qformer_local=0.05,
                        orca_align_weight_local=0.05, orca_rope_theta=float(g["rope_theta_used"]), orca_global_cross_attn=gca, orca_local_enabled=local)
    return g, d, o, w, batch, cfg


def test_orca_forward_vs_reference_golden(golden_dir):
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    g, d, o, w, batch, cfg = _case(golden_dir)
    model = DeSTA25AudioModel(cfg, weights=w)
    assert sorted(model.trainable_parameter_names) == sorted(R.trainable_names(d, o))       # the reference's state-dict keys
    for n in R.trainable_names(d, o):
        assert torch.equal(model.arena.param(n).cpu(), w[n].reshape(model.arena.shapes[n])), n
    model.train()
    out = model(**batch, keep_logits=True)
    m = g["attention_mask"].bool()
    rec = dict(dloss=abs(float(out.loss) - float(g["loss"])), logits=rel_err(out.logits.float().cpu()[m], g["logits"][m]),
               global_tokens=rel_err(out.audio_global.float().cpu(), g["global_tokens"]), local_tokens=rel_err(out.audio_local.float().cpu(), g["local_tokens"]),
               hidden_1=rel_err(model.llm.xs[1].float().cpu().view(g["hidden_1"].shape)[m], g["hidden_1"][m]))            # output of decoder layer 0 INCLUDING its injection
    losses = {k: float(v) for k, v in out.orca_losses.items()}
    ref = {k[len("orca_loss::"):]: float(v) for k, v in g.items() if k.startswith("orca_loss::")}
    print("orca forward:", {k: (round(v, 6) if isinstance(v, float) else v) for k, v in rec.items()}, losses, ref)
    assert sorted(losses) == sorted(ref)
    assert rec["global_tokens"] < 1e-2 and rec["local_tokens"] < 1e-2, rec
    assert rec["hidden_1"] < 1.5e-2 and rec["logits"] < 2e-2 and rec["dloss"] < 3e-3, rec
    for k in ref:
        assert abs(losses[k] - ref[k]) < 2e-2 * abs(ref[k]) + 2e-6, (k, losses[k], ref[k])
    total = float(out.loss) + sum(losses.values())                                           # what the trainer optimises (desta_trainer.py:56-92)
    assert abs(total - (float(g["loss"]) + sum(ref.values()))) < 4e-3
    # eval mode: no alignment loss (modeling_desta25.py:487-488), the other two stay; logits of the eval forward
    model.eval()
    out_e = model(**batch)
    assert "L_align_layerwise" not in out_e.orca_losses and "L_ortho_diversity" in out_e.orca_losses
    assert rel_err(out_e.logits.float().cpu()[m], g["logits_eval"][m]) < 2e-2
    # backward: every gradient of the trainer's total loss (LM + the three ORCA terms) against the reference's own autograd
    model.train()
    out = model(**batch)
    assert out.logits is None                                                               # dlogits took the buffer, as on the qformer_1 path
    model.backward()
    names = R.trainable_names(d, o)
    gn = sorted(float(g["grad::" + n].double().norm()) for n in names)
    floor = gn[len(gn) // 2] * 1e-2
    errs = {n: float((model.arena.grad(n).double().cpu() - g["grad::" + n].double().reshape(model.arena.shapes[n])).norm()
                     / max(float(g["grad::" + n].double().norm()), floor)) for n in names}
    a = torch.cat([model.arena.grad(n).reshape(-1).double().cpu() for n in names])
    b = torch.cat([g["grad::" + n].reshape(-1).double() for n in names])
    worst = sorted(errs, key=errs.get)[-6:]
    print("orca backward: whole arena rel", float((a - b).norm() / b.norm()), "cos", float((a @ b) / (a.norm() * b.norm())),
          [(n.replace("perception.connector.", "").replace("orca_cross_attns.", "x."), round(errs[n], 4)) for n in reversed(worst)])
    # measured: whole arena 6.5e-3 (cosine 0.99998), worst tensor 2.1 % (a gate-MLP bias); bounds at 3x
    assert float((a - b).norm() / b.norm()) < 2e-2 and float((a @ b) / (a.norm() * b.norm())) > 0.9995
    assert errs[worst[-1]] < 6.5e-2, (worst[-1], errs[worst[-1]])
    # config round trip keeps the mode and every orca_* field
    c2 = DeSTA25Config(**{k: v for k, v in cfg.to_dict().items() if k not in ("model_type", "info")})
    assert c2.connector_mode == "orca_hybrid" and c2.orca_global_num_tokens == cfg.orca_global_num_tokens and c2.orca_enabled
    with pytest.raises(NotImplementedError):
        DeSTA25Config(**{**{k: v for k, v in cfg.to_dict().items() if k not in ("model_type", "info")}, "connector_mode": "something_else"})


def test_orca_kernels_vs_oracle(golden_dir):
    """The row-wise `desta_orca_*` entry points one by one against the oracle's restatement on random inputs."""
    from desta import _hip as H
    gen = torch.Generator().manual_seed(3)
    B, T, Hd = 3, 10, 256
    x = torch.randn(B, T, Hd, generator=gen).to(torch.bfloat16)
    y = torch.empty(B * T, Hd, dtype=torch.bfloat16, device="cuda")
    H.orca_rope(x.cuda(), y, B, T, Hd, 10000.0, 2.5, round_cos_sin=False)
    assert rel_err(y.float().cpu().view(B, T, Hd), R.rope_whole_vector(x.float(), 10000.0, 2.5)) < 6e-3
    H.orca_rope(x.cuda(), y, B, T, Hd, 10000.0, 2.5, round_cos_sin=True)          # what the model passes: bf16 cos / sin, as on a bf16 x
    assert rel_err(y.float().cpu().view(B, T, Hd), R.rope_whole_vector(x, 10000.0, 2.5).float()) < 6e-3
    # local mix
    taps, rows, dd = 4, 50, 128
    e = torch.randn(taps, rows, dd, generator=gen).to(torch.bfloat16)
    lw = torch.randn(taps, generator=gen)
    out = torch.empty(rows, dd, dtype=torch.bfloat16, device="cuda")
    H.orca_local_mix(e.cuda(), lw.cuda(), taps, rows, dd, out)
    ref = (e.float() * torch.softmax(lw, 0).view(-1, 1, 1)).sum(0)
    assert rel_err(out.float().cpu(), ref) < 4e-3
    # similarity losses
    gt = torch.randn(B, 8, Hd, generator=gen).to(torch.bfloat16)
    lt = torch.randn(B, 130, Hd, generator=gen).to(torch.bfloat16)
    od = R.OrcaDims(ortho_diversity_weight=1.0, ortho_weight_qformer_local=1.0)
    want = R.orca_losses(od, gt.float(), lt.float(), [])
    part = torch.empty(B * 8, device="cuda")
    H.orca_sim_loss(gt.cuda(), gt.cuda(), None, B, 8, 8, 8, Hd, True, part)
    assert abs(float(part.sum()) / (B * 64) - float(want["L_ortho_diversity"])) < 1e-5 + 1e-4 * float(want["L_ortho_diversity"])
    idx = torch.linspace(0, 129, 100, dtype=torch.long).to("cuda", torch.int32)
    H.orca_sim_loss(gt.cuda(), lt.cuda(), idx, B, 8, 100, 130, Hd, False, part)
    assert abs(float(part.sum()) / (B * 800) - float(want["L_ortho_qformer_local"])) < 1e-6 + 1e-4 * float(want["L_ortho_qformer_local"])
    # gate + residual
    M = 37
    hs = torch.randn(M, Hd, generator=gen).to(torch.bfloat16)
    cr = torch.randn(M, Hd, generator=gen).to(torch.bfloat16)
    g1 = torch.randn(M, Hd // 4, generator=gen).to(torch.bfloat16)
    w2, b2 = torch.randn(Hd // 4, generator=gen) / 8, torch.tensor([0.1])
    hsd = hs.clone().cuda()
    gate = torch.empty(M, device="cuda")
    H.orca_gate_residual(hsd, Hd, cr.cuda(), g1.cuda(), w2.cuda(), b2.cuda(), M, Hd, Hd // 4, gate_out=gate)
    gref = torch.sigmoid(g1.float() @ w2 + b2)
    assert rel_err(gate.cpu(), gref) < 1e-5
    assert rel_err(hsd.float().cpu(), hs.float() + gref[:, None] * cr.float()) < 6e-3
    # alignment
    a = torch.randn(B, T, Hd, generator=gen).to(torch.bfloat16)
    S = 12
    hid = torch.randn(B, S, Hd, generator=gen).to(torch.bfloat16)
    spans = torch.tensor([[0, 2, 7], [1, 0, 12], [2, 11, 12]], dtype=torch.int32)
    outa = torch.empty(3, device="cuda")
    H.orca_align(a.cuda(), T, hid.cuda(), Hd, S * Hd, Hd, spans.cuda(), 3, outa)
    ra = torch.stack([1 - torch.nn.functional.cosine_similarity(a[i].float().mean(0), hid[r, s0:s1].float().mean(0), dim=0) for i, (r, s0, s1) in enumerate(spans.tolist())])
    assert float((outa.cpu() - ra).abs().max()) < 1e-4


def test_orca_trainer_steps_follow_the_oracle(golden_dir):
    """Three optimizer steps of `DeSTA25Trainer` on the ORCA model (total loss = LM + ORCA terms, clip 1.0, Adafactor over the whole
    ORCA parameter set: connector + 2 x gated cross-attention) against the oracle's `train`-style restatement: same total loss per
    step to bf16 noise, parameters move, loss goes down."""
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    from desta.trainer.desta_trainer import DeSTA25Trainer, TrainingArguments
    import orca_oracle
    g, d, o, w, batch, cfg = _case(golden_dir)
    model = DeSTA25AudioModel(cfg, weights=w)
    tr = DeSTA25Trainer(model, args=TrainingArguments(learning_rate=2e-3, warmup_steps=0, max_steps=3, logging_steps=1, overlap_comm=False, overlap_encoder=False))
    names = R.trainable_names(d, o)
    wo = {k: v.clone() for k, v in w.items()}
    st = O.adafactor_init([wo[n] for n in names])
    theta = float(g["rope_theta_used"])
    orig = orca_oracle.rope_whole_vector
    orca_oracle.rope_whole_vector = lambda x, th, sc: orig(x, theta, sc)
    try:
        hip, ref = [], []
        for i in range(3):
            hip.append(float(tr.training_step(batch)))
            for n in names:
                wo[n].requires_grad_(True)
                wo[n].grad = None
            loss, _, losses = R.model_forward(wo, d, o, batch, training=True)
            tot = R.total_loss(loss, losses)
            tot.backward()
            grads = [wo[n].grad.detach().clone() for n in names]
            params = [wo[n].detach() for n in names]
            O.clip_grad_norm(grads, 1.0)
            O.adafactor_step(params, grads, st, O.linear_warmup_lr(i, 2e-3, 0, 3), [0.01 if dm else 0.0 for dm in O.decay_mask(names)])
            for n, p_ in zip(names, params):
                wo[n] = p_.detach()
            ref.append(float(tot))
    finally:
        orca_oracle.rope_whole_vector = orig
    print("orca trainer: total loss HIP", hip, "oracle", ref)
    assert all(abs(a - b) < 6e-3 for a, b in zip(hip, ref)), (hip, ref)                    # measured 6e-4 / 1.1e-3 / 1.4e-3
    assert hip[-1] < hip[0]
    assert set(tr.log_history[0]) >= {"train/lm_loss", "train/L_ortho_diversity", "train/L_align_layerwise", "train/orca_total", "train/loss"}


def _oracle_with_theta(theta):
    """The oracle's cross-attention rotation reads `d.rope_theta`; the golden was made under transformers 5.x where the reference's
    getattr falls back to 10000.0 (see OrcaHIP.__init__) — same substitution as tests/test_oracle_pin.py."""
    orig = R.rope_whole_vector
    R.rope_whole_vector = lambda x, th, scale: orig(x, theta, scale)
    return orig


@pytest.mark.parametrize("gca", [False, True, "nolocal"])
def test_orca_generation_and_global_cross_attn_variant(golden_dir, gca):
    """(a) `orca_global_cross_attn: true` (global | local tokens in the injected sequence; the shipped ORCA configs carry the switch):
    forward against the reference-made golden, EVERY gradient against the oracle's autograd (the oracle is pinned to the golden's
    subset in tests/test_oracle_pin.py) and the golden's subset directly.  (b) `_generate_step` with deep injection — gated
    cross-attention behind every layer of the prompt pass and of every KV-cached decode step, audio K|V projected once per layer —
    teacher-forced on the tokens the REFERENCE's own ORCA `_generate_step` produced, per-step logits against the oracle; then free
    running (structure of tests/test_gpu_generate.py::test_generate_step_vs_reference_golden)."""
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    g, d, o, w, batch, cfg = _case(golden_dir, gca)
    model = DeSTA25AudioModel(cfg, weights=w)
    names = R.trainable_names(d, o)
    orig = _oracle_with_theta(float(g["rope_theta_used"]))
    try:
        if gca:
            model.train()
            out = model(**batch, keep_logits=True)
            m = g["attention_mask"].bool()
            rec = dict(dloss=abs(float(out.loss) - float(g["loss"])), logits=rel_err(out.logits.float().cpu()[m], g["logits"][m]))
            losses = {k: float(v) for k, v in out.orca_losses.items()}
            ref = {k[len("orca_loss::"):]: float(v) for k, v in g.items() if k.startswith("orca_loss::")}
            assert rec["logits"] < 2e-2 and rec["dloss"] < 3e-3, rec
            for k in ref:
                assert abs(losses[k] - ref[k]) < 2e-2 * abs(ref[k]) + 2e-6, (k, losses[k], ref[k])
            model.backward()
            for n in names:
                w[n].requires_grad_(True)
            loss_o, _, losses_o = R.model_forward(w, d, o, batch, training=True)
            R.total_loss(loss_o, losses_o).backward()
            go = {n: w[n].grad.detach().double() for n in names}
            for n in names:
                w[n].requires_grad_(False)
            gn = sorted(float(go[n].norm()) for n in names)
            floor = gn[len(gn) // 2] * 1e-2
            errs = {n: float((model.arena.grad(n).double().cpu() - go[n].reshape(model.arena.shapes[n])).norm() / max(float(go[n].norm()), floor)) for n in names}
            a = torch.cat([model.arena.grad(n).reshape(-1).double().cpu() for n in names])
            b = torch.cat([go[n].reshape(-1) for n in names])
            worst = max(errs, key=errs.get)
            print("orca gca:", rec, "grads rel", float((a - b).norm() / b.norm()), "cos", float((a @ b) / (a.norm() * b.norm())), worst, errs[worst])
            assert float((a - b).norm() / b.norm()) < 2e-2 and float((a @ b) / (a.norm() * b.norm())) > 0.9995
            assert errs[worst] < 6.5e-2, (worst, errs[worst])
            for k in g:
                if k.startswith("grad::"):
                    n = k[len("grad::"):]
                    e = float((model.arena.grad(n).double().cpu() - g[k].double().reshape(model.arena.shapes[n])).norm() / max(float(g[k].double().norm()), floor))
                    assert e < 6.5e-2, (n, e)
        model.eval()
        n_ctx, ref_ids = int(g["gen_ctx_len"]), g["gen_ids"]
        T = ref_ids.shape[1]
        inputs = {"context_input_ids": batch["input_ids"][:, :n_ctx], "context_attention_mask": batch["attention_mask"][:, :n_ctx],
                  "context_batch_start_positions": batch["batch_start_positions"], "batch_features": batch["batch_features"],
                  "batch_transcription_ids": batch["batch_transcription_ids"]}
        ids_f, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref_ids, collect_logits=True)
        assert ids_f.cpu().tolist() == ref_ids.tolist()
        with torch.no_grad():
            lo = R.generate(w, d, o, inputs, T, 0, forced_tokens=ref_ids)[1]
        assert logits.shape == lo.shape
        es = [rel_err(logits[t].float(), lo[t]) for t in range(T)]
        pick = logits.float().cpu().argmax(-1)
        gap = lo.max(-1).values - lo.gather(-1, pick.unsqueeze(-1)).squeeze(-1)
        print("orca generate (gca %s): per-step logits rel" % gca, [round(e, 4) for e in es], "gap/std", float((gap / lo.std(-1)).max()))
        assert max(es) < 3e-2, es
        assert float((gap / lo.std(-1)).max()) < 0.1 and float((pick == lo.argmax(-1)).float().mean()) >= 0.9
        # without the injection the same prompt gives other logits: the hook is live in the decode steps, not only in the prompt pass
        ids = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False).cpu()
        print("   free-running agreement with the reference's tokens:", float((ids == ref_ids).float().mean()))
        assert (ids[:, 0] == ref_ids[:, 0]).all()
        with torch.no_grad():
            lo2 = R.generate(w, d, o, inputs, T, 0, forced_tokens=ids)[1]
        gap2 = lo2.max(-1).values - lo2.gather(-1, ids.t().unsqueeze(-1)).squeeze(-1)
        assert float((gap2 / lo2.std(-1)).max()) < 0.1
        saved = model.config.orca_deep_injection_enabled
        model.config.orca_deep_injection_enabled = False
        try:
            _, logits_off = model._generate_step(inputs, pad_token_id=0, max_new_tokens=T, do_sample=False, forced_tokens=ref_ids, collect_logits=True)
        finally:
            model.config.orca_deep_injection_enabled = saved
        assert min(rel_err(logits_off[t].float(), lo[t]) for t in range(1, T)) > 3 * max(es)
    finally:
        R.rope_whole_vector = orig


def test_orca_cross_attention_head_size_80_vs_oracle():
    """`nn.MultiheadAttention(hidden, llm heads)` has head size hidden / heads — 80 for the shipped Qwen3-4B ORCA config (2560 / 32),
    which the flash kernels (64 / 128) run zero-padded to 128 (`OrcaHIP.hdp`): loss, logits, EVERY gradient (un-padded back into the
    arena) and teacher-forced generation logits against the oracle at hidden 1280 / 16 heads (head size 80; the decoder's own q width
    16 x 64 = 1024 != hidden, as in Qwen3-4B), global | local tokens injected, left padding, a transcription span in one row."""
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = copy.copy(O.tiny_dims(False))
    d.llm_h, d.llm_hq, d.llm_hkv, d.llm_hd, d.llm_inter = 1280, 16, 4, 64, 768
    kg = 6
    o = R.OrcaDims(global_num_tokens=kg, local_downsample=4, local_kernel_size=5, ortho_diversity_weight=0.05, ortho_weight_qformer_local=0.05,
                   align_weight_local=0.05, global_cross_attn=True)
    w = R.init_weights(d, o, seed=11)
    d.prompt_size = kg
    batch = O.synthetic_batch(d, B=2, S_ctx=9, S_tgt=14, seed=4, pad=[3, 0])
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=4, orca_local_kernel_size=5,
                        orca_ortho_diversity_weight=0.05, orca_ortho_weight_qformer_local=0.05, orca_align_weight_local=0.05, orca_global_cross_attn=True)
    model = DeSTA25AudioModel(cfg, weights=w)
    assert model.orca.hd == 80 and model.orca.hdp == 128 and model.orca.padded
    names = R.trainable_names(d, o)
    model.train()
    out = model(**batch, keep_logits=True)
    for n in names:
        w[n].requires_grad_(True)
    loss_o, logits_o, losses_o = R.model_forward(w, d, o, batch, training=True)
    R.total_loss(loss_o, losses_o).backward()
    m = batch["attention_mask"].bool()
    rec = dict(dloss=abs(float(out.loss) - float(loss_o)), logits=rel_err(out.logits.float().cpu()[m], logits_o.detach()[m]))
    for k, v in losses_o.items():
        assert abs(float(out.orca_losses[k]) - float(v)) < 2e-2 * abs(float(v)) + 2e-6, (k, float(out.orca_losses[k]), float(v))
    model.backward()
    go = {n: w[n].grad.detach().double() for n in names}
    for n in names:
        w[n].requires_grad_(False)
    gn = sorted(float(go[n].norm()) for n in names)
    floor = gn[len(gn) // 2] * 1e-2
    errs = {n: float((model.arena.grad(n).double().cpu() - go[n].reshape(model.arena.shapes[n])).norm() / max(float(go[n].norm()), floor)) for n in names}
    a = torch.cat([model.arena.grad(n).reshape(-1).double().cpu() for n in names])
    b = torch.cat([go[n].reshape(-1) for n in names])
    worst = max(errs, key=errs.get)
    rec.update(grad=float((a - b).norm() / b.norm()), cos=float((a @ b) / (a.norm() * b.norm())), worst=(worst, round(errs[worst], 4)))
    print("orca head size 80:", rec)
    assert rec["dloss"] < 3e-3 and rec["logits"] < 2e-2, rec
    assert rec["grad"] < 2e-2 and rec["cos"] > 0.9995 and errs[worst] < 6.5e-2, rec
    model.eval()
    n_ctx = 9 + 3 + kg
    inputs = {"context_input_ids": batch["input_ids"][:, :n_ctx], "context_attention_mask": batch["attention_mask"][:, :n_ctx],
              "context_batch_start_positions": batch["batch_start_positions"], "batch_features": batch["batch_features"],
              "batch_transcription_ids": batch["batch_transcription_ids"]}
    with torch.no_grad():
        ref_ids, lo = R.generate(w, d, o, inputs, 5, 0)
    _, logits = model._generate_step(inputs, pad_token_id=0, max_new_tokens=5, do_sample=False, forced_tokens=ref_ids, collect_logits=True, eos_token_id=[])
    es = [rel_err(logits[t].float(), lo[t]) for t in range(5)]
    assert max(es) < 3e-2, es


@pytest.mark.parametrize("name", ["desta25_qwen3-0.6b_ORCAHybrid", "desta25_qwen3-4b_ORCAHybrid", "desta25_llama31-8B_ORCAHybrid"])
def test_orca_full_size_step_properties(name):
    """The three ORCA configs the reference ships at their TRUE shapes (whisper-large-v3, 6-layer global Q-Former, 28 / 36 / 32 decoder
    layers each followed by a trainable gated cross-attention over 64 | 8 global + 375 local tokens), through size-independent
    properties like tests/test_gpu_fullsize.py: CE ~ ln V at random init, finite non-zero gradients in every tensor family, a
    bit-identical rerun, loss descent over a few optimizer steps on a repeated batch, greedy generation rerun-stable."""
    import math
    from desta import _hip as H
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    from desta.synthetic import FULL_CONFIGS, RandomWeights, synthetic_inputs, synthetic_waveform
    from desta.trainer.desta_trainer import DeSTA25Trainer, TrainingArguments
    cfg = DeSTA25Config(**FULL_CONFIGS[name])
    model = DeSTA25AudioModel(cfg, weights=RandomWeights(cfg, "cuda:0", seed=0), device="cuda:0")
    c = cfg.llm_config
    per_layer = 4 * c.hidden_size ** 2 + 4 * c.hidden_size + (c.hidden_size // 4) * (c.hidden_size + 2) + 1 + 2 * c.hidden_size
    assert sum(math.prod(model.arena.shapes[n]) for n in model.arena.names if n.startswith("orca_cross_attns.")) == c.num_hidden_layers * per_layer
    assert model.orca.hd == c.hidden_size // c.num_attention_heads and model.orca.padded == ("4b" in name)
    B = 4
    batch = synthetic_inputs(cfg, B, 40, 200, "cuda:0", seed=3, S_tr=16)        # 16 transcription tokens per clip: the alignment loss reads their span
    assert batch["input_ids"].shape[1] == 40 + cfg.orca_global_num_tokens + 16 + 200
    batch["batch_features"] = H.logmel(synthetic_waveform(B, "cuda:0", seed=3), 128)
    model.train()
    model._fwd_count = 0
    out = model(**batch)
    loss0 = float(out.loss)
    assert abs(loss0 - math.log(c.vocab_size)) < 1.0, loss0
    assert sorted(out.orca_losses) == ["L_align_layerwise", "L_ortho_diversity", "L_ortho_qformer_local"]
    aux0 = {k: float(v) for k, v in out.orca_losses.items()}
    assert all(math.isfinite(v) and v >= 0 for v in aux0.values()), aux0
    assert out.audio_local.shape == (B, 375, c.hidden_size) and out.audio_global.shape == (B, cfg.orca_global_num_tokens, c.hidden_size)
    model.backward()
    g1 = model.arena.grads.clone()
    assert torch.isfinite(g1).all()
    for fam in ("perception.connector.global_qformer.", "perception.connector.local_conv.weight", "perception.connector.global_queries.",
                "orca_cross_attns.0.cross_attn.in_proj_weight", f"orca_cross_attns.{c.num_hidden_layers - 1}.gate_proj.2.weight",     # (gate_proj.0 starts with a zero gradient: gate_proj.2.weight is zero-initialised, :382-383)
                f"orca_cross_attns.{c.num_hidden_layers // 2}.cross_attn.out_proj.weight"):
        assert any(float(model.arena.grad(n).abs().max()) > 0 for n in model.arena.names if n.startswith(fam)), fam
    model.mark_weights_updated()
    model._fwd_count = 0
    out = model(**batch)
    model.backward()
    assert float(out.loss) == loss0 and torch.equal(model.arena.grads, g1)              # bit-identical rerun
    del g1
    tr = DeSTA25Trainer(model, args=TrainingArguments(learning_rate=1e-3, warmup_steps=0, max_steps=100, logging_steps=100))
    losses = tr.train([batch] * 5)
    print(name, "lm loss", round(loss0, 4), aux0, "total loss over 5 steps", [round(x, 4) for x in losses])
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0] - 0.03, losses
    model.eval()
    t = synthetic_inputs(cfg, 2, 24, 8, "cuda:0", seed=9)
    inputs = {"context_input_ids": t["input_ids"], "context_attention_mask": t["attention_mask"], "context_batch_start_positions": t["batch_start_positions"],
              "batch_features": batch["batch_features"][:2], "batch_transcription_ids": t["batch_transcription_ids"]}
    ids = model._generate_step(inputs, pad_token_id=0, max_new_tokens=4, do_sample=False, eos_token_id=[])
    assert ids.shape == (2, 4) and torch.equal(ids, model._generate_step(inputs, pad_token_id=0, max_new_tokens=4, do_sample=False, eos_token_id=[]))


def test_orca_weight_gradient_gemm_forms_agree():
    """`OrcaHIP._dW` picks explicit transposes + the 256x256 NT kernel for the large projections of a full-size decoder (no tiny-model
    test reaches that branch) and transposed-storage operands otherwise: both against fp32 matmul, with a token count that is not a
    multiple of 64 (zero pad columns of the scratch), a caller-held X^T, and a second call that reuses the scratch."""
    from desta.models.modeling_desta25 import OrcaHIP
    o = OrcaHIP.__new__(OrcaHIP)
    o._tb, o.dev = {}, torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    for M, N, K in ((1100, 4096, 2048), (1100, 4096, 2048), (1100, 512, 256), (1088, 512, 256)):
        dY = torch.randn(M, N, generator=gen).to(torch.bfloat16).cuda()
        X = torch.randn(M, K, generator=gen).to(torch.bfloat16).cuda()
        gw, gb = torch.empty(N, K, device="cuda"), torch.empty(N, device="cuda")
        o._dW(dY, X, M, N, K, gw, gb)
        ref = dY.float().T @ X.float()
        assert rel_err(gw.cpu(), ref.cpu()) < 2e-5, (M, N, K)
        assert rel_err(gb.cpu(), dY.float().sum(0).cpu()) < 1e-5
        if N * K >= 1 << 23:
            assert ("dY", N, 1152) in o._tb                                     # the transposed form ran (r64(1100) = 1152 columns)
            gw2 = torch.empty_like(gw)
            o._dW(dY, X, M, N, K, gw2, None, xT=o._transposed("audio", X, M, K))
            assert torch.equal(gw, gw2)


def test_orca_use_all_layers_vs_oracle():
    """`orca_use_all_layers: true` (ORCAHybridConnector.__init__ :221-224): EVERY encoder layer is tapped — here 10 of 10 (more than the
    8-tap register arrays of rounds 1-3; whisper-large has 32) — one global query set and one Q-Former pass per layer, softmax mixes
    over all of them in both branches.  Loss, the three ORCA losses and every gradient against the oracle."""
    from desta.models.modeling_desta25 import DeSTA25AudioModel, DeSTA25Config
    d = copy.copy(O.tiny_dims(False))
    d.enc_layers, d.taps = 10, tuple(range(10))
    kg = 4
    o = R.OrcaDims(global_num_tokens=kg, local_downsample=4, local_kernel_size=5, ortho_diversity_weight=0.05, ortho_weight_qformer_local=0.05,
                   align_weight_local=0.05, global_cross_attn=True)
    w = R.init_weights(d, o, seed=13)
    d.prompt_size = kg + 2
    batch = O.synthetic_batch(d, B=2, S_ctx=6, S_tgt=10, seed=8, pad=[0, 2])
    g = torch.Generator().manual_seed(2)
    batch["batch_transcription_ids"] = [torch.randint(3, d.vocab, (1, 2), generator=g) for _ in range(2)]
    kw = dict(connector_mode="orca_hybrid", orca_enabled=True, orca_use_all_layers=True, orca_global_num_tokens=kg, orca_local_downsample=4,
              orca_local_kernel_size=5, orca_ortho_diversity_weight=0.05, orca_ortho_weight_qformer_local=0.05, orca_align_weight_local=0.05,
              orca_global_cross_attn=True)
    cfg = cfg_from_dims(d, **kw)
    # the config derives the tap list itself when none is given (encoder depth from the encoder config)
    c2 = DeSTA25Config(llm_model_id="x", encoder_model_id="openai/whisper-tiny", llm_config=cfg.to_dict()["llm_config"],
                       encoder_config=cfg.to_dict()["encoder_config"], **kw)
    assert c2.target_layer_ids == list(range(10)) and cfg.target_layer_ids == list(range(10))
    model = DeSTA25AudioModel(cfg, weights=w)
    names = R.trainable_names(d, o)
    assert sorted(model.trainable_parameter_names) == sorted(names)
    model.train()
    out = model(**batch, keep_logits=True)
    for n in names:
        w[n].requires_grad_(True)
    loss_o, logits_o, losses_o = R.model_forward(w, d, o, batch, training=True)
    R.total_loss(loss_o, losses_o).backward()
    m = batch["attention_mask"].bool()
    assert abs(float(out.loss) - float(loss_o)) < 3e-3 and rel_err(out.logits.float().cpu()[m], logits_o.detach()[m]) < 2e-2
    for k, v in losses_o.items():
        assert abs(float(out.orca_losses[k]) - float(v)) < 2e-2 * abs(float(v)) + 2e-6, (k, float(out.orca_losses[k]), float(v))
    model.backward()
    go = {n: w[n].grad.detach().double() for n in names}
    gn = sorted(float(go[n].norm()) for n in names)
    floor = gn[len(gn) // 2] * 1e-2
    errs = {n: float((model.arena.grad(n).double().cpu() - go[n].reshape(model.arena.shapes[n])).norm() / max(float(go[n].norm()), floor)) for n in names}
    a = torch.cat([model.arena.grad(n).reshape(-1).double().cpu() for n in names])
    b = torch.cat([go[n].reshape(-1) for n in names])
    worst = max(errs, key=errs.get)
    print("orca all layers: grads rel", float((a - b).norm() / b.norm()), "cos", float((a @ b) / (a.norm() * b.norm())), worst, errs[worst])
    assert float((a - b).norm() / b.norm()) < 2e-2 and float((a @ b) / (a.norm() * b.norm())) > 0.9995 and errs[worst] < 6.5e-2


def test_orca_local_index_is_the_reference_device_linspace():
    """The global / local orthogonality loss reads 100 sampled local tokens above 100 (modeling_desta25.py:1188-1194); the reference
    builds the list with `torch.linspace(..., dtype=torch.long, device=l_norm.device)`.  For every Tl the shipped encoders can give
    (101 .. 1500) the model's list is that device list, built once per Tl; how many differ from the CPU `linspace` is printed."""
    from desta.models.modeling_desta25 import OrcaHIP
    o = OrcaHIP.__new__(OrcaHIP)
    o.dev, o._lidx = torch.device("cuda:0"), {}
    assert o.local_index(24) is None and o.local_index(100) is None
    differ = []
    for Tl in range(101, 1501):
        want = torch.linspace(0, Tl - 1, 100, dtype=torch.long, device="cuda:0")
        got = o.local_index(Tl)
        assert got.dtype == torch.int32 and got.device == want.device and torch.equal(got.long(), want), Tl
        assert o.local_index(Tl) is got
        if not torch.equal(want.cpu(), torch.linspace(0, Tl - 1, 100, dtype=torch.long)):
            differ.append(Tl)
    print(f"device vs CPU linspace: {len(differ)} of 1400 lists differ", differ[:20])


def test_orca_sampled_local_tokens_vs_oracle():
    """The shipped local-token path: a 1500-position encoder (whisper's 1500 frames) gives Tl = 375 local tokens, so
    `L_ortho_qformer_local` reads the reference's sample of 100 of them (index list on the y side of the forward and on the x side of
    the local gradient).  Loss, the three ORCA losses and every gradient against the oracle given the same (device) index list."""
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = copy.copy(O.tiny_dims(False))
    d.enc_T = 1500
    kg = 4
    o = R.OrcaDims(global_num_tokens=kg, local_downsample=4, local_kernel_size=5, ortho_diversity_weight=0.05, ortho_weight_qformer_local=0.5,
                   align_weight_local=0.05)
    w = R.init_weights(d, o, seed=17)
    d.prompt_size = kg + 2
    batch = O.synthetic_batch(d, B=2, S_ctx=6, S_tgt=10, seed=5, pad=[2, 0])
    g = torch.Generator().manual_seed(4)
    batch["batch_transcription_ids"] = [torch.randint(3, d.vocab, (1, 2), generator=g) for _ in range(2)]
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=4,
                        orca_local_kernel_size=5, orca_ortho_diversity_weight=0.05, orca_ortho_weight_qformer_local=0.5, orca_align_weight_local=0.05)
    model = DeSTA25AudioModel(cfg, weights=w)
    names = R.trainable_names(d, o)
    model.train()
    out = model(**batch, keep_logits=True)
    assert out.audio_local.shape[1] == 375
    idx = model.orca.local_index(375)
    assert idx is not None and idx.numel() == 100
    for n in names:
        w[n].requires_grad_(True)
    loss_o, logits_o, losses_o = R.model_forward(w, d, o, batch, training=True, local_index=idx)
    R.total_loss(loss_o, losses_o).backward()
    m = batch["attention_mask"].bool()
    assert abs(float(out.loss) - float(loss_o)) < 3e-3 and rel_err(out.logits.float().cpu()[m], logits_o.detach()[m]) < 2e-2
    assert sorted(out.orca_losses) == sorted(losses_o) == ["L_align_layerwise", "L_ortho_diversity", "L_ortho_qformer_local"]
    for k, v in losses_o.items():
        assert abs(float(out.orca_losses[k]) - float(v)) < 2e-2 * abs(float(v)) + 2e-6, (k, float(out.orca_losses[k]), float(v))
    model.backward()
    go = {n: w[n].grad.detach().double() for n in names}
    gn = sorted(float(go[n].norm()) for n in names)
    floor = gn[len(gn) // 2] * 1e-2
    errs = {n: float((model.arena.grad(n).double().cpu() - go[n].reshape(model.arena.shapes[n])).norm() / max(float(go[n].norm()), floor)) for n in names}
    a = torch.cat([model.arena.grad(n).reshape(-1).double().cpu() for n in names])
    b = torch.cat([go[n].reshape(-1) for n in names])
    worst = max(errs, key=errs.get)
    print("orca sampled local tokens:", {k: float(v) for k, v in out.orca_losses.items()}, "grads rel", float((a - b).norm() / b.norm()),
          "cos", float((a @ b) / (a.norm() * b.norm())), worst, errs[worst])
    assert float((a - b).norm() / b.norm()) < 2e-2 and float((a @ b) / (a.norm() * b.norm())) > 0.9995 and errs[worst] < 6.5e-2


def test_orca_checkpoint_resume_and_hf_adafactor_interop(golden_dir, tmp_path):
    """ORCA through the checkpoint wire format: `checkpoint-<step>/model.safetensors` holds exactly the reference's trainable ORCA keys,
    a resumed run reproduces the uninterrupted one bit for bit, `optimizer.pt` loads into a REAL `transformers.Adafactor` (decay / no-decay
    groups in named_parameters order — incl. the 3-D Conv1d weight, whose factored state has the shapes HF gives it) and both take the
    same next step, and a checkpoint written under the reference's old `ocar_cross_attns` prefix (:1300-1309) loads."""
    from safetensors.torch import load_file, save_file
    from transformers.optimization import Adafactor
    from desta.models.modeling_desta25 import DeSTA25AudioModel, reference_parameter_names
    from desta.trainer.desta_trainer import DeSTA25Trainer, TrainingArguments
    g, d, o, w, batch, cfg = _case(golden_dir, True)
    batches = [batch] * 4
    args = TrainingArguments(learning_rate=1e-3, warmup_steps=2, max_steps=10, logging_steps=1, overlap_comm=False)

    def fresh():
        m = DeSTA25AudioModel(cfg, weights=w)
        return m, DeSTA25Trainer(m, args=args)
    m_a, t_a = fresh()
    la = t_a.train(batches)
    m_b, t_b = fresh()
    lb = t_b.train(batches[:2])
    ck = str(tmp_path / "checkpoint-2")
    t_b.save_checkpoint(ck)
    sd = load_file(os.path.join(ck, "model.safetensors"))
    names = reference_parameter_names(m_b.config)
    assert sorted(sd) == sorted(R.trainable_names(d, o)) == sorted(names)
    m_c, t_c = fresh()
    t_c.resume_from_checkpoint(ck)
    lc = t_c.train(batches[2:])
    assert lb + lc == la and torch.equal(m_c.arena.params, m_a.arena.params)
    # HF interop
    params = {n: torch.nn.Parameter(sd[n].clone()) for n in names}
    dm = dict(zip(names, O.decay_mask(names)))
    hf = Adafactor([{"params": [params[n] for n in names if dm[n]], "weight_decay": 0.01},
                    {"params": [params[n] for n in names if not dm[n]], "weight_decay": 0.0}], lr=1e-3, scale_parameter=False, relative_step=False)
    hf.load_state_dict(torch.load(os.path.join(ck, "optimizer.pt"), weights_only=True))
    conv = hf.state[params["perception.connector.local_conv.weight"]]
    h = d.llm_h
    assert tuple(conv["exp_avg_sq_row"].shape) == (h, h) and tuple(conv["exp_avg_sq_col"].shape) == (h, o.local_kernel_size)
    m_d, t_d = fresh()
    t_d.resume_from_checkpoint(ck)
    gen = torch.Generator().manual_seed(9)
    for n in names:
        gr = 0.01 * torch.randn(params[n].shape, generator=gen)
        params[n].grad = gr.clone()
        m_d.arena.grad(n).copy_(gr)
    torch.nn.utils.clip_grad_norm_(list(params.values()), 1.0)
    lr = O.linear_warmup_lr(2, 1e-3, 2, 10)
    for gq in hf.param_groups:
        gq["lr"] = lr
    hf.step()
    t_d.optimizer.step(lr)
    for n in names:
        torch.testing.assert_close(m_d.arena.param(n).cpu(), params[n].detach(), rtol=1e-5, atol=1e-6)
    # old checkpoints spell the cross-attention prefix `ocar_cross_attns`
    old = str(tmp_path / "old")
    os.makedirs(old)
    save_file({k.replace("orca_cross_attns.", "ocar_cross_attns."): v for k, v in sd.items()}, os.path.join(old, "model.safetensors"))
    m_b.config.save_pretrained(old)
    m_e = DeSTA25AudioModel.from_pretrained(old, weights={k: v for k, v in w.items() if not (k.startswith("perception.connector.") or k.startswith("orca_cross_attns."))})
    for n in names:
        assert torch.equal(m_e.arena.param(n).cpu(), sd[n].reshape(m_e.arena.shapes[n])), n


def test_checkpoint_with_all_layers_reconfigures_a_default_model(tmp_path):
    """The reference's layer-count alignment (modeling_desta25.py:1311-1345; its `test_layer_alignment.py` loads an all-layers checkpoint
    into a default-configured model): `global_layer_weights` [K, L] of the checkpoint decides how many encoder layers are tapped.
    Both doors: `from_pretrained` (config.json says 4 taps, the tensors say 10 = every encoder layer) and `load_state_dict` on a live
    default model, which rebuilds its trainable half.  The reloaded models reproduce the all-layers model's forward bit for bit."""
    import json
    from safetensors.torch import load_file
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = copy.copy(O.tiny_dims(False))
    d.enc_layers, d.taps = 10, tuple(range(10))
    kg = 4
    o = R.OrcaDims(global_num_tokens=kg, local_downsample=4, local_kernel_size=5, global_cross_attn=True)
    w = R.init_weights(d, o, seed=21)
    kw = dict(connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=4, orca_local_kernel_size=5,
              orca_global_cross_attn=True)
    m_all = DeSTA25AudioModel(cfg_from_dims(d, orca_use_all_layers=True, **kw), weights=w)
    d.prompt_size = kg
    batch = O.synthetic_batch(d, B=2, S_ctx=6, S_tgt=10, seed=8)
    m_all.eval()
    ref = m_all(**batch)
    m_all.save_pretrained(str(tmp_path / "ck"))
    # a config.json as a default (4-tap) run would have written it
    d4 = copy.copy(d)
    d4.taps = (0, 1, 2, 3)
    cfg4 = cfg_from_dims(d4, **kw)
    cfg4.save_pretrained(str(tmp_path / "ck"))
    assert json.load(open(tmp_path / "ck" / "config.json"))["target_layer_ids"] == [0, 1, 2, 3]
    base = {k: v for k, v in w.items() if not (k.startswith("perception.connector.") or k.startswith("orca_cross_attns."))}
    m1 = DeSTA25AudioModel.from_pretrained(str(tmp_path / "ck"), weights=base)
    assert m1.config.orca_use_all_layers and m1.config.target_layer_ids == list(range(10))
    m1.eval()
    out1 = m1(**batch)
    assert float(out1.loss) == float(ref.loss) and torch.equal(out1.logits, ref.logits)
    # the live-model door
    m2 = DeSTA25AudioModel(cfg_from_dims(d4, **kw), weights=base)
    assert m2.arena.shapes["perception.connector.global_layer_weights"] == (kg, 4)
    m2.eval()
    m2(**batch)                                                                  # buffers of the 4-tap shape exist before the reload
    missing, unexpected = m2.load_state_dict(load_file(str(tmp_path / "ck" / "model.safetensors")), strict=True)
    assert not missing and not unexpected and m2.arena.shapes["perception.connector.global_layer_weights"] == (kg, 10)
    assert m2.config.orca_use_all_layers and len(m2.trainable_parameter_names) == len(m_all.trainable_parameter_names)
    out2 = m2(**batch)
    assert float(out2.loss) == float(ref.loss) and torch.equal(out2.logits, ref.logits)
