"""GPU: the fused clip + Adafactor step (csrc/adafactor.hip through desta.optim.FusedAdafactor and ParamArena) held PER ELEMENT
to a float64 reference: every parameter, every state slot, the global norm (workspace[0]) and the clip coefficient (workspace[1]).

Reference, bounds with their derivation, the conforming emulation and the restated plan: tests/adafactor_reference.py.  The
instrument is proved on the CPU by tests/test_adafactor_bound_host.py over the case table this file runs (adafactor_reference.CASES).

Per case three steps (beta2t = 0, 0.4257, 0.5848), each checked on its own: step k + 1 starts from the kernel's own parameters
and state after step k, so nothing compounds.  Per step
    |out - fp64| <= 2 x bound        (`FACTOR`: what the emulation leaves out - the fp32 order inside a sum, fused multiply-adds,
                                      rsqrtf / sqrtf / the division; where the bound is 0 the output must be exact)
on every element, and `max |err| / bound` is printed per case and kind of output (run with -s).  The arena padding of `params`
and `grads` and the 4-float alignment gaps of `state` hold a large finite sentinel (a read of the gradient padding would wreck
the norm) and are bitwise unchanged afterwards, as are the gradients.  Each case is run twice (bit-identical), its plan tables
are compared with adafactor_reference.plan(), and the plan cut into three launch groups gives the bits of the one-group plan.

What a kernel error turns red here while the parameters-only tests of test_gpu_kernels.py stay green: see
test_adafactor_bound_host.py (host evidence).  Tried by hand on the MI355X, once each: the column mean over `cols` in af_finalize
fails 16 of the 17 cases here (the column state 6e4 ... 2e8 bounds off; `all-zero` holds eps1 alone); one unit per batch item
for tensors with ragged rows in FusedAdafactor.__init__ passes all of test_gpu_kernels.py's Adafactor tests and fails `narrow`
and `ragged-wide` here at the plan comparison ("Adafactor against fp64").
Measured on the MI355X: profiles/r17_adafactor_fp64_tests.log."""
import math

import pytest
import torch

import adafactor_reference as A

pytestmark = pytest.mark.gpu

FACTOR = 2.0


@pytest.fixture(scope="module")
def optim():
    assert torch.cuda.is_available()
    from desta import optim
    return optim


def _names(shapes):
    """names whose decay group (desta.optim.decay_mask) is adafactor_reference.decay_of"""
    return [f"t{i}.{'weight' if d else 'bias'}" for i, d in enumerate(A.decay_of(shapes))]


def _build(optim, case, group_floats=None, monkeypatch=None):
    names = _names(case["shapes"])
    assert optim.decay_mask(names) == A.decay_of(case["shapes"])
    if group_floats is not None:
        monkeypatch.setattr(optim, "GROUP_FLOATS", group_floats)
    arena = optim.ParamArena(list(zip(names, case["shapes"])), "cuda")
    opt = optim.FusedAdafactor(arena, weight_decay=case["weight_decay"], eps1=case["eps1"], clip_threshold=case["clip_threshold"],
                               max_grad_norm=case["max_grad_norm"])
    if group_floats is not None:
        monkeypatch.undo()
    return names, arena, opt


def _masks(arena, opt, pl):
    """boolean masks of the arena padding and of the state's alignment gaps"""
    pad = torch.ones(arena.numel, dtype=torch.bool)
    for n in arena.names:
        pad[arena.offsets[n]:arena.offsets[n] + math.prod(arena.shapes[n])] = False
    gap = torch.ones(opt.state.numel(), dtype=torch.bool)
    for sl in pl["slots"]:
        for off, n in sl.values():
            gap[off:off + n] = False
    return pad.cuda(), gap.cuda()


def _load(arena, opt, names, o, pad, gap):
    """operands -> arena / state, sentinels in every element no tensor owns"""
    arena.params.fill_(A.SENTINEL)
    arena.grads.fill_(A.SENTINEL)
    opt.state.fill_(A.SENTINEL)
    for i, n in enumerate(names):
        arena.param(n).copy_(o["params"][i])
        arena.grad(n).copy_(o["grads"][i])
        for key, hf in (("row", "exp_avg_sq_row"), ("col", "exp_avg_sq_col"), ("sq", "exp_avg_sq")):
            if key in o["state"][i]:
                opt.slots[n][hf].copy_(o["state"][i][key])
    opt.workspace.fill_(float("nan"))                                   # nothing may depend on what a previous step left
    assert bool((arena.params[pad] == A.SENTINEL).all()) and bool((opt.state[gap] == A.SENTINEL).all())


def _read(arena, opt, names, shapes):
    out = {"grad_norm": opt.workspace[0].cpu(), "coef": opt.workspace[1].cpu()}
    for i, (n, s) in enumerate(zip(names, shapes)):
        out[("p", i)] = arena.param(n).cpu()
        if len(s) >= 2:
            out[("row", i)], out[("col", i)] = opt.slots[n]["exp_avg_sq_row"].cpu(), opt.slots[n]["exp_avg_sq_col"].cpu()
        else:
            out[("sq", i)] = opt.slots[n]["exp_avg_sq"].cpu()
    return out


def _exact(o, big):
    """the float64 reference and its bound, on the device for the one large case"""
    if not big:
        ref = A.exact(o)
        return o, ref, A.bound(o, ref)
    od = dict(o, params=[t.cuda() for t in o["params"]], grads=[t.cuda() for t in o["grads"]],
              state=[{k: v.cuda() for k, v in st.items()} for st in o["state"]])
    ref = A.exact(od)
    return od, ref, A.bound(od, ref)


def _assert_plan(opt, pl):
    """FusedAdafactor's tables equal adafactor_reference.plan()'s"""
    p = opt.plan
    assert opt._tensors.tolist()[:p.n_tensors] == pl["tensors"] and p.n_tensors == len(pl["tensors"])
    assert opt._units.tolist()[:p.n_units] == pl["units"] and p.n_units == len(pl["units"])
    assert opt._ucol.tolist()[:p.n_units] == pl["unit_col_off"]
    assert opt._vecs.tolist()[:p.n_vec] == pl["vecs"] and p.n_vec == len(pl["vecs"])
    assert opt._chunks.tolist()[:p.n_chunks] == pl["chunks"] and p.n_chunks == len(pl["chunks"])
    assert opt._ten_chunks.tolist()[:p.n_tensors] == pl["ten_chunks"]
    assert opt._fin.tolist()[:p.n_fin] == pl["fin"] and p.n_fin == len(pl["fin"])
    assert list(opt._ragged)[:2 * p.n_ragged] == pl["ragged_units"] and 2 * p.n_ragged == len(pl["ragged_units"])
    assert list(opt._group_bounds) == pl["group_bounds"] and p.n_groups == pl["n_groups"]
    assert p.state_floats == pl["state_floats"] and p.colpart_floats == pl["colpart_floats"]
    assert opt.arena.numel == pl["numel"] and [opt.arena.offsets[n] for n in opt.arena.names] == pl["offsets"]
    assert p.max_chunks_per_tensor == max([c[1] for c in pl["ten_chunks"]] or [0])


def _run_steps(optim, case, group_floats=None, monkeypatch=None, check=True):
    """three steps through the kernel, each from the kernel's own results -> [(params bits, state bits, workspace[:2] bits)]"""
    names, arena, opt = _build(optim, case, group_floats, monkeypatch)
    pl = A.plan(case["shapes"], group_floats or A.GROUP_FLOATS)
    _assert_plan(opt, pl)
    pad, gap = _masks(arena, opt, pl)
    params, state = A.initial(case)
    bits, worst = [], {}
    for k in range(1, A.STEPS + 1):
        o = A.operands(case, k, params, state)
        _load(arena, opt, names, o, pad, gap)
        g_before = arena.grads.clone()
        opt.step(o["lr"])
        torch.cuda.synchronize()
        assert opt.step_count == k and A.f32(1.0 - math.pow(k, opt.decay_rate)) == A.f32(o["beta2t"])
        assert torch.equal(arena.grads.view(torch.int32), g_before.view(torch.int32)), "the gradients changed"
        assert bool((arena.params[pad] == A.SENTINEL).all()), "arena padding of params written"
        assert bool((opt.state[gap] == A.SENTINEL).all()), "alignment gap of state written"
        out = _read(arena, opt, names, case["shapes"])
        bits.append((arena.params.clone(), opt.state.clone(), opt.workspace[:2].clone()))
        if check:
            od, ref, bnd = _exact(o, case["big"])
            for key in A.outputs(o):
                assert bool(torch.isfinite(out[key]).all()), (case["name"], k, key)
            kinds = A.by_kind(A.ratios(od, ref, {kk: v.to(ref[kk].device) for kk, v in out.items()}, bnd))
            print(f"\n{case['name']} step {k}: " + " ".join(f"{kd} {r:.3f}" for kd, r in kinds.items()), end="")
            for kd, r in kinds.items():
                worst[kd] = max(worst.get(kd, 0.0), r)
        params, state = A.carry(case, out)
    beyond = {kd: r for kd, r in worst.items() if not r <= FACTOR}
    assert not beyond, (case["name"], beyond)
    return bits, opt


@pytest.mark.parametrize("case", A.CASES, ids=A.CASE_IDS)
def test_step_against_fp64(optim, case, monkeypatch):
    bits, opt = _run_steps(optim, case, case["group_floats"], monkeypatch)
    if case["group_floats"]:
        assert opt.plan.n_groups >= 3
    if case["name"] == "all-ragged":
        assert opt.plan.n_chunks == 0 and opt.plan.n_vec > 0               # the 1-D tensors on their own launch
    if case["name"] == "all-zero":
        assert float(bits[-1][2][0]) == 0.0 and float(bits[-1][2][1]) == 1.0
    if not case["big"]:                                                    # a second run from the same inputs: the same bits
        again, _ = _run_steps(optim, case, case["group_floats"], monkeypatch, check=False)
        for a, b in zip(bits, again):
            assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b)), "two runs differ"


def test_group_cut_changes_launches_not_arithmetic(optim, monkeypatch):
    """The plan of small tensors cut into three launch groups (a group opened by a tensor above the limit, ragged tensors in
    between, the 1-D tensors in the last group) gives the bits of the one-group plan of the same arena."""
    case = A.CASES[A.CASE_IDS.index("groups")]
    cut, opt_cut = _run_steps(optim, case, A.SMALL_GROUP_FLOATS, monkeypatch, check=False)
    one, opt_one = _run_steps(optim, case, None, None, check=False)
    assert opt_cut.plan.n_groups == 3 and opt_one.plan.n_groups == 1 and optim.GROUP_FLOATS == A.GROUP_FLOATS
    bounds = list(opt_cut._group_bounds)
    chunks = opt_cut._chunks.tolist()
    opener = opt_cut._tensors.tolist()[chunks[bounds[1]][0]]
    assert opener[1] * opener[2] * opener[3] > A.SMALL_GROUP_FLOATS and opt_cut.plan.n_ragged == 2 and opt_cut.plan.n_vec == 2
    for a, b in zip(cut, one):
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), "parameters differ between the group cuts"
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), "state differs between the group cuts"


def test_table_reaches_every_form_and_the_kernel_takes_it(optim):
    """Each tensor's form is a function of its shape alone (af_stats :127-160, k34_update :414): what plan() names is what the
    plan tables route - chunked tensors carry chunks, ragged ones a unit range - and the table reaches every form, every
    stats_rows instantiation and a plan of three groups."""
    forms, rows, groups = set(), set(), 0
    for case in A.CASES:
        pl = A.plan(case["shapes"], case["group_floats"] or A.GROUP_FLOATS)
        forms |= set(pl["forms"])
        rows |= {ln.get("stats_rows") for ln in pl["lens"]} - {None}
        groups = max(groups, pl["n_groups"])
        fact = [i for i, s in enumerate(case["shapes"]) if len(s) >= 2]
        for ti, i in enumerate(fact):
            ragged = pl["forms"][i] in ("narrow", "ragged-wide")
            assert (pl["ten_chunks"][ti][1] == 0) == ragged
            assert (pl["tensors"][ti][6:8] in [pl["ragged_units"][j:j + 2] for j in range(0, len(pl["ragged_units"]), 2)]) == ragged
            assert pl["tensors"][ti][3] <= A.MAXSEG * 256
    assert forms == set(A.FORMS) and rows == {4, 2, 1} and groups >= 3


def test_rejections_launch_nothing(optim):
    for shapes, message in (([(40,), (7,)], "without any factored"), ([(8, 4100), (40,)], "4100 columns")):
        names = [f"t{i}.weight" for i in range(len(shapes))]
        arena = optim.ParamArena(list(zip(names, shapes)), "cuda")
        opt = optim.FusedAdafactor(arena)
        arena.params.fill_(1.25)
        arena.grads.fill_(0.5)
        opt.state.fill_(0.75)
        with pytest.raises(RuntimeError, match=message):
            opt.step(1e-2)
        torch.cuda.synchronize()
        assert bool((arena.params == 1.25).all()) and bool((opt.state == 0.75).all()) and bool((arena.grads == 0.5).all())
        assert bool((opt.workspace == 0).all())
