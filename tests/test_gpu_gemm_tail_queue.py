"""Split-K tail grids on the persistent tile queue (`gemm_bf16_nt_256p_kernel`): both item orders (option 12: K-slices behind or in
front of a queue's whole tiles) against the one-tile-per-block kernel, both with the fix-up launch, on the same operands and the
same workspace.  (The reduce inside the queue launch that the issue staged as part B measured slower and is not in the tree.)  No tolerances: every item keeps its
tile, its K range and its slab, the slabs are added in slice order and the epilogue is epilogue4<true> on both sides, so every output
has the same bits (`torch.equal`).  Each case is launched twice back to back: the second launch finds whatever the first left in the
queue counters.  The reference and the queue kernel share the stream's workspace and write the same slabs, so the slab
area (everything but the last 4 KiB) is filled with NaN in front of EVERY queue-kernel launch: a slab that is not written, written to
another place turns outputs into NaN instead of finding the right bits left over.  Every case asserts through the library's own plan (`desta_gemm_plan_query`) that the queue kernel and
the expected split were taken, and the reference that the one-tile-per-block kernel and the fix-up launch were: a case that falls back
to another path fails.

Grids: the smallest with a tail behind one full round.  272 tiles (tail 16) at K = 1024 / 2048 / 4096, i.e. split 2 / 4 / 8 with
option 14's floor of 8 K-tiles per slice; 320 tiles (tail 64, four tail tiles per M-group column);
M = 4300 (clamped last rows, a last M-group of one tile row); N = 4000 (a partial column tile).  Operands: real-valued (normal; a
wrong slice order changes bits) and dyadic (every sum exact)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, N, K) -> split under option 14 = 1 (tail tiles rem = T - 256; split = min(256 // rem, 8, (K / 64) // 8))
SHAPES = {(4352, 4096, 1024): 2, (4352, 4096, 2048): 4, (4352, 4096, 4096): 8, (5120, 4096, 1024): 2, (5120, 4096, 2048): 4,
          (4300, 4096, 2048): 4, (4352, 4000, 2048): 4}
EPILOGUES = ["plain", "residual", "bias", "bias_gelu", "rotary", "f32_stream", "preact"]
KINDS = ["real", "dyadic"]
SENTINEL = 3.0


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from desta import _hip
    yield _hip
    _operands.clear()                                                       # (device memory of the shared operands and references)
    _reference.clear()


_operands, _reference = {}, {}
DEFAULTS = {0: 1, 5: 0, 12: 0, 14: 0}                                # desta_gemm_set_option defaults of the options the cases move


def _ops(shape, kind):
    """device operands of a shape, made once"""
    if (shape, kind) not in _operands:
        M, N, K = shape
        g = torch.Generator(device="cuda").manual_seed(M + N + K + len(kind))
        if kind == "real":
            def rnd(*s, scale=1.0):
                return torch.randn(*s, generator=g, device="cuda") * scale
            o = dict(A=rnd(M, K), B=rnd(N, K, scale=1 / 16), bias=rnd(N), res=rnd(M, N), res32=rnd(M, N))
        else:                                                               # integers / 2^s: K * 4 * 4 < 2^24, every partial sum exact
            def rnd(*s, scale=1.0):
                return torch.randint(-4, 5, s, generator=g, device="cuda").float() * scale
            o = dict(A=rnd(M, K), B=rnd(N, K, scale=1 / 16), bias=rnd(N, scale=1 / 4), res=rnd(M, N, scale=1 / 2), res32=rnd(M, N, scale=1 / 8))
        for n in ("A", "B", "res"):
            o[n] = o[n].to(torch.bfloat16)
        o["pos"] = torch.randint(0, 512, (M,), generator=g, device="cuda", dtype=torch.int32)
        o["cs"] = torch.randn(512, 64, 2, generator=g, device="cuda")
        _operands[(shape, kind)] = o
    return _operands[(shape, kind)]


def _launch(hip, shape, o, epi):
    """one call into sentinel-filled outputs -> tuple of outputs"""
    M, N, K = shape
    out = torch.full((M, N), SENTINEL, dtype=torch.float32 if epi == "f32_stream" else torch.bfloat16, device="cuda")
    kw, extra = {}, ()
    if epi == "residual":
        kw = dict(residual=o["res"])
    elif epi == "bias":
        kw = dict(bias=o["bias"])
    elif epi == "bias_gelu":
        kw = dict(bias=o["bias"], act=1)
    elif epi == "rotary":
        kw = dict(rope=(o["cs"], o["pos"], N - N % 128, 128))
    elif epi == "f32_stream":
        kw = dict(bias=o["bias"], residual=o["res32"])
    elif epi == "preact":
        pre = torch.full((M, N), SENTINEL, dtype=torch.bfloat16, device="cuda")
        kw, extra = dict(preact=pre), (pre,)
    hip.gemm(o["A"], o["B"], out, M, N, K, alpha=0.75, **kw)
    return (out,) + extra


def _with(hip, variant, opts, fn):
    try:
        hip.gemm_force_variant(variant)
        for k, v in opts.items():
            hip.gemm_set_option(k, v)
        return fn()
    finally:
        hip.gemm_force_variant(0)
        for k, v in DEFAULTS.items():
            hip.gemm_set_option(k, v)


def _ref(hip, shape, kind, epi):
    """the one-tile-per-block kernel (variant 6) + the fix-up launch at the same split, computed once per (shape, operands, epilogue)"""
    key = (shape, kind, epi)
    if key not in _reference:
        def run():
            out = _launch(hip, shape, _ops(shape, kind), epi)
            pl = hip.gemm_plan()
            assert (pl["kernel"], pl["split"], pl["fixup_launch"], pl["inkernel"]) == ("256", SHAPES[shape], 1, 0), pl
            torch.cuda.synchronize()
            return out
        _reference[key] = _with(hip, 6, {5: 0, 14: 1}, run)
    return _reference[key]


@pytest.mark.parametrize("order", [0, 1], ids=["whole_first", "slices_first"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("shape", list(SHAPES), ids=["x".join(map(str, s)) for s in SHAPES])
def test_tail_queue_equals_one_tile_per_block(hip, shape, epi, kind, order):
    M, N, K = shape
    split, rem = SHAPES[shape], ((M + 255) // 256) * ((N + 255) // 256) - 256
    ref = _ref(hip, shape, kind, epi)
    ws = hip._workspace(torch.device("cuda", torch.cuda.current_device()), hip.stream())
    counters = ws[-1024:].view(torch.int32)                                 # option 5's tickets (first 1 KiB) and the queue counters (last 64 B)

    def run():
        outs = []
        for _ in range(2):                                                  # back to back: the second launch runs on the first's counters
            ws[:-1024].fill_(float("nan"))                                  # no slab of an earlier launch survives
            outs.append(_launch(hip, shape, _ops(shape, kind), epi))
            pl = hip.gemm_plan()
            assert pl == dict(kernel="256p", split=split, full_tiles=256, items=256 + rem * split, slices_first=order,
                              inkernel=0, fixup_launch=1), pl
        torch.cuda.synchronize()
        return outs

    outs = _with(hip, 4, {5: 0, 12: order, 14: 1}, run)
    assert not bool(counters.any()), "queue counters not reset"
    for out in outs:
        assert len(out) == len(ref)
        for x, y in zip(out, ref):
            assert torch.equal(x, y)


def test_default_choice_takes_the_queue_for_the_step_shapes(hip):
    """No forced variant, default options: the o_proj shape of the step goes through the queue kernel with its split-K tail and gives
    the bits of option 0 = 0 (one tile per block, same split)."""
    shape = (5120, 4096, 4096)
    M, N, K = shape
    g = torch.Generator(device="cuda").manual_seed(11)
    o = dict(A=torch.randn(M, K, generator=g, device="cuda").to(torch.bfloat16), B=(torch.randn(N, K, generator=g, device="cuda") / 16).to(torch.bfloat16),
             res=torch.randn(M, N, generator=g, device="cuda").to(torch.bfloat16))

    def run(kernel):
        out = _launch(hip, shape, o, "residual")
        pl = hip.gemm_plan()
        assert (pl["kernel"], pl["split"], pl["fixup_launch"]) == (kernel, 4, 1), pl
        torch.cuda.synchronize()
        return out

    ws = hip._workspace(torch.device("cuda", torch.cuda.current_device()), hip.stream())

    def fresh(kernel):
        ws[:-1024].fill_(float("nan"))
        return run(kernel)

    new = [fresh("256p"), fresh("256p")]
    ref = _with(hip, 0, {0: 0}, lambda: run("256"))
    for out in new:
        assert torch.equal(out[0], ref[0])
