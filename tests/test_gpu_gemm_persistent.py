"""The persistent tile-queue form of the 256x256 GEMM (`gemm_bf16_nt_256p_kernel`) against the one-tile-per-block kernel of the
same call: every epilogue instance, split-K tails, the self-resetting queue counters, and a run beside a concurrent load.  No
tolerances: each item is computed by one block in the same K order with the same epilogue arithmetic, so every output is
bit-identical (`torch.equal`).  Option 0 of desta_gemm_set_option: 0 = never persistent, 2 = persistent for every multi-round grid.
Both kernels run the same epilogue code: what that code computes is checked against float64 in tests/test_gpu_gemm_fp64.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

REPEATS = 3                                   # a schedule race would show up as differing bits between repeats


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    from desta import _hip
    return _hip


def _bf(x):
    return x.to(torch.bfloat16)


def _run(hip, persistent, fn):
    """fn() -> tuple of output tensors; runs it REPEATS times under option 0 = persistent and checks the repeats agree."""
    hip.gemm_set_option(0, persistent)
    try:
        outs = [tuple(o.clone() for o in fn()) for _ in range(REPEATS)]
    finally:
        hip.gemm_set_option(0, 1)
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert torch.equal(x, y)
    return outs[0]


def _check(hip, fn, expect_kernel=2):
    ref = _run(hip, 0, fn)
    new = _run(hip, 2, fn)
    assert hip.lib.desta_gemm_last_kernel() == expect_kernel
    for x, y in zip(ref, new):
        assert torch.equal(x, y)


# (M, N, K): 17 x 27 = 459 tiles (459 % 8 = 3: unequal queues, ragged M and N) and 16 x 32 = 512 tiles (every queue equal)
SHAPES = [(4100, 6880, 512), (4096, 8192, 512)]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("mode", ["plain", "residual", "bias", "bias_gelu", "preact", "rope", "f32_stream", "dropout", "f32_out"])
def test_persistent_epilogue_instances(hip, M, N, K, mode):
    g = torch.Generator().manual_seed(M + N + K + len(mode))
    A = _bf(torch.randn(M, K, generator=g)).cuda()
    B = _bf(torch.randn(N, K, generator=g) / 16).cuda()
    bias = torch.randn(N, generator=g).cuda()
    res = _bf(torch.randn(M, N, generator=g)).cuda()
    res32 = torch.randn(M, N, generator=g).cuda()
    pos = torch.randint(0, 4096, (M,), generator=g, dtype=torch.int32).cuda()
    cs = torch.randn(4096, 64, 2, generator=g).cuda()

    def fn():
        out = torch.full((M, N), 3.0, dtype=torch.float32 if mode in ("f32_stream", "f32_out") else torch.bfloat16, device="cuda")
        kw = {}
        extra = ()
        if mode == "residual":
            kw = dict(residual=res)
        elif mode == "bias":
            kw = dict(bias=bias)
        elif mode == "bias_gelu":
            kw = dict(bias=bias, act=1)
        elif mode == "preact":
            pre = torch.full((M, N), 3.0, dtype=torch.bfloat16, device="cuda")
            kw = dict(preact=pre)
            extra = (pre,)
        elif mode == "rope":
            kw = dict(rope=(cs, pos, N - N % 128 if N % 128 else N, 128))
        elif mode == "f32_stream":
            kw = dict(bias=bias, residual=res32)
        elif mode == "dropout":
            kw = dict(bias=bias, act=1, residual=res, dropout_p=0.1, dropout_seed=1234)
        hip.gemm(A, B, out, M, N, K, alpha=0.75, **kw)
        return (out,) + extra

    _check(hip, fn)


@pytest.mark.parametrize("M,I,K", [(4100, 3424, 512), (4096, 4096, 512)])
def test_persistent_swiglu_epilogues(hip, M, I, K):
    """act 2 (gate|up projection + SwiGLU into aux) and act 3 (d(act) GEMM + SwiGLU backward reading the saved gate|up from aux)."""
    g = torch.Generator().manual_seed(M + I)
    x = _bf(torch.randn(M, K, generator=g)).cuda()
    w = _bf(torch.randn(2 * I, K, generator=g) / 16).cuda()
    dy = _bf(torch.randn(M, K, generator=g)).cuda()
    wd = _bf(torch.randn(2 * I, K, generator=g) / 16).cuda()

    def fwd():
        gu = torch.full((M, 2 * I), 7.0, dtype=torch.bfloat16, device="cuda")
        act = torch.full((M, I), 7.0, dtype=torch.bfloat16, device="cuda")
        hip.gemm(x, w, gu, M, 2 * I, K, act=2, aux=act, ld_aux=I)
        return gu, act

    _check(hip, fwd)
    gu = fwd()[0]

    def bwd():
        dgu = torch.full((M, 4 * I), 7.0, dtype=torch.bfloat16, device="cuda")
        gu2 = torch.cat([gu, gu], 1).contiguous()                       # [M, 4I]: the saved gate|up of a 2I-wide activation
        hip.gemm(dy, wd, dgu, M, 2 * I, K, ldc=4 * I, act=3, aux=gu2, ld_aux=4 * I)
        return (dgu,)

    _check(hip, bwd)


@pytest.mark.parametrize("M,N,K", [(5120, 4096, 2048), (4608, 4352, 4096)])
def test_persistent_splitk_tail(hip, M, N, K):
    """Grids with a split-K tail (320 tiles: 64 tail tiles in 2 K-slices; 306 tiles: 50 in 4): the slices go into the queues after
    the whole tiles and the fix-up launch sums them, as with the one-tile-per-block kernel."""
    g = torch.Generator().manual_seed(M + N + K)
    A = _bf(torch.randn(M, K, generator=g)).cuda()
    B = _bf(torch.randn(N, K, generator=g) / 16).cuda()
    bias = torch.randn(N, generator=g).cuda()
    res = _bf(torch.randn(M, N, generator=g)).cuda()

    def fn():
        o32 = torch.empty(M, N, dtype=torch.float32, device="cuda")
        hip.gemm(A, B, o32, M, N, K)
        ob = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        hip.gemm(A, B, ob, M, N, K, bias=bias, residual=res)
        return o32, ob

    _check(hip, fn)


def test_persistent_counter_reset_and_streams(hip):
    """The queue counters reset themselves: back-to-back calls on one stream, then calls interleaved on two streams (each with its
    own workspace, hence its own counters), all give the bits of the non-persistent kernel."""
    M, N, K = 4100, 6880, 512
    g = torch.Generator().manual_seed(5)
    A = _bf(torch.randn(M, K, generator=g)).cuda()
    B = _bf(torch.randn(N, K, generator=g) / 16).cuda()
    A2 = _bf(torch.randn(M, K, generator=g)).cuda()
    ref = _run(hip, 0, lambda: (hip.gemm(A, B, torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), M, N, K),))[0]
    ref2 = _run(hip, 0, lambda: (hip.gemm(A2, B, torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), M, N, K),))[0]
    hip.gemm_set_option(0, 2)
    try:
        outs = [torch.empty(M, N, dtype=torch.bfloat16, device="cuda") for _ in range(REPEATS)]
        for o in outs:
            hip.gemm(A, B, o, M, N, K)
        torch.cuda.synchronize()
        for o in outs:
            assert torch.equal(o, ref)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        o1 = [torch.empty(M, N, dtype=torch.bfloat16, device="cuda") for _ in range(REPEATS)]
        o2 = [torch.empty(M, N, dtype=torch.bfloat16, device="cuda") for _ in range(REPEATS)]
        torch.cuda.synchronize()
        for i in range(REPEATS):
            with torch.cuda.stream(s1):
                hip.gemm(A, B, o1[i], M, N, K)
            with torch.cuda.stream(s2):
                hip.gemm(A2, B, o2[i], M, N, K)
        torch.cuda.synchronize()
    finally:
        hip.gemm_set_option(0, 1)
    for i in range(REPEATS):
        assert torch.equal(o1[i], ref)
        assert torch.equal(o2[i], ref2)


def test_persistent_beside_concurrent_load(hip):
    """One call while a long kernel occupies CUs from a second stream: blocks of the queue kernel start late or share a CU, and
    the tiles still come out exactly as from the non-persistent kernel."""
    M, N, K = 4096, 8192, 512
    g = torch.Generator().manual_seed(9)
    A = _bf(torch.randn(M, K, generator=g)).cuda()
    B = _bf(torch.randn(N, K, generator=g) / 16).cuda()
    ref = _run(hip, 0, lambda: (hip.gemm(A, B, torch.empty(M, N, dtype=torch.bfloat16, device="cuda"), M, N, K),))[0]
    X = torch.randn(8192, 8192, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    hip.gemm_set_option(0, 2)
    try:
        outs = []
        for _ in range(REPEATS):
            with torch.cuda.stream(side):
                Y = X @ X                                              # fp32 matmul: tens of ms on the side stream
            o = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
            hip.gemm(A, B, o, M, N, K)
            outs.append(o)
        torch.cuda.synchronize()
        del Y
    finally:
        hip.gemm_set_option(0, 1)
    for o in outs:
        assert torch.equal(o, ref)
