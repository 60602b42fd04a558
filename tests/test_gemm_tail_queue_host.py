"""CPU-only: the tile choice of desta_gemm_bf16_nt (`desta_gemm_plan_query`, host arithmetic in the library) for the GEMM shapes of
the headline training step at batch 8: which kernel, how many K-slices per tail tile, how many work items."""
from desta import _hip as H

# (M, N, K, act) -> (kernel, split, full tiles, items).  256 CUs, 256x256 tiles, T = tiles; a tail of rem = T % 256 <= 128 tiles is
# cut into split = min(256 // rem, 8, (K / 64) // 16) K-slices when that is >= 2; the tile queue takes every grid with T > 256.
LLM = {
    (5120, 28672, 4096, 2): ("256p", 1, 2240, 2240),     # gate|up + SwiGLU: never split
    (4608, 4096, 28672, 0): ("256p", 8, 256, 512),       # d(down): 288 tiles, tail 32
    (4608, 14336, 4096, 3): ("256p", 1, 1008, 1008),     # d(act) + SwiGLU backward
    (5120, 4096, 14336, 0): ("256p", 4, 256, 512),       # down + residual: 320 tiles, tail 64
    (5120, 6144, 4096, 0): ("256p", 1, 480, 480),        # q|k|v + rotary: tail 224 > 128, no split
    (4608, 4096, 6144, 0): ("256p", 6, 256, 448),        # d(q|k|v): 96 K-tiles / 16
    (5120, 4096, 4096, 0): ("256p", 4, 256, 512),        # o_proj + residual
    (4608, 4096, 4096, 0): ("256p", 4, 256, 384),        # d(o_proj): 64 K-tiles / 16
    (4096, 128256, 4096, 0): ("256p", 3, 7936, 8176),    # lm_head: 8016 tiles, tail 80
}
WHISPER = {
    (12000, 5120, 1280, 1): ("256p", 1, 940, 940),       # fc1 + GELU: tail 172 > 128
    (12000, 1280, 5120, 0): ("256", 1, 235, 235),        # fc2: one round
    (12000, 3840, 1280, 0): ("256p", 1, 705, 705),       # q|k|v
    (12000, 1280, 1280, 0): ("256", 1, 235, 235),        # out-proj
}


def _plan(M, N, K, act):
    p = H.gemm_plan(M, N, K, act=act)
    return p["kernel"], p["split"], p["full_tiles"], p["items"]


def test_plan_of_the_step_shapes():
    for (M, N, K, act), want in {**LLM, **WHISPER}.items():
        assert _plan(M, N, K, act) == want, (M, N, K, act)
        p = H.gemm_plan(M, N, K, act=act)
        assert p["fixup_launch"] == (p["split"] > 1) and not p["slices_first"] and not p["inkernel"], p


def test_plan_options():
    try:
        H.gemm_set_option(14, 1)                                    # >= 8 K-tiles per slice: the 288-tile grids fill their tail round
        assert _plan(4608, 4096, 4096, 0) == ("256p", 8, 256, 512) and _plan(4608, 4096, 6144, 0) == ("256p", 8, 256, 512)
        assert _plan(5120, 4096, 4096, 0) == ("256p", 4, 256, 512)
        H.gemm_set_option(0, 0)                                     # the same split on the one-tile-per-block kernel: the floor goes by what the grid CAN take
        p = H.gemm_plan(4608, 4096, 4096)
        assert (p["kernel"], p["split"], p["items"], p["fixup_launch"]) == ("256", 8, 512, 1), p
    finally:
        for k, v in {0: 1, 14: 0}.items():
            H.gemm_set_option(k, v)
    assert H.gemm_plan(4608, 4096, 4096, workspace=False)["split"] == 1          # no workspace: no slices, no queue
    assert H.gemm_plan(5120, 4096, 4096, batch=2)["kernel"] == "256"                     # a batch: one tile per block, no slices
