"""GPU: the chunked, memory-lean prompt pass of generate() (`set_prefill_chunk`, `CausalLMHIP.prefill`) and the kernel that hands a
chunk's attention the FP8 cache as bf16 (desta_kv8_dequant).

Kernel: bit for bit against the host rule (tests/test_gpu_fp8_decode.py::dequant_bf16) on [kv_start, slot1), a sentinel everywhere
else, NaN scales and NaN bytes outside the visible range without effect, an output slab with strides of its own; rejections.
Attention: the forward kernel in exactly the configuration `prefill` uses (Q rows of a [B * Cc, qkvw] buffer, K | V the halves of a
[B, Smax, kvw] slab, causal with cached keys in front, left pads), held per element to fp64 by the criterion of
tests/test_gpu_attention_fp64.py (tests/attention_reference.py).
Model (tiny Qwen3 geometry, G = 2 and G = 4, B = 3 with left pads 0 / 5 / 131, forced tokens from the fp32 oracle):
  * one chunk (chunk size >= prompt) gives the bits of the unchunked pass: every step's logits and every layer's cache slab; under
    the FP8 cache layer 0's prompt bytes and scales (the logits, and the cache from layer 1 on, cannot agree: the chunk attends
    dequantised keys, the unchunked pass the bf16 projection);
  * prompts of 251 = 128 + 123 and 300 = 128 + 128 + 44 positions at chunk 128 (the row with pad 131 has an all-padding first
    chunk) and 61 = 16 + 16 + 16 + 13 at chunk 16, bf16 and FP8 caches, against the oracle within the decode path's own bounds
    (tests/test_gpu_decode_attention.py: rel-L2 3e-2, gap / spread 0.1; FP8: REL_BOUND / GAP_BOUND of tests/test_gpu_kv8_cache.py),
    and, per cache kind, the chunked run's worst rel-L2 at most 1.5 x the unchunked run's on the same inputs (the rule of
    tests/test_gpu_decode_attention.py::test_agreement_with_the_forward_kernel); two chunked runs give the same bits;
  * the peak memory of a `_generate_step` grows from a 251- to a 507-position prompt by no more than what scales with the prompt
    by design (cache, scales, staging slab, the embedding buffer, the cos / sin table, the integer inputs) plus 1 MiB;
  * ORCA injection per chunk (audio K|V projected on the first chunk only) against the ORCA oracle;
  * launch counts: L x chunks dequantisations under the FP8 cache, none under bf16; the decode counters move by the decode steps only.

Measured (MI355X; profiles/r13_prefill_tests.log), worst per-step logits rel-L2 against the fp32 oracle over T = 12 steps,
unchunked -> chunked (ratio; gap / spread of the chunked run):
    G  S    C    bf16 cache                          FP8 cache
    2  251  128  5.685e-3 -> 5.597e-3 (0.984; 0.000)   7.296e-3 -> 7.404e-3 (1.015; 0.000)
    2  300  128  5.896e-3 -> 5.830e-3 (0.989; 0.000)   6.963e-3 -> 7.055e-3 (1.013; 0.000)
    2  61   16   5.706e-3 -> 5.706e-3 (1.000; 0.000)   9.601e-3 -> 9.992e-3 (1.041; 0.015)
    4  251  128  6.023e-3 -> 5.857e-3 (0.973; 0.000)   7.684e-3 -> 7.985e-3 (1.039; 0.000)
    4  300  128  5.720e-3 -> 5.898e-3 (1.031; 0.000)   7.115e-3 -> 7.398e-3 (1.040; 0.016)
    4  61   16   5.928e-3 -> 5.928e-3 (1.000; 0.000)   1.014e-2 -> 1.074e-2 (1.058; 0.035)
The FP8 chunked worst, 1.074e-2, is below 2e-2: the decode path's own bounds (REL_BOUND = 3e-2, GAP_BOUND = 0.1) hold unchanged, and
every ratio is far inside 1.5.  ORCA, three chunks: 6.75e-3 (gap / spread 0.011) bf16 cache, 8.16e-3 (0.023) FP8 cache.
Chunk attention against fp64, worst |err| / bound (the emulation's ratio): 0.642 (0.642) 128 x 256, 0.511 (0.511) 128 x 300,
0.672 (0.672) 123 x 251, 0.313 (0.313) 1 x 257, 0.387 (0.387) 44 x 300, 0.761 (0.761) 128 x 128; |lse - fp64| / (1 + |fp64|) <= 1.5e-7.
Peak memory of a _generate_step, chunk 128, S = 251 -> 507: +1 747 456 B (bf16 cache; allowed 3 171 072, of which cache 1 572 864) and
+1 772 032 B (FP8; allowed 3 195 648); per-layer buffers alone would add 11 796 480 B.  One chunk under the FP8 cache: layer 1's
prompt bytes agree with the unchunked run's in 81-84 % of the positions.
"""
import copy
import os

import pytest
import torch

import attention_reference as R
import desta_oracle as O
from helpers import cfg_from_dims, rel_err  # noqa: F401
from test_gpu_decode_attention import _check_against_oracle  # noqa: F401  (the decode path's bounds: 3e-2, 0.1)
from test_gpu_kv8_cache import GAP_BOUND, HD, REL_BOUND, _dims, _errors, _gen, _text_inputs, pow2_spread, quantize_slab

pytestmark = pytest.mark.gpu

BF16_REL_BOUND, BF16_GAP_BOUND = 3e-2, 0.1                                   # tests/test_gpu_decode_attention.py::_check_against_oracle
SENTINEL = 7.0


@pytest.fixture(scope="module")
def hip():
    assert torch.cuda.is_available()
    from desta import _hip
    return _hip


# ---------------------------------------------------------------------------------------------------------------- 1
_SLABS = {}


def _slab(Hkv):
    """(bytes, scales, dequantised bf16) of a [3, 300, 2 Hkv 128] cache with per-head power-of-two factors, made once."""
    if Hkv not in _SLABS:
        g = torch.Generator().manual_seed(40 + Hkv)
        cache = pow2_spread(torch.randn(3, 300, 2 * Hkv * HD, generator=g).bfloat16(), seed=Hkv)
        _SLABS[Hkv] = quantize_slab(cache)
    return _SLABS[Hkv]


KV_START = [0, 5, 131]


def _dequant(hip, by, sc, kv, slot1, out, n_heads, out_bs=None, out_rs=None):
    hip.kv8_dequant(by, by.stride(0), by.stride(1), sc, sc.stride(0), sc.stride(1), kv, by.shape[0], n_heads, HD, slot1, out,
                    out.stride(0) if out_bs is None else out_bs, out.stride(1) if out_rs is None else out_rs)
    torch.cuda.synchronize()


@pytest.mark.parametrize("slot1", [1, 131, 132, 300])
@pytest.mark.parametrize("Hkv", [1, 2])
def test_dequant_is_exact(hip, Hkv, slot1):
    by, sc, deq = _slab(Hkv)
    B, Smax, kvw = by.shape
    kv = torch.tensor(KV_START, dtype=torch.int32)
    want = torch.full((B, Smax, kvw), SENTINEL, dtype=torch.bfloat16)
    for b, k0 in enumerate(KV_START):
        want[b, min(k0, slot1):slot1] = deq[b, min(k0, slot1):slot1]
    n0 = hip.KV8_DEQUANT_CALLS
    out = torch.full((B, Smax, kvw), SENTINEL, dtype=torch.bfloat16, device="cuda")
    _dequant(hip, by.cuda(), sc.cuda(), kv.cuda(), slot1, out, 2 * Hkv)
    assert hip.KV8_DEQUANT_CALLS == n0 + 1
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    # nothing outside [kv_start, slot1) is read: NaN scales and NaN bytes there, the same bits
    by2, sc2 = by.clone(), sc.clone()
    by2[:, slot1:], sc2[:, slot1:] = 0x7F, float("nan")
    for b, k0 in enumerate(KV_START):
        by2[b, :min(k0, slot1)], sc2[b, :min(k0, slot1)] = 0x7F, float("nan")
    out2 = torch.full((B, Smax, kvw), SENTINEL, dtype=torch.bfloat16, device="cuda")
    _dequant(hip, by2.cuda(), sc2.cuda(), kv.cuda(), slot1, out2, 2 * Hkv)
    assert torch.equal(out2.cpu().view(torch.int16), want.view(torch.int16))
    # an output slab with strides of its own (more slots, wider rows): the pad columns and rows keep the sentinel
    big = torch.full((B, Smax + 7, kvw + 64), SENTINEL, dtype=torch.bfloat16, device="cuda")
    _dequant(hip, by.cuda(), sc.cuda(), kv.cuda(), slot1, big, 2 * Hkv)
    big = big.cpu()
    assert torch.equal(big[:, :Smax, :kvw].contiguous().view(torch.int16), want.view(torch.int16))
    assert bool((big[:, Smax:] == SENTINEL).all()) and bool((big[:, :, kvw:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- 2
def test_dequant_rejections(hip):
    by, sc, _ = _slab(2)
    B, Smax, kvw = by.shape
    by, sc, kv = by.cuda(), sc.cuda(), torch.tensor(KV_START, dtype=torch.int32).cuda()
    out = torch.full((B, Smax, kvw), SENTINEL, dtype=torch.bfloat16, device="cuda")
    wide8 = torch.zeros(B, Smax, kvw + 8, dtype=torch.uint8, device="cuda")                 # a byte row stride that is no multiple of 16
    wide4 = torch.full((B, Smax, kvw + 4), SENTINEL, dtype=torch.bfloat16, device="cuda")   # an output row stride that is no multiple of 8
    ok = dict(cache=by, kv_bs=by.stride(0), kv_rs=by.stride(1), scale=sc, scale_bs=sc.stride(0), scale_rs=sc.stride(1), kv_start=kv, batch=B,
              n_heads=4, hd=HD, slot1=200, out=out, out_bs=out.stride(0), out_rs=out.stride(1))
    bad = [("head_dim", dict(hd=64)), ("batch", dict(batch=0)), ("batch", dict(batch=-2)), ("n_heads", dict(n_heads=0)), ("slot1", dict(slot1=0)),
           ("slot1", dict(slot1=-5)), ("null", dict(cache=None)), ("null", dict(scale=None)), ("null", dict(out=None)),
           ("cache must be 16-byte aligned", dict(cache=by.view(-1)[1:])), ("cache must be 16-byte aligned", dict(cache=wide8, kv_bs=wide8.stride(0), kv_rs=wide8.stride(1))),
           ("cache must be 16-byte aligned", dict(kv_rs=kvw - 16)),                          # a row narrower than the heads
           ("scale stride", dict(scale_rs=3)),
           ("output must be 16-byte aligned", dict(out=out.view(-1)[1:])), ("output must be 16-byte aligned", dict(out=wide4, out_bs=wide4.stride(0), out_rs=wide4.stride(1))),
           ("output must be 16-byte aligned", dict(out_rs=kvw - 8))]
    n0 = hip.KV8_DEQUANT_CALLS
    for name, change in bad:
        with pytest.raises(RuntimeError, match=name) as ei:
            hip.kv8_dequant(**{**ok, **change})
        assert "(-1)" in str(ei.value), name                                # DESTA_EINVAL
    torch.cuda.synchronize()
    assert hip.KV8_DEQUANT_CALLS == n0
    assert bool((out == SENTINEL).all()) and bool((wide4 == SENTINEL).all())  # nothing was launched
    hip.kv8_dequant(**ok)
    torch.cuda.synchronize()
    assert hip.KV8_DEQUANT_CALLS == n0 + 1 and bool((out[0, :200] != SENTINEL).any()) and bool((out[:, 200:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- 3
CHUNK_ATTN_CASES = [(4, 2, 128, 256), (8, 2, 128, 300), (4, 2, 123, 251), (4, 2, 1, 257), (8, 2, 44, 300),
                    (4, 2, 128, 128)]                                        # (and the first chunk itself: the padded row sees no key at all)


@pytest.mark.parametrize("Hq,Hkv,Cc,c1", CHUNK_ATTN_CASES)
def test_chunk_attention_vs_fp64(hip, Hq, Hkv, Cc, c1):
    """The chunk's queries sit at slots [c1 - Cc, c1) of the slab; key j is visible to query i iff pad <= j <= i + (c1 - Cc).
    Criterion of tests/test_gpu_attention_fp64.py: worst |O - fp64| / bound <= min(2, 2 x the conforming emulation's ratio), exactly 0
    where no key is visible, |lse - fp64| <= 1e-4 (1 + |fp64|), +inf on rows without a key."""
    B, pads = 2, [0, 131]
    Smax, qkvw, kvw = c1 + 9, (Hq + 2 * Hkv) * HD, 2 * Hkv * HD
    g = torch.Generator().manual_seed(Hq * 1000 + Cc * 7 + c1)
    qbuf = torch.randn(B * Cc, qkvw, generator=g).bfloat16()
    slab = torch.randn(B, Smax, kvw, generator=g).bfloat16()
    kv = torch.tensor(pads, dtype=torch.int32)
    q = qbuf[:, :Hq * HD].reshape(B, Cc, Hq, HD)
    k, v = slab[:, :c1, :Hkv * HD].reshape(B, c1, Hkv, HD), slab[:, :c1, Hkv * HD:].reshape(B, c1, Hkv, HD)
    a = (q, k, v, torch.zeros_like(q), HD ** -0.5, True, kv)
    ref = R.exact(*a)
    fwd8 = Cc >= 128                                                         # desta_attention_fwd: the 8-wave kernel from 128 query rows on
    emu_ratio = R.worst_ratio(ref, "O", R.emulate(*a, fwd8=fwd8)["O"])
    o = torch.full((B * Cc, Hq * HD), SENTINEL, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, Hq, Cc), SENTINEL, device="cuda")
    qd, sd = qbuf.cuda(), slab.cuda()
    d = hip.attn_desc(qd, sd, sd, o, lse, batch=B, hq=Hq, hkv=Hkv, sq=Cc, sk=c1, hd=HD, scale=HD ** -0.5, causal=True, kv_start=kv.cuda(),
                      q_off=0, k_off=0, v_off=Hkv * HD, q_rs=qkvw, k_rs=kvw, v_rs=kvw, o_rs=Hq * HD, k_bs=Smax * kvw, v_bs=Smax * kvw)
    hip.attention_fwd(d)
    torch.cuda.synchronize()
    got, lse = o.cpu().view(B, Cc, Hq, HD), lse.cpu()
    ratio = R.worst_ratio(ref, "O", got.double())
    live = ref["live"]
    lse_err = float(((lse.double() - ref["lse"])[live].abs() / (1 + ref["lse"][live].abs())).max())
    dead_rows = int((~live[1, 0]).sum())
    print(f"CHUNK_ATTN Hq {Hq} Hkv {Hkv} Cc {Cc} c1 {c1} fwd{8 if fwd8 else 4}: O {ratio:.3f} ({emu_ratio:.3f}) lse {lse_err:.1e} "
          f"rows of the padded sequence without a key {dead_rows}")
    assert dead_rows == min(Cc, max(0, 131 - (c1 - Cc))) and bool(live[0].all())
    assert ratio <= min(2.0, 2.0 * emu_ratio), (ratio, emu_ratio)
    assert lse_err <= 1e-4
    assert bool(torch.isinf(lse[~live]).all()) and bool((lse[~live] > 0).all())
    assert bool((got[1, :dead_rows] == 0).all())                            # rows that lie wholly in the padding


# ---------------------------------------------------------------------------------------------------------------- 4 .. 8
_MODELS, _ORACLE = {}, {}
PADS = {251: [0, 5, 131], 300: [0, 5, 131], 61: [0, 5, 19]}


def _model(g4):
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    if g4 not in _MODELS:
        d = _dims(g4)
        w = O.init_weights(d, seed=7)
        _MODELS[g4] = (d, w, DeSTA25AudioModel(cfg_from_dims(d), weights=w))
    return _MODELS[g4]


def _oracle(g4, S, T):
    """(inputs, forced ids, fp32 logits [T, B, V]) of the oracle's greedy run on the prompt of length S: computed once."""
    key = (g4, S, T)
    if key not in _ORACLE:
        d, w, _ = _model(g4)
        ids, am, inputs = _text_inputs(d, S, PADS[S], seed=S)
        with torch.no_grad():
            ref, lo = O.greedy_generate(w, d, O.embed_splice(w, d, ids, None, [], []), am, T, 0)
        _ORACLE[key] = (inputs, ref, lo)
    return _ORACLE[key]


def _poison_free_memory():
    """NaN patterns into memory the allocator will hand out next (small and large pool): a buffer that the pass reads before it
    writes shows as NaN logits instead of passing on fresh, zeroed memory."""
    junk = [torch.full((256 << 10,), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(16)]
    junk.append(torch.full((16 << 20,), float("nan"), dtype=torch.bfloat16, device="cuda"))
    torch.cuda.synchronize()
    del junk


def _slabs(llm, pads, n):
    """Every layer's cache (and scales) over [kv_start, n) of each row, on the CPU."""
    out = []
    for li in range(len(llm.kv_cache)):
        for b, k0 in enumerate(pads):
            out.append(llm.kv_cache[li][b, k0:n].cpu())
            if llm.kv_scale is not None:
                out.append(llm.kv_scale[li][b, k0:n].cpu())
    return out


@pytest.mark.parametrize("g4", [False, True])
def test_one_chunk_equals_the_unchunked_pass_bit_for_bit(g4):
    d, w, model = _model(g4)
    S, T = 251, 6
    inputs, ref, _ = _oracle(g4, S, T)
    llm = model.llm
    try:
        model.set_kv_cache("bf16")
        model.set_prefill_chunk(None)
        out0, lg0 = _gen(model, inputs, T, ref)
        slabs0 = _slabs(llm, PADS[S], S + T - 1)
        assert getattr(llm, "_pf", None) is None
        model.set_prefill_chunk(256)                                         # >= the prompt: one chunk, the lean pass without chunking
        out1, lg1 = _gen(model, inputs, T, ref)
        assert llm._pf is not None and llm._pf["key"] == (3, S, S)
        assert torch.equal(out0, out1)
        for t in range(T):
            assert torch.equal(lg0[t], lg1[t]), t
        for a, b in zip(slabs0, _slabs(llm, PADS[S], S + T - 1)):
            assert a.dtype == torch.bfloat16 and torch.equal(a.view(torch.int16), b.view(torch.int16))
        # FP8 cache, one chunk.  Layer 0's append sees the unchunked run's input, so its bytes and scales are that run's, bit for
        # bit.  From layer 1 on they cannot be: by the FP8 rule the chunk's attention reads dequantised keys where the unchunked
        # pass reads the bf16 projection, so the layer's input, and with it the K | V it appends, differ (recorded, not asserted;
        # the runs are held to the oracle in test_chunked_vs_oracle).
        model.set_kv_cache("fp8")
        model.set_prefill_chunk(None)
        _gen(model, inputs, T, ref)
        q0 = _slabs(llm, PADS[S], S)
        model.set_prefill_chunk(256)
        _gen(model, inputs, T, ref)
        q1 = _slabs(llm, PADS[S], S)
        assert len(q0) == len(q1) == 2 * 3 * d.llm_layers and q0[0].dtype == torch.uint8 and q0[1].dtype == torch.float32
        per_layer = 2 * 3
        for a, b in zip(q0[:per_layer], q1[:per_layer]):
            assert torch.equal(a, b)
        for li in range(1, d.llm_layers):
            same = [float((a == b).float().mean()) for a, b in zip(q0[li * per_layer:(li + 1) * per_layer:2], q1[li * per_layer:(li + 1) * per_layer:2])]
            print(f"PREFILL_CHUNK one chunk, FP8 cache, layer {li}: fraction of prompt bytes equal to the unchunked run's, per row {[round(x, 4) for x in same]}")
            assert min(same) > 0.5                                           # the same keys to e4m3 rounding, not other data
        # back to None: the first run's bits
        model.set_kv_cache("bf16")
        model.set_prefill_chunk(None)
        assert llm._pf is None and llm.kv_stage is None
        out2, lg2 = _gen(model, inputs, T, ref)
        assert torch.equal(out0, out2) and torch.equal(lg0, lg2)
    finally:
        model.set_kv_cache("bf16")
        model.set_prefill_chunk(None)


@pytest.mark.parametrize("S,C", [(251, 128), (300, 128), (61, 16)])
@pytest.mark.parametrize("g4", [False, True])
def test_chunked_vs_oracle(g4, S, C):
    """See the module docstring for the measured numbers."""
    from desta.models.modeling_desta25 import prefill_chunks
    d, w, model = _model(g4)
    T = 12
    inputs, ref, lo = _oracle(g4, S, T)
    assert len(prefill_chunks(S, C)) == {251: 2, 300: 3, 61: 4}[S] and PADS[S][2] > C       # the last row's first chunk is all padding
    try:
        for kind, rel_bound, gap_bound in (("bf16", BF16_REL_BOUND, BF16_GAP_BOUND), ("fp8", REL_BOUND, GAP_BOUND)):
            model.set_kv_cache(kind)
            model.set_prefill_chunk(None)
            out_u, lg_u = _gen(model, inputs, T, ref)                        # the unchunked pass on the same inputs
            model.set_prefill_chunk(C)
            _poison_free_memory()                                            # the chunk buffers and the staging slab are made by the next run
            out_c, lg_c = _gen(model, inputs, T, ref)
            assert bool(torch.isfinite(lg_c.float()).all())
            out_c2, lg_c2 = _gen(model, inputs, T, ref)
            e_u, g_u = _errors(lg_u, lo, T)
            e_c, g_c = _errors(lg_c, lo, T)
            agree = float((lg_c.float().argmax(-1).cpu() == lo.argmax(-1)).float().mean())
            print(f"PREFILL_CHUNK G {d.llm_hq // d.llm_hkv} S {S} C {C} {kind} cache: worst per-step logits rel-L2 vs fp32 oracle  "
                  f"unchunked {e_u:.3e} (gap/spread {g_u:.3f})  chunked {e_c:.3e} (gap/spread {g_c:.3f})  ratio {e_c / e_u:.3f}  "
                  f"argmax agreement with the oracle {agree:.3f}")
            assert out_c.cpu().tolist() == ref.tolist() and lg_c.shape == lo.shape
            assert e_c < rel_bound and g_c < gap_bound, (kind, e_c, g_c)
            assert e_c <= 1.5 * e_u, (kind, e_c, e_u)
            assert torch.equal(out_c, out_c2) and torch.equal(lg_c, lg_c2)   # two chunked runs: the same bits
    finally:
        model.set_kv_cache("bf16")
        model.set_prefill_chunk(None)


def _drop_generation_buffers(llm):
    llm._pf = llm.kv_cache = llm.kv_scale = llm.kv_scale_v = llm.kv_stage = None
    llm._gen_shape = None
    for name in [n for n in vars(llm) if n.startswith("g_")] + ["gen_cos_sin"]:
        setattr(llm, name, None)


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_peak_memory_does_not_follow_the_prompt_or_the_save_set(kind):
    from desta.models.modeling_desta25 import DeSTA25AudioModel
    d = _dims(True)
    model = DeSTA25AudioModel(cfg_from_dims(d), weights=O.init_weights(d, seed=7))          # fresh: no training forward ran
    llm = model.llm
    model.set_kv_cache(kind)
    model.set_prefill_chunk(128)
    B, T, C = 3, 4, 128
    _gen(model, _text_inputs(d, 140, [0, 5, 131], seed=1)[2], T)             # warm-up: the library's own workspaces exist from here on
    peaks = {}
    for S in (251, 507):
        inputs = _text_inputs(d, S, [0, 5, 131], seed=S)[2]
        _drop_generation_buffers(llm)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = _gen(model, inputs, T)
        torch.cuda.synchronize()
        peaks[S] = torch.cuda.max_memory_allocated() - base
        assert llm._pf["key"] == (B, S, C) and llm._pf["x0"].shape == (B * S, d.llm_h)
        del out
    dS = 507 - 251
    kvw = 2 * d.llm_hkv * HD
    cache = d.llm_layers * B * dS * kvw * (1 if kind == "fp8" else 2)
    if kind == "fp8":
        cache += d.llm_layers * B * dS * 2 * d.llm_hkv * 4 + B * dS * kvw * 2            # scales; the one bf16 staging slab
    embed = B * dS * d.llm_h * 2                                              # the [B * S, h] embedding buffer
    cos_sin = dS * HD * 4                                                    # [Smax, 2, hd / 2] fp32
    ints = B * dS * (8 + 8 + 4 + 4 + 1 + 8)                                  # ids and mask (int64), their int32 forms, the pad compare, slack for one more
    allowed = cache + embed + cos_sin + ints + (1 << 20)
    growth = peaks[507] - peaks[251]
    # what a pass with per-layer buffers (the training forward's save set, without its backward scratch and logits) would add
    per_layer = d.llm_layers * B * dS * ((d.llm_hq + 2 * d.llm_hkv) * HD + d.llm_hq * HD + d.llm_h + 2 * d.llm_inter) * 2
    print(f"PREFILL_MEM {kind} cache: peak over a _generate_step {peaks[251]} B at S = 251, {peaks[507]} B at S = 507: growth {growth} B, "
          f"allowed {allowed} B (cache {cache}, embeddings {embed}, cos/sin {cos_sin}, integer inputs {ints}, 1 MiB); "
          f"per-layer buffers alone would add {per_layer} B")
    assert per_layer > 2 * (1 << 20)                                         # the allowance cannot hide a pass that keeps per-layer buffers
    assert 0 < growth <= allowed, (growth, allowed)
    assert getattr(llm, "sv", None) is None and getattr(llm, "xs", None) is None and getattr(llm, "logits", None) is None


def test_orca_injection_per_chunk(golden_dir):
    """The ORCA golden's inputs on the Qwen3 tiny geometry, as tests/test_gpu_kv8_cache.py::test_fp8_cache_with_orca_injection
    builds them.  The golden's context has 22 positions, two chunks at the smallest chunk size: 14 more columns in front (text for
    row 1, padding for row 0, whose first chunk then is all padding) make it 36 = 16 + 16 + 4."""
    import orca_oracle as RO
    from safetensors.torch import load_file
    from test_gpu_orca import _oracle_with_theta
    from desta.models.modeling_desta25 import DeSTA25AudioModel, prefill_chunks
    g = load_file(os.path.join(golden_dir, "ref_orca_tiny.safetensors"))
    kg, ds, ks, ntr = (int(x) for x in g["orca_dims"])
    d = copy.copy(O.tiny_dims(True))
    d.prompt_size = kg + ntr
    o = RO.OrcaDims(global_num_tokens=kg, local_downsample=ds, local_kernel_size=ks, ortho_diversity_weight=0.05,
                    ortho_weight_qformer_local=0.05, align_weight_local=0.05, global_cross_attn=False, local_enabled=True)
    w = RO.init_weights(d, o, seed=7)
    cfg = cfg_from_dims(d, connector_mode="orca_hybrid", orca_enabled=True, orca_global_num_tokens=kg, orca_local_downsample=ds,
                        orca_local_kernel_size=ks, orca_ortho_diversity_weight=0.05, orca_ortho_weight_qformer_local=0.05,
                        orca_align_weight_local=0.05, orca_rope_theta=float(g["rope_theta_used"]), orca_global_cross_attn=False, orca_local_enabled=True)
    n_ctx, T, extra = int(g["gen_ctx_len"]), int(g["gen_ids"].shape[1]), 14
    n = g["starts"].shape[0]
    front = torch.randint(3, d.vocab, (n, extra), generator=torch.Generator().manual_seed(3))
    front_mask = torch.ones(n, extra, dtype=g["attention_mask"].dtype)
    front[0], front_mask[0] = 0, 0
    inputs = {"context_input_ids": torch.cat([front.to(g["input_ids"].dtype), g["input_ids"][:, :n_ctx]], 1),
              "context_attention_mask": torch.cat([front_mask, g["attention_mask"][:, :n_ctx]], 1),
              "context_batch_start_positions": [(int(b), int(p) + extra) for b, p in g["starts"].tolist()], "batch_features": g["batch_features"],
              "batch_transcription_ids": [g["transcription_ids"][i:i + 1] for i in range(n)]}
    S = n_ctx + extra
    assert len(prefill_chunks(S, 16)) >= 3 and int((inputs["context_attention_mask"][0] == 0).sum()) > 16
    model = DeSTA25AudioModel(cfg, weights=w).eval()
    orig = _oracle_with_theta(float(g["rope_theta_used"]))
    try:
        with torch.no_grad():
            ref_ids = RO.generate(w, d, o, inputs, T, 0)[0]
            lo = RO.generate(w, d, o, inputs, T, 0, forced_tokens=ref_ids)[1]
        for kind in ("bf16", "fp8"):
            model.set_kv_cache(kind)
            model.set_prefill_chunk(None)
            ids_u = _gen(model, inputs, T)[0]                                # the unchunked run's own greedy ids
            model.set_prefill_chunk(16)
            _poison_free_memory()
            ids_c = _gen(model, inputs, T)[0]
            _, logits = _gen(model, inputs, T, ref_ids)
            assert model.orca.S == 1 and all(x is not None for x in model.orca.kv_layers)
            e, gap = _errors(logits, lo, T)
            print(f"PREFILL_CHUNK orca, {kind} cache, chunks {prefill_chunks(S, 16)}: worst per-step logits rel-L2 {e:.3e}  gap/spread {gap:.3f}")
            assert e < REL_BOUND and gap < GAP_BOUND
            assert ids_c.cpu().tolist() == ids_u.cpu().tolist()
    finally:
        RO.rope_whole_vector = orig


def test_launch_counts(hip):
    from desta.models.modeling_desta25 import prefill_chunks
    d, w, model = _model(False)
    H = hip
    S, T, C = 300, 12, 128
    inputs, ref, _ = _oracle(False, S, T)
    L, nch = d.llm_layers, len(prefill_chunks(S, C))
    keys = [S + t + 1 for t in range(T - 1)]                                 # seq_k of the decode steps
    try:
        model.set_prefill_chunk(C)
        model.set_kv_cache("fp8")
        nd, n8, n16 = H.KV8_DEQUANT_CALLS, H.ATTN_KV8_CALLS, H.ATTN_DECODE_CALLS
        _gen(model, inputs, T, ref)
        assert H.KV8_DEQUANT_CALLS - nd == L * nch == 6
        assert H.ATTN_KV8_CALLS - n8 == L * (T - 1) and H.ATTN_DECODE_CALLS == n16
        assert model.llm.kv_stage.shape == (3, S + T, 2 * d.llm_hkv * HD) and model.llm.kv_stage.dtype == torch.bfloat16
        model.set_kv_cache("bf16")
        nd, n8, n16 = H.KV8_DEQUANT_CALLS, H.ATTN_KV8_CALLS, H.ATTN_DECODE_CALLS
        _gen(model, inputs, T, ref)
        assert H.KV8_DEQUANT_CALLS == nd and H.ATTN_KV8_CALLS == n8 and model.llm.kv_stage is None
        assert H.ATTN_DECODE_CALLS - n16 == L * sum(k >= H.DECODE_ATTN_MIN_KEYS for k in keys)
        model.set_prefill_chunk(None)                                        # the unchunked FP8 pass dequantises nothing
        model.set_kv_cache("fp8")
        nd = H.KV8_DEQUANT_CALLS
        _gen(model, inputs, T, ref)
        assert H.KV8_DEQUANT_CALLS == nd
    finally:
        model.set_kv_cache("bf16")
        model.set_prefill_chunk(None)
