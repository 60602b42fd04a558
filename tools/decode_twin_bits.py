"""sha256 digests of what the decode twins write, for the library named by DESTA_HIP_LIB (default: the in-tree build).
attn_decode_k / attn_kv8_k and rope_k / rope_kv8_k come from one source each, so the tests that hold kv8 to the bf16 kernel's bits
cannot see a change made to both: run this under the library of the commit before a change and under the new one, every line
must be equal.  One line per case over the raw bytes of
  * O, lse and the whole NaN-filled workspace of attention_decode and attention_decode_kv8: the cases of
    tests/test_gpu_decode_attention.py and tests/test_gpu_kv8_cache.py (HEADS x the seven _seq_ks lengths x B in {1, 3}:
    chunk edges, left pads, an all-masked chunk);
  * the q|k|v buffer, the cache slab and the scales after rope_kv_append and rope_kv_append_e4m3: the eight configurations of
    test_append_is_exact, and a 3 x 251-row prompt with and without the q/k-norm (the small ones miss a fused multiply-add that
    took the other product in one element pair of sixteen; the model tests caught it);
  * the same three after the append pair with a non-zero q|k|v bias: the inputs of tests/test_gpu_qwen2_kernels.py for its
    SHAPES x GRIDS (e4m3 where hd = 128), and a 3 x 251-row prompt for the reason above;
  * the q|k|v buffer after rope in place at hd 64 and 128, at (B, S) = (3, 5), (20, 4) and (3, 251), batch-major and
    position-major, with and without pos_shift: forward and backward, each with and without the q/k-norm (the backward with
    its pre_norm), and the forward with a bias.  Together: every instantiation of rope_k and rope_kv8_k.
  python tools/decode_twin_bits.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("desta2.5-audio_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
from desta import _hip as H
import test_gpu_decode_attention as T16
import test_gpu_kv8_cache as T8
import test_gpu_qwen2_kernels as TQ


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def main():
    for c8 in T8._all_cases8(H):
        c = c8.c
        qbuf, by, sc, kv, deq = c8.device()
        out, lse = T8._outputs(c.B, c.Hq)
        ws = T8._workspace(H, c.B, c.Hq, c.sk)
        H.attention_decode(T8._desc(H, c, qbuf, deq, kv, out, lse, c.Smax), ws)
        torch.cuda.synchronize()
        d16 = sha(out, lse, ws)
        out, lse = T8._outputs(c.B, c.Hq)
        ws = T8._workspace(H, c.B, c.Hq, c.sk)
        H.attention_decode_kv8(T8._desc(H, c, qbuf, by, kv, out, lse, by.shape[1]), sc, sc[:, :, c.Hkv:], sc.stride(0), sc.stride(1), ws)
        torch.cuda.synchronize()
        print(f"attn Hq {c.Hq} Hkv {c.Hkv} B {c.B} sk {c.sk:5d}  bf16 {d16}  kv8 {sha(out, lse, ws)}", flush=True)
    for Hq, Hkv, norm, form in T8.APPEND_CONFIGS + [(4, 2, False, "long"), (4, 2, True, "long")]:
        if form == "long":                                                   # 753 rows, positions to 250: a rounding that differs in one
            g = torch.Generator().manual_seed(251 + norm)                    # element of a few shows here, not in 5 to 15 rows
            B, S, slot0, Smax, ld = 3, 251, 0, 263, (Hq + 2 * Hkv) * T8.HD
            qkv, cs = torch.randn(B * S, ld, generator=g).bfloat16(), T8._cos_sin(Smax).cuda()
            qn = (1 + 0.1 * torch.randn(T8.HD, generator=g)).cuda() if norm else None
            kn = (1 + 0.1 * torch.randn(T8.HD, generator=g)).cuda() if norm else None
            shift = torch.tensor([0, -5, -131], dtype=torch.int32).cuda()
        else:
            B, S, slot0, Smax, ld, qkv, cs, qn, kn, shift = T8.append_inputs(Hq, Hkv, norm, form)
        kvw = 2 * Hkv * T8.HD
        a, b = qkv.cuda(), qkv.cuda()
        c16 = torch.full((B, Smax, kvw), -3.0, dtype=torch.bfloat16, device="cuda")
        c8 = torch.full((B, Smax, kvw), 0xAB, dtype=torch.uint8, device="cuda")
        sc = torch.full((B, Smax, 2 * Hkv), -7.0, dtype=torch.float32, device="cuda")
        H.rope_kv_append(a, ld, B * S, S, Hq, Hkv, T8.HD, cs, qn, kn, 1e-6, shift, c16, c16.stride(0), c16.stride(1), slot0)
        H.rope_kv_append_e4m3(b, ld, B * S, S, Hq, Hkv, T8.HD, cs, qn, kn, 1e-6, shift, c8, c8.stride(0), c8.stride(1), sc, sc.stride(0), sc.stride(1), slot0)
        torch.cuda.synchronize()
        print(f"append Hq {Hq} Hkv {Hkv} norm {int(norm)} {form:6s}  bf16 {sha(a, c16)}  e4m3 {sha(b, c8, sc)}", flush=True)
    rope_cases()


def rope_cases():
    """The append pair with a non-zero q|k|v bias, and rope in place: every instantiation of rope_k and rope_kv8_k."""
    for (Hq, Hkv, hd), (B, S) in [(s, g) for s in TQ.SHAPES for g in TQ.GRIDS + [(3, 251)]]:
        if S == 251 and (Hq, Hkv, hd) != TQ.SHAPES[-1]:
            continue                                                         # the long case once
        ld, qkv, bias, shift, cs = TQ._inputs(Hq, Hkv, hd, B, S)
        slot0, Smax, kvw = 3, S + 6, 2 * Hkv * hd
        a, b, cs, bias, shift = qkv.cuda(), qkv.cuda(), cs.cuda(), bias.cuda(), shift.cuda()
        c16 = torch.full((B, Smax, kvw), -3.0, dtype=torch.bfloat16, device="cuda")
        c8 = torch.full((B, Smax, kvw), 0xAB, dtype=torch.uint8, device="cuda")
        sc = torch.full((B, Smax, 2 * Hkv), -7.0, dtype=torch.float32, device="cuda")
        H.rope_kv_append(a, ld, B * S, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c16, c16.stride(0), c16.stride(1), slot0, bias=bias)
        d8 = "-"
        if hd == 128:
            H.rope_kv_append_e4m3(b, ld, B * S, S, Hq, Hkv, hd, cs, None, None, 1e-6, shift, c8, c8.stride(0), c8.stride(1), sc, sc.stride(0), sc.stride(1),
                                  slot0, bias=bias)
            d8 = sha(b, c8, sc)
        torch.cuda.synchronize()
        print(f"append+bias Hq {Hq} Hkv {Hkv} hd {hd} B {B} S {S}  bf16 {sha(a, c16)}  e4m3 {d8}", flush=True)
    for hd in (64, 128):
        for B, S in TQ.GRIDS + [(3, 251)]:
            Hq, Hkv = 4, 2
            ld, qkv, bias, shift, cs = TQ._inputs(Hq, Hkv, hd, B, S)
            g = torch.Generator().manual_seed(hd + B + S)
            qn, kn = ((1 + 0.1 * torch.randn(hd, generator=g)).cuda() for _ in range(2))
            pre = torch.randn(B * S, ld, generator=g).bfloat16().cuda()        # the backward's saved pre-norm q|k
            cs, bias, shift = cs.cuda(), bias.cuda(), shift.cuda()
            for smb in (0, B):
                for sh in (None, shift):
                    for what, kw in (("fwd", dict()), ("fwd+norm", dict(q_norm_w=qn, k_norm_w=kn)), ("bwd", dict(backward=True)),
                                     ("bwd+norm", dict(q_norm_w=qn, k_norm_w=kn, backward=True, pre_norm=pre, ld_pre=ld)), ("fwd+bias", dict(bias=bias))):
                        buf = qkv.cuda()
                        H.rope(buf, ld, B * S, S, Hq, Hkv, hd, cs, pos_shift=sh, s_major_batch=smb, **kw)
                        torch.cuda.synchronize()
                        print(f"rope hd {hd} B {B} S {S} s_major {int(smb > 0)} shift {int(sh is not None)} {what:8s}  {sha(buf)}", flush=True)


if __name__ == "__main__":
    main()
