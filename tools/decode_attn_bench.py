"""Attention of one KV-cached decode step at Llama-3.1-8B geometry (32 / 8 heads, head_dim 128): the split-KV kernel
(desta_attention_decode: main launch + combine launch) against the forward kernel the decode step used at every length before
(desta_attention_fwd with seq_q = 1), per batch size and cache length.  Operands as decode_step passes them: Q a slice of the
[B, 6144] q|k|v buffer, K | V the halves of [B, Smax, 4096] slabs with Smax = the longest cache of the table; --slabs (32) separate
slabs are visited in rotation, as the 32 layers are, and each line says whether the bytes a rotation touches exceed the 256 MiB
Infinity Cache (HBM) or not (MALL: the figures are then cache bandwidth, not HBM bandwidth).  Both legs alternate in one process
(--rounds alternations).  Per leg: median us over the rounds and the spread (max - min); GB/s counts the K + V bytes of the visible
cache once per KV head; x = forward median / split-KV median.  us = HIP events around a run of back-to-back calls from Python, so it
is kernel time only while the host enqueues faster than the device runs: `enqueue` is the host time per iteration to issue the
calls (no synchronise), and a line whose enqueue time reaches 90 % of a leg's us is marked HOST-BOUND (that leg's figure is then an
upper bound of its kernel time, and the ratio says nothing about the kernels).  `win` = the split-KV leg is faster by more than the
two spreads added: DECODE_ATTN_MIN_KEYS is the smallest multiple of 64 (>= 256) from which every batch size says win.
--kv fp8: the kv8 kernel (desta_attention_decode_kv8) on [B, Smax, 4096] e4m3 byte slabs + [B, Smax, 16] fp32 scales against the
bf16 split-KV kernel (the shipped path from DECODE_ATTN_MIN_KEYS keys on, NOT the forward kernel) at every length; each leg's
GB/s counts the bytes that leg streams (bytes + scales for kv8), x = bf16 split-KV median / kv8 median.
--rows w (2..8, G w <= 16: w <= 4 at this geometry): the attention of a VERIFY step of draft-and-verify decoding, w query rows per
sequence under the causal mask.  New leg: the split-KV verify kernel (desta_attention_verify); old leg: the forward kernel at
seq_q = w on the same slab, what a verify step runs without `set_speculative(attention="split")`.  With --kv fp8 the new leg is
desta_attention_verify_kv8 and the old leg its own bf16 leg, desta_attention_verify.  Both legs stream the bytes the one-row legs
stream (K / V once per KV head), so the GB/s columns compare with a --rows 1 run; a third column, `1row`, is the one-row split-KV
kernel of the new leg's cache kind at the same B and keys, timed in the same alternation: new GB/s well below it means the R = G w
query rows made the kernel VALU-bound.
  python tools/decode_attn_bench.py [--batches 1,8,16,32,64] [--keys 128,256,512,1024,2048,4096] [--rounds 3] [--slabs 32] [--kv {bf16,fp8}] [--rows w]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "desta2.5-audio_amd"))
import torch
from desta import _hip as H

HQ, HKV, HD = 32, 8, 128


def timeit(fn, nbuf):
    reps = max(2 * nbuf, 12)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for i in range(reps):
        fn(i % nbuf)
    enq = (time.perf_counter() - t0) * 1e6 / reps                            # host time to ENQUEUE one iteration
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, enq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,16,32,64")
    ap.add_argument("--keys", default="128,256,512,1024,2048,4096")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slabs", type=int, default=32)
    ap.add_argument("--kv", choices=("bf16", "fp8"), default="bf16", help="fp8: kv8 kernel against the bf16 split-KV kernel")
    ap.add_argument("--rows", type=int, default=1, help="query rows per sequence; > 1: the verify kernels against the forward kernel at seq_q = rows")
    a = ap.parse_args()
    assert a.rounds >= 3, "at least three alternations"
    w = a.rows
    assert 1 <= w <= 8 and (w == 1 or HQ // HKV * w <= H.VERIFY_ATTN_MAX_ROWS), "rows: 1, or 2..8 with G * rows <= 16"
    keys = [int(k) for k in a.keys.split(",")]
    Smax, qkvw, kvw = max(keys), (HQ + 2 * HKV) * HD, 2 * HKV * HD
    kv8 = a.kv == "fp8"
    names = ("kv8", "split-KV") if kv8 else ("split-KV", "forward")
    if w > 1:
        names = (f"verify-kv8 w={w}", f"verify w={w}") if kv8 else (f"verify w={w}", f"forward q={w}")
    print(f"chunk {H.DECODE_ATTN_CHUNK} keys, dispatch threshold {H.DECODE_ATTN_MIN_KEYS} keys, {a.slabs} slabs of [B, {Smax}, {kvw}] bf16"
          + (f" and {a.slabs} of [B, {Smax}, {kvw}] e4m3 bytes + [B, {Smax}, {2 * HKV}] fp32 scales; MiB = both legs' visible bytes" if kv8 else ""))
    for B in (int(b) for b in a.batches.split(",")):
        slabs = [torch.empty(B, Smax, kvw, dtype=torch.bfloat16, device="cuda").normal_() for _ in range(a.slabs)]
        if kv8:                                                              # finite e4m3 bytes of either sign, scales 2^-7 (a Gaussian head's)
            slabs8 = [(torch.randint(0, 0x78, (B, Smax, kvw), dtype=torch.uint8, device="cuda") | (torch.randint(0, 2, (B, Smax, kvw), dtype=torch.uint8, device="cuda") << 7))
                      for _ in range(a.slabs)]
            scales = [torch.full((B, Smax, 2 * HKV), 2.0 ** -7, dtype=torch.float32, device="cuda") for _ in range(a.slabs)]
        qkv = torch.randn(B * w, qkvw, device="cuda").to(torch.bfloat16)
        out = torch.empty(B * w, HQ * HD, dtype=torch.bfloat16, device="cuda")
        lse = torch.empty(B, HQ, w, dtype=torch.float32, device="cuda")
        kv0 = torch.zeros(B, dtype=torch.int32, device="cuda")
        nws = H.attention_verify_workspace_bytes(B, HQ, w, Smax, HD) if w > 1 else H.attention_decode_workspace_bytes(B, HQ, Smax, HD)
        ws = torch.empty(max(nws // 4, 1), dtype=torch.float32, device="cuda")
        for sk in keys:
            def desc(s, sq):                                                 # sq rows per sequence: the descriptor of decode_step / verify_step
                return H.attn_desc(qkv, s, s, out, lse, batch=B, hq=HQ, hkv=HKV, sq=sq, sk=sk, hd=HD, scale=HD ** -0.5, causal=sq > 1, kv_start=kv0,
                                   q_off=0, k_off=0, v_off=HKV * HD, q_rs=qkvw, k_rs=kvw, v_rs=kvw, o_rs=HQ * HD,
                                   q_bs=sq * qkvw, k_bs=Smax * kvw, v_bs=Smax * kvw, o_bs=sq * HQ * HD)
            descs = [desc(s, w) for s in slabs]
            descs1 = [desc(s, 1) for s in (slabs8 if kv8 else slabs)] if w > 1 else None
            if kv8:
                descs8 = [desc(s, w) for s in slabs8]
                vsc = [sc[:, :, HKV:] for sc in scales]
                attn8, attn16 = (H.attention_verify_kv8, H.attention_verify) if w > 1 else (H.attention_decode_kv8, H.attention_decode)

                def new(i):
                    attn8(descs8[i], scales[i], vsc[i], Smax * 2 * HKV, 2 * HKV, ws)

                def old(i):
                    attn16(descs[i], ws)

                def one(i):
                    H.attention_decode_kv8(descs1[i], scales[i], vsc[i], Smax * 2 * HKV, 2 * HKV, ws)
            else:
                def new(i):
                    (H.attention_verify if w > 1 else H.attention_decode)(descs[i], ws)

                def old(i):
                    H.attention_fwd(descs[i])

                def one(i):
                    H.attention_decode(descs1[i], ws)

            for fn in (new, old) + ((one,) if w > 1 else ()):                # warm up every leg on every slab
                for i in range(a.slabs):
                    fn(i)
            tn, to, en, eo, t1 = [], [], [], [], []
            for _ in range(a.rounds):
                t, e = timeit(new, a.slabs)
                tn.append(t), en.append(e)
                t, e = timeit(old, a.slabs)
                to.append(t), eo.append(e)
                if w > 1:
                    t1.append(timeit(one, a.slabs)[0])
            mn, mo = sorted(tn)[len(tn) // 2], sorted(to)[len(to) // 2]
            sn, so = max(tn) - min(tn), max(to) - min(to)
            cache = B * sk * kvw * 2                                         # K + V bytes of one slab's visible cache
            cache_new = B * sk * (kvw + 2 * HKV * 4) if kv8 else cache       # kv8: bytes + scales
            where = "HBM " if (cache + cache_new if kv8 else cache) * a.slabs > 256 * 2**20 else "MALL"
            hb = " HOST-BOUND" if min(en) > 0.9 * mn or min(eo) > 0.9 * mo else ""
            win = "win " if mo - mn > sn + so else "no  "
            print(f"B={B:2d} keys={sk:4d} {where} {(cache + cache_new if kv8 else cache) * a.slabs / 2**20:8.0f} MiB  {names[0]} {mn:8.1f}us (spread {sn:5.1f}, enqueue {min(en):5.1f}) "
                  f"{cache_new / mn / 1e3:7.1f} GB/s   {names[1]} {mo:8.1f}us (spread {so:5.1f}, enqueue {min(eo):5.1f}) {cache / mo / 1e3:7.1f} GB/s   "
                  f"x{mo / mn:5.2f} {win}{hb}" + (f"   1row {sorted(t1)[len(t1) // 2]:8.1f}us {cache_new / sorted(t1)[len(t1) // 2] / 1e3:7.1f} GB/s" if w > 1 else ""), flush=True)
        del slabs, descs
        if kv8:
            del slabs8, scales, descs8, vsc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
