"""sha256 digests of what the training attention kernels write, for the library named by DESTA_HIP_LIB (default: the in-tree build).
attn_fwd_k / attn_bwd_dq_k and attn_fwd8_k / attn_bwd_dq8_k share their geometry, key range, K / V staging and mask code
(csrc/attention.hip), so a change there reaches every path at once: run this under the library of the commit before a change and
under the new one, every line must be equal.  One line per case over the raw bytes of every buffer the kernels write, each
pre-filled with a sentinel: O, O_f32 where given, lse, dQ, dK, dV, the dQ-only dQ, and the whole backward workspace (delta and the
dQ / bias partials) after each backward call.  The cases are the tests' own (same builders, same operands):
  * every entry of test_gpu_ops.ATTN_CASES under default switches: forward + backward + dQ-only backward;
  * the O_f32 and transposed-dK|dV cases of tests/test_gpu_attention_fp64.py;
  * every (setting, case) pair of that file's _switch_cases, set_concurrent_bwd(False) included;
  * the four (Sq, Sk) of test_attention_dropout_fwd_bwd, and dropout on a four-wave block (130 x 200), which no test reaches;
  * the two rotary-backward cases of test_rope_in_gemm_epilogue_and_attention_backward.
  python tools/attention_bits.py"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("desta2.5-audio_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import torch
from desta import _hip as H
import test_gpu_attention_fp64 as T
import test_gpu_ops as TO

FILL = 7.0                                                                   # the tests' sentinel


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


class Recording:
    """desta._hip with attention_bwd wrapped: the workspace starts as the sentinel and is kept after every backward call."""

    def __init__(self):
        self.ws = []

    def __getattr__(self, name):
        return getattr(H, name)

    def attention_bwd(self, d, do, *args, **kwargs):
        n = H.lib.desta_attention_bwd_workspace_floats(d.batch, d.n_q_heads, d.seq_q)
        ws = H.scratch(n, do.device, "attn")
        ws.fill_(FILL)
        H.attention_bwd(d, do, *args, **kwargs)
        torch.cuda.synchronize()
        self.ws.append(ws[:n].clone())


def run_case(case, o_f32=False):
    """T._run (forward, backward, dQ-only backward on 7.0-filled buffers) -> digest of its outputs and both workspaces"""
    rec = Recording()
    got = T._run(rec, T.Prepared(case, o_f32, reference=False))
    return sha(*(got[n] for n in sorted(got)), *rec.ws)


def transposed():
    B, Hq, Hkv, Sq, Sk, D, causal, pad = case = T.TRANSPOSED_CASE
    P = T.Prepared(case, False, reference=False)
    qd, kvd, dod, kvs = P.device()
    rec = Recording()
    o = torch.full((B * Sq, Hq * D), FILL, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, Hq, Sq), FILL, device="cuda")
    d = H.attn_desc(qd, kvd, kvd, o, lse, batch=B, hq=Hq, hkv=Hkv, sq=Sq, sk=Sk, hd=D, scale=P.ops["scale"], k_off=0, v_off=Hkv * D)
    H.attention_fwd(d)
    ld = (B * Sk + 63) // 64 * 64 + 64
    t = torch.full((2 * Hq * D, ld), FILL, dtype=torch.bfloat16, device="cuda")
    bias = torch.full((2 * Hq * D,), -1.0, device="cuda")
    dq = torch.full((B * Sq, Hq * D), FILL, dtype=torch.bfloat16, device="cuda")
    rec.attention_bwd(d, dod, dq, dkv_t=(t, ld, bias))
    return sha(o, lse, dq, t, bias, *rec.ws)


def dropout(Sq, Sk, B, H_, D=64):
    qb, kvb, do = TO.dropout_operands(Sq, Sk, B, H_, D)
    rec = Recording()
    o = torch.full((B * Sq, H_ * D), FILL, dtype=torch.bfloat16, device="cuda")
    lse = torch.full((B, H_, Sq), FILL, device="cuda")
    qd, kvd = qb.cuda(), kvb.cuda()
    d = H.attn_desc(qd, kvd, kvd, o, lse, batch=B, hq=H_, hkv=H_, sq=Sq, sk=Sk, hd=D, scale=D ** -0.5, k_off=0, v_off=H_ * D,
                    dropout_p=TO.DROPOUT_P, dropout_seed=TO.DROPOUT_SEED)
    H.attention_fwd(d)
    dq = torch.full((B * Sq, H_ * D), FILL, dtype=torch.bfloat16, device="cuda")
    dkv = torch.full((B * Sk, 2 * H_ * D), FILL, dtype=torch.bfloat16, device="cuda")
    rec.attention_bwd(d, do.cuda(), dq, dkv, dkv, dk_off=0, dv_off=H_ * D)
    dq2 = torch.full((B * Sq, H_ * D), FILL, dtype=torch.bfloat16, device="cuda")
    rec.attention_bwd(d, do.cuda(), dq2)
    return sha(o, lse, dq, dkv, dq2, *rec.ws)


def rope(hd, smajor):
    B, S, Hq, Hkv, K = TO.ROPE_SHAPE
    g, x, W, fr, cs_il, pos, out = TO.rope_projection(H, hd, smajor)
    do = TO.bf(torch.randn(B * S, Hq * hd, generator=g))
    rec = Recording()
    o, lse, dqkv = TO.rope_attention(rec, out, cs_il, do, hd, smajor, fill=FILL)
    return sha(o, lse, dqkv, *rec.ws)


def main():
    for case in TO.ATTN_CASES:
        print(f"default        {str(case):48s} {run_case(case)}", flush=True)
    for case in (T.O_F32_CASE, T.O_F32_FLAT):
        print(f"o_f32          {str(case):48s} {run_case(case, o_f32=True)}", flush=True)
    print(f"transposed     {str(T.TRANSPOSED_CASE):48s} {transposed()}", flush=True)
    for setting, case in T.SWITCH_PARAMS:
        which, value = T.SETTINGS[setting]
        try:
            H.attention_set_option(which, value)
            if setting.endswith("serial"):
                H.attention_set_concurrent_bwd(False)
            print(f"{setting:14s} {str(case):48s} {run_case(case)}", flush=True)
        finally:
            H.attention_set_option(which, T.DEFAULTS[which])
            H.attention_set_concurrent_bwd(True)
    try:                                                                     # the O_f32 case on one stream (its test does the same)
        H.attention_set_concurrent_bwd(False)
        print(f"o_f32,serial   {str(T.O_F32_CASE):48s} {run_case(T.O_F32_CASE, o_f32=True)}", flush=True)
    finally:
        H.attention_set_concurrent_bwd(True)
    for Sq, Sk in TO.DROPOUT_SHAPES:
        print(f"dropout        B 2 H 3 D 64 Sq {Sq:4d} Sk {Sk:4d}                   {dropout(Sq, Sk, 2, 3)}", flush=True)
    print(f"dropout 4-wave B 1 H 2 D 64 Sq  130 Sk  200                   {dropout(130, 200, 1, 2)}", flush=True)
    for hd, smajor in TO.ROPE_CASES:
        print(f"rope           hd {hd:3d} {'position' if smajor else 'batch'}-major S 160{'':22s} {rope(hd, smajor)}", flush=True)


if __name__ == "__main__":
    main()
