"""Host (no GPU): the dropout-mask restatement and the readouts of tests/dropout_reference.py are proved before they are pointed
at a kernel (tests/test_gpu_dropout_mask.py).

  * known answers: literal (seed, idx) -> 16 bits, computed once with the restatement (the GPU test confirms them against
    dropout_mask_k) and cross-checked here against the Python-integer rng32 of tests/sampling_reference.py;
  * the statistics the comment above desta_rng32 (csrc/common.h) claims, at fixed seeds and N = 2^22 elements, p = 0.1: keep
    fraction within 4.5 binomial sigma; |r| <= 4.5 / sqrt(N) for the masks of seeds s and s + d, of seed_hi neighbours, of
    adjacent elements and at the index shift d * 0x9e3779b9 the additive seed term implies; every output bit of rng32 at mean
    0.5 within 4.5 sigma.  Without the key (the hash before it was added) the shifted streams correlate at exactly 1.0;
  * the four readouts decode the planted mask exactly, values inside the tolerance, through the fp64 emulation at
    (Sq, Sk) = (40, 520), (64, 2), (65, 66), and at (40, 200) with a GQA group (4 query heads on 2 kv heads);
  * every mutation of dropout_reference.MUTATIONS makes at least one readout fail, and what the existing whole-tensor criterion
    (rel-L2 8e-3 on O, 1.5e-2 on dQ / dK / dV; random operands at 2 x 3 x 64 x 1500, and 2 x 4 (2 kv heads) x 64 x 1500 for the
    mutation that needs a GQA group) says to each is printed.

Measured (run with -s), this file's seeds.  Every claim of the common.h comment holds under these bounds:
    keep fraction 0.899890 (thresh / 65536 = 0.100006; limit 0.9 +- 6.6e-4); correlations, limit 2.2e-3: seeds s and s + d
    -6.5e-4, -1.6e-5, +8.5e-4, -1.9e-4, +3.3e-4, -3.0e-4 for d = 1, 16, 256, 512, 256 * 60, 256 * 1000; seed_hi neighbours
    +1.7e-4 and -4.2e-4; adjacent elements -2.3e-4 (pair partners +1.3e-5, neighbouring pairs -4.7e-4); at the implied shift
    -3.6e-4, +5.3e-4, +8.0e-4 (d = 256 * 60: 8 870 912 pairs), +9.5e-4, and exactly 1.0 without the key; output bits
    0.49949 .. 0.50038 (limit 0.5 +- 1.1e-3).
    mutation                 rejected by the readout                                 the whole-tensor criterion at 64 x 1500
    pair_halves_swapped      fwd dV dQ dK at all three shapes                        rejects it too (O 0.45, dQ 0.47, dK 0.46, dV 0.45)
    thresh_strict            fwd dV dQ dK at all three (1-2 pairs differ)            ACCEPTS it (O 6.8e-3, dQ 7.2e-3, dK 6.9e-3, dV 6.6e-3)
    head_uses_hkv            fwd dV dQ dK at all three (Hq 4, Hkv 2: dV / dK read    rejects it too (O 0.33, dQ 0.31, dK 0.31, dV 0.32)
                             one head of each group per pass)
    row_unclamped_tail       fwd at all three; dQ dK as well at Sk = 2 and 66, where  rejects it on O (1.2e-2 against 8e-3); dQ 1.7e-3,
                             the forward's delta moves by more than the tolerance    dK 5.5e-4, dV 0 pass
    bwd_rows_8_15_from_0_7   dV dK at all three, fwd and dQ pass                     rejects it too (dK 0.33, dV 0.32; O, dQ 0)
So of the five only thresh_strict gets past the whole-tensor criterion at this shape; what the readouts add for the others is
the exact statement (the mask IS the reference's, pair by pair, in each kernel family) and the pair, tile and row where it is not."""
import numpy as np
import pytest
import torch

import dropout_reference as R
import sampling_reference as S

P = 0.1
N = 1 << 22
SEED = (7 << 40) | 12345
SIGMA = 4.5
READOUT_SHAPES = [(40, 520), (64, 2), (65, 66)]
OLD_LIMIT = {"O": 8e-3, "dQ": 1.5e-2, "dK": 1.5e-2, "dV": 1.5e-2}

# (seed, element index) -> bits16: seed 0, a seed with a high word, idx >= 2^32 (the pair index carries into the high word from
# 2^33 on), odd and even halves.  The GPU test imports this table.
KNOWN = [
    (0, 0, 0x0000), (0, 1, 0x0000), (0, 2, 0x90C0), (0, 3, 0x6889),
    (12345, 6, 0x5A02), (12345, 7, 0xE652),
    ((7 << 40) | 12345, 0, 0xC409), ((7 << 40) | 12345, 1, 0x8BD0),
    ((7 << 40) | 12345, (1 << 32) + 4, 0xBC8E), ((7 << 40) | 12345, (1 << 33) + 5, 0x3294),
    ((1 << 64) - 1, (1 << 33) + 2, 0x9D7F), ((1 << 64) - 1, 1000001, 0x436E),
]


def test_known_answers():
    for seed, idx, bits in KNOWN:
        got = int(R.bits16(seed, [idx])[0])
        print(f"bits16({seed:#x}, {idx:#x}) = {got:#06x}")
        assert got == bits, (hex(seed), hex(idx), hex(got))
        pair = idx >> 1
        h = S.rng32(seed, pair >> 32, pair & R.M32)                        # an independent spelling of the same hash
        assert got == ((h >> 16) if idx & 1 else (h & 0xFFFF))
    assert {i & 1 for _, i, _ in KNOWN} == {0, 1} and any(i >= 1 << 33 for _, i, _ in KNOWN) and any(s >> 32 for s, _, _ in KNOWN)
    assert [R.drop_thresh(p) for p in (1e-6, 0.1, 0.5, 0.99999)] == [1, 6554, 32768, 0xFFFF]
    assert R.drop_scale(0.1) == float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(0.1)))


def _corr(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std()))


def _pairs_keep(seed, pairs, key=True):
    """keep of the 2 x len(pairs) elements of the given pair indices (low half first); key=False: the hash without the key."""
    h = R.rng32(seed, pairs) if key else _rng32_keyless(seed, pairs)
    t = np.uint64(R.drop_thresh(P))
    return np.stack([(h & np.uint64(0xFFFF)) >= t, (h >> np.uint64(16)) >= t], axis=1).reshape(-1)


def _rng32_keyless(seed, idx):
    m = np.uint64(R.M32)
    seed_lo, seed_hi = seed & R.M32, seed >> 32
    with np.errstate(over="ignore"):
        x = ((idx & m) + np.uint64((seed_lo * 0x9E3779B9) & R.M32) + (((idx >> np.uint64(32)) + np.uint64(seed_hi)) & m) * np.uint64(0x85EBCA6B)) & m
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7FEB352D)) & m
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x846CA68B)) & m
        x ^= x >> np.uint64(16)
    return x


def test_keep_fraction():
    frac = float(R.keep(SEED, N, P).mean())
    q = R.drop_thresh(P) / 65536.0
    lim = SIGMA * np.sqrt(0.09 / N)
    print(f"keep fraction {frac:.6f} (p = {P}: thresh / 65536 = {q:.6f}; limit 0.9 +- {lim:.1e})")
    assert abs(frac - 0.9) <= lim


def test_stream_correlations():
    lim = SIGMA / np.sqrt(N)
    base = R.keep(SEED, N, P)
    res = {}
    for d in (1, 16, 256, 512, 256 * 60, 256 * 1000):
        res[f"seed + {d}"] = _corr(base, R.keep(SEED + d, N, P))
    res["seed_hi + 1"] = _corr(base, R.keep(SEED + (1 << 32), N, P))
    res["seed_hi + 1 (low seed)"] = _corr(R.keep(12345, N, P), R.keep(12345 + (1 << 32), N, P))
    res["adjacent elements"] = _corr(base[:-1], base[1:])
    res["pair partners"] = _corr(base[0::2], base[1::2])
    res["neighbouring pairs"] = _corr(base[1:-1:2], base[2::2])
    for name, r in res.items():
        print(f"correlation, {name}: {r:+.2e} (limit {lim:.1e})")
    for name, r in res.items():
        assert abs(r) <= lim, (name, r)


def test_shifted_stream_correlations():
    """mask(seed + d, pair i) against mask(seed, pair i + d * 0x9e3779b9): identical without the key, independent with it."""
    lim = SIGMA / np.sqrt(N)
    pairs = np.arange(N // 2, dtype=np.uint64)
    for d in (1, 256, 256 * 60, 256 * 1000):
        shift = (d * 0x9E3779B9) & R.M32
        moved = (pairs + np.uint64(shift)) & np.uint64(R.M32)
        r = _corr(_pairs_keep(SEED + d, pairs), _pairs_keep(SEED, moved))
        r0 = _corr(_pairs_keep(SEED + d, pairs, key=False), _pairs_keep(SEED, moved, key=False))
        print(f"correlation at the implied shift, d = {d} ({shift} pairs): {r:+.2e} (limit {lim:.1e}); without the key {r0:.3f}")
        assert abs(r) <= lim, (d, r)
        assert r0 == 1.0 or abs(r0 - 1.0) < 1e-12
    assert (256 * 60 * 0x9E3779B9) & R.M32 == 8870912                       # the figure of the common.h comment


def test_every_output_bit_is_fair():
    h = R.rng32(SEED, np.arange(N, dtype=np.uint64))
    means = [float(((h >> np.uint64(b)) & np.uint64(1)).mean()) for b in range(32)]
    lim = SIGMA * 0.5 / np.sqrt(N)
    print(f"output bits: mean {min(means):.5f} .. {max(means):.5f} (limit 0.5 +- {lim:.1e})")
    assert all(abs(m - 0.5) <= lim for m in means), means


# ------------------------------------------------------------------------------------------------------- readouts, mutations
def _read_all(keeps, ref, Hkv, scale, kinds=R.KINDS):
    """{kind: (decoded == ref everywhere, worst value error / tolerance, first mismatch)} through the fp64 emulation."""
    c = R.drop_scale(P)
    out = {}
    for kind in kinds:
        mask, worst = R.read_mask(kind, lambda q, k, v, do: R.attention(q, k, v, do, scale, keeps, c), ref, Hkv, P, scale)
        out[kind] = (bool(torch.equal(mask, ref)), worst, R.first_mismatch(mask, ref))
    return out


@pytest.mark.parametrize("Sq,Sk,H,Hkv", [s + (3, 3) for s in READOUT_SHAPES] + [(40, 200, 4, 2)])
def test_readouts_decode_the_planted_mask(Sq, Sk, H, Hkv):
    B = 2
    ref = torch.from_numpy(R.attn_keep(SEED, B, H, Sq, Sk, P))
    assert torch.equal(R.planted_keeps(SEED, B, H, Hkv, Sq, Sk, P)["fwd"], ref)
    res = _read_all(ref, ref, Hkv, 0.125)
    for kind, (same, worst, where) in res.items():
        print(f"({Sq}, {Sk}) Hq {H} Hkv {Hkv} {kind}: mask {'exact' if same else where}; worst value error {worst:.2e} of the tolerance")
        assert same and worst <= 1e-6, (kind, worst, where)                  # fp64 has nothing to round
    assert set(res) == set(R.KINDS)


def _mutation_case(mut, Sq, Sk):
    """(seed, B, Hq, Hkv) at which the mutation is looked for."""
    B, Hq, Hkv, seed = 2, 3, 3, SEED
    if mut == "head_uses_hkv":
        Hq, Hkv = 4, 2
    if mut == "thresh_strict":
        seed, at = R.seed_with_boundary(B * Hq * Sq * Sk, P, SEED)
        assert int(R.bits16(seed, [at])[0]) == R.drop_thresh(P)
    return seed, B, Hq, Hkv


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_mutations_are_rejected_by_a_readout(mut):
    applicable = 0
    for Sq, Sk in READOUT_SHAPES:
        seed, B, Hq, Hkv = _mutation_case(mut, Sq, Sk)
        ref = torch.from_numpy(R.attn_keep(seed, B, Hq, Sq, Sk, P))
        keeps = R.planted_keeps(seed, B, Hq, Hkv, Sq, Sk, P, mutation=mut)
        if all(torch.equal(m, ref) for m in keeps.values()):
            print(f"{mut} ({Sq}, {Sk}): changes no pair at this shape")
            assert mut == "row_unclamped_tail"                               # (a tail pair may draw the same bits twice: (64, 2))
            continue
        applicable += 1
        res = _read_all(keeps, ref, Hkv, 0.125)
        failed = [k for k, (same, worst, _) in res.items() if not same or worst > 1.0]
        print(f"{mut} ({Sq}, {Sk}) Hq {Hq} Hkv {Hkv}: " + (f"rejected by the readout ({' '.join(failed)}): {res[failed[0]][2]}" if failed else "NOT rejected"))
        assert failed, (mut, Sq, Sk)
        # the readouts of the kernels a mutation leaves alone pass; a forward that disagrees with the backward also moves delta
        # (= O[q, 0]) by c / n per pair, which the dQ / dK VALUES see once 1 / n is over the tolerance (Sk < 64)
        if mut == "row_unclamped_tail":
            assert "fwd" in failed and "dV" not in failed, failed
        if mut == "bwd_rows_8_15_from_0_7":
            assert set(failed) == {"dV", "dK"}, failed
    assert applicable >= 2


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_what_the_whole_tensor_criterion_says(mut):
    """Printed, not asserted: the rel-L2 of test_attention_dropout_fwd_bwd on random operands with the mutated masks."""
    Sq, Sk = 64, 1500
    seed, B, Hq, Hkv = _mutation_case(mut, Sq, Sk)
    g = torch.Generator().manual_seed(Sq + Sk)
    q, do = (torch.randn(B, Sq, Hq, 64, generator=g).bfloat16() for _ in range(2))
    k, v = (torch.randn(B, Sk, Hkv, 64, generator=g).bfloat16() for _ in range(2))
    c = R.drop_scale(P)
    ref = R.attention(q, k, v, do, 0.125, torch.from_numpy(R.attn_keep(seed, B, Hq, Sq, Sk, P)), c)
    out = R.attention(q, k, v, do, 0.125, R.planted_keeps(seed, B, Hq, Hkv, Sq, Sk, P, mutation=mut), c)
    rel = {n: float((out[n] - ref[n]).norm() / ref[n].norm()) for n in ("O", "dQ", "dK", "dV")}
    over = [n for n in rel if rel[n] >= OLD_LIMIT[n]]
    print(f"{mut} at {B} x {Hq} ({Hkv} kv) x {Sq} x {Sk}: whole-tensor rel-L2 " + " ".join(f"{n} {r:.1e}" for n, r in rel.items())
          + (f": rejected there too (on {' '.join(over)})" if over else ": ACCEPTED by the old criterion"))
    assert any(r > 0 for r in rel.values())
