"""Exact references, kernel-shaped emulations and seeded mutations for the glue kernels of csrc/embed_ce.hip and
csrc/norm_act.hip: the row movers (embed_gather_k, gather_rows_k, scatter_rows_k), target_rows_k, mask_tokens_k, the column sum
(colsum_partial_k<8|4> + reduce_partials_k), the transposes (transpose_k / transpose_vec_k, bf16 and fp32 input),
cast_f32_bf16_k and add_f32_k.  Plain torch on the CPU; imported by the host test (test_glue_exact_host.py) and the GPU test
(test_gpu_glue_exact.py), which share the case table `CASES` and the operand generator `operands()`.

These kernels are exact by contract, so there is no error bound to hold them to (one exception below): a fault shows as the
wrong row, a missing column, a dropped partial.  Per operation this module has

    fresh(op, o)            -> {name: flat buffer}   every buffer the kernel writes, as it is BEFORE the call: the output filled
                                                     with the sentinel (or with what the operation updates in place), followed by
                                                     GUARD sentinel elements; for the transpose also two whole rows behind row
                                                     `cols`, and `off` elements in front where the output is an offset view
    reference(op, o)        -> {name: flat buffer}   the same buffers as they must be AFTER the call, written the obvious way
                                                     (indexing, Python loops, int64 / float64 sums) into fresh(): whatever the
                                                     operation does not own still holds the sentinel
    emulate(op, o, mutation)-> {name: flat buffer}   the same, written the way the KERNEL partitions the work (below), optionally
                                                     with one seeded mutation of that partition
    mismatch(op, o, ref, got) -> None | str          the comparison rule, the one the GPU test applies to the kernel's buffers

16-bit data travels as int16 bit patterns (the GPU test views them as bf16 on the device), so NaN payloads, signed zeros and
denormals are compared as bits.

Comparison rules (`mismatch`):
    copies (embed_gather, gather_rows, scatter_rows, transpose of bf16 input, mask_tokens, and idx / lab / count of
    target_rows): every element of every buffer equal, guards and untouched regions included
    fp32 -> bf16 (cast, transpose of fp32 input): equal bits to x.bfloat16() on the CPU; where that is a NaN the result must be
    a NaN (any payload)
    add: equal bits to the CPU fp32 add
    colsum, data = "int" (integers in [-8, 8], exact in bf16): out == the int64 column sum (+ the integer `prev` with
    accumulate), EXACTLY: `rows * 8 + 64 < 2^24` for every case, so every partial sum of every summation order is an integer fp32
    holds exactly (asserted from the table by the host test)
    colsum, data = "randn": per column |out - fp64| <= gamma_L sum_r |x[r, c]| (+ half an fp32 ulp of |out| for the accumulate
    add), gamma_L = L 2^-24 / (1 - L 2^-24).  The limit is 1 x the bound.

L of a colsum case (`colsum_chain`), derived from the case alone: nr = colsum_splits(rows, cols);
    L = ceil(rows / nr)      additions of one thread of colsum_partial_k (rows r0, r0 + nr, ...)
      + ceil(nr / 64)        additions into one accumulator of reduce_partials_k (partial rows b, b + 64, ...)
      + 8                    the fixed combine: (a0 + a1) + (a2 + a3) is 2 deep, (comb[g] + comb[g+1]) + (comb[g+2] + comb[g+3])
                             2 deep, and `s +=` runs 4 times
The step-16 tail of reduce_partials_k goes into a0 alone and can add up to 3 further terms to that accumulator (nr = 113: wave
group 1 adds rows 1 | 65, 81, 97).  L still bounds the number of ROUNDINGS on the longest chain, because three of the additions it
counts are onto a zero and exact: the first of a partial thread, the first of an accumulator and the first `s +=`.
`colsum_roundings` counts them by walking the loops and the host test asserts colsum_roundings <= L for every case.

How the emulations partition (what a mutation then breaks):
    row movers      blocks of 4 rows (one wave each, `row >= rows` leaves), a lane copies 8 elements at lane * 8 and strides
                    by 512; audio row -(s + 1); the scatter writes row idx[row]
    target_rows     1024 threads, thread t owns rows [t per, (t + 1) per), per = ceil(B S / 1024); counts, exclusive scan,
                    compaction; a row m is a target iff (m % S) + 1 < S and labels[m + 1] != -100
    mask_tokens     one thread per (row, id): r = i / n, c = ids[i % n], written iff 0 <= c < cols
    colsum          nr = colsum_splits partial rows, V = 8 iff cols % 8 == 0, ld % 8 == 0 and x 16-byte aligned, else 4; the
                    reduce in blocks of 64 columns, 16 wave groups x 4 accumulators stepping 64 while b + 48 < nr, then a
                    step-16 tail into a0; all additions in fp32 in the kernel's order
    transpose       64 x 64 tiles over a grid of ceil(cols / 64) x ceil(ld_out / 64); the vector kernel iff cols, ld_in,
                    ld_out are multiples of 8 and both pointers 16-byte aligned, writing 8 output columns at a time where
                    r0 + rc * 8 < ld_out; rows >= `rows` of a tile are zeros
    cast / add      8 / 4 elements per thread
A read a mutation sends out of bounds returns 0 (-100 for labels, -1 for ids, row 0 for a row index); a write it sends past the
buffer (output + guard) is dropped.  `no_row_test` is seeded in the two gathers only: there the stray wave writes row `row` of
the output, which is the guard; in the scatter its destination is an index read out of bounds, which no test can place.
`v8_on_4` is a race between blocks (a partial row's last vector spills into the next partial row); the emulation lets the spill
land last.

`MUTANTS`: name -> (operations, what it is).  `lane_stride_256` changes no output of any case: the lanes then copy every
vector twice, and a copy is idempotent.  It is kept in the table as the one EQUIVALENT mutant (`EQUIVALENT`); the host test
asserts that it equals the reference on every case rather than pretending a case catches it.
"""
import torch

GUARD = 64
SENT16 = 0x40E0                  # bf16 7.0
F = 2.0 ** -24

MOVERS = ("embed_gather", "gather_rows", "scatter_rows")
OPS = MOVERS + ("target_rows", "mask_tokens", "colsum", "transpose", "cast", "add")

MUTANTS = {
    "lane_stride_256": (MOVERS, "lane stride 512 -> 256 elements"),
    "lane_stride_1024": (MOVERS, "lane stride 512 -> 1024 elements"),
    "last_chunk_skipped": (MOVERS, "last 8-element chunk of a row skipped"),
    "no_row_test": (("embed_gather", "gather_rows"), "`row >= rows` dropped for the last block (the write lands in the guard)"),
    "audio_minus_s": (("embed_gather",), "audio index -(s + 1) -> -s"),
    "scatter_to_row": (("scatter_rows",), "scatter writes row `row` instead of idx[row]"),
    "no_shift_guard": (("target_rows",), "`(m % S) + 1 < S` dropped"),
    "per_floor": (("target_rows",), "per = M / 1024"),
    "first_from_row": (("target_rows",), "count[1] from row ids instead of positions"),
    "s_major_swapped": (("target_rows",), "s_major formula with B and S swapped"),
    "no_trailing_label": (("target_rows",), "lab[1 + n] = -100 missing"),
    "mask_div_mod_swapped": (("mask_tokens",), "i / n and i % n swapped"),
    "mask_bound_ld": (("mask_tokens",), "bound c < ld instead of c < cols"),
    "mask_plus_inf": (("mask_tokens",), "value 0xff80 -> 0x7f80"),
    "reduce_tail_late": (("colsum",), "tail loop of reduce_partials_k starts one group late"),
    "reduce_64_no_tail": (("colsum",), "b + 48 < nblk -> b + 64 < nblk with no tail"),
    "last_partial_dropped": (("colsum",), "last partial row dropped"),
    "v8_on_4": (("colsum",), "V = 8 path taken when cols % 8 == 4"),
    "accumulate_ignored": (("colsum",), "accumulate ignored"),
    "no_tail_tiles": (("transpose",), "zero tail not written beyond the last row tile"),
    "vec_tail_rows": (("transpose",), "vector path's r0 + rc*8 < ld_out -> < rows"),
    "f32_truncated": (("transpose", "cast"), "fp32 input truncated instead of rounded to nearest even"),
}
EQUIVALENT = ("lane_stride_256",)

# 16-bit patterns every copied operand carries: quiet / signalling NaN payloads, +-0, +-inf, denormals
SPECIAL16 = (0x7FC0, 0x7F81, 0xFFC1, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x0001, 0x807F, 0x7FFF, 0xFFFF, 0x0080)
# fp32 patterns of the cast: bf16 ties with an even / odd lower neighbour (both signs), one bit either side of a tie, the
# largest finite fp32 (rounds to inf) and a tie that does, +-inf, quiet and signalling NaNs (0x7f800001 truncates to inf),
# fp32 denormals (0x00008000 is a tie of the bf16 denormals, 0x00018000 one with an odd neighbour), +-0
SPECIAL32 = (0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F817FFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,
             0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC12345, 0x00000001, 0x007FFFFF, 0x00008000, 0x00018000,
             0x807FFFFF, 0x00000000, 0x80000000, 0x3F800000)


def case_id(case):
    return "-".join(f"{k}={v}" for k, v in case.items()).replace(" ", "")


def _i16(vals):
    return torch.tensor([v - 65536 if v >= 32768 else v for v in vals], dtype=torch.int16)


def _f32_bits(vals):
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in vals], dtype=torch.int32).view(torch.float32)


def bf16_bits(x):
    """fp32 tensor -> the int16 bit patterns of x.bfloat16() (round to nearest even, NaN kept a NaN)"""
    return x.bfloat16().view(torch.int16)


def bits_f32(b):
    """int16 bf16 bit patterns -> the fp32 values (exact)"""
    return (b.to(torch.int32) << 16).view(torch.float32)


def is_nan16(b):
    return (b.to(torch.int32) & 0x7FFF) > 0x7F80


def sentinel(dtype):
    return SENT16 if dtype == torch.int16 else 7


def _buf(n, dtype):
    return torch.full((n + GUARD,), sentinel(dtype), dtype=dtype)


# ------------------------------------------------------------------------------------------------------------ case table
def colsum_splits(rows, cols):
    """colsum_splits of norm_act.hip"""
    xb = (cols // 4 + 255) // 256
    return max(1, min((2048 + xb - 1) // xb, rows // 8, 512))


def _up(v, m):
    return (v + m - 1) // m * m


def _cases():
    c = {}
    hid, rws = (8, 504, 512, 520, 1024, 3584, 4096), (1, 3, 4, 9)
    for op in MOVERS:
        c[op] = [dict(rows=5, hidden=h, idx="mixed") for h in hid] + [dict(rows=r, hidden=520, idx="mixed") for r in rws]
    c["embed_gather"] += [dict(rows=9, hidden=1024, idx="tokens"), dict(rows=9, hidden=1024, idx="audio")]
    c["target_rows"] = [dict(B=B, S=S, labels=p, s_major=sm)
                        for B, S in ((1, 1), (3, 1), (1, 2), (5, 37), (2, 512), (1, 1025), (3, 683), (7, 1171))
                        for p in ("prefix", "none", "all", "first", "last") for sm in (0, 1)]
    c["mask_tokens"] = [dict(rows=r, n=n, cols=504, ld=504 + pad) for r in (1, 3, 64) for n in (1, 88, 300) for pad in (0, 8)]
    # colsum: rows -> nr = colsum_splits(rows, 72) in the comment; every case with integer and with random normal data
    cs = []
    for i, (rows, nr) in enumerate(((1, 1), (5, 1), (7, 1), (19, 2), (123, 15), (131, 16), (139, 17), (387, 48), (395, 49),
                                    (507, 63), (515, 64), (523, 65), (899, 112), (907, 113), (4104, 512))):
        assert colsum_splits(rows, 72) == nr
        cs.append(dict(rows=rows, cols=72, ld=72, off=0, accumulate=i % 2))
    for i, cols in enumerate((4, 8, 60, 64, 68, 1028, 2056)):
        cs.append(dict(rows=139, cols=cols, ld=cols, off=0, accumulate=1 - i % 2))
    cs += [dict(rows=139, cols=72, ld=76, off=0, accumulate=0), dict(rows=139, cols=72, ld=80, off=0, accumulate=1),
           dict(rows=139, cols=72, ld=72, off=8, accumulate=1), dict(rows=139, cols=72, ld=72, off=4, accumulate=0),
           dict(rows=523, cols=2056, ld=2064, off=8, accumulate=0), dict(rows=523, cols=1028, ld=1032, off=4, accumulate=1),
           # cols % 8 == 4 with everything else fit for 16-byte loads: only `cols % 8` keeps these on V = 4
           dict(rows=139, cols=68, ld=72, off=0, accumulate=0), dict(rows=523, cols=1028, ld=1032, off=0, accumulate=1)]
    c["colsum"] = [dict(k, data=d) for k in cs for d in ("int", "randn")]
    tr = []
    sizes = (1, 7, 8, 63, 64, 65, 72, 129)
    for rows, cols in [(s, s) for s in sizes] + [(7, 72), (72, 7), (129, 8), (8, 129), (65, 64)]:
        lds = sorted({rows, _up(rows, 8), _up(rows, 64), _up(rows, 64) + 64})
        for k, ld_out in enumerate(lds):
            for j, f32 in enumerate((0, 1)):
                tr.append(dict(rows=rows, cols=cols, ld_out=ld_out, ld_in=cols + 8 * ((k + j) % 2), f32=f32))
    c["transpose"] = tr
    c["cast"] = [dict(n=n) for n in (8, 2048, 2056)]
    c["add"] = [dict(n=n) for n in (4, 1024, 1028)]
    return c


CASES = _cases()


# ------------------------------------------------------------------------------------------------------------ operands
def _bits16(g, n):
    return torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16)


def _rows16(g, rows, h):
    """[rows, h] random 16-bit patterns, the special ones at the head of the first and the tail of the last row"""
    x = _bits16(g, rows * h).view(rows, h)
    sp = _i16(SPECIAL16)
    k = min(h, len(sp))
    x[0, :k] = sp[:k]
    x[-1, h - k:] = sp[len(sp) - k:]
    return x


TABLE_ROWS, AUDIO_ROWS, SRC_ROWS = 11, 6, 7


def operands(op, case, seed=0):
    """The operands of one case on the CPU (deterministic in (op, case, seed)); 16-bit data as int16 bit patterns."""
    g = torch.Generator().manual_seed(1000 * seed + sum(ord(ch) for ch in op + case_id(case)))
    o = dict(case)
    if op in MOVERS:
        rows, h = case["rows"], case["hidden"]
        if op == "embed_gather":
            V, A = TABLE_ROWS, AUDIO_ROWS
            o["table"], o["audio"] = _rows16(g, V, h), _rows16(g, A, h)
            pat = {"mixed": [V - 1, -A, 0, -1, V - 1, 3, -2, 0, -A], "tokens": [V - 1, 0, 4, 4, 0, 7, V - 1, 1, 2],
                   "audio": [-1, -A, -3, -3, -1, -2, -A, -5, -4]}[case["idx"]]
            o["src"] = torch.tensor(pat[:rows], dtype=torch.int32)
            if case["idx"] == "tokens":
                o["audio"] = None
        elif op == "gather_rows":
            o["x"] = _rows16(g, SRC_ROWS, h)
            o["src"] = torch.tensor([6, 0, 6, 3, 0, 5, 1, 6, 2][:rows], dtype=torch.int32)       # duplicates
        else:
            o["x"] = _rows16(g, rows, h)
            o["out_rows"] = R = rows + 3                                                      # a strict subset is written
            idx = [R - 1 - i for i in range(rows)]
            if rows > 1:
                idx[0], idx[1] = idx[1], idx[0]
            o["src"] = torch.tensor(idx, dtype=torch.int32)
    elif op == "target_rows":
        B, S, pat = case["B"], case["S"], case["labels"]
        lab = torch.randint(0, 1000, (B, S), generator=g)
        if pat == "prefix":                                  # -100 prefixes; sequence 0 has the longest, so the first POSITION
            pre = torch.randint(0, max(1, S // 2), (B,), generator=g)       # with a target is not in the first rows
            pre[0] = int(pre.max()) + 1 if B > 1 else pre[0]
            for b in range(B):
                lab[b, :int(pre[b])] = -100
            if S > 8:
                lab[B - 1, S // 2:S // 2 + 3] = -100
        elif pat == "none":
            lab[:] = -100
        elif pat == "first":
            lab[:, 1:] = -100
        elif pat == "last":
            lab[:, :S - 1] = -100
        elif pat == "old":                                   # the labels of test_gpu_ops.py::test_target_rows_and_scatter
            lab[:, :9] = -100
            lab[2, 20:25] = -100
            lab[4] = -100
        else:
            assert pat == "all"
        o["lab_in"] = lab
    elif op == "mask_tokens":
        rows, n, cols, ld = case["rows"], case["n"], case["cols"], case["ld"]
        o["x"] = _bits16(g, rows * ld)
        sp = [cols - 1, -1, cols, ld - 1, ld + 3, 17, 17, 0, 2 * ld + 5]
        ids = torch.randint(0, cols, (n,), generator=g, dtype=torch.int32)
        k = min(n, len(sp))
        ids[:k] = torch.tensor(sp[:k], dtype=torch.int32)
        o["ids"] = ids
        o["x"][int(ids[0])] = _i16([0x7FC0])[0]              # a masked position that holds a NaN beforehand (ids[0] = cols - 1)
    elif op == "colsum":
        rows, cols, ld, off = case["rows"], case["cols"], case["ld"], case["off"]
        n = off + rows * ld
        if case["data"] == "int":
            xv = torch.randint(-8, 9, (n,), generator=g).float()
            prev = torch.randint(-50, 51, (cols,), generator=g).float()
        else:
            xv = torch.randn(n, generator=g)
            prev = 3 * torch.randn(cols, generator=g)
        o["xbuf"] = bf16_bits(xv)                             # the whole buffer; the operand is the view from `off`
        o["prev"] = prev
    elif op == "transpose":
        rows, cols, ld_in = case["rows"], case["cols"], case["ld_in"]
        o["off"] = case.get("off", 0)
        if case["f32"]:
            x = torch.randn(rows, ld_in, generator=g)
            sp = _f32_bits(SPECIAL32)
            body = x[:, :cols].reshape(-1).clone()
            k = min(body.numel(), len(sp))
            body[:k] = sp[:k]
            x[:, :cols] = body.view(rows, cols)
            x[:, cols:] = float("nan")
        else:
            x = _rows16(g, rows, ld_in)
            x[:, cols:] = _i16([0x7FC0])[0]
        o["x"] = x
    elif op == "cast":
        x = torch.randn(case["n"], generator=g) * torch.exp2(torch.randint(-20, 20, (case["n"],), generator=g).float())
        sp = _f32_bits(SPECIAL32)
        k = min(case["n"], len(sp))
        x[:k] = sp[:k]
        if case["n"] > 2 * len(sp):
            x[-len(sp):] = sp                                 # and in the last vectors (the grid's tail)
        o["x"] = x
    elif op == "add":
        n = case["n"]
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
        # a tie that rounds to even downwards, one that rounds upwards, a cancellation to +0, 2^24 + 1
        a[:4] = torch.tensor([1.0, 1.0 + 2.0 ** -23, 0.3, 16777216.0])
        b[:4] = torch.tensor([2.0 ** -24, 2.0 ** -24, -0.3, 1.0])
        if n > 8:
            a[-4:], b[-4:] = a[:4].clone(), b[:4].clone()
            b[n // 2] = -a[n // 2]
        o["a"], o["b"] = a, b
    else:
        raise KeyError(op)
    return o


def fresh(op, o):
    """every buffer the kernel writes, before the call (see the module docstring)"""
    if op in MOVERS:
        return {"out": _buf((o["out_rows"] if op == "scatter_rows" else o["rows"]) * o["hidden"], torch.int16)}
    if op == "target_rows":
        M = o["B"] * o["S"]
        return {"idx": _buf(M, torch.int32), "lab": _buf(M + 2, torch.int64), "count": _buf(2, torch.int32)}
    if op == "mask_tokens":
        b = _buf(o["rows"] * o["ld"], torch.int16)
        b[:o["x"].numel()] = o["x"]
        return {"x": b}
    if op == "colsum":
        b = _buf(o["cols"], torch.float32)
        if o["accumulate"]:
            b[:o["cols"]] = o["prev"]
        return {"out": b}
    if op == "transpose":
        return {"out": _buf(o["off"] + (o["cols"] + 2) * o["ld_out"], torch.int16)}
    if op == "cast":
        return {"y": _buf(o["n"], torch.int16)}
    if op == "add":
        b = _buf(o["n"], torch.float32)
        b[:o["n"]] = o["a"]
        return {"y": b}
    raise KeyError(op)


# ------------------------------------------------------------------------------------------------------------ references
def reference(op, o):
    """the buffers of fresh() as they must be after the call, written the obvious way"""
    bufs = fresh(op, o)
    if op in MOVERS:
        h, out = o["hidden"], bufs["out"]
        view = out[:out.numel() - GUARD].view(-1, h)
        for r in range(o["rows"]):
            s = int(o["src"][r])
            if op == "embed_gather":
                view[r] = o["table"][s] if s >= 0 else o["audio"][-(s + 1)]
            elif op == "gather_rows":
                view[r] = o["x"][s]
            else:
                view[s] = o["x"][r]
    elif op == "target_rows":
        B, S, lab = o["B"], o["S"], o["lab_in"]
        hits = [(b, s) for b in range(B) for s in range(S - 1) if int(lab[b, s + 1]) != -100]
        n = len(hits)
        bufs["count"][0], bufs["count"][1] = n, min([s for _, s in hits], default=S)
        bufs["lab"][0] = bufs["lab"][1 + n] = -100
        for i, (b, s) in enumerate(hits):
            bufs["idx"][i] = s * B + b if o["s_major"] else b * S + s
            bufs["lab"][1 + i] = lab[b, s + 1]
    elif op == "mask_tokens":
        view = bufs["x"][:o["rows"] * o["ld"]].view(o["rows"], o["ld"])
        for c in o["ids"].tolist():
            if 0 <= c < o["cols"]:
                view[:, c] = _i16([0xFF80])[0]
    elif op == "colsum":
        total = colsum_exact(o)
        bufs["out"][:o["cols"]] = (total + (o["prev"].double() if o["accumulate"] else 0)).float()
    elif op == "transpose":
        rows, cols, ld_out, off = o["rows"], o["cols"], o["ld_out"], o["off"]
        view = bufs["out"][off:off + cols * ld_out].view(cols, ld_out)
        src = o["x"][:, :cols]
        view[:, :rows] = (bf16_bits(src) if o["f32"] else src).T
        view[:, rows:] = 0
    elif op == "cast":
        bufs["y"][:o["n"]] = bf16_bits(o["x"])
    elif op == "add":
        bufs["y"][:o["n"]] = o["a"] + o["b"]
    return bufs


def colsum_x(o):
    """the [rows, cols] fp32 values of the operand"""
    rows, cols, ld, off = o["rows"], o["cols"], o["ld"], o["off"]
    return bits_f32(o["xbuf"][off:off + rows * ld].view(rows, ld)[:, :cols])


def colsum_exact(o):
    """float64 column sums (exact for data = int: computed in int64)"""
    x = colsum_x(o)
    return x.to(torch.int64).sum(0).double() if o["data"] == "int" else x.double().sum(0)


def colsum_chain(rows, cols):
    """L of the module docstring"""
    nr = colsum_splits(rows, cols)
    return -(-rows // nr) + -(-nr // 64) + 8


def _reduce_walk(grp, nblk, lim=48, tail=True, late=False):
    """partial rows wave group `grp` of reduce_partials_k adds -> (rows of a0, a1, a2, a3)"""
    acc, b = ([], [], [], []), grp
    while b + lim < nblk:
        for j in range(4):
            acc[j].append(b + 16 * j)
        b += 64
    if tail:
        b += 16 if late else 0
        while b < nblk:
            acc[0].append(b)
            b += 16
    return acc


def colsum_roundings(rows, cols):
    """roundings on the longest chain of a column sum, by walking the loops (an addition onto a zero is exact)"""
    nr = colsum_splits(rows, cols)
    deepest = max(len(_reduce_walk(g, nr)[0]) for g in range(16))
    return (-(-rows // nr) - 1) + max(deepest - 1, 0) + 2 + 2 + 3


def colsum_bound(o, out):
    """per-column bound of the random-data rule for the result `out` (float64)"""
    L = colsum_chain(o["rows"], o["cols"])
    b = (L * F / (1 - L * F)) * colsum_x(o).double().abs().sum(0)
    if o["accumulate"]:
        b = b + 0.5 * torch.exp2(torch.floor(torch.log2(out.double().abs().clamp_min(2.0 ** -126))) - 23)
    return b


def colsum_ratio(o, ref, got):
    """max over columns of |out - fp64| / bound for data = randn"""
    cols = o["cols"]
    exact = colsum_exact(o) + (o["prev"].double() if o["accumulate"] else 0)
    err = (got["out"][:cols].double() - exact).abs()
    ratio = err / colsum_bound(o, got["out"][:cols])             # no error is inside a bound of 0 (a column of zeros)
    return float(torch.where(err == 0, torch.zeros_like(err), ratio).max())


# ------------------------------------------------------------------------------------------------------------ comparison
def _where(bad):
    ix = bad.nonzero().flatten().tolist()
    return f"{len(ix)} elements, first at {ix[:8]}"


def mismatch(op, o, ref, got):
    """the comparison rule: None, or what differs"""
    for name, r in ref.items():
        g = got[name]
        if g.shape != r.shape or g.dtype != r.dtype:
            return f"{name}: shape / dtype {tuple(g.shape)} {g.dtype} against {tuple(r.shape)} {r.dtype}"
        if op == "colsum" and o["data"] == "randn":
            cols = o["cols"]
            if not torch.equal(g[cols:], r[cols:]):
                return f"{name}: guard overwritten"
            ratio = colsum_ratio(o, ref, got)
            if not ratio <= 1.0:
                return f"{name}: |err| / bound = {ratio:.3f}"
            continue
        if (op == "transpose" and o["f32"]) or op == "cast":
            nan = is_nan16(r)
            bad = torch.where(nan, ~is_nan16(g), g != r)
        else:
            bad = g != r
            if g.is_floating_point():                          # bits: -0.0 is not +0.0, and no NaN is expected
                bad = g.view(torch.int32) != r.view(torch.int32)
                if op == "colsum":
                    bad = g != r                               # an integer sum: the value (a zero of either sign)
        if bool(bad.any()):
            return f"{name}: {_where(bad)} (size {g.numel()}, guard from {g.numel() - GUARD})"
    return None


# ------------------------------------------------------------------------------------------------------------ emulations
def _put(buf, at, cols, vals):
    """buf[at + cols] = vals; what falls past the buffer is dropped"""
    pos = at + cols
    ok = pos < buf.numel()
    buf[pos[ok]] = vals[ok]


def _lane_cols(h, stride, skip_last):
    starts = [c for lane in range(64) for c in range(lane * 8, h, stride) if not (skip_last and c == h - 8)]
    return (torch.tensor(starts, dtype=torch.long)[:, None] + torch.arange(8)).reshape(-1)


def _emulate_mover(op, o, mut):
    rows, h, out = o["rows"], o["hidden"], fresh(op, o)["out"]
    stride = {"lane_stride_256": 256, "lane_stride_1024": 1024}.get(mut, 512)
    cols = _lane_cols(h, stride, mut == "last_chunk_skipped")
    zero = torch.zeros(h, dtype=torch.int16)
    nblk = (rows + 3) // 4
    for blk in range(nblk):
        for wave in range(4):
            row = blk * 4 + wave
            if row >= rows and not (mut == "no_row_test" and blk == nblk - 1):
                continue
            s = int(o["src"][row]) if row < rows else 0
            if op == "embed_gather":
                if s >= 0:
                    src = o["table"][s]
                else:
                    a = -s if mut == "audio_minus_s" else -(s + 1)
                    src = o["audio"][a] if a < o["audio"].shape[0] else zero
                at = row * h
            elif op == "gather_rows":
                src, at = o["x"][s], row * h
            else:
                src = o["x"][row] if row < rows else zero
                at = (row if mut == "scatter_to_row" else s) * h
            _put(out, at, cols, src[cols])
    return {"out": out}


def _emulate_target_rows(o, mut):
    B, S = o["B"], o["S"]
    M = B * S
    labels = o["lab_in"].reshape(-1).tolist() + [-100]
    bufs = fresh("target_rows", o)
    idx, lab, count = bufs["idx"], bufs["lab"], bufs["count"]
    per = M // 1024 if mut == "per_floor" else (M + 1023) // 1024

    def target(m):
        return ((m % S) + 1 < S or mut == "no_shift_guard") and labels[m + 1] != -100

    part, first = [0] * 1024, [S] * 1024
    for tid in range(1024):
        for m in range(tid * per, min(M, tid * per + per)):
            if target(m):
                part[tid] += 1
                first[tid] = min(first[tid], m if mut == "first_from_row" else m % S)
    run, fmin = 0, S
    for i in range(1024):
        part[i], run, fmin = run, run + part[i], min(fmin, first[i])
    count[0], count[1] = run, fmin
    lab[0] = -100
    if mut != "no_trailing_label":
        lab[1 + run] = -100
    for tid in range(1024):
        pos = part[tid]
        for m in range(tid * per, min(M, tid * per + per)):
            if target(m):
                if o["s_major"]:
                    idx[pos] = (m % B) * S + m // B if mut == "s_major_swapped" else (m % S) * B + m // S
                else:
                    idx[pos] = m
                lab[1 + pos] = labels[m + 1]
                pos += 1
    return bufs


def _emulate_mask_tokens(o, mut):
    rows, n, cols, ld = o["rows"], o["n"], o["cols"], o["ld"]
    x = fresh("mask_tokens", o)["x"]
    ids = torch.full((max(n, rows),), -1, dtype=torch.long)
    ids[:n] = o["ids"]
    i = torch.arange(rows * n)
    r, j = (i % n, i // n) if mut == "mask_div_mod_swapped" else (i // n, i % n)
    c = ids[j]
    ok = (c >= 0) & (c < (ld if mut == "mask_bound_ld" else cols))
    at = (r * ld + c)[ok]
    x[at[at < x.numel()]] = _i16([0x7F80 if mut == "mask_plus_inf" else 0xFF80])[0]
    return {"x": x}


def colsum_vector_width(o, mut=None):
    ok8 = o["cols"] % 8 == 0 or (mut == "v8_on_4" and o["cols"] % 8 == 4)
    return 8 if ok8 and o["ld"] % 8 == 0 and o["off"] % 8 == 0 else 4


def _emulate_colsum(o, mut):
    rows, cols, ld, off = o["rows"], o["cols"], o["ld"], o["off"]
    nr, V = colsum_splits(rows, cols), colsum_vector_width(o, mut)
    width = _up(cols, V)                                        # the last thread's vector may reach past `cols`
    flat = torch.cat([bits_f32(o["xbuf"][off:]), torch.zeros(8)])
    x = flat.as_strided((rows, width), (ld, 1))
    s = torch.zeros(nr, width)
    for t in range(-(-rows // nr)):                             # thread (r0, c) adds rows r0, r0 + nr, ... in order
        k = min(nr, rows - t * nr)
        s[:k] = s[:k] + x[t * nr:t * nr + k]
    ws = torch.zeros(nr * cols + 8)
    ws[:nr * cols] = s[:, :cols].reshape(-1)
    for r0 in range(nr):                                        # only under v8_on_4: the spill into the next partial row
        ws[r0 * cols + cols:r0 * cols + width] = s[r0, cols:]
    part = ws[:nr * cols].view(nr, cols)
    nblk = nr - 1 if mut == "last_partial_dropped" else nr
    total = torch.zeros(cols)
    for blk in range((cols + 63) // 64):                        # reduce_partials_k: 64 columns per block
        c = slice(blk * 64, min(cols, blk * 64 + 64))
        comb = []
        for grp in range(16):
            walk = _reduce_walk(grp, nblk, lim=64 if mut == "reduce_64_no_tail" else 48, tail=mut != "reduce_64_no_tail",
                                late=mut == "reduce_tail_late")
            a = [torch.zeros(c.stop - c.start) for _ in range(4)]
            for step in range(max(len(w) for w in walk)):
                for j in range(4):
                    if step < len(walk[j]):
                        a[j] = a[j] + part[walk[j][step], c]
            comb.append((a[0] + a[1]) + (a[2] + a[3]))
        sm = torch.zeros(c.stop - c.start)
        for g in range(0, 16, 4):
            sm = sm + ((comb[g] + comb[g + 1]) + (comb[g + 2] + comb[g + 3]))
        total[c] = sm
    out = fresh("colsum", o)["out"]
    out[:cols] = out[:cols] + total if o["accumulate"] and mut != "accumulate_ignored" else total
    return {"out": out}


def transpose_is_vector(o):
    return o["cols"] % 8 == 0 and o["ld_in"] % 8 == 0 and o["ld_out"] % 8 == 0 and o["off"] % 8 == 0


def _emulate_transpose(o, mut):
    rows, cols, ld_out, off = o["rows"], o["cols"], o["ld_out"], o["off"]
    out = fresh("transpose", o)["out"]
    view = out[off:off + cols * ld_out].view(cols, ld_out)
    if o["f32"]:
        bits = (o["x"].view(torch.int32) >> 16).to(torch.int16) if mut == "f32_truncated" else bf16_bits(o["x"])
    else:
        bits = o["x"]
    vec = transpose_is_vector(o)
    for by in range(((rows if mut == "no_tail_tiles" else ld_out) + 63) // 64):
        for bx in range((cols + 63) // 64):
            r0, c0 = by * 64, bx * 64
            rr, cc = max(0, min(64, rows - r0)), min(64, cols - c0)
            tile = torch.zeros(64, 64, dtype=torch.int16)
            tile[:rr, :cc] = bits[r0:r0 + rr, c0:c0 + cc]
            if vec:
                for rc in range(8):
                    if r0 + rc * 8 < (rows if mut == "vec_tail_rows" else ld_out):
                        view[c0:c0 + cc, r0 + rc * 8:r0 + rc * 8 + 8] = tile[rc * 8:rc * 8 + 8, :cc].T
            else:
                k = min(64, ld_out - r0)
                view[c0:c0 + cc, r0:r0 + k] = tile[:k, :cc].T
    return {"out": out}


def _emulate_cast(o, mut):
    y = fresh("cast", o)["y"]
    for i in range(o["n"] // 8):
        v = o["x"][i * 8:i * 8 + 8]
        y[i * 8:i * 8 + 8] = (v.view(torch.int32) >> 16).to(torch.int16) if mut == "f32_truncated" else bf16_bits(v)
    return {"y": y}


def _emulate_add(o, mut):
    y = fresh("add", o)["y"]
    for i in range(o["n"] // 4):
        y[i * 4:i * 4 + 4] = y[i * 4:i * 4 + 4] + o["b"][i * 4:i * 4 + 4]
    return {"y": y}


def emulate(op, o, mutation=None):
    """the buffers of fresh() after a run partitioned the way the kernel partitions it, optionally with one mutation"""
    assert mutation is None or op in MUTANTS[mutation][0], (op, mutation)
    if op in MOVERS:
        return _emulate_mover(op, o, mutation)
    return {"target_rows": _emulate_target_rows, "mask_tokens": _emulate_mask_tokens, "colsum": _emulate_colsum,
            "transpose": _emulate_transpose, "cast": _emulate_cast, "add": _emulate_add}[op](o, mutation)
