"""Constructed inputs for the 4-bit activation quantiser, on which the right codes and scales are known EXACTLY, and the bit-for-bit comparison the GPU tests
use (tests/test_gpu_quantiser_profiles.py launches them, tests/test_quantiser_profiles.py checks their preconditions and the comparison's teeth on the CPU).

The quantiser exists five times (quantize_kernel, quantize_kernel_v2, the GELU_QUANT epilogue of the W4A4 GEMM, the fused output quantiser of attention_kernel
and of attention_kernel64 / the split low-rank path).  None rounds with rint and a clamp: each hands ``x_hat * (1 / scale)`` to the FP6 e2m3 converter, and the
codes are right only while code / 8 stays in the uniformly spaced part of e2m3, the converter rounds to nearest even and |x_hat / scale| needs no clamp.
``helpers.checked_codes`` cannot see a site that breaks one of these: at a tie the approximation envelope holds both neighbours, and 1e-3 of the scales may
differ.  Here every step is an exactly rounded IEEE operation (or exact: scales that are powers of two), so the expectation is ``oracle.quantize_rows`` -- the
IEEE oracle, never the envelope -- and the comparison is equality.

Everything is numpy: float32 carriers of values that are exactly representable in the 16-bit type.
"""

import numpy as np

from oracle import svdq_oracle as O

F32 = np.float32
DTYPES = ("bf16", "fp16")
GROUP = O.GROUP
QMAX = {False: 7, True: 15}

# exponents k of the grids (amax = 7 * 2^k signed, 15 * 2^k unsigned).  The largest k with a finite amax: bf16 7 * 2^125 = 1.75 * 2^127, 15 * 2^124; fp16
# 7 * 2^13 = 57344, 15 * 2^12 = 61440.  fp16 -20 and -24: amax is an fp16 subnormal (at -24 the ties are below the format's last bit and drop out; the codes stay).
# bf16 -120: the scale 2^-120 and its reciprocal 2^120 are both normal fp32 numbers.
GRID_K = {("bf16", False): (-120, -3, 0, 5, 125), ("bf16", True): (-120, -3, 0, 5, 124),
          ("fp16", False): (-24, -20, -3, 0, 5, 13), ("fp16", True): (-24, -20, -3, 0, 5, 12)}
GELU_STEP = {"bf16": 128.0, "fp16": 1024.0}  # gelu_grid_bias: the 16-bit add of 0.171875 rounds back to every code value and tie of the grid at this step


def is16(x, dtype) -> np.ndarray:
    """elementwise: finite and exactly representable in ``dtype``"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.isfinite(x) & (O.round16(x.astype(F32), dtype).astype(np.float64) == x)


def neighbours16(v, dtype):
    """the 16-bit values just below and just above each finite ``v`` (exactly representable), by the format's own bit patterns"""
    v = np.asarray(v, dtype=F32)
    b = O.to_bits16(v, dtype).astype(np.int32)
    mag, neg = b & 0x7FFF, (b & 0x8000) != 0
    up = np.where(neg, np.where(mag == 0, 1, (mag - 1) | 0x8000), mag + 1)       # towards +inf (-0 -> smallest positive)
    dn = np.where(neg, (mag + 1) | 0x8000, np.where(mag == 0, 0x8001, mag - 1))  # towards -inf (+0 -> smallest negative)
    return O.from_bits16(dn.astype(np.uint16), dtype), O.from_bits16(up.astype(np.uint16), dtype)


def positive_finite16(dtype) -> np.ndarray:
    """every positive finite value of the format, ascending: 32639 (bf16) / 31743 (fp16)"""
    top = 0x7F7F if dtype == "bf16" else 0x7BFF
    return O.from_bits16(np.arange(1, top + 1, dtype=np.uint16), dtype)


def expected(x: np.ndarray, dtype: str, unsigned: bool = False):
    """The IEEE oracle on an already smoothed 16-bit matrix [M, K] -> (codes int8 [M, K], scale bit patterns uint16 [K / 64, M])"""
    q, s = O.quantize_rows(np.ascontiguousarray(x, dtype=F32), dtype, unsigned)
    return q, O.to_bits16(s, dtype)


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# the builders
# ----------------------------------------------------------------------------------------------------------------------------------------------------------
def code_grid(dtype: str, unsigned: bool, k: int) -> dict:
    """One 64-channel group with amax = 7 * 2^k (15 * 2^k unsigned).  In fp32 7 * fl(1/7) == 1 and 15 * fl(1/15) == 1 (asserted), so the oracle's scale is exactly
    2^k, its reciprocal is exact and x * rscale is exact: every code value n * 2^k, every tie (n + 0.5) * 2^k, the 16-bit neighbours of each tie on both
    sides, +0 and -0 (unsigned: no negative number; -0 stays).  What the format cannot hold at this k (ties of a subnormal grid) drops out; the code values
    never do.  -> x [64], kind [64] ('code' | 'tie' | 'near' | 'zero' | 'fill'), n [64] (x / 2^k), codes int8 [64], scale_bits (uint16), k"""
    qmax = QMAX[unsigned]
    step = np.float64(2.0) ** k
    codes_n = np.arange(0 if unsigned else -qmax, qmax + 1, dtype=np.float64)
    ties_n = np.arange(0.5 if unsigned else -qmax + 0.5, qmax, 1.0)
    vals, kinds = list(codes_n * step), ["code"] * len(codes_n)
    assert is16(vals, dtype).all(), (dtype, k, "a code value is not representable")
    ties = [t for t in ties_n * step if is16(t, dtype)]
    vals += ties
    kinds += ["tie"] * len(ties)
    if ties:
        dn, up = neighbours16(np.array(ties, dtype=F32), dtype)
        seen = set(vals)
        for v in np.concatenate([dn, up]).astype(np.float64):
            if v not in seen and abs(v) <= qmax * step:
                seen.add(v)
                vals.append(v)
                kinds.append("near")
    x = np.zeros(GROUP, dtype=F32)
    kind = np.array(["fill"] * GROUP, dtype=object)
    assert len(vals) + 1 <= GROUP, len(vals)
    order = np.random.default_rng(1000 + k + 7 * unsigned).permutation(GROUP)  # where a value sits in the group must not matter: scatter them
    x[order[:len(vals)]] = np.array(vals, dtype=np.float64).astype(F32)
    kind[order[:len(vals)]] = kinds
    x[order[len(vals)]] = F32(-0.0)
    kind[order[len(vals)]] = "zero"
    assert is16(x, dtype).all()
    q, s = expected(x[None, :], dtype, unsigned)
    # preconditions: the scale is the power of two, so every product x * (1 / scale) is exact and the ties ARE ties
    rq = F32(1.0) / F32(qmax)
    assert F32(qmax) * rq == F32(1.0), "7 * fl(1/7) and 15 * fl(1/15) are exactly 1 in fp32"
    assert (F32(np.abs(x).max()) * rq).astype(F32) == F32(step) and O.from_bits16(s, dtype)[0, 0] == F32(step), (dtype, unsigned, k)
    n = x.astype(np.float64) / step
    even = 2.0 * np.round(n[kind == "tie"] / 2.0)          # the even neighbour of n + 0.5
    assert np.array_equal(q[0][kind == "tie"], even.astype(np.int8)) and np.array_equal(q[0][kind == "code"], n[kind == "code"].astype(np.int8))
    return {"x": x, "kind": kind, "n": n, "codes": q[0], "scale_bits": s[0, 0], "k": k}


def grid_rows(dtype: str, unsigned: bool, K: int, rows: int, ks=None) -> np.ndarray:
    """[rows, K]: the code grids of GRID_K (or of the exponents ``ks``), one exponent per row in turn, the group's channels rotated from group to group and row
    to row so that every value visits many lane / register positions"""
    ks = GRID_K[(dtype, unsigned)] if ks is None else ks
    x = np.zeros((rows, K), dtype=F32)
    for m in range(rows):
        g0 = code_grid(dtype, unsigned, ks[m % len(ks)])["x"]
        for g in range(K // GROUP):
            x[m, g * GROUP:(g + 1) * GROUP] = np.roll(g0, 5 * m + 17 * g)
    return x


def max_position_rows(dtype: str) -> np.ndarray:
    """[128, 128]: row i has its single largest magnitude, 7, at channel i (negative for odd i); the other 64-channel group of the row has its own maximum,
    3.5, at channel (i + 64) % 128 (negative for even i).  Every other channel holds a small non-zero value n / 2, n in +-{1, 2, 3}: on the grid of both groups
    (scale 1: codes and ties; scale 1/2: codes).  Walks the lane-local maximum and the one ``lane ^ 32`` exchange through every position of both groups."""
    i = np.arange(128)[:, None]
    c = np.arange(128)[None, :]
    n = (3 * i + 5 * c) % 3 + 1
    x = (np.where((i + c) % 2 == 0, 1.0, -1.0) * n / 2.0).astype(F32)
    x[np.arange(128), np.arange(128)] = np.where(np.arange(128) % 2, -7.0, 7.0)
    x[np.arange(128), (np.arange(128) + 64) % 128] = np.where(np.arange(128) % 2, 3.5, -3.5)
    assert is16(x, dtype).all() and (x != 0).all()
    a = np.abs(x)
    assert (a.argmax(axis=1) == np.arange(128)).all() and ((a == 7.0).sum(axis=1) == 1).all()
    _, s = expected(x, dtype)
    sc = O.from_bits16(s, dtype)                          # [2, 128]
    assert set(np.unique(sc)) == {F32(0.5), F32(1.0)} and (sc[0, :64] == 1).all() and (sc[1, 64:] == 1).all()
    return x


def max_position_matrix(dtype: str, M: int, K: int) -> np.ndarray:
    """[M, K] from max_position_rows: chunk c of row m is builder row (m + 51 c) % 128 (M = 77, two chunks: rows 0 .. 76 and 51 .. 127 -- every position)"""
    base = max_position_rows(dtype)
    return np.concatenate([base[(np.arange(M) + 51 * c) % 128] for c in range(K // 128)], axis=1)


def amax_sweep(dtype: str, unsigned: bool = False, subsample=None) -> dict:
    """One group per positive finite 16-bit value ``a`` used as amax: a, -a, the 16-bit roundings of a * j / 14 (j = 0 .. 14) with alternating signs, zeros
    (unsigned: magnitudes only).  ``subsample`` = n: every exponent with four mantissa patterns (all zeros, all ones, 1010.., 0101..), filled to n values
    with evenly spaced bit patterns.  The domain of bit-equality is every ``a`` whose fp32 scale ``a * fl(1/7)`` is a NORMAL number: its reciprocal is then
    finite and no denormal mode matters; the others are counted from the oracle and returned, not hard-coded.
    -> a [n], x [n, 64], in_domain bool [n], codes int8 [n, 64], scale_bits uint16 [n]"""
    a = positive_finite16(dtype)
    if subsample is not None:
        mant = 7 if dtype == "bf16" else 10
        bits = O.to_bits16(a, dtype).astype(np.int64)
        full = (1 << mant) - 1
        pats = {0, full, 0x2AAAAAAA & full, 0x15555555 & full}
        keep = np.isin(bits & full, list(pats))
        extra = np.zeros(len(a), dtype=bool)
        if keep.sum() < subsample:
            extra[np.linspace(0, len(a) - 1, subsample - int(keep.sum()) + 1).astype(np.int64)] = True
        a = a[keep | extra]
        assert len(a) <= subsample, (len(a), subsample)
    n = len(a)
    x = np.zeros((n, GROUP), dtype=F32)
    j = np.arange(15)
    with np.errstate(under="ignore"):
        frac = O.round16((a.astype(np.float64)[:, None] * j[None, :] / 14.0).astype(F32), dtype)
    sign = F32(1.0) if unsigned else np.where(j % 2 == 0, F32(1.0), F32(-1.0))[None, :]
    # scattered over both lane halves of the group (channels 4h .. 4h + 3 of every 8 belong to lane half h)
    pos = (np.arange(17) * 11 + 3) % GROUP
    assert len(set(pos.tolist())) == 17
    x[:, pos[0]] = a
    x[:, pos[1]] = a if unsigned else -a
    x[:, pos[2:]] = frac * sign
    scale = (a * (F32(1.0) / F32(QMAX[unsigned]))).astype(F32)
    tiny = np.finfo(F32).tiny
    in_domain = np.isfinite(scale) & (scale >= tiny)
    q, s = expected(x.reshape(1, -1), dtype, unsigned)
    return {"a": a, "x": x, "in_domain": in_domain, "codes": q.reshape(n, GROUP), "scale_bits": s[:, 0]}


def sweep_matrix(groups: np.ndarray, M: int, K: int) -> np.ndarray:
    """[n, 64] groups -> [M, K], group t at row t % M, group slot t // M (consecutive amax values in consecutive ROWS: every row tile and K slice sees the whole
    range); the slots left over are zero groups"""
    G = K // GROUP
    n = len(groups)
    assert n <= M * G, (n, M, G)
    x = np.zeros((G, M, GROUP), dtype=F32)
    x.reshape(G * M, GROUP)[:n] = groups
    return np.ascontiguousarray(x.transpose(1, 0, 2)).reshape(M, K)


def sweep_slots(n: int, M: int):
    """(row, group) of sweep group t in sweep_matrix's layout"""
    t = np.arange(n)
    return t % M, t // M


def one_hot_rows(K: int, R: int, M: int, dtype: str) -> dict:
    """Row m is zero except a single 1.0 at channel (37 m) % K: lora_act[m, :] must be bit-equal to row (37 m) % K of lora_down -- exact in fp32 because every
    other addend is +0, and the value times 2^32 exactly in the Q31.32 format.  lora_down [K, R]: n / 64, n in -128 .. 127 (exact in both formats and times
    2^32).  -> x [M, K], lora_down [K, R], lora_act float32 [M, R], lora_act_q32 int64 [M, R]"""
    x = np.zeros((M, K), dtype=F32)
    ch = (37 * np.arange(M)) % K
    x[np.arange(M), ch] = 1.0
    D = (np.random.default_rng(K + R).integers(-128, 128, (K, R)) / 64.0).astype(F32)
    assert is16(D, dtype).all()
    la = D[ch]
    return {"x": x, "lora_down": D, "channel": ch, "lora_act": la, "lora_act_q32": np.round(la.astype(np.float64) * 2.0 ** 32).astype(np.int64)}


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# exact front ends: the input a launch reads so that the quantiser sees exactly ``x``
# ----------------------------------------------------------------------------------------------------------------------------------------------------------
def smooth_pow2(K: int, lo: int = -2, hi: int = 2) -> np.ndarray:
    """per-channel powers of two between 2^lo and 2^hi (1/4 .. 4), every value on both lane halves"""
    return (2.0 ** ((np.arange(K) * 7 // 4) % (hi - lo + 1) + lo)).astype(F32)


def presmoothed(x: np.ndarray, smooth: np.ndarray, dtype: str):
    """x * smooth where that is exact in the 16-bit type and divides back to x; a GROUP that holds an element for which it is not (the product overflows, or
    loses bits among the subnormals) is zeroed whole.  The division -- x * v_rcp_f32(smooth) or IEEE -- is exact for a power of two.
    -> (the input to feed [M, K], the x_hat the quantiser then sees [M, K], number of groups zeroed)"""
    M, K = x.shape
    s = smooth.astype(np.float64)[None, :]
    y = x.astype(np.float64) * s
    ok = is16(y, dtype) & (np.abs(y) >= np.finfo(F32).tiny) | (x == 0)
    okg = ok.reshape(M, K // GROUP, GROUP).all(axis=2)
    keep = np.repeat(okg, GROUP, axis=1)
    xin = np.where(keep, y, 0.0).astype(F32)
    xh = np.where(keep, x, F32(0.0)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        back = O.round16((xin / smooth.astype(F32)[None, :]).astype(F32), dtype)
    assert np.array_equal(O.to_bits16(back, dtype) & 0x7FFF, O.to_bits16(xh, dtype) & 0x7FFF) and np.array_equal(back, xh)
    return xin, xh, int((~okg).sum())


def ln_identity(M: int, K: int, x: np.ndarray, dtype: str):
    """LayerNorm front end that is the identity: ln_stats rows (mean, rstd) = (0, 1), mod_scale = 1, mod_shift = -0 (x + -0 == x for every x, +0 and -0
    included).  Asserts that oracle.ln_mod_ref returns ``x`` bit for bit.  -> (stats float32 [M, 2], mod_scale [K], mod_shift [K])"""
    stats = np.tile(np.array([[0.0, 1.0]], dtype=F32), (M, 1))
    scale, shift = np.ones(K, dtype=F32), np.full(K, -0.0, dtype=F32)
    got = O.ln_mod_ref(x, stats, scale, shift, dtype)
    assert np.array_equal(O.to_bits16(got, dtype), O.to_bits16(x, dtype)), "the LayerNorm front end is not the identity on this input"
    return stats, scale, shift


def glu_identity(x: np.ndarray, dtype: str) -> np.ndarray:
    """[M, 2K] (value, gate) pairs with every gate 32 and value = x / 32: exp2(-1.4427 * 32) vanishes against 1 in fp32, silu is the identity on the gate and
    value * 32 is exact.  Asserts with oracle.glu_pairs that the pairs give back ``x`` (values x / 32 cannot hold -- subnormal bits -- are refused)."""
    M, K = x.shape
    v = (x.astype(np.float64) / 32.0)
    assert is16(v, dtype).all(), "x / 32 is not exact in the 16-bit type"
    x2 = np.empty((M, 2 * K), dtype=F32)
    x2[:, 0::2], x2[:, 1::2] = v.astype(F32), F32(32.0)
    assert (F32(1.0) + np.exp2(F32(-1.4426950408889634) * F32(32.0)).astype(F32)) == F32(1.0)
    got = O.glu_pairs(x2, dtype)
    assert np.array_equal(got, x) and np.array_equal(np.signbit(got), np.signbit(x)), "fuse_glu front end is not the identity on this input"
    return x2


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# site 3: the GELU_QUANT epilogue
# ----------------------------------------------------------------------------------------------------------------------------------------------------------
def smooth_pow2_up(N: int) -> np.ndarray:
    """next_smooth for the epilogue: 1, 2, 4 per column.  (Below 1 the pre-activation grid value * smooth gets fine enough for the 16-bit add of 0.171875 to
    move it: the shift is added BEFORE the division, so the epilogue's exact grid needs smooth >= 1.)"""
    return smooth_pow2(N, 0, 2)


def gelu_grid_bias(dtype: str, N: int, next_smooth: np.ndarray | None = None) -> dict:
    """A bias [N] whose 64-column groups are the unsigned code grid at step S = GELU_STEP (times next_smooth, powers of two >= 1), the group's channels rotated
    from group to group.  With all-zero weight codes and no low-rank branch the GEMM's pre-activation is the bias itself; gelu returns x exactly for x >= 6
    (exp2 underflows against 1) and -0 for x <= -6 (it overflows), so entries that should read as zero are -S: they become 0.171875 after the shift, code 0.
    Asserts on the CPU that the oracle's epilogue reproduces the intended grid at every code value and tie, that its GELU envelope is degenerate where the
    format allows it (see ``envelope_open``) and the envelope of codes and scales everywhere.
    -> bias [N], next_smooth [N], codes int8 [N], scale_bits uint16 [N / 64], kind [N], envelope_open bool [N]"""
    S = GELU_STEP[dtype]
    k = int(np.log2(S))
    ns = np.ones(N, dtype=F32) if next_smooth is None else next_smooth.astype(F32)
    assert (ns >= 1).all() and is16(ns, dtype).all() and (np.log2(ns) % 1 == 0).all()
    g = code_grid(dtype, True, k)
    grid = np.concatenate([np.roll(g["x"], 9 * j) for j in range(N // GROUP)])
    kind = np.concatenate([np.roll(g["kind"], 9 * j) for j in range(N // GROUP)])
    zero = grid == 0                                     # code 0, -0 and the fill: -S, the GELU's -0
    pre = np.where(zero, -S, grid.astype(np.float64)) * ns
    assert is16(pre, dtype).all() and ((pre >= 6) | (pre <= -6)).all()
    bias = pre.astype(F32)
    # the oracle on a one-row launch: zero activation codes x zero weight codes, pre-activation = bias
    K = 64
    r = O.gemm_w4a4(np.zeros((1, K), dtype=np.int8), np.ones((1, 1), dtype=F32), np.zeros((N, K), dtype=np.int8), np.ones((1, N), dtype=F32), dtype=dtype,
                    bias=bias, fuse="gelu_quant", next_smooth=ns, envelope=True)
    want = np.where(zero, 0.0, grid)
    assert np.array_equal(r["g16"][0], np.where(zero, -0.0, bias)), "gelu is not the identity / -0 on the grid"
    sh = O.round16((r["g16"][0] + F32(O.GELU_SHIFT)).astype(F32), dtype)
    exact = (kind == "code") | (kind == "tie")
    assert np.array_equal(sh[exact & ~zero], bias[exact & ~zero]), f"the 16-bit add of the shift moves a grid value at step {S}"
    assert (sh[zero] == F32(O.GELU_SHIFT)).all()
    xh = O.round16((sh / ns).astype(F32), dtype)
    q, s = expected(xh[None, :], dtype, unsigned=True)
    assert np.array_equal(q, r["qout"]) and np.array_equal(s, O.to_bits16(r["oscales"], dtype))
    assert (O.from_bits16(s, dtype) == F32(S)).all(), "every group's scale is the step"
    n = want.astype(np.float64) / S
    assert np.array_equal(q[0][kind == "code"], n[kind == "code"].astype(np.int8))
    assert np.array_equal(q[0][kind == "tie"], (2.0 * np.round(n[kind == "tie"] / 2.0)).astype(np.int8)) and (q[0][zero] == 0).all()
    # The GELU envelope (gelu_tanh_envelope: tanh.approx at 2^-11 relative) is degenerate -- lower end == upper end == the value itself -- at every element
    # but two kinds, which no choice of S avoids: the -S entries (x * (1 - |tanh|) may be +-S 2^-12 instead of -0: still 0.171875 +- S 2^-12 after the shift,
    # far inside code 0) and, fp16 only, the two values at a change of the format's spacing: an exact power of two (x (1 - 2^-12) is the tie below x, where the
    # spacing halves: the lower end is one step below x) and the value just below one (its upper end is the power of two).  The kernel's own GELU is exact at
    # all of them (exp2 over- / underflows against 1).
    env = r["envelope"]
    assert np.array_equal(env["s_lo"], env["s_hi"]) and np.array_equal(O.to_bits16(env["s_lo"], dtype), s), "the epilogue's envelope of scales is not degenerate"
    open_ = r["g16_lo"][0] != r["g16_hi"][0]
    edge = open_ & ~zero
    assert dtype == "fp16" or not edge.any(), "bf16: the GELU envelope is open at an element that is not -S"
    dn, up = neighbours16(bias[edge], dtype)
    at_pow2 = np.frexp(bias[edge].astype(np.float64))[0] == 0.5
    below_pow2 = np.frexp(up.astype(np.float64))[0] == 0.5
    assert (at_pow2 | below_pow2).all(), "the GELU envelope is open at an element that is neither -S nor at a change of the fp16 spacing"
    lo_e, hi_e = r["g16_lo"][0][edge], r["g16_hi"][0][edge]  # never further than the neighbouring 16-bit value
    assert ((lo_e == dn) | (lo_e == bias[edge])).all() and ((hi_e == up) | (hi_e == bias[edge])).all()
    assert (np.abs(r["g16_lo"][0][zero]) + O.GELU_SHIFT < S / 4).all() and (np.abs(r["g16_hi"][0][zero]) + O.GELU_SHIFT < S / 4).all()
    assert np.array_equal(r["g16_lo"][0][~open_], r["g16"][0][~open_])
    return {"bias": bias, "next_smooth": ns, "codes": q[0], "scale_bits": s[:, 0], "kind": kind, "envelope_open": open_, "g16_lo": r["g16_lo"][0],
            "g16_hi": r["g16_hi"][0], "g16": r["g16"][0]}


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# the comparison
# ----------------------------------------------------------------------------------------------------------------------------------------------------------
def assert_exact(codes, scale_bits, want_codes, want_scale_bits, what: str, rows=None, mask=None):
    """codes [M, K] and scale bit patterns [K / 64, M] equal to the expectation, no envelope, no flip budget.  ``rows``: compare these rows only; ``mask``
    (bool [M, K / 64]): compare these groups only.  Names the first differing (row, group, channel)."""
    codes, want_codes = np.asarray(codes).astype(np.int16), np.asarray(want_codes).astype(np.int16)
    sb, wsb = np.asarray(scale_bits).astype(np.int32).T, np.asarray(want_scale_bits).astype(np.int32).T  # [M, G]
    M, K = want_codes.shape
    G = K // GROUP
    assert codes.shape == (M, K) and sb.shape == (M, G) and wsb.shape == (M, G), (what, codes.shape, sb.shape, want_codes.shape, wsb.shape)
    use = np.ones((M, G), dtype=bool) if mask is None else np.asarray(mask, dtype=bool).copy()
    if rows is not None:
        sel = np.zeros(M, dtype=bool)
        sel[rows] = True
        use &= sel[:, None]
    bad_c = (codes != want_codes).reshape(M, G, GROUP) & use[:, :, None]
    bad_s = (sb != wsb) & use
    if bad_s.any():
        m, g = np.argwhere(bad_s)[0]
        raise AssertionError(f"{what}: {int(bad_s.sum())} of {int(use.sum())} scales differ; first at (row {m}, group {g}): got bits 0x{sb[m, g]:04x}, "
                             f"the IEEE oracle 0x{wsb[m, g]:04x}")
    if bad_c.any():
        m, g, c = np.argwhere(bad_c)[0]
        raise AssertionError(f"{what}: {int(bad_c.sum())} of {int(use.sum()) * GROUP} codes differ; first at (row {m}, group {g}, channel {c}): got "
                             f"{codes[m, g * GROUP + c]}, the IEEE oracle {want_codes[m, g * GROUP + c]}")


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# subtly wrong quantisers (CPU only): what the comparison must catch
# ----------------------------------------------------------------------------------------------------------------------------------------------------------
def mutant_quantize_rows(xh: np.ndarray, dtype: str, unsigned: bool, how: str):
    """oracle.quantize_rows with one planted error: 'half-away' (ties away from zero), 'truncate' (towards zero), 'one-rounding' (the stored scale is ONE
    rounding of the exact product amax * fl(1/7) to 16 bits, not round16 of the fp32 product), 'clamp-8' (rounds half up: -amax can reach beyond the end)."""
    M, K = xh.shape
    G = K // GROUP
    xg = xh.reshape(M, G, GROUP).astype(F32)
    amax = np.fmax.reduce(np.abs(xg), axis=2, initial=F32(0))
    rq = F32(1.0) / F32(QMAX[unsigned])
    scale = (amax * rq).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        v = (xg * (F32(1.0) / scale).astype(F32)[:, :, None]).astype(F32)
    v = np.where(np.isnan(v), F32(0), v)
    if how == "half-away":
        q = np.sign(v) * np.floor(np.abs(v).astype(np.float64) + 0.5)   # (float64: |v| + 0.5 itself must not round)
    elif how == "truncate":
        q = np.trunc(v)
    else:
        q = np.rint(v)
    lo, hi = (0, 15) if unsigned else (-8, 7)
    q = np.clip(q, lo, hi).astype(np.int8).reshape(M, K)
    if how == "one-rounding":
        exact = amax.astype(np.float64) * np.float64(rq)
        s16 = exact.astype(np.float16).astype(F32) if dtype == "fp16" else _bf16_round64(exact)
    else:
        s16 = O.round16(scale, dtype)
    return q, O.to_bits16(s16.T.copy(), dtype)


def _bf16_round64(x64: np.ndarray) -> np.ndarray:
    """float64 -> nearest-even bf16 in ONE rounding (normal range), as float32"""
    m, e = np.frexp(x64)                                  # x = m 2^e, 0.5 <= |m| < 1
    r = np.ldexp(np.rint(np.ldexp(m, 8)), e - 8)          # 8 significant bits
    return np.where(x64 == 0, 0.0, r).astype(F32)
