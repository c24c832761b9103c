"""tests/quantiser_profiles.py on the CPU: the preconditions of every input tests/test_gpu_quantiser_profiles.py launches hold (scales are exact powers of two,
the front ends are the identity, fp16 excludes no amax value, the GELU envelope is degenerate where the format allows), and the comparison those tests use has
teeth: fed the codes of a quantiser that rounds ties away from zero, of one that truncates, and the scales of one that rounds the product once, it fails and
names the first differing (row, group, channel) -- so a subtly wrong kernel would be caught, shown without running a wrong kernel on a GPU.

What the builders computed (asserted below): amax values outside the pinned domain -- the fp32 scale amax * fl(1 / qmax) is subnormal -- fp16 0 signed / 0
unsigned, bf16 479 signed (the largest 8.19e-38) / 623 unsigned.  One-rounding scales: 186 of the 32639 bf16 amax values; NONE of the 31743 fp16 values -- for
every fp16 amax, rounding the exact product amax * fl(1/7) (or the exact quotient amax / 7) to fp16 once gives the bits of the two roundings, so in fp16 that
error is not an error on any input and no comparison can or need see it (asserted: ``test_one_rounding_of_the_scale_is_invisible_in_fp16``)."""

import re

import numpy as np
import pytest

from oracle import svdq_oracle as O
from tests import quantiser_profiles as P

DT = list(P.DTYPES)
F32 = np.float32


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("unsigned", [False, True], ids=["signed", "unsigned"])
def test_code_grids_have_power_of_two_scales_and_even_ties(dtype, unsigned):
    qmax = P.QMAX[unsigned]
    for k in P.GRID_K[(dtype, unsigned)]:
        g = P.code_grid(dtype, unsigned, k)                      # (asserts its own preconditions)
        assert O.from_bits16(np.array([g["scale_bits"]], dtype=np.uint16), dtype)[0] == F32(2.0) ** k
        assert (g["kind"] == "code").sum() == (16 if unsigned else 15) and g["codes"].max() == qmax and g["codes"].min() == (0 if unsigned else -qmax)
        tie = g["kind"] == "tie"
        assert (g["codes"][tie] % 2 == 0).all()
        # the products are exact: x * (1 / 2^k) in fp32 is the real quotient
        with np.errstate(over="ignore"):
            v = (g["x"] * (F32(1.0) / F32(2.0) ** k)).astype(F32)
        assert np.array_equal(v.astype(np.float64), g["n"])
        # the neighbours of a tie land on the two sides of it
        near = g["kind"] == "near"
        assert np.array_equal(g["codes"][near], np.clip(np.rint(g["n"][near]), 0 if unsigned else -8, qmax).astype(np.int8))
    full = [k for k in P.GRID_K[(dtype, unsigned)] if (P.code_grid(dtype, unsigned, k)["kind"] == "tie").sum() == (15 if unsigned else 14)]
    assert len(full) >= 4
    # the largest finite amax, and (fp16) a subnormal one
    top = P.code_grid(dtype, unsigned, max(P.GRID_K[(dtype, unsigned)]))["x"]
    assert P.is16(top, dtype).all() and not P.is16(top.astype(np.float64) * 2.0, dtype).all()
    if dtype == "fp16":
        assert qmax * 2.0 ** -20 < 2.0 ** -14 and -20 in full


def test_the_oracle_rounds_the_issues_ties_to_even():
    x = np.zeros((1, 64), dtype=F32)
    vals = np.array([7, -7, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, 4.5, 5.5, 6.5, -6.5]) * 2.0 ** -3
    x[0, :len(vals)] = vals
    assert P.expected(x, "bf16")[0][0, :len(vals)].tolist() == [7, -7, 0, 0, 2, -2, 2, -2, 4, 4, 6, 6, -6]
    x[:] = 0
    vals = np.array([15, .5, 1.5, 2.5, 7.5, 8.5, 13.5, 14.5]) * 2.0 ** -3
    x[0, :len(vals)] = vals
    assert P.expected(x, "fp16", True)[0][0, :len(vals)].tolist() == [15, 0, 2, 2, 8, 8, 14, 14]


@pytest.mark.parametrize("dtype", DT)
def test_max_position_rows_walk_both_groups(dtype):
    x = P.max_position_rows(dtype)
    assert x.shape == (128, 128)
    m = P.max_position_matrix(dtype, 77, 256)
    assert m.shape == (77, 256)
    pos = {int(np.abs(m[r, c * 128:(c + 1) * 128]).argmax()) for r in range(77) for c in range(2)}
    assert pos == set(range(128))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("unsigned", [False, True], ids=["signed", "unsigned"])
def test_amax_sweep_domain(dtype, unsigned):
    s = P.amax_sweep(dtype, unsigned)
    n = {"bf16": 32639, "fp16": 31743}[dtype]
    assert len(s["a"]) == n and n <= 512 * 64
    ex = ~s["in_domain"]
    scale = (s["a"] * (F32(1) / F32(P.QMAX[unsigned]))).astype(F32)
    assert np.array_equal(ex, (scale < np.finfo(F32).tiny)) and np.isfinite(F32(1) / scale[~ex]).all()
    if dtype == "fp16":
        assert ex.sum() == 0                                       # the precondition of the GPU sweep: fp16 excludes no amax value
    else:
        assert ex.sum() == (623 if unsigned else 479) and s["a"][ex].max() < (1.8e-37 if unsigned else 8.3e-38)
    # +-amax sit on the ends, never beyond
    dom = s["codes"][~ex]
    assert (dom.max(axis=1) == P.QMAX[unsigned]).all() and (dom.min(axis=1) == (0 if unsigned else -7)).all()
    x = P.sweep_matrix(s["x"], 512, 4096)
    rows, groups = P.sweep_slots(n, 512)
    assert np.array_equal(x.reshape(512, 64, 64)[rows, groups], s["x"])
    sub = P.amax_sweep(dtype, False, subsample=2048)
    bits = O.to_bits16(sub["a"], dtype).astype(np.int64)
    mant = 7 if dtype == "bf16" else 10
    assert len(sub["a"]) <= 2048 and len(np.unique(bits >> mant)) == (255 if dtype == "bf16" else 31)


@pytest.mark.parametrize("dtype", DT)
def test_exact_front_ends_are_the_identity(dtype):
    K, M = 256, 77
    for x in (P.grid_rows(dtype, False, K, M), P.max_position_matrix(dtype, M, K), P.one_hot_rows(K, 32, M, dtype)["x"]):
        sm = P.smooth_pow2(K)
        assert set(np.unique(sm)) == {0.25, 0.5, 1.0, 2.0, 4.0}
        xin, xh, zeroed = P.presmoothed(x, sm, dtype)
        q0, s0, _ = O.quantize_w4a4_act_fuse_lora(xin, sm, None, dtype, pad_size=1)
        q1, s1 = O.quantize_rows(xh, dtype, False)
        assert np.array_equal(q0, q1) and np.array_equal(s0, s1)
        assert zeroed < xh.shape[0] * K // 64 // 2 and np.array_equal(xh[xh != 0], x[xh != 0])
        P.ln_identity(M, K, xin, dtype)                           # (asserts oracle.ln_mod_ref returns its input bit for bit)
    ks = tuple(k for k in P.GRID_K[(dtype, False)] if P.is16(P.code_grid(dtype, False, k)["x"].astype(np.float64) / 32.0, dtype).all())
    assert len(ks) >= 4 and max(ks) == max(P.GRID_K[(dtype, False)])
    for x in (P.grid_rows(dtype, False, K, M, ks=ks), P.max_position_matrix(dtype, M, K)):
        for xin in (x, P.presmoothed(x, P.smooth_pow2(K), dtype)[0]):
            x2 = P.glu_identity(xin, dtype)                       # (asserts oracle.glu_pairs gives back xin)
            assert x2.shape == (M, 2 * K) and (x2[:, 1::2] == 32).all()


@pytest.mark.parametrize("dtype", DT)
def test_one_hot_rows_select_a_row_of_lora_down_exactly(dtype):
    for K, R, M in ((256, 32, 77), (256, 176, 300)):
        r = P.one_hot_rows(K, R, M, dtype)
        assert ((r["x"] != 0).sum(axis=1) == 1).all()
        got = O.lora_down_project(r["x"], r["lora_down"])
        assert got.dtype == F32 and np.array_equal(got, r["lora_act"]) and np.array_equal(r["lora_act"], r["lora_down"][(37 * np.arange(M)) % K])
        assert np.array_equal(r["lora_act_q32"].astype(np.float64) * 2.0 ** -32, r["lora_act"].astype(np.float64))
        # through power-of-two smoothing the projection reads the un-smoothed input: still one exact product per element
        xin, _, _ = P.presmoothed(r["x"], P.smooth_pow2(K), dtype)
        assert np.array_equal(O.lora_down_project(xin, r["lora_down"]).astype(np.float64), xin.astype(np.float64) @ r["lora_down"].astype(np.float64))


@pytest.mark.parametrize("dtype", DT)
def test_gelu_grid_bias_reproduces_the_grid_through_the_oracles_epilogue(dtype):
    for N, ns in ((256, None), (256, P.smooth_pow2_up(256)), (8192, P.smooth_pow2_up(8192))):
        r = P.gelu_grid_bias(dtype, N, ns)                        # (asserts gelu == identity / -0, the shift rounds back, the scale is S, ties to even)
        assert r["codes"].max() == 15 and r["codes"].min() == 0
        S = P.GELU_STEP[dtype]
        # the GELU envelope is degenerate at every element but the -S entries and, fp16, the values at a change of the format's spacing (gelu_grid_bias asserts which)
        open_ = r["envelope_open"]
        zero = r["bias"] < 0
        assert zero[open_].all() if dtype == "bf16" else (open_ & ~zero).sum() > 0
        closed = ~open_
        assert np.array_equal(r["g16_lo"][closed], r["g16_hi"][closed]) and closed.sum() > (0.7 if dtype == "fp16" else 0.9) * (~zero).sum()
        assert (O.from_bits16(r["scale_bits"], dtype) == S).all()


# ---- the comparison has teeth --------------------------------------------------------------------------------------------------------------------------
def _profile_inputs(dtype):
    """the stand-alone profiles of the GPU file as one [M, K] matrix each"""
    return {"grid": P.grid_rows(dtype, False, 256, 77), "max-position": P.max_position_matrix(dtype, 77, 256),
            "sweep": P.sweep_matrix(P.amax_sweep(dtype, False)["x"], 512, 4096)}


@pytest.mark.parametrize("dtype", DT)
def test_the_comparison_passes_the_oracle_and_names_the_first_difference(dtype):
    x = _profile_inputs(dtype)["grid"]
    q, s = P.expected(x, dtype)
    P.assert_exact(q, s, q, s, "oracle")
    q2 = q.copy()
    q2[5, 2 * 64 + 9] += 1
    q2[40, 3] -= 1
    with pytest.raises(AssertionError, match=r"2 of \d+ codes differ; first at \(row 5, group 2, channel 9\)"):
        P.assert_exact(q2, s, q, s, "planted")
    s2 = s.copy()
    s2[1, 7] ^= 1
    with pytest.raises(AssertionError, match=r"1 of \d+ scales differ; first at \(row 7, group 1\)"):
        P.assert_exact(q, s2, q, s, "planted")
    P.assert_exact(q2, s2, q, s, "masked", rows=np.array([0, 1, 2]))                # rows / mask restrict it
    mask = np.ones((77, 4), dtype=bool)
    mask[5, 2] = mask[40, 0] = mask[7, 1] = False
    P.assert_exact(q2, s2, q, s, "masked", mask=mask)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("how", ["half-away", "truncate"])
def test_the_comparison_catches_a_quantiser_that_rounds_wrongly(how, dtype):
    """round-half-away-from-zero differs from the oracle at ties ONLY (on the grids: every odd-below tie; nowhere on the walking maximum's non-tie channels);
    truncation nearly everywhere.  Both fail on the grid profile and on the full amax sweep, with the first (row, group, channel) named."""
    for name, x in _profile_inputs(dtype).items():
        q, s = P.expected(x, dtype)
        qm, sm = P.mutant_quantize_rows(x, dtype, False, how)
        assert np.array_equal(sm, s)
        diff = np.argwhere(qm != q)
        assert len(diff), (name, how)
        if how == "half-away":                                                      # it differs at exact ties and nowhere else
            amax = np.abs(x.reshape(x.shape[0], -1, 64)).max(axis=2, keepdims=True)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                v = (x.reshape(x.shape[0], -1, 64) * (F32(1) / (amax * (F32(1) / F32(7))).astype(F32)).astype(F32)).astype(F32).reshape(x.shape)
            assert (np.abs(v[qm != q]) % 1 == 0.5).all()
        m, c = diff[0]
        with pytest.raises(AssertionError) as e:
            P.assert_exact(qm, sm, q, s, f"{how} on {name}")
        assert re.search(rf"codes differ; first at \(row {m}, group {c // 64}, channel {c % 64}\)", str(e.value)), str(e.value)


def test_the_comparison_catches_a_scale_rounded_once():
    """bf16: 186 of the 32639 amax values give another scale when the exact product amax * fl(1/7) is rounded to 16 bits once instead of twice; the sweep
    holds every one of them and the comparison names the first."""
    x = _profile_inputs("bf16")["sweep"]
    q, s = P.expected(x, "bf16")
    qm, sm = P.mutant_quantize_rows(x, "bf16", False, "one-rounding")
    assert np.array_equal(qm, q) and (sm != s).sum() == 186
    g, m = np.argwhere(sm != s)[0]
    with pytest.raises(AssertionError, match=rf"186 of \d+ scales differ; first at \(row {m}, group {g}\)"):
        P.assert_exact(qm, sm, q, s, "one-rounding")


def test_one_rounding_of_the_scale_is_invisible_in_fp16():
    """For EVERY positive finite fp16 amax, one rounding of the exact product amax * fl(1/7) to fp16 -- and one rounding of the exact quotient amax / 7 --
    gives the bits of the two roundings (fp32 product, then fp16).  A kernel that folds the two into one is therefore not wrong on any fp16 input (signed
    or unsigned), and this is the whole input space of the scale: nothing is left for a GPU comparison to catch."""
    a = P.positive_finite16("fp16")
    for qmax in (7.0, 15.0):
        rq = F32(1) / F32(qmax)
        two = (a * rq).astype(F32).astype(np.float16)
        assert np.array_equal((a.astype(np.float64) * np.float64(rq)).astype(np.float16), two)
        assert np.array_equal((a.astype(np.float64) / qmax).astype(np.float16), two)
    x = _profile_inputs("fp16")["sweep"]
    _, s = P.expected(x, "fp16")
    assert np.array_equal(P.mutant_quantize_rows(x, "fp16", False, "one-rounding")[1], s)
