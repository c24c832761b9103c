"""What the oracle says the reference does at the numeric edges: fp16 saturation of EpilogueDefault, the group quantiser on +-inf / NaN,
GEMMs whose activation scales are infinite.  Hand-written cases; every expected value is derived here from the cited reference lines, not
from the function under test.  Warnings are errors in this file: non-finite numbers are ordinary data for the oracle."""

import numpy as np
import pytest

from oracle import svdq_oracle as O

pytestmark = pytest.mark.filterwarnings("error")

NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _same(a, b):
    """equal, NaN == NaN, and the sign of zero ignored"""
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32), equal_nan=True)


# ----------------------------------------------------------------------------- EpilogueDefault's clamp
def test_fp16_clamp_follows_the_reference_order():
    """gemm_base.cuh:692-693: v = __hmin(v, 65504); v = __hmax(v, -65504).  Both return the non-NaN operand:
    NaN -> hmin(NaN, 65504) = 65504 -> hmax(65504, -65504) = +65504 (the other order, max first, would give -65504)."""
    y = np.array([NAN, INF, -INF, 65504.0, -65504.0, 65472.0, -1.5, 0.0], np.float32)
    want = np.array([65504.0, 65504.0, -65504.0, 65504.0, -65504.0, 65472.0, -1.5, 0.0], np.float32)
    assert _same(O.clamp16_default(y, "fp16"), want)
    # bf16: `if constexpr (std::is_same_v<half_t, half>)` (:689) -- no clamp, values stored as they are
    assert _same(O.clamp16_default(y, "bf16"), y)


def _one_group_gemm(a_codes, ascale, w_codes, wscale, dtype, **kw):
    """M x 64 codes against N x 64 codes, one group"""
    qa = np.asarray(a_codes, np.int8)
    qw = np.asarray(w_codes, np.int8)
    asc = np.asarray(ascale, np.float32).reshape(1, -1)
    ws = np.asarray(wscale, np.float32).reshape(1, -1)
    return O.gemm_w4a4(qa, asc, qw, ws, dtype=dtype, **kw)["out"]


def _codes(first, n=64):
    c = np.zeros(n, np.int8)
    c[: len(first)] = first
    return c


def test_plain_and_silu_outputs_saturate_in_fp16_only():
    # row 0: 7 * 7 * (1024 * 4) = 200704 > 65504; row 1: the negative of it; row 2: 1 * 7 * 4096 = 28672 (exact in fp16); row 3: zero codes under an
    # INFINITE scale: 0 * inf = NaN (IEEE; the reference's __hfma2 chain alike)
    qa = np.stack([_codes([7]), _codes([-7]), _codes([1]), _codes([])])
    qw = np.stack([_codes([7]), _codes([-7])])
    asc = [1024.0, 1024.0, 1024.0, INF]
    ws = [4.0, 4.0]
    out = _one_group_gemm(qa, asc, qw, ws, "fp16")
    want = np.array([[65504.0, -65504.0], [-65504.0, 65504.0], [28672.0, -28672.0], [65504.0, 65504.0]], np.float32)  # NaN -> +65504
    assert _same(out, want)
    # bf16: 200704 = 49 * 2^12 is a bf16 number and is stored as it is; the NaN row stays NaN
    out = _one_group_gemm(qa, asc, qw, ws, "bf16")
    want = np.array([[200704.0, -200704.0], [-200704.0, 200704.0], [28672.0, -28672.0], [NAN, NAN]], np.float32)
    assert _same(out, want)
    # SiLU then EpilogueDefault (gemm_w4a4_launch_impl.cuh:416-417) on the 16-bit tile: the fp16 tile holds +-inf where the sum overflowed;
    # silu(+inf) = inf * 1 = inf -> 65504; silu(-inf) = -inf * sigmoid(-inf) = -inf * 0 = NaN -> +65504; silu(28672) = 28672, silu(-28672) = -0
    out = _one_group_gemm(qa, asc, qw, ws, "fp16", fuse="silu")
    want = np.array([[65504.0, 65504.0], [65504.0, 65504.0], [28672.0, 0.0], [65504.0, 65504.0]], np.float32)
    assert _same(out, want)
    out = _one_group_gemm(qa, asc, qw, ws, "bf16", fuse="silu")
    want = np.array([[200704.0, 0.0], [0.0, 200704.0], [28672.0, 0.0], [NAN, NAN]], np.float32)  # bf16: -200704 is finite, silu = -0
    assert _same(out, want)


def test_bias_and_low_rank_terms_saturate_too():
    """the clamp is the LAST step (EpilogueBias -> LoraUp -> ... -> EpilogueDefault, launch_impl.cuh:172-280): a bias or a low-rank term alone can saturate"""
    qa = np.stack([_codes([1]), _codes([1])])
    qw = np.stack([_codes([1])])
    out = O.gemm_w4a4(qa, np.full((1, 2), 1.0, np.float32), qw, np.full((1, 1), 1.0, np.float32), dtype="fp16", bias=np.array([65504.0], np.float32),
                      lora_act_in=np.array([[32.0] + [0.0] * 15, [-8.0] + [0.0] * 15], np.float32), lora_up=np.array([[1024.0] + [0.0] * 15], np.float32))["out"]
    # 1 + 65504 + 32 * 1024 = 98273 -> 65504;   1 + 65504 - 8 * 1024 = 57313 -> fp16 (spacing 32 above 32768): 57312
    assert _same(out, np.array([[65504.0], [57312.0]], np.float32))


def test_rmsnorm_rope_out_form_is_clamped_and_packed_form_is_not():
    """launch_impl.cuh:395-404: EpilogueRMSNormRope -> EpilogueDefault for ``out``: V (untouched by the epilogue, epilogues.cuh:414-423) overflows and is clamped;
    :377-394: -> EpiloguePackQKV for out_q / out_k / out_v, which converts and stores (epilogues.cuh:446-549): no clamp."""
    N = 384
    qa = np.stack([_codes([7]), _codes([])])
    qw = np.stack([_codes([7 if n % 2 == 0 else -7]) for n in range(N)])
    rot = np.zeros((2, 64, 2), np.float32)
    rot[:, :, 1] = 1.0  # cos = 1, sin = 0: the rotation is the identity
    ones = np.ones(128, np.float32)
    kw = dict(dtype="fp16", fuse="rmsnorm_rope", norm_q=ones, norm_k=ones, rot=rot)
    asc = np.array([[1024.0, INF]], np.float32)
    ws = np.full((1, N), 4.0, np.float32)
    out = O.gemm_w4a4(qa, asc, qw, ws, **kw)["out"]
    sign = np.where(np.arange(128) % 2 == 0, 1.0, -1.0).astype(np.float32)
    assert _same(out[0, 256:], 65504.0 * sign)                     # V: +-200704 -> +-inf in fp16 -> +-65504
    assert _same(out[1], np.full(N, 65504.0, np.float32))          # NaN row: Q, K (NaN through norm and rotation) and V all +65504
    packed = O.gemm_w4a4(qa, asc, qw, ws, packed_qkv=True, **kw)["out"]
    assert _same(packed[0, 256:], INF * sign)
    assert np.isnan(packed[1]).all()
    # Q / K of row 0: every pre-norm value is +-inf in fp16, the mean of squares is inf, coef = 0, inf * 0 = NaN -> +65504 clamped, NaN packed
    assert _same(out[0, :256], np.full(256, 65504.0, np.float32)) and np.isnan(packed[0, :256]).all()


# ----------------------------------------------------------------------------- the group quantiser
def _row(values, fill=0.0):
    r = np.full(64, fill, np.float32)
    r[: len(values)] = values
    return r


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_quantize_rows_on_non_finite_groups(dtype):
    """gemm_w4a4.cuh:455-497.  Expected values by hand; 3.5 = 7 * 0.5 so that scale = fp32(3.5 * fp32(1/7)) and code = rni(x / scale):
    3.5 -> 7, -1.0 -> -2, 0.75 -> 1.5 -> rni = 2 (ties to even), 0.25 -> 0.5 -> 0."""
    base = [3.5, -1.0, 0.75, 0.25]
    base_codes = [7, -2, 2, 0]
    x = np.stack([
        _row(base),                       # 0 clean
        _row(base + [INF]),               # 1 +inf: amax inf, scale inf, rcp = +0: finite * 0 = 0, inf * 0 = NaN -> 0
        _row(base + [-INF]),              # 2 -inf: the same (amax is of |x|)
        _row(base + [NAN]),               # 3 NaN among finite: __hmax skips it; NaN * rcp = NaN -> code 0, the others unchanged
        _row(base + [NAN, INF]),          # 4 NaN and inf: as the inf group
        _row([], fill=NAN),               # 5 all NaN: amax = 0 (the chain starts at 0, :456-457) -> scale 0 -> rcp inf -> NaN -> 0
        _row([]),                         # 6 all zero: scale 0, 0 * inf = NaN -> 0
    ])
    q, asc = O.quantize_rows(x, dtype, unsigned=False)
    s_clean = float(O.round16(np.array([np.float32(3.5) * (np.float32(1.0) / np.float32(7.0))], np.float32), dtype)[0])
    want_q = np.zeros((7, 64), np.int8)
    want_q[0, :4] = base_codes
    want_q[3, :4] = base_codes
    assert np.array_equal(q, want_q)
    assert _same(asc[0], [s_clean, INF, INF, s_clean, INF, 0.0, 0.0])
    # unsigned (the GELU epilogue's requantiser): scale = amax / 15, negatives saturate to 0; 3.75 -> 15, 1.0 -> 4, -1.0 -> 0
    xu = np.stack([_row([3.75, 1.0, -1.0]), _row([3.75, 1.0, -1.0, NAN]), _row([3.75, 1.0, INF])])
    q, asc = O.quantize_rows(xu, dtype, unsigned=True)
    want_q = np.zeros((3, 64), np.int8)
    want_q[0, :2] = want_q[1, :2] = [15, 4]
    s_u = float(O.round16(np.array([np.float32(3.75) * (np.float32(1.0) / np.float32(15.0))], np.float32), dtype)[0])
    assert np.array_equal(q, want_q) and _same(asc[0], [s_u, s_u, INF])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_quantiser_entry_point_and_envelope_accept_non_finite_input(dtype):
    """through quantize_w4a4_act_fuse_lora (smoothing division, padding, low-rank projection) and quantize_envelope: two groups per row, one polluted;
    the clean group's codes and scales are those of the clean input, the envelope contains the oracle's codes and pins the polluted groups"""
    rng = np.random.default_rng(0)
    x = O.round16(rng.standard_normal((4, 128)).astype(np.float32), dtype)
    smooth = O.round16(np.exp(rng.standard_normal(128) * 0.5).astype(np.float32), dtype)
    ld = O.round16(rng.standard_normal((128, 16)).astype(np.float32) * 0.05, dtype)
    q0, a0, l0 = O.quantize_w4a4_act_fuse_lora(x, smooth, ld, dtype, pad_size=4)
    xp = x.copy()
    xp[0, 3] = INF
    xp[1, 64 + 5] = NAN
    xp[2, 10], xp[2, 11] = -INF, NAN
    q, a, l = O.quantize_w4a4_act_fuse_lora(xp, smooth, ld, dtype, pad_size=4)
    clean = np.ones((4, 2), bool)
    clean[0, 0] = clean[1, 1] = clean[2, 0] = False
    cm = np.repeat(clean, 64, axis=1)
    assert np.array_equal(q[cm], q0[cm]) and _same(a.T[clean], a0.T[clean])
    assert not q[0, :64].any() and not q[2, :64].any() and a[0, 0] == INF and a[0, 2] == INF
    # row 1, group 1: NaN element -> 0, every other code unchanged unless the NaN replaced the group's maximum (it did not: checked)
    assert np.abs(x[1, 64:]).argmax() != 5
    want = q0[1, 64:].copy()
    want[5] = 0
    assert np.array_equal(q[1, 64:], want) and a[1, 1] == a0[1, 1]
    assert not np.isfinite(l[:3]).any() and np.isnan(l[1:3]).all() and _same(l[3], l0[3])   # x @ lora_down: a non-finite element reaches every rank of ITS row only (inf * w = +-inf; NaN)
    env = O.quantize_envelope(xp, smooth, dtype, pad_size=4)
    assert np.all(env["q_lo"] <= q) and np.all(q <= env["q_hi"])
    assert not env["q_lo"][0, :64].any() and not env["q_hi"][0, :64].any() and env["s_lo"][0, 0] == INF and env["s_hi"][0, 0] == INF
    assert env["q_lo"][1, 64 + 5] == 0 and env["q_hi"][1, 64 + 5] == 0


def test_gemm_with_infinite_ascales_and_gelu_quant_on_nan_rows():
    """an infinite ascale over zero codes is 0 * inf = NaN in float64 as in the reference's fp16 / bf16 FMA; the row is NaN, other rows untouched;
    GELU_QUANT requantises a NaN row to code 0 / scale 0 (quantize_rows: amax ignores NaN) and its next-layer low-rank sums are NaN"""
    L = O.make_svdq_layer(128, 128, 16, seed=1, dtype="bf16", cheap=True)
    L2 = O.make_svdq_layer(128, 128, 16, seed=2, dtype="bf16", cheap=True)
    x = O.make_activations(4, 128, seed=1, dtype="bf16")
    q0, a0, l0 = O.quantize_w4a4_act_fuse_lora(x, L["smooth"], L["proj_down"], "bf16", pad_size=4)
    x[2, 7] = INF
    q, a, l = O.quantize_w4a4_act_fuse_lora(x, L["smooth"], L["proj_down"], "bf16", pad_size=4)
    kw = dict(dtype="bf16", bias=L["bias"], lora_up=L["proj_up"])
    ref = O.gemm_w4a4(q0, a0, L["qweight"], L["wscales"], lora_act_in=l0, **kw)["out"]
    got = O.gemm_w4a4(q, a, L["qweight"], L["wscales"], lora_act_in=l, **kw)["out"]
    assert np.isnan(got[2]).all() and _same(got[[0, 1, 3]], ref[[0, 1, 3]])
    got16 = O.gemm_w4a4(q, a, L["qweight"], L["wscales"], lora_act_in=l, dtype="fp16", bias=L["bias"], lora_up=L["proj_up"])["out"]
    assert _same(got16[2], np.full(128, 65504.0, np.float32))
    r = O.gemm_w4a4(q, a, L["qweight"], L["wscales"], lora_act_in=l, fuse="gelu_quant", next_smooth=L2["smooth"], next_lora_down=L2["proj_down"], envelope=True, **kw)
    r0 = O.gemm_w4a4(q0, a0, L["qweight"], L["wscales"], lora_act_in=l0, fuse="gelu_quant", next_smooth=L2["smooth"], next_lora_down=L2["proj_down"], **kw)
    assert not r["qout"][2].any() and not r["oscales"][:, 2].any() and np.isnan(r["lora_act_out"][2]).all()
    keep = [0, 1, 3]
    assert np.array_equal(r["qout"][keep], r0["qout"][keep]) and _same(r["oscales"][:, keep], r0["oscales"][:, keep])
    assert _same(r["lora_act_out"][keep], r0["lora_act_out"][keep])
