"""All five copies of the 4-bit activation quantiser on the constructed inputs of tests/quantiser_profiles.py, compared BIT FOR BIT with the IEEE oracle
(``oracle.quantize_rows``): codes through ``layout.unpack_act``, scale bit patterns through ``layout.unpack_scales``, no envelope and no flip budget.

  sites 1, 2  quantize_kernel (general family, fuse_glu front end) and quantize_kernel_v2 (fast family): code grids with every tie, the walking maximum,
              one-hot rows (lora_act bit-equal to a row of lora_down, fp32 and Q31.32), ragged M = 77, the grouped launch, exact front ends (power-of-two
              smoothing, identity LayerNorm, identity GLU), and EVERY positive finite 16-bit value as amax (512 x 4096)
  site 3      the GELU_QUANT epilogue of svdq_gemm_w4a4 (unsigned codes) on a bias that IS the unsigned grid, in its plain (both tile heights), carry, hybrid
              carry, solo carry and split-down variants
  sites 4, 5  the fused output quantiser of attention_kernel, attention_kernel64 and the split low-rank path, on one-hot score rows whose output is a chosen V
              row exactly (asserted first, so that a softmax difference is not misread as a quantiser one)

Every test asserts the kernel it claims: ``quant_plan`` (svdq_quantize_plan), ``ops.gemm_last_plan()``, ``ops.attention_last_plan()``.
tests/test_quantiser_profiles.py checks the builders' preconditions on the CPU and shows that the comparison used here catches round-half-away, truncation and a
singly rounded scale.
"""

import functools
import math

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests import helpers as Hh
from tests import quantiser_profiles as P
from tests.helpers import TORCH_DT, make_module, t16
from tests.test_gpu_hot_instantiations import attn_plan_key, quant_plan

pytestmark = pytest.mark.gpu

DT = list(P.DTYPES)
M_RAGGED, K_SMALL = 77, 256       # ragged in the last 32-row tile of the first 256-row block; two 128-channel chunks
M_GROUPED = 300                   # the grouped launch: a second stream behind 256 rows


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nunchaku_amd import _lib

    _lib.load()


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _unpacked(act, asc, K, M_pad, unsigned=False):
    from nunchaku_amd import layout

    return layout.unpack_act(act, K, unsigned=unsigned).cpu().numpy(), _bits(layout.unpack_scales(asc, M_pad))


# =======================================================================================================================================================
# sites 1 and 2: the stand-alone quantiser
# =======================================================================================================================================================
# (name, R, smoothing, LayerNorm front end, fuse_glu, grouped, lora_act format, family the plan must name)
QUANT_CASES = (
    [(f"fast-r{R}{'-smooth' if sm else ''}{'-ln' if ln else ''}", R, sm, ln, False, False, "f32", "fast") for R in (0, 32) for sm in (False, True) for ln in (False, True)]
    + [("fast-r32-smooth-q32", 32, True, False, False, False, "q32", "fast"),
       ("fast-grouped-r32-smooth-ln", 32, True, True, False, True, "f32", "fast"),
       ("fast-grouped-r0", 0, False, False, False, True, "f32", "fast"),
       ("general-r176", 176, False, False, False, False, "f32", "general"),
       ("general-r176-smooth-q32", 176, True, False, False, False, "q32", "general"),
       ("general-glu-r32", 32, False, False, True, False, "f32", "general"),
       ("general-glu-r32-smooth", 32, True, False, True, False, "f32", "general")]
)


def _glu_ks(dtype):
    """the grid exponents whose values divided by 32 are still exact in the format"""
    return tuple(k for k in P.GRID_K[(dtype, False)] if P.is16(P.code_grid(dtype, False, k)["x"].astype(np.float64) / 32.0, dtype).all())


@functools.lru_cache(maxsize=None)
def _profile(name, dtype, M, K, glu):
    """-> (x_hat the quantiser must see [M, K], one-hot record | None)"""
    if name == "grid":
        return P.grid_rows(dtype, False, K, M, ks=_glu_ks(dtype) if glu else None), None
    if name == "max-position":
        return P.max_position_matrix(dtype, M, K), None
    rec = P.one_hot_rows(K, 176, M, dtype)
    return rec["x"], rec


def _smooth_of(K, stream):
    return np.roll(P.smooth_pow2(K), 3 * stream)


class _Stream:
    """one input with its parameter set, built so that the quantiser sees ``xh`` exactly"""

    def __init__(self, xh, rec, R, smooth, ln, glu, dtype, stream):
        M, K = xh.shape
        self.smooth = _smooth_of(K, stream) if smooth else None
        if smooth:
            xin, xh, self.zeroed = P.presmoothed(xh, self.smooth, dtype)
        else:
            xin, self.zeroed = xh, 0
        self.xh, self.xin = xh, xin          # xin: the 16-bit input of the projection (what lora_act sums)
        self.D = None
        if R:
            self.D = np.roll(rec["lora_down"][:, :R], stream, axis=0) if rec is not None else (np.random.default_rng(R + stream).integers(-8, 8, (K, R)) / 64.0).astype(np.float32)
        self.kw = {}
        if ln:
            stats, scale, shift = P.ln_identity(M, K, xin, dtype)
            self.kw = dict(ln_stats=torch.from_numpy(stats).cuda(), mod_scale=t16(scale, dtype), mod_shift=t16(shift, dtype))
            assert _bits(self.kw["mod_shift"])[0] == 0x8000  # -0 survived the trip
        self.xt = t16(P.glu_identity(xin, dtype) if glu else xin, dtype)
        self.smooth_t = None if self.smooth is None else t16(O.pack_vec_ref(self.smooth), dtype)
        self.D_t = None if self.D is None else t16(O.pack_lowrank_ref(np.ascontiguousarray(self.D.T), down=True), dtype)

    def lora_act(self):
        """exact where at most one addend per element is non-zero (one-hot rows)"""
        return (self.xin.astype(np.float64) @ self.D.astype(np.float64))


def _quantize(streams, R, glu, fmt, K, M_pad, dtype):
    from nunchaku_amd._C import ops

    act = torch.full((M_pad, K * 3 // 4), 0xA5, dtype=torch.uint8, device="cuda")
    asc = torch.full((K // 64, M_pad), float("nan"), dtype=TORCH_DT[dtype], device="cuda")
    la = None
    if R:  # junk: the op clears what it accumulates into
        la = torch.full((M_pad, R), 3.0, dtype=torch.float32, device="cuda") if fmt == "f32" else torch.full((M_pad, R), 12345, dtype=torch.int64, device="cuda")
    s0 = streams[0]
    second = None
    if len(streams) == 2:
        s1 = streams[1]
        second = dict(input=s1.xt, smooth=s1.smooth_t, lora_down=s1.D_t, **s1.kw)
    ops.quantize_w4a4_act_fuse_lora(s0.xt, act, asc, s0.D_t, la, s0.smooth_t, glu, False, second=second, **s0.kw)
    return act, asc, la


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", QUANT_CASES, ids=lambda c: c[0])
def test_quantiser_is_exact_on_grids_walking_maxima_and_one_hot_rows(case, dtype):
    """Code grids (every code value, every tie, the ties' 16-bit neighbours, +-0, at exponents from the smallest to the largest the format holds), the walking
    maximum and one-hot rows at M = 77 (grouped: M = 300), K = 256: codes and scale bits equal to the IEEE oracle's, padded rows code 0 / scale 0, and on the
    one-hot rows lora_act bit-equal to the selected row of lora_down (times its power-of-two smoothing factor's inverse image: the projection reads the
    un-smoothed input) -- as fp32, or as the value times 2^32 in the fixed-point format."""
    name, R, smooth, ln, glu, grouped, fmt, family = case
    M, K = (M_GROUPED if grouped else M_RAGGED), K_SMALL
    M_pad = math.ceil(M / 256) * 256
    plan = quant_plan(R, smooth, ln, glu, grouped, fmt, M, K, M_pad)
    assert plan["family"] == family and plan["glu"] == glu, plan
    if family == "fast":
        assert (plan["sel"] >> 2 & 1, plan["sel"] >> 1 & 1, plan["sel"] & 1) == (int(R > 0), int(ln), int(smooth)), plan
    for prof in ("grid", "max-position", "one-hot"):
        xh, rec = _profile(prof, dtype, M, K, glu)
        cuts = [(0, 256), (256, M)] if grouped else [(0, M)]
        streams = [_Stream(xh[a:b], rec, R, smooth, ln, glu, dtype, i) for i, (a, b) in enumerate(cuts)]
        act, asc, la = _quantize(streams, R, glu, fmt, K, M_pad, dtype)
        codes, sbits = _unpacked(act, asc, K, M_pad)
        want = np.zeros((M_pad, K), dtype=np.float32)
        want[:M] = np.concatenate([s.xh for s in streams])
        q, s = P.expected(want, dtype)
        assert not q[M:].any() and not s[:, M:].any()
        P.assert_exact(codes, sbits, q, s, f"{name} {prof} {dtype}")
        if prof == "one-hot" and R:
            ref = np.zeros((M_pad, R))
            ref[:M] = np.concatenate([s_.lora_act() for s_ in streams])
            got = la.cpu().numpy()
            ref = ref.astype(np.float32) if fmt == "f32" else np.round(ref * 2.0 ** 32).astype(np.int64)
            bad = np.argwhere(got != ref)
            assert got.dtype == ref.dtype and not len(bad), (f"{name} {dtype}: lora_act of one-hot rows: {len(bad)} elements differ, first (row, rank) {bad[0].tolist()}: "
                                                             f"got {got[tuple(bad[0])]!r}, lora_down gives {ref[tuple(bad[0])]!r}")


@functools.lru_cache(maxsize=None)
def _sweep(dtype):
    s = P.amax_sweep(dtype, False)
    M, K = 512, 4096
    n = len(s["a"])
    rows, groups = P.sweep_slots(n, M)
    q = np.zeros((M, K // 64, 64), dtype=np.int8)
    sb = np.zeros((K // 64, M), dtype=np.uint16)
    dom = np.zeros((M, K // 64), dtype=bool)
    filled = np.zeros((M, K // 64), dtype=bool)
    q[rows, groups], sb[groups, rows], dom[rows, groups], filled[rows, groups] = s["codes"], s["scale_bits"], s["in_domain"], True
    x = P.sweep_matrix(s["x"], M, K)
    q2, sb2 = P.expected(x, dtype)
    assert np.array_equal(q2, q.reshape(M, K)) and np.array_equal(sb2, sb)
    return s, x, q.reshape(M, K), sb, dom | ~filled, filled & ~dom


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("family,R", [("fast", 0), ("general", 176)], ids=["fast", "general-r176"])
def test_every_16_bit_amax_gives_the_oracles_codes_and_scale(family, R, dtype):
    """One group per positive finite 16-bit value used as amax (32639 bf16 / 31743 fp16 groups in one 512 x 4096 launch, signed, no smoothing): wherever the
    fp32 scale amax * fl(1/7) is a normal number -- every fp16 value; every bf16 value but the 479 below about 8.2e-38 -- codes and scale bits equal the IEEE
    oracle's.  In particular x = +-amax gives +-7 for every amax of the domain: the converter's -8 .. 7 clamp never fires, and no scale is a step off.
    On the excluded bf16 values (products below 1e-36) only finiteness is asserted; what the kernel does there is printed.  Observed on an MI355X, both
    families alike: all 479 stored scales equal the oracle's bits (3 of them zero); the codes equal the oracle's in 255 groups and differ in 224 (the
    reciprocal of a subnormal scale), none decodes beyond |15|."""
    s, x, q, sb, compare, excluded = _sweep(dtype)
    M, K = x.shape
    plan = quant_plan(R, False, False, False, False, "f32", M, K, M)
    assert plan["family"] == family, plan
    D_t = None if not R else torch.zeros(K, R, dtype=TORCH_DT[dtype], device="cuda")
    from nunchaku_amd._C import ops

    act = torch.full((M, K * 3 // 4), 0xA5, dtype=torch.uint8, device="cuda")
    asc = torch.full((K // 64, M), float("nan"), dtype=TORCH_DT[dtype], device="cuda")
    la = torch.zeros(M, R, dtype=torch.float32, device="cuda") if R else None
    ops.quantize_w4a4_act_fuse_lora(t16(x, dtype), act, asc, D_t, la, None)
    codes, sbits = _unpacked(act, asc, K, M)
    n_ex = int(excluded.sum())
    assert n_ex == int((~s["in_domain"]).sum()) and (n_ex == 0) == (dtype == "fp16")
    ends = np.abs(q.reshape(M, K // 64, 64)).max(axis=2)
    assert (ends[compare & (np.abs(x).reshape(M, K // 64, 64).max(axis=2) > 0)] == 7).all()
    P.assert_exact(codes, sbits, q, sb, f"amax sweep {family} {dtype}", mask=compare)
    if n_ex:
        sc = O.from_bits16(sbits, dtype).T[excluded]
        cg = codes.reshape(M, K // 64, 64)[excluded]
        assert np.isfinite(sc).all() and np.isfinite(cg.astype(np.float32)).all()  # (int8 codes: finite by type; the scales could be inf / NaN and are not)
        same_c = (cg == q.reshape(M, K // 64, 64)[excluded]).all(axis=1)
        same_s = sbits.T[excluded] == sb.T[excluded]
        print(f"excluded bf16 amax values ({family}): {n_ex} groups; codes equal to the oracle's in {int(same_c.sum())}, all-zero codes in {int((cg == 0).all(axis=1).sum())}, "
              f"scale bits equal in {int(same_s.sum())}, zero scales {int((sc == 0).sum())}, largest |code| {int(np.abs(cg.astype(np.int32)).max())}")


# =======================================================================================================================================================
# site 3: the GELU_QUANT epilogue
# =======================================================================================================================================================
# (geometry, own rank R, next rank R2, M, K, N, plan variant, tile rows).  Hybrid carry needs the row-run schedule, which the launcher takes from
# (M_pad / 256) * (N / 128) = 2 * 256 CUs on: (1800, 128, 8192), the smallest such shape (tests/test_gpu_hot_instantiations.py).  Split-down needs an own rank on
# the all-rank path: rank 64 with an all-zero lora_up, which adds +0 to the pre-activation.
GELU_CASES = (
    (1, 0, 0, 300, 128, 256, "plain", 256),
    (3, 0, 0, 300, 128, 256, "plain", 128),
    (0, 0, 32, 300, 128, 256, "carry", 256),
    (0, 0, 48, 1800, 128, 8192, "hybrid_carry", 256),
    (6, 0, 128, 300, 128, 256, "solo_carry", 128),
    (7, 64, 128, 300, 128, 256, "split_down", 256),
)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", GELU_CASES, ids=lambda c: f"g{c[0]}-r{c[1]}-next{c[2]}-{c[6]}")
def test_gelu_quant_epilogue_is_exact_on_the_unsigned_grid(case, dtype):
    """All-zero weight codes, no (or an all-zero) low-rank branch and a bias that is the unsigned code grid at step 128 (bf16) / 1024 (fp16): the pre-activation
    is the bias, gelu is the identity on it (-0 on the -S entries), the 16-bit add of 0.171875 rounds back to the grid, and the epilogue's quantiser must give
    the oracle's codes (ties to even, 15 at the end, 0 for the shifted zeros) and the scale S bit for bit -- with next_smooth all ones and with powers of two
    1 .. 4.  The epilogue has no row count: a padded row is a zero activation row, whose pre-activation is the bias too, so EVERY row of the M_pad equals the
    first.  qout and oscales only (lora_act_out is judged by tests/test_gpu_hot_instantiations.py)."""
    from nunchaku_amd import layout
    from nunchaku_amd._C import _Ops, ops
    from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda

    geometry, R, R2, M, K, N, variant, tile_rows = case
    td = TORCH_DT[dtype]
    M_pad = math.ceil(M / 256) * 256
    rng = np.random.default_rng(M + N)
    x = O.round16(rng.standard_normal((M, K)).astype(np.float32), dtype)
    for ns in (None, P.smooth_pow2_up(N)):
        rec = P.gelu_grid_bias(dtype, N, ns)
        Rm, R2m = max(R, 16), max(R2, 16)
        L1 = {"qweight": np.zeros((N, K), dtype=np.int8), "wscales": np.ones((K // 64, N), dtype=np.float32), "smooth": np.ones(K, dtype=np.float32),
              "proj_down": (rng.integers(-8, 8, (K, Rm)) / 64.0).astype(np.float32), "proj_up": np.zeros((N, Rm), dtype=np.float32), "bias": rec["bias"]}
        L2 = {"qweight": np.zeros((128, N), dtype=np.int8), "wscales": np.ones((N // 64, 128), dtype=np.float32), "smooth": rec["next_smooth"],
              "proj_down": (rng.integers(-8, 8, (N, R2m)) / 64.0).astype(np.float32), "proj_up": np.zeros((128, R2m), dtype=np.float32), "bias": None}
        m1, m2 = make_module(L1, dtype), make_module(L2, dtype, act_unsigned=True)
        m1._ensure_layout()
        m2._ensure_layout()
        qx, asc, la = m1.quantize(t16(x, dtype))
        assert qx.shape[0] == M_pad
        qh = torch.full(layout.act_image_shape(M_pad, N), 0xA5, dtype=torch.uint8, device="cuda")
        sh = torch.full((N // 64, M_pad), float("nan"), dtype=td, device="cuda")
        kw = dict(act=qx, wgt=m1.qweight, ascales=asc, wscales=m1.wscales, bias=m1.bias, qout=qh, oscales=sh, smooth_factor=m2.smooth_factor)
        if R:
            kw.update(lora_act_in=la, lora_up=m1.proj_up)
        if R2:
            kw.update(lora_down=m2.proj_down, lora_act_out=torch.full((M_pad, R2), 3.0, dtype=torch.float32, device="cuda"))
        saved = (_Ops.gemm_geometry, _Ops.gemm_use_workspace)
        _Ops.gemm_geometry, _Ops.gemm_use_workspace = geometry, True
        try:
            svdq_gemm_w4a4_cuda(**kw)
            plan = ops.gemm_last_plan()
            ops.gemm_workspace_status()
        finally:
            _Ops.gemm_geometry, _Ops.gemm_use_workspace = saved
        assert (plan["tile_rows"], plan["variant"]) == (tile_rows, variant), f"claimed {variant} on {tile_rows}-row tiles, launched {plan}"
        codes = layout.unpack_act(qh, N, unsigned=True)
        scales = layout.unpack_scales(sh, M_pad)
        what = f"GELU_QUANT {variant} {dtype} next_smooth {'ones' if ns is None else 'powers of two'}"
        P.assert_exact(codes[:1].cpu().numpy(), _bits(scales[:, :1]), rec["codes"][None, :], rec["scale_bits"][:, None], what)
        diff = (codes != codes[:1]).any(dim=1) | (scales != scales[:, :1]).any(dim=0)
        assert not diff.any(), f"{what}: rows {diff.nonzero().flatten().tolist()[:8]} .. differ from row 0 ({int(diff.sum())} of {M_pad})"


# =======================================================================================================================================================
# sites 4 and 5: the fused output quantiser of the attention kernels
# =======================================================================================================================================================
ATT_L, ATT_H = 512, 2
# (geometry, rank of the output projection's low-rank branch, split low-rank path)
ATTN_CASES = ((1, 32, False), (2, 32, False), (1, 128, True), (2, 128, True))


@functools.lru_cache(maxsize=None)
def _attn_values(dtype, which, smoothed):
    """V [L, H, 128] carrying the profiles (times the smoothing factors), the x_hat [L, H * 128] behind them, the smoothing factors [H * 128]"""
    L, H = ATT_L, ATT_H
    K = H * 128
    # |V| < FLT_MAX / 16L.  Before a row reaches its winner's tile the online softmax has summed the values of the earlier tiles' best keys (probability 1 until
    # the winner's tile multiplies them by alpha = 0): L values of 7 * 2^125 overflow that sum, and inf * 0 is NaN.  That is the softmax, not the quantiser --
    # no attention output comes near 1e35 -- so the bf16 grids stop at 7 * 2^111 here and the sweep at 2^115; the stand-alone tests hold the full range.
    limit = float(np.finfo(np.float32).max) / (16 * L)  # (a factor 4 for the smoothing factors, 4 to spare)
    if which == "grid+max-position":
        ks = tuple(k for k in P.GRID_K[(dtype, False)] if 7.0 * 2.0 ** k < limit)
        ks += tuple(k for k in (int(np.floor(np.log2(limit / 7.0))) - 1,) if len(ks) < len(P.GRID_K[(dtype, False)]))
        chunks = np.concatenate([P.max_position_rows(dtype), P.grid_rows(dtype, False, 128, L * H - 128, ks=ks)])
    else:
        s = P.amax_sweep(dtype, False, subsample=2 * L * H)
        g = np.zeros((2 * L * H, 64), dtype=np.float32)
        g[:len(s["a"])] = np.where((s["in_domain"] & (s["a"] < limit))[:, None], s["x"], 0.0)
        chunks = g[np.random.default_rng(5).permutation(2 * L * H)].reshape(L * H, 128)
    xh = chunks.reshape(L, K)
    smooth = P.smooth_pow2(K) if smoothed else np.ones(K, dtype=np.float32)
    xin, xh, zeroed = P.presmoothed(xh, smooth, dtype)
    return xin.reshape(L, H, 128), xh, smooth


@functools.lru_cache(maxsize=None)
def _attn_selection(dtype, geometry):
    """one-hot score rows (tests/helpers.py: attn_onehot at a = 2048): q as the kernel reads it, k, the winners pi [L, H]; asserts in float64 that every other
    key's probability underflows to exactly 0 in fp32 (more than 200 log2 units below the winner), so the output row IS the winner's V row whatever it holds"""
    L, H = ATT_L, ATT_H
    pi = Hh.attn_winners(L, H, "scattered")
    q, k, _ = Hh.attn_onehot(L, H, dtype, 2048.0, 1.0, pi, seed=L + H)
    qr, c = (Hh.attn_prescaled(q, dtype), 1.0) if geometry == 2 else (q, Hh.ATT_C)
    s = Hh.attn_scores_log2(qr, k, c)                                  # [H, L, L]
    win = np.take_along_axis(s, pi.T[:, :, None], axis=2)
    other = s.copy()
    np.put_along_axis(other, pi.T[:, :, None], -np.inf, axis=2)
    assert (win[:, :, 0] - other.max(axis=2)).min() > 200.0
    return qr, k, pi


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("geometry,R,split", ATTN_CASES, ids=lambda v: str(v))
def test_attention_fused_quantiser_is_exact_on_selected_value_rows(geometry, R, split, dtype):
    """One-hot score rows at (L, H) = (512, 2): the attention output row is a chosen V row exactly, and the V rows carry the code grids with the walking
    maximum, then a subsample of the amax sweep (every exponent, four mantissa patterns; left out: the values whose fp32 scale is subnormal, groups holding an
    fp32-subnormal element, and bf16 magnitudes from 2^115 up, which overflow the online softmax's running sum -- ``_attn_values``).  Per launch: the 16-bit
    ``out`` equals the selected V rows bit for bit FIRST; then qact / qscales equal the IEEE oracle on those rows -- qsmooth all ones, then powers of two
    1/4 .. 4 -- and the launch without a 16-bit output (what a pipeline runs) gives the same bits.  attention_kernel (8 waves) at rank 32, attention_kernel64
    with a prescaled Q, and the split low-rank path at rank 128, all on the persistent schedule."""
    from nunchaku_amd import layout
    from nunchaku_amd._C import _Ops, ops

    L, H = ATT_L, ATT_H
    K = H * 128
    td = TORCH_DT[dtype]
    qr, k, pi = _attn_selection(dtype, geometry)
    tq, tk = t16(qr, dtype), t16(k, dtype)
    D = (np.random.default_rng(R).integers(-8, 8, (K, R)) / 64.0).astype(np.float32)
    for smoothed in (False, True):
        for which in ("grid+max-position", "amax-sweep"):
            v, xh, smooth = _attn_values(dtype, which, smoothed)
            layer = {"qweight": np.zeros((128, K), dtype=np.int8), "wscales": np.ones((K // 64, 128), dtype=np.float32), "smooth": smooth, "proj_down": D,
                     "proj_up": np.zeros((128, R), dtype=np.float32), "bias": None}
            lin = make_module(layer, dtype)
            lin._ensure_layout()
            vt = t16(v, dtype).permute(1, 2, 0).contiguous()
            want_out = np.take_along_axis(v, pi[:, :, None], axis=0)                                  # [L, H, 128]
            want_xh = np.take_along_axis(xh.reshape(L, H, 128), pi[:, :, None], axis=0).reshape(L, K)
            q_ref, s_ref = P.expected(want_xh, dtype)
            saved = (_Ops.attention_geometry, _Ops.attention_use_workspace, _Ops.attention_split_lowrank)
            got = []
            try:
                _Ops.attention_geometry, _Ops.attention_use_workspace, _Ops.attention_split_lowrank = geometry, True, True
                for with_out in (True, False):
                    out = torch.full((L, H, 128), float("nan"), device="cuda", dtype=td) if with_out else None
                    act = torch.full((L, K * 3 // 4), 0xA5, dtype=torch.uint8, device="cuda")
                    asc = torch.full((K // 64, L), float("nan"), dtype=td, device="cuda")
                    lact = torch.zeros(L, R, dtype=torch.float32, device="cuda")
                    quant = dict(act=act, ascales=asc, lora_act=lact, R=R, smooth=lin.smooth_factor, lora_down=lin.proj_down)
                    ops.attention(tq, tk, vt, out, 1.0 / math.sqrt(128), None, quant, q_prescaled=geometry == 2)
                    plan = ops.attention_last_plan()
                    ops.attention_workspace_status()
                    kernel, targs = attn_plan_key(L, plan)
                    assert (kernel, targs[0 if geometry == 1 else 1]) == (("attention_kernel64", 0) if geometry == 2 else ("attention_kernel", 8)), plan
                    assert plan["persistent_groups"] > 0, plan
                    assert plan["split_lowrank"] == split, plan
                    got.append((out, act, asc))
            finally:
                _Ops.attention_geometry, _Ops.attention_use_workspace, _Ops.attention_split_lowrank = saved
            what = f"attention geometry {geometry} rank {R} {dtype} {which} qsmooth {'powers of two' if smoothed else 'ones'}"
            ob, wb = _bits(got[0][0]), O.to_bits16(want_out, dtype)
            bad = np.argwhere((ob != wb) & ~((ob & 0x7FFF == 0) & (wb & 0x7FFF == 0)))                # (+0 and -0: the same value)
            assert not len(bad), f"{what}: the 16-bit out is not the selected V row: {len(bad)} elements, first (row, head, channel) {bad[0].tolist()}: 0x{ob[tuple(bad[0])]:04x} vs 0x{wb[tuple(bad[0])]:04x}"
            codes, sbits = _unpacked(got[0][1], got[0][2], K, L)
            P.assert_exact(codes, sbits, q_ref, s_ref, what)
            assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2]), f"{what}: the launch without a 16-bit output gives other bits"
