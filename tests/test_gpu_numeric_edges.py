"""The W4A4 kernels where their hand-made numerics live and no seeded N(0, 1) test reaches: GEMM outputs beyond +-65504 (the fp16 clamp of the 8-wave C++
epilogue, of the generated wave-tile epilogue, and the oracle's), +-inf / NaN fed to the quantiser and to every GEMM epilogue (row isolation: one bad token
must not touch another), activation scales that are fp16 subnormals, weight scales at the limit of the x32 scale image.

Non-finite numbers are ordinary data here: no kernel's control flow or addressing depends on them.  Conventions of test_gpu_parity.py: everything through
the C ABI, kernel selection with ``_Ops.gemm_geometry`` (1: 256 x 128 tiles / 8 waves, 2 and 3: 128 x 128 tiles, 6 / 7: the GELU_QUANT carry variants,
8: the wave-tile 128 kernel, plain epilogue at rank 0 or 32 only -- a test that claims it ran asserts the plan)."""

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests.helpers import TORCH_DT, assert_close_16, checked_codes, f32, make_module, t16

pytestmark = pytest.mark.gpu

FP16_MAX = 65504.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nunchaku_amd import _lib

    _lib.load()


def _with_geometry(g, fn):
    """fn() under gemm_geometry g -> (result, plan of the last GEMM launch)"""
    from nunchaku_amd._C import _Ops, ops

    _Ops.gemm_geometry = g
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, ops.gemm_last_plan()
    finally:
        _Ops.gemm_geometry = 0


def _check_plan(g, plan, wave_tile_ok=True):
    if g == 8 and wave_tile_ok:
        assert plan["variant"] == "wave_tile_128", plan
    else:
        assert plan["variant"] != "wave_tile_128", plan


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """equal element for element, a NaN equal to a NaN (two kernels may produce different NaN payloads)"""
    if a.dtype in (torch.float16, torch.bfloat16, torch.float32):
        return bool(((a == b) | (a.isnan() & b.isnan())).all())
    return torch.equal(a, b)


def _rot(M_pad, seed=0):
    ang = np.random.default_rng(seed).uniform(0, 6.28, (M_pad, 64)).astype(np.float32)
    rot = np.stack([np.sin(ang), np.cos(ang)], axis=-1).astype(np.float32)
    return rot, torch.from_numpy(O.pack_rotemb_ref(rot)).cuda().view(1, M_pad, 128)


class _W:  # stands in for torch.nn.RMSNorm: only .weight is read
    def __init__(self, w, dtype):
        self.weight = t16(w, dtype)


def _norm_weights(dtype, seed=12):
    rng = np.random.default_rng(seed)
    return (O.round16((1 + 0.1 * rng.standard_normal(128)).astype(np.float32), dtype), O.round16((1 + 0.1 * rng.standard_normal(128)).astype(np.float32), dtype))


# ----------------------------------------------------------------------------- (a) fp16 saturation
def _saturating_layer(K, N, dtype):
    """weight scales, low-rank up factor and bias times 2^15, activations times 2 (all exact in either 16-bit type): the outputs of the seeded layer, |y| ~ 1,
    land around 2^16 -- saturated, nearly saturated and ordinary elements together.  Largest weight scale ~1300 < 2047 (the scale image's limit)."""
    L = O.make_svdq_layer(K, N, 32, seed=11, dtype=dtype, cheap=True)
    for name in ("wscales", "proj_up", "bias"):
        L[name] = O.round16(L[name] * np.float32(2.0 ** 15), dtype)
    assert float(np.abs(L["wscales"]).max()) < 2047.0
    x = O.round16(O.make_activations(300, K, seed=11, dtype=dtype) * np.float32(2.0), dtype)
    return L, x


def _assert_saturation_share(ref, dtype, what):
    """precondition, on the oracle alone: between 1 % and 50 % of the outputs beyond the fp16 range, both signs"""
    hi, lo = (ref >= FP16_MAX), (ref <= -FP16_MAX)
    if dtype == "bf16":
        hi, lo = (ref > FP16_MAX), (ref < -FP16_MAX)
    share = (hi | lo).mean()
    print(f"{what} [{dtype}]: {hi.mean():.3%} at or beyond +65504, {lo.mean():.3%} at or beyond -65504, median |y| {np.median(np.abs(ref)):.0f}")
    assert 0.01 <= share <= 0.5 and hi.any() and lo.any(), f"{what}: the case does not saturate as designed ({share:.3%})"
    return hi | lo


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_outputs_beyond_the_fp16_range_plain_and_silu(dtype):
    """EpilogueDefault's clamp (gemm_base.cuh:689-695; oracle.clamp16_default) in the 8-wave kernel, a 128 x 128 geometry and the wave-tile kernel, M = 300 (an M
    tail): fp16 stores exactly +-65504 wherever the oracle saturates, never inf or NaN, all kernels bit-identical; bf16 is NOT clamped -- values beyond 65504
    are stored as they are.  SiLU (EpilogueSilu -> EpilogueDefault): an fp16 pre-activation that overflowed to -inf gives -inf * sigmoid(-inf) = NaN, which
    the reference's clamp order turns into +65504."""
    from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda

    M, K, N = 300, 384, 256
    L, x = _saturating_layer(K, N, dtype)
    mod = make_module(L, dtype)
    qx, asc, la = mod.quantize(t16(x, dtype))
    q, a = checked_codes(qx, asc, x, L["smooth"], dtype)
    kw = dict(dtype=dtype, bias=L["bias"], lora_act_in=la.cpu().numpy(), lora_up=L["proj_up"])
    ref = O.gemm_w4a4(q, a, L["qweight"], L["wscales"], **kw)["out"][:M]
    ref_silu = O.gemm_w4a4(q, a, L["qweight"], L["wscales"], fuse="silu", **kw)["out"][:M]
    sat = _assert_saturation_share(ref, dtype, "plain")
    sat_silu = np.abs(ref_silu) >= FP16_MAX
    assert sat_silu.mean() >= 0.01
    if dtype == "fp16":
        assert np.abs(ref).max() == FP16_MAX and np.abs(ref_silu).max() == FP16_MAX
    else:
        assert np.abs(ref).max() > 2 * FP16_MAX and np.isfinite(ref).all()

    def run(silu):
        out = torch.empty(M, N, dtype=TORCH_DT[dtype], device="cuda")
        svdq_gemm_w4a4_cuda(act=qx, wgt=mod.qweight, out=out, ascales=asc, wscales=mod.wscales, lora_act_in=la, lora_up=mod.proj_up, bias=mod.bias, fuse_silu=silu)
        return out

    outs = {}
    for g in (1, 2, 8):
        outs[g], plan = _with_geometry(g, lambda: run(False))
        _check_plan(g, plan)
        got = f32(outs[g])
        assert np.isfinite(got).all(), f"geometry {g}: inf or NaN in the output"
        assert_close_16(got, ref, dtype, f"plain, geometry {g}", max_bad_frac=0.0, ulps=1.0)
        if dtype == "fp16":
            assert np.array_equal(got[sat], ref[sat]), f"geometry {g}: {(got[sat] != ref[sat]).sum()} saturated elements are not the oracle's"
    assert torch.equal(outs[1], outs[2]) and torch.equal(outs[1], outs[8]), "the kernels disagree on a saturating layer"
    souts = {}
    for g in (1, 2, 3):
        souts[g], plan = _with_geometry(g, lambda: run(True))
        _check_plan(g, plan)
        got = f32(souts[g])
        assert np.isfinite(got).all(), f"SiLU, geometry {g}: inf or NaN in the output"
        assert_close_16(got, ref_silu, dtype, f"silu, geometry {g}", max_bad_frac=2e-3, ulps=1.0)  # (test_silu_epilogue's tolerances)
        assert_close_16(got, ref_silu, dtype, f"silu(2ulp), geometry {g}", ulps=2.0)
        if dtype == "fp16":
            assert np.array_equal(got[sat_silu], ref_silu[sat_silu]), f"SiLU, geometry {g}: {(got[sat_silu] != ref_silu[sat_silu]).sum()} saturated elements differ"
    assert torch.equal(souts[1], souts[2]) and torch.equal(souts[1], souts[3])


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_outputs_beyond_the_fp16_range_qkv_epilogue(dtype):
    """EpilogueRMSNormRope -> EpilogueDefault (gemm_w4a4_launch_impl.cuh:395-404): the V third passes the clamp, in ``out`` and in ``out_vt`` (this library's
    transposed V for its attention kernel: the ``out`` form's values); Q / K stay finite in fp16 (an overflowed pre-norm value makes its head NaN, which the
    clamp stores as +65504)."""
    from nunchaku_amd.ops.fused import fused_qkv_norm_rottary

    M, K, N = 300, 384, 384
    M_pad = 512
    L, x = _saturating_layer(K, N, dtype)
    mod = make_module(L, dtype)
    nq, nk = _norm_weights(dtype)
    rot, packed = _rot(M_pad)
    xt = t16(x, dtype)
    quantized = mod.quantize(xt)
    q, a = checked_codes(quantized[0], quantized[1], x, L["smooth"], dtype)
    ref = O.gemm_w4a4(q, a, L["qweight"], L["wscales"], dtype=dtype, bias=L["bias"], lora_act_in=quantized[2].cpu().numpy(), lora_up=L["proj_up"],
                      fuse="rmsnorm_rope", norm_q=nq, norm_k=nk, rot=rot)["out"][:M]
    V = slice(2 * N // 3, N)
    sat = _assert_saturation_share(ref[:, V], dtype, "V third")

    def run():
        vt = torch.zeros(N // 3, M_pad, dtype=TORCH_DT[dtype], device="cuda")
        y = fused_qkv_norm_rottary(xt.view(1, M, K), mod, _W(nq, dtype), _W(nk, dtype), packed, quantized=quantized)
        y2 = fused_qkv_norm_rottary(xt.view(1, M, K), mod, _W(nq, dtype), _W(nk, dtype), packed, out_vt=vt[:, :M], quantized=quantized)
        return y[0].clone(), y2[0, :, : 2 * N // 3].clone(), vt

    outs = {}
    for g in (1, 2, 3):
        outs[g], plan = _with_geometry(g, run)
        _check_plan(g, plan)
        y, qk2, vt = outs[g]
        got, got_vt = f32(y), f32(vt)[:, :M].T
        for name, v in (("V", got[:, V]), ("V^T", got_vt)):
            assert np.isfinite(v).all()
            assert_close_16(v, ref[:, V], dtype, f"{name}, geometry {g}", max_bad_frac=0.0, ulps=1.0)
            if dtype == "fp16":
                assert np.array_equal(v[sat], ref[:, V][sat]), f"{name}, geometry {g}: saturated elements are not the oracle's"
        if dtype == "fp16":
            assert np.isfinite(got).all(), f"geometry {g}: inf or NaN in Q / K"
            assert float(np.abs(got).max()) == FP16_MAX
        else:
            assert float(np.abs(got[:, V]).max()) > 2 * FP16_MAX
        assert torch.equal(y[:, : 2 * N // 3], qk2), "Q / K differ between the out and the out_vt launch"
    for g in (2, 3):
        for i, name in enumerate(("out", "qk", "v^T")):
            assert _same_bits(outs[1][i], outs[g][i]), f"geometry {g} vs 1: {name} differs"


# ----------------------------------------------------------------------------- (b) non-finite activations through the quantiser
NAN, INF = float("nan"), float("inf")
# (row, group, {element inside the group: value}) -- rows on the tile seams (31 | 32: 32-row tiles, 255 | 256: row blocks) and on the last real row
POLLUTION = [
    (0, 0, {5: INF}),
    (31, 1, {63: -INF}),
    (32, 2, {0: NAN}),                          # one NaN among finite values
    (255, 3, {7: NAN, 40: INF}),                # NaN and inf together
    (256, 4, {j: NAN for j in range(64)}),      # an all-NaN group
    (299, 5, {33: -INF}),
    (299, 0, {1: NAN, 62: NAN}),
]
BAD_ROWS = sorted({r for r, _, _ in POLLUTION})


def _polluted_inputs(M, K, dtype, fuse_glu, seed=21):
    """(polluted input, the same with the polluted GROUPS zeroed, the same with only the non-finite ELEMENTS zeroed, logical [M, K] mask of polluted groups,
    mask of inf groups).  With fuse_glu the input holds (value, gate) pairs and the VALUES are polluted: value * silu(gate) is then non-finite."""
    if fuse_glu:
        x = O.round16(np.random.default_rng(seed).standard_normal((M, 2 * K)).astype(np.float32) * 1.5, dtype)
        col = lambda k: 2 * k
    else:
        x = O.make_activations(M, K, seed=seed, dtype=dtype)
        col = lambda k: k
    xp, xb, xz = x.copy(), x.copy(), x.copy()
    gmask = np.zeros((M, K // 64), bool)
    infmask = np.zeros((M, K // 64), bool)
    for r, g, cells in POLLUTION:
        gmask[r, g] = True
        for k in range(64 * g, 64 * g + 64):
            xb[r, col(k)] = 0.0
        for j, v in cells.items():
            xp[r, col(64 * g + j)] = v
            xz[r, col(64 * g + j)] = 0.0
            infmask[r, g] |= np.isinf(v)
    return xp, xb, xz, gmask, infmask


def _quantise(mod, x, dtype, fuse_glu):
    from nunchaku_amd import layout
    from nunchaku_amd.ops.quantize import svdq_quantize_w4a4_act_fuse_lora_cuda

    mod._ensure_layout()
    qx, asc, la = svdq_quantize_w4a4_act_fuse_lora_cuda(t16(x, dtype), lora_down=mod.proj_down, smooth=mod.smooth_factor, fuse_glu=fuse_glu)
    K = mod.in_features
    codes = layout.unpack_act(qx, K).cpu().numpy()
    scales = layout.unpack_scales(asc, codes.shape[0])
    torch.cuda.synchronize()
    return (qx, asc, la), codes, scales


@pytest.mark.parametrize("fuse_glu", [False, True], ids=["plain", "glu"])
@pytest.mark.parametrize("R", [32, 128], ids=["rank-32", "rank-128"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_quantiser_isolates_non_finite_groups(dtype, R, fuse_glu):
    """gemm_w4a4.cuh:455-497 / oracle.quantize_rows: a group holding +-inf has ascale inf and every code 0; a NaN element has code 0 and changes nothing else of
    its group (the maximum ignores it); an all-NaN group has ascale 0.  Everything that does not belong to a polluted (row, group) -- codes, scales, and the
    low-rank sums of every clean ROW -- is bit-identical to the run with those groups zeroed."""
    from nunchaku_amd import mode

    M, K = 300, 384
    L = O.make_svdq_layer(K, 128, R, seed=20 + R, dtype=dtype, cheap=True)
    mod = make_module(L, dtype)
    xp, xb, xz, gmask, infmask = _polluted_inputs(M, K, dtype, fuse_glu)
    with mode.deterministic_mode():  # the K-sliced low-rank sums are compared bit for bit
        (qx, asc, la), codes, scales = _quantise(mod, xp, dtype, fuse_glu)
        (qx2, asc2, la2), _, _ = _quantise(mod, xp, dtype, fuse_glu)
        (_, _, la_b), codes_b, scales_b = _quantise(mod, xb, dtype, fuse_glu)
        (_, _, la_z), codes_z, scales_z = _quantise(mod, xz, dtype, fuse_glu)
    (_, _, la32), _, _ = _quantise(mod, xp, dtype, fuse_glu)
    (_, _, la32_b), _, _ = _quantise(mod, xb, dtype, fuse_glu)
    assert torch.equal(qx, qx2) and torch.equal(asc.view(torch.int16), asc2.view(torch.int16)) and torch.equal(la, la2), "two calls differ"
    M_pad = codes.shape[0]
    assert M_pad == 512
    gm = np.zeros((M_pad, K // 64), bool)
    gm[:M] = gmask
    em = np.repeat(gm, 64, axis=1)
    sb, sb_b, sb_z = (s.view(torch.int16).cpu().numpy().T for s in (scales, scales_b, scales_z))   # [M_pad, G] raw bits
    # clean groups / rows: bit-identical to the baseline, nothing left out
    assert np.array_equal(codes[~em], codes_b[~em]), f"{(codes[~em] != codes_b[~em]).sum()} codes of clean groups changed"
    assert np.array_equal(sb[~gm], sb_b[~gm]), f"{(sb[~gm] != sb_b[~gm]).sum()} scales of clean groups changed"
    clean_rows = np.setdiff1d(np.arange(M_pad), BAD_ROWS)
    ci = torch.as_tensor(clean_rows, device=la.device)
    assert torch.equal(la[ci], la_b[ci]), "low-rank sums of clean rows changed"
    # padded rows stay zero
    assert not codes[M:].any() and not sb[M:].any() and not la[M:].any().item()
    # polluted groups: the oracle's scale and codes
    sc = f32(scales).T
    for r, g, cells in POLLUTION:
        grp = slice(64 * g, 64 * g + 64)
        if infmask[r, g]:
            assert sc[r, g] == INF, f"row {r} group {g}: ascale {sc[r, g]} for a group holding inf"
            assert not codes[r, grp].any(), f"row {r} group {g}: codes {codes[r, grp]} for a group holding inf (the reference: rcp(inf) = 0, inf * 0 = NaN -> code 0)"
        else:
            # NaN elements only: amax, scale and the other codes are those of the group with the NaN elements zeroed; the NaN element itself has code 0 (as the zero has)
            assert sb[r, g] == sb_z[r, g], f"row {r} group {g}: ascale {sc[r, g]} differs from the group without its NaN elements"
            assert np.array_equal(codes[r, grp], codes_z[r, grp]), f"row {r} group {g}: codes differ from the group without its NaN elements: {codes[r, grp]} vs {codes_z[r, grp]}"
            assert all(codes[r, 64 * g + j] == 0 for j in cells)
            if len(cells) == 64:
                assert sc[r, g] == 0.0
    if not fuse_glu:   # (the GLU front end's SiLU is held to +-1 code by test_quantize_fuse_glu, not to an envelope)
        # the oracle on the polluted input itself, through its approximation envelope (exact -- lo == hi -- for the inf groups and at the NaN elements)
        env = O.quantize_envelope(xp, L["smooth"], dtype)
        assert np.all(codes >= env["q_lo"]) and np.all(codes <= env["q_hi"]), "codes outside the oracle's envelope"
        assert np.all(sc[gm] >= env["s_lo"].T[gm]) and np.all(sc[gm] <= env["s_hi"].T[gm]), f"polluted groups' scales {sc[gm]} outside the oracle's [{env['s_lo'].T[gm]}, {env['s_hi'].T[gm]}]"
    else:
        # the oracle on value * silu(gate) of the polluted input: inf groups exactly; NaN-only groups within the GLU front end's own tolerance
        # (test_quantize_fuse_glu: the hardware SiLU may move an input one 16-bit step: codes +-1, scales one 16-bit step), code 0 at every NaN element
        q_ref, a_ref, _ = O.quantize_w4a4_act_fuse_lora(xp, L["smooth"], None, dtype, fuse_glu=True)
        for r, g, cells in POLLUTION:
            grp = slice(64 * g, 64 * g + 64)
            if infmask[r, g]:
                assert a_ref[g, r] == INF and not q_ref[r, grp].any()   # (what the GPU was held to above)
            else:
                assert np.abs(codes[r, grp].astype(int) - q_ref[r, grp].astype(int)).max() <= 1, f"row {r} group {g}: codes vs the oracle's"
                assert all(q_ref[r, 64 * g + j] == 0 for j in cells)
                assert abs(sc[r, g] - a_ref[g, r]) <= abs(a_ref[g, r]) * (2.0 ** -7 if dtype == "bf16" else 2.0 ** -10), f"row {r} group {g}: ascale {sc[r, g]} vs the oracle's {a_ref[g, r]}"
    # fp32 accumulators (the default mode): a non-finite element reaches the low-rank sums of ITS row only
    la32, la32_b = la32.cpu().numpy(), la32_b.cpu().numpy()
    assert not np.isfinite(la32[BAD_ROWS]).any(), "x @ lora_down of a row holding inf / NaN must be non-finite in every rank"
    assert np.isfinite(la32[clean_rows]).all()
    assert np.allclose(la32[clean_rows], la32_b[clean_rows], rtol=0, atol=4e-6 * float(np.abs(la32_b).max()) + 1e-7)


# ----------------------------------------------------------------------------- (c) non-finite rows through the GEMMs
def _rows_equal(a, b, rows, what):
    idx = torch.as_tensor(rows, device=a.device)
    assert _same_bits(a[idx], b[idx]), f"{what}: rows differ"


def _check_fp16_rows_against_oracle(got, ref, what, ulps=1.0, max_bad_frac=0.0):
    """rows of an fp16 output that held non-finite operands: no NaN, no inf; exactly +-65504 where the oracle's restated clamp gives it (NaN -> +65504); the
    rest within the usual bound"""
    assert np.isfinite(got).all(), f"{what}: inf or NaN stored in fp16"
    sat = np.abs(ref) == FP16_MAX
    assert np.array_equal(got[sat], ref[sat]), f"{what}: {(got[sat] != ref[sat]).sum()} of {sat.sum()} clamped elements differ from the oracle (got {np.unique(got[sat])})"
    if (~sat).any():
        assert_close_16(np.where(sat, 0, got), np.where(sat, 0, ref), "fp16", what, max_bad_frac=max_bad_frac, ulps=ulps)


@pytest.mark.parametrize("R", [32, 128], ids=["rank-32", "rank-128"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemm_epilogues_isolate_non_finite_rows(dtype, R):
    """The quantised tensors of a polluted input (and of its baseline with the polluted groups zeroed) through the plain, SiLU, GELU_QUANT and RMSNorm + RoPE
    launches of every geometry: rows (columns of out_vt) of clean tokens are bit-identical to the baseline run -- the scale tile, the bias and both low-rank
    projections are MFMAs, and an MFMA sums over its k-slots: inf * 0 = NaN must not reach another row's accumulator --; the polluted rows are the same in
    every kernel; in fp16 they hold no NaN and no inf and equal the oracle's restated clamp.

    The comparisons between launches run in deterministic mode (Q31.32 low-rank sums).  There the conversion stores 0 for a NaN partial sum and saturates an
    infinite one, so a row whose only pollution is a NaN element (row 32) comes out FINITE where the reference, with fp32 sums, gives NaN -> +65504: the
    polluted-row oracle check of that part feeds the oracle the library's own converted sums -- it pins the GEMM given its operands, not the reference's
    value for such a row.  The reference's value (every polluted row NaN before the clamp) is asserted in the default-mode part at the end, which is also
    where the wave-tile kernel runs (it takes fp32 sums only)."""
    from nunchaku_amd import layout, mode
    from nunchaku_amd.mode import alloc_lora_act
    from nunchaku_amd.ops.fused import fused_qkv_norm_rottary
    from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda

    M, K, N, Hd = 300, 384, 384, 512
    M_pad = 512
    L = O.make_svdq_layer(K, N, R, seed=40 + R, dtype=dtype, cheap=True)           # plain / SiLU / QKV (N = 3 x 128)
    L1 = O.make_svdq_layer(K, Hd, R, seed=41 + R, dtype=dtype, cheap=True)         # fc1 of a GELU MLP
    mod, fc1 = make_module(L, dtype), make_module(L1, dtype)
    fc2s = {r2: make_module(O.make_svdq_layer(Hd, K, r2, seed=42 + r2, dtype=dtype, cheap=True), dtype, act_unsigned=True) for r2 in (32, 64)}
    for m_ in (mod, fc1, *fc2s.values()):
        m_._ensure_layout()
    nq, nk = _norm_weights(dtype)
    rot, packed = _rot(M_pad)
    xp, xb, _, _, _ = _polluted_inputs(M, K, dtype, False)
    clean = np.setdiff1d(np.arange(M), BAD_ROWS)
    clean_pad = np.setdiff1d(np.arange(M_pad), BAD_ROWS)
    bad = np.array(BAD_ROWS)

    def launches(m, f1, qt, q1):
        qx, asc, la = qt
        plain = torch.empty(M, N, dtype=TORCH_DT[dtype], device="cuda")
        svdq_gemm_w4a4_cuda(act=qx, wgt=m.qweight, out=plain, ascales=asc, wscales=m.wscales, lora_act_in=la, lora_up=m.proj_up, bias=m.bias)
        from nunchaku_amd._C import ops
        plan_plain = ops.gemm_last_plan()
        silu = torch.empty(M, N, dtype=TORCH_DT[dtype], device="cuda")
        svdq_gemm_w4a4_cuda(act=qx, wgt=m.qweight, out=silu, ascales=asc, wscales=m.wscales, lora_act_in=la, lora_up=m.proj_up, bias=m.bias, fuse_silu=True)
        vt = torch.zeros(N // 3, M_pad, dtype=TORCH_DT[dtype], device="cuda")
        x_unused = torch.empty(1, M, K, dtype=TORCH_DT[dtype], device="cuda")
        qkv = fused_qkv_norm_rottary(x_unused, m, _W(nq, dtype), _W(nk, dtype), packed, quantized=qt)[0].clone()
        fused_qkv_norm_rottary(x_unused, m, _W(nq, dtype), _W(nk, dtype), packed, out_vt=vt[:, :M], quantized=qt)
        res = {"plain": plain, "silu": silu, "qkv": qkv, "vt": vt.T.contiguous()}   # (vt transposed: tokens are rows again)
        for r2, fc2 in fc2s.items():
            qh = torch.empty(layout.act_image_shape(M_pad, Hd), dtype=torch.uint8, device="cuda")
            sh = torch.empty(Hd // 64, M_pad, dtype=TORCH_DT[dtype], device="cuda")
            lh, zeroed = alloc_lora_act(M_pad, r2, "cuda")
            svdq_gemm_w4a4_cuda(act=q1[0], wgt=f1.qweight, qout=qh, ascales=q1[1], wscales=f1.wscales, oscales=sh, lora_act_in=q1[2], lora_up=f1.proj_up,
                                lora_down=fc2.proj_down, lora_act_out=lh, bias=f1.bias, smooth_factor=fc2.smooth_factor, lora_act_zeroed=zeroed)
            res[f"gelu{r2}_codes"] = layout.unpack_act(qh, Hd, unsigned=True)
            res[f"gelu{r2}_oscales"] = layout.unpack_scales(sh, M_pad).view(torch.int16).T.contiguous()
            res[f"gelu{r2}_lora_act_out"] = lh
        return res, plan_plain

    with mode.deterministic_mode():
        qt_p, qt_b = mod.quantize(t16(xp, dtype)), mod.quantize(t16(xb, dtype))
        q1_p, q1_b = fc1.quantize(t16(xp, dtype)), fc1.quantize(t16(xb, dtype))
        got = {}
        for g in (1, 2, 3, 6, 7):   # (the wave-tile kernel takes fp32 low-rank sums only: it runs in the default-mode part below)
            (res_p, plan), _ = _with_geometry(g, lambda: launches(mod, fc1, qt_p, q1_p))
            _check_plan(g, plan)
            (res_b, _), _ = _with_geometry(g, lambda: launches(mod, fc1, qt_b, q1_b))
            got[g] = res_p
            for name in res_p:
                rows = clean_pad if res_p[name].shape[0] == M_pad else clean
                _rows_equal(res_p[name], res_b[name], rows, f"geometry {g}, {name}: clean tokens vs the baseline run")
        for g in (2, 3, 6, 7):
            for name in got[1]:
                _rows_equal(got[1][name], got[g][name], bad, f"geometry {g} vs 1, {name}: polluted rows")
        # GELU_QUANT on a row that is NaN before the GELU (an infinite ascale): the requantiser's maximum ignores NaN -> oscale 0, every code 0
        # (oracle.quantize_rows; the kernel: v_max skips NaN, v_med3_f32(NaN, 0, 1) returns the minimum)
        inf_rows = torch.as_tensor(sorted({r for r, _, cells in POLLUTION if any(np.isinf(v) for v in cells.values())}), device="cuda")
        for g in got:
            for r2 in fc2s:
                assert not got[g][f"gelu{r2}_codes"][inf_rows].any().item(), f"geometry {g}, next rank {r2}: non-zero codes for a NaN row"
                assert not got[g][f"gelu{r2}_oscales"][inf_rows].any().item(), f"geometry {g}, next rank {r2}: non-zero oscales for a NaN row"
    if dtype == "fp16":
        codes = layout.unpack_act(qt_p[0], K).cpu().numpy()[bad]
        scales = f32(layout.unpack_scales(qt_p[1], M_pad))[:, bad]
        la = mode.lora_act_to_float(qt_p[2]).cpu().numpy()[bad]
        assert np.isinf(scales).any()
        kw = dict(dtype=dtype, bias=L["bias"], lora_act_in=la, lora_up=L["proj_up"])
        ref = O.gemm_w4a4(codes, scales, L["qweight"], L["wscales"], **kw)["out"]
        assert (ref == FP16_MAX).all(axis=1).any(), "expected at least one all-NaN row (an infinite ascale) in the oracle"
        _check_fp16_rows_against_oracle(f32(got[1]["plain"])[bad], ref, "plain, polluted rows")
        ref = O.gemm_w4a4(codes, scales, L["qweight"], L["wscales"], fuse="silu", **kw)["out"]
        _check_fp16_rows_against_oracle(f32(got[1]["silu"])[bad], ref, "SiLU, polluted rows", ulps=2.0)
        ref = O.gemm_w4a4(codes, scales, L["qweight"], L["wscales"], fuse="rmsnorm_rope", norm_q=nq, norm_k=nk, rot=rot[bad], **kw)["out"]
        _check_fp16_rows_against_oracle(f32(got[1]["qkv"])[bad], ref, "RMSNorm + RoPE, polluted rows", ulps=2.0, max_bad_frac=2e-3)
        _check_fp16_rows_against_oracle(f32(got[1]["vt"])[bad], ref[:, 2 * N // 3:], "V^T, polluted columns")
    # the default mode (fp32 low-rank sums: a polluted row's lora_act is NaN / inf and enters the up projection as such): plain epilogue, the 8-wave and
    # the wave-tile kernel.  Codes and scales are deterministic; the K-sliced fp32 low-rank sums of two quantiser runs are not, so the baseline launch reads
    # the POLLUTED run's lora_act with only the polluted rows replaced by the baseline's: every clean row has identical operand bits in both launches.
    qt32_p, qt32_b = mod.quantize(t16(xp, dtype)), mod.quantize(t16(xb, dtype))
    bad_t = torch.as_tensor(bad, device="cuda")
    la_spliced = qt32_p[2].clone()
    la_spliced[bad_t] = qt32_b[2][bad_t]
    assert bool(torch.isfinite(la_spliced).all()) and not bool(torch.isfinite(qt32_p[2][bad_t]).any())
    o32 = {}
    for g in (1, 8):
        o32[g], plan = _with_geometry(g, lambda: (mod.forward_quant(*qt32_p)[:M], mod.forward_quant(qt32_b[0], qt32_b[1], la_spliced)[:M]))
        _check_plan(g, plan, wave_tile_ok=(R == 32))
        _rows_equal(o32[g][0], o32[g][1], clean, f"default mode, geometry {g}: clean tokens vs the baseline run")
        assert np.isfinite(f32(o32[g][0])[clean]).all()
    assert _same_bits(o32[1][0], o32[8][0]), "default mode: geometry 8 vs 1"
    if dtype == "fp16":
        assert (f32(o32[1][0])[bad] == FP16_MAX).all(), "fp32 low-rank sums: every polluted row is NaN before the clamp, +65504 after it"
    else:
        assert np.isnan(f32(o32[1][0])[bad]).all()


# ----------------------------------------------------------------------------- (d) fp16 subnormal activation scales
def _subnormal_scale_case(shift):
    from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda

    dtype, M, K, N = "fp16", 300, 384, 256
    L = O.make_svdq_layer(K, N, 32, seed=11, dtype=dtype, cheap=True)
    L["wscales"] = O.round16(L["wscales"] * np.float32(2.0 ** 10), dtype)
    x = O.round16(O.make_activations(M, K, seed=11, dtype=dtype) * np.float32(2.0 ** -shift), dtype)
    a_ref = O.quantize_w4a4_act_fuse_lora(x, L["smooth"], None, dtype)[1][:, :M]
    sub = (a_ref != 0) & (np.abs(a_ref) < 2.0 ** -14)
    print(f"activations x 2^-{shift}: {sub.mean():.1%} of the ascales are fp16 subnormals, {(a_ref == 0).sum()} are zero")
    assert sub.mean() > 0.5 and not (a_ref == 0).any(), "precondition: most activation scales subnormal, none zero"
    mod = make_module(L, dtype)
    qx, asc, la = mod.quantize(t16(x, dtype))
    q, a = checked_codes(qx, asc, x, L["smooth"], dtype)
    ref = O.gemm_w4a4(q, a, L["qweight"], L["wscales"], dtype=dtype, bias=L["bias"], lora_act_in=la.cpu().numpy(), lora_up=L["proj_up"])["out"][:M]
    # the 4-bit branch must matter in the result: without it (ascales flushed to zero) the outputs are bias + low-rank only
    no4 = O.gemm_w4a4(q, np.zeros_like(a), L["qweight"], L["wscales"], dtype=dtype, bias=L["bias"], lora_act_in=la.cpu().numpy(), lora_up=L["proj_up"])["out"][:M]
    assert (np.abs(ref - no4) > 4 * 2.0 ** -10 * np.abs(ref)).mean() > 0.5, "precondition: the scaled 4-bit product is visible in the outputs"
    outs = {}
    for g in (1, 2, 8):
        out = torch.empty(M, N, dtype=TORCH_DT[dtype], device="cuda")
        _, plan = _with_geometry(g, lambda: svdq_gemm_w4a4_cuda(act=qx, wgt=mod.qweight, out=out, ascales=asc, wscales=mod.wscales, lora_act_in=la, lora_up=mod.proj_up,
                                                                 bias=mod.bias))
        _check_plan(g, plan)
        outs[g] = out
        assert_close_16(f32(out), ref, dtype, f"subnormal ascales (x 2^-{shift}), geometry {g}", max_bad_frac=0.0, ulps=1.0)
    assert torch.equal(outs[1], outs[2]) and torch.equal(outs[1], outs[8])


@pytest.mark.parametrize("shift", [14, 16])
def test_fp16_subnormal_activation_scales(shift):
    """ascale = fp16(amax / 7) is an fp16 subnormal when a group's amax is below 4.3e-4, and is then an operand of the scale-product MFMA: the hardware must
    honour it (the reference's HFMA2 chain does).  Quantiser inside its usual envelope, GEMM to 1 ulp of the float64 oracle, all kernels bit-identical."""
    _subnormal_scale_case(shift)


# ----------------------------------------------------------------------------- (e) fp16 weight scales at the scale image's limit
def _layer_with_largest_wscale(dtype, top):
    L = O.make_svdq_layer(384, 256, 32, seed=11, dtype=dtype, cheap=True)
    ws = O.round16(L["wscales"] * np.float32(2.0 ** 15), dtype)
    g, n = np.unravel_index(np.abs(ws).argmax(), ws.shape)
    assert float(np.abs(ws).max()) < top
    ws[g, n] = top   # (a weight scale is a free parameter of the layer: the oracle stays exact)
    L["wscales"] = ws
    return L, n


def _forward_matches_oracle(L, mod, dtype, col):
    M, K = 300, 384
    x = O.make_activations(M, K, seed=11, dtype=dtype)
    xt = t16(x, dtype)
    qx, asc, la = mod.quantize(xt)
    q, a = checked_codes(qx, asc, x, L["smooth"], dtype)
    ref = O.gemm_w4a4(q, a, L["qweight"], L["wscales"], dtype=dtype, bias=L["bias"], lora_act_in=la.cpu().numpy(), lora_up=L["proj_up"])["out"][:M]
    got = f32(mod.forward_quant(qx, asc, la))[:M]
    assert np.isfinite(got).all() or dtype == "bf16"
    assert_close_16(got, ref, dtype, "largest weight scale", max_bad_frac=0.0, ulps=1.0)
    assert_close_16(got[:, col], ref[:, col], dtype, "the column of the largest weight scale", max_bad_frac=0.0, ulps=1.0)


def test_fp16_weight_scale_limit_of_the_scale_image():
    """The weight-side scale image holds 32 x the scale (csrc/repack.hip): 32 x 2047 = 65504 is the last fp16 number.  A checkpoint whose largest fp16 scale is
    exactly 2047 loads and computes; 2048 loads (load_state_dict copies the checkpoint layout) and raises ValueError at the FIRST FORWARD, when the scale image
    is built -- never an inf in the image -- and the message names bfloat16, where the same layer works."""
    L, col = _layer_with_largest_wscale("fp16", 2047.0)
    mod = make_module(L, "fp16")
    _forward_matches_oracle(L, mod, "fp16", col)

    L, col = _layer_with_largest_wscale("fp16", 2048.0)
    mod = make_module(L, "fp16")     # loading succeeds
    x = t16(O.make_activations(300, 384, seed=11, dtype="fp16"), "fp16")
    with pytest.raises(ValueError, match="bfloat16"):
        mod(x.view(1, 300, 384))
    with pytest.raises(ValueError, match="bfloat16"):   # and again: a failed conversion leaves the module unconverted, not half-converted
        mod(x.view(1, 300, 384))

    L, col = _layer_with_largest_wscale("bf16", 2048.0)
    mod = make_module(L, "bf16")
    _forward_matches_oracle(L, mod, "bf16", col)
