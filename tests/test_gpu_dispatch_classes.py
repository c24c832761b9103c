"""Every dispatched instantiation of the small kernels around the GEMM: the row-per-wave kernels (residual_gate_stats, residual_diff,
modulated_diff: NV = ceil(C / 512)), the AWQ GEMV (M = 1 .. 8, both M = 1 paths, the batched form), the AWQ GEMM (BM = 32 / 64 / 128, every
K-split count) and the image-prompt attention (NKT = ceil(N / 32), the multi-tile loop).  Each picks one of many template instantiations
with a runtime switch on a shape class; the family modules (test_gpu_fused_norm, test_gpu_fbcache, test_gpu_teacache, test_gpu_awq,
test_gpu_awq_gemm, test_gpu_ip_attention) launch the classes FLUX at 1024 x 1024 needs, this module launches the rest with the same
assertions.  The case tables are module-level constants: tests/test_dispatch_ledger.py compares the classes they reach with the
instantiations the built library holds."""
import math

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests.helpers import TORCH_DT, assert_close_16, f32, t16

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "fp16")
U32 = 2.0 ** -24  # unit roundoff of fp32

# ---- the case tables ------------------------------------------------------------------------------------------------------------------
# row kernels: every NV the three launchers switch on, a full last pass and one with 25 live lanes
ROW_NV = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 32)
ROW_WIDTHS = tuple(c for nv in ROW_NV for c in (512 * nv, 512 * (nv - 1) + 200))
ROW_M = 6                 # one full workgroup + half of one
ROW_M_PAIR = (5, 6)       # grouped launches: the second problem starts at wave 1 of a workgroup, the last workgroup has a dead wave
ROW_LD_GAP = 24           # row-strided views: ld = C + 24
ROW_UNSUPPORTED = (4608, 8704, 16392)  # classes 9, 17, 33: refused, not rounded to a neighbouring kernel
# AWQ GEMV, single launches (M, N, K): N = 20 is no multiple of 16 (a partly filled last block), K = 576 is 9 chunks (a ragged second wave load),
# (64, 64) one chunk; M = 1 at the LDS limit K = 8192 and at the first K of the row-group path (129 chunks, 5 load batches, the last ragged)
GEMV_M = (1, 2, 3, 4, 5, 6, 7, 8)
GEMV_SHAPES = ((20, 576), (64, 64))
GEMV_SINGLE = tuple((m, n, k) for n, k in GEMV_SHAPES for m in GEMV_M) + ((1, 64, 8192), (1, 64, 8256))
GEMV_LDX_GAP = 8
GEMV_BATCHED_ENTRIES = ((20, 1), (64, 1), (36, 6), (1536, 6))  # (N, out_chunks): N = 20 in front fills its last block partly
GEMV_BATCHED_K = (256, 8256)
# AWQ GEMM (M, N, K, K-split count the planner must choose)
AWQ_GEMM_CASES = (
    (33, 192, 640, 1),     # BM 64, no split, ragged M, half an output tile
    (64, 128, 1152, 2),    # BM 64, 2 slices of 4 and 5 K-steps
    (40, 192, 2048, 4),    # BM 64, 4 slices, N % 128 == 64
    (8, 64, 8192, 16),     # BM 32, 16 slices
    (200, 192, 1152, 2),   # BM 128, ragged second row tile, 2 uneven slices
    (7, 64, 128, 1),       # one K-step
)
# image-prompt attention (T, H, N): NKT 3, 5 and 6, each with a ragged and a full last key tile
IP_CASES = ((48, 2, 70), (300, 2, 96), (256, 1, 130), (64, 2, 160), (300, 1, 161), (128, 2, 192))
IP_PROBE_COVERED = ((256, 2, 20), (256, 2, 40), (256, 2, 128), (256, 2, 200), (256, 2, 256))  # the selection probe on NKT 1, 2, 4, 7, 8
IP_MULTI_TILE = ((513, 200, 20), (513, 200, 161))  # (workgroups per head, tiles per workgroup) = (2, 2) and (1, 3)


@pytest.fixture(autouse=True)
def _need_gpu(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


# =======================================================================================================================================
# 1. row-per-wave kernels
# =======================================================================================================================================
GUARD = 2      # rows in front of and behind a problem inside its buffer
CONST_ROW = 2  # this row of every problem is the constant 3.0
NAN = float("nan")
SENTINEL = 7.0


def _embed(real: torch.Tensor, ld: int, fill: float):
    """``real`` [M, C] as rows [GUARD, GUARD + M), columns [0, C) of a [M + 2 GUARD, ld] buffer of ``fill`` -> (buffer, view of the problem)"""
    M, C = real.shape
    buf = torch.full((M + 2 * GUARD, ld), fill, dtype=real.dtype, device=real.device)
    view = buf[GUARD:GUARD + M, :C]
    view.copy_(real)
    return buf, view


def _outside_keeps(buf: torch.Tensor, M: int, C: int, fill: float) -> bool:
    """the gap columns and the guard rows of an ``_embed`` buffer still hold ``fill``"""
    outside = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    outside[GUARD:GUARD + M, :C] = False
    edge = buf[outside].float()
    return bool(torch.isnan(edge).all()) if math.isnan(fill) else bool((edge == fill).all())


def _ld(C: int, strided: bool) -> int:
    return C + ROW_LD_GAP if strided else C


def _row_inputs(M: int, C: int, dtype: str, seed: int):
    """res about 3 +- 0.5 (a wrong divisor, a missing tail mask or a one-pass variance shows in the statistics), a, b about +- 0.3, gate
    about +- 1; row CONST_ROW of res is 3.0 and of a, b is 0: y = 3.0 there whatever the gate"""
    rng = np.random.default_rng(seed)
    res = O.round16((3.0 + 0.5 * rng.standard_normal((M, C))).astype(np.float32), dtype)
    a = O.round16((0.3 * rng.standard_normal((M, C))).astype(np.float32), dtype)
    b = O.round16((0.3 * rng.standard_normal((M, C))).astype(np.float32), dtype)
    gate = O.round16(rng.standard_normal(C).astype(np.float32), dtype)
    res[CONST_ROW], a[CONST_ROW], b[CONST_ROW] = 3.0, 0.0, 0.0
    return res, a, b, gate


def _stats_ratios(stats: torch.Tensor, y16: np.ndarray, what: str, eps: float = 1e-6):
    """The statistics of residual_kernel against the float64 mean and rstd of the stored 16-bit ``y16`` [M, C].

    Bound, from the summation depth (csrc/residual.hip), u = 2^-24, NV = ceil(C / 512), first order in u:
      * mean: a lane adds its 8 NV values in sequence, 6 butterfly levels fold the wave: a term passes through at most 8 NV + 6 additions, so
        |sum - sum64| <= (8 NV + 6) u sum|y|; the division by C rounds once more, one unit covers the second-order terms:
        |mean - mean64| <= (8 NV + 8) u mean|y|.
      * rstd: d = y - mean rounds once (u), d * d is formed inside the fma (no rounding of its own), the fma chain and the butterfly are
        again 8 NV + 6 roundings; the error of the mean shifts every d by the same delta, and because sum d = 0 it reaches sum d^2 only
        as C delta^2: second order.  So sum d^2 is off by at most (2 + 8 NV + 6) u, the division by C and the addition of eps add one each:
        (8 NV + 10) u on var + eps, halved by the square root, plus the roundings of sqrtf and of the division: (4 NV + 7) u.  The
        asserted bound is the looser (8 NV + 12) u.  Lanes beyond C add exact zeros to both sums.
    The constant row: every d is 0, so rstd must be 1 / sqrt(eps) up to the roundings of sqrtf and the division: within 2 fp32 steps.
    -> (worst mean error / bound, worst rstd error / bound)"""
    M, C = y16.shape
    nv = math.ceil(C / 512)
    got = stats.cpu().numpy().astype(np.float64)
    y = y16.astype(np.float64)
    mean64 = y.mean(axis=1)
    rstd64 = 1.0 / np.sqrt(((y - mean64[:, None]) ** 2).mean(axis=1) + float(np.float32(eps)))
    mean_ratio = (np.abs(got[:, 0] - mean64) / ((8 * nv + 8) * U32 * np.abs(y).mean(axis=1))).max()
    rstd_ratio = (np.abs(got[:, 1] / rstd64 - 1.0) / ((8 * nv + 12) * U32)).max()
    assert np.isfinite(got).all() and mean_ratio <= 1.0, f"{what}: mean off by {mean_ratio:.3g} x the bound (8 NV + 8) 2^-24 mean|y|"
    assert rstd_ratio <= 1.0, f"{what}: rstd off by {rstd_ratio:.3g} x the bound (8 NV + 12) 2^-24"
    assert np.array_equal(y16[CONST_ROW], np.full(C, 3.0, np.float32)) and got[CONST_ROW, 0] == 3.0, f"{what}: the constant row"
    const = 1.0 / math.sqrt(eps)
    assert abs(got[CONST_ROW, 1] - const) <= 2 * float(np.spacing(np.float32(const))), f"{what}: constant row: rstd {got[CONST_ROW, 1]!r}"
    return float(mean_ratio), float(rstd_ratio)


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "row-strided"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_gate_stats_every_width_class(dtype, strided):
    """residual_kernel<DT, NV> at every NV, a full and a ragged last pass each, M = 6: with b and gate (out of place, the scratch-clearing
    side job riding along), with gate alone (in place), statistics only.  The assertions of test_gpu_fused_norm.test_residual_gate_stats,
    the statistics held to the derived bound of ``_stats_ratios``."""
    from nunchaku_amd._C import ops

    worst = [0.0, 0.0]
    for C in ROW_WIDTHS:
        M, ld = ROW_M, _ld(C, strided)
        res, a, b, gate = _row_inputs(M, C, dtype, seed=C)
        tg = t16(gate, dtype)
        what = f"{dtype} C={C} ld={ld}"
        # ---- res + gate * (a + b), out of place, + the side job ----
        (rbuf, rv), (abuf, av), (bbuf, bv) = (_embed(t16(x, dtype), ld, NAN) for x in (res, a, b))
        obuf, ov = _embed(torch.zeros(M, C, dtype=TORCH_DT[dtype], device="cuda"), ld, SENTINEL)
        stats = torch.full((M, 2), NAN, device="cuda")
        scratch = torch.full((1000,), SENTINEL, device="cuda")
        ops.residual_gate_stats(rv, av, bv, tg, ov, stats, 1e-6, scratch)
        ref = O.residual_gate_ref(res, a, gate, b, dtype)
        assert np.array_equal(f32(ov), ref), f"{what}: {int((f32(ov) != ref).sum())} elements differ from residual_gate_ref"
        assert torch.equal(ov, t16(res, dtype) + tg[None] * (t16(a, dtype) + t16(b, dtype))), f"{what}: differs from the torch op sequence"
        assert _outside_keeps(obuf, M, C, SENTINEL) and all(_outside_keeps(x, M, C, NAN) for x in (rbuf, abuf, bbuf)), what
        assert np.array_equal(f32(rv), res), f"{what}: res is only read when out is another buffer"
        assert not scratch.any(), f"{what}: the scratch buffer was not cleared"
        ratios = [_stats_ratios(stats, ref, what + " (a + b)")]
        # ---- res + gate * a, in place ----
        rbuf, rv = _embed(t16(res, dtype), ld, NAN)
        stats = torch.full((M, 2), NAN, device="cuda")
        ops.residual_gate_stats(rv, av, None, tg, rv, stats)
        ref = O.residual_gate_ref(res, a, gate, None, dtype)
        assert np.array_equal(f32(rv), ref) and torch.equal(rv, t16(res, dtype) + tg[None] * t16(a, dtype)), f"{what}: in place, no b"
        assert _outside_keeps(rbuf, M, C, NAN) and _outside_keeps(abuf, M, C, NAN), what
        ratios.append(_stats_ratios(stats, ref, what + " (a)"))
        # ---- statistics only ----
        stats = torch.full((M, 2), NAN, device="cuda")
        ops.residual_gate_stats(rv, None, None, None, None, stats)
        assert np.array_equal(f32(rv), ref) and _outside_keeps(rbuf, M, C, NAN), f"{what}: statistics only must not write"
        ratios.append(_stats_ratios(stats, ref, what + " (statistics only)"))
        worst = [max(worst[0], *(r[0] for r in ratios)), max(worst[1], *(r[1] for r in ratios))]
    print(f"residual_gate_stats {dtype} {'row-strided' if strided else 'contiguous'}: worst error / bound: mean {worst[0]:.3f}, rstd {worst[1]:.3f}")


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "row-strided"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_gate_stats_grouped_every_width_class(dtype, strided):
    """The grouped launch (two problems, M = 5 and M2 = 6: the second problem's first row is wave 1 of workgroup 1, wave 3 of the last
    workgroup has no row) at every NV, in place, with the side job."""
    from nunchaku_amd._C import ops

    worst = [0.0, 0.0]
    for C in ROW_WIDTHS:
        ld = _ld(C, strided)
        tensors, refs = [], []
        for i, M in enumerate(ROW_M_PAIR):
            res, a, _, gate = _row_inputs(M, C, dtype, seed=2 * C + i)
            rbuf, rv = _embed(t16(res, dtype), ld, NAN)
            abuf, av = _embed(t16(a, dtype), ld, NAN)
            tensors.append((rbuf, rv, abuf, av, t16(gate, dtype), torch.full((M, 2), NAN, device="cuda")))
            refs.append(O.residual_gate_ref(res, a, gate, None, dtype))
        (_, r1, _, a1, g1, s1), (_, r2, _, a2, g2, s2) = tensors
        scratch = torch.full((64,), SENTINEL, device="cuda")
        ops.residual_gate_stats(r1, a1, None, g1, r1, s1, 1e-6, scratch, second=(r2, a2, None, g2, r2, s2))
        for (rbuf, rv, abuf, _, _, st), ref, M in zip(tensors, refs, ROW_M_PAIR):
            what = f"{dtype} C={C} ld={ld} problem of {M} rows"
            assert np.array_equal(f32(rv), ref), f"{what}: {int((f32(rv) != ref).sum())} elements differ from residual_gate_ref"
            assert _outside_keeps(rbuf, M, C, NAN) and _outside_keeps(abuf, M, C, NAN), what
            r = _stats_ratios(st, ref, what)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
        assert not scratch.any()
    print(f"residual_gate_stats grouped {dtype} {'row-strided' if strided else 'contiguous'}: worst error / bound: mean {worst[0]:.3f}, rstd {worst[1]:.3f}")


def _check_record(rec: list, diff_terms: torch.Tensor, prev_terms: torch.Tensor, rows: int, C: int, dt, what: str) -> float:
    """The record of a residual_diff / modulated_diff launch (sum_diff, sum_prev, mean_diff, mean_prev, ratio): the sums within
    tree_depth(rows, C) * 2^-24 of the float64 sums of the same 16-bit terms, the derived 16-bit values reproduced from the kernel's own sums.
    -> worst error / bound"""
    from tests.test_gpu_fbcache import tree_depth

    bound = tree_depth(rows, C) * U32
    worst = 0.0
    for got, terms, key in ((rec[0], diff_terms, "sum_diff"), (rec[1], prev_terms, "sum_prev")):
        r64 = terms.double().sum().item()
        rel = abs(got - r64) / r64
        worst = max(worst, rel / bound)
        assert math.isfinite(got) and rel <= bound, f"{what} {key}: kernel {got!r} float64 {r64!r}: relative error {rel:.3e} > {bound:.3e}"
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(rows * C), dtype=torch.float32)
    md = (torch.tensor(rec[0], dtype=torch.float32) * inv).to(dt)
    mp = (torch.tensor(rec[1], dtype=torch.float32) * inv).to(dt)
    assert rec[2] == md.item() and rec[3] == mp.item() and rec[4] == (md / mp).item(), f"{what}: derived means / ratio {rec}"
    return worst


def _diff_inputs(M: int, C: int, dtype: str, seed: int):
    """prev about 3 +- 0.5 (row CONST_ROW: 3.0), base about +- 2, cur = base + prev + 5 % noise, all 16-bit values as torch tensors"""
    rng = np.random.default_rng(seed)
    prev = (3.0 + 0.5 * rng.standard_normal((M, C))).astype(np.float32)
    prev[CONST_ROW] = 3.0
    prev = t16(O.round16(prev, dtype), dtype)
    base = t16(O.round16((2.0 * rng.standard_normal((M, C))).astype(np.float32), dtype), dtype)
    noise = torch.from_numpy((0.05 * rng.standard_normal((M, C))).astype(np.float32)).cuda()
    cur = base + (prev.float() + noise).to(prev.dtype)
    return prev, base, cur


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "row-strided"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_diff_every_width_class(dtype, strided):
    """residual_diff_kernel<DT, NV> at every NV, a full and a ragged last pass each, one problem of 6 rows and two of 5 and 6: the
    assertions of test_gpu_fbcache.test_residual_diff_kernel_vs_torch_sequence, and out_res aliasing cur."""
    from nunchaku_amd._C import ops

    dt = TORCH_DT[dtype]
    worst = 0.0
    for C in ROW_WIDTHS:
        ld = _ld(C, strided)
        for Ms in ((ROW_M,), ROW_M_PAIR):
            rows = sum(Ms)
            what = f"{dtype} C={C} ld={ld} rows={Ms}"
            probs = [_diff_inputs(M, C, dtype, seed=3 * C + 7 * i + len(Ms)) for i, M in enumerate(Ms)]

            def launch(alias_cur=False):
                views, bufs = [], []
                for prev, base, cur in probs:
                    M = prev.shape[0]
                    (pb, pv), (bb, bv), (cb, cv) = (_embed(x, ld, NAN) for x in (prev, base, cur))
                    ob, ov = (cb, cv) if alias_cur else _embed(torch.zeros_like(cur), ld, SENTINEL)
                    views.append((cv, bv, pv, ov))
                    bufs.append((M, pb, bb, cb, ob))
                partials = torch.full((rows, 2), NAN, device="cuda")
                result = torch.full((8,), NAN, device="cuda")
                ops.residual_diff(*views[0], partials=partials, result=result, second=views[1] if len(views) == 2 else None)
                return views, bufs, result

            views, bufs, result = launch()
            for (prev, base, cur), (cv, bv, pv, ov), (M, pb, bb, cb, ob) in zip(probs, views, bufs):
                assert torch.equal(ov, cur - base), f"{what}: out_res differs from torch's 16-bit subtraction"
                assert _outside_keeps(ob, M, C, SENTINEL) and all(_outside_keeps(x, M, C, NAN) for x in (pb, bb, cb)), what
                assert torch.equal(cv, cur) and torch.equal(pv, prev) and torch.equal(bv, base), f"{what}: the inputs are only read"
            diff_terms = torch.cat([(prev - (cur - base)).abs() for prev, base, cur in probs])
            prev_terms = torch.cat([prev.abs() for prev, _, _ in probs])
            worst = max(worst, _check_record(result[:5].tolist(), diff_terms, prev_terms, rows, C, dt, what))
            # bit-reproducible from launch to launch; out_res may alias cur
            views2, _, result2 = launch()
            assert torch.equal(result.view(torch.int32), result2.view(torch.int32)), f"{what}: two launches differ"
            assert all(torch.equal(v[3], w[3]) for v, w in zip(views, views2)), f"{what}: two launches differ"
            views3, bufs3, result3 = launch(alias_cur=True)
            assert torch.equal(result.view(torch.int32)[:5], result3.view(torch.int32)[:5]), f"{what}: out_res = cur changes the record"
            for v, w, (M, _, _, cb, _) in zip(views, views3, bufs3):
                assert torch.equal(v[3], w[3]) and _outside_keeps(cb, M, C, NAN), f"{what}: out_res = cur"
    print(f"residual_diff {dtype} {'row-strided' if strided else 'contiguous'}: worst sum error / (tree_depth * 2^-24): {worst:.3f}")


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "row-strided"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_modulated_diff_every_width_class(dtype, strided):
    """modulated_diff_kernel<DT, NV> at every NV, a full and a ragged last pass each, on the statistics residual_kernel<DT, NV> produced for the same
    view: the assertions of test_gpu_teacache.test_modulated_diff_kernel."""
    from nunchaku_amd._C import ops

    dt = TORCH_DT[dtype]
    worst = 0.0
    for C in ROW_WIDTHS:
        M, ld = ROW_M, _ld(C, strided)
        what = f"{dtype} C={C} ld={ld}"
        rng = np.random.default_rng(5 * C + 1)
        x_np = (3.0 + 0.5 * rng.standard_normal((M, C))).astype(np.float32)
        x_np[CONST_ROW] = 3.0
        x_np = O.round16(x_np, dtype)
        scale_np = O.round16(1 + 0.3 * rng.standard_normal(C).astype(np.float32), dtype)
        shift_np = O.round16(0.5 * rng.standard_normal(C).astype(np.float32), dtype)
        scale, shift = t16(scale_np, dtype), t16(shift_np, dtype)
        xbuf, xv = _embed(t16(x_np, dtype), ld, NAN)
        stats = torch.full((M, 2), NAN, device="cuda")
        ops.residual_gate_stats(xv, None, None, None, None, stats)
        _stats_ratios(stats, x_np, what + " (the statistics handed on)")
        ref = O.ln_mod_ref(x_np, stats.cpu().numpy(), scale_np, shift_np, dtype)
        m_ref = t16(ref, dtype)
        noise = torch.from_numpy((0.05 * rng.standard_normal((M, C))).astype(np.float32)).cuda()
        prev = (m_ref.float() + noise).to(dt)

        def launch(in_place=False):
            pbuf, pv = _embed(prev, ld, NAN)
            obuf, ov = (pbuf, pv) if in_place else _embed(torch.zeros_like(prev), ld, SENTINEL)
            partials = torch.full((M, 2), NAN, device="cuda")
            result = torch.full((8,), NAN, device="cuda")
            ops.modulated_diff(xv, stats, scale, shift, pv, ov, partials=partials, result=result)
            return pbuf, pv, obuf, ov, result

        pbuf, pv, obuf, ov, result = launch()
        assert np.array_equal(f32(ov), ref), f"{what}: {int((f32(ov) != ref).sum())} of {ref.size} elements differ from ln_mod_ref"
        assert _outside_keeps(obuf, M, C, SENTINEL) and _outside_keeps(xbuf, M, C, NAN) and _outside_keeps(pbuf, M, C, NAN), what
        assert torch.equal(pv, prev) and np.array_equal(f32(xv), x_np), f"{what}: x and prev are only read"
        worst = max(worst, _check_record(result[:5].tolist(), (prev - m_ref).abs(), prev.abs(), M, C, dt, what))
        _, _, _, ov2, result2 = launch()
        assert torch.equal(result.view(torch.int32), result2.view(torch.int32)) and torch.equal(ov, ov2), f"{what}: two launches differ"
        ibuf, iv, _, _, result3 = launch(in_place=True)  # out is prev: the buffer the engine keeps across steps
        assert torch.equal(result.view(torch.int32)[:5], result3.view(torch.int32)[:5]), f"{what}: out_mod = prev changes the record"
        assert torch.equal(iv, ov) and _outside_keeps(ibuf, M, C, NAN), f"{what}: out_mod = prev"
    print(f"modulated_diff {dtype} {'row-strided' if strided else 'contiguous'}: worst sum error / (tree_depth * 2^-24): {worst:.3f}")


def test_row_kernels_refuse_unsupported_widths():
    """A width whose class has no instantiation raises instead of launching a neighbouring kernel (classes 9, 17, 33: NotImplementedError from
    all three ops); C = 12 (no multiple of 8) and ld = C + 4 raise ValueError.  Nothing is written."""
    from nunchaku_amd._C import ops

    dt = torch.bfloat16

    def calls(M, C, ld):
        buf = lambda fill: torch.full((M, ld), fill, dtype=dt, device="cuda")
        x, a, p = buf(1.0), buf(1.0), buf(1.0)
        out = buf(SENTINEL)
        vec = torch.ones(C, dtype=dt, device="cuda")
        stats = torch.full((M, 2), SENTINEL, device="cuda")
        partials, result = torch.full((M, 2), SENTINEL, device="cuda"), torch.full((8,), SENTINEL, device="cuda")
        v = lambda t: t[:, :C]
        watched = (out, stats, partials, result)
        return watched, [
            ("residual_gate_stats", lambda: ops.residual_gate_stats(v(x), v(a), None, vec, v(out), stats)),
            ("residual_diff", lambda: ops.residual_diff(v(x), v(a), v(p), v(out), partials=partials, result=result)),
            ("modulated_diff", lambda: ops.modulated_diff(v(x), stats, vec, vec, v(p), v(out), partials=partials, result=result)),
        ]

    for C, ld, exc in [(C, C, NotImplementedError) for C in ROW_UNSUPPORTED] + [(12, 16, ValueError), (512, 516, ValueError)]:
        watched, fns = calls(ROW_M, C, ld)
        for name, fn in fns:
            with pytest.raises(exc):
                fn()
            torch.cuda.synchronize()
            assert all(bool((t == SENTINEL).all()) for t in watched), f"{name} C={C} ld={ld}: a refused call wrote"


# =======================================================================================================================================
# 2. AWQ GEMV
# =======================================================================================================================================
def _w16_table(q, s, z, dtype) -> np.ndarray:
    """[N, K] float32: the dequantised 16-bit weights, the first step of oracle.awq_gemv_w4a16 (one exact fma, one rounding)"""
    sc = np.repeat(s.T.astype(np.float64), O.AWQ_GROUP, axis=1)
    zz = np.repeat(z.T.astype(np.float64), O.AWQ_GROUP, axis=1)
    return O.round16(q.astype(np.float64) * sc + zz, dtype)


def _edge_targets(K: int, step: int):
    """the first and the last column of every ``step``-wide piece of K"""
    return [c * step + e for c in range(K // step) for e in (0, step - 1)]


def _gemv_x(rows: torch.Tensor, K: int, strided: bool) -> torch.Tensor:
    """the [M, K] activations of one launch, contiguous or as a view with row stride K + GEMV_LDX_GAP whose gap holds NaN"""
    if not strided:
        return rows.contiguous()
    buf = torch.full((rows.shape[0], K + GEMV_LDX_GAP), NAN, dtype=rows.dtype, device=rows.device)
    buf[:, :K] = rows
    return buf[:, :K]


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_awq_every_m_and_both_single_row_paths(dtype):
    """gemv_awq_kernel<DT, M> for M = 1 .. 8 at a ragged-N, nine-chunk shape and a one-chunk shape, M = 1 at the LDS limit (K = 8192) and on the
    row-group path behind it (K = 8256), with and without bias, x contiguous and (M > 1) row-strided.
    Exact probe: row m of x is the one-hot e_k with value 1.0 -- out[m, n] is then one product, nothing for the summation order to change, and
    must be the oracle's w16[n, k] (+ bias, one 16-bit add) BIT FOR BIT; over a few launches k visits the first and the last channel of every
    64-channel chunk.  Random parity: test_gpu_awq's gate (at most 2 % of the elements differ, none by more than one 16-bit step)."""
    from nunchaku_amd.ops.gemv import awq_gemv_w4a16_cuda
    from tests.test_gpu_awq import _layer

    worst = 0.0
    for m, N, K in GEMV_SINGLE:
        q, s, z, bias = _layer(N, K, dtype, seed=N + K + m)
        kern = torch.from_numpy(O.pack_awq_w4_ref(q)).cuda()
        ts, tz, tb = t16(s, dtype), t16(z, dtype), t16(bias, dtype)
        w16 = _w16_table(q, s, z, dtype)
        tw = t16(w16, dtype)
        targets = _edge_targets(K, O.AWQ_GROUP)
        launches = math.ceil(len(targets) / m)
        ks = torch.tensor([targets[i % len(targets)] for i in range(launches * m)], device="cuda")
        onehot = torch.zeros(launches * m, K, dtype=TORCH_DT[dtype], device="cuda")
        onehot[torch.arange(launches * m, device="cuda"), ks] = 1.0
        x_rand = O.round16(np.random.default_rng(7 + m).standard_normal((m, K)).astype(np.float32), dtype)
        for with_bias in (False, True):
            b = tb if with_bias else None
            for strided in ((False, True) if m > 1 else (False,)):
                what = f"{dtype} M={m} N={N} K={K} bias={with_bias} strided={strided}"
                outs = [awq_gemv_w4a16_cuda(_gemv_x(onehot[i * m:(i + 1) * m], K, strided), kern, ts, tz, m, N, K, bias=b) for i in range(launches)]
                got = torch.cat(outs)
                ref = tw.t()[ks]
                ref = ref + tb if with_bias else ref
                assert got.shape == ref.shape and torch.equal(got, ref), \
                    f"{what}: one-hot probe: {int((got != ref).sum())} of {ref.numel()} outputs are not the oracle's dequantised weight"
                if K <= 576:  # ... which is what the oracle itself gives for these rows
                    first = O.awq_gemv_w4a16(f32(onehot[:m]), q, s, z, dtype, bias=bias if with_bias else None)
                    assert np.array_equal(f32(ref[:m]), first), what
                y = awq_gemv_w4a16_cuda(_gemv_x(t16(x_rand, dtype), K, strided), kern, ts, tz, m, N, K, bias=b)
                ref = O.awq_gemv_w4a16(x_rand, q, s, z, dtype, bias=bias if with_bias else None)
                frac = float((f32(y) != ref).mean())
                worst = max(worst, frac / 0.02)
                assert frac <= 0.02, f"{what}: {frac:.4f} of the outputs differ from the oracle"
                assert_close_16(f32(y), ref, dtype, what)
    print(f"gemv_awq {dtype}: one-hot probes bit-exact; random parity: worst share of differing outputs / 0.02: {worst:.3f}, none beyond 1 ulp")


def _cheap_gemv_layer(N: int, K: int, dtype: str, seed: int):
    """an AWQW4A16Linear with random codes, scales in [0.004, 0.03) and integer zero points (no quantisation pass: N x K may be large)"""
    from nunchaku_amd.models.linear import AWQW4A16Linear

    rng = np.random.default_rng(seed)
    q = rng.integers(0, 16, size=(N, K)).astype(np.uint8)
    s = O.round16((0.004 + 0.026 * rng.random((K // 64, N))).astype(np.float32), dtype)
    z = O.round16(-(rng.integers(0, 16, size=(K // 64, N)).astype(np.float32) * s), dtype)
    bias = O.round16(rng.standard_normal(N).astype(np.float32) * 0.1, dtype)
    lin = AWQW4A16Linear(K, N, torch_dtype=TORCH_DT[dtype], device="cuda")
    lin.load_state_dict({"qweight": torch.from_numpy(O.pack_awq_w4_ref(q)), "wscales": t16(s, dtype), "wzeros": t16(z, dtype), "bias": t16(bias, dtype)})
    return lin


@pytest.mark.parametrize("K", GEMV_BATCHED_K)
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_awq_batched_ragged_entry_and_row_group_path(dtype, K):
    """gemv_awq_batched_kernel with an entry in front whose N = 20 fills its last block partly (the block-ownership scan must still hand the
    next entry its first block), on the LDS path (K = 256) and on the row-group path (K = 8256): every entry equals its single launch bit for
    bit, and the single launch of the small entries is the kernel the test above pins to the oracle."""
    from nunchaku_amd.ops.gemv import awq_gemv_w4a16_batched

    layers = []
    for i, (N, chunks) in enumerate(GEMV_BATCHED_ENTRIES):
        lin = _cheap_gemv_layer(N, K, dtype, seed=300 + i)
        lin.out_chunks = chunks
        layers.append(lin)
    x = t16(np.random.default_rng(K).standard_normal((1, K)).astype(np.float32), dtype)
    outs = awq_gemv_w4a16_batched(x, layers)
    assert len(outs) == len(layers)
    for lin, o in zip(layers, outs):
        single = lin(x)
        assert o.shape == single.shape and torch.isfinite(o.float()).all()
        assert torch.equal(o, single), f"{dtype} K={K} entry N={lin.out_features}: batched launch differs from the single launch"


# =======================================================================================================================================
# 3. AWQ GEMM
# =======================================================================================================================================
def awq_gemm_layer(N: int, K: int, dt, seed: int, device="cuda"):
    """test_gpu_awq_gemm.make_layer drawn from a CPU generator (the two-hot probe's exactness share is checked on the host for the same
    seeds): random codes, scales in [0.004, 0.03), zeros = -z * scale with z in [0, 16) -> the checkpoint buffers on ``device``"""
    from nunchaku_amd.models.text_encoders.tinychat_utils import _pack_codes

    g = torch.Generator().manual_seed(seed)
    G = K // 128
    codes = torch.randint(0, 16, (N, K), generator=g)
    s = (torch.rand(G, N, generator=g) * 0.026 + 0.004).to(dt)
    z = -(torch.randint(0, 16, (G, N), generator=g).float() * s.float()).to(dt)
    return _pack_codes(codes).to(device), s.to(device), z.to(device)


def awq_gemm_slices(K: int, splits: int):
    """the K-step ranges [kb0, kb1) of the slices of gemm_awq_kernel (restated: kb0 = sl * KS / splits, integer division)"""
    KS = K // 128
    return [(sl * KS // splits, (sl + 1) * KS // splits) for sl in range(splits)]


def awq_gemm_two_hot(w16: torch.Tensor, M: int, K: int, splits: int, shift: int = 0):
    """x[m] = e_k1 + e_k2 with k1 and k2 in different K-slices (one slice: in different K-steps; one K-step: two columns of it); row m takes the
    pair of index m + shift, so launches with shift = 0, M, 2 M, ... below the number of slices start a pair in every slice.
    -> x [M, K] in the dtype of w16, the float64 sums w16[n, k1] + w16[n, k2] as [M, N], the mask of the elements whose fp32 sum is exact"""
    sl = awq_gemm_slices(K, splits) if splits > 1 else [(kb, kb + 1) for kb in range(K // 128)]
    m = torch.arange(M)
    k1, k2 = torch.empty(M, dtype=torch.long), torch.empty(M, dtype=torch.long)
    L = len(sl)
    for row in range(M):  # pair r: piece r mod L and the piece 1 .. L - 1 further on (every pair of neighbours, then wider pairs)
        r = row + shift
        a = sl[r % L]
        b = sl[(r + 1 + (r // L) % (L - 1)) % L] if L > 1 else a
        k1[row] = a[0] * 128 + (37 * r) % ((a[1] - a[0]) * 128)
        k2[row] = b[0] * 128 + (53 * r + 11) % ((b[1] - b[0]) * 128)
        if k2[row] == k1[row]:
            k2[row] = b[0] * 128 + (k2[row] - b[0] * 128 + 1) % ((b[1] - b[0]) * 128)
    x = torch.zeros(M, K, dtype=w16.dtype, device=w16.device)
    x[m, k1], x[m, k2] = 1.0, 1.0
    ref64 = w16.double().t()[k1.to(w16.device)] + w16.double().t()[k2.to(w16.device)]
    return x, ref64, ref64 == ref64.float().double()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,splits", AWQ_GEMM_CASES)
def test_awq_gemm_tile_and_split_classes(dtype, M, N, K, splits):
    """gemm_awq_kernel<DT, 64> (never launched before), every K-split count the planner can choose (1, 2, 4, 8 is in test_gpu_awq_gemm, 16),
    slices of unequal length, the reduce kernel with bias on N % 128 == 64.
    One-hot probe: x[m] = e_k, out[m, n] = w16[n, k] (+ bias: the 16-bit add) bit for bit, k visiting the first and the last column of every
    K-step.  Two-hot probe: x[m] = e_k1 + e_k2 across two K-slices, out = round16(w16[n, k1] + w16[n, k2]) bit for bit wherever that fp32 sum
    is exact (all but < 1 %): a slice the reduce kernel drops, doubles or takes from a neighbour shows.  Then the random parity, fused bias and
    reproducibility assertions of test_gpu_awq_gemm."""
    from nunchaku_amd import _lib
    from tests.test_awq_gemm_host import dequantise
    from tests.test_gpu_awq_gemm import gemm

    dt = TORCH_DT[dtype]
    planned = int(_lib.load().svdq_gemm_awq_workspace_bytes(M, N, K)) // (4 * M * N) or 1
    assert planned == splits, f"the planner splits ({M}, {N}, {K}) {planned} ways, this case is meant for {splits}: move the case, do not empty it"
    assert all(b > a for a, b in awq_gemm_slices(K, splits))
    qw, sc, zr = awq_gemm_layer(N, K, dt, seed=M + N + K)
    w16 = dequantise(qw, sc, zr, K)  # [N, K] on the device
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.1).to(dt).cuda()
    # ---- one-hot ----
    targets = _edge_targets(K, 128)
    for launch in range(math.ceil(len(targets) / M)):
        ks = torch.tensor([targets[(launch * M + m) % len(targets)] for m in range(M)], device="cuda")
        x = torch.zeros(M, K, dtype=dt, device="cuda")
        x[torch.arange(M, device="cuda"), ks] = 1.0
        ref = w16.t()[ks]
        for b, r in ((None, ref), (bias, ref + bias)):
            got = gemm(x, qw, sc, zr, bias=b)
            assert torch.equal(got, r), f"one-hot launch {launch} bias={b is not None}: {int((got != r).sum())} of {r.numel()} outputs are not the dequantised weight"
    # ---- two-hot ----
    share = 0.0
    for shift in range(0, max(splits, 1), M):
        x, ref64, exact = awq_gemm_two_hot(w16, M, K, splits, shift)
        share = max(share, 1.0 - exact.float().mean().item())
        assert share < 0.01, f"two-hot probe: {share:.4f} of the fp32 sums are inexact"
        ref = ref64.to(dt)
        for b, r in ((None, ref), (bias, ref + bias)):
            got = gemm(x, qw, sc, zr, bias=b)
            assert torch.equal(got[exact], r[exact]), \
                f"two-hot shift {shift} bias={b is not None}: {int((got[exact] != r[exact]).sum())} of {int(exact.sum())} sums of two weights differ"
    # ---- random parity, fused bias, reproducibility ----
    xr = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(dt).cuda()
    out = gemm(xr, qw, sc, zr)
    ref = (xr.double() @ w16.double().t()).to(dt)
    differ = (out != ref).float().mean().item()
    assert_close_16(f32(out), f32(ref), dtype, f"gemm_awq {M}x{N}x{K}", max_bad_frac=2e-3)
    biased = gemm(xr, qw, sc, zr, bias=bias)
    assert torch.equal(biased, out + bias), "the fused bias is not the 16-bit add"
    assert torch.equal(out, gemm(xr, qw, sc, zr)) and torch.equal(biased, gemm(xr, qw, sc, zr, bias=bias)), "two launches differ"
    print(f"gemm_awq {dtype} ({M}, {N}, {K}) splits {splits}: probes bit-exact ({share:.4f} of the two-hot sums skipped as inexact); random parity: "
          f"{differ:.4f} of the outputs differ from the float64 restatement, none by more than 1 ulp (allowed beyond 1 ulp: 0.002)")


# =======================================================================================================================================
# 4. image-prompt attention
# =======================================================================================================================================
def _selection_probe(T: int, H: int, N: int, dtype: str, seed: int = 0, tag: str = ""):
    """Every-key selection: k[n] is a vector of +-1 per head, q[t] = 12 k[(t + shift) mod N], so row t's own score is 12 * 128 / sqrt(128) ~ 136
    and every other one 12 (k_i . k_j) / sqrt(128), about +- 12.  Checked on the device in fp32: the own score leads all others by more than 40
    after scaling, i.e. every other probability is below e^-40 ~ 4e-18 (fp16: rounds to 0; bf16: 256 of them are < 2^-24 of the winner's 1.0, so
    l = 1 and, with 0.5 <= |v| < 2, O = v[winner] in fp32).  out[t] must then be v[(t + shift) mod N] BIT FOR BIT.  The shifts 0, T, 2 T, ... < N
    select every key position of every key tile at least once: a wrong piece order or swizzle in the K or V^T image of the NKT class fails here.
    -> the smallest margin seen"""
    from nunchaku_amd.ops.attention import ip_attention

    td, hd = TORCH_DT[dtype], H * 128
    g = torch.Generator(device="cuda").manual_seed(seed + 1000 * T + 10 * H + N)
    k = (torch.randint(0, 2, (N, hd), device="cuda", generator=g) * 2 - 1).to(td)
    v = ((torch.rand(N, hd, device="cuda", generator=g) * 1.5 + 0.5) * (torch.randint(0, 2, (N, hd), device="cuda", generator=g) * 2 - 1)).to(td)
    margin = float("inf")
    for shift in range(0, N, T):
        sel = (torch.arange(T, device="cuda") + shift) % N
        q = 12.0 * k[sel]
        s = torch.einsum("thd,nhd->htn", q.float().view(T, H, 128), k.float().view(N, H, 128)) / math.sqrt(128)
        idx = sel[None, :, None].expand(H, T, 1)
        own = s.gather(2, idx).squeeze(2)
        lead = (own - s.scatter(2, idx, float("-inf")).max(dim=2).values).min().item() if N > 1 else float("inf")
        del s
        assert lead > 40, f"{tag} shift {shift}: the selected key leads by {lead:.1f} only: the probe's precondition does not hold"
        margin = min(margin, lead)
        out = ip_attention(q, k, v, H)
        want = v[sel]
        assert torch.equal(out, want), f"{tag} shift {shift}: {int((out != want).any(dim=1).sum())} of {T} rows are not the selected key's V row"
    return margin


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,H,N", IP_CASES)
def test_ip_attention_remaining_key_tile_counts(T, H, N, dtype):
    """ip_attention_kernel<DT, NKT> for NKT 3 (12 key-holding pieces inside a 16-piece V^T row), 5 and 6, a ragged and a full last key tile
    each: test_gpu_ip_attention's accuracy gate, plain and prescaled, and the selection probe."""
    from nunchaku_amd.ops.attention import ip_attention
    from tests.test_gpu_ip_attention import _gate, _inputs, _prescaled

    qkv, k, v = _inputs(T, H, N, dtype)
    out = ip_attention(qkv, k, v, H)
    _gate(out, qkv[:, : H * 128], k, v, H, 1.0 / math.sqrt(128), dtype, f"({T},{H},{N}) {dtype} plain")
    pre, scale = _prescaled(qkv, H)
    out = ip_attention(pre, k, v, H, q_prescaled=True)
    _gate(out, pre[:, : H * 128], k, v, H, scale, dtype, f"({T},{H},{N}) {dtype} prescaled")
    margin = _selection_probe(T, H, N, dtype, tag=f"({T},{H},{N}) {dtype}")
    print(f"({T},{H},{N}) {dtype}: selection probe bit-exact, smallest lead {margin:.1f} (needs > 40)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ip_attention_selects_every_key_of_the_covered_classes(dtype):
    """the selection probe on the NKT classes test_gpu_ip_attention already launches (its dominant-key test only ever selects key 17)"""
    for T, H, N in IP_PROBE_COVERED:
        margin = _selection_probe(T, H, N, dtype, tag=f"({T},{H},{N}) {dtype}")
        print(f"({T},{H},{N}) {dtype}: selection probe bit-exact, smallest lead {margin:.1f} (needs > 40)")


def ip_grid(T: int, H: int, N: int):
    """(256-row query tiles, workgroups per head, tiles a workgroup walks at most) -- the rule of svdq_ip_attention restated: 512 workgroup slots
    (256 when K and V of a head take more than half of the 160 KiB of LDS), slots // H per head, then the fewest with the same number of rounds"""
    nkt = math.ceil(N / 32)
    pieces = 4 if nkt <= 1 else 8 if nkt <= 2 else 16 if nkt <= 4 else 32
    lds = nkt * 32 * 256 + 128 * pieces * 16
    slots = 512 if 2 * lds <= 160 * 1024 else 256
    tiles = math.ceil(T / 256)
    per_head = min(max(slots // H, 1), tiles)
    rounds = math.ceil(tiles / per_head)
    return tiles, math.ceil(tiles / rounds), rounds


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,H,N", IP_MULTI_TILE)
def test_ip_attention_tile_loop_makes_more_than_one_iteration(T, H, N, dtype):
    """200 heads leave 2 workgroups per head (N = 20) or 1 (N = 161: K and V take more than half the LDS) for 3 query tiles: the loop
    ``for (tile = blockIdx.x; tile < tiles; tile += gridDim.x)`` walks tiles 0 and 2 in one workgroup and tile 1 in the other, or all three in
    one.  A tile's result must not depend on which iteration produced it: rows [0, 256) equal a T = 256 launch (one iteration everywhere)."""
    from nunchaku_amd.ops.attention import ip_attention
    from tests.test_gpu_ip_attention import _gate

    assert ip_grid(T, H, N) == ((3, 2, 2) if N == 20 else (3, 1, 3)) and ip_grid(256, H, N) == (1, 1, 1)
    td, hd = TORCH_DT[dtype], H * 128
    g = torch.Generator(device="cuda").manual_seed(N)
    q = torch.randn(T, hd, device="cuda", generator=g).to(td)
    q[: T // 2] *= 4.0  # peaky rows, as test_gpu_ip_attention._inputs
    k = torch.randn(N, hd, device="cuda", generator=g).to(td)
    v = torch.randn(N, hd, device="cuda", generator=g).to(td)
    out = ip_attention(q, k, v, H)
    _gate(out, q, k, v, H, 1.0 / math.sqrt(128), dtype, f"({T},{H},{N}) {dtype} multi-tile")
    assert torch.equal(out, ip_attention(q, k, v, H)), "two launches differ"
    assert torch.equal(out[:256], ip_attention(q[:256], k, v, H)), "rows [0, 256) depend on the workgroup iteration that produced them"
    margin = _selection_probe(T, H, N, dtype, tag=f"({T},{H},{N}) {dtype} multi-tile")
    print(f"({T},{H},{N}) {dtype}: selection probe bit-exact, smallest lead {margin:.1f} (needs > 40)")
