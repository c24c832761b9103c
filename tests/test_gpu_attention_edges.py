"""svdq_attention's online softmax on CONSTRUCTED score profiles (tests/helpers.py: attn_*), where the exact answer follows from the inputs alone.
tests/test_gpu_attention.py feeds the kernel randn only: which tile moves the deferred reference point is then an accident of the seed, and a lost
or doubly rescaled tile of small weight hides below its global bound.  Here the decisive key sits in a chosen tile -- the segment's first tile, the
first loop iteration, both buffer parities, the last tile, an "extra" tile of a masked launch, the first / last tile of a persistent segment -- and
an error changes an output by a whole value:

  1. one-hot selection      Q[l] = a K[pi(l)], K in {+-1}^128: out[l] == V[pi(l)] bit for bit (and two identical winners: their exact mean)
  2. uniform rows           Q = 0: out == round16(mean of the real V rows): every key counted exactly once
  3. controlled growth      rank-1 scores a_l b_j, b_j a chosen level per tile: the deferred move below, at and above its threshold, alpha = 0,
                            probabilities falling through the fp16 subnormals; elementwise against float64 and against oracle.attention_tiled
  4. non-finite query rows  NaN / +-inf rows of Q (svdq_amd.h: padded Q rows "may hold anything") do not reach any other row, fused quantiser included

Geometry 2 always reads a prescaled Q (the builder's Q times q_prescale(128), rounded once; q_prescaled=True) and is compared with references over
those same 16-bit values in log2 units.  Every test asserts the path it claims with ops.attention_last_plan().

Plans run (MI355X, 256 CUs; geometry, persistent workgroups): plain (128, 1), (256, 2), (1152, 2): (1, 0) and, at (256, 2), (2, 0); with the workspace
(256, 3): (1 | 2, 6), (1024, 3): (1 | 2, 96); masked (512, (300, 384, 500)): (1, 24) and (2, 0, masked_geometry2) with main segment [0, 4), (768, (700,)):
(1, 48) / main [0, 10), (1024, (37, 256, 1000)): (1, 96) / main [4, 14); non-finite rows (512, 3): geometry 1 | 2 on the plain grid and persistent; fused quantiser (512, 2): geometry 1 | 2 with the
workspace, split_lowrank at rank 128 only.

Largest section-3 ratios observed on an MI355X (|out - ref| in units of ulp16 * sum_j p_j |v_jd|, ulp16 = 2^-8 / 2^-11; bars 3.0 / 2.5, <= 1e-2 beyond 1):
  bf16  geometry 1: 0.60 against float64 (spike-second), 0.32 against the restatement (fall-7.5), none beyond 1;  geometry 2: 0.60, 0.32, none
  fp16  geometry 1: 0.46 against float64 (fall-30),      0.36 against the restatement (rise-20),  none beyond 1;  geometry 2: 0.46 (the masked spike), 0.36, none
"""

import math

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests import helpers as Hh
from tests.helpers import TORCH_DT, f32, make_module, t16

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


# (mode, L, H, kv_valid, geometry): lengths that are not a multiple of 256 always run geometry 1; masked launches keep the workspace, as a pipeline does
CASES = [("plain", L, H, None, g) for L, H in Hh.ATTN_PLAIN for g in ((1, 2) if L % 256 == 0 else (1,))]
CASES += [("persistent", L, H, None, g) for L, H in Hh.ATTN_PERSISTENT for g in (1, 2)]
CASES += [("masked", L, Hh.ATTN_MASKED_H, valid, g) for L, valid in Hh.ATTN_MASKED for g in (1, 2)]
CASE_IDS = [f"{m}-{L}x{H}{'' if v is None else '-' + '_'.join(map(str, v))}-{'8x32' if g == 1 else '4x64'}" for m, L, H, v, g in CASES]


def _as_read(q, dtype, geometry):
    """-> (the 16-bit Q the kernel reads, the factor from its scores to log2 units, the softmax scale of ops.attention / attention_tiled)"""
    return (Hh.attn_prescaled(q, dtype), 1.0, math.log(2.0)) if geometry == 2 else (q, Hh.ATT_C, 1.0 / math.sqrt(128))


def _launch(q, k, v, dtype, mode, geometry, valid=None, scale=None, repeat=1):
    """One ops.attention launch on numpy [L, H, 128] inputs (q: as the kernel reads it) -> ([L, H, 128] float32 per launch, the plan it ran)."""
    from nunchaku_amd._C import _Ops, ops

    L, H = q.shape[:2]
    tq, tk = t16(q, dtype), t16(k, dtype)
    vt = t16(v, dtype).permute(1, 2, 0).contiguous()
    saved = (_Ops.attention_geometry, _Ops.attention_use_workspace)
    outs = []
    try:
        _Ops.attention_geometry, _Ops.attention_use_workspace = geometry, mode != "plain"
        for _ in range(repeat):
            out = torch.full((L, H, 128), float("nan"), device="cuda", dtype=TORCH_DT[dtype])
            ops.attention(tq, tk, vt, out, 1.0 / math.sqrt(128) if scale is None else scale, kv_valid=valid, q_prescaled=geometry == 2)
            outs.append(f32(out))
        plan = ops.attention_last_plan()
        if mode != "plain":
            ops.attention_workspace_status()
    finally:
        _Ops.attention_geometry, _Ops.attention_use_workspace = saved
    want_geometry = geometry if L % 256 == 0 else 1
    assert plan["geometry"] == want_geometry and plan["masked_geometry2"] == (valid is not None and geometry == 2), plan
    if mode == "plain" or (valid is not None and geometry == 2):
        assert plan["persistent_groups"] == 0, plan
    else:
        assert plan["persistent_groups"] > 0, plan
    return outs, plan


def _where(out, want, rows, keys):
    """names the first wrong (row, head) of an exact comparison and the tile(s) its answer lives in"""
    bad = np.argwhere((out != want).any(axis=2) & rows[:, None])
    l, h = bad[0]
    d = np.flatnonzero(out[l, h] != want[l, h])[0]
    tiles = [int(np.broadcast_to(kk.reshape(len(rows), -1), out.shape[:2])[l, h]) // Hh.ATT_KB for kk in keys]
    return f"{len(bad)} rows differ; first: row {l} (block {l // 32}, row {l % 32} of it) head {h}, winner tile(s) {tiles}: out[{d}] = {out[l, h, d]!r}, exact {want[l, h, d]!r}"


def _placements(mode, L, H, valid):
    if mode == "masked":
        (j0, j1), targets = Hh.attn_mask_targets(L, H, valid)
        return [("targets", {"targets": targets, "real": Hh.attn_real_keys(L, valid)})]
    pl = [("scattered", {}), ("block", {})]
    if mode == "persistent":
        pl.append(("segments", {"segments": Hh.attn_schedule(L, H)}))
    return pl


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mode,L,H,valid,geometry", CASES, ids=CASE_IDS)
def test_one_hot_rows_select_their_value_bit_for_bit(mode, L, H, valid, geometry, dtype):
    """Q[l] = a K[pi(l)] over K in {+-1}^128: score(l, pi(l)) = 128 a, everything else 75 log2 units and more below (asserted in float64 on the inputs:
    the rest of the row weighs < 2^-6 of half a 16-bit ulp of min|V|), so out[l] == V[pi(l)] exactly -- wherever the winner sits: every tile of every
    32-row block (scattered), one tile per block (block), the first and last tile of each segment of a split task (segments: the winning partial result
    comes from a contributor's slab for some rows, from the owner's registers for others), the main segment's edges, the extra tiles and the partially
    padded tiles of a masked launch (targets), whose padded K rows hold decoys that would win by far -- or NaN -- and whose padded V rows are large.
    a = 2048: alpha and every other probability underflow to 0; v_amp = 2^14: fp16 values up to 32 000, and nothing may overflow: it is a selection."""
    real = Hh.attn_real_keys(L, valid)
    for pl, kw in _placements(mode, L, H, valid):
        pi = Hh.attn_winners(L, H, pl, **kw)
        for a in (8.0, 2048.0):
            for v_amp in (1.0, 2.0 ** 14):
                for padded_k in (("decoy", "nan") if valid is not None else ("decoy",)):
                    q, k, v = Hh.attn_onehot(L, H, dtype, a, v_amp, pi, seed=L + H, real=real, padded_k=padded_k)
                    qr, c, _ = _as_read(q, dtype, geometry)
                    if v_amp == 1.0 and padded_k == "decoy":  # (max|V| / min|V| does not depend on v_amp, the real rows not on the padding)
                        assert Hh.attn_selection_margin(qr, k, v, c, dtype, [pi], real) < 1.0
                    outs, plan = _launch(qr, k, v, dtype, mode, geometry, valid, repeat=2 if mode == "persistent" else 1)
                    want = np.take_along_axis(v, np.maximum(pi, 0)[:, :, None], axis=0)
                    ok = np.array_equal(outs[0][real], want[real])
                    assert ok, f"{pl} a={a} v_amp={v_amp} padded K={padded_k} {plan}: " + _where(outs[0], want, real, [pi])
                    assert all(np.array_equal(o, outs[0], equal_nan=True) for o in outs[1:]), f"{pl} a={a}: two launches differ"
    print(f"one-hot {CASE_IDS[CASES.index((mode, L, H, valid, geometry))]} {dtype}: {plan}")


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mode,L,H,valid,geometry", CASES, ids=CASE_IDS)
def test_two_identical_winners_give_their_exact_mean(mode, L, H, valid, geometry, dtype):
    """Two identical key rows in different tiles (persistent shapes: in different segments of the split task): both probabilities are exp2(0), l = 2,
    the sums are exact and both merge factors are exp2(0): out == round16((V1 + V2) / 2)."""
    real = Hh.attn_real_keys(L, valid)
    targets = Hh.attn_mask_targets(L, H, valid)[1] if valid is not None else None
    pairs = Hh.attn_twin_pairs(L, real, targets)
    q, k, v, j1, j2 = Hh.attn_two_winners(L, H, dtype, 8.0, pairs, seed=3 * L + H, real=real)
    qr, c, _ = _as_read(q, dtype, geometry)
    assert Hh.attn_selection_margin(qr, k, v, c, dtype, [j1, j2], real) < 1.0
    outs, plan = _launch(qr, k, v, dtype, mode, geometry, valid, repeat=2 if mode == "persistent" else 1)
    want = O.round16((v[j1].astype(np.float64) + v[j2]) / 2, dtype)
    assert np.array_equal(outs[0][real], want[real]), f"{plan}: " + _where(outs[0], want, real, [j1, j2])
    assert all(np.array_equal(o, outs[0], equal_nan=True) for o in outs[1:])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mode,L,H,valid,geometry", CASES, ids=CASE_IDS)
def test_uniform_rows_count_every_real_key_once(mode, L, H, valid, geometry, dtype):
    """Q = 0: every probability is exactly 1, O = sum V exactly in fp32 and l = the number of real keys.  Power-of-two lengths: bit-equal to
    round16(mean V); L = 1152 and the masked launches (1 / l is inexact): at most one 16-bit ulp from round16 of the float64 mean -- over the REAL keys
    only: the padded K rows hold NaN, the padded V rows +-1000, one leaked or lost key moves every channel by many ulps."""
    real = Hh.attn_real_keys(L, valid)
    q, k, v, want = Hh.attn_uniform(L, H, dtype, seed=L + 5, real=real)
    outs, plan = _launch(q, k, v, dtype, mode, geometry, valid)
    out = outs[0][real]
    if valid is None and L & (L - 1) == 0:
        assert np.array_equal(out, np.broadcast_to(want, out.shape)), f"{plan}: " + _where(outs[0], np.broadcast_to(want, outs[0].shape), real, [])
    else:
        err = np.abs(out - want) / Hh.ulp16_of(want, dtype)
        assert np.isfinite(out).all() and err.max() <= 1.0, f"{plan}: {err.max():.2f} ulp from round16(mean V) at (row, head, channel) {np.argwhere(err > 1.0)[:4].tolist()}"


def _growth_bars(out, q, k, v, dtype, what, real=None):
    """The two bars of the growth section for one launch ([L, H, 128]); -> (largest ratio against float64, largest against the restatement)"""
    L, H = q.shape[:2]
    ulp = Hh.ULP16[dtype]
    rows = np.ones(L, dtype=bool) if real is None else real
    worst64, worst, off = 0.0, 0.0, 0.0
    for h in range(H):
        ref, cond = Hh.attn_softmax64(q[:, h], k[:, h], v[:, h], 1.0, real)
        worst64 = max(worst64, float((np.abs(out[:, h] - ref) / cond)[rows].max() / ulp))
        vz = v[:, h] if real is None else np.where(real[:, None], v[:, h], 0.0).astype(np.float32)
        tiled = O.attention_tiled(q[:, h], k[:, h], vz, math.log(2.0), dtype, key_mask=real)
        tcond = O.attention_tiled(q[:, h], k[:, h], np.abs(vz), math.log(2.0), dtype, key_mask=real)
        err = (np.abs(out[:, h] - tiled) / tcond)[rows] / ulp
        worst, off = max(worst, float(err.max())), max(off, float((err > 1.0).mean()))
    print(f"growth {what} {dtype}: vs float64 {worst64:.3f}, vs the restatement {worst:.3f} ulp16 of sum p|v|, {off:.2e} of the outputs beyond 1")
    return worst64, worst, off


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("profile", list(Hh.ATTN_PROFILES))
def test_controlled_growth_moves_the_reference_point_where_chosen(profile, dtype):
    """Rank-1 scores a_l b_j in log2 units (geometry 1: softmax scale ln 2; geometry 2: q_prescaled), a_l from {-2 .. 4} per row -- one 32-row block mixes
    rising, falling and flat rows, and the ballot moves them all -- and b_j = a chosen level per key tile + a multiple of 1/8: the deferred move
    (ATT_DEFER_LOG2 = 8) not quite reached, exactly reached, just passed, passed by far (alpha underflows to 0), scores falling until P runs through the
    fp16 subnormals to 0, a spike in the second tile (first loop iteration) or the last (last_tile), a zigzag.  Plain grid (512, 2) and persistent (1024, 3).
      against float64 softmax over the same 16-bit inputs, ELEMENTWISE: |out - ref| <= 3 ulp16 sum_j p_j |v_jd|  (P rounded to 16 bits: <= 1/2 ulp in
        the numerator and again in the row sum; the final rounding: 1/2; fp16-subnormal P: < 0.3 at these lengths; the rest for exp2 and summation order)
      against oracle.attention_tiled: the thresholds of test_attention_matches_its_tile_by_tile_restatement: <= 2.5 ulp16, at most 1e-2 of the outputs beyond 1."""
    for mode, L, H in (("plain", 512, 2), ("persistent", 1024, 3)):
        q, k, v = Hh.attn_rank1(L, H, dtype, profile, seed=L + 11)
        for geometry in (1, 2):
            outs, plan = _launch(q, k, v, dtype, mode, geometry, scale=math.log(2.0))
            w64, w, off = _growth_bars(outs[0], q, k, v, dtype, f"{profile} {mode} ({L}, {H}) geometry {geometry}")
            assert np.isfinite(outs[0]).all() and w64 <= 3.0 and w <= 2.5 and off <= 1e-2, (profile, dtype, mode, geometry, plan, w64, w, off)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_controlled_growth_in_an_extra_tile_of_a_masked_launch(dtype):
    """The +40 spike aimed at the last extra tile of the masked geometry-2 launch (1024, (37, 256, 1000)): the C++ extra tile behind the assembly loop
    must move the reference point of the rising rows by 10 .. 160 log2 units and leave the falling rows alone.  NaN in the padded K rows."""
    L, valid = Hh.ATTN_MASKED[2]
    H = Hh.ATTN_MASKED_H
    real = Hh.attn_real_keys(L, valid)
    (j0, j1), targets = Hh.attn_mask_targets(L, H, valid)
    spike = valid[2] // Hh.ATT_KB
    assert spike in targets[2:] and not real[spike * 64:(spike + 1) * 64].all()  # an extra tile, partially padded
    q, k, v = Hh.attn_rank1(L, H, dtype, "spike-last", seed=L + 11, spike_tile=spike)
    k[~real] = np.nan
    v[~real] = 0.0
    outs, plan = _launch(q, k, v, dtype, "masked", 2, valid, scale=math.log(2.0))
    w64, w, off = _growth_bars(outs[0], q, k, v, dtype, f"spike-extra masked ({L}, {valid}) geometry 2", real)
    assert np.isfinite(outs[0][real]).all() and w64 <= 3.0 and w <= 2.5 and off <= 1e-2, (plan, w64, w, off)


# ---- non-finite query rows ------------------------------------------------------------------------------------------------------------
POISON = {5: float("nan"), 100: float("inf"), 300: float("-inf")}


def _groups_of(rows, L):
    near = np.zeros(L, dtype=bool)
    for r in rows:
        near[r // 64 * 64:r // 64 * 64 + 64] = True
    return near


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("geometry", [1, 2], ids=["8x32", "4x64"])
def test_non_finite_query_rows_stay_in_their_rows(geometry, dtype):
    """svdq_amd.h: padded Q rows "may hold anything, including NaN".  Rows 5 / 100 / 300 of Q are NaN / +inf / -inf in every head (the randn inputs of
    test_attention_matches_fp32_reference at (512, 3), plain grid and persistent schedule): every other row is finite and meets that test's bar, and
    every row outside the 64-row groups of the three is bit-identical to the same launch with a clean Q (inside a group the ballot may move the
    reference point of the whole block: rounding only, held to the bar)."""
    from nunchaku_amd._C import _Ops, ops
    from nunchaku_amd.ops.attention import attention_packed
    from tests.test_gpu_attention import _as_produced_for, _ref_attention

    L, H = 512, 3
    td = TORCH_DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(L + H)
    qkv = torch.randn(L, 3 * H * 128, device="cuda", generator=g).to(td)
    qkv[: L // 2, : H * 128] *= 4.0
    bad = qkv.clone()
    for r, x in POISON.items():
        bad[r, : H * 128] = x
    clean = torch.ones(L, dtype=torch.bool, device="cuda")
    clean[list(POISON)] = False
    far = torch.from_numpy(~_groups_of(POISON, L)).cuda()
    saved = (_Ops.attention_geometry, _Ops.attention_use_workspace)
    try:
        for ws in (False, True):
            _Ops.attention_geometry, _Ops.attention_use_workspace = geometry, ws
            outs = []
            for x in (qkv, bad):
                x, kw, scale = _as_produced_for(geometry, x, H)
                vt = x[:, 2 * H * 128:].t().contiguous()
                outs.append(attention_packed(x, vt, H, **kw))
                plan = ops.attention_last_plan()
                assert plan["geometry"] == geometry and (plan["persistent_groups"] > 0) == ws, plan
            x, _, scale = _as_produced_for(geometry, qkv, H)
            q, k, v = (x[:, i * H * 128:(i + 1) * H * 128].unflatten(1, (H, 128)) for i in range(3))
            ref = _ref_attention(q, k, v, scale).reshape(L, H * 128)
            got = outs[1].float()
            assert torch.isfinite(got[clean]).all(), (ws, (~torch.isfinite(got)).any(1).nonzero().flatten().tolist())
            tol = 3 * Hh.ULP16[dtype] * ref.abs().max().item()
            assert (got[clean] - ref[clean]).abs().max().item() <= tol
            assert torch.equal(outs[0][far], outs[1][far]), (ws, (outs[0] != outs[1]).any(1).nonzero().flatten().tolist())
        ops.attention_workspace_status()
    finally:
        _Ops.attention_geometry, _Ops.attention_use_workspace = saved


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("geometry", [1, 2], ids=["8x32", "4x64"])
def test_non_finite_padded_rows_of_q_and_k(geometry, dtype):
    """The padded pipeline's shape, kv_valid = (300, 384, 500) at L = 512: NaN in the padded rows of Q AND K, zeros in the padded V columns.  Real rows:
    finite, inside the bar of test_key_padding_mask_matches_masked_sdpa against fp32 softmax over the real keys, and outside the 64-row groups that
    hold padded rows bit-identical to the launch whose padded Q rows are ordinary numbers."""
    from nunchaku_amd._C import _Ops, ops

    L, H, D, valid = 512, 3, 128, (300, 384, 500)
    td = TORCH_DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(L + len(valid))
    q, k, v = (torch.randn(L, H, D, device="cuda", generator=g) for _ in range(3))
    if geometry == 2:
        q = q * Hh.ATT_C
    q, k, v = q.to(td), k.to(td), v.to(td)
    real_np = Hh.attn_real_keys(L, valid)
    real = torch.from_numpy(real_np).cuda()
    far = torch.from_numpy(~_groups_of(np.flatnonzero(~real_np), L)).cuda()
    assert far.sum().item() == 320 and real[far].all()  # rows 0 .. 255 and 384 .. 447
    k_pad, v_pad, q_nan = k.clone(), v.clone(), q.clone()
    k_pad[~real] = float("nan")
    v_pad[~real] = 0
    q_nan[~real] = float("nan")
    vt = v_pad.permute(1, 2, 0).contiguous()
    saved = _Ops.attention_geometry
    outs = []
    try:
        _Ops.attention_geometry = geometry
        for qq in (q, q_nan):
            out = torch.empty(L, H, D, device="cuda", dtype=td)
            ops.attention(qq, k_pad, vt, out, D ** -0.5, kv_valid=valid, q_prescaled=geometry == 2)
            plan = ops.attention_last_plan()
            assert plan["geometry"] == geometry and plan["masked_geometry2"] == (geometry == 2), plan
            outs.append(out)
        ops.attention_workspace_status()
    finally:
        _Ops.attention_geometry = saved
    s = torch.einsum("lhd,mhd->hlm", q.float(), k[real].float()) * (math.log(2.0) if geometry == 2 else D ** -0.5)
    ref = torch.einsum("hlm,mhd->lhd", torch.softmax(s, dim=-1), v[real].float())
    got = outs[1].float()
    assert torch.isfinite(got[real]).all()
    assert (got[real] - ref[real]).abs().max().item() <= (2e-2 if dtype == "bf16" else 4e-3)
    assert torch.equal(outs[0][far], outs[1][far]), (outs[0] != outs[1]).flatten(1).any(1).nonzero().flatten().tolist()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("geometry", [1, 2], ids=["8x32", "4x64"])
@pytest.mark.parametrize("R", [32, 128], ids=["r32-passes", "r128-split"])
def test_non_finite_query_rows_through_the_fused_quantiser(R, geometry, dtype):
    """attention_packed_quantized at (512, 2) with rows 5 / 100 / 300 of Q NaN / +inf / -inf: the codes and the scales of every other row are bit-identical
    to the clean launch's, lora_act within the fused quantiser test's 2e-3 max + 1e-5 -- through the in-epilogue low-rank passes (rank 32) and the split
    contraction kernel (rank 128).  Nothing is asserted about the three rows themselves: the header calls them unspecified."""
    from nunchaku_amd import layout
    from nunchaku_amd._C import _Ops, ops
    from nunchaku_amd.ops.attention import attention_packed_quantized
    from tests.test_gpu_attention import _as_produced_for

    L, H = 512, 2
    K = H * 128
    td = TORCH_DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(3)
    qkv = torch.randn(L, 3 * K, device="cuda", generator=g).to(td)
    qkv[: L // 2, :K] *= 4.0
    bad = qkv.clone()
    for r, x in POISON.items():
        bad[r, :K] = x
    lin = make_module(O.make_svdq_layer(K, 128, R, seed=2, dtype=dtype, cheap=True), dtype)
    clean = torch.ones(L, dtype=torch.bool, device="cuda")
    clean[list(POISON)] = False
    saved = (_Ops.attention_geometry, _Ops.attention_use_workspace, _Ops.attention_split_lowrank)
    got = []
    try:
        _Ops.attention_geometry, _Ops.attention_use_workspace, _Ops.attention_split_lowrank = geometry, True, True
        for x in (qkv, bad):
            x, kw, _ = _as_produced_for(geometry, x, H)
            res = attention_packed_quantized(x, x[:, 2 * K:].t().contiguous(), H, lin, **kw)
            assert res is not None
            plan = ops.attention_last_plan()
            assert plan["geometry"] == geometry and plan["split_lowrank"] == (R == 128), plan
            got.append((layout.unpack_act(res[0], K), layout.unpack_scales(res[1], L), res[2].float()))
        ops.attention_workspace_status()
    finally:
        _Ops.attention_geometry, _Ops.attention_use_workspace, _Ops.attention_split_lowrank = saved
    (c0, s0, l0), (c1, s1, l1) = got
    diff = (c0 != c1).any(1) & clean
    assert not diff.any(), f"codes of clean rows differ: rows {diff.nonzero().flatten().tolist()[:16]}"
    diff = (s0 != s1).any(0) & clean
    assert not diff.any(), f"scales of clean rows differ: rows {diff.nonzero().flatten().tolist()[:16]}"
    assert torch.isfinite(l1[clean]).all()
    assert (l1[clean] - l0[clean]).abs().max() <= 2e-3 * l0[clean].abs().max() + 1e-5
