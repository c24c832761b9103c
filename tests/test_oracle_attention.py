"""CPU checks of oracle.attention_tiled (the tile-by-tile restatement the GPU attention tests compare against): it must
itself be a correct softmax(QK^T/sqrt(d))V up to the 16-bit roundings it models, whatever the deferred-rescale threshold."""
import math

import numpy as np
import pytest

from oracle import svdq_oracle as O


def _inputs(L, d, dtype, seed, peaky):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((L, d)).astype(np.float32)
    if peaky:
        q[: L // 2] *= 4.0
    k = rng.standard_normal((L, d)).astype(np.float32)
    v = rng.standard_normal((L, d)).astype(np.float32)
    return tuple(O.round16(t, dtype) for t in (q, k, v))


def _softmax_ref(q, k, v, scale):
    s = q.astype(np.float64) @ k.astype(np.float64).T * scale
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    return p @ v.astype(np.float64), p @ np.abs(v.astype(np.float64))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("peaky", [False, True])
def test_tiled_restatement_is_a_softmax_attention(dtype, peaky):
    L, d = 256, 128
    q, k, v = _inputs(L, d, dtype, 3, peaky)
    scale = 1.0 / math.sqrt(d)
    out = O.attention_tiled(q, k, v, scale, dtype)
    ref, cond = _softmax_ref(q, k, v, scale)
    ulp = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
    # probabilities rounded to 16 bits before the PV product and the output rounded once more: a few ulp of sum p |v|
    assert np.abs(out - ref).max() <= 3 * ulp * cond.max()
    assert (np.abs(out - ref) / cond).max() <= 3 * ulp


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_deferred_rescale_threshold_does_not_change_the_result(dtype):
    """Any reference point of the online softmax is valid as long as numerator and denominator share it: thresholds 0 (always
    rescale to the running maximum) and 8 (the kernel's) agree within 2.5 ulp (16-bit) of sum p |v|, 99 % within one, on peaky rows."""
    L, d = 384, 128
    q, k, v = _inputs(L, d, dtype, 5, True)
    scale = 1.0 / math.sqrt(d)
    a = O.attention_tiled(q, k, v, scale, dtype, defer_log2=0.0)
    b = O.attention_tiled(q, k, v, scale, dtype, defer_log2=8.0)
    _, cond = _softmax_ref(q, k, v, scale)
    ulp = 2.0 ** -8 if dtype == "bf16" else 2.0 ** -11
    assert (np.abs(a - b) / cond).max() <= 2.5 * ulp and (np.abs(a - b) / cond > ulp).mean() < 1e-2
    # a row dominated by ONE key returns that key's value exactly (its probability's rounding cancels between O and l)
    q2 = q.copy()
    q2[0] = O.round16(k[7] * 40.0, dtype)
    out = O.attention_tiled(q2[:32], k, v, scale, dtype)
    assert np.array_equal(out[0], v[7])


# ---------------------------------------------------------------------------------------------------------------------
# The constructed score profiles of tests/test_gpu_attention_edges.py, at its shapes: the builders, their preconditions, and the restatement
# itself on them -- exact where the answer is exact, inside the GPU test's elementwise bar on the growth profiles.
# ---------------------------------------------------------------------------------------------------------------------
from tests import helpers as Hh  # noqa: E402


def _as_read(q, dtype, prescaled):
    """(the Q the kernel reads, the factor from its scores to log2 units, the softmax scale of attention_tiled)"""
    return (Hh.attn_prescaled(q, dtype), 1.0, math.log(2.0)) if prescaled else (q, Hh.ATT_C, 1.0 / math.sqrt(128))


def _onehot_cases(built_lib):
    """(L, H, kv_valid, placement name, pi-builder arguments) of the one-hot section"""
    for L, H in Hh.ATTN_PLAIN:
        for pl in ("scattered", "block"):
            yield L, H, None, pl, {}
    for L, H in Hh.ATTN_PERSISTENT:
        for pl in ("scattered", "block"):
            yield L, H, None, pl, {}
        yield L, H, None, "segments", {"segments": Hh.attn_schedule(L, H)}
    for L, valid in Hh.ATTN_MASKED:
        _, targets = Hh.attn_mask_targets(L, Hh.ATTN_MASKED_H, valid)
        yield L, Hh.ATTN_MASKED_H, valid, "targets", {"targets": targets, "real": Hh.attn_real_keys(L, valid)}


@pytest.mark.parametrize("prescaled", [False, True], ids=["raw", "prescaled"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_one_hot_builder_and_the_restatement_select_exactly(built_lib, dtype, prescaled):
    """Q[l] = a K[pi(l)] over K in {+-1}^128: the winner's score is 128 a, the rest of the row weighs less than 2^-6 of half a 16-bit ulp of the
    smallest |V| (asserted on the inputs), so the answer is V[pi(l)] bit for bit -- and attention_tiled returns it, decoy or NaN keys in the padding or not."""
    for L, H, valid, pl, kw in _onehot_cases(built_lib):
        real = Hh.attn_real_keys(L, valid)
        pi = Hh.attn_winners(L, H, pl, **kw)
        nt = L // Hh.ATT_KB
        if valid is None:  # the placements do what they claim: every 32-row block meets every tile / one tile; split tasks win at their segments' edges
            tiles = (pi // Hh.ATT_KB).reshape(L // 32, 32, H)
            if pl == "scattered":
                assert all(len(np.unique(tiles[b, :, h])) == min(32, nt) for b in range(L // 32) for h in range(H))
            elif pl == "block":
                assert (tiles == (np.arange(L // 32) % nt)[:, None, None]).all()
            else:
                seg = kw["segments"]
                split = seg[(seg[:, 2] > 0) | (seg[:, 3] < nt)]
                assert len(split) >= 2 * H
                for _, task, j0, j1, _, _ in split:
                    head, qt = divmod(int(task), L // 256)
                    assert {j0, j1 - 1} <= set(np.unique(tiles[qt * 8:(qt + 1) * 8, :, head]))
        else:
            (j0, j1), targets = Hh.attn_mask_targets(L, H, valid)
            assert (pi[~real] == -1).all() and real[pi[real]].all()
            assert set(np.unique(pi[real] // Hh.ATT_KB)) == set(targets) and {j0, j1 - 1} <= set(targets)
            assert any(not real[t * 64:(t + 1) * 64].all() for t in targets)
        for a, v_amp in ((8.0, 1.0), (2048.0, 1.0), (8.0, 2.0 ** 14)):
            for padded_k in (("decoy", "nan") if valid is not None and v_amp == 1.0 else ("decoy",)):
                q, k, v = Hh.attn_onehot(L, H, dtype, a, v_amp, pi, seed=L + H, real=real, padded_k=padded_k)
                qr, c, scale = _as_read(q, dtype, prescaled)
                if v_amp == 1.0 and padded_k == "decoy":  # (max|V| / min|V| does not depend on v_amp, the real rows not on the padding)
                    margin = Hh.attn_selection_margin(qr, k, v, c, dtype, [pi], real)
                    assert margin < 1.0, (L, H, valid, pl, a, v_amp, margin)
                    if valid is not None and a == 8.0:  # a decoy would win if it counted
                        s = Hh.attn_scores_log2(qr[real], k, c)
                        assert (s[:, :, ~real].max(axis=2) >= 2.9 * s[:, :, real].max(axis=2)).all()
                for h in {0, H - 1} if a == 8.0 and v_amp == 1.0 else {H - 1}:  # (the restatement is a Python loop: not every head at every amplitude)
                    out = O.attention_tiled(qr[:, h], k[:, h], v[:, h], scale, dtype, key_mask=None if valid is None else real)
                    want = v[pi[:, h], h]
                    assert np.array_equal(out[real], want[real]), (L, H, valid, pl, a, v_amp, padded_k, h)


@pytest.mark.parametrize("prescaled", [False, True], ids=["raw", "prescaled"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_two_identical_winners_average_exactly(built_lib, dtype, prescaled):
    """Two identical key rows in different tiles: both probabilities are exp2(0), l = 2, out = round16((V1 + V2) / 2)."""
    cases = [(L, H, None, None) for L, H in Hh.ATTN_PLAIN + Hh.ATTN_PERSISTENT]
    cases += [(L, Hh.ATTN_MASKED_H, valid, Hh.attn_mask_targets(L, Hh.ATTN_MASKED_H, valid)[1]) for L, valid in Hh.ATTN_MASKED]
    for L, H, valid, targets in cases:
        real = Hh.attn_real_keys(L, valid)
        pairs = Hh.attn_twin_pairs(L, real, targets)
        assert all(j1 // 64 != j2 // 64 and real[j1] and real[j2] for j1, j2 in pairs) and len({j for p in pairs for j in p}) == 2 * len(pairs)
        if (L, H) in Hh.ATTN_PERSISTENT:  # ... and in different segments of the split task
            seg = Hh.attn_schedule(L, H)
            of = lambda t: next(i for i, r in enumerate(seg) if r[1] == 0 and r[2] <= t < r[3])
            assert all(of(j1 // 64) != of(j2 // 64) for j1, j2 in pairs)
        q, k, v, j1, j2 = Hh.attn_two_winners(L, H, dtype, 8.0, pairs, seed=3 * L + H, real=real)
        qr, c, scale = _as_read(q, dtype, prescaled)
        assert Hh.attn_selection_margin(qr, k, v, c, dtype, [j1, j2], real) < 1.0
        for h in range(H):
            out = O.attention_tiled(qr[:, h], k[:, h], v[:, h], scale, dtype, key_mask=None if valid is None else real)
            want = O.round16((v[j1, h].astype(np.float64) + v[j2, h]) / 2, dtype)
            assert np.array_equal(out[real], want[real]), (L, H, valid, h)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_uniform_rows_count_every_real_key_once(built_lib, dtype):
    """Q = 0: every probability is exactly 1, O = sum V exactly in fp32, l = the number of real keys.  Power-of-two lengths: bit-equal to
    round16(mean V); L = 1152 and the masked cases (1 / l is inexact): within one 16-bit ulp of it."""
    cases = [(L, H, None) for L, H in Hh.ATTN_PLAIN + Hh.ATTN_PERSISTENT] + [(L, Hh.ATTN_MASKED_H, valid) for L, valid in Hh.ATTN_MASKED]
    for L, H, valid in cases:
        real = Hh.attn_real_keys(L, valid)
        q, k, v, want = Hh.attn_uniform(L, H, dtype, seed=L + 5, real=real)
        for h in range(H):
            out = O.attention_tiled(q[:, h], k[:, h], v[:, h], 1.0 / math.sqrt(128), dtype, key_mask=None if valid is None else real)
            if valid is None and L & (L - 1) == 0:
                assert np.array_equal(out, np.broadcast_to(want[h], out.shape)), (L, H, h)
            else:
                assert (np.abs(out[real] - want[h]) <= Hh.ulp16_of(want[h], dtype)).all(), (L, H, valid, h)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("profile", list(Hh.ATTN_PROFILES))
def test_growth_profiles_stay_inside_the_elementwise_bar(dtype, profile):
    """Rank-1 scores a_l b_j with a chosen level per key tile: the deferred move at, just below and just above its threshold, alpha underflowing to 0,
    probabilities falling through the fp16 subnormals.  attention_tiled against float64 softmax over the same 16-bit inputs, ELEMENTWISE:
    |out - ref| <= 3 ulp16 sum_j p_j |v_jd|  (probabilities rounded to 16 bits: half an ulp in the numerator, half in the row sum; one final rounding:
    half; subnormal fp16 probabilities: < 0.3 at these lengths) -- the bar the GPU test applies to the kernel."""
    worst = 0.0
    for L, H in ((512, 2), (1024, 3)):
        q, k, v = Hh.attn_rank1(L, H, dtype, profile, seed=L + 11)
        assert set(np.unique(q[:, :, 0])) == set(Hh.ATTN_SLOPES) and not q[:, :, 1:].any() and not k[:, :, 1:].any()
        for h in range(H):
            out = O.attention_tiled(q[:, h], k[:, h], v[:, h], math.log(2.0), dtype)
            ref, cond = Hh.attn_softmax64(q[:, h], k[:, h], v[:, h], 1.0)
            worst = max(worst, float((np.abs(out - ref) / cond).max() / Hh.ULP16[dtype]))
    assert worst <= 3.0, f"{profile} {dtype}: {worst:.2f} ulp16 of sum p|v|"
    # the masked case of the GPU test: the spike aimed at the last extra tile
    if profile == "spike-last":
        L, valid = Hh.ATTN_MASKED[2]
        real = Hh.attn_real_keys(L, valid)
        q, k, v = Hh.attn_rank1(L, 3, dtype, profile, seed=L + 11, spike_tile=valid[2] // 64)
        assert (k[(valid[2] // 64) * 64:(valid[2] // 64 + 1) * 64, :, 0] >= 40).all() and (k[:valid[1], :, 0] < 1).all()
        k[~real] = np.nan
        for h in range(3):
            out = O.attention_tiled(q[:, h], k[:, h], v[:, h], math.log(2.0), dtype, key_mask=real)
            ref, cond = Hh.attn_softmax64(q[:, h], k[:, h], v[:, h], 1.0, real)
            assert (np.abs(out - ref)[real] <= 3.0 * Hh.ULP16[dtype] * cond[real]).all()
