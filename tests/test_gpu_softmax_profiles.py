"""svdq_attention_d64 and svdq_cross_attention on CONSTRUCTED score profiles (tests/softmax_profiles.py), where the exact answer follows from the
inputs alone.  Their own files feed them randn under a global gate (3 ulp16 of max|ref|, set by the peaky rows): a lost, stale or doubly rescaled
64-key chunk of a flat row hides below it.  Here an error changes an output by a whole value:

  (a) one-hot selection     Q[t] = a K[winner], K in {+-1}^D: out[t] == V[winner] bit for bit, at EVERY key position of every chunk and both
                            buffers of d64's double-buffered stage (which also walks its V transposition order key by key), neighbouring rows
                            of a wave winning 67 keys apart, a = 2048 with |V| up to 32 000 (alpha and every other probability underflow to 0)
  (b) two tied winners      in different chunks, an odd number of chunks apart among them: out == round16((V1 + V2) / 2) bit for bit
  (c) uniform rows          Q = 0: out == round16(mean V) (N a power of two: bit for bit; otherwise that value or its neighbour), every key
                            counted exactly once across the ragged last chunk
  (d) controlled growth     rank-1 scores, a chosen level per chunk (alpha below 1 in every chunk, alpha = 0, probabilities falling through the
                            fp16 subnormals), scale ln 2: ELEMENTWISE |out - ref64| <= 3.0 ulp16 sum_j p_j |v_jd| + sub16 sum_j |v_jd| / l.
                            The 3.0 is the first-order worst case of one rounding of P in the numerator, one in the row sum and the final one.
  (e) scale                 randn at scale 0.03 / 0.2 / 1.0 inside the bar of (d); op(2 q, scale / 2) == op(q, scale) bit for bit
  (f) non-finite Q rows     a NaN row, a row with one +inf channel and row T - 1 = -inf (the row that rows beyond T are clamped to) reach no other row
  (g) rounded row sum       two score levels: out is the quotient over the ROUNDED probabilities, which differs from the float64 softmax by less
                            than the bar of (d) can see

d64 runs (B, T, H, N) = (2, 130, 2, 200), (1, 96, 3, 520), (2, 40, 1, 65), (1, 33, 2, 77), (1, 64, 1, 128) and (1, 130, 2, 130), the last one
also from one packed [B, S, 3*H*64] buffer; cross-attention (B, T, H, D, counts) = (2, 260, 2, 112, [300, 65]), (2, 260, 2, 72, [320, 1]) and
(1, 40, 1, 128, [128]) from q rows of ceil128(H*D) columns, the packed kv halves and cu_seqlens.  tests/test_softmax_profiles.py runs the same
assertions on the CPU restatement and on seven planted errors.

Largest ratios observed on an MI355X: |out - ref64| in the unit of the bar 3.0 over all eleven profiles of (d) and every shape, then the same
for |out - restatement| (chunked_softmax_ref before its final rounding; printed, not asserted), then the largest of (e):
  d64              bf16  1.00 (rise-8),     0.98 (rise-7.5),    scale: 1.22 (scale 1.0)      fp16  1.05 (fall-30),    0.97 (rise-200),   scale: 1.29 (scale 1.0)
  cross-attention  bf16  0.95 (fall-7.5),   0.95 (fall-7.5),    scale: 1.52 (scale 1.0)      fp16  0.96 (rise-8.125), 0.96 (rise-8.125), scale: 1.43 (scale 1.0)
Both kernels pass every assertion as written; to three digits every figure equals what the CPU restatement gives on the same inputs.
"""


import pytest
import torch

from tests import softmax_profiles as S

pytestmark = pytest.mark.gpu

DT = list(S.DTYPES)
NAN, INF = float("nan"), float("inf")


def _ceil128(n):
    return (n + 127) // 128 * 128


def _d64_tensors(samples):
    q, k, v = (torch.stack([s[i] for s in samples]).cuda() for i in range(3))
    return q, k, v


def _d64_launch(samples, H, D, scale, dtype):
    """[B, T, H*64] and [B, N, H*64]; where T == N also the thirds of one packed [B, S, 3*H*64] buffer, which must give the same bits"""
    from nunchaku_amd.ops import attention_d64

    assert D == 64
    q, k, v = _d64_tensors(samples)
    out = attention_d64(q, k, v, H, scale=scale)
    if q.shape[1] == k.shape[1]:
        hd = H * 64
        qkv = torch.cat([q, k, v], dim=-1)
        packed = attention_d64(qkv[..., :hd], qkv[..., hd:2 * hd], qkv[..., 2 * hd:], H, scale=scale)
        assert torch.equal(packed, out), "the packed [B, S, 3*H*64] form differs from three contiguous tensors"
    return list(out.cpu())


def _xattn_tensors(samples, H, D, pad_fill=None):
    """q in rows of ceil128(H*D) columns (numbers in the padding columns, or ``pad_fill``), the packed kv halves, cu_seqlens"""
    hd = H * D
    B, T = len(samples), samples[0][0].shape[0]
    g = torch.Generator().manual_seed(B + T)
    q = torch.randn(B, T, _ceil128(hd), generator=g).to(samples[0][0].dtype)
    if pad_fill is not None:
        q[..., hd:] = pad_fill
    q[..., :hd] = torch.stack([s[0] for s in samples])
    kv = torch.cat([torch.cat([s[1], s[2]], dim=1) for s in samples]).cuda()
    counts = [s[1].shape[0] for s in samples]
    cu = torch.tensor([sum(counts[:b]) for b in range(B + 1)], dtype=torch.int32, device="cuda")
    return q.cuda(), kv, cu, max(counts)


def _xattn_launch(samples, H, D, scale, dtype):
    from nunchaku_amd.ops import cross_attention

    hd = H * D
    q, kv, cu, mk = _xattn_tensors(samples, H, D)
    return list(cross_attention(q, kv[:, :hd], kv[:, hd:], H, D, cu_seqlens=cu, max_keys=mk, scale=scale).cpu())


KERNELS = {"d64": (_d64_launch, S.D64_CASES), "xattn": (_xattn_launch, S.XATTN_CASES)}
PARAMS = [pytest.param(name, case, id=f"{name}-{S.case_id(case)}") for name, (_, cases) in KERNELS.items() for case in cases]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel,case", PARAMS)
def test_one_hot_rows_select_their_value_bit_for_bit_at_every_key_position(kernel, case, dtype):
    margin = S.check_onehot(KERNELS[kernel][0], case, S.DTYPES[dtype])
    print(f"one-hot {kernel} {S.case_id(case)} {dtype}: bit-exact at every key position, largest selection margin {margin:.3g} (needs < 1)")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel,case", PARAMS)
def test_two_tied_winners_in_different_chunks_give_their_exact_mean(kernel, case, dtype):
    S.check_two_winners(KERNELS[kernel][0], case, S.DTYPES[dtype])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel,case", PARAMS)
def test_uniform_rows_count_every_key_once(kernel, case, dtype):
    S.check_uniform(KERNELS[kernel][0], case, S.DTYPES[dtype])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel,case", PARAMS)
def test_controlled_growth_stays_inside_the_elementwise_bar(kernel, case, dtype):
    """every profile; the samples of one launch run different profiles (cross-attention: different counts too)"""
    worst = max((r for p in S.PROFILES for r in S.check_growth(KERNELS[kernel][0], case, S.DTYPES[dtype], p)), key=lambda r: r[1])
    print(f"growth {kernel} {S.case_id(case)} {dtype}: largest {worst[1]:.3f} against float64 ({worst[0]}), bar {S.BAR}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel,case", PARAMS)
def test_scale_is_applied(kernel, case, dtype):
    S.check_scale(KERNELS[kernel][0], case, S.DTYPES[dtype])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("kernel,case", PARAMS)
def test_the_row_sum_runs_over_the_rounded_probabilities(kernel, case, dtype):
    S.check_rounded_sum(KERNELS[kernel][0], case, S.DTYPES[dtype])


# ---- (f) non-finite query rows ------------------------------------------------------------------------------------------------------------
def _poison(q, rows, hd):
    """q [B, T, >= hd] -> a copy with row rows[0] NaN, one +inf channel in row rows[1], row rows[2] -inf (in every sample)"""
    bad = q.clone()
    bad[:, rows[0], :hd] = NAN
    bad[:, rows[1], 3] = INF
    bad[:, rows[2], :hd] = -INF
    return bad


def _assert_other_rows_equal(clean, got, rows, what):
    keep = torch.ones(clean.shape[1], dtype=torch.bool, device=clean.device)
    keep[list(rows)] = False
    assert torch.isfinite(clean).all()
    diff = (clean[:, keep] != got[:, keep]).flatten(2).any(dim=2).nonzero()
    assert diff.numel() == 0, f"{what}: {len(diff)} clean rows changed; first (sample, index among the clean rows) {diff[0].tolist()}"


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", [S.D64_CASES[0], S.D64_CASES[5]], ids=S.case_id)
def test_non_finite_query_rows_stay_in_their_rows_d64(case, dtype):
    """T = 130: rows 5 and 70 sit in waves 0 and 2 of the first query tile, row 129 = T - 1 in the last tile, whose rows 130 .. 159 are clamped to it"""
    from nunchaku_amd.ops import attention_d64

    T, H, D, Ns = case
    assert T % 32 != 0 and T > 128
    rows = (5, 70, T - 1)
    q, k, v = _d64_tensors([S.randn_inputs(T, N, H, D, S.DTYPES[dtype], 40 * b + N) for b, N in enumerate(Ns)])
    clean = attention_d64(q, k, v, H)
    _assert_other_rows_equal(clean, attention_d64(_poison(q, rows, H * D), k, v, H), rows, f"d64 {S.case_id(case)} {dtype}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", S.XATTN_CASES[:2], ids=S.case_id)
def test_non_finite_query_rows_stay_in_their_rows_cross_attention(case, dtype):
    """T = 260: rows 5 and 100 sit in waves 0 and 3 of the first 256-row tile, row 259 = T - 1 in the last; NaN in q's padding columns too"""
    from nunchaku_amd.ops import cross_attention

    T, H, D, Ns = case
    hd = H * D
    assert T % 32 != 0 and T > 256
    rows = (5, 100, T - 1)
    samples = [S.randn_inputs(T, N, H, D, S.DTYPES[dtype], 40 * b + N) for b, N in enumerate(Ns)]
    q, kv, cu, mk = _xattn_tensors(samples, H, D)
    bad, _, _, _ = _xattn_tensors(samples, H, D, pad_fill=NAN)
    assert _ceil128(hd) > hd and torch.isnan(bad[..., hd:]).all() and torch.equal(bad[..., :hd], q[..., :hd])
    run = lambda x: cross_attention(x, kv[:, :hd], kv[:, hd:], H, D, cu_seqlens=cu, max_keys=mk)
    _assert_other_rows_equal(run(q), run(_poison(bad, rows, hd)), rows, f"cross-attention {S.case_id(case)} {dtype}")
