"""tests/softmax_profiles.py on the CPU: the preconditions of every case tests/test_gpu_softmax_profiles.py launches hold, the restatement of the
kernels' order of operations (chunked_softmax_ref, rounded once) passes every assertion that file makes of the GPU, and seven deliberate errors
planted in the restatement are each caught by at least one of those assertions -- so the GPU tests can be checked, and shown to have teeth,
on a machine without a GPU.

Largest growth ratios of the restatement (|out - ref64| in the unit of the bar 3.0) over all eleven profiles and every shape: D = 64 bf16 1.00
(rise-8), fp16 1.05 (fall-30); D = 72 / 112 / 128 bf16 0.95 (fall-7.5), fp16 0.96 (rise-8.125); at scale 1.0 on randn 1.52 / 1.43."""

import math

import pytest
import torch

from tests import softmax_profiles as S
from tests.attention_d64_ref import kernel_order_ref

CASES = S.D64_CASES + S.XATTN_CASES
IDS = [S.case_id(c) for c in CASES]
DT = list(S.DTYPES)


def _sections(launch, case, dtype, profiles=tuple(S.PROFILES)):
    """every assertion of the GPU file on one case -> {section: the AssertionError's text} for the sections that fail"""
    td = S.DTYPES[dtype]
    runs = {"onehot": lambda: S.check_onehot(launch, case, td), "two-winners": lambda: S.check_two_winners(launch, case, td),
            "uniform": lambda: S.check_uniform(launch, case, td), "scale": lambda: S.check_scale(launch, case, td),
            "rounded-sum": lambda: S.check_rounded_sum(launch, case, td)}
    runs.update({f"growth:{p}": (lambda p=p: S.check_growth(launch, case, td, p)) for p in profiles})
    failed = {}
    for name, run in runs.items():
        try:
            run()
        except AssertionError as e:
            failed[name] = str(e)
    return failed


def test_round16_rounds_once_and_spacing16_is_the_formats():
    for td, mant in ((torch.bfloat16, 7), (torch.float16, 10)):
        one = torch.tensor([1.0, 1.5, 0.75, 100.0], dtype=torch.float64)
        assert torch.equal(S.spacing16(one, td), torch.tensor([2.0 ** -mant, 2.0 ** -mant, 2.0 ** -(mant + 1), 2.0 ** (6 - mant)], dtype=torch.float64))
        # just above a tie: a cast by way of float32 lands ON the tie and then rounds to even (down); one rounding goes up
        x = torch.tensor([1.0 + 2.0 ** -(mant + 1) + 2.0 ** -40], dtype=torch.float64)
        assert S.round16(x, td).item() == 1.0 + 2.0 ** -mant and x.float().to(td).item() == 1.0
        y = torch.randn(1000, generator=torch.Generator().manual_seed(0)).to(td)
        assert torch.equal(S.round16(y.double(), td), y)


def test_values_are_exact_and_their_fp32_sums_too():
    v = S.values(520, 3, 72, 1.0, seed=1)
    for td in S.DTYPES.values():
        assert torch.equal(v.to(td).float(), v)
    assert (v.abs() >= 1).all() and (v.abs() < 2).all() and torch.equal(v.sum(0).double(), v.double().sum(0))
    assert torch.equal((v * 2.0 ** 14).to(torch.float16).float(), v * 2.0 ** 14)


@pytest.mark.parametrize("N", [65, 77, 128, 130, 200, 300, 320, 520])
def test_twin_pairs_are_disjoint_in_different_chunks_and_one_is_an_odd_distance_apart(N):
    pairs = S.twin_pairs(N)
    flat = [j for p in pairs for j in p]
    assert len(set(flat)) == len(flat) and all(0 <= j < N for j in flat)
    assert all(a // 64 != b // 64 for a, b in pairs)
    assert any((a // 64 - b // 64) % 2 == 1 for a, b in pairs)
    if N > 128:
        assert {c for p in pairs for c in (p[0] // 64, p[1] // 64)} == set(range((N + 63) // 64))


@pytest.mark.parametrize("dtype", DT)
def test_onehot_rows_of_one_wave_win_in_different_chunks_and_the_shifts_cover_every_key(dtype):
    T, N, H, D = 96, 520, 3, 64
    seen = torch.zeros(N, dtype=torch.bool)
    for shift in range(0, N, T):
        q, k, v, win = S.onehot(T, N, H, D, S.DTYPES[dtype], 16.0, shift, seed=3)
        seen[win[:, 0]] = True
        s = torch.einsum("thd,nhd->htn", q.double().view(T, H, D), k.double().view(N, H, D)) * 0.125
        own = s.gather(2, win.t()[:, :, None])
        assert (own == 128.0).all() and (own - s.scatter(2, win.t()[:, :, None], -1e9).amax(2, keepdim=True)).min() >= 40
    assert seen.all()
    win = S.onehot(T, N, H, D, S.DTYPES[dtype], 16.0, 11, seed=3, stride=67)[3]
    chunks = {int(w) // 64 for w in win[:32, 0]}
    assert (win[1:] // 64 != win[:-1] // 64).all() and len(chunks) >= 8 and {c % 2 for c in chunks} == {0, 1}   # one wave: both buffers


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("D", [64, 72, 128])
@pytest.mark.parametrize("N", [64, 65, 77, 200, 520])
def test_uniform_inputs_notice_every_lost_and_every_doubled_key(N, D, dtype):
    """no exclusions: for EVERY key, removing it or counting it twice moves the float64 mean by more than 2 spacings in some channel of every head"""
    for b in range(2):
        for H in (1, 3):
            q, k, v, want = S.uniform(4, N, H, D, S.DTYPES[dtype], 500 * b + N + D)
            assert S.uniform_sensitivity(v, H, D, S.DTYPES[dtype]) > 2.0
            assert not q.any()


@pytest.mark.parametrize("dtype", DT)
def test_two_level_probabilities_sit_between_the_16_bit_values(dtype):
    td = S.DTYPES[dtype]
    deltas = S.two_level_deltas(td)
    assert len(deltas) >= 4
    for d in deltas:
        p = torch.tensor(2.0 ** -d, dtype=torch.float64)
        rel = abs(S.round16(p, td).item() - p.item()) / p.item()
        assert rel >= 0.15 * S.ULP16[td] and torch.tensor(d).to(td).item() == d
    q, k, v, want = S.two_level(40, 200, 2, 64, td, seed=5)
    # a row sum over the unrounded probabilities moves EVERY output by 0.1 .. 1 ulp16: what section (g) resolves and the bar of (d) cannot
    wrong = S.chunked_softmax_ref(q, k, v, 2, 64, math.log(2.0), td, mutate="sum-unrounded").double()
    gap = (want - wrong).abs() / want.abs()
    assert 0.1 * S.ULP16[td] < gap.min().item() and gap.max().item() < S.ULP16[td]
    right = S.chunked_softmax_ref(q, k, v, 2, 64, math.log(2.0), td).double()
    assert ((want - right).abs() / want.abs()).max().item() < 204 * 2.0 ** -24


def test_softmax64_and_the_restatement_agree_with_a_dense_softmax():
    T, N, H, D = 33, 77, 2, 72
    q, k, v = S.randn_inputs(T, N, H, D, torch.bfloat16, seed=2)
    ref, condp, condl = S.softmax64(q, k, v, H, D, 0.2)
    s = torch.einsum("thd,nhd->htn", q.double().view(T, H, D), k.double().view(N, H, D)) * 0.2
    p = torch.softmax(s, dim=-1)
    dense = torch.einsum("htn,nhd->thd", p, v.double().view(N, H, D)).reshape(T, H * D)
    assert (ref - dense).abs().max() < 1e-12 and (condp >= ref.abs() - 1e-12).all()
    l = torch.exp(s - s.amax(-1, keepdim=True)).sum(-1)                                     # [H, T]
    assert torch.allclose(condl.view(T, H, D)[:, :, 0] * l.t(), v.double().abs().view(N, H, D).sum(0)[None, :, 0].expand(T, H))
    got = S.chunked_softmax_ref(q, k, v, H, D, 0.2, torch.bfloat16)
    assert got.dtype == torch.float32 and (got.double() - dense).abs().max() <= 2 * 2.0 ** -8 * v.double().abs().max()


def test_kernel_order_ref_is_the_restatement_at_head_dim_64():
    q, k, v = S.randn_inputs(40, 150, 2, 64, torch.float16, seed=4)
    assert torch.equal(kernel_order_ref(q, k, v, 2, dtype=torch.float16), S.chunked_softmax_ref(q, k, v, 2, 64, None, torch.float16))
    assert torch.equal(kernel_order_ref(q, k, v, 2, 0.3), S.chunked_softmax_ref(q, k, v, 2, 64, 0.3, torch.bfloat16))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_restatement_passes_every_assertion_made_of_the_gpu(case, dtype):
    """exact selection at every key position (both amplitudes), the tied winners' means, the uniform mean, the bar of every growth profile, the
    scales and the rounded row sum -- with every precondition those assertions state (selection margins below 1, exact ties, sensitive means)"""
    failed = _sections(S.restatement_launch(), case, dtype)
    assert not failed, failed


EXPECTED = {  # mutant -> a section that must catch it (others may too)
    "alpha-not-on-l": "onehot", "last-key-dropped": "uniform", "key-beyond-n-counted": "rounded-sum", "stale-v-buffer": "onehot",
    "v-keys-swapped": "onehot", "scale-ignored": "scale", "sum-unrounded": "rounded-sum",
}
MUTANT_CASES = [S.D64_CASES[0], S.D64_CASES[1], S.XATTN_CASES[0]]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_each_planted_error_fails_an_assertion(mutant, dtype):
    assert set(EXPECTED) == set(S.MUTANTS)
    for case in MUTANT_CASES:
        failed = _sections(S.restatement_launch(mutant), case, dtype, profiles=("rise-8", "fall-30", "spike-last"))
        print(f"{mutant} {S.case_id(case)} {dtype}: caught by {sorted(failed)}")
        assert EXPECTED[mutant] in failed, f"{mutant} survives {EXPECTED[mutant]} at {S.case_id(case)} {dtype}; caught by {sorted(failed)}"
        print("   " + failed[EXPECTED[mutant]][:200])
