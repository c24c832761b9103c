"""``svdq_sandwich_norm`` and ``svdq_qk_norm_rope`` on the GPU against their CPU restatements (tests/zimage_ref.py), bit for bit.

The kernels' reciprocal RMS values come back through ``stats`` / ``rstd``; they are held to a float64 evaluation within the bound of their
longest chain of roundings and then fed to the restatement, so that every 16-bit output can be compared with ``torch.equal``.

The bound, relative: ``(8 * ceil(C / 512) + 12) * 2^-24``.  A term of the sum of squares passes through at most ``8 * ceil(C / 512)`` additions
inside its lane and 6 in the butterfly, all terms non-negative, so the sum carries at most that many half-ulps; the square, the division by C,
the addition of eps, the root and the reciprocal add one each (the root halves what it is given), the comparison value's rounding to fp32
another: 12 covers them."""

import pytest
import torch

from tests import zimage_ref as Z
from tests.test_gpu_dispatch_classes import ROW_WIDTHS

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "fp16"]
B, T = 2, 5            # M = 10 rows: a workgroup (4 rows) spans two samples, the last one has two idle waves
GAP = 24               # row strides wider than C


def _bound(C):
    return (8 * -(-C // 512) + 12) * 2.0 ** -24


def _rand16(shape, dtype, g, scale=1.0, shift=0.0):
    return (torch.randn(shape, generator=g) * scale + shift).to(Z.TD[dtype])


def _strided(t):
    """a [B, T, C] view with row stride C + GAP of a NaN-filled buffer that holds t (on the GPU)"""
    b, n, c = t.shape
    buf = torch.full((b, n, c + GAP), float("nan"), dtype=t.dtype, device="cuda")
    buf[..., :c] = t.cuda()
    return buf[..., :c], buf


def _check_rstd(got, values, C, what):
    want = Z.rstd64(values)
    rel = ((got.double() - want).abs() / want).max().item()
    assert rel <= _bound(C), f"{what}: rstd off by {rel:.3g} relative, bound {_bound(C):.3g}"


def _sandwich_case(C, dtype, g, *, use_a, use_gate, use_pre, use_scale, alias, strided):
    from nunchaku_amd.ops import sandwich_norm

    res, a = _rand16((B, T, C), dtype, g), _rand16((B, T, C), dtype, g, 3.0)
    res[1, 2] = 0      # a row of zeros (of both inputs) gives zeros
    a[1, 2] = 0
    w_post, w_pre = _rand16((C,), dtype, g, 0.2, 1.0), _rand16((C,), dtype, g, 0.2, 1.0)
    gate, scale = _rand16((B, C), dtype, g).tanh(), _rand16((B, C), dtype, g, 0.3, 1.0)
    res_d, res_buf = _strided(res) if strided else (res.cuda(), None)
    a_d = (_strided(a)[0] if strided else a.cuda()) if use_a else None
    out = (res_d if alias else _strided(torch.zeros_like(res))[0] if strided else True) if use_a else False
    out_mod = (_strided(torch.zeros_like(res))[0] if strided else True) if use_pre else False
    o, m, stats = sandwich_norm(res_d, a_d, w_post=w_post.cuda() if use_a else None, gate=gate.cuda() if use_gate else None,
                                w_pre=w_pre.cuda() if use_pre else None, scale=scale.cuda() if use_scale else None, out=out, out_mod=out_mod,
                                want_stats=True)
    torch.cuda.synchronize()
    what = f"C={C} {dtype} a={use_a} gate={use_gate} w_pre={use_pre} scale={use_scale} alias={alias} strided={strided}"
    stats = stats.cpu().view(B, T, 2)
    rstd_a, rstd_y = stats[..., 0:1], stats[..., 1:2]
    f = lambda t: t.float()
    if use_a:
        _check_rstd(rstd_a, a, C, what + " (a)")
    else:
        assert torch.equal(rstd_a, torch.zeros_like(rstd_a)), what
    ry, rm = Z.sandwich_ref(f(res), f(a) if use_a else None, w_post=f(w_post) if use_a else None, gate=f(gate) if use_gate else None,
                            w_pre=f(w_pre) if use_pre else None, scale=f(scale) if use_scale else None, rstd_a=rstd_a, rstd_y=rstd_y, dtype=dtype)
    _check_rstd(rstd_y, ry, C, what + " (y)")
    if use_a:
        assert o.data_ptr() == res_d.data_ptr() if alias else True
        assert torch.equal(o.float().cpu(), ry), what + ": out"
    else:
        assert o is None
    if use_pre:
        assert torch.equal(m.float().cpu(), rm), what + ": out_mod"
        assert torch.equal(m[1, 2].float().cpu(), torch.zeros(C)), what + ": the row of zeros"
    else:
        assert m is None
    if strided and res_buf is not None:   # nothing was written between the rows
        assert torch.isnan(res_buf[..., C:]).all(), what
        if not alias:
            assert torch.equal(res_buf[..., :C].cpu(), res), what + ": res was written"


@pytest.mark.parametrize("dtype", DTYPES)
def test_sandwich_norm_is_bit_equal_to_the_restatement_at_every_width_class(dtype):
    """every class of row_pass.h with a full and a ragged last pass; the full pass strided with out aliasing res, the others by turns"""
    for i, C in enumerate(ROW_WIDTHS):
        g = torch.Generator().manual_seed(C)
        _sandwich_case(C, dtype, g, use_a=True, use_gate=True, use_pre=True, use_scale=True, alias=True, strided=True)
        _sandwich_case(C, dtype, g, use_a=True, use_gate=i % 2 == 0, use_pre=True, use_scale=i % 2 == 1, alias=False, strided=i % 4 < 2)
        _sandwich_case(C, dtype, g, use_a=False, use_gate=False, use_pre=True, use_scale=i % 2 == 0, alias=False, strided=i % 2 == 1)   # the opening pass
        _sandwich_case(C, dtype, g, use_a=True, use_gate=i % 2 == 1, use_pre=False, use_scale=False, alias=i % 2 == 0, strided=False)   # the closing pass


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [256, 520, 3840])
def test_sandwich_norm_each_optional_tensor_absent_and_two_calls_agree(C, dtype):
    g = torch.Generator().manual_seed(C + 1)
    for use_gate in (True, False):
        for use_scale in (True, False):
            _sandwich_case(C, dtype, g, use_a=True, use_gate=use_gate, use_pre=True, use_scale=use_scale, alias=False, strided=True)
    from nunchaku_amd.ops import sandwich_norm

    res, a = _rand16((B, T, C), dtype, g).cuda(), _rand16((B, T, C), dtype, g).cuda()
    w, s = _rand16((C,), dtype, g, 0.2, 1.0).cuda(), _rand16((B, C), dtype, g, 0.3, 1.0).cuda()
    first = sandwich_norm(res, a, w_post=w, gate=s, w_pre=w, scale=s, want_stats=True)
    second = sandwich_norm(res, a, w_post=w, gate=s, w_pre=w, scale=s, want_stats=True)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    only_stats = sandwich_norm(res, a, w_post=w, out=False, out_mod=False, want_stats=True)
    assert only_stats[0] is None and only_stats[1] is None and torch.equal(only_stats[2][:, 0], first[2][:, 0])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [520, 3840])
def test_sandwich_norm_of_a_single_value_in_a_row(C, dtype):
    from nunchaku_amd.ops import sandwich_norm

    v, col = 3.0, C - 3   # (a column of the ragged last pass)
    res = torch.zeros(1, 6, C, dtype=Z.TD[dtype])
    res[0, 4, col] = v
    w = torch.full((C,), 1.5, dtype=Z.TD[dtype])
    _, m, stats = sandwich_norm(res.cuda(), w_pre=w.cuda(), want_stats=True)
    want = 1.0 / (v * v / C + Z.EPS) ** 0.5
    assert abs(stats[4, 1].item() - want) / want <= _bound(C)
    assert abs(stats[0, 1].item() - Z.EPS ** -0.5) / Z.EPS ** -0.5 <= _bound(C)      # a row of zeros: 1 / sqrt(eps)
    m = m.float().cpu()
    expect = Z.r16(Z.r16(torch.tensor(v) * stats[4, 1].cpu(), dtype) * 1.5, dtype)
    assert m[0, 4, col] == expect and m.abs().sum() == expect.abs()                  # exact zeros everywhere else


# ---- svdq_qk_norm_rope ----------------------------------------------------------------------------------------------------------------
QK_SHAPES = [(1, 1, 128), (63, 1, 128), (64, 3, 128), (65, 3, 128), (130, 3, 256)]


def _qk_inputs(T_, H, L, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    HD = H * 128
    qkv = torch.full((L, 3 * HD + 64), float("nan"), dtype=Z.TD[dtype])     # row stride wider than 3 * H * 128
    qkv[:, :3 * HD] = _rand16((L, 3 * HD), dtype, g, 2.0)
    wq, wk = _rand16((128,), dtype, g, 0.2, 1.0), _rand16((128,), dtype, g, 0.2, 1.0)
    ang = torch.rand(T_, 64, generator=g) * 6.2831853
    fc = torch.polar(torch.ones_like(ang), ang)
    return qkv, wq, wk, fc


def _run_qk(qkv, H, T_, L, **kw):
    from nunchaku_amd.ops import qk_norm_rope

    HD = H * 128
    buf = qkv.cuda()
    vt = torch.full((HD, L + 128), float("nan"), dtype=qkv.dtype, device="cuda")   # ldvt = L_pad + 128
    _, rstd = qk_norm_rope(buf[:, :3 * HD], H, T_, vt=vt, want_rstd=True, **{k: None if v is None else v.cuda() for k, v in kw.items()})
    torch.cuda.synchronize()
    return buf.cpu(), vt.cpu(), rstd.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T_,H,L", QK_SHAPES)
def test_qk_norm_rope_is_bit_equal_to_the_restatement(T_, H, L, dtype):
    HD = H * 128
    qkv, wq, wk, fc = _qk_inputs(T_, H, L, dtype, seed=T_ * 10 + H)
    fr = torch.view_as_real(fc)
    got, vt, rstd = _run_qk(qkv, H, T_, L, norm_q=wq, norm_k=wk, freqs_cis=fc)
    x = lambda third: qkv[:T_, third * HD:(third + 1) * HD].float().view(T_, H, 128)
    for third, w, name in ((0, wq, "Q"), (1, wk, "K")):
        r = rstd[:, third * H:(third + 1) * H]
        want64 = Z.rstd64(x(third))[..., 0]
        assert ((r.double() - want64).abs() / want64).max().item() <= (8 + 4 + 12) * 2.0 ** -24, name   # 8 in the lane, 4 in the butterfly
        ref = Z.qk_ref(x(third), w.float(), r[..., None], fr, dtype)
        assert torch.equal(got[:T_, third * HD:(third + 1) * HD].float().view(T_, H, 128), ref), f"{name} at T={T_} H={H} {dtype}"
    # V's third, the rows behind T and the columns behind the packed width are as they were
    same = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert same(got[:, 2 * HD:], qkv[:, 2 * HD:]) and same(got[T_:], qkv[T_:])
    # V^T: the real columns, zeros up to L_pad, the prefill beyond
    assert torch.equal(vt[:, :T_], qkv[:T_, 2 * HD:3 * HD].t())
    assert torch.equal(vt[:, T_:L], torch.zeros(HD, L - T_, dtype=vt.dtype)) and torch.isnan(vt[:, L:]).all()
    # two calls are bit-equal
    again, vt2, rstd2 = _run_qk(qkv, H, T_, L, norm_q=wq, norm_k=wk, freqs_cis=fc)
    assert same(again, got) and same(vt2, vt) and torch.equal(rstd2, rstd)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T_,H,L", [(65, 3, 128), (130, 3, 256)])
def test_qk_norm_rope_fixed_rotations_and_absent_tensors(T_, H, L, dtype):
    HD = H * 128
    qkv, wq, wk, fc = _qk_inputs(T_, H, L, dtype, seed=T_ + 1)
    one, zero = torch.ones(T_, 64), torch.zeros(T_, 64)
    q_of = lambda buf: buf[:T_, :HD].float().view(T_, H, 128)
    plain, _, rstd = _run_qk(qkv, H, T_, L, norm_q=wq, norm_k=wk)                               # no rotation: exactly rms(.)
    n = Z.qk_ref(q_of(qkv), wq.float(), rstd[:, :H, None], None, dtype)
    assert torch.equal(q_of(plain), n)
    ident, _, _ = _run_qk(qkv, H, T_, L, norm_q=wq, norm_k=wk, freqs_cis=torch.stack([one, zero], -1))   # (1, 0)
    assert torch.equal(q_of(ident), n)
    quarter, _, _ = _run_qk(qkv, H, T_, L, norm_q=wq, norm_k=wk, freqs_cis=torch.stack([zero, one], -1))  # (0, 1)
    assert torch.equal(q_of(quarter)[..., 0::2], -n[..., 1::2]) and torch.equal(q_of(quarter)[..., 1::2], n[..., 0::2])
    raw, _, rstd_raw = _run_qk(qkv, H, T_, L, norm_k=wk, freqs_cis=fc)                          # norm_q NULL: the raw values are rotated
    assert torch.equal(q_of(raw), Z.qk_ref(q_of(qkv), None, None, torch.view_as_real(fc), dtype))
    assert torch.equal(rstd_raw[:, :H], torch.zeros(T_, H)) and torch.equal(rstd_raw[:, H:], rstd[:, H:])
    k_of = lambda buf: buf[:T_, HD:2 * HD].float().view(T_, H, 128)
    assert torch.equal(k_of(raw), Z.qk_ref(k_of(qkv), wk.float(), rstd[:, H:, None], torch.view_as_real(fc), dtype))
    # without vt and without anything to do, nothing is written
    from nunchaku_amd.ops import qk_norm_rope

    buf = qkv.cuda()
    qk_norm_rope(buf[:, :3 * HD], H, T_)
    assert torch.equal(buf.cpu().view(torch.int16), qkv.view(torch.int16))
