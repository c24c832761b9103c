"""Addresses beyond 2 and 4 GiB from a tensor's base, on the GPU: every op here runs once on compact tensors and once on views of very wide-strided
buffers that hold the same 16-bit values -- few live rows, so the work stays tiny while byte offsets cross 2^31 and 2^32 -- and the two results must be
bit-equal (compared as int16: the buffers are full of NaN).

The wide buffers ("arenas") are filled with a NaN of a fixed payload that no kernel produces.  After the call the number of elements of an output arena
that differ from it must be exactly the number of live output elements (counted over the whole arena, in chunks), and an input arena must hold its live
values and nothing else: a store that wrapped lands inside the arena and is counted, a load that wrapped reads NaN and breaks the equality.

Every stride lies inside the reach DESIGN.md section 7 ("Addressing reach") derives and tests/test_addressing_reach.py pins on the host; nothing beyond a
reach is ever launched here.  The compact result is known good either because the shape is a row of a table another module holds to its reference
(QUANT_CASES, GEMM_CASES, ATTN_CASES of tests/test_gpu_hot_instantiations.py) or because this module runs that reference on it.

Which field of which entry point is reached here, and at which stride, is tabulated in DESIGN.md section 7; what is not listed there is classified by reading alone.

Choosing ld (offsets are relative to each tensor's own data_ptr): at least one live row starts beyond 2^31 bytes and one beyond 2^32; where the row width
allows one row straddles each line.  ld = 2^29 - 8 with 6 rows of 520: row 2 crosses 2^31 at column 16, row 4 crosses 2^32 at column 32.
ld = (2^31 - 128) / 255 = 8421504: row 255 starts 256 bytes below 2^32.  ld = (2^30 - 64) / 255 = 4210752: row 255 starts 128 bytes below 2^31, row 510
256 bytes below 2^32."""
import gc
import math

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests import test_gpu_dispatch_classes as D
from tests import test_gpu_hot_instantiations as T
from tests.helpers import TORCH_DT, ULP16, attn_softmax64, checked_codes, f32, retargeted, t16

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "fp16")
SENTINEL = {"bf16": 0x7FA5, "fp16": 0x7DA5}  # a NaN with a payload: the kernels' own NaN (if they made one) is the canonical 0x7FC0 / 0x7E00, fp16 outputs clamp
CHUNK = 1 << 28                              # elements per counting step: a 256 MiB bool temporary
GIB = 1 << 30

ROW_M, ROW_C, ROW_LD = 6, 520, 2 ** 29 - 8
SLOT = 1024                                  # column offset between the views that share an arena of the row kernels
LD_255 = 8421504                             # (2^31 - 128) / 255
LD_510 = 4210752                             # (2^30 - 64) / 255
VEC_BS = 2 ** 31 + 8                         # batch stride of a per-sample vector: sample 1 starts beyond 4 GiB
assert 2 * ROW_LD * 2 < 2 ** 31 < 2 * ROW_LD * 2 + 2 * ROW_C and 4 * ROW_LD * 2 < 2 ** 32 < 4 * ROW_LD * 2 + 2 * ROW_C and 5 * ROW_LD * 2 > 2 ** 32
assert 255 * LD_255 * 2 == 2 ** 32 - 256 and 255 * LD_510 * 2 == 2 ** 31 - 128 and 510 * LD_510 * 2 == 2 ** 32 - 256 and LD_255 % 8 == LD_510 % 8 == 0


@pytest.fixture(autouse=True)
def _gpu_and_release(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _need(nbytes: int):
    """a test holds `nbytes` at once; on a card that others have filled it skips instead of failing in the allocator"""
    assert nbytes <= 13 * GIB, "a layout of this module holds about 12 GiB at the most"
    free = torch.cuda.mem_get_info()[0]
    if free < 1.5 * nbytes:
        pytest.skip(f"needs {nbytes / GIB:.1f} GiB, {free / GIB:.1f} GiB free")


class Arena:
    """one wide buffer full of the sentinel, the strided views handed out of it, and the count of what differs from the sentinel afterwards"""

    def __init__(self, elems: int, dtype: str):
        self.dtype, self.live = dtype, 0
        self.buf = torch.full((elems,), SENTINEL[dtype], dtype=torch.int16, device="cuda")

    @staticmethod
    def bytes(elems: int) -> int:
        return 2 * elems + CHUNK

    def view(self, shape, strides, offset=0, fill=None):
        v = self.buf.view(TORCH_DT[self.dtype]).as_strided(tuple(shape), tuple(strides), offset)
        if fill is not None:
            assert tuple(fill.shape) == tuple(shape)
            v.copy_(fill)
        self.live += math.prod(shape)
        return v

    def changed(self) -> int:
        n = 0
        for i in range(0, self.buf.numel(), CHUNK):
            n += int((self.buf[i:i + CHUNK] != SENTINEL[self.dtype]).sum())
        return n

    def holds_only(self, *pairs) -> bool:
        """an input arena: its views still equal what was copied in, and nothing else was written"""
        return self.changed() == self.live and all(same(v, x) for v, x in pairs)


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def bits32(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def span(rows: int, ld: int, width: int, slots: int = 1) -> int:
    return (rows - 1) * ld + (slots - 1) * SLOT + width


def crosses(rows: int, ld: int, width: int):
    """the property the layouts are chosen for: a row starts beyond 2^31 bytes, a row starts beyond 2^32 bytes"""
    starts = [r * ld * 2 for r in range(rows)]
    return any(s >= 2 ** 31 for s in starts) and any(s >= 2 ** 32 for s in starts)


# =======================================================================================================================================
# 1. the row kernels: M = 6, C = 520, ld = 2^29 - 8.  The op takes one row stride for all its views, so the inputs share one arena (column slots
#    1024 apart) and the outputs another.
# =======================================================================================================================================
def _row_arena(dtype, slots):
    return Arena(span(ROW_M, ROW_LD, ROW_C, slots), dtype)


def _row_view(arena, M, slot, fill=None):
    return arena.view((M, ROW_C), (ROW_LD, 1), slot * SLOT, fill)


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_gate_stats(dtype):
    """in place (out = res: the in-place operand is the wide output), a in a second arena"""
    from nunchaku_amd._C import ops

    assert crosses(ROW_M, ROW_LD, ROW_C)
    _need(2 * Arena.bytes(span(ROW_M, ROW_LD, ROW_C)))
    res, a, _, gate = D._row_inputs(ROW_M, ROW_C, dtype, seed=11)
    tg, ta = t16(gate, dtype), t16(a, dtype)
    rc, sc = t16(res, dtype), torch.zeros(ROW_M, 2, device="cuda")
    ops.residual_gate_stats(rc, ta, None, tg, rc, sc)
    ref = O.residual_gate_ref(res, a, gate, None, dtype)
    assert np.array_equal(f32(rc), ref), "compact: differs from residual_gate_ref"
    D._stats_ratios(sc, ref, f"compact {dtype}")
    io, inp = _row_arena(dtype, 1), _row_arena(dtype, 1)
    rv, av = _row_view(io, ROW_M, 0, t16(res, dtype)), _row_view(inp, ROW_M, 0, ta)
    ss = torch.zeros(ROW_M, 2, device="cuda")
    ops.residual_gate_stats(rv, av, None, tg, rv, ss)
    torch.cuda.synchronize()
    assert same(rv, rc), f"{int((rv.view(torch.int16) != rc.view(torch.int16)).sum())} elements differ from the compact call"
    assert torch.equal(bits32(ss), bits32(sc)), "statistics differ from the compact call"
    assert io.changed() == ROW_M * ROW_C, (io.changed(), ROW_M * ROW_C)
    assert inp.holds_only((av, ta))
    # statistics only: nothing is written
    ss2 = torch.zeros(ROW_M, 2, device="cuda")
    ops.residual_gate_stats(rv, None, None, None, None, ss2)
    sc2 = torch.zeros(ROW_M, 2, device="cuda")
    ops.residual_gate_stats(rc, None, None, None, None, sc2)
    assert torch.equal(bits32(ss2), bits32(sc2)) and io.changed() == ROW_M * ROW_C and same(rv, rc)


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_gate_stats_pair(dtype):
    """the grouped launch, M = 5 and 6: both problems in the same two arenas, one column slot apart"""
    from nunchaku_amd._C import ops

    _need(2 * Arena.bytes(span(ROW_M, ROW_LD, ROW_C, 2)))
    io, inp = _row_arena(dtype, 2), _row_arena(dtype, 2)
    compact, sparse, refs = [], [], []
    for slot, M in enumerate((5, 6)):
        res, a, _, gate = D._row_inputs(M, ROW_C, dtype, seed=21 + slot)
        tg, ta = t16(gate, dtype), t16(a, dtype)
        compact.append((t16(res, dtype), ta, None, tg, None, torch.zeros(M, 2, device="cuda")))
        sparse.append((_row_view(io, M, slot, t16(res, dtype)), _row_view(inp, M, slot, ta), None, tg, None, torch.zeros(M, 2, device="cuda")))
        refs.append(O.residual_gate_ref(res, a, gate, None, dtype))
    for probs in (compact, sparse):
        (r1, a1, _, g1, _, s1), (r2, a2, _, g2, _, s2) = probs
        ops.residual_gate_stats(r1, a1, None, g1, r1, s1, second=(r2, a2, None, g2, r2, s2))
    torch.cuda.synchronize()
    for c, s, ref in zip(compact, sparse, refs):
        assert np.array_equal(f32(c[0]), ref), "compact: differs from residual_gate_ref"
        D._stats_ratios(c[5], ref, f"compact pair {dtype}")
        assert same(s[0], c[0]) and torch.equal(bits32(s[5]), bits32(c[5]))
    assert io.changed() == 11 * ROW_C, (io.changed(), 11 * ROW_C)
    assert inp.holds_only(*((s[1], c[1]) for c, s in zip(compact, sparse)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_diff(dtype):
    from nunchaku_amd._C import ops

    _need(2 * Arena.bytes(span(ROW_M, ROW_LD, ROW_C, 3)))
    prev, base, cur = D._diff_inputs(ROW_M, ROW_C, dtype, seed=31)
    scratch = lambda: (torch.zeros(ROW_M, 2, device="cuda"), torch.zeros(8, device="cuda"))
    oc, (pc, rc) = torch.zeros_like(cur), scratch()
    ops.residual_diff(cur, base, prev, oc, partials=pc, result=rc)
    assert torch.equal(oc, cur - base), "compact: out_res differs from torch's 16-bit subtraction"
    D._check_record(rc[:5].tolist(), (prev - (cur - base)).abs(), prev.abs(), ROW_M, ROW_C, TORCH_DT[dtype], f"compact {dtype}")
    inp, out = _row_arena(dtype, 3), _row_arena(dtype, 1)
    cv, bv, pv = (_row_view(inp, ROW_M, i, x) for i, x in enumerate((cur, base, prev)))
    ov, (ps, rs) = _row_view(out, ROW_M, 0), scratch()
    ops.residual_diff(cv, bv, pv, ov, partials=ps, result=rs)
    torch.cuda.synchronize()
    assert same(ov, oc) and torch.equal(bits32(rs), bits32(rc)) and torch.equal(bits32(ps), bits32(pc))
    assert out.changed() == ROW_M * ROW_C, (out.changed(), ROW_M * ROW_C)
    assert inp.holds_only((cv, cur), (bv, base), (pv, prev))
    # out_res = cur: the in-place operand is the wide one
    (ps, rs) = scratch()
    ops.residual_diff(cv, bv, pv, cv, partials=ps, result=rs)
    assert same(cv, oc) and torch.equal(bits32(rs)[:5], bits32(rc)[:5]) and inp.changed() == 3 * ROW_M * ROW_C and same(bv, base) and same(pv, prev)


@pytest.mark.parametrize("dtype", DTYPES)
def test_modulated_diff(dtype):
    from nunchaku_amd._C import ops

    _need(2 * Arena.bytes(span(ROW_M, ROW_LD, ROW_C, 2)))
    rng = np.random.default_rng(41)
    x_np = (3.0 + 0.5 * rng.standard_normal((ROW_M, ROW_C))).astype(np.float32)
    x_np[D.CONST_ROW] = 3.0
    x_np = O.round16(x_np, dtype)
    scale_np = O.round16(1 + 0.3 * rng.standard_normal(ROW_C).astype(np.float32), dtype)
    shift_np = O.round16(0.5 * rng.standard_normal(ROW_C).astype(np.float32), dtype)
    x, scale, shift = t16(x_np, dtype), t16(scale_np, dtype), t16(shift_np, dtype)
    stats = torch.zeros(ROW_M, 2, device="cuda")
    ops.residual_gate_stats(x, None, None, None, None, stats)
    ref = O.ln_mod_ref(x_np, stats.cpu().numpy(), scale_np, shift_np, dtype)
    prev = (t16(ref, dtype).float() + torch.from_numpy((0.05 * rng.standard_normal((ROW_M, ROW_C))).astype(np.float32)).cuda()).to(TORCH_DT[dtype])
    scratch = lambda: (torch.zeros(ROW_M, 2, device="cuda"), torch.zeros(8, device="cuda"))
    oc, (pc, rc) = torch.zeros_like(x), scratch()
    ops.modulated_diff(x, stats, scale, shift, prev, oc, partials=pc, result=rc)
    assert np.array_equal(f32(oc), ref), "compact: differs from ln_mod_ref"
    inp, out = _row_arena(dtype, 2), _row_arena(dtype, 1)
    xv, pv = _row_view(inp, ROW_M, 0, x), _row_view(inp, ROW_M, 1, prev)
    ov, (ps, rs) = _row_view(out, ROW_M, 0), scratch()
    ops.modulated_diff(xv, stats, scale, shift, pv, ov, partials=ps, result=rs)
    torch.cuda.synchronize()
    assert same(ov, oc) and torch.equal(bits32(rs), bits32(rc)) and torch.equal(bits32(ps), bits32(pc))
    assert out.changed() == ROW_M * ROW_C, (out.changed(), ROW_M * ROW_C)
    assert inp.holds_only((xv, x), (pv, prev))
    # out_mod = prev: the buffer the engine keeps across steps
    (ps, rs) = scratch()
    ops.modulated_diff(xv, stats, scale, shift, pv, pv, partials=ps, result=rs)
    assert same(pv, oc) and torch.equal(bits32(rs)[:5], bits32(rc)[:5]) and inp.changed() == 2 * ROW_M * ROW_C and same(xv, x)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sandwich_norm(dtype):
    """B, T = 2, 3 at C = 520: the four row strides are the op's own, so res and a are wide in one call, out and out_mod in another.  The compact result
    is held to tests/zimage_ref.py as tests/test_gpu_zimage_ops.py holds it: the kernel's rstd within that module's bound, the 16-bit outputs bit for bit."""
    from nunchaku_amd.ops import sandwich_norm
    from tests import test_gpu_zimage_ops as ZO
    from tests import zimage_ref as Z

    B, Tn, C = 2, 3, ROW_C
    assert B * Tn == ROW_M
    _need(2 * Arena.bytes(span(ROW_M, ROW_LD, C)))
    g = torch.Generator().manual_seed(51)
    res, a = ZO._rand16((B, Tn, C), dtype, g), ZO._rand16((B, Tn, C), dtype, g, 3.0)
    w_post, w_pre = ZO._rand16((C,), dtype, g, 0.2, 1.0), ZO._rand16((C,), dtype, g, 0.2, 1.0)
    gate, scale = ZO._rand16((B, C), dtype, g).tanh(), ZO._rand16((B, C), dtype, g, 0.3, 1.0)
    kw = dict(w_post=w_post.cuda(), gate=gate.cuda(), w_pre=w_pre.cuda(), scale=scale.cuda(), want_stats=True)
    rd, ad = res.cuda(), a.cuda()
    oc, mc, sc = sandwich_norm(rd, ad, out=True, out_mod=True, **kw)
    stats = sc.cpu().view(B, Tn, 2)
    f = lambda t: t.float()
    ZO._check_rstd(stats[..., 0:1], a, C, "compact (a)")
    ry, rm = Z.sandwich_ref(f(res), f(a), w_post=f(w_post), gate=f(gate), w_pre=f(w_pre), scale=f(scale), rstd_a=stats[..., 0:1], rstd_y=stats[..., 1:2], dtype=dtype)
    ZO._check_rstd(stats[..., 1:2], ry, C, "compact (y)")
    assert torch.equal(oc.float().cpu(), ry) and torch.equal(mc.float().cpu(), rm), "compact: differs from sandwich_ref"
    wide = lambda arena, t=None: arena.view((B, Tn, C), (Tn * ROW_LD, ROW_LD, 1), 0, t)
    # ---- res and a ----
    a1, a2 = _row_arena(dtype, 1), _row_arena(dtype, 1)
    rv, av = wide(a1, rd), wide(a2, ad)
    o, m, st = sandwich_norm(rv, av, out=True, out_mod=True, **kw)
    torch.cuda.synchronize()
    assert same(o, oc) and same(m, mc) and torch.equal(bits32(st), bits32(sc)), "wide res / a: differs from the compact call"
    assert a1.holds_only((rv, rd)) and a2.holds_only((av, ad))
    del a1, a2, rv, av
    torch.cuda.empty_cache()
    # ---- out and out_mod ----
    a1, a2 = _row_arena(dtype, 1), _row_arena(dtype, 1)
    ov, mv = wide(a1), wide(a2)
    o, m, st = sandwich_norm(rd, ad, out=ov, out_mod=mv, **kw)
    torch.cuda.synchronize()
    assert same(ov, oc) and same(mv, mc) and torch.equal(bits32(st), bits32(sc)), "wide out / out_mod: differs from the compact call"
    assert a1.changed() == ROW_M * C and a2.changed() == ROW_M * C, (a1.changed(), a2.changed())
    del a1, a2, ov, mv
    torch.cuda.empty_cache()
    # ---- gate and scale: the second sample's vector 2^31 + 8 elements (beyond 4 GiB) behind the first ----
    a1, a2 = Arena(VEC_BS + C, dtype), Arena(VEC_BS + C, dtype)
    gv, sv = a1.view((B, C), (VEC_BS, 1), 0, kw["gate"]), a2.view((B, C), (VEC_BS, 1), 0, kw["scale"])
    o, m, st = sandwich_norm(rd, ad, out=True, out_mod=True, **{**kw, "gate": gv, "scale": sv})
    torch.cuda.synchronize()
    assert same(o, oc) and same(m, mc) and torch.equal(bits32(st), bits32(sc)), "wide gate / scale: differs from the compact call"
    assert a1.holds_only((gv, kw["gate"])) and a2.holds_only((sv, kw["scale"]))


DW_H, DW_W, DW_LD = 5, 7, 2 ** 26 - 8  # 35 pixels: pixel 16 straddles 2^31 bytes, pixel 32 straddles 2^32, pixels 33 and 34 start beyond it


@pytest.mark.parametrize("dtype", DTYPES)
def test_dwconv3x3(dtype):
    """B = 1, 5 x 7 pixels of 520 channels, the pixel stride wide on x, then on out; the compact result bit-equal to tests/dwconv_ref.py's dwconv_ref32"""
    from nunchaku_amd._C import ops
    from tests.dwconv_ref import dwconv_ref32

    H, W, C, P = DW_H, DW_W, ROW_C, DW_H * DW_W
    assert crosses(P, DW_LD, C)
    _need(Arena.bytes(span(P, DW_LD, C)))
    g = torch.Generator().manual_seed(61)
    x = torch.randn(1, H, W, C, generator=g)
    x[:, :3, :4] *= 8.0
    x = x.to(TORCH_DT[dtype])
    w = (torch.randn(C, 3, 3, 1, generator=g) / 3).to(TORCH_DT[dtype])
    b = torch.randn(C, generator=g).to(TORCH_DT[dtype])
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    oc = torch.zeros_like(xd)
    ops.dwconv3x3(xd, wd, bd, oc)
    assert torch.equal(oc.cpu(), dwconv_ref32(x, w, b)), "compact: differs from dwconv_ref32"
    wide = lambda arena, t=None: arena.view((1, H, W, C), (P * DW_LD, W * DW_LD, DW_LD, 1), 0, t)
    ax = Arena(span(P, DW_LD, C), dtype)
    xv, out = wide(ax, xd), torch.zeros_like(xd)
    ops.dwconv3x3(xv, wd, bd, out)
    torch.cuda.synchronize()
    assert same(out, oc), "wide x: differs from the compact call"
    assert ax.holds_only((xv, xd))
    del ax, xv
    torch.cuda.empty_cache()
    ao = Arena(span(P, DW_LD, C), dtype)
    ov = wide(ao)
    ops.dwconv3x3(xd, wd, bd, ov)
    torch.cuda.synchronize()
    assert same(ov, oc), "wide out: differs from the compact call"
    assert ao.changed() == P * C, (ao.changed(), P * C)


# =======================================================================================================================================
# 2. the quantiser: the rows of x are the wide operand; codes, scales and lora_act are contiguous images
# =======================================================================================================================================
QUANT_K = T.QUANT_K
QUANT_LAYOUTS = (
    # (name, R, fuse_glu, M, M_pad, ldx of the (second, if grouped) input, grouped, family the plan must name)
    ("fast-below-the-line", 32, False, 250, 256, 2 ** 22 - 8, False, "fast"),   # M_pad * ldx * 2 = 2^31 - 4096: the widest stride the fast kernel takes
    ("general-r32", 32, False, T.QUANT_M, 512, LD_255, False, "general"),
    ("general-r176", 176, False, T.QUANT_M, 512, LD_255, False, "general"),
    ("general-glu-r32", 32, True, T.QUANT_M, 512, LD_255, False, "general"),
    ("grouped-wide-x2", 32, False, T.QUANT_M, 512, 2 ** 26 - 8, True, "general"),  # 44 rows: row 16 straddles 2^31 bytes, row 32 straddles 2^32
)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", QUANT_LAYOUTS, ids=lambda l: l[0])
def test_quantize(layout, dtype):
    """codes, scales and lora_act bit-equal to the compact call, and through ``checked_codes`` against the oracle (the GLU row: the compact call is the
    QUANT_CASES row that tests/test_gpu_hot_instantiations.py holds to test_quantize_fuse_glu's assertions); the plan query asserted before each launch"""
    name, R, glu, M, M_pad, ld, grouped, family = layout
    width, rows = 2 * QUANT_K if glu else QUANT_K, M - 256 if grouped else M
    assert name.startswith("fast") or crosses(rows, ld, width)
    _need(Arena.bytes(span(rows, ld, width)))
    if grouped:
        streams = [T._QuantStream(R, True, False, glu, 256, QUANT_K, dtype, 41), T._QuantStream(R, True, False, glu, M - 256, QUANT_K, dtype, 42)]
    else:
        streams = [T._QuantStream(R, True, False, glu, M, QUANT_K, dtype, 41)]
    wide = streams[-1]
    assert wide.xt.shape[0] == rows
    plan = lambda **kw: T.quant_plan(R, True, False, glu, grouped, "f32", M, QUANT_K, M_pad, **kw)
    assert plan()["family"] == ("general" if glu or R > 160 else "fast")  # the compact launch: the kernel the QUANT_CASES row of this shape claims
    compact = T._quant_launch(streams, R, glu, "f32", QUANT_K, M_pad, dtype)
    assert plan(**{"ldx2" if grouped else "ldx": ld})["family"] == family
    arena = Arena(span(rows, ld, width), dtype)
    xc = wide.xt
    wide.xt = arena.view((rows, width), (ld, 1), 0, xc)
    try:
        sparse = T._quant_launch(streams, R, glu, "f32", QUANT_K, M_pad, dtype)
    finally:
        xv, wide.xt = wide.xt, xc
    torch.cuda.synchronize()
    for what, c, s in zip(("codes", "scales", "lora_act"), compact, sparse):
        assert torch.equal(c.view(torch.int16 if c.element_size() == 2 else c.dtype), s.view(torch.int16 if s.element_size() == 2 else s.dtype)), \
            f"{name}: {what} differ from the compact call"
    assert arena.holds_only((xv, xc))
    if not glu:
        x_all, row0 = np.concatenate([s.xp for s in streams]), 0
        for s in streams:
            n = s.xp.shape[0]
            checked_codes(sparse[0], sparse[1], x_all, s.smooth, dtype, rows=np.arange(row0, row0 + n))
            row0 += n


# =======================================================================================================================================
# 3. the W4A4 GEMM: out (ldo) and out_vt (ldvt).  ops.gemm_w4a4 takes a contiguous out, so the launch of tests/test_gpu_hot_instantiations.py's _GemmRun
#    is retargeted on its way into the library: out / ldo / out_vt / ldvt of the args struct are replaced, everything else is the table row's.
# =======================================================================================================================================
def _gemm_case(fuse, geometry, R):
    rows = [c for c in T.GEMM_CASES if c[0] == fuse and c[1] == geometry and c[2] == "f32" and c[3] == R and c[5] == T.M_SMALL]
    assert len(rows) == 1, rows
    return rows[0]


LDO_HIGH = 2 ** 24 - 8  # the upper half of the wave-tile kernel's reach: the 32-bit store offset of a wave's row 127 (254 ldo + 16) passes 2^31
GEMM_LAYOUTS = (("8-wave-plain", "none", 1, 32, LD_255), ("wave-tile-r0", "none", 8, 0, LD_255), ("wave-tile-r32", "none", 8, 32, LD_255),
                ("8-wave-silu", "silu", 1, 32, LD_255), ("wave-tile-r32-upper-half", "none", 8, 32, LDO_HIGH))
assert 2 ** 31 < 254 * LDO_HIGH + 16 < 2 ** 32 and LDO_HIGH <= 16909316
LDVT_GEMM = 2 ** 23 + 2 ** 16  # 256 channel rows: row 255 starts beyond 2^32 bytes


def _retargeted(monkeypatch, run, **fields):
    """run.launch() with `fields` written into the args struct just before the library sees it -> plan"""
    return retargeted(monkeypatch, "svdq_gemm_w4a4", run.launch, **fields)[1]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", GEMM_LAYOUTS, ids=lambda l: l[0])
def test_gemm_out(layout, dtype, monkeypatch):
    """a row of GEMM_CASES (held to the oracle by test_gemm_case) with out 8421504 (once 16777208) elements per row apart: inside the wave-tile kernel's reach of 16909316"""
    name, fuse, geometry, R, ldo = layout
    case = _gemm_case(fuse, geometry, R)
    M, N, key = case[5], case[7], case[9]
    assert crosses(M, ldo, N) and ldo <= 16909316
    _need(Arena.bytes(span(M, ldo, N)))
    run = T._GemmRun(case, dtype)
    (out_c,), plan_c = run.launch()
    assert T._plan_key(plan_c) == key[:2], plan_c
    # the compact launch into a buffer of the sentinel: what a launch writes at all
    small = Arena(M * N, dtype)
    sv = small.view((M, N), (N, 1))
    _retargeted(monkeypatch, run, out=sv.data_ptr())
    assert same(sv, out_c) and small.changed() == M * N
    arena = Arena(span(M, ldo, N), dtype)
    ov = arena.view((M, N), (ldo, 1))
    plan = _retargeted(monkeypatch, run, out=ov.data_ptr(), ldo=ldo)
    assert T._plan_key(plan) == key[:2], f"the wide launch took {plan}, the table row claims {key}"
    assert same(ov, out_c), f"{name}: {int((ov.view(torch.int16) != out_c.view(torch.int16)).sum())} elements differ from the compact launch"
    assert arena.changed() == M * N, (arena.changed(), M * N)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_qkv_out_and_out_vt(dtype, monkeypatch):
    """the RMSNorm + RoPE epilogue with out (Q, K) and out_vt (V transposed) both wide.  The compact out_vt is held to the V columns of the table row's plain
    launch, which test_gemm_case holds to the oracle."""
    case = _gemm_case("rmsnorm_rope", 1, 32)
    M, N, key = case[5], case[7], case[9]
    H3 = N // 3
    assert crosses(M, LD_255, N) and crosses(H3, LDVT_GEMM, M) and LDVT_GEMM <= 429496716
    _need(Arena.bytes(span(M, LD_255, N)) + Arena.bytes(span(H3, LDVT_GEMM, M)))
    run = T._GemmRun(case, dtype)
    (out_c,), plan_c = run.launch()
    assert T._plan_key(plan_c) == key[:2], plan_c
    small_o, small_v = Arena(M * N, dtype), Arena(H3 * run.M_pad, dtype)
    so, sv = small_o.view((M, N), (N, 1)), small_v.view((H3, M), (run.M_pad, 1))
    _retargeted(monkeypatch, run, out=so.data_ptr(), out_vt=sv.data_ptr(), ldvt=run.M_pad)
    assert same(so[:, :2 * H3], out_c[:, :2 * H3]) and same(sv, out_c[:, 2 * H3:].t()), "compact: out_vt is not the V columns transposed"
    assert small_o.changed() == M * 2 * H3 and small_v.changed() == H3 * M, "with out_vt the V columns of out stay unwritten"
    ao, av = Arena(span(M, LD_255, N), dtype), Arena(span(H3, LDVT_GEMM, M), dtype)
    ov, vv = ao.view((M, N), (LD_255, 1)), av.view((H3, M), (LDVT_GEMM, 1))
    plan = _retargeted(monkeypatch, run, out=ov.data_ptr(), ldo=LD_255, out_vt=vv.data_ptr(), ldvt=LDVT_GEMM)
    assert T._plan_key(plan) == key[:2], plan
    assert same(ov[:, :2 * H3], so[:, :2 * H3]) and same(vv, sv)
    assert ao.changed() == M * 2 * H3 and av.changed() == H3 * M, (ao.changed(), av.changed())


# =======================================================================================================================================
# 4. attention, head_dim 128: q and out (64-bit row addresses), k (reach 33554424) and vt (reach 16909312), each wide in a call of its own
# =======================================================================================================================================
LDK_HIGH = 2 ** 24 + 2 ** 19  # the upper half of ldk's reach: the 32-bit offset of key row 63 (126 ldk) and the tile stride (128 ldk) both pass 2^31
ATTN_LAYOUTS = (  # (L, geometry, workspace, Q prescaled), the row stride of q / k / out for that L, the operands made wide, the kernel (None: the ATTN_CASES row's)
    ((384, 0, True, False), LD_255, "qkv", None),
    ((512, 1, True, False), LD_510, "qkv", None),
    ((512, 0, True, True), LD_510, "qkv", None),
    ((256, 1, False, False), LDK_HIGH, "k", ("attention_kernel", (8, 0))),
    ((256, 0, True, True), LDK_HIGH, "k", ("attention_kernel64", (0, 0))),
)
assert 126 * LDK_HIGH > 2 ** 31 and 128 * LDK_HIGH > 2 ** 31 and LDK_HIGH <= 33554424
LDVT_ATT = 2 ** 23 + 2 ** 17  # 256 channel rows (2 heads): row 255 starts beyond 2^32 bytes; the kernels' 32-bit offset of channel row 127 of a head passes 2^31


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("layout", ATTN_LAYOUTS, ids=lambda l: f"L{l[0][0]}-g{l[0][1]}-pre{int(l[0][3])}")
def test_attention(layout, dtype):
    from nunchaku_amd._C import _Ops, ops
    from nunchaku_amd.ops.attention import q_prescale

    (L, geometry, ws, prescaled), ld, parts, key = layout
    if key is None:
        key = next(c for c in T.ATTN_CASES if c[:4] == (L, geometry, ws, prescaled) and c[4] is None)[5]
    H, td, W = T.ATTN_H, TORCH_DT[dtype], T.ATTN_H * 128
    assert crosses(L, ld, W) and crosses(W, LDVT_ATT, L) and ld <= 33554424 and LDVT_ATT <= 16909312 and 127 * LDVT_ATT * 2 > 2 ** 31
    _need((2 if "q" in parts else 1) * Arena.bytes(span(L, ld, W)))
    g = torch.Generator(device="cuda").manual_seed(L + 10 * geometry)
    qkv = torch.randn(L, 3 * W, device="cuda", generator=g).to(td)
    qkv[: L // 2, :W] *= 4.0  # peaky rows
    c = 1.0 / math.sqrt(128.0) * 1.4426950408889634
    if prescaled:
        qkv[:, :W] = (qkv[:, :W].float() * q_prescale(128)).to(td)
        c = 1.0
    q, k = (qkv[:, i * W:(i + 1) * W].contiguous().view(L, H, 128) for i in (0, 1))
    vt = qkv[:, 2 * W:].t().contiguous().view(H, 128, L)
    scale = 1.0 / math.sqrt(128.0)
    saved = (_Ops.attention_geometry, _Ops.attention_use_workspace)
    _Ops.attention_geometry, _Ops.attention_use_workspace = geometry, ws

    def launch(q, k, vt, out):
        ops.attention(q, k, vt, out, scale, q_prescaled=prescaled)
        plan = ops.attention_last_plan()
        ops.attention_workspace_status()
        assert T.attn_plan_key(L, plan) == key, f"claimed {key}, launched {plan}"

    try:
        out_c = torch.zeros(L, H, 128, dtype=td, device="cuda")
        launch(q, k, vt, out_c)
        x, got = f32(qkv).reshape(L, 3, H, 128), f32(out_c)
        for h in range(H):  # the bar of test_attention_case on the compact result
            ref, _ = attn_softmax64(x[:, 0, h], x[:, 1, h], x[:, 2, h], c, None)
            assert np.abs(got[:, h] - ref).max() <= 3 * ULP16[dtype] * np.abs(ref).max(), f"compact: head {h}"
        wide = lambda arena, t: arena.view((L, H, 128), (ld, 128, 1), 0, t)
        # ---- q and out ----
        if "q" in parts:
            aq, ao = Arena(span(L, ld, W), dtype), Arena(span(L, ld, W), dtype)
            qv, ov = wide(aq, q), wide(ao, None)
            launch(qv, k, vt, ov)
            assert same(ov, out_c), f"wide q / out: {int((ov.contiguous().view(torch.int16) != out_c.view(torch.int16)).sum())} elements differ"
            assert ao.changed() == L * W and aq.holds_only((qv, q))
            del aq, ao, qv, ov
            torch.cuda.empty_cache()
        # ---- k ----
        ak, out = Arena(span(L, ld, W), dtype), torch.zeros_like(out_c)
        kv = wide(ak, k)
        launch(q, kv, vt, out)
        assert same(out, out_c), f"wide k: {int((out.view(torch.int16) != out_c.view(torch.int16)).sum())} elements differ"
        assert ak.holds_only((kv, k))
        del ak, kv
        torch.cuda.empty_cache()
        if "v" not in parts:
            return
        # ---- vt (vt_hs with it) ----
        avt, out = Arena(span(W, LDVT_ATT, L), dtype), torch.zeros_like(out_c)
        vv = avt.view((H, 128, L), (128 * LDVT_ATT, LDVT_ATT, 1), 0, vt)
        launch(q, k, vv, out)
        assert same(out, out_c), f"wide vt: {int((out.view(torch.int16) != out_c.view(torch.int16)).sum())} elements differ"
        assert avt.holds_only((vv, vt))
    finally:
        _Ops.attention_geometry, _Ops.attention_use_workspace = saved


# =======================================================================================================================================
# 5. attention at head_dim 64: every row stride wide in turn, then B = 3 with samples 2^30 + 8 elements apart (sample 2 starts beyond 4 GiB)
# =======================================================================================================================================
D64_CASE = (1, 129, 2, 65)     # tests/test_gpu_attention_d64.py's smallest case with two query tiles and two key chunks
D64_LDQ = 2 ** 24 + 8          # 129 rows: row 64 starts beyond 2^31 bytes, row 128 beyond 2^32
D64_LDK = 2 ** 25 + 8          # 65 rows: row 32 starts beyond 2^31 bytes, row 64 beyond 2^32
D64_BS = 2 ** 30 + 8


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_d64_row_strides(dtype):
    from nunchaku_amd.ops import attention_d64
    from tests import test_gpu_attention_d64 as A

    B, Tn, H, N = D64_CASE
    assert D64_CASE in A.CASES and crosses(Tn, D64_LDQ, H * 64) and crosses(N, D64_LDK, H * 64)
    _need(Arena.bytes(span(N, D64_LDK, H * 64)))
    q, k, v = A._inputs(B, Tn, H, N, dtype)
    out_c = attention_d64(q, k, v, H)
    A._gate(out_c, q, k, v, H, dtype, f"compact {dtype}")
    for which, rows, ld in (("q", Tn, D64_LDQ), ("k", N, D64_LDK), ("v", N, D64_LDK), ("out", Tn, D64_LDQ)):
        arena = Arena(span(rows, ld, H * 64), dtype)
        src = {"q": q, "k": k, "v": v, "out": None}[which]
        view = arena.view((B, rows, H * 64), (rows * ld, ld, 1), 0, src)
        args = {"q": q, "k": k, "v": v}
        if which == "out":
            got = attention_d64(q, k, v, H, out=view)
            torch.cuda.synchronize()
            assert same(view, out_c) and arena.changed() == B * Tn * H * 64, f"wide out: {arena.changed()} elements written"
        else:
            args[which] = view
            got = attention_d64(args["q"], args["k"], args["v"], H)
            torch.cuda.synchronize()
            assert same(got, out_c), f"wide {which}: differs from the compact call"
            assert arena.holds_only((view, src))
        del arena, view, got
        torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_d64_batch_stride(dtype):
    from nunchaku_amd.ops import attention_d64
    from tests import test_gpu_attention_d64 as A

    B, (_, Tn, H, N) = 3, D64_CASE
    hd = H * 64
    assert 2 * D64_BS * 2 >= 2 ** 32 and D64_BS * 2 >= 2 ** 31
    elems = lambda rows: 2 * D64_BS + rows * hd
    _need(2 * Arena.bytes(elems(Tn)))
    q, k, v = A._inputs(B, Tn, H, N, dtype, seed=5)
    out_c = attention_d64(q, k, v, H)
    A._gate(out_c, q, k, v, H, dtype, f"compact B = 3 {dtype}")
    wide = lambda arena, rows, t=None: arena.view((B, rows, hd), (D64_BS, hd, 1), 0, t)
    aq, ao = Arena(elems(Tn), dtype), Arena(elems(Tn), dtype)
    qv, ov = wide(aq, Tn, q), wide(ao, Tn)
    attention_d64(qv, k, v, H, out=ov)
    torch.cuda.synchronize()
    assert same(ov, out_c), "wide q / out batch stride: differs from the compact call"
    assert ao.changed() == B * Tn * hd and aq.holds_only((qv, q))
    del aq, ao, qv, ov
    torch.cuda.empty_cache()
    ak, av = Arena(elems(N), dtype), Arena(elems(N), dtype)
    kv, vv = wide(ak, N, k), wide(av, N, v)
    got = attention_d64(q, kv, vv, H)
    torch.cuda.synchronize()
    assert same(got, out_c), "wide k / v batch stride: differs from the compact call"
    assert ak.holds_only((kv, k)) and av.holds_only((vv, v))


# =======================================================================================================================================
# 6. the remaining row passes: sana_glue (four row strides of its own) and qk_norm_rope (qkv in place, V transposed into vt)
# =======================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
def test_sana_glue(dtype):
    """B, T = 2, 3 at C = 520 (C_pad = 640): res and a wide in one call, out and out_mod in another.  The compact result is the one
    tests/test_gpu_sana_block.py's ``_run_and_compare`` holds to tests/sana_glue_ref.py, bit for bit."""
    from nunchaku_amd.ops import sana_glue
    from tests import sana_glue_ref as R
    from tests import test_gpu_sana_block as SB

    B, Tn, C, C_pad = 2, 3, ROW_C, 640
    _need(2 * Arena.bytes(span(ROW_M, ROW_LD, C_pad)))
    inp = SB._inputs(B, Tn, C, dtype, seed=71)
    shift, scale, gate = SB.MLP
    ref_o, ref_m, ref_s = SB._run_and_compare(inp, C_pad, dtype, True, gate, (shift, scale), True, what=f"compact {dtype}")
    cuda = lambda x: R.to_torch(x, dtype).cuda()
    res, a, ts, gtab, mtab = (cuda(inp[k]) for k in ("res", "a", "ts", "gtab", "mtab"))
    kw = dict(timestep=ts, gate_table=gtab, gate_row=gate, mod_table=mtab, scale_row=scale, shift_row=shift, channels=C, pad_to=C_pad, want_stats=True)
    oc, mc, sc = sana_glue(res, a, out=True, out_mod=True, **kw)
    assert same(oc, ref_o) and same(mc, ref_m), "compact: differs from the launch held to sana_glue_ref"
    wide = lambda arena, width, t=None: arena.view((B, Tn, width), (Tn * ROW_LD, ROW_LD, 1), 0, t)
    a1, a2 = Arena(span(ROW_M, ROW_LD, C), dtype), Arena(span(ROW_M, ROW_LD, C), dtype)
    rv, av = wide(a1, C, res), wide(a2, C, a)
    o, m, st = sana_glue(rv, av, out=True, out_mod=True, **kw)
    torch.cuda.synchronize()
    assert same(o, oc) and same(m, mc) and torch.equal(bits32(st), bits32(sc)), "wide res / a: differs from the compact call"
    assert a1.holds_only((rv, res)) and a2.holds_only((av, a))
    del a1, a2, rv, av
    torch.cuda.empty_cache()
    a1, a2 = Arena(span(ROW_M, ROW_LD, C_pad), dtype), Arena(span(ROW_M, ROW_LD, C_pad), dtype)
    ov, mv = wide(a1, C_pad), wide(a2, C_pad)
    o, m, st = sana_glue(res, a, out=ov, out_mod=mv, **kw)
    torch.cuda.synchronize()
    assert same(ov, oc) and same(mv, mc) and torch.equal(bits32(st), bits32(sc)), "wide out / out_mod: differs from the compact call"
    assert a1.changed() == ROW_M * C_pad and a2.changed() == ROW_M * C_pad, (a1.changed(), a2.changed())  # (the tail [C, C_pad) is written too: +0)
    del a1, a2, ov, mv
    torch.cuda.empty_cache()
    # ---- timestep: the second sample's [6, C] block 2^31 + 8 elements (beyond 4 GiB) behind the first ----
    a1 = Arena(VEC_BS + 6 * C, dtype)
    tv = a1.view((B, 6, C), (VEC_BS, C, 1), 0, ts)
    o, m, st = sana_glue(res, a, out=True, out_mod=True, **{**kw, "timestep": tv})
    torch.cuda.synchronize()
    assert same(o, oc) and same(m, mc) and torch.equal(bits32(st), bits32(sc)), "wide timestep: differs from the compact call"
    assert a1.holds_only((tv, ts))


QK_T, QK_H, QK_L = 65, 1, 128
QK_LD = 2 ** 26 - 8    # 65 rows: row 16 straddles 2^31 bytes, row 32 straddles 2^32, rows 33 .. 64 start beyond it
QK_LDVT = 2 ** 25 + 8  # 128 channel rows: row 32 starts beyond 2^31 bytes, row 64 beyond 2^32


@pytest.mark.parametrize("dtype", DTYPES)
def test_qk_norm_rope(dtype):
    """T = 65, H = 1, L_pad = 128: qkv (the in-place operand) wide in one call, vt in another.  The compact result is held to tests/zimage_ref.py's qk_ref as
    tests/test_gpu_zimage_ops.py holds its shapes: rstd within that module's bound, Q and K bit for bit, V^T the V columns transposed."""
    from nunchaku_amd._C import ops as _C_ops
    from nunchaku_amd.ops import qk_norm_rope
    from tests import test_gpu_zimage_ops as ZO
    from tests import zimage_ref as Z

    T_, H, L, HD = QK_T, QK_H, QK_L, QK_H * 128
    assert crosses(T_, QK_LD, 3 * HD) and crosses(HD, QK_LDVT, L)
    _need(Arena.bytes(span(T_, QK_LD, 3 * HD)))
    qkv, wq, wk, fc = ZO._qk_inputs(T_, H, L, dtype, seed=81)
    qkv = qkv[:, :3 * HD].contiguous()
    fr = torch.view_as_real(fc)
    kw = dict(norm_q=wq.cuda(), norm_k=wk.cuda(), freqs_cis=fc.cuda(), want_rstd=True)
    buf_c, vt_c = qkv.cuda(), torch.zeros(HD, L, dtype=qkv.dtype, device="cuda")
    _, rstd_c = qk_norm_rope(buf_c, H, T_, vt=vt_c, **kw)
    got, rstd = buf_c.cpu(), rstd_c.cpu()
    for third, w, name in ((0, wq, "Q"), (1, wk, "K")):
        x = qkv[:T_, third * HD:(third + 1) * HD].float().view(T_, H, 128)
        r = rstd[:, third * H:(third + 1) * H]
        want64 = Z.rstd64(x)[..., 0]
        assert ((r.double() - want64).abs() / want64).max().item() <= (8 + 4 + 12) * 2.0 ** -24, name
        assert torch.equal(got[:T_, third * HD:(third + 1) * HD].float().view(T_, H, 128), Z.qk_ref(x, w.float(), r[..., None], fr, dtype)), f"compact: {name}"
    assert torch.equal(vt_c.cpu()[:, :T_], qkv[:T_, 2 * HD:].t()) and not vt_c[:, T_:].any(), "compact: V^T"
    # ---- qkv ----
    aq = Arena(span(T_, QK_LD, 3 * HD), dtype)
    qv, vt = aq.view((T_, 3 * HD), (QK_LD, 1), 0, qkv[:T_].cuda()), torch.zeros_like(vt_c)
    # (the C-level op: it takes the T real rows alone and L_pad beside them; the wrapper above wants all L_pad rows of qkv, 17 GiB at this stride)
    rstd_s = torch.zeros_like(rstd_c)
    _C_ops.qk_norm_rope(qv, kw["norm_q"], kw["norm_k"], torch.view_as_real(kw["freqs_cis"]).contiguous(), vt, rstd_s, T_, L, H)
    torch.cuda.synchronize()
    assert same(qv, buf_c[:T_]) and same(vt, vt_c) and torch.equal(bits32(rstd_s), bits32(rstd_c)), "wide qkv: differs from the compact call"
    assert aq.changed() == T_ * 3 * HD, (aq.changed(), T_ * 3 * HD)
    del aq, qv
    torch.cuda.empty_cache()
    # ---- vt ----
    av, buf = Arena(span(HD, QK_LDVT, L), dtype), qkv.cuda()
    vv = av.view((HD, L), (QK_LDVT, 1))
    _, rstd_s = qk_norm_rope(buf, H, T_, vt=vv, **kw)
    torch.cuda.synchronize()
    assert same(vv, vt_c) and same(buf, buf_c) and torch.equal(bits32(rstd_s), bits32(rstd_c)), "wide vt: differs from the compact call"
    assert av.changed() == HD * L, (av.changed(), HD * L)  # (the columns [T, L_pad) are written too: zeros)


# =======================================================================================================================================
# 7. the small attentions: image-prompt, SANA's cross-attention, PuLID's folded cross-attention, SANA's linear attention
# =======================================================================================================================================
def _each_wide(dtype, operands, call, out_c, out_shape, out_strides, out_elems, what):
    """`operands`: {name: (compact tensor, strides of its wide view, elements of its arena)}; each wide in turn, then the output.
    `call(tensors by name, out or None)` -> the output tensor"""
    for name, (t, strides, elems) in operands.items():
        arena = Arena(elems, dtype)
        view = arena.view(tuple(t.shape), strides, 0, t)
        got = call({**{n: o[0] for n, o in operands.items()}, name: view}, None)
        torch.cuda.synchronize()
        assert same(got, out_c), f"{what}: wide {name}: differs from the compact call"
        assert arena.holds_only((view, t)), f"{what}: wide {name}: the input arena changed"
        del arena, view, got
        torch.cuda.empty_cache()
    arena = Arena(out_elems, dtype)
    view = arena.view(out_shape, out_strides)
    call({n: o[0] for n, o in operands.items()}, view)
    torch.cuda.synchronize()
    assert same(view, out_c), f"{what}: wide out: differs from the compact call"
    assert arena.changed() == math.prod(out_shape), f"{what}: wide out: {arena.changed()} elements written, {math.prod(out_shape)} live"


IP_CASE = (300, 3, 128)  # a row of tests/test_gpu_ip_attention.py's CASES: three query tiles, two key tiles
IP_LDK = 2 ** 25 + 8     # 128 key rows: row 32 starts beyond 2^31 bytes, row 64 beyond 2^32


@pytest.mark.parametrize("dtype", DTYPES)
def test_ip_attention(dtype):
    from nunchaku_amd.ops.attention import ip_attention
    from tests import test_gpu_ip_attention as IP

    Tn, H, N = IP_CASE
    W = H * 128
    assert IP_CASE in IP.CASES and crosses(Tn, LD_255, W) and crosses(N, IP_LDK, W)
    _need(Arena.bytes(span(N, IP_LDK, W)))
    qkv, k, v = IP._inputs(Tn, H, N, dtype)
    q = qkv[:, :W].contiguous()
    out_c = ip_attention(q, k, v, H)
    IP._gate(out_c, q, k, v, H, 1.0 / math.sqrt(128), dtype, f"compact {dtype}")
    ops_ = {"q": (q, (LD_255, 1), span(Tn, LD_255, W)), "k": (k, (IP_LDK, 1), span(N, IP_LDK, W)), "v": (v, (IP_LDK, 1), span(N, IP_LDK, W))}
    _each_wide(dtype, ops_, lambda t, out: ip_attention(t["q"], t["k"], t["v"], H, out=out), out_c, (Tn, W), (LD_255, 1), span(Tn, LD_255, W), "ip_attention")


XA_CASE = (2, 257, 1, 112, [33, 300])  # a row of tests/test_gpu_cross_attention.py's CASES: three query tiles per sample, five key chunks


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_attention(dtype):
    from nunchaku_amd.ops import cross_attention
    from tests import test_gpu_cross_attention as XA

    B, Tn, H, Dh, counts = XA_CASE
    hd, rows, keys = H * Dh, B * Tn, sum(counts)
    assert tuple(XA_CASE) in [tuple(c) for c in XA.CASES] and crosses(rows, LD_510, 128) and crosses(keys, LD_255, hd)
    _need(Arena.bytes(span(keys, LD_255, hd)))
    q, kv, k, v = XA._inputs(B, Tn, H, Dh, counts, dtype)
    k, v = k.contiguous(), v.contiguous()
    kw = dict(cu_seqlens=XA._cu(counts), max_keys=max(counts))
    out_c = cross_attention(q, k, v, H, Dh, **kw)
    XA._gate(out_c, q, k, v, H, Dh, XA._offsets(counts), counts, dtype, f"compact {dtype}")
    ops_ = {"q": (q, (Tn * LD_510, LD_510, 1), span(rows, LD_510, q.shape[-1])), "k": (k, (LD_255, 1), span(keys, LD_255, hd)),
            "v": (v, (LD_255, 1), span(keys, LD_255, hd))}
    _each_wide(dtype, ops_, lambda t, out: cross_attention(t["q"], t["k"], t["v"], H, Dh, out=out, **kw), out_c, (B, Tn, hd), (Tn * LD_510, LD_510, 1),
               span(rows, LD_510, hd), "cross_attention")


PULID_CASE = (130, 256, 8, 1)  # a row of tests/test_gpu_pulid.py's SHAPES: three row tiles
PULID_LD = 2 ** 25 + 8         # 130 rows: row 32 starts beyond 2^31 bytes, row 64 beyond 2^32


@pytest.mark.parametrize("dtype", DTYPES)
def test_pulid_ca(dtype):
    """x wide, then out; the compact call is bit-equal to the launch tests/test_gpu_pulid.py holds to its restatement stage by stage"""
    from nunchaku_amd.ops.attention import pulid_ca
    from tests import pulid_ref
    from tests import test_gpu_pulid as PU

    Tn, C, H, N = PULID_CASE
    assert PULID_CASE in PU.SHAPES and crosses(Tn, PULID_LD, C)
    _need(Arena.bytes(span(Tn, PULID_LD, C)))
    r = PU._run(Tn, C, H, N, dtype, out_scale=0.7)
    fold, stats = r["fold"], r["stats"]
    x = pulid_ref.stream_inputs(Tn, C, Tn + N, PU.TD[dtype], "cuda")
    assert same(x, r["x"])
    out_c, probs_c = pulid_ca(x, fold, out_scale=0.7, stats=stats, return_probs=True)
    assert same(out_c, r["out"]) and same(probs_c, r["probs"]), "compact: differs from the launch held to the restatement"

    def call(t, out):
        got, probs = pulid_ca(t["x"], fold, out_scale=0.7, stats=stats, out=out, return_probs=True)
        assert same(probs, probs_c), "probabilities differ from the compact call"
        return got

    _each_wide(dtype, {"x": (x, (PULID_LD, 1), span(Tn, PULID_LD, C))}, call, out_c, (Tn, C), (PULID_LD, 1), span(Tn, PULID_LD, C), "pulid_ca")


LA_CASE = (3, 300, 5)  # a row of tests/test_gpu_linear_attention.py's SHAPES: two token chunks per sample
LA_BS = 2 ** 30 + 8    # batch stride in elements: sample 1 starts beyond 2^31 bytes, sample 2 beyond 2^32


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_attention(dtype):
    """q, kv and out wide in turn through the C-level op (the packed form has one row stride for q and kv), then B = 3 with the samples 2^30 + 8 elements
    apart.  out and the fp32 sums vk against the packed call on the same values, which tests/test_gpu_linear_attention.py holds to its references."""
    from nunchaku_amd._C import ops
    from nunchaku_amd.ops.attention import linear_attention
    from tests import test_gpu_linear_attention as LA

    B, Tn, H = LA_CASE
    hd, rows = H * 32, B * Tn
    assert LA_CASE in LA.SHAPES and crosses(rows, LD_510, 2 * hd) and LA_BS * 2 >= 2 ** 31
    _need(2 * Arena.bytes(2 * LA_BS + Tn * hd))
    qkv = LA._case(B, Tn, H, dtype)[0].cuda()
    out_c, vk_c = linear_attention(qkv, H, return_vk=True)
    q, kv = qkv[..., :hd].contiguous().unflatten(-1, (H, 32)), qkv[..., hd:].contiguous().unflatten(-1, (H, 64))

    def call(t, out):
        out = torch.zeros(B, Tn, H, 32, dtype=qkv.dtype, device="cuda") if out is None else out
        vk = torch.zeros_like(vk_c)
        ops.linear_attention(t["q"], t["kv"], out, vk)
        assert torch.equal(bits32(vk), bits32(vk_c)), "vk differs from the packed call"
        return out

    o4 = out_c.unflatten(-1, (H, 32))
    assert same(call({"q": q, "kv": kv}, None), o4), "the C-level op on contiguous q / kv differs from the packed call"
    rowwise = lambda w: (Tn * LD_510, LD_510, w, 1)
    ops_ = {"q": (q, rowwise(32), span(rows, LD_510, hd)), "kv": (kv, rowwise(64), span(rows, LD_510, 2 * hd))}
    _each_wide(dtype, ops_, call, o4, (B, Tn, H, 32), rowwise(32), span(rows, LD_510, hd), "linear_attention rows")
    batched = lambda w: (LA_BS, H * w, w, 1)
    ops_ = {"q": (q, batched(32), 2 * LA_BS + Tn * hd), "kv": (kv, batched(64), 2 * LA_BS + Tn * 2 * hd)}
    _each_wide(dtype, ops_, call, o4, (B, Tn, H, 32), batched(32), 2 * LA_BS + Tn * hd, "linear_attention batch stride")


# =======================================================================================================================================
# 8. AWQ W4A16: the rows of x are the only strided operand (the batched GEMVs take one contiguous row: nothing of theirs can be wide)
# =======================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_awq(dtype):
    """M = 8 rows 2^29 - 8 elements apart, at both shapes of GEMV_SINGLE (held to the oracle by tests/test_gpu_dispatch_classes.py)"""
    from nunchaku_amd.ops.gemv import awq_gemv_w4a16_cuda
    from tests.test_gpu_awq import _layer

    m = 8
    _need(Arena.bytes(span(m, ROW_LD, 576)))
    for N, K in D.GEMV_SHAPES:
        assert (m, N, K) in D.GEMV_SINGLE and crosses(m, ROW_LD, K)
        qw, s, z, bias = _layer(N, K, dtype, seed=N + K + m)
        kern = torch.from_numpy(O.pack_awq_w4_ref(qw)).cuda()
        ts, tz, tb = t16(s, dtype), t16(z, dtype), t16(bias, dtype)
        x = t16(O.round16(np.random.default_rng(7 + m).standard_normal((m, K)).astype(np.float32), dtype), dtype)
        out_c = awq_gemv_w4a16_cuda(x, kern, ts, tz, m, N, K, bias=tb)
        arena = Arena(span(m, ROW_LD, K), dtype)
        xv = arena.view((m, K), (ROW_LD, 1), 0, x)
        got = awq_gemv_w4a16_cuda(xv, kern, ts, tz, m, N, K, bias=tb)
        torch.cuda.synchronize()
        assert same(got, out_c), f"N={N} K={K}: wide x differs from the compact call"
        assert arena.holds_only((xv, x))
        del arena, xv
        torch.cuda.empty_cache()


AWQ_GEMM_CASE = (40, 192, 2048, 4)  # a row of AWQ_GEMM_CASES: BM 64, K split four ways
AWQ_GEMM_LD = 2 ** 26 - 8           # 40 rows: row 16 straddles 2^31 bytes, row 32 straddles 2^32, rows 33 .. 39 start beyond it


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_awq(dtype):
    from nunchaku_amd._C import ops

    M, N, K, _ = AWQ_GEMM_CASE
    assert AWQ_GEMM_CASE in D.AWQ_GEMM_CASES and crosses(M, AWQ_GEMM_LD, K)
    _need(Arena.bytes(span(M, AWQ_GEMM_LD, K)))
    dt = TORCH_DT[dtype]
    qw, sc, zr = D.awq_gemm_layer(N, K, dt, seed=M + N + K)
    bias = (torch.randn(N, generator=torch.Generator().manual_seed(N)) * 0.1).to(dt).cuda()
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(M)).to(dt).cuda()
    out_c = ops.gemm_awq(x, qw, sc, zr, bias)
    arena = Arena(span(M, AWQ_GEMM_LD, K), dtype)
    xv = arena.view((M, K), (AWQ_GEMM_LD, 1), 0, x)
    got = ops.gemm_awq(xv, qw, sc, zr, bias)
    torch.cuda.synchronize()
    assert same(got, out_c), "wide x differs from the compact call"
    assert arena.holds_only((xv, x))


# =======================================================================================================================================
# 9. attention's fused output quantiser (rank 32): Q and K wide, read in place from a packed qkv whose rows lie 4210752 elements apart
# =======================================================================================================================================
@pytest.fixture
def strict_mode():
    from nunchaku_amd import mode

    with mode.deterministic_mode("strict"):  # the low-rank sums in fixed point: no fp32 atomics, bit-equal from launch to launch
        yield


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_fused_quantiser(dtype, strict_mode):
    """codes, scales and low-rank sums of the attention epilogue bit-equal to the compact call; the compact call held to the stand-alone quantiser on the
    attention output as tests/test_gpu_attention.py holds it (codes and scales bit for bit, the sums within 2e-3 of the largest)"""
    from nunchaku_amd import layout, mode
    from nunchaku_amd.ops.attention import attention_packed, attention_packed_quantized
    from tests.helpers import make_module

    L, H, R = 512, T.ATTN_H, 32
    K = H * 128
    assert crosses(L, LD_510, 3 * K)
    _need(Arena.bytes(span(L, LD_510, 3 * K)))
    g = torch.Generator(device="cuda").manual_seed(3)
    qkv = torch.randn(L, 3 * K, device="cuda", generator=g).to(TORCH_DT[dtype])
    vt = qkv[:, 2 * K:].t().contiguous()
    lin = make_module(O.make_svdq_layer(K, 128, R, seed=2, dtype=dtype, cheap=True), dtype)
    compact = attention_packed_quantized(qkv, vt, H, lin)
    assert compact is not None
    p = lin.quantize(attention_packed(qkv, vt, H))
    assert torch.equal(layout.unpack_act(compact[0], K), layout.unpack_act(p[0], K)) and torch.equal(layout.unpack_scales(compact[1], L), layout.unpack_scales(p[1], L))
    la_c, la_p = mode.lora_act_to_float(compact[2]), mode.lora_act_to_float(p[2])
    assert (la_c - la_p).abs().max() <= 2e-3 * la_p.abs().max() + 1e-5
    arena = Arena(span(L, LD_510, 3 * K), dtype)
    wide = arena.view((L, 3 * K), (LD_510, 1), 0, qkv)
    sparse = attention_packed_quantized(wide, vt, H, lin)
    torch.cuda.synchronize()
    for what, c, s in zip(("codes", "scales", "lora_act"), compact, sparse):
        assert torch.equal(c.view(torch.int16) if c.element_size() == 2 else c, s.view(torch.int16) if s.element_size() == 2 else s), f"{what} differ from the compact call"
    assert arena.holds_only((wide, qkv))
