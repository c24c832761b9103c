"""SANA's block glue kernel, block, stack and model class on the GPU.

The kernel: ``out`` and ``out_mod`` bit for bit against the CPU restatement (tests/sana_glue_ref.py) fed with the kernel's own statistics, the
statistics against the float64 ones (``oracle.ln_stats_ref``) at ``rtol = atol = 2e-6`` (the tolerance test_gpu_fused_norm.py uses for the same
two-pass fp32 statistics).  The modules: ``torch.equal`` against the same block composed from the three public layers and the glue written
as separate 16-bit torch operations at the rounding points the header states -- the LayerNorm there takes the kernel's ``(mean, rstd)`` (the
kernel tests above are what holds those), everything else is torch's own arithmetic."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import sana_glue_ref as R

pytestmark = pytest.mark.gpu
DTYPES = ["bf16", "fp16"]
TD = R.TORCH_DT
NAN = float("nan")
SHAPES = [(8, 128), (512, 512), (1152, 1152), (2240, 2304), (224, 256)]
BT = [(1, 1), (3, 5), (2, 7)]  # row counts that are no multiple of 4; at (3, 5) the rows of a workgroup belong to two samples
MSA, MLP = (0, 1, 2), (3, 4, 5)  # (shift, scale, gate) rows


def _inputs(B, T, C, dtype, seed=0):
    """16-bit-valued float32 arrays: res, a [B, T, C], timestep [B, 6, C] (every sample its own), two different tables [6, C]"""
    g = np.random.default_rng(seed + 1000 * C + 10 * B + T)
    r16 = lambda x: R.round16(x.astype(np.float32), dtype)
    return dict(res=r16(g.standard_normal((B, T, C))), a=r16(g.standard_normal((B, T, C))), ts=r16(0.5 * g.standard_normal((B, 6, C))),
                gtab=r16(0.5 * g.standard_normal((6, C))), mtab=r16(0.5 * g.standard_normal((6, C))))


class Device:
    """the operands on the GPU inside larger NaN-filled buffers: ``a`` is the first C columns of a C_pad-wide buffer (NaN behind them), the
    outputs sit in buffers with 64 canary columns behind C_pad and 3 canary rows below B * T, the unused rows of timestep can be NaN"""

    def __init__(self, inp, C_pad, dtype, used_rows=range(6)):
        self.B, self.T, self.C = inp["res"].shape
        self.C_pad, self.dtype, td = C_pad, dtype, TD[dtype]
        B, T, C = self.B, self.T, self.C
        cuda = lambda x: R.to_torch(x, dtype).cuda()
        self.res = cuda(inp["res"])
        self.a_wide = torch.full((B, T, C_pad + 8), NAN, dtype=td, device="cuda")
        self.a_wide[..., :C] = cuda(inp["a"])
        self.a = self.a_wide[..., :C]
        ts = inp["ts"].copy()
        ts[:, [i for i in range(6) if i not in used_rows]] = NAN
        self.ts_wide = torch.full((B, 8, C), NAN, dtype=td, device="cuda")  # a batch stride of 8 * C: two NaN rows behind every sample
        self.ts_wide[:, :6] = cuda(ts)
        self.ts = self.ts_wide[:, :6]
        self.gtab, self.mtab = cuda(inp["gtab"]), cuda(inp["mtab"])

    def buffer(self):
        big = torch.full((self.B * self.T + 3, self.C_pad + 64), NAN, dtype=TD[self.dtype], device="cuda")
        return big, big[: self.B * self.T, : self.C_pad].unflatten(0, (self.B, self.T))

    @staticmethod
    def canaries_untouched(big, B, T, C_pad):
        return bool(torch.isnan(big[B * T:]).all() and torch.isnan(big[:, C_pad:]).all())


def _run_and_compare(inp, C_pad, dtype, with_a, gate_row, mod_rows, want_out, other_table=True, what=""):
    """one launch in the given mode against the restatement; returns the kernel's (out, out_mod, stats) as float32 numpy (or None)"""
    from oracle import svdq_oracle as O

    from nunchaku_amd.ops import sana_glue

    used = ([gate_row] if gate_row is not None else []) + (list(mod_rows[:2]) if mod_rows else [])
    d = Device(inp, C_pad, dtype, used_rows=used)
    B, T, C = d.B, d.T, d.C
    big_o, out = d.buffer() if want_out else (None, None)
    big_m, out_mod = d.buffer() if mod_rows else (None, None)
    mtab = d.mtab if other_table else d.gtab
    got_out, got_mod, stats = sana_glue(d.res, d.a if with_a else None, timestep=d.ts if used else None,
                                        gate_table=d.gtab if gate_row is not None else None, gate_row=gate_row,
                                        mod_table=mtab if mod_rows else None, scale_row=mod_rows[1] if mod_rows else None,
                                        shift_row=mod_rows[0] if mod_rows else None, channels=C, pad_to=C_pad,
                                        out=out if want_out else False, out_mod=out_mod if mod_rows else False, want_stats=True)
    torch.cuda.synchronize()
    assert got_out is out and got_mod is out_mod and tuple(stats.shape) == (B * T, 2)
    st = stats.cpu().numpy()
    t = R.glue_residual(inp["res"], inp["a"] if with_a else None, inp["ts"], inp["gtab"], gate_row, dtype)
    np.testing.assert_allclose(st, O.ln_stats_ref(t.reshape(B * T, C)), rtol=2e-6, atol=2e-6, err_msg=f"stats {what}")
    ref_out, ref_mod = R.sana_glue_ref(inp["res"], inp["a"] if with_a else None, timestep=inp["ts"], gate_table=inp["gtab"], gate_row=gate_row,
                                       mod_table=(inp["mtab"] if other_table else inp["gtab"]) if mod_rows else None,
                                       scale_row=mod_rows[1] if mod_rows else None, shift_row=mod_rows[0] if mod_rows else None, stats=st,
                                       C_pad=C_pad, dtype=dtype)
    for name, big, got, ref in (("out", big_o, out, ref_out), ("out_mod", big_m, out_mod, ref_mod)):
        if got is None:
            continue
        assert torch.equal(got.cpu(), R.to_torch(ref, dtype)), f"{name} {what}: {(got.cpu().float() - torch.from_numpy(ref)).abs().max().item()}"
        tail = got[..., C:].cpu().view(torch.int16)
        assert (tail == 0).all(), f"{name} {what}: the tail [C, C_pad) must be +0 (all bits clear)"
        assert Device.canaries_untouched(big, B, T, C_pad), f"{name} {what}: canary columns / rows were written"
    return got_out, got_mod, st


MODES = [  # (with_a, gate_row, (shift, scale) rows or None, want_out, a second table for the modulation)
    ("no a, out + out_mod (the stack's first modulate)", False, None, MSA, True, True),
    ("no a, out_mod only", False, None, MSA, False, True),
    ("a without gate, out + out_mod (cross residual)", True, None, MLP, True, False),
    ("a with gate_msa, out only", True, 2, None, True, True),
    ("a with gate_mlp, out + the next table's out_mod", True, 5, MSA, True, True),
    ("a with gate, out_mod only", True, 2, MLP, False, True),
    ("a without gate, out only", True, None, None, True, True),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T", BT)
@pytest.mark.parametrize("C,C_pad", SHAPES)
def test_kernel_is_bit_equal_to_the_restatement_in_every_mode(C, C_pad, B, T, dtype):
    inp = _inputs(B, T, C, dtype)
    for what, with_a, gate_row, mod_rows, want_out, other in MODES:
        _run_and_compare(inp, C_pad, dtype, with_a, gate_row, mod_rows, want_out, other, what=f"[{what}] C={C} C_pad={C_pad} B={B} T={T} {dtype}")


ROW_NV = (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 32)  # csrc/row_pass.h RowClasses


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nv", ROW_NV)
def test_one_case_per_width_class(nv, dtype):
    """C_pad a whole class, C ragged inside the last pass (C_pad - 136: zero-tail lanes and data lanes in one pass), 2 samples x 3 tokens"""
    C_pad = 512 * nv
    C = C_pad - 136
    assert math.ceil(C_pad / 512) == nv and C % 8 == 0
    inp = _inputs(2, 3, C, dtype, seed=nv)
    _run_and_compare(inp, C_pad, dtype, True, 5, MSA, True, True, what=f"NV={nv} {dtype}")


def test_a_width_class_without_an_instantiation_is_refused():
    from nunchaku_amd.ops import sana_glue

    z = torch.zeros(1, 2, 4608, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(NotImplementedError, match="must be one of"):
        sana_glue(z, z, out=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_out_may_alias_res_and_two_calls_are_bit_equal(dtype):
    from nunchaku_amd.ops import sana_glue

    B, T, C, C_pad = 3, 5, 224, 256
    inp = _inputs(B, T, C, dtype, seed=7)
    d = Device(inp, C_pad, dtype)
    kw = dict(timestep=d.ts, gate_table=d.gtab, gate_row=5, mod_table=d.mtab, scale_row=1, shift_row=0, channels=C, pad_to=C_pad, want_stats=True)
    o1, m1, s1 = sana_glue(d.res, d.a, out=True, out_mod=True, **kw)
    o2, m2, s2 = sana_glue(d.res, d.a, out=True, out_mod=True, **kw)
    assert torch.equal(o1, o2) and torch.equal(m1, m2) and torch.equal(s1, s2)
    wide = torch.full((B, T, C_pad), NAN, dtype=TD[dtype], device="cuda")  # the stream as the block keeps it: res in a C_pad-wide buffer
    wide[..., :C] = d.res
    o3, m3, s3 = sana_glue(wide, d.a, out=wide, out_mod=True, **kw)
    assert o3 is wide and torch.equal(wide, o1) and torch.equal(m3, m1) and torch.equal(s3, s1)


def test_fp16_products_past_65504_are_clipped_and_the_statistics_see_the_clipped_value():
    from oracle import svdq_oracle as O

    B, T, C = 2, 3, 16
    inp = _inputs(B, T, C, "fp16", seed=3)
    inp["ts"][:, 2], inp["gtab"][2] = 1.0, 1.0                       # gate = 2
    inp["a"][0, :, ::4] = 60000.0                                    # 120000: past the fp16 range; sample 0 upwards, sample 1 downwards (a row
    inp["a"][1, :, ::4] = -60000.0                                   # with both would cancel in the mean, which rtol could not judge)
    inp["ts"][:, 4], inp["mtab"][4], inp["ts"][:, 3], inp["mtab"][3] = 30000.0, 30000.0, 40000.0, 30000.0  # scale 60001 -> 60000, shift inf -> 65504
    out, mod, st = _run_and_compare(inp, 128, "fp16", True, 2, MLP, True, True, what="fp16 clip")
    o = out.cpu().float()
    assert (o[0, :, 0:C:4] == 65504.0).all() and (o[1, :, 0:C:4] == -65504.0).all() and torch.isfinite(o).all()
    ref_t = R.glue_residual(inp["res"], inp["a"], inp["ts"], inp["gtab"], 2, "fp16")
    assert ref_t.max() == 65504.0 and ref_t.min() == -65504.0
    np.testing.assert_allclose(st, O.ln_stats_ref(ref_t.reshape(B * T, C)), rtol=2e-6, atol=2e-6)  # the statistics of the clipped values
    m = mod.cpu().float()[..., :C]
    assert torch.isfinite(m).all() and (m.abs() == 65504.0).any()
    # bf16 has the range: the same inputs pass unclipped
    inp16 = {k: R.round16(v, "bf16") for k, v in inp.items()}
    out_b, _, _ = _run_and_compare(inp16, 128, "bf16", True, 2, MLP, True, True, what="bf16, the fp16 clip inputs")
    assert out_b.cpu().float().abs().max() > 1e5


def test_the_call_captures_and_replays():
    from nunchaku_amd.ops import sana_glue

    B, T, C, C_pad = 3, 5, 224, 256
    inp = _inputs(B, T, C, "bf16", seed=9)
    d = Device(inp, C_pad, "bf16")
    kw = dict(timestep=d.ts, gate_table=d.gtab, gate_row=5, mod_table=d.mtab, scale_row=1, shift_row=0, channels=C, pad_to=C_pad)
    want_o, want_m, _ = sana_glue(d.res, d.a, out=True, out_mod=True, **kw)
    out, out_mod = torch.empty_like(want_o), torch.empty_like(want_m)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sana_glue(d.res, d.a, out=out, out_mod=out_mod, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_o) and torch.equal(out_mod, want_m)
    d.res.neg_()  # a replay reads what the buffers hold then
    graph.replay()
    o2, m2, _ = sana_glue(d.res, d.a, out=True, out_mod=True, **kw)
    assert torch.equal(out, o2) and torch.equal(out_mod, m2) and not torch.equal(out, want_o)


# ---- block, stack, wrapper, model -----------------------------------------------------------------------------------------------------------
CONFIGS = {  # dim -> config: 128 = 4 x 32, cross 1 x 128, no padding of the stream; 224 = 7 x 32, cross 2 x 112, dim_pad 256, hid_pad 640 != C_gemm / 2
    128: dict(num_layers=3, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=1, mlp_ratio=2.5),
    224: dict(num_layers=3, num_attention_heads=7, attention_head_dim=32, num_cross_attention_heads=2, mlp_ratio=2.5),
}
GRID = (3, 5)
PAG_LAYERS = [1]


@pytest.fixture
def strict_mode():
    from nunchaku_amd import mode

    with mode.deterministic_mode("strict"):
        yield


def _random_state_dict(model, seed):
    """random W4A4 layers (oracle.make_svdq_layer, as test_gpu_cross_attention.py::_layer builds them) and random 16-bit parameters; every
    block gets a different scale_shift_table"""
    from oracle import svdq_oracle as O
    from tests.helpers import reference_state_dict

    from nunchaku_amd.models.linear import SVDQW4A4Linear

    g = torch.Generator().manual_seed(seed)
    sd, n = {}, 0
    for name, mod in model.named_modules():
        if isinstance(mod, SVDQW4A4Linear):
            n += 1
            L = O.make_svdq_layer(mod.in_features, mod.out_features, 32, seed=seed * 100 + n, dtype="bf16", bias=mod.bias is not None, cheap=True)
            sd.update({f"{name}.{k}": v for k, v in reference_state_dict(L, "bf16").items()})
    for k, v in model.state_dict().items():
        if k in sd:
            continue
        scale = v.shape[-1] ** -0.5 if k.endswith("kv_linear.weight") else 1 / 3 if k.endswith("depth_conv.weight") else 0.5 if k.endswith("scale_shift_table") else 0.1
        sd[k] = (torch.randn(v.shape, generator=g) * scale).to(torch.bfloat16)
    return sd


_MODELS = {}


def _model(dim):
    """one model per configuration, built once and left unchanged"""
    from nunchaku_amd.models import SanaModel

    if dim not in _MODELS:
        m = SanaModel(CONFIGS[dim], pag_layers=PAG_LAYERS, device="cuda")
        sd = _random_state_dict(m, seed=dim)
        m.load_state_dict(sd, strict=True)
        tabs = [b.scale_shift_table for b in m.transformer_blocks]
        assert not torch.equal(tabs[0], tabs[1]) and not torch.equal(tabs[1], tabs[2])
        _MODELS[dim] = (m, sd)
    return _MODELS[dim]


def _acts(dim, B, counts, seed=0):
    g = torch.Generator().manual_seed(seed + dim + B)
    T = GRID[0] * GRID[1]
    x = torch.randn(B, T, dim, generator=g).to(torch.bfloat16).cuda()
    ts = (0.5 * torch.randn(B, 6 * dim, generator=g)).to(torch.bfloat16).cuda()
    L = 24
    cond_pad = torch.randn(B, L, dim, generator=g).to(torch.bfloat16).cuda()
    packed = torch.cat([cond_pad[b, :n] for b, n in enumerate(counts)])
    cu = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device="cuda")
    kc = torch.tensor(counts, dtype=torch.int32, device="cuda")
    return x, ts, cond_pad, packed, cu, kc


def _composed_block(block, x, packed, cu, ts, H, W, pag, cfg):
    """the block from its three public layers and separate 16-bit torch operations (SanaModel.cpp:250-312); the LayerNorm from the kernel's
    statistics: n = ((x - mean) * rstd) in fp32, rounded once"""
    from nunchaku_amd.ops import sana_glue

    B, T, dim = x.shape
    mod = ts.view(B, 6, dim) + block.scale_shift_table[None]                                   # mul_add_batch(timestep, {}, ..., table)
    shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp = (mod[:, i:i + 1] for i in range(6))

    def norm(h):
        st = sana_glue(h, want_stats=True, channels=dim)[2].view(B, T, 2)
        return ((h.float() - st[..., 0:1]) * st[..., 1:2]).to(h.dtype)

    n = norm(x) * (scale_msa + 1) + shift_msa
    a = block.attn.forward_pag(n, cfg) if pag else block.attn(n)
    h = a * gate_msa + x
    h = block.cross_attn(h, packed, None, cu) + h
    n = norm(h) * (scale_mlp + 1) + shift_mlp
    return block.ff(n, H, W) * gate_mlp + h


BLOCK_CASES = [  # (B, pag, cfg, text counts) -- one sample with few keys
    (2, False, False, [24, 3]),
    (3, True, True, [17, 1, 24]),
    (2, True, False, [5, 20]),
]


@pytest.mark.parametrize("B,pag,cfg,counts", BLOCK_CASES, ids=["B2", "B3-pag-cfg", "B2-pag"])
@pytest.mark.parametrize("dim", sorted(CONFIGS))
def test_block_equals_its_composition_and_the_padded_form(dim, B, pag, cfg, counts, strict_mode):
    m, _ = _model(dim)
    block = m.transformer_blocks[1]  # the layer with pag_to_v
    assert block.dim_pad == (128 if dim == 128 else 256) and (dim == 128 or (block.ff.hid_pad == 640 and 2 * block.ff.hid_pad != block.ff.c_gemm))
    x, ts, cond_pad, packed, cu, kc = _acts(dim, B, counts)
    x0 = x.clone()
    y = block(x, packed, ts, None, cu, *GRID, pag, cfg)
    assert y.shape == (B, GRID[0] * GRID[1], dim) and y.dtype == torch.bfloat16 and torch.isfinite(y).all() and y.float().abs().max() > 0.01
    assert torch.equal(x, x0), "the block must not write into its input"
    want = _composed_block(block, x, packed, cu, ts, *GRID, pag, cfg)
    assert torch.equal(y, want), (y.float() - want.float()).abs().max().item()
    assert torch.equal(block.forward_padded(x, cond_pad, ts, kc, *GRID, pag, cfg), y)  # packed and padded: bit-equal
    if pag:  # the perturbed samples really take the other path
        assert not torch.equal(block(x, packed, ts, None, cu, *GRID, False, cfg), y)


@pytest.mark.parametrize("dim", sorted(CONFIGS))
def test_stack_equals_chained_layers(dim, strict_mode):
    m, _ = _model(dim)
    B, counts = 3, [17, 1, 24]
    x, ts, cond_pad, packed, cu, kc = _acts(dim, B, counts, seed=1)
    args = (packed, ts, None, cu, *GRID)
    for pag in (False, True):
        y = m(x, *args, pag, True)
        h = x
        for i in range(3):
            h = m.forward_layer(i, h, *args, pag, True)
        assert torch.equal(y, h), f"pag={pag}: {(y.float() - h.float()).abs().max().item()}"
        h = x
        for i in (1, 2):
            h = m.forward_layer(i, h, *args, pag, True)
        assert torch.equal(m(x, *args, pag, True, True), h), f"skip_first_layer, pag={pag}"
    # PAG applies on pag_layers only: layers 0 and 2 have no pag_to_v and ignore the flag, layer 1 does not
    assert torch.equal(m.forward_layer(0, x, *args, True, True), m.forward_layer(0, x, *args, False, True))
    assert not torch.equal(m.forward_layer(1, x, *args, True, True), m.forward_layer(1, x, *args, False, True))
    assert not torch.equal(m(x, *args, True, True), m(x, *args, False, True))
    # (every block has its own table: a pass behind a feed-forward that modulated with its own block's table, not the next one's, fails above)
    assert torch.equal(m.forward_padded(x, cond_pad, ts, kc, *GRID, True, True), m(x, *args, True, True))


@pytest.mark.parametrize("dim", sorted(CONFIGS))
def test_wrapper_packed_and_padded_agree_and_count_three_glue_launches_per_block(dim, strict_mode, monkeypatch):
    from nunchaku_amd.models import sana as sana_mod
    from nunchaku_amd.models.transformer_sana import NunchakuSanaTransformerBlocks

    m, _ = _model(dim)
    B, counts, L = 3, [17, 1, 24], 24
    x, ts, cond_pad, packed, cu, kc = _acts(dim, B, counts, seed=2)
    mask = torch.full((B, 1, L), -10000.0, device="cuda", dtype=torch.bfloat16)
    for b, n in enumerate(counts):
        mask[b, 0, :n] = 0
    calls = []
    real = sana_mod.sana_glue
    monkeypatch.setattr(sana_mod, "sana_glue", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    padded = NunchakuSanaTransformerBlocks(m, torch.bfloat16, "cuda")
    packing = NunchakuSanaTransformerBlocks(m, torch.bfloat16, "cuda", pack_condition=True)
    kw = dict(encoder_hidden_states=cond_pad, encoder_attention_mask=mask, timestep=ts, height=GRID[0], width=GRID[1])
    y = padded(x.float(), **kw)
    assert len(calls) == 3 * 3 + 1, f"{len(calls)} glue launches for 3 blocks"
    assert y.dtype == torch.float32 and torch.equal(y, m(x, packed, ts, None, cu, *GRID, True, True).float())  # B % 3 == 0: pag, cfg
    assert torch.equal(packing(x.float(), **kw), y)
    del calls[:]
    assert torch.equal(padded(x, skip_first_layer=True, **kw), packing(x, skip_first_layer=True, **kw)) and len(calls) == 2 * (3 * 2 + 1)
    del calls[:]
    one = padded.forward_layer_at(1, x, **kw)
    assert len(calls) == 4 and torch.equal(one, packing.forward_layer_at(1, x, **kw)) and torch.equal(one, m.forward_layer(1, x, packed, ts, None, cu, *GRID, True, True))
    with pytest.raises(ValueError, match="does not hold 15 tokens"):
        padded(x, **{**kw, "height": 4, "width": None})


def test_the_padded_path_captures_and_replays(strict_mode):
    m, _ = _model(224)
    B, counts = 3, [17, 1, 24]
    x, ts, cond_pad, packed, cu, kc = _acts(224, B, counts, seed=3)
    want = m.forward_padded(x, cond_pad, ts, kc, *GRID, True, True)  # (also warms up every allocation and cached conversion)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = m.forward_padded(x, cond_pad, ts, kc, *GRID, True, True)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)
    kc.copy_(torch.tensor([3, 24, 0], dtype=torch.int32, device="cuda"))  # the counts are read on the device at replay time
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, m.forward_padded(x, cond_pad, ts, kc, *GRID, True, True)) and not torch.equal(y, want)


def test_a_checkpoint_round_trip_through_from_pretrained_reproduces_the_output(tmp_path, strict_mode):
    from safetensors.torch import save_file

    from nunchaku_amd.models import transformer_sana as tsana

    m, _ = _model(224)
    B, counts, L = 3, [17, 1, 24], 24
    x, ts, cond_pad, packed, cu, kc = _acts(224, B, counts, seed=4)
    want = m.forward_padded(x, cond_pad, ts, kc, *GRID, True, True)
    path = str(tmp_path / "sana_tiny.safetensors")
    sd = {k: v.detach().cpu().contiguous() for k, v in m.state_dict().items()}
    sd["caption_projection.linear_1.bias"] = torch.zeros(224, dtype=torch.bfloat16)
    save_file(sd, path, metadata={"config": json.dumps(CONFIGS[224]), "quantization_config": json.dumps({"rank": 32})})
    if tsana.HAVE_DIFFUSERS:  # the class then builds diffusers' own skeleton (tests/test_sana_block.py runs that build): the loader alone
        from types import SimpleNamespace

        net = SimpleNamespace(config=CONFIGS[224], dtype=torch.bfloat16)
        fresh = tsana.inject_quantized_module(net, tsana.load_quantized_module(net, path, device="cuda", pag_layers=PAG_LAYERS), "cuda")
    else:
        fresh = tsana.NunchakuSanaTransformer2DModel.from_pretrained(path, device="cuda", pag_layers=PAG_LAYERS)
        assert set(fresh.unquantized_state_dict) == {"caption_projection.linear_1.bias"}
        with pytest.raises(RuntimeError, match="diffusers"):
            fresh(x)
    blocks = fresh.transformer_blocks[0]
    assert blocks.m is not m
    mask = torch.full((B, 1, L), -10000.0, device="cuda", dtype=torch.bfloat16)
    for b, n in enumerate(counts):
        mask[b, 0, :n] = 0
    got = blocks(x, encoder_hidden_states=cond_pad, encoder_attention_mask=mask, timestep=ts, height=GRID[0], width=GRID[1])
    assert torch.equal(got, want)
