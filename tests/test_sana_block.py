"""SANA's block glue, block, stack and model class, the parts that need no GPU: the C ABI (header, bindings, exported symbol, validation
without a launch), the CPU restatement the GPU tests compare against (tests/sana_glue_ref.py), the op wrapper's checks, the modules' names
and shapes, the checkpoint converter and the diffusers-facing class in both of its builds."""

import ctypes as C
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nunchaku_amd import _lib
from nunchaku_amd import build as svdq_build
from tests import sana_glue_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_1600M = dict(num_layers=20, num_attention_heads=70, attention_head_dim=32, num_cross_attention_heads=20, mlp_ratio=2.5)
CFG_600M = dict(num_layers=28, num_attention_heads=36, attention_head_dim=32, num_cross_attention_heads=16, mlp_ratio=2.5)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_and_sources_agree_and_the_abi_version_stays():
    text = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    assert re.search(r"^int svdq_sana_glue\(const svdq_sana_glue_args \*args, void \*stream\);", text, re.M)
    assert re.search(r"^} svdq_sana_glue_args;", text, re.M)
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M)
    assert "this project fixes the reading above" in text  # the contraction the reference's compiler is free to make is named
    assert _lib.ABI_VERSION == 24
    assert _lib.EXPORTS.get("svdq_sana_glue") == (C.c_int, [C.POINTER(_lib.SanaGlueArgs), C.c_void_p])
    assert "sana_glue.hip" in svdq_build.SOURCES and os.path.exists(os.path.join(svdq_build.CSRC, "sana_glue.hip"))
    src = open(os.path.join(svdq_build.CSRC, "sana_glue.hip")).read()
    assert '#include "row_pass.h"' in src and "for_row_class(" in src and "__shared__" not in src and "atomic" not in src.replace("no atomics", "")
    from nunchaku_amd._C import ops

    assert callable(ops.sana_glue)


def test_struct_layout_matches_header(built_lib, tmp_path):
    cname, cls = "svdq_sana_glue_args", _lib.SanaGlueArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "svdq_amd.h")}"', "int main(void) {",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"offsetof({cname}, {f})"


Bv, Tv, Cv, CPv = 3, 5, 2240, 2304


def _args(**over):
    """a call that would pass validation (the pointers are made up: no test below lets it reach a launch)"""
    a = _lib.SanaGlueArgs()
    a.res, a.a, a.timestep, a.gate_table, a.mod_table = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
    a.out, a.out_mod, a.stats = 0x600000, 0x700000, 0x800000
    a.timestep_bs, a.ld_res, a.ld_a, a.ld_out, a.ld_mod = 6 * Cv, CPv, CPv, CPv, CPv
    a.B, a.T, a.C, a.C_pad = Bv, Tv, Cv, CPv
    a.gate_row, a.scale_row, a.shift_row = 2, 4, 3
    a.dtype, a.eps = _lib.SVDQ_BF16, 1e-6
    for k, v in over.items():
        setattr(a, k, v)
    return a


INVALID, UNSUPPORTED = 1, 2
REFUSED = [
    (dict(res=None), INVALID, b"res and one of out / out_mod / stats are required"),
    (dict(out=None, out_mod=None, stats=None), INVALID, b"res and one of out / out_mod / stats are required"),
    (dict(a=None), INVALID, b"gate_row=2 needs a"),
    (dict(gate_row=6), INVALID, b"table rows are 0..5"),
    (dict(scale_row=6), INVALID, b"table rows are 0..5"),
    (dict(scale_row=-1), INVALID, b"table rows are 0..5"),
    (dict(shift_row=6), INVALID, b"table rows are 0..5"),
    (dict(shift_row=-1), INVALID, b"table rows are 0..5"),
    (dict(timestep=None), INVALID, b"out_mod needs timestep and mod_table"),
    (dict(mod_table=None), INVALID, b"out_mod needs timestep and mod_table"),
    (dict(timestep=None, out_mod=None), INVALID, b"a gate needs timestep and gate_table"),
    (dict(gate_table=None), INVALID, b"a gate needs timestep and gate_table"),
    (dict(B=0), INVALID, b"B=0"),
    (dict(T=0), INVALID, b"T=0"),
    (dict(C=0), INVALID, b"C=0"),
    (dict(B=1 << 16, T=1 << 15), INVALID, b"B * T < 2^31"),
    (dict(C=CPv + 8), INVALID, b"C=2312 <= C_pad=2304"),
    (dict(C=Cv + 4), INVALID, b"both multiples of 8"),
    (dict(C_pad=CPv + 4, ld_out=CPv + 8, ld_mod=CPv + 8), INVALID, b"both multiples of 8"),
    (dict(ld_res=Cv - 8), INVALID, b"a stride is smaller than its row"),
    (dict(ld_a=Cv - 8), INVALID, b"a stride is smaller than its row"),
    (dict(ld_out=CPv - 8), INVALID, b"a stride is smaller than its row"),
    (dict(ld_mod=CPv - 8), INVALID, b"a stride is smaller than its row"),
    (dict(timestep_bs=6 * Cv - 8), INVALID, b"a stride is smaller than its row"),
    (dict(ld_res=CPv + 4), INVALID, b"multiple of 8 elements"),
    (dict(ld_a=CPv + 4), INVALID, b"multiple of 8 elements"),
    (dict(ld_out=CPv + 4), INVALID, b"multiple of 8 elements"),
    (dict(ld_mod=CPv + 4), INVALID, b"multiple of 8 elements"),
    (dict(timestep_bs=6 * Cv + 4), INVALID, b"multiple of 8 elements"),
    (dict(res=0x100008), INVALID, b"16-byte aligned"),
    (dict(a=0x200008), INVALID, b"16-byte aligned"),
    (dict(timestep=0x300002), INVALID, b"16-byte aligned"),
    (dict(gate_table=0x400004), INVALID, b"16-byte aligned"),
    (dict(mod_table=0x500008), INVALID, b"16-byte aligned"),
    (dict(out=0x600008), INVALID, b"16-byte aligned"),
    (dict(out_mod=0x700008), INVALID, b"16-byte aligned"),
    (dict(stats=0x800004), INVALID, b"stats 8-byte aligned"),
    (dict(dtype=7), INVALID, b"unknown dtype 7"),
    (dict(eps=-1e-6), INVALID, b"eps must be finite and not negative"),
    (dict(eps=float("inf")), INVALID, b"eps must be finite and not negative"),
    (dict(eps=float("nan")), INVALID, b"eps must be finite and not negative"),
    # width classes without an instantiation: ceil(C_pad / 512) = 9 and 33
    (dict(C=4104, C_pad=4608, ld_res=4608, ld_a=4608, ld_out=4608, ld_mod=4608, timestep_bs=6 * 4104), UNSUPPORTED, b"must be one of"),
    (dict(C=16392, C_pad=16512, ld_res=16512, ld_a=16512, ld_out=16512, ld_mod=16512, timestep_bs=6 * 16392), UNSUPPORTED, b"must be one of"),
]


def test_exported_and_every_validation_error_is_returned_without_a_launch(built_lib):
    raw = C.CDLL(built_lib)
    assert hasattr(raw, "svdq_sana_glue")
    lib = _lib.load()
    assert lib.svdq_abi_version() == 24
    assert lib.svdq_sana_glue(None, None) == 1 and b"NULL" in lib.svdq_last_error()
    for over, want, needle in REFUSED:
        rc = lib.svdq_sana_glue(C.byref(_args(**over)), None)
        msg = lib.svdq_last_error()
        assert rc == want and needle in msg, f"{over}: returned {rc}, {msg!r}"


# ---- the CPU restatement --------------------------------------------------------------------------------------------------------------
def _exact64(res, a, ts, gtab, grow, mtab, srow, hrow, stats):
    """the same formulas in float64 without any rounding or clip: (t, out_mod)"""
    B, T, _ = res.shape
    f = lambda x: np.asarray(x, dtype=np.float64)
    t = f(res)
    if a is not None:
        t = f(a) * (f(ts[:, grow]) + f(gtab[grow]))[:, None] + f(res) if grow is not None else f(a) + f(res)
    mean, rstd = f(stats[:, 0]).reshape(B, T, 1), f(stats[:, 1]).reshape(B, T, 1)
    s = (f(ts[:, srow]) + f(mtab[srow]) + 1.0)[:, None]
    h = (f(ts[:, hrow]) + f(mtab[hrow]))[:, None]
    return t, ((t - mean) * rstd) * s + h


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_restatement_is_exact_where_every_rounding_is(dtype):
    """small integers and a power of two for rstd: every intermediate is a multiple of 1/2 below 128, which bf16's eight bits hold, so the
    restatement equals the float64 evaluation"""
    g = np.random.default_rng(3)
    B, T, Cc = 3, 5, 16
    ints = lambda *s, lo=-3, hi=4: g.integers(lo, hi, size=s).astype(np.float32)
    res, a = ints(B, T, Cc), ints(B, T, Cc)
    ts, gtab, mtab = ints(B, 6, Cc, lo=-2, hi=3), ints(6, Cc, lo=-2, hi=3), ints(6, Cc, lo=-2, hi=3)
    stats = np.stack([ints(B * T, lo=-2, hi=3), 2.0 ** ints(B * T, lo=-1, hi=1)], axis=1).astype(np.float32)
    for grow in (None, 2, 5):
        out, mod = R.sana_glue_ref(res, a, timestep=ts, gate_table=gtab, gate_row=grow, mod_table=mtab, scale_row=4, shift_row=3, stats=stats,
                                   C_pad=128, dtype=dtype)
        t64, m64 = _exact64(res, a, ts, gtab, grow, mtab, 4, 3, stats)
        # t is stored (exact here), the modulation continues from it
        assert np.array_equal(out[..., :Cc].astype(np.float64), t64) and np.array_equal(mod[..., :Cc].astype(np.float64), m64)
        assert not out[..., Cc:].any() and not mod[..., Cc:].any() and out.shape == mod.shape == (B, T, 128)
    out, mod = R.sana_glue_ref(res, None, timestep=ts, mod_table=mtab, scale_row=1, shift_row=0, stats=stats, C_pad=16, dtype=dtype)
    assert np.array_equal(out, res) and np.array_equal(mod.astype(np.float64), _exact64(res, None, ts, None, None, mtab, 1, 0, stats)[1])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_restatement_stays_within_the_bound_of_its_roundings(dtype):
    """Random inputs against float64.  With u the unit roundoff (2^-8 bf16, 2^-11 fp16) and every rounding a factor (1 + d), |d| <= u:
    t = (a * g(1 + d1)(1 + d2) + res)(1 + d3): two roundings on the product and one on the sum, |t - t64| <= u (2 |a g| + |t64|) to first order.
    out_mod: n, mod(scale), (. + 1) and the product n * s are the FOUR roundings on the product path, h and the sum add one each.  The
    rounding of mod(scale) is relative to |mod|, not to |s| = |mod + 1| (which may be far smaller), so
    |m - m64| <= u (|n| (|mod| + |s|) + 2 |n s| + |h| + |m64|) to first order; 1.05 covers the second-order terms (u <= 2^-8)."""
    u = R.UNIT[dtype]
    g = np.random.default_rng(11)
    B, T, Cc = 2, 7, 224
    r16 = lambda x: R.round16(x.astype(np.float32), dtype)
    res, a = r16(g.standard_normal((B, T, Cc))), r16(g.standard_normal((B, T, Cc)))
    ts, gtab, mtab = r16(0.5 * g.standard_normal((B, 6, Cc))), r16(0.5 * g.standard_normal((6, Cc))), r16(0.5 * g.standard_normal((6, Cc)))
    f = lambda x: np.asarray(x, dtype=np.float64)
    for grow in (None, 2):
        t = R.glue_residual(res, a, ts, gtab, grow, dtype)
        ag = f(a) * (f(ts[:, grow]) + f(gtab[grow]))[:, None] if grow is not None else f(a)
        t64 = ag + f(res)
        assert (np.abs(f(t) - t64) <= 1.05 * u * ((2 if grow is not None else 0) * np.abs(ag) + np.abs(t64)) + 1e-30).all()
        stats = R.stats64(t)
        m = R.glue_modulate(t, stats, ts, mtab, 4, 3, dtype)
        _, m64 = _exact64(t, None, ts, None, None, mtab, 4, 3, stats)
        n64 = (f(t) - f(stats[:, 0]).reshape(B, T, 1)) * f(stats[:, 1]).reshape(B, T, 1)
        s64, h64 = (f(ts[:, 4]) + f(mtab[4]) + 1.0)[:, None], (f(ts[:, 3]) + f(mtab[3]))[:, None]
        bound = np.abs(n64) * (np.abs(s64 - 1.0) + np.abs(s64)) + 2 * np.abs(n64 * s64) + np.abs(h64) + np.abs(m64)
        assert (np.abs(f(m) - m64) <= 1.05 * u * bound + 1e-30).all()
        assert np.abs(f(m) - m64).max() > 0  # (the roundings are really there)


def test_restatement_clips_fp16_only_and_rounds_fp16_once():
    ts, tab = np.zeros((1, 6, 8), np.float32), np.zeros((6, 8), np.float32)
    tab[2] = 2.0
    res, a = np.full((1, 1, 8), 100.0, np.float32), np.full((1, 1, 8), 60000.0, np.float32)
    assert (R.glue_residual(res, a, ts, tab, 2, "fp16") == 65504.0).all() and (R.glue_residual(-res, -a, ts, tab, 2, "fp16") == -65504.0).all()
    assert (R.glue_residual(res, a, ts, tab, 2, "bf16") == 119808.0).all()  # 234 * 2^9: no clip, 120000 and then + 100 rounded to eight bits
    # 2049 + 2^-13 lies just above the midpoint of the fp16 neighbours 2048 and 2050: one rounding gives 2050; through fp32 (2049.0, a tie) 2048
    x = np.float64(2049.0) + 2.0 ** -13
    assert R.one_op(np.array([x]), "fp16")[0] == 2050.0 and np.float32(x).astype(np.float16) == 2048.0


# ---- the op wrapper -------------------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_mismatched_arguments_and_cpu_tensors(built_lib):
    from nunchaku_amd.ops import sana_glue
    from nunchaku_amd.ops.elementwise import sana_glue as same

    assert sana_glue is same
    z = lambda *s, dtype=torch.bfloat16: torch.zeros(*s, dtype=dtype)
    res, a, ts, tab = z(2, 5, 224), z(2, 5, 256)[..., :224], z(2, 6 * 224), z(6, 224)
    ok = dict(timestep=ts, gate_table=tab, gate_row=2, mod_table=tab, scale_row=4, shift_row=3)
    with pytest.raises(ValueError, match="res must be a GPU tensor"):
        sana_glue(res, a, **ok)
    with pytest.raises(TypeError, match="res must be bfloat16 or float16"):
        sana_glue(res.float(), a, **ok)
    with pytest.raises(TypeError, match="a must be a torch.bfloat16 tensor"):
        sana_glue(res, a.half(), **ok)
    with pytest.raises(TypeError, match="timestep must be a torch.bfloat16 tensor"):
        sana_glue(res, a, **{**ok, "timestep": ts.half()})
    with pytest.raises(ValueError, match=r"res must be a \[B, T, C\] tensor"):
        sana_glue(res[0], a[0], **ok)
    with pytest.raises(ValueError, match=r"a must be \[2, 5, >= 224\]"):
        sana_glue(res, a[:, :4], **ok)
    with pytest.raises(ValueError, match="unit stride on its last axis"):
        sana_glue(res, z(2, 5, 448)[..., ::2], **ok)
    with pytest.raises(ValueError, match="unit stride on its last axis"):
        sana_glue(z(5, 2, 224).transpose(0, 1), a, **ok)
    with pytest.raises(ValueError, match=r"timestep must be \[2, 6, 224\]"):
        sana_glue(res, a, **{**ok, "timestep": z(3, 6 * 224)})
    with pytest.raises(ValueError, match=r"gate_table must be a contiguous torch.bfloat16 \[6, 224\]"):
        sana_glue(res, a, **{**ok, "gate_table": z(6, 256)})
    with pytest.raises(ValueError, match=r"mod_table must be a contiguous torch.bfloat16 \[6, 224\]"):
        sana_glue(res, a, **{**ok, "mod_table": z(224, 6).t()})
    with pytest.raises(ValueError, match="a gate needs a, gate_table and timestep"):
        sana_glue(res, None, **ok)
    with pytest.raises(ValueError, match="out_mod needs timestep, mod_table, scale_row and shift_row"):
        sana_glue(res, a, timestep=ts, mod_table=tab, scale_row=4)
    with pytest.raises(ValueError, match="gate_row=6: the tables have rows 0..5"):
        sana_glue(res, a, **{**ok, "gate_row": 6})
    with pytest.raises(ValueError, match="nothing to do"):
        sana_glue(res)
    with pytest.raises(ValueError, match=r"out must be \[2, 5, 256\]"):
        sana_glue(res, a, out=z(2, 5, 224), **ok)
    with pytest.raises(ValueError, match=r"out_mod must be \[2, 5, 256\]"):
        sana_glue(res, a, out_mod=z(2, 5, 224), **ok)
    with pytest.raises(ValueError, match="need channels=220"):
        sana_glue(res, a, channels=220, **ok)
    with pytest.raises(ValueError, match="pad_to=128 >= channels"):
        sana_glue(res, a, pad_to=128, **ok)
    with pytest.raises(ValueError, match="eps=-1.0 must be finite and not negative"):
        sana_glue(res, a, eps=-1.0, **ok)
    with pytest.raises(ValueError, match="must live on res's device"):
        sana_glue(res, a.to("meta"), **ok)


# ---- block, stack -----------------------------------------------------------------------------------------------------------------------
def test_intermediate_size_rule():
    from nunchaku_amd.models import sana_intermediate_size

    """ceilDiv(int(round(ratio * dim)), 64) * 64 (SanaModel.cpp:329).  SANA-1.6B: round(2.5 * 2240) = 5600 is no multiple of 64 and goes up to
    5632; the GEMM operands are the same for both (ceil128(5600) = 5632, ceil128(2 * 5600) = 2 * 5632).  SANA-0.6B: 2880 = 45 * 64 stays."""
    from nunchaku_amd.models import SanaGLUMBConv

    assert sana_intermediate_size(1152, 2.5) == 2880 and int(round(2.5 * 2240)) == 5600 and sana_intermediate_size(2240, 2.5) == 5632
    a, b = SanaGLUMBConv(2240, 5600, device="meta"), SanaGLUMBConv(2240, 5632, device="meta")
    assert (a.in_pad, a.c_gemm, a.hid_pad) == (b.in_pad, b.c_gemm, b.hid_pad) == (2304, 11264, 5632)
    assert sana_intermediate_size(128, 2.5) == 320 and sana_intermediate_size(224, 2.5) == 576 and sana_intermediate_size(100, 2.504) == 256


def test_block_and_stack_names_and_shapes_match_the_reference(golden_dir):
    from nunchaku.models.sana import SanaLinearTransformerBlock as MirroredBlock
    from nunchaku.models.sana import SanaModel as MirroredModel
    from nunchaku_amd.models import SanaCrossAttention, SanaGLUMBConv, SanaLinearAttention, SanaLinearTransformerBlock, SanaModel

    assert MirroredBlock is SanaLinearTransformerBlock and MirroredModel is SanaModel
    golden = json.load(open(os.path.join(golden_dir, "sana_block_keys.json")))
    for name, cfg in (("sana_1600m", CFG_1600M), ("sana_600m", CFG_600M)):
        m = SanaModel(dict(cfg, num_layers=3), pag_layers=[1], device="meta")
        dim = cfg["num_attention_heads"] * 32
        assert (m.inner_dim, m.intermediate_size, len(m.transformer_blocks)) == (dim, 5632 if dim == 2240 else 2880, 3)
        assert [b.attn.pag_to_v is not None for b in m.transformer_blocks] == [False, True, False]  # pag_to_v on exactly those layers
        for i, b in enumerate(m.transformer_blocks):
            assert [n for n, _ in b.named_children()] == ["attn", "cross_attn", "ff"]
            assert isinstance(b.attn, SanaLinearAttention) and isinstance(b.cross_attn, SanaCrossAttention) and isinstance(b.ff, SanaGLUMBConv)
            assert tuple(b.scale_shift_table.shape) == (6, dim) and b.scale_shift_table.dtype == torch.bfloat16
            assert b.cross_attn.head_dim == dim // cfg["num_cross_attention_heads"] and b.attn.qkv_proj.bias is None
            assert {k: list(v.shape) for k, v in b.state_dict().items()} == golden[name + ("_pag" if i == 1 else "")]
        assert set(m.state_dict()) == {f"transformer_blocks.{i}.{k}" for i in range(3) for k in golden[name + ("_pag" if i == 1 else "")]}
    # the block golden holds the three layer goldens (SANA-0.6B is what the cross-attention and feed-forward files record)
    for f, prefix in (("sana_cross_attention_keys.json", "cross_attn."), ("sana_ff_keys.json", "ff.")):
        layer = json.load(open(os.path.join(golden_dir, f)))
        assert {prefix + k: v for k, v in layer.items()}.items() <= golden["sana_600m"].items(), f
    assert SanaModel(CFG_600M, pag_layers=8, device="meta").pag_layers == [8]
    with pytest.raises(ValueError, match="outside the 28 layers"):
        SanaModel(CFG_600M, pag_layers=[28], device="meta")
    with pytest.raises(ValueError, match="not a multiple of num_cross_attention_heads"):
        SanaLinearTransformerBlock(1152, 2880, 10, device="meta")
    b = SanaLinearTransformerBlock(224, 576, 2, device="meta")
    mk = lambda *s: torch.empty(*s, dtype=torch.bfloat16, device="meta")
    with pytest.raises(ValueError, match="expected hidden_states"):
        b(mk(2, 15, 128), mk(9, 224), mk(2, 6 * 224), None, torch.empty(3, dtype=torch.int32, device="meta"), 3, 5)
    with pytest.raises(ValueError, match="timestep must be"):
        b(mk(2, 15, 224), mk(9, 224), mk(2, 224), None, torch.empty(3, dtype=torch.int32, device="meta"), 3, 5)


def _legacy(sd):
    out = {}
    for k, v in sd.items():
        k = k.replace("proj_down", "lora_down").replace("proj_up", "lora_up").replace("smooth_factor_orig", "smooth_orig").replace("smooth_factor", "smooth")
        out[k] = torch.empty(v.shape, dtype=v.dtype)
    return out


def test_a_converted_legacy_checkpoint_loads_strictly():
    from nunchaku_amd.models import SanaModel, convert_sana_state_dict

    cfg = dict(num_layers=2, num_attention_heads=7, attention_head_dim=32, num_cross_attention_heads=2, mlp_ratio=2.5)
    sd = SanaModel(cfg, pag_layers=[0], device="meta").state_dict()
    legacy = _legacy(sd)
    legacy["caption_projection.linear_1.smooth"] = torch.empty(3)  # outside transformer_blocks.: not touched, whatever it is called
    assert "transformer_blocks.0.attn.pag_to_v.lora_down" in legacy and "transformer_blocks.1.ff.point_conv.smooth_orig" in legacy
    assert not any(s in k for k in legacy for s in ("proj_down", "proj_up", "smooth_factor"))
    conv = convert_sana_state_dict(legacy)
    assert set(conv) == set(sd) | {"caption_projection.linear_1.smooth"}
    for k in ("transformer_blocks.1.scale_shift_table", "transformer_blocks.0.ff.depth_conv.weight", "transformer_blocks.0.cross_attn.kv_linear.bias"):
        assert conv[k] is legacy[k]
    assert convert_sana_state_dict(conv).keys() == conv.keys()  # names that are already converted pass through
    cpu = SanaModel(cfg, pag_layers=[0])
    quantised = {k: v for k, v in conv.items() if k.startswith("transformer_blocks.")}
    cpu.load_state_dict(quantised, strict=True)
    with pytest.raises(RuntimeError):
        cpu.load_state_dict({k: v for k, v in legacy.items() if k.startswith("transformer_blocks.")}, strict=True)
    with pytest.raises(RuntimeError):
        SanaModel(cfg).load_state_dict(quantised, strict=True)  # a model without pag_to_v does not take a checkpoint layer's silently


# ---- the wrapper's derivations ------------------------------------------------------------------------------------------------------------
def test_mask_and_grid_derivations_agree_with_the_references_expressions():
    from nunchaku_amd.models.transformer_sana import MASK_THRESHOLD, mask_key_counts, token_grid

    B, L = 3, 9
    counts = [9, 4, 0]
    m = torch.full((B, 1, L), -10000.0)
    for b, n in enumerate(counts):
        m[b, 0, :n] = 0.0
    mask, kc, cu = mask_key_counts(m, B, L)
    # the reference's own lines (transformer_sana.py:96-99)
    ref_mask = m.reshape(B, L)
    ref_cu = F.pad((ref_mask > -9000).sum(dim=1).cumsum(dim=0), pad=(1, 0), value=0).to(torch.int32)
    assert MASK_THRESHOLD == -9000 and torch.equal(mask, ref_mask) and torch.equal(cu, ref_cu) and cu.dtype == kc.dtype == torch.int32
    assert kc.tolist() == counts and torch.equal(cu[1:] - cu[:-1], kc)
    # on a prefix mask the padded form's ranges select what the boolean index packs
    cond = torch.arange(B * L * 2, dtype=torch.float32).view(B, L, 2)
    packed = cond[ref_mask > -9000]
    assert torch.equal(packed, torch.cat([cond[b, :n] for b, n in enumerate(counts)]))
    assert torch.equal(mask_key_counts(m.bfloat16(), B, L)[1], kc)
    with pytest.raises(ValueError, match=r"encoder_attention_mask must be \[3, 1, 9\]"):
        mask_key_counts(m[:, 0], B, L)
    with pytest.raises(ValueError, match=r"encoder_attention_mask must be \[3, 1, 9\]"):
        mask_key_counts(None, B, L)
    img_tokens = 1024
    assert token_grid(img_tokens, None, None) == (int(img_tokens ** 0.5),) * 2 == (32, 32)
    assert token_grid(15, None, 5) == (15 // 5, 5) and token_grid(15, 3, None) == (3, 15 // 3) and token_grid(15, 5, 3) == (5, 3)
    for bad in ((15, None, None), (15, 4, None), (15, 4, 4)):
        with pytest.raises(ValueError, match="does not hold 15 tokens"):  # (the reference asserts)
            token_grid(*bad)


# ---- the model class ------------------------------------------------------------------------------------------------------------------------
TINY = dict(num_layers=2, num_attention_heads=4, attention_head_dim=32, num_cross_attention_heads=1, mlp_ratio=2.5, in_channels=4, caption_channels=16)


def _tiny_checkpoint(path, legacy=True):
    from safetensors.torch import save_file

    from nunchaku_amd.models import SanaModel

    torch.manual_seed(0)
    src = SanaModel(TINY, pag_layers=[1])
    with torch.no_grad():
        for p in src.parameters():
            p.copy_(torch.randint(-100, 100, p.shape, dtype=torch.int64) if p.dtype in (torch.int8, torch.int32) else torch.randn(p.shape))
    sd = {k: v.contiguous() for k, v in src.state_dict().items()}
    if legacy:
        sd = {k: sd[k2] for k, k2 in zip(_legacy(sd), sd)}
    sd["caption_projection.linear_1.weight"] = torch.randn(128, 16).bfloat16()
    sd["patch_embed.proj.bias"] = torch.randn(128).bfloat16()
    save_file(sd, path, metadata={"config": json.dumps(TINY), "quantization_config": json.dumps({"rank": 32})})
    return src, sd


def test_diffusers_free_build_loads_the_blocks_and_refuses_forward_and_fp4(tmp_path):
    try:
        import diffusers  # noqa: F401

        return  # the real build is the one in use
    except ImportError:
        pass
    import nunchaku
    from nunchaku.models.transformers.transformer_sana import NunchakuSanaTransformer2DModel as Mirrored
    from nunchaku_amd.models import transformer_sana as ts

    assert nunchaku.NunchakuSanaTransformer2DModel is Mirrored is ts.NunchakuSanaTransformer2DModel and "NunchakuSanaTransformer2DModel" in nunchaku.__all__
    assert not ts.HAVE_DIFFUSERS and issubclass(ts.NunchakuSanaTransformer2DModel, torch.nn.Module)
    path = str(tmp_path / "tiny.safetensors")
    src, sd = _tiny_checkpoint(path)
    m, meta = ts.NunchakuSanaTransformer2DModel.from_pretrained(path, device="cpu", pag_layers=[1], return_metadata=True)
    assert json.loads(meta["config"]) == TINY and m.config.num_layers == 2 and m.dtype == torch.bfloat16 and m.device.type == "cpu"
    assert len(m.transformer_blocks) == 1 and isinstance(m.transformer_blocks[0], ts.NunchakuSanaTransformerBlocks)
    a, b = src.state_dict(), m.transformer_blocks[0].m.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert set(m.unquantized_state_dict) == {"caption_projection.linear_1.weight", "patch_embed.proj.bias"}
    assert torch.equal(m.unquantized_state_dict["patch_embed.proj.bias"], sd["patch_embed.proj.bias"])
    with pytest.raises(RuntimeError, match="diffusers"):
        m(torch.zeros(1, 4, 8, 8))
    with pytest.raises(NotImplementedError, match="NVFP4"):
        ts.NunchakuSanaTransformer2DModel.from_pretrained(path, device="cpu", precision="fp4")
    with pytest.raises(NotImplementedError, match="NVFP4"):
        ts.load_quantized_module(m, sd, device="cpu", use_fp4=True)
    with pytest.raises(RuntimeError):  # strict: the checkpoint has pag_to_v on layer 1, this model would not
        ts.NunchakuSanaTransformer2DModel.from_pretrained(path, device="cpu")
    # the free functions
    q = ts.load_quantized_module(m, path, device="cpu", pag_layers=1)
    assert q.pag_layers == [1] and all(torch.equal(a[k], v) for k, v in q.state_dict().items())
    assert ts.inject_quantized_module(m, q, "cpu") is m and m.transformer_blocks[0].m is q


FAKE_DIFFUSERS = '''
import inspect
import torch
from torch import nn

class FrozenDict(dict):
    def __getattr__(self, k):
        try: return self[k]
        except KeyError: raise AttributeError(k)

class SanaTransformer2DModel(nn.Module):
    """the shape of diffusers' class that matters here: config registration, from_config, a module tree with full-size blocks, a forward
    that walks transformer_blocks with the per-block argument list"""
    def __init__(self, in_channels=32, num_attention_heads=70, attention_head_dim=32, num_layers=20, num_cross_attention_heads=20,
                 caption_channels=2304, mlp_ratio=2.5):
        super().__init__()
        self.config = FrozenDict(in_channels=in_channels, num_attention_heads=num_attention_heads, attention_head_dim=attention_head_dim,
                                 num_layers=num_layers, num_cross_attention_heads=num_cross_attention_heads, caption_channels=caption_channels,
                                 mlp_ratio=mlp_ratio)
        dim = num_attention_heads * attention_head_dim
        self.patch_embed = nn.Module()
        self.patch_embed.proj = nn.Linear(in_channels, dim)
        self.caption_projection = nn.Module()
        self.caption_projection.linear_1 = nn.Linear(caption_channels, dim, bias=False)
        self.transformer_blocks = nn.ModuleList([nn.Linear(dim, dim) for _ in range(num_layers)])

    @classmethod
    def from_config(cls, config):
        expected = set(inspect.signature(cls.__init__).parameters) - {"self", "kwargs"}
        return cls(**{k: v for k, v in config.items() if k in expected})

    @property
    def dtype(self):
        return next(p for n, p in self.named_parameters() if not n.startswith("transformer_blocks.")).dtype

    @property
    def device(self):
        return next(p for n, p in self.named_parameters() if not n.startswith("transformer_blocks.")).device
'''

DIFFUSERS_SCRIPT = '''
import json, sys, torch
sys.path.insert(0, sys.argv[2])
import diffusers
from nunchaku_amd.models import transformer_sana as ts
from tests.test_sana_block import TINY, _tiny_checkpoint
assert ts.HAVE_DIFFUSERS
cls = ts.NunchakuSanaTransformer2DModel
assert issubclass(cls, diffusers.SanaTransformer2DModel) and issubclass(cls, ts.NunchakuModelLoaderMixin)
src, sd = _tiny_checkpoint(sys.argv[1])
m = cls.from_pretrained(sys.argv[1], device="cpu", pag_layers=[1])
assert isinstance(m, diffusers.SanaTransformer2DModel)
assert not any(p.is_meta for p in m.parameters()), "a meta-device parameter of the diffusers skeleton survived"
assert m.config.num_layers == 2 and m.config["in_channels"] == 4          # the FrozenDict diffusers registered
assert len(m.transformer_blocks) == 1 and isinstance(m.transformer_blocks[0], ts.NunchakuSanaTransformerBlocks)
a, b = src.state_dict(), m.transformer_blocks[0].m.state_dict()
assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
assert torch.equal(m.caption_projection.linear_1.weight, sd["caption_projection.linear_1.weight"])   # the unquantised part, strict=False
assert torch.equal(m.patch_embed.proj.bias, sd["patch_embed.proj.bias"])
assert m.dtype == torch.bfloat16 and m.device.type == "cpu" and not hasattr(m, "unquantized_state_dict")
try:
    cls.from_pretrained(sys.argv[1], device="cpu", precision="fp4")
    raise SystemExit("fp4 was not refused")
except NotImplementedError:
    pass
print("OK")
'''


def test_real_subclass_build_against_a_stand_in_diffusers(tmp_path):
    pkg = tmp_path / "diffusers"
    pkg.mkdir()
    (pkg / "__init__.py").write_text(FAKE_DIFFUSERS)
    script = tmp_path / "run.py"
    script.write_text(textwrap.dedent(DIFFUSERS_SCRIPT))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([str(tmp_path), ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "tiny.safetensors"), ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
