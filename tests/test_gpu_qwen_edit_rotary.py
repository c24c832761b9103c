"""``svdq_qwen_rotary`` on the GPU: all five tables of ``ops.qwen_rotary`` against ``pack_qwen_rotary(*qwen_rope_freqs_multi(..., device="cuda"))``
bit for bit (the kernel moves data; the torch sequence on the same device computes every entry with the same fp32 product and the same
elementwise ``polar``), into buffers filled with NaN first, so a byte the launch leaves out shows.  Then the model under an Edit pipeline's
``img_shapes``: the fused path against the torch-op blocks, the step captured into a graph, First-Block Cache over all real image rows.

Shapes: the smallest at which the work mapping can go wrong -- tables with and without padding rows, the gap in ``"all"``, image rows that
cross a 256-row boundary with a grid boundary inside a 16-row tile of the packed order (24 + 15 = 39), eight grids, two frames, positions
not centred.  The model: 3 blocks of 2 heads x 128 (tests/test_gpu_qwenimage.py), 376 image tokens in two grids and 19 text tokens."""

import pytest
import torch

from tests.flux_ref import psnr_rel

pytestmark = pytest.mark.gpu

ALL = ("img", "txt", "all", "img_cs", "txt_cs")


@pytest.fixture(autouse=True)
def _need_gpu(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


_AXIS = {}


def _axis_tables():
    from nunchaku_amd.models.qwenimage import qwen_rope_axis_tables

    if "t" not in _AXIS:
        _AXIS["t"] = qwen_rope_axis_tables(device="cuda")
    return _AXIS["t"]


def _poisoned(grids, txt_len, tables):
    """torch.empty, then a NaN pattern over every byte"""
    from nunchaku_amd.ops.rotary import qwen_rotary_shapes

    out = {}
    for name in tables:
        t = torch.empty(qwen_rotary_shapes(grids, txt_len)[name], dtype=torch.float32, device="cuda")
        t.view(torch.int32).fill_(0x7FC0BEEF)
        out[name] = t
    return out


def _reference(grids, txt_len, scale_rope=True):
    from nunchaku_amd.models.qwenimage import pack_qwen_rotary, qwen_rope_freqs_multi

    return pack_qwen_rotary(*qwen_rope_freqs_multi(grids, txt_len, scale_rope=scale_rope, device="cuda"))


def _run(grids, txt_len, scale_rope=True, tables=ALL):
    from nunchaku_amd import ops

    pos_cs, neg_cs = _axis_tables()
    out = _poisoned(grids, txt_len, tables)
    got = ops.qwen_rotary(pos_cs, neg_cs, grids, txt_len, scale_rope=scale_rope, tables=tables, out=out)
    assert sorted(got) == sorted(tables) and all(got[k] is out[k] for k in tables)
    return got


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


CASES = {
    "no padding rows": ([(1, 16, 16)], 256, True),
    "padding everywhere and the gap in all": ([(1, 5, 3)], 1, True),
    "three grids across a 256-row boundary": ([(1, 4, 6), (1, 5, 3), (1, 17, 15)], 77, True),
    "eight grids of one token": ([(1, 1, 1)] * 8, 3, True),
    "two frames": ([(2, 3, 3), (1, 2, 2)], 4, True),
    "positions not centred": ([(1, 4, 6), (2, 5, 3)], 7, False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_all_five_tables_equal_the_torch_sequence(case):
    grids, txt_len, scale_rope = CASES[case]
    ref = _reference(grids, txt_len, scale_rope)
    got = _run(grids, txt_len, scale_rope)
    t_img = sum(f * h * w for f, h, w in grids)
    assert ref["img_cs"].shape == (t_img, 64, 2) and ref["all"].shape[1] == (t_img + -t_img % 256) + (txt_len + -txt_len % 256)
    for name in ALL:
        assert not torch.isnan(got[name]).any(), f"{case}: {name} has bytes the launch did not write"
        assert _same_bits(got[name], ref[name]), f"{case}: {name} differs in {(got[name] != ref[name]).sum().item()} entries"
    if case == "three grids across a 256-row boundary":
        assert t_img == 294 and got["img"].shape == (1, 512, 128) and 24 < 39 < 48  # rows 24 and 39: grid boundaries inside tiles 1 and 2


@pytest.mark.parametrize("tables", [("all",), ALL, ("img", "txt"), ("img_cs", "txt_cs"), ("txt_cs",)])
def test_absent_outputs_are_skipped_and_the_others_complete(tables):
    """("all",) is what the model's fused path asks for, all five what its torch-op path asks for"""
    grids, txt_len = [(1, 4, 6), (1, 5, 3), (1, 17, 15)], 77
    ref = _reference(grids, txt_len)
    got = _run(grids, txt_len, tables=tables)
    for name in tables:
        assert _same_bits(got[name], ref[name]), name


def test_two_calls_are_bit_equal_and_allocate_their_own_outputs():
    from nunchaku_amd import ops

    grids, txt_len = [(1, 4, 6), (1, 5, 3), (1, 17, 15)], 77
    pos_cs, neg_cs = _axis_tables()
    a = ops.qwen_rotary(pos_cs, neg_cs, grids, txt_len)
    b = ops.qwen_rotary(pos_cs, neg_cs, grids, txt_len)
    ref = _reference(grids, txt_len)
    assert sorted(a) == sorted(ALL)
    for name in ALL:
        assert a[name] is not b[name] and _same_bits(a[name], b[name]) and _same_bits(a[name], ref[name]), name


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
GRIDS, T_IMG, T_TXT = [(1, 16, 16), (1, 10, 12)], 376, 19
_MODEL = {}


def _model():
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    if "m" not in _MODEL:
        _MODEL["m"] = NunchakuQwenImageTransformer2DModel(num_layers=3, num_attention_heads=2, attention_head_dim=128, in_channels=64, out_channels=16,
                                                          joint_attention_dim=128, device="cuda").init_synthetic_(seed=5).eval()
    return _MODEL["m"]


def _inputs(seed=4, timestep=0.4):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.randn(1, T_IMG, 64, device="cuda", generator=g).bfloat16()
    enc = torch.randn(1, T_TXT, 128, device="cuda", generator=g).bfloat16()
    return [lat, enc, None, torch.tensor([timestep], device="cuda"), [GRIDS]]


def test_model_tables_come_from_the_kernel_and_equal_the_torch_sequence(monkeypatch):
    """what ``_prologue`` hands the blocks: the joint table alone on the fused path, all five on the torch-op path, bit-equal to the torch
    sequence; one grid gives the tables of ``qwen_rope_freqs``; grids that do not add up are refused before anything runs"""
    from nunchaku_amd.models import qwenimage as Q

    model, x = _model(), _inputs()
    calls = []
    real = Q.qwen_rotary
    monkeypatch.setattr(Q, "qwen_rotary", lambda *a, **k: (calls.append(k["tables"]), real(*a, **k))[1])
    ref = _reference(GRIDS, T_TXT)
    with torch.no_grad():
        model.__dict__.pop("_rot_cache", None)
        st = model._prologue(*x)
        assert st.fused and sorted(st.rot) == ["all"] and _same_bits(st.rot["all"], ref["all"])
        assert model._prologue(*x).rot is st.rot and calls == [("all",)]  # kept: one launch per (grids, text length)
        monkeypatch.setattr(Q.NunchakuQwenImageTransformer2DModel, "fused_norm", False)
        assert "fused_norm" not in model.__dict__  # (the class's switch is the one the model reads)
        st = model._prologue(*x)
        assert not st.fused and sorted(st.rot) == sorted(ALL) and all(_same_bits(st.rot[k], ref[k]) for k in ALL)
        one = model._prologue(x[0][:, :256], x[1], None, x[3], [(1, 16, 16)])
        single = Q.pack_qwen_rotary(*Q.qwen_rope_freqs((1, 16, 16), T_TXT, device="cuda"))
        assert not one.fused and all(_same_bits(one.rot[k], single[k]) for k in ALL)
        with pytest.raises(ValueError, match=r"376 image tokens.*has 375"):
            model._prologue(x[0][:, :375], x[1], None, x[3], [GRIDS])
    assert not any("rope" in k for k in model.state_dict())


def test_model_fused_path_matches_the_torch_op_blocks_with_two_grids():
    """tolerance: tests/test_gpu_qwenimage.py::test_qwen_model_fused_passes_match_the_torch_op_blocks (same model, deterministic mode)"""
    from nunchaku_amd import mode
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    model, x = _model(), _inputs()
    outs, ran_fused = {}, {}
    prologue = model._prologue
    with torch.no_grad(), mode.deterministic_mode():
        for fused in (True, False):
            NunchakuQwenImageTransformer2DModel.fused_norm = fused
            try:
                ran_fused[fused] = bool(prologue(*x).fused)
                outs[fused] = model(*x).sample.float()
            finally:
                NunchakuQwenImageTransformer2DModel.fused_norm = True
    assert ran_fused == {True: True, False: False}, "the switch did not select the path"
    assert outs[True].shape == (1, T_IMG, 64)  # every image row: the Edit pipelines cut the noise rows off themselves
    psnr, rel = psnr_rel(outs[True], outs[False])
    print(f"qwen model, two grids, fused vs torch-op blocks: PSNR {psnr:.1f} dB rel {rel:.2e}")
    assert torch.isfinite(outs[True]).all() and psnr > 45.0 and rel < 2.5e-2, (psnr, rel)


def test_model_step_captured_into_a_graph():
    from nunchaku_amd import mode
    from nunchaku_amd.graph import CapturedStep

    model, x = _model(), _inputs()
    with torch.no_grad(), mode.deterministic_mode():
        eager = model(*x).sample.float()
        step = CapturedStep(lambda lat, enc, t: model(lat, enc, None, t, [GRIDS]).sample, [x[0], x[1], x[3]])
        first = step(x[0], x[1], x[3]).clone()
        second = step(x[0], x[1], x[3]).clone()
        torch.cuda.synchronize()
    assert torch.equal(first, second)
    psnr, rel = psnr_rel(first.float(), eager)
    print(f"qwen model, two grids, graph replay vs eager: PSNR {psnr:.1f} dB rel {rel:.2e}")
    assert torch.isfinite(first.float()).all() and psnr > 45.0 and rel < 2.5e-2, (psnr, rel)


def test_forward_cached_with_two_grids(monkeypatch):
    """a miss that stores, then the same call: a hit whose output is the first block's image rows + the stored residual (over ALL real image
    rows, the reference image's included) through the tail -- tests/test_gpu_fbcache_qwen_sana.py's composition"""
    from nunchaku_amd import mode
    from nunchaku_amd.caching import fbcache

    model, x = _model(), _inputs()
    seen = []
    real = fbcache.are_two_tensors_similar
    monkeypatch.setattr(fbcache, "are_two_tensors_similar", lambda *a, **k: (seen.append(real(*a, **k)), seen[-1])[1])
    with torch.no_grad(), mode.deterministic_mode("strict"):
        ref = model(*x).sample
        ctx = fbcache.create_cache_context()
        with fbcache.cache_context(ctx):
            miss = model.forward_cached(*x, residual_diff_threshold=0.12).sample
            assert not seen and torch.equal(miss, ref)
            rest = ctx.get_buffer("multi_hidden_states_residual_0")
            assert rest.shape == ctx.get_buffer("first_multi_hidden_states_residual_0").shape == (1, T_IMG, 256)
            hit = model.forward_cached(*x, residual_diff_threshold=0.12).sample
            assert len(seen) == 1 and bool(seen[0][0]) and float(seen[0][1]) == 0.0
            st = model._prologue(*x)
            model._launch_mods(st, 0, 1)
            model._run_blocks(st, 0, 1)
            st.hidden = torch.cat([st.hidden[:, :T_IMG] + rest, st.hidden[:, T_IMG:]], dim=1)
            want = model._tail(st)
    assert hit.shape == (1, T_IMG, 64) and torch.equal(hit, want)
