"""TeaCache on the GPU: the svdq_modulated_diff kernel against the oracle's restatement of the quantiser's AdaLayerNormZero front end and
the torch-op sequence the reference runs for the distance, and the cached forward of the FLUX engine (computed / skipped steps, launch
counts, refusals) on a small FLUX-shaped model."""

import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import svdq_oracle as O
from tests.helpers import f32, t16

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
PAD = 3  # rows in front of and behind the problem inside the larger buffers


@pytest.fixture(autouse=True)
def _need_gpu(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def tree_depth(rows: int, Cc: int) -> int:
    """Additions a term of svdq_modulated_diff's sums passes through at most (csrc/modulated_diff.hip, the route of residual_diff.hip): a lane
    adds its 8 * ceil(C / 512) elements in sequence, 6 butterfly levels fold the wave, one thread of the finishing kernel adds ceil(rows / 256)
    row sums in sequence, 6 butterfly levels + 2 levels over the four waves fold the workgroup."""
    return 8 * math.ceil(Cc / 512) + 6 + math.ceil(rows / 256) + 8


def _inside(real: torch.Tensor, fill: float) -> torch.Tensor:
    """``real`` as rows [PAD, PAD + M) of a larger buffer whose other rows hold ``fill``; returns the view of the real rows"""
    M, Cc = real.shape
    buf = torch.full((M + 2 * PAD, Cc), fill, dtype=real.dtype, device=real.device)
    buf[PAD:PAD + M] = real
    return buf


def _untouched(buf: torch.Tensor, fill: float) -> bool:
    edge = torch.cat([buf[:PAD], buf[-PAD:]]).float()
    return bool(torch.isnan(edge).all()) if math.isnan(fill) else bool((edge == fill).all())


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(64, 256), (300, 3072), (1027, 3072)], ids=["64x256", "300x3072", "1027x3072"])
def test_modulated_diff_kernel(name, shape):
    """One and six 512-column chunks, a row count that is a multiple of nothing, more than four 256-row blocks for the finishing kernel.
    The rows around the problem are NaN in x and prev and 7.0 in out: they must stay out of the sums and stay as they are."""
    from nunchaku_amd.ops.elementwise import modulated_diff, residual_gate_stats

    dt = DTYPES[name]
    M, Cc = shape
    rng = np.random.default_rng(M + Cc)
    x_np = O.round16(rng.standard_normal((M, Cc)).astype(np.float32) * 2 + 0.5, name)
    scale_np = O.round16(1 + 0.3 * rng.standard_normal(Cc).astype(np.float32), name)  # (the checkpoint's scale carries the +1)
    shift_np = O.round16(0.5 * rng.standard_normal(Cc).astype(np.float32), name)
    nan = float("nan")
    xbuf = _inside(t16(x_np, name), nan)
    x = xbuf[PAD:PAD + M]
    scale, shift = t16(scale_np, name), t16(shift_np, name)
    stats = residual_gate_stats(x)[1]
    ref = O.ln_mod_ref(x_np, stats.cpu().numpy(), scale_np, shift_np, name)
    m_ref = t16(ref, name)
    g = torch.Generator(device="cuda").manual_seed(M)
    prev_real = (m_ref.float() + 0.05 * torch.randn(M, Cc, device="cuda", generator=g)).to(dt)  # m plus 5 % noise: both sums well away from 0
    pbuf = _inside(prev_real, nan)
    prev = pbuf[PAD:PAD + M]
    obuf = torch.full((M + 2 * PAD, Cc), 7.0, dtype=dt, device="cuda")
    out = obuf[PAD:PAD + M]

    got_out, rec = modulated_diff(x, stats, scale, shift, prev=prev, out=out)
    got = rec.read()
    assert got_out.data_ptr() == out.data_ptr()
    # the modulated input: the quantiser's front end as the oracle restates it, bit for bit; the rows around it keep their fill
    assert np.array_equal(f32(out), ref), f"{int((f32(out) != ref).sum())} of {ref.size} elements differ from ln_mod_ref"
    assert _untouched(obuf, 7.0) and _untouched(xbuf, nan) and _untouched(pbuf, nan)
    assert torch.equal(prev, prev_real)  # prev is only read
    # the sums: float64 sums of the same 16-bit terms
    diff_terms, prev_terms = (prev - m_ref).abs(), prev.abs()
    d = tree_depth(M, Cc)
    bound = d * 2.0 ** -24
    assert bound < 2.0 ** -10, f"depth {d}"
    for key, terms in (("sum_diff", diff_terms), ("sum_prev", prev_terms)):
        r64 = terms.double().sum().item()
        rel = abs(got[key] - r64) / r64
        print(f"{name} {shape} {key}: kernel {got[key]!r} float64 {r64!r} rel {rel:.3e} bound d * 2^-24 = {bound:.3e} (d = {d})")
        assert math.isfinite(got[key]) and rel <= bound, f"{key}: relative error {rel:.3e} > {bound:.3e}"
    # the derived 16-bit values: torch's mean (fp32 sum times 1/N, one rounding) and quotient on the kernel's own sums
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(M * Cc), dtype=torch.float32)
    md = (torch.tensor(got["sum_diff"], dtype=torch.float32) * inv).to(dt)
    mp = (torch.tensor(got["sum_prev"], dtype=torch.float32) * inv).to(dt)
    assert got["mean_diff"] == md.item() and got["mean_prev"] == mp.item() and got["ratio"] == (md / mp).item()
    # the torch sequence on the device (layer_norm, *, +, -, abs, mean x 2, /): two means and a quotient, three 16-bit roundings of half a
    # unit (2^-9 bf16, 2^-12 fp16) each -- within four whole units, the bar of the First-Block-Cache decision pass
    m_t = F.layer_norm(x, (Cc,), eps=1e-6) * scale + shift
    t_ratio = ((m_t - prev).abs().mean() / prev.abs().mean()).item()
    print(f"{name} {shape} ratio: kernel {got['ratio']!r} torch sequence {t_ratio!r}")
    assert abs(got["ratio"] - t_ratio) <= 4 * t_ratio * (2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11)
    # bit-reproducible from launch to launch
    obuf2 = torch.full_like(obuf, 7.0)
    _, rec2 = modulated_diff(x, stats, scale, shift, prev=prev, out=obuf2[PAD:PAD + M])
    assert torch.equal(rec.record.view(torch.int32), rec2.record.view(torch.int32)) and torch.equal(obuf.view(torch.int16), obuf2.view(torch.int16))
    # in place: out is prev -- the buffer the engine keeps across steps
    ibuf = pbuf.clone()
    inplace = ibuf[PAD:PAD + M]
    got_in, rec3 = modulated_diff(x, stats, scale, shift, prev=inplace, out=inplace)
    assert got_in.data_ptr() == inplace.data_ptr()
    assert torch.equal(rec3.record.view(torch.int32), rec.record.view(torch.int32))
    assert torch.equal(inplace.view(torch.int16), out.view(torch.int16)) and _untouched(ibuf, nan)
    # no prev: modulate and store only (the first step of a run)
    obuf4 = torch.full_like(obuf, 7.0)
    only, none = modulated_diff(x, stats, scale, shift, out=obuf4[PAD:PAD + M])
    assert none is None and torch.equal(obuf4.view(torch.int16), obuf.view(torch.int16))
    fresh, none = modulated_diff(x, stats, scale, shift)
    assert none is None and fresh.shape == x.shape and torch.equal(fresh.view(torch.int16), out.view(torch.int16))


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
SIDE_H, SIDE_W, T_TXT = 15, 20, 77  # 300 image and 77 text tokens: neither a multiple of 256 -- streams padded to 512 and 256 rows
DIM = 256


def _model(dt, nj=2, ns=2, seed=1):
    from nunchaku_amd.models.flux import FluxTransformerAMD

    return FluxTransformerAMD(num_layers=nj, num_single_layers=ns, dim=DIM, heads=2, in_channels=64, joint_attention_dim=128,
                              pooled_projection_dim=64, torch_dtype=dt, device="cuda").init_synthetic_(seed=seed).eval()


def _inputs(dt, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    n = SIDE_H * SIDE_W
    lat = torch.randn(1, n, 64, device="cuda", generator=g).to(dt)
    enc = torch.randn(1, T_TXT, 128, device="cuda", generator=g).to(dt)
    pooled = torch.randn(1, 64, device="cuda", generator=g).to(dt)
    img_ids = torch.zeros(n, 3, device="cuda")
    img_ids[:, 1] = torch.arange(SIDE_H, device="cuda").repeat_interleave(SIDE_W)
    img_ids[:, 2] = torch.arange(SIDE_W, device="cuda").repeat(SIDE_H)
    return [lat, enc, pooled, torch.tensor([0.7], device="cuda"), img_ids, torch.zeros(T_TXT, 3, device="cuda"), torch.tensor([3.5], device="cuda")]


def _launch_counts(fn):
    """-> (fn(), launches per kernel class) from the library's event counters, every class selected"""
    from nunchaku_amd import _lib

    lib = _lib.load()
    _lib.check(lib.svdq_prof_select(0xFFFFFFFF), "svdq_prof_select")
    _lib.check(lib.svdq_prof_enable(4096), "svdq_prof_enable")
    counts = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        for cname, cls in (("gemm", 0), ("quantize", 1), ("attention", 2), ("gemv", 3)):
            n, ms, work = C.c_int64(0), C.c_double(0), C.c_double(0)
            _lib.check(lib.svdq_prof_read(cls, C.byref(n), C.byref(ms), C.byref(work)), "svdq_prof_read")
            counts[cname] = n.value
    finally:
        lib.svdq_prof_enable(0)
        lib.svdq_prof_select(0xFFFFFFFF)
    return out, counts


def _restated_skip(model, inputs, residual):
    """A skipped step from the engine's own pieces: proj_out(norm_out(hidden_after_embed + previous_residual)) on the real image rows"""
    st = model._prologue(*inputs)
    st.hidden = st.hidden[:, :st.t_img] + residual
    return model._tail(st)


def _restated_residual(model, inputs):
    """What a computed step stores, out of band: the blocks' output on the real image rows minus the embedded latents (the plain forward's
    stages, which update the stream in place -- the embedded latents are copied first), one 16-bit torch subtraction"""
    st = model._prologue(*inputs)
    h0 = st.hidden[0, :st.t_img].clone()
    nj, ns = len(model.blocks), len(model.single_blocks)
    model._launch_mods(st, range(nj), range(ns))
    model._run_joint(st, 0, nj)
    model._join(st)
    model._run_single(st, 0, ns)
    return st.hidden[0, st.p_txt:st.p_txt + st.t_img] - h0


def _restated_modulated_input(model, inputs):
    """block 0's AdaLayerNormZero output on the real image rows in torch ops (shift_msa, scale_msa: chunks 0 and 1 of the projection)"""
    st = model._prologue(*inputs)
    shift_msa, scale_msa = model.blocks[0].mod(st.temb_act).view(6, -1)[:2]
    return F.layer_norm(st.hidden[0, :st.t_img], (DIM,), eps=1e-6) * scale_msa + shift_msa


@pytest.mark.parametrize("fused", [True, False], ids=["fused_norm", "torch_norm"])
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_teacache_forward(name, fused):
    from nunchaku.caching.teacache import TeaCache
    from nunchaku_amd import mode
    from nunchaku_amd.models.flux import FluxTransformerAMD

    dt = DTYPES[name]
    n_img = SIDE_H * SIDE_W
    FluxTransformerAMD.fused_norm = fused
    try:
        with torch.no_grad(), mode.deterministic_mode("runs"):
            model = _model(dt)
            xs = [_inputs(dt, seed=5 + i) for i in range(4)]  # seeded inputs that change per step
            ref0, n_full = _launch_counts(lambda: model(*xs[0]))
            refs = [ref0] + [model(*x) for x in xs[1:]]
            plain = model.forward
            # threshold 0 (never "<"): every step computes, bit-equal to the plain forward; cnt wraps into a second run
            with TeaCache(model, num_steps=4, rel_l1_thresh=0.0):
                for k in range(6):
                    assert torch.equal(model(*xs[k % 4]), refs[k % 4]), f"step {k}: a computed step must equal the plain forward bit for bit"
                    assert model.cnt == (k + 1) % 4 and model.accumulated_rel_l1_distance == 0.0
                    assert model.previous_modulated_input.shape == (n_img, DIM)
            assert model.forward == plain and not hasattr(model, "cnt") and not hasattr(model, "previous_residual")
            # a huge threshold: steps 0 and 3 compute (forced), steps 1 and 2 skip
            with TeaCache(model, num_steps=4, rel_l1_thresh=1e30):
                out, n0 = _launch_counts(lambda: model(*xs[0]))
                assert torch.equal(out, refs[0]) and (n0["gemm"], n0["attention"]) == (n_full["gemm"], n_full["attention"])
                residual, mod_buf = model.previous_residual, model.previous_modulated_input
                assert residual.shape == (n_img, DIM) and torch.isfinite(residual.float()).all()
                assert torch.equal(residual, _restated_residual(model, xs[0])), "previous_residual = hidden_after_blocks - hidden_after_embed"
                kept = residual.clone()
                # the engine hands the kernel block 0's statistics, scale and shift: its modulated input is the torch-op one up to the
                # three 16-bit roundings of a value (half a unit each) and the fp32 statistics
                want = _restated_modulated_input(model, xs[0]).float()
                err = (mod_buf.float() - want).abs().max().item()
                assert err <= 4 * (2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11) * want.abs().max().item(), f"modulated input off by {err}"
                for k in (1, 2):
                    want = _restated_skip(model, xs[k], residual)
                    out, n_skip = _launch_counts(lambda: model(*xs[k]))
                    print(f"{name} fused={fused} step {k}: launches skipped step {n_skip} full step {n_full}, accumulated {model.accumulated_rel_l1_distance}")
                    assert n_skip["gemm"] == 0 and n_skip["attention"] == 0 and n_skip["quantize"] == 0, "a skipped step runs no block"
                    assert torch.equal(out, want) and torch.isfinite(out.float()).all()
                    assert not torch.equal(out, refs[k]), "the inputs changed: a skipped step is not the computed one"
                    assert model.previous_residual is residual and torch.equal(residual, kept), "a skip leaves the stored residual alone"
                    assert model.previous_modulated_input is mod_buf, "one buffer, updated in place"
                    assert 0.0 < model.accumulated_rel_l1_distance < 1e30 and model.cnt == k + 1
                out, n3 = _launch_counts(lambda: model(*xs[3]))
                assert torch.equal(out, refs[3]) and (n3["gemm"], n3["attention"]) == (n_full["gemm"], n_full["attention"])
                assert model.cnt == 0 and model.accumulated_rel_l1_distance == 0.0
                assert model.previous_residual is residual  # (the last step of a run lies in no refresh window: cnt has wrapped to 0)
    finally:
        FluxTransformerAMD.fused_norm = True


def test_skip_window_computes_without_refreshing_the_residual():
    """skip_steps = 1: step 0 runs every block and stores nothing; step 1 is outside the window, the rule says skip, nothing is stored ->
    computed and stored; step 2 skips with that residual."""
    from nunchaku.caching.teacache import TeaCache
    from nunchaku_amd import mode

    dt = torch.bfloat16
    with torch.no_grad(), mode.deterministic_mode("runs"):
        model = _model(dt)
        xs = [_inputs(dt, seed=5 + i) for i in range(3)]
        refs = [model(*x) for x in xs]
        with TeaCache(model, num_steps=4, rel_l1_thresh=1e30, skip_steps=1):
            assert torch.equal(model(*xs[0]), refs[0]) and model.previous_residual is None
            assert torch.equal(model(*xs[1]), refs[1]) and model.previous_residual is not None
            residual = model.previous_residual
            assert torch.equal(residual, _restated_residual(model, xs[1]))
            assert torch.equal(model(*xs[2]), _restated_skip(model, xs[2], residual))


def test_teacache_refusals_on_the_device():
    from nunchaku.caching.diffusers_adapters.flux_v2 import apply_cache_on_transformer
    from nunchaku.caching.teacache import TeaCache
    from nunchaku_amd.graph import CapturedStep

    dt = torch.bfloat16
    with torch.no_grad():
        model = _model(dt, nj=1, ns=1)
        x = _inputs(dt, seed=5)
        decide = lambda ratio_fn: (True, True)
        with TeaCache(model, num_steps=4):
            model(*x)
            two = [torch.cat([t, t]) if i in (0, 1, 2, 3, 6) else t for i, t in enumerate(x)]
            with pytest.raises(ValueError, match="batch 1"):
                model(*two)
            with pytest.raises(ValueError, match="joint_attention_kwargs"):
                model(*x, joint_attention_kwargs={"ip_adapter_image_embeds": None})
            cn = [torch.zeros(1, SIDE_H * SIDE_W, DIM, device="cuda", dtype=dt)]
            with pytest.raises(ValueError, match="ControlNet"):
                model.teacache_forward(*x, controlnet_block_samples=cn, decide=decide)
            with pytest.raises(ValueError, match="ControlNet"):
                model.teacache_forward(*x, controlnet_single_block_samples=cn, decide=decide)
            with pytest.raises(RuntimeError, match="captured"):
                CapturedStep(lambda *inp: model(*inp), x)
            torch.cuda.synchronize()
            assert model.cnt == 3, "one step + the two eager warm-up calls of CapturedStep; a refused call leaves the state machine where it was"
            assert torch.isfinite(model(*x).float()).all()  # and the model still runs afterwards
        model.offload = True
        with pytest.raises(NotImplementedError, match="offloaded"):
            model.teacache_forward(*x, decide=decide)
        del model.offload
        apply_cache_on_transformer(model)  # First-Block Cache switched on on the same model
        with pytest.raises(RuntimeError, match="First-Block Cache"):
            TeaCache(model).__enter__()
        with pytest.raises(RuntimeError, match="First-Block Cache"):
            model.teacache_forward(*x, decide=decide)
