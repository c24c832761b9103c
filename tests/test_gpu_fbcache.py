"""First-Block Cache on the GPU: the svdq_residual_diff kernel against the torch-op sequence the reference runs, and the cached
forward of the FLUX engine (hit / miss, both modes, launch counts, refusals) on a small FLUX-shaped model."""

import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(autouse=True)
def _need_gpu(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def tree_depth(rows: int, Cc: int) -> int:
    """Additions a term of svdq_residual_diff's sums passes through at most (csrc/residual_diff.hip): a lane adds its 8 * ceil(C / 512) elements
    in sequence, 6 butterfly levels fold the wave, one thread of the second kernel adds ceil(rows / 256) row sums in sequence, 6 butterfly
    levels + 2 levels over the four waves fold the workgroup."""
    return 8 * math.ceil(Cc / 512) + 6 + math.ceil(rows / 256) + 8


def _problem(shape, dt, seed):
    """prev / base / cur on the device: cur - base is prev plus 5 % noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    M, Cc = shape
    base = (torch.randn(M, Cc, device="cuda", generator=g) * 2).to(dt)
    prev = torch.randn(M, Cc, device="cuda", generator=g).to(dt)
    cur = base + (prev.float() + 0.05 * torch.randn(M, Cc, device="cuda", generator=g)).to(dt)
    return prev, base, cur


@pytest.mark.parametrize("name", ["bf16", "fp16"])
@pytest.mark.parametrize("shape,split", [((4096, 3072), None), ((4608, 3072), (400, 512, 3900)), ((300, 3072), None), ((64, 256), None)],
                         ids=["4096x3072", "two-problems-4608x3072", "300x3072", "64x256"])
def test_residual_diff_kernel_vs_torch_sequence(name, shape, split):
    """Rows that take part: all of them, or -- the (4608, 3072) case -- text rows [0, 400) and image rows [512, 512 + 3900) as two problems;
    every other row (the padding behind each stream, 512 + 4096 rows in all) is NaN in every input and must neither reach the sums nor
    be written."""
    from nunchaku_amd.ops.elementwise import residual_diff

    dt = DTYPES[name]
    prev, base, cur = _problem(shape, dt, seed=shape[0] + shape[1])
    M, Cc = shape
    if split is None:
        ranges = [(0, M)]
    else:
        t, p, i = split
        ranges = [(0, t), (p, p + i)]
        pad = torch.ones(M, dtype=torch.bool, device="cuda")
        for a, b in ranges:
            pad[a:b] = False
        for x in (prev, base, cur):
            x[pad] = float("nan")
    out = torch.full_like(cur, 7.0)
    cut = lambda x: [x[a:b] for a, b in ranges]
    res, rec = residual_diff(cut(cur), cut(base), cut(prev), cut(out))
    got = rec.read()
    real = torch.cat([torch.arange(a, b, device="cuda") for a, b in ranges])
    # the subtraction: torch's 16-bit op, bit for bit; untouched rows keep their fill
    assert torch.equal(out[real], (cur - base)[real])
    if split is not None:
        assert bool((out[pad] == 7.0).all())
    # the sums: float64 sums of the same 16-bit terms
    r = (cur - base)[real]
    diff_terms, prev_terms = (prev[real] - r).abs(), prev[real].abs()
    rows = real.numel()
    d = tree_depth(rows, Cc)
    bound = d * 2.0 ** -24
    assert bound < 2.0 ** -10, f"depth {d}"
    for key, terms in (("sum_diff", diff_terms), ("sum_prev", prev_terms)):
        ref = terms.double().sum().item()
        rel = abs(got[key] - ref) / ref
        print(f"{name} {shape} {key}: kernel {got[key]!r} float64 {ref!r} rel {rel:.3e} bound d * 2^-24 = {bound:.3e} (d = {d})")
        assert rel <= bound, f"{key}: relative error {rel:.3e} > {bound:.3e}"
    # the derived 16-bit values: torch's mean (fp32 sum times 1/N, one rounding) and quotient on the kernel's own sums
    n = rows * Cc
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)
    md = (torch.tensor(got["sum_diff"], dtype=torch.float32) * inv).to(dt)
    mp = (torch.tensor(got["sum_prev"], dtype=torch.float32) * inv).to(dt)
    assert got["mean_diff"] == md.item() and got["mean_prev"] == mp.item() and got["ratio"] == (md / mp).item()
    # and the torch sequence itself on the device (its fp32 sums run in another order): two means and a quotient, three 16-bit roundings of
    # half a unit (2^-9 bf16, 2^-12 fp16) each -- within four whole units
    t_ratio = (diff_terms.mean() / prev_terms.mean()).item()
    assert abs(got["ratio"] - t_ratio) <= 4 * t_ratio * (2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11)
    # bit-reproducible from launch to launch
    out2 = torch.full_like(cur, 7.0)
    _, rec2 = residual_diff(cut(cur), cut(base), cut(prev), cut(out2))
    assert torch.equal(rec.record.view(torch.int32), rec2.record.view(torch.int32)) and torch.equal(out.view(torch.int16), out2.view(torch.int16))
    # subtraction only; comparison of an existing residual (base NULL) gives the same record
    only, none = residual_diff(cut(cur), cut(base))
    assert none is None and all(torch.equal(o, (cur - base)[a:b]) for o, (a, b) in zip(only, ranges))
    _, rec3 = residual_diff(only, prev=cut(prev))
    assert torch.equal(rec3.record.view(torch.int32), rec.record.view(torch.int32))


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_decision_on_the_reference_fixture(golden_dir, name):
    from nunchaku.caching import fbcache

    g, dt = np.load(os.path.join(golden_dir, f"fbcache_{name}.npz")), DTYPES[name]
    thr = float(g["threshold"])
    dev = lambda a: torch.from_numpy(a.view(np.int16).copy()).view(dt).cuda()
    prev = dev(g["sim_prev"])
    for i in range(len(g["amplitudes"])):
        similar, ratio = fbcache.are_two_tensors_similar(prev, dev(g[f"sim_cur_{i}"]), threshold=thr)
        ref = torch.from_numpy(g[f"sim_ratio_{i}"].view(np.int16).copy()).view(dt).float().item()
        print(f"{name} amplitude {g['amplitudes'][i]}: kernel ratio {float(ratio)} reference {ref}")
        assert bool(similar) == bool(g[f"sim_similar_{i}"])
        assert abs(float(ratio) - ref) <= 4 * ref * (2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11)
    # the recorded trace on the device: the same hits and misses through the kernel
    for mode in ("multi", "single"):
        with fbcache.cache_context(fbcache.create_cache_context()):
            for k in range(int(g["steps"])):
                p = f"trace_{mode}_{k}_"
                hit, _ = fbcache.get_can_use_cache(dev(g[p + "first"]), threshold=thr, mode=mode)
                assert bool(hit) == bool(g[p + "hit"]), f"{mode} step {k}"
                if not hit:
                    fbcache.set_buffer(f"first_{mode}_hidden_states_residual", dev(g[p + "first"]))


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
SIDE_H, SIDE_W, T_TXT = 15, 20, 77  # 300 image and 77 text tokens: neither a multiple of 256 -- streams padded to 512 and 256 rows


def _model(dt, nj=2, ns=2, seed=1):
    from nunchaku_amd.models.flux import FluxTransformerAMD

    return FluxTransformerAMD(num_layers=nj, num_single_layers=ns, dim=256, heads=2, in_channels=64, joint_attention_dim=128,
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


def _restated_hit(model, inputs, ctx, double):
    """A hit step in torch ops on the device: block 0's outputs + the stored residuals [, single block 0 + its stored residual], the tail."""
    from nunchaku_amd.ops.elementwise import residual_gate_stats

    def set_streams(st, hidden, enc):  # the statistics that travel with the streams on the fused path: a statistics-only pass
        st.hidden, st.enc = hidden, enc
        if st.fused:
            st.stats = ((residual_gate_stats(hidden)[1], None), (residual_gate_stats(enc)[1], None))

    st = model._prologue(*inputs)
    model._run_joint(st, 0, 1)
    set_streams(st, st.hidden + ctx.get_buffer("multi_hidden_states_residual"), st.enc + ctx.get_buffer("multi_encoder_hidden_states_residual"))
    if double:
        model._join(st)
        model._run_single(st, 0, 1)
        st.hidden = st.hidden + ctx.get_buffer("single_hidden_states_residual")
    return model._tail(st)


@pytest.mark.parametrize("double", [False, True], ids=["single-cache", "double-cache"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused_norm", "torch_norm"])
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_cached_forward(name, fused, double):
    from nunchaku.caching import fbcache
    from nunchaku.caching.diffusers_adapters.flux_v2 import apply_cache_on_transformer
    from nunchaku_amd import mode
    from nunchaku_amd.models.flux import FluxTransformerAMD

    dt = DTYPES[name]
    thr = 0.12
    FluxTransformerAMD.fused_norm = fused
    try:
        with torch.no_grad(), mode.deterministic_mode("strict"):
            model = _model(dt)
            a, b = _inputs(dt, seed=5), _inputs(dt, seed=6)
            (ref_a, n_full) = _launch_counts(lambda: model(*a))
            ref_b = model(*b)
            apply_cache_on_transformer(model, use_double_fb_cache=double, residual_diff_threshold=0.0, residual_diff_threshold_single=0.0)
            # threshold 0 (never "<"): every step a miss, bit-equal to the uncached forward
            with fbcache.cache_context(fbcache.create_cache_context()):
                for x, ref in ((a, ref_a), (b, ref_b), (b, ref_b), (a, ref_a)):
                    assert torch.equal(model(*x), ref), "a miss step must equal the uncached forward bit for bit"
            # the same inputs twice at 0.12: a miss, then a hit with ratio 0
            apply_cache_on_transformer(model, use_double_fb_cache=double, residual_diff_threshold=thr, residual_diff_threshold_single=thr)
            ctx = fbcache.create_cache_context()
            firsts = ["first_multi_hidden_states_residual"] + (["first_single_hidden_states_residual"] if double else [])
            with fbcache.cache_context(ctx):
                assert torch.equal(model(*a), ref_a)
                stored = {k: (ctx.get_buffer(k), ctx.get_buffer(k).clone()) for k in firsts}
                n_img = SIDE_H * SIDE_W
                assert stored[firsts[0]][0].shape == (1, n_img, 256)
                if double:
                    assert stored[firsts[1]][0].shape == (1, T_TXT + n_img, 256)  # the real rows of [text | image]
                for k in firsts:
                    hit, ratio = fbcache.are_two_tensors_similar(stored[k][0], stored[k][1], threshold=thr)
                    assert bool(hit) and float(ratio) == 0.0
                hit_out, n_hit = _launch_counts(lambda: model(*a))
                for k in firsts:  # a hit leaves the stored first residual alone
                    assert ctx.get_buffer(k) is stored[k][0] and torch.equal(stored[k][0], stored[k][1])
                assert torch.equal(hit_out, _restated_hit(model, a, ctx, double))
                assert torch.isfinite(hit_out.float()).all()
                # a hit step launches what ONE uncached step of a (1 joint, 0 | 1 single) model launches
                small = _model(dt, nj=1, ns=1 if double else 0)
                _, n_small = _launch_counts(lambda: small(*a))
                print(f"{name} fused={fused} double={double}: launches hit {n_hit} small model {n_small} full step {n_full}")
                assert n_hit == n_small and n_hit["gemm"] < n_full["gemm"]
                # fresh random latents: a miss.  The ratio synthetic weights give must be clear of the threshold before the decision is trusted
                prev = ctx.get_buffer(firsts[0])
                out_b = model(*b)
                new = ctx.get_buffer(firsts[0])
                assert new is not prev, "a miss stores the new first residual"
                ratio = float(fbcache.are_two_tensors_similar(prev, new, threshold=thr)[1])
                print(f"{name} fused={fused} double={double}: fresh latents give ratio {ratio}")
                assert ratio > 2 * thr, f"ratio {ratio} of fresh latents is not above 2 x threshold: scale the perturbation"
                assert torch.equal(out_b, ref_b)
    finally:
        FluxTransformerAMD.fused_norm = True


def test_cached_forward_refusals():
    from nunchaku.caching import fbcache
    from nunchaku.caching.diffusers_adapters.flux_v2 import apply_cache_on_transformer
    from nunchaku_amd.graph import CapturedStep

    dt = torch.bfloat16
    with torch.no_grad():
        model = _model(dt, nj=1, ns=1)
        x = _inputs(dt, seed=5)
        apply_cache_on_transformer(model)
        with pytest.raises(AssertionError, match="cache_context must be set before"):
            model(*x)
        with fbcache.cache_context(fbcache.create_cache_context()):
            model(*x)
            two = [torch.cat([t, t]) if i in (0, 1, 2, 3, 6) else t for i, t in enumerate(x)]
            with pytest.raises(ValueError, match="batch 1"):
                model(*two)
            cn = [torch.zeros(1, SIDE_H * SIDE_W, 256, device="cuda", dtype=dt)]
            with pytest.raises(ValueError, match="ControlNet"):
                model.engine_forward_cached(*x, controlnet_block_samples=cn)
            with pytest.raises(ValueError, match="ControlNet"):
                model.engine_forward_cached(*x, controlnet_single_block_samples=cn)
            with pytest.raises(RuntimeError, match="captured"):
                CapturedStep(lambda *inp: model(*inp), x)
            torch.cuda.synchronize()
            assert torch.isfinite(model(*x).float()).all()  # and the model still runs afterwards
