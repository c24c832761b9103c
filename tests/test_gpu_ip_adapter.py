"""IP-Adapter on the GPU: the small FLUX-shaped transformer of tests/test_flux_block_parity.py (1 joint + 1 single block, hidden 256 =
2 heads x 128) with an adapter (cross_dim 128) against the CPU twin of tests/ipa_ref.py, the fused path against the torch-op arm, and
the interplay with ControlNet residuals, First-Block Cache and a batch."""

import pytest
import torch

from tests.flux_ref import fill_model_, psnr_rel, r16, synthetic_inputs
from tests.ipa_ref import IPARef, adapter_state_dict

pytestmark = pytest.mark.gpu

CROSS = 128
# K / V projection weights are randn * WEIGHT_SCALE / sqrt(cross_dim).  At 0.5 the image-prompt attention output has about 0.3 of the
# image stream's RMS (this model's stream has RMS 1): a contribution the output clearly depends on -- without the adapter the result is
# far (< 40 dB) from the twin's -- that does not exceed the stream it is added to.  The add has no gate, and the adapter's query is a
# second 4-bit projection of the block's OUTPUT: the GPU's and the twin's streams agree there to ~65 dB, a 16-bit step apart on some
# elements, which flips 4-bit codes of that projection's input, so the two queries agree to ~43 dB only (the twin's projection of the
# GPU's own stream agrees with the GPU's query far better).  A larger WEIGHT_SCALE would weigh this inherent code-flip noise of the reference's
# arithmetic, not the adapter's code, against the gate.
WEIGHT_SCALE = 0.5


def _small(num_layers=1, num_single_layers=1):
    from nunchaku_amd.models.flux import FluxTransformerAMD

    model = FluxTransformerAMD(num_layers=num_layers, num_single_layers=num_single_layers, dim=256, heads=2, in_channels=64,
                               joint_attention_dim=128, pooled_projection_dim=64, guidance_embeds=True, device="cuda")
    layers = fill_model_(model, seed=0)
    return model.eval(), layers


def _adapter(model, n_ip, scale, seed=0):
    """attach a synthetic adapter; -> (state dict, image embeddings [1, n_ip, CROSS] on the CPU as float32 of 16-bit values)"""
    from nunchaku.models.ip_adapter.diffusers_adapters.flux import apply_IPA_on_transformer

    sd = adapter_state_dict(len(model.transformer_blocks), CROSS, 256, seed=seed, weight_scale=WEIGHT_SCALE)
    apply_IPA_on_transformer(model, ip_adapter_scale=scale, repo_id=sd)
    emb = r16(torch.randn(1, n_ip, CROSS, generator=torch.Generator().manual_seed(100 + n_ip)))
    return sd, emb


def _args(lat, enc, pooled, img_ids, txt_ids, t=0.7):
    cuda = lambda x: x.cuda().bfloat16()[None]
    return (cuda(lat), cuda(enc), pooled.cuda().bfloat16(), torch.tensor([t]).cuda(), img_ids.cuda(), txt_ids.cuda(), torch.tensor([3.5]).cuda())


def _count_ip_attention(fn):
    """run fn() with ``ops.ip_attention`` wrapped: (result, calls)"""
    from nunchaku_amd._C import ops

    calls, orig = [], ops.ip_attention

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    ops.ip_attention = counted
    try:
        return fn(), len(calls)
    finally:
        del ops.ip_attention  # (the instance attribute; the class's static method is uncovered again)


@pytest.mark.parametrize("grid,t_txt", [(16, 128), ((13, 20), 77)], ids=["aligned", "padded"])
@pytest.mark.parametrize("n_ip,scale", [(4, 1.0), (20, 0.7)], ids=["n4-s1.0", "n20-s0.7"])
def test_adapter_matches_the_twin(grid, t_txt, n_ip, scale):
    """The gate is the one of the sibling tests of tests/test_flux_block_parity.py, whose measured values are 54 - 58.6 dB.  Measured here
    (MI355X, profiles/ip_adapter.txt): N_ip 4 / scale 1.0: 54.1 dB aligned, 53.0 dB padded; N_ip 20 / scale 0.7: 54.6 and 53.6 dB; the
    same calls without the adapter 24.0 - 34.4 dB."""
    model, layers = _small()
    sd, emb = _adapter(model, n_ip, scale)
    lat, enc, pooled, img_ids, txt_ids = synthetic_inputs(grid, t_txt, 128, 64, seed=21)
    args = _args(lat, enc, pooled, img_ids, txt_ids)
    t, gd = torch.tensor([0.7]), torch.tensor([3.5])
    with torch.no_grad():
        (got, calls) = _count_ip_attention(lambda: model.engine_forward(*args, ip_hidden_states=[emb.cuda().bfloat16()])[0].float().cpu())
        model.ip_adapter.set_ip_hidden_states(emb.cuda().bfloat16())
        stored, calls_stored = _count_ip_attention(lambda: model(*args)[0].float().cpu())  # the stored embeddings serve a call that passes none
        ref = IPARef(model, layers, sd, emb, scale).forward(lat, enc, pooled, t, img_ids, txt_ids, gd)
        from nunchaku.models.ip_adapter.utils import undo_all_mods_on_transformer

        undo_all_mods_on_transformer(model)
        plain = model(*args)[0].float().cpu()
    assert calls == 1, f"ops.ip_attention ran {calls} times for one joint block"
    assert got.shape == ref.shape and torch.isfinite(got).all()
    psnr, rel = psnr_rel(stored, ref)
    assert calls_stored == 1 and psnr > 50.0 and rel < 1.5e-2
    psnr, rel = psnr_rel(got, ref)
    print(f"adapter N_ip={n_ip} scale={scale} {grid}+{t_txt}: PSNR {psnr:.1f} dB, relative L2 {rel:.3e}; without the adapter {psnr_rel(plain, ref)[0]:.1f} dB")
    assert psnr > 50.0 and rel < 1.5e-2
    assert psnr_rel(plain, ref)[0] < 40.0  # the adapter matters: without it the output is somewhere else


def test_fused_path_equals_torch_op_arm():
    """the same inputs through the fused path (svdq_ip_attention + one residual / statistics pass) and through the reference's op
    sequence (F.layer_norm, modulation, the QKV projection, SDPA, ``hidden + scale * o``): the bar of
    test_padded_path_equals_unpadded_torch_op_path_rows"""
    from nunchaku_amd.models.flux import FluxAttentionAMD

    model, _ = _small()
    _, emb = _adapter(model, 20, 0.7)
    args = _args(*synthetic_inputs((13, 20), 77, 128, 64, seed=9), t=0.4)
    ip = emb.cuda().bfloat16()
    with torch.no_grad():
        a, n_a = _count_ip_attention(lambda: model.engine_forward(*args, ip_hidden_states=ip)[0].float())
        FluxAttentionAMD.padded_tokens, model.fused_norm = False, False
        try:
            b, n_b = _count_ip_attention(lambda: model.engine_forward(*args, ip_hidden_states=ip)[0].float())
        finally:
            FluxAttentionAMD.padded_tokens, model.fused_norm = True, True
        model.set_attention_impl("flashattn2")  # fused blocks around a torch-op adapter step
        try:
            c, n_c = _count_ip_attention(lambda: model.engine_forward(*args, ip_hidden_states=ip)[0].float())
        finally:
            model.set_attention_impl("nunchaku-fp16")
    assert (n_a, n_b, n_c) == (1, 0, 0)
    psnr = psnr_rel(a.cpu(), b.cpu())[0]
    psnr_c = psnr_rel(a.cpu(), c.cpu())[0]
    print(f"adapter: fused path vs torch-op arm {psnr:.1f} dB; vs fused blocks with SDPA {psnr_c:.1f} dB")
    assert psnr > 48.0 and psnr_c > 48.0  # measured 53.5 dB both


@pytest.mark.parametrize("grid,t_txt", [(16, 128), ((13, 20), 77)], ids=["aligned", "padded"])
def test_adapter_with_controlnet_residuals(grid, t_txt):
    """order behind the joint block: the query from the block's output, the ControlNet add, then the adapter's add"""
    model, layers = _small()
    sd, emb = _adapter(model, 20, 0.7)
    lat, enc, pooled, img_ids, txt_ids = synthetic_inputs(grid, t_txt, 128, 64, seed=11)
    g = torch.Generator().manual_seed(3)
    c_joint, c_single = r16(torch.randn(lat.shape[0], 256, generator=g) * 0.5), r16(torch.randn(lat.shape[0], 256, generator=g) * 0.5)
    args = _args(lat, enc, pooled, img_ids, txt_ids, t=0.5)
    cuda = lambda x: x.cuda().bfloat16()[None]
    with torch.no_grad():
        got = model.engine_forward(*args, controlnet_block_samples=[cuda(c_joint)], controlnet_single_block_samples=[cuda(c_single)],
                                   ip_hidden_states=emb.cuda().bfloat16())[0].float().cpu()
        ref = IPARef(model, layers, sd, emb, 0.7).forward(lat, enc, pooled, torch.tensor([0.5]), img_ids, txt_ids, torch.tensor([3.5]),
                                                          control=c_joint, control_single=c_single)
    psnr, rel = psnr_rel(got, ref)
    print(f"adapter + controlnet {grid}+{t_txt}: PSNR {psnr:.1f} dB, relative L2 {rel:.3e}")
    assert psnr > 50.0 and rel < 1.5e-2  # measured 57.2 dB aligned, 55.8 dB padded


def test_adapter_with_first_block_cache():
    from nunchaku.caching import fbcache
    from nunchaku.caching.diffusers_adapters.flux_v2 import apply_cache_on_transformer
    from nunchaku_amd import mode

    with torch.no_grad(), mode.deterministic_mode("strict"):
        model, _ = _small(num_layers=2, num_single_layers=1)
        _, emb = _adapter(model, 20, 0.7)
        model.ip_adapter.set_ip_hidden_states(emb.cuda().bfloat16())
        a = _args(*synthetic_inputs((13, 20), 77, 128, 64, seed=5))
        b = _args(*synthetic_inputs((13, 20), 77, 128, 64, seed=6))
        ref_a, n_full = _count_ip_attention(lambda: model(*a))
        ref_b = model(*b)
        assert n_full == 2  # exactly one launch per joint block per step
        apply_cache_on_transformer(model, residual_diff_threshold=0.0)
        with fbcache.cache_context(fbcache.create_cache_context()):  # threshold 0: every step a miss
            for x, ref in ((a, ref_a), (b, ref_b), (b, ref_b), (a, ref_a)):
                out, n = _count_ip_attention(lambda: model(*x))
                assert n == 2 and torch.equal(out, ref), "a miss step must equal the uncached forward with the adapter bit for bit"
        apply_cache_on_transformer(model, residual_diff_threshold=1e6)
        with fbcache.cache_context(fbcache.create_cache_context()):
            out, n = _count_ip_attention(lambda: model(*a))
            assert n == 2 and torch.equal(out, ref_a)  # nothing stored yet: a miss
            hit, n = _count_ip_attention(lambda: model(*b))
            # a hit: block 0 and its adapter step ran (the decision compares their result), nothing behind them did
            assert n == 1 and torch.isfinite(hit.float()).all() and not torch.equal(hit, ref_b)
        # without the adapter the cached model is the plain model again
        from nunchaku.models.ip_adapter.utils import undo_all_mods_on_transformer

        undo_all_mods_on_transformer(model)
        apply_cache_on_transformer(model, residual_diff_threshold=-1.0)
        plain, n = _count_ip_attention(lambda: model(*a))
        assert n == 0 and not torch.equal(plain, ref_a)


def test_batch_of_two_equals_the_samples_run_singly():
    model, _ = _small()
    _, emb = _adapter(model, 4, 1.0)
    emb2 = torch.cat([emb, r16(torch.randn(1, 4, CROSS, generator=torch.Generator().manual_seed(5)))]).cuda().bfloat16()  # [2, 4, CROSS]
    a = _args(*synthetic_inputs(16, 128, 128, 64, seed=31))
    b = _args(*synthetic_inputs(16, 128, 128, 64, seed=32), t=0.3)
    both = tuple(torch.cat([x, y]) if i in (0, 1, 2, 3, 6) else x for i, (x, y) in enumerate(zip(a, b)))
    from nunchaku_amd import mode

    with torch.no_grad(), mode.deterministic_mode("strict"):  # (bit-equality across launches: the low-rank accumulators without fp32 atomics)
        out, n = _count_ip_attention(lambda: model.engine_forward(*both, ip_hidden_states=[emb2]))
        one = model.engine_forward(*a, ip_hidden_states=emb2[0:1])
        two = model.engine_forward(*b, ip_hidden_states=emb2[1:2])
        shared = model.engine_forward(*both, ip_hidden_states=emb2[0])  # no batch axis: every sample sees the same image prompt
    assert n == 2 and out.shape[0] == 2
    assert torch.equal(out[0], one[0]) and torch.equal(out[1], two[0])
    assert torch.equal(shared[0], one[0]) and not torch.equal(shared[1], two[0])
