"""The fused_conv path of SANA's feed-forward: off it is today's path, on it equals the hand composition and is no farther from float64."""

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests.dwconv_ref import dwconv_ref64
from tests.glu_halves_ref import act64
from tests.helpers import TORCH_DT, f32, reference_state_dict, t16

pytestmark = pytest.mark.gpu
B, H, W = 2, 5, 7


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("features,hidden", [(128, 160), (256, 256)])  # C_gemm 384 against 2 * hid_pad 512 | equal widths
def test_fused_feed_forward(features, hidden, dtype):
    from nunchaku_amd.mode import deterministic_mode
    from nunchaku_amd.models.sana import SanaGLUMBConv
    from nunchaku_amd.ops import svdq_quantize_dwconv_glu
    m = SanaGLUMBConv(features, hidden, torch_dtype=TORCH_DT[dtype], device="cuda")
    cg, hp = m.c_gemm, m.hid_pad
    L1 = O.make_svdq_layer(m.in_pad, cg, 32, seed=1, dtype=dtype, cheap=True, bias=True)
    L2 = O.make_svdq_layer(hp, m.in_pad, 32, seed=2, dtype=dtype, cheap=True, bias=False)
    rng = np.random.default_rng(features)
    m.inverted_conv.load_state_dict(reference_state_dict(L1, dtype))
    m.point_conv.load_state_dict(reference_state_dict(L2, dtype))
    m.depth_conv.weight.copy_(t16(rng.standard_normal((cg, 3, 3, 1)) / 3, dtype))
    m.depth_conv.bias.copy_(t16(rng.standard_normal(cg), dtype))
    x = t16(rng.standard_normal((B, H * W, features)), dtype)
    pc = m.point_conv
    with torch.no_grad(), deterministic_mode(True):
        plain = m(x, H, W)
        wide = m.gated_input(x, H, W)
        today = pc.forward_quant(*pc.quantize(wide.view(B * H * W, -1), fuse_glu=True))[: B * H * W].view(B, H * W, -1)[..., :features]
        assert torch.equal(plain, today)  # the flag is off: today's path
        m.fused_conv = True
        fused = m(x, H, W)
        y = m.inverted_conv.forward_silu(x)
        hand = pc.forward_quant(*svdq_quantize_dwconv_glu(y, m.depth_conv.weight, m.depth_conv.bias, H, W, lora_down=pc.proj_down,
                                                          smooth=pc.smooth_factor, quantized_features=hp))
    assert torch.equal(fused.reshape(B * H * W, -1), hand[: B * H * W, :features])
    # float64 evaluation of the same quantised layer on the exact convolution and gated product of the same 16-bit GEMM output
    c = np.zeros((B * H * W, 2 * hp))
    c[:, :cg] = dwconv_ref64(y.view(B, H, W, cg), m.depth_conv.weight, m.depth_conv.bias).numpy().reshape(-1, cg)
    hx = c[:, 0::2] * act64(c[:, 1::2], "silu")
    Wq = (L2["qweight"].astype(np.float64).reshape(m.in_pad, -1, 64) * L2["wscales"].T.astype(np.float64)[:, :, None]).reshape(m.in_pad, -1)
    ref = (hx / L2["smooth"].astype(np.float64)) @ Wq.T + (hx @ L2["proj_down"].astype(np.float64)) @ L2["proj_up"].astype(np.float64).T
    dist = lambda t: float(np.sqrt(np.mean((f32(t).reshape(B * H * W, -1).astype(np.float64) - ref[:, :features]) ** 2)))
    print(f"{features} {dtype}: rms distance from float64 fused {dist(fused):.6g} unfused {dist(plain):.6g} ratio {dist(fused) / dist(plain):.4f}")
    assert dist(fused) <= 1.5 * dist(plain)


def test_set_fused_conv_reaches_every_block():
    from nunchaku_amd.models.sana import SanaGLUMBConv, SanaModel
    from nunchaku_amd.models.transformer_sana import NunchakuSanaTransformer2DModel
    for cls in (SanaModel, NunchakuSanaTransformer2DModel):
        model = torch.nn.Module()
        model.blocks = torch.nn.ModuleList([torch.nn.Sequential(SanaGLUMBConv(128, 160, device="cuda")) for _ in range(3)])
        assert cls.set_fused_conv(model, True) is model and all(m.fused_conv for m in model.modules() if isinstance(m, SanaGLUMBConv))
        cls.set_fused_conv(model, False)
        assert not any(m.fused_conv for m in model.modules() if isinstance(m, SanaGLUMBConv)) and SanaGLUMBConv.fused_conv is False
