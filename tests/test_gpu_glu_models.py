"""The fused_glu path of Z-Image's and SDXL's feed-forward: equal to the hand composition, no farther from float64 than the unfused path."""

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests.glu_halves_ref import act64
from tests.helpers import TORCH_DT, f32, reference_state_dict, t16

pytestmark = pytest.mark.gpu



def _feed_forward(model, dtype):
    """(ff, act, the oracle layer of net[2]) with random quantised weights"""
    from nunchaku_amd.models import sdxl, zimage
    kw = dict(rank=32, torch_dtype=TORCH_DT[dtype], device="cuda")
    if model == "zimage":
        ff, act, dim, hidden = zimage.NunchakuZImageFeedForward(256, 384, **kw), "silu", 256, 384
    else:
        ff, act, dim, hidden = sdxl.NunchakuSDXLFeedForward(128, **kw), "gelu", 128, 512
    L1 = O.make_svdq_layer(dim, 2 * hidden, 32, seed=1, dtype=dtype, cheap=True, bias=model == "sdxl")
    L2 = O.make_svdq_layer(hidden, dim, 32, seed=2, dtype=dtype, cheap=True, bias=model == "sdxl")
    ff.net[0].proj.load_state_dict(reference_state_dict(L1, dtype))
    ff.net[2].load_state_dict(reference_state_dict(L2, dtype))
    return ff.eval(), act, L2


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("model", ["zimage", "sdxl"])
def test_fused_feed_forward(model, dtype):
    from nunchaku_amd.ops import svdq_quantize_glu_halves
    ff, act, L2 = _feed_forward(model, dtype)
    dim = ff.net[2].out_features
    x = t16(np.random.default_rng(0).standard_normal((1, 77, dim)).astype(np.float32), dtype)
    with torch.no_grad():
        plain = ff(x)
        h, g = ff.net[0].proj(x).chunk(2, dim=-1)
        today = ff.net[2](h * (torch.nn.functional.silu(g) if act == "silu" else torch.nn.functional.gelu(g)))
        assert torch.equal(plain, today)  # the flag is off: today's path
        ff.fused_glu = True
        fused = ff(x)
        y = ff.net[0].proj(x)[0]
        hand = ff.net[2].forward_quant(*svdq_quantize_glu_halves(y, lora_down=ff.net[2].proj_down, smooth=ff.net[2].smooth_factor, act=act))[:77]
    assert torch.equal(fused[0], hand)
    # float64 evaluation of the same quantised layer on the exact gated product of the same 16-bit projection output
    v64, g16 = f32(y)[:, : y.shape[1] // 2].astype(np.float64), f32(y)[:, y.shape[1] // 2:]
    hx = v64 * act64(g16, act)
    W = (L2["qweight"].astype(np.float64).reshape(dim, -1, 64) * L2["wscales"].T.astype(np.float64)[:, :, None]).reshape(dim, -1)
    ref = (hx / L2["smooth"].astype(np.float64)) @ W.T + (hx @ L2["proj_down"].astype(np.float64)) @ L2["proj_up"].astype(np.float64).T
    ref = ref + (0.0 if L2.get("bias") is None else L2["bias"].astype(np.float64))
    dist = lambda t: float(np.sqrt(np.mean((f32(t)[0].astype(np.float64) - ref) ** 2)))
    print(f"{model} {dtype}: rms distance from float64 fused {dist(fused):.6g} unfused {dist(plain):.6g} ratio {dist(fused) / dist(plain):.4f}")
    assert dist(fused) <= 1.5 * dist(plain)


def test_set_fused_glu_reaches_every_block():
    from nunchaku_amd.models import sdxl, zimage
    for cls, ffc, args in ((zimage.NunchakuZImageTransformer2DModel, zimage.NunchakuZImageFeedForward, (256, 384)),
                           (sdxl.NunchakuSDXLUNet2DConditionModel, sdxl.NunchakuSDXLFeedForward, (128,))):
        model = torch.nn.Module()
        model.blocks = torch.nn.ModuleList([torch.nn.Sequential(ffc(*args, device="cuda")) for _ in range(3)])
        assert cls.set_fused_glu(model, True) is model and all(m.fused_glu for m in model.modules() if isinstance(m, ffc))
        cls.set_fused_glu(model, False)
        assert not any(m.fused_glu for m in model.modules() if isinstance(m, ffc)) and ffc.fused_glu is False
