"""``ops.t5_residual_norm`` (svdq_t5_residual_norm) on the GPU: the 16-bit add bit for bit, T5LayerNorm's torch sequence bit for bit on the
kernel's own ``rstd``, and that ``rstd`` against float64."""
import pytest
import torch

from tests import zimage_ref as Z

pytestmark = pytest.mark.gpu
EPS = 1e-6


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("use_weight", [False, True], ids=["noweight", "weight"])
@pytest.mark.parametrize("use_a", [False, True], ids=["noa", "a"])
@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("C", [256, 4096])
def test_add_norm_and_rstd(C, M, use_a, use_weight, dtype):
    from nunchaku_amd.ops import t5_residual_norm

    dt, g = Z.TD[dtype], torch.Generator(device="cuda").manual_seed(C + M)
    rand = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    wide = (rand(M, C + 24) * 3).to(dt)
    res, a, w = wide[:, 8:8 + C], rand(M, C).to(dt) if use_a else None, (1 + 0.1 * rand(C)).to(dt) if use_weight else None
    out, out_norm, rstd = t5_residual_norm(res, a, w, EPS, want_stats=True)
    y = res + a if use_a else res
    assert (out is None) == (not use_a) and (out_norm is None) == (not use_weight)
    if use_a:
        assert torch.equal(out, y)
    if use_weight:  # T5LayerNorm.forward behind its variance, on the kernel's rstd
        assert torch.equal(out_norm, w * (y * rstd[:, None]).to(dt))
    want = Z.rstd64(y, EPS)[:, 0]
    rel = ((rstd.double() - want).abs() / want).max().item()
    assert rel <= (8 * -(-C // 512) + 12) * 2.0 ** -24, rel
