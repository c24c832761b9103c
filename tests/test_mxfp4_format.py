"""The MXFP4 format of DESIGN.md section 6v on the host: quantize_weight_mxfp4 / dequantize_mxfp4 against a float64 numpy restatement on
constructed blocks, bit for bit, and the module surface of SVDQW4A4Linear(precision="mxfp4").  No GPU."""

import numpy as np
import pytest
import torch

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float64)


def constructed_blocks(dtype: str) -> torch.Tensor:
    """[blocks, 32] 16-bit: every tie in both signs (amax 5: X = 0) | amax a power of two | just below | just above | all zero | subnormals |
    a value above 6 * 2^X | NaN and +-inf | values at the dtype's maximum"""
    fi = torch.finfo(DT[dtype])
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    sub = [k * fi.smallest_normal / 8 for k in (0, 1, 2, 3, -4, 5, -6, 7)]
    rows = [ties + [-t for t in ties], [8.0, 1.0, -3.0, 0.75], [7.96875, 1.0, -3.0, 5.0], [8.0625, 1.0, -3.0, 5.0], [], sub, [7.5, 6.5, -7.0, 1.0],
            [float("nan"), float("inf"), float("-inf"), 1.0, fi.max / 2], [fi.max, -fi.max / 2, fi.max / 4, fi.max / 16]]
    return torch.tensor([r + [0.0] * (32 - len(r)) for r in rows], dtype=torch.float64).to(DT[dtype])


def mxfp4_ref(v: np.ndarray, top: float):
    """the rule restated: v float64 [rows, K] -> (codes uint8 [rows, K] one a byte, scale bytes uint8 [rows, K/32])"""
    b = v.reshape(v.shape[0], -1, 32)
    mag = np.where(np.isnan(b), 0.0, np.minimum(np.abs(b), top))
    amax = mag.max(-1)
    byte = np.where(amax > 0, np.clip(np.floor(np.log2(np.where(amax > 0, amax, 1.0))) - 2 + 127, 0, 254), 0).astype(np.int64)
    y = b * 2.0 ** (127.0 - byte)[..., None]
    ay = np.where(np.isnan(y), 0.0, np.minimum(np.abs(y), 6.0))
    e = np.floor(np.log2(np.maximum(ay, 1.0)))
    c = np.where(ay < 1, np.rint(ay * 2), 2 + 2 * e + np.rint((ay / 2.0 ** e - 1) * 2)).astype(np.int64)  # np.rint: ties to even
    c = np.where((y < 0) & (c > 0), c | 8, c)
    return c.reshape(v.shape).astype(np.uint8), byte.astype(np.uint8)


def nibbles(codes: torch.Tensor) -> np.ndarray:
    c = codes.cpu().view(torch.uint8).numpy()
    return np.stack((c & 15, c >> 4), -1).reshape(c.shape[0], -1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_encoder_matches_the_rule_bit_for_bit(dtype):
    from nunchaku_amd.quantization.mxfp4 import dequantize_mxfp4, quantize_weight_mxfp4

    blocks = constructed_blocks(dtype)
    w = torch.cat([blocks.reshape(1, -1), torch.randn(3, blocks.numel(), generator=torch.Generator().manual_seed(1)).to(DT[dtype])])
    codes, scales = quantize_weight_mxfp4(w)
    ref_c, ref_s = mxfp4_ref(w.double().numpy(), float(torch.finfo(DT[dtype]).max))
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and tuple(scales.shape) == (w.shape[1] // 32, 4)
    assert np.array_equal(nibbles(codes), ref_c) and np.array_equal(scales.numpy().T, ref_s) and ref_s.max() < 255
    ties = nibbles(codes)[0, :14] & 7  # 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4, in both signs
    assert np.array_equal(E2M1[ties], np.array([0, 1, 1, 2, 2, 4, 4] * 2)) and np.array_equal(nibbles(codes)[0, 7:14] >> 3, [0] + [1] * 6)
    sign = np.where(ref_c & 8, -1.0, 1.0)
    assert np.array_equal(dequantize_mxfp4(codes, scales).numpy(), sign * E2M1[ref_c & 7] * np.repeat(2.0 ** (ref_s.astype(np.float64) - 127), 32, axis=1))


def test_module_surface():
    from nunchaku_amd.models.linear import SVDQW4A4Linear

    m = SVDQW4A4Linear(128, 128, precision="mxfp4")
    assert m.group_size == 32 and m.wscales.dtype == torch.uint8 and m.qweight.shape == (128, 64)
    with torch.no_grad():
        for t in m.state_dict().values():
            t.copy_(torch.randint(0, 100, t.shape).to(t.dtype))
    sd = m.state_dict()
    assert sd["wscales"].dtype == torch.uint8 and tuple(sd["wscales"].shape) == (4, 128)
    m2 = SVDQW4A4Linear(128, 128, precision="mxfp4")
    m2.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in sd.items())
    with pytest.raises(ValueError, match="act_unsigned"):
        SVDQW4A4Linear(128, 128, precision="mxfp4", act_unsigned=True)
    with pytest.raises(NotImplementedError):
        SVDQW4A4Linear(128, 128, precision="nvfp4")
    with pytest.raises(ValueError, match="Invalid precision"):
        SVDQW4A4Linear(128, 128, precision="fp8")
