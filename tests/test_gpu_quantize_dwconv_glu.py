"""svdq_quantize_dwconv_glu on the GPU against tests/dwconv_glu_ref.py (bit for bit), and against the two launches it replaces."""

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests.dwconv_glu_ref import quantize_dwconv_glu
from tests.glu_halves_ref import act64, rounding_margin
from tests.helpers import f32, t16

pytestmark = pytest.mark.gpu

# (B, H, W, K, C, R, smooth, bias, row-stride padding)
CASES = [
    (3, 1, 1, 128, 256, 16, True, True, 0),      # every tap but the centre outside the image; one chunk holds three samples
    (2, 5, 7, 128, 128, 32, False, True, 0),     # T = 35: a chunk wraps grid rows and straddles the samples; a whole group of absent channels
    (1, 3, 40, 384, 768, 0, True, False, 8),     # a chunk inside one grid row, chunks across row ends; 3 chunks on 4 waves; no bias, no low rank, strided
    (1, 9, 32, 640, 1280, 80, True, True, 0),    # M = 288: a partial second 256-row tile; 2 K slices (atomics, the clearing kernel); 3 rank slabs
    (2, 2, 2, 1152, 2176, 32, True, True, 0),    # 3 K slices; C = 2K - 128 at a sliced width
]


def _inputs(case, dtype, gates):
    """x [B, H, W, C] (a view with the case's row stride), weight, bias, smooth, down.  gates "exact": positive gate inputs and taps, a bias that puts
    every gate at >= 18 (silu(g) == g in fp32 and in float64 alike); "real": identity gate taps, designed gates in [-3, 6]; "random": everything random"""
    B, H, W, K, C, R, smoothed, biased, pad = case
    rng = np.random.default_rng(B * 1000 + W + K + R)
    r16 = lambda a: O.round16(np.asarray(a, np.float32), dtype)
    x = r16(rng.standard_normal((B, H, W, C)))
    w = r16(rng.standard_normal((C, 3, 3, 1)) / 3)
    b = r16(rng.standard_normal(C))
    kept = 1.0
    if gates == "exact":  # corner pixels see 4 taps of >= 2 * 3 (case 3 has no bias); the single pixel of case 1 one tap and the bias
        x[..., 1::2] = r16(rng.uniform(3.0, 4.0, (B, H, W, C // 2)))
        w[1::2] = r16(rng.uniform(2.0, 3.0, (C // 2, 3, 3, 1)))
        b[1::2] = r16(rng.uniform(20.0, 24.0, C // 2))
    elif gates == "real":
        g = r16(rng.uniform(-3.0, 6.0, (B, H, W, C // 2)))
        a = act64(g, "silu")  # a gate is kept where the exact activation lies farther from a rounding boundary than glu_silu's stated error
        keep = rounding_margin(g, dtype, "silu") > 32 * 2.0 ** -24 * np.maximum(np.abs(a), np.abs(g))
        kept = keep.mean()
        x[..., 1::2] = np.where(keep, g, 0.0)
        w[1::2], b[1::2] = 0.0, 0.0
        w[1::2, 1, 1, 0] = 1.0
    smooth = (2.0 ** rng.integers(-2, 3, K)).astype(np.float32) if smoothed else None  # powers of two: x * rcp(smooth) is the IEEE quotient
    down = r16(rng.standard_normal((K, R)) * 0.05) if R else None
    buf = t16(np.concatenate([x, np.full((B, H, W, pad), 3.0, np.float32)], axis=-1), dtype)
    return buf[..., :C], t16(w, dtype), t16(b, dtype) if biased else None, smooth, down, kept


def _params(smooth, down, dtype):  # checkpoint layout, as a state dict holds them
    return dict(smooth=None if smooth is None else t16(O.pack_vec_ref(smooth), dtype),
                lora_down=None if down is None else t16(O.pack_lowrank_ref(np.ascontiguousarray(down.T), down=True), dtype))


def _run(x, w, b, smooth, down, K, dtype):
    from nunchaku_amd import layout
    from nunchaku_amd.mode import lora_act_to_float
    from nunchaku_amd.ops import svdq_quantize_dwconv_glu as op
    qx, asc, la = op(x, w, b, quantized_features=K, **_params(smooth, down, dtype))
    return layout.unpack_act(qx, K).cpu().numpy(), f32(layout.unpack_scales(asc, qx.shape[0])), la, lora_act_to_float(la).cpu().numpy()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("gates", ["exact", "real"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:6])))
def test_bit_for_bit(case, gates, dtype):
    from nunchaku_amd.mode import deterministic_mode
    K, R = case[3], case[5]
    x, w, b, smooth, down, kept = _inputs(case, dtype, gates)
    print(f"kept {kept:.4f}")
    assert kept >= 0.90
    (q_ref, s_ref, la_ref), prod = quantize_dwconv_glu(x, w, b, smooth, down, K, dtype)
    codes, scales, _, la = _run(x, w, b, smooth, down, K, dtype)
    assert np.array_equal(codes, q_ref) and np.array_equal(scales, s_ref)
    if R and gates == "exact":
        xa = np.concatenate([np.abs(prod), np.zeros((q_ref.shape[0] - prod.shape[0], K), np.float32)])
        bound = 2e-5 * (xa @ np.abs(down)) + 1e-6  # the existing quantiser tests' bound (tests/test_gpu_parity.py)
        assert np.all(np.abs(la - la_ref) <= bound), f"lora_act: worst err / bound = {(np.abs(la - la_ref) / bound).max():.2f}"
        with deterministic_mode(True):  # Q31.32: integer atomics, bit-equal from run to run
            one, two = (_run(x, w, b, smooth, down, K, dtype)[2] for _ in range(2))
        assert one.dtype == torch.int64 and torch.equal(one, two) and np.all(np.abs(f32(one.double() * 2.0 ** -32) - la_ref) <= bound + 2.0 ** -30)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", [CASES[1], CASES[3]], ids=lambda c: "x".join(map(str, c[:6])))
def test_equal_to_the_two_launches_it_replaces(case, dtype):
    from nunchaku_amd.mode import lora_act_to_float
    from nunchaku_amd.ops import dwconv3x3, svdq_quantize_dwconv_glu
    from nunchaku_amd.ops.quantize import svdq_quantize_w4a4_act_fuse_lora_cuda
    B, H, W, K, C, R = case[:6]
    x, w, b, smooth, down, _ = _inputs(case, dtype, "random")
    kw = _params(smooth, down, dtype)
    wide = torch.zeros(B, H * W, 2 * K, dtype=x.dtype, device="cuda")
    dwconv3x3(x, w, b, out=wide[..., :C])
    q2, s2, la2 = svdq_quantize_w4a4_act_fuse_lora_cuda(wide.view(B * H * W, 2 * K), fuse_glu=True, **kw)
    q1, s1, la1 = svdq_quantize_dwconv_glu(x, w, b, quantized_features=K, **kw)
    assert torch.equal(q1, q2) and torch.equal(s1, s2)  # the same SiLU expression (quantize.hip's GLU front end)
    prod = quantize_dwconv_glu(x, w, b, smooth, down, K, dtype)[1]
    bound = 2e-5 * (np.abs(prod) @ np.abs(down)) + 1e-6
    diff = np.abs(f32(lora_act_to_float(la1)) - f32(lora_act_to_float(la2)))
    assert np.all(diff[: prod.shape[0]] <= bound) and not diff[prod.shape[0]:].any()
