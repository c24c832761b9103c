"""svdq_quantize_glu_halves on the GPU against tests/glu_halves_ref.py: bit for bit from the 16-bit rounding of the activation on."""

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests.glu_halves_ref import act64, glu_halves, quantize_glu_halves, rounding_margin
from tests.helpers import f32, t16

pytestmark = pytest.mark.gpu


def _run(value, gate, smooth, down, dtype, act, tail=8):  # the op on the two halves of one [M, 2K + tail] buffer; codes, scales, lora_act as numpy
    from nunchaku_amd import layout
    from nunchaku_amd.mode import lora_act_to_float
    from nunchaku_amd.ops import svdq_quantize_glu_halves as op
    M, K = value.shape
    buf = t16(np.concatenate([value, gate, np.full((M, tail), 3.0, np.float32)], axis=1), dtype)
    qx, asc, la = op(buf[:, :2 * K], act=act, smooth=None if smooth is None else t16(O.pack_vec_ref(smooth), dtype),  # (checkpoint layout, as a state dict)
                     lora_down=None if down is None else t16(O.pack_lowrank_ref(np.ascontiguousarray(down.T), down=True), dtype))
    return layout.unpack_act(qx, K).cpu().numpy(), f32(layout.unpack_scales(asc, qx.shape[0])), la, lora_act_to_float(la).cpu().numpy()


# one row | a partial second row tile, 3 chunks on 4 waves | a third 256-row pad tile, 5 chunks = 2 K slices (atomics, the clearing kernel) | 3 slices
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("act", ["silu", "gelu"])
@pytest.mark.parametrize("M,K,R,smoothed", [(1, 128, 16, True), (33, 384, 32, False), (257, 640, 80, True), (33, 384, 0, True), (40, 1152, 32, True)])
def test_bit_for_bit_from_the_rounding_on(dtype, act, M, K, R, smoothed):
    from nunchaku_amd.mode import deterministic_mode
    rng = np.random.default_rng(M + K + R)
    gate = O.round16(rng.uniform(-3.0, 6.0, (M, K)).astype(np.float32), dtype)
    # a gate is kept where the exact activation lies farther from a rounding boundary than the kernel's stated error
    a = act64(gate, act)
    keep = rounding_margin(gate, dtype, act) > 32 * 2.0 ** -24 * np.maximum(np.abs(a), np.abs(gate))
    print(f"kept {keep.mean():.4f}")
    assert keep.mean() >= 0.90
    gate = np.where(keep, gate, 0.0).astype(np.float32)
    value = O.round16(rng.standard_normal((M, K)).astype(np.float32) * 1.5, dtype)
    # powers of two: x * rcp(smooth) is then the IEEE quotient the oracle forms (other factors differ on 2^-15 .. 2^-12 of the elements)
    smooth = (2.0 ** rng.integers(-2, 3, K)).astype(np.float32) if smoothed else None
    down = O.round16(rng.standard_normal((K, R)).astype(np.float32) * 0.05, dtype) if R else None
    q_ref, s_ref, la_ref = quantize_glu_halves(value, gate, smooth, down, dtype, act)
    codes, scales, _, la = _run(value, gate, smooth, down, dtype, act)
    assert np.array_equal(codes, q_ref) and np.array_equal(scales, s_ref)
    if R:
        x = np.concatenate([glu_halves(value, gate, dtype, act), np.zeros((q_ref.shape[0] - M, K), np.float32)])
        bound = 2e-5 * (np.abs(x) @ np.abs(down)) + 1e-6  # the existing quantiser tests' bound (tests/test_gpu_parity.py)
        assert np.all(np.abs(la - la_ref) <= bound), f"lora_act: worst err / bound = {(np.abs(la - la_ref) / bound).max():.2f}"
        with deterministic_mode(True):  # Q31.32: integer atomics, bit-equal from run to run
            one, two = (_run(value, gate, smooth, down, dtype, act)[2] for _ in range(2))
        assert one.dtype == torch.int64 and torch.equal(one, two) and np.all(np.abs(f32(one.double() * 2.0 ** -32) - la_ref) <= bound + 2.0 ** -30)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("act", ["silu", "gelu"])
def test_every_finite_16_bit_gate(dtype, act):
    """one gate pattern per (row, 64-group), value 1, the other 63 gates 0: the group's scale is round16(|a| / 7) and its one code +-7"""
    bits = np.arange(65536, dtype=np.uint16)
    g = O.from_bits16(bits, dtype)
    bits = bits[np.isfinite(g)]
    n = -(-bits.size // 512) * 512
    gate = np.zeros((n // 2, 128), np.float32)
    gate.reshape(-1, 64)[: bits.size, 0] = O.from_bits16(bits, dtype)
    codes, scales, _, _ = _run(np.ones_like(gate), gate, None, None, dtype, act, tail=0)
    g64 = gate.reshape(-1, 64)[: bits.size, 0]
    with np.errstate(over="ignore", invalid="ignore"):
        a = O.round16(act64(g64, act).astype(np.float32), dtype)
        ab = O.to_bits16(a, dtype).astype(np.int64)
        near = [O.from_bits16(np.clip(ab + d, 0, 0xFFFF).astype(np.uint16), dtype) for d in (0, 1, -1)]
        want = [O.round16(np.abs(v) * np.float32(1.0 / 7.0), dtype) for v in near]
    got = scales.T.reshape(-1)[: bits.size]  # [K/64, M_pad] -> (row, group)
    ok = (got == want[0]) | (got == want[1]) | (got == want[2])
    assert ok.all(), f"{(~ok).sum()} scales off, first gates {g64[~ok][:8]}: got {got[~ok][:8]}, want {want[0][~ok][:8]}"
    code = codes[: n // 2].reshape(-1, 64)[: bits.size, 0]
    nz = a != 0
    normal = np.abs(a) * np.float32(1.0 / 7.0) >= 2.0 ** -126  # (where the fp32 scale is a normal number, as for the other quantisers: quantize.hip)
    assert np.array_equal(np.sign(code[nz]), np.sign(a[nz])) and np.all(np.abs(code[normal]) == 7)
