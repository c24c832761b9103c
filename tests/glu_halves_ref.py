"""Float64 reference of ``ops.quantize.svdq_quantize_glu_halves``: the activation and the product in float64, rounded where the 16-bit torch
sequence rounds, then the oracle's quantiser."""

import math

import numpy as np

from oracle import svdq_oracle as O

_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def act64(gate: np.ndarray, act: str) -> np.ndarray:
    """silu / erf-gelu of 16-bit gates in float64 (gelu as g * erfc(-g / sqrt 2) / 2: the same function, without the cancellation of 1 + erf)"""
    g = gate.astype(np.float64)
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g)) if act == "silu" else 0.5 * g * _erfc(-g / math.sqrt(2.0))


def glu_halves(value: np.ndarray, gate: np.ndarray, dtype: str, act: str) -> np.ndarray:  # x = round16(value * round16(act(gate)))
    a = O.round16(act64(gate, act).astype(np.float32), dtype)
    return O.round16((value.astype(np.float64) * a.astype(np.float64)).astype(np.float32), dtype)


def rounding_margin(gate: np.ndarray, dtype: str, act: str) -> np.ndarray:
    """distance of act(gate) from the nearest 16-bit rounding boundary (the midpoint of two neighbours), in float64"""
    a = act64(gate, act)
    r = O.round16(a.astype(np.float32), dtype).astype(np.float64)
    bits = O.to_bits16(r.astype(np.float32), dtype).astype(np.int64)
    up, dn = (O.from_bits16(np.clip(bits + d, 0, 0xFFFF).astype(np.uint16), dtype).astype(np.float64) for d in (1, -1))
    return np.minimum(np.abs(a - 0.5 * (r + up)), np.abs(a - 0.5 * (r + dn)))


def quantize_glu_halves(value, gate, smooth, lora_down, dtype: str, act: str):  # -> codes [M_pad, K], ascales [K/64, M_pad], lora_act [M_pad, R] | None
    return O.quantize_w4a4_act_fuse_lora(glu_halves(value, gate, dtype, act), smooth, lora_down, dtype)
