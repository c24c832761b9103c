"""svdq_quantize_glu_halves: what the library refuses before it launches (no GPU: nothing here reaches a launch)."""

import ctypes as C

import pytest

from nunchaku_amd import _lib

P = 1 << 20


def _args(**kw):
    a = _lib.ARGS["svdq_quantize_glu_args"]()
    a.value, a.gate, a.smooth, a.lora_down, a.act, a.ascales, a.lora_act = P, P + 768, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P
    a.M, a.M_pad, a.K, a.R, a.ld_value, a.ld_gate = 200, 256, 384, 32, 776, 776
    a.dtype = 7  # an unknown dtype: the last thing validation looks at here, so "admitted" never launches
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refusal(a):
    rc = _lib.load().svdq_quantize_glu_halves(C.byref(a), None)
    return rc, _lib.load().svdq_last_error().decode()


@pytest.mark.parametrize("field,value,text", [
    ("value", P + 8, "16-byte aligned"), ("gate", P + 776, "16-byte aligned"), ("ld_gate", 772, "multiples of 8"), ("ld_value", 376, ">= K"),
    ("K", 320, "multiple of 128"), ("R", 8, "multiple of 16"), ("R", 272, "multiple of 16"), ("act_fn", 2, "unknown act_fn"), ("M_pad", 128, "M_pad"),
])
def test_refused_before_launch(built_lib, field, value, text):
    rc, msg = _refusal(_args(**{field: value}))
    assert rc == 1 and text in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc, "quantize_glu_halves")


def test_the_reach(built_lib):
    """strides are unbounded (64-bit row addresses); lora_down's byte offsets are 32-bit"""
    for kw in (dict(), dict(ld_value=2 ** 31 - 8, ld_gate=2 ** 31 - 8), dict(value=P + 16)):
        rc, msg = _refusal(_args(**kw))
        assert rc == 1 and "unknown dtype" in msg, msg  # everything else was admitted
    K = 128 * 32768  # R * K * 2 = 2^31 at R = 256
    rc, msg = _refusal(_args(K=K, R=256, ld_value=K, ld_gate=K, dtype=0))
    assert rc == 2 and "lora_down" in msg, msg
