"""svdq_quantize_dwconv_glu: what the library refuses before it launches (no GPU: nothing here reaches a launch)."""

import ctypes as C

import pytest

from nunchaku_amd import _lib

P = 1 << 20


def _args(**kw):
    a = _lib.ARGS["svdq_quantize_dwconv_glu_args"]()
    a.x, a.weight, a.bias, a.smooth, a.lora_down, a.act, a.ascales, a.lora_act = P, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P, 7 * P, 8 * P
    a.B, a.H, a.W, a.C, a.ldx, a.x_bs = 2, 5, 7, 640, 648, 35 * 648
    a.M_pad, a.K, a.R = 256, 384, 32
    a.dtype = 7  # an unknown dtype: the last thing validation looks at here, so "admitted" never launches
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _refusal(a):
    rc = _lib.load().svdq_quantize_dwconv_glu(C.byref(a), None)
    return rc, _lib.load().svdq_last_error().decode()


@pytest.mark.parametrize("field,value,text", [
    ("x", P + 8, "16-byte aligned"), ("bias", 3 * P + 2, "16-byte aligned"), ("C", 644, "multiple of 8"), ("C", 776, "at most 2K"), ("K", 320, "multiple of 128"),
    ("R", 8, "multiple of 16"), ("R", 272, "multiple of 16"), ("ldx", 632, ">= C"), ("ldx", 652, "multiple of 8"), ("x_bs", 35 * 648 - 8, "at least H * W * ldx"),
    ("M_pad", 128, "M_pad"), ("B", 8, "M_pad"), ("W", 0, ">= 1"),
])
def test_refused_before_launch(built_lib, field, value, text):
    rc, msg = _refusal(_args(**{field: value}))
    assert rc == 1 and text in msg, msg
    with pytest.raises(ValueError):
        _lib.check(rc, "quantize_dwconv_glu")


def test_the_reach(built_lib):
    """the strides are unbounded (64-bit pixel addresses); lora_down's byte offsets are 32-bit"""
    for kw in (dict(), dict(ldx=2 ** 31 - 8, x_bs=2 ** 62), dict(x=P + 16), dict(C=768, ldx=768, x_bs=35 * 768), dict(bias=None, smooth=None)):
        rc, msg = _refusal(_args(**kw))
        assert rc == 1 and "unknown dtype" in msg, msg  # everything else was admitted
    K = 128 * 32768  # R * K * 2 = 2^31 at R = 256
    rc, msg = _refusal(_args(K=K, R=256, dtype=0))
    assert rc == 2 and "lora_down" in msg, msg
