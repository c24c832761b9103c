"""How far from a tensor's base every entry point can address, pinned on the host -- no GPU, nothing is launched.

Three layers, from the outside in:

* ``nunchaku_amd/_C.py`` hands strides and extents to 32-bit struct fields, and ctypes keeps the low 32 bits of whatever it is given.  Every such assignment
  goes through ``_i32`` (``_i64`` for the 64-bit head and batch strides), which raises instead: tested on the helper, on every wrapper that takes a strided
  view (stand-in tensors: the wrappers only read shapes and strides before they marshal; ``gemv_awq_batched`` and ``gemv_awq_lora_batched`` make their one
  row contiguous and have no stride to hand on) and by reading the module's syntax tree.
* A kernel that keeps part of its address arithmetic in 32 bits has a finite reach ("Addressing reach").  ``REACH`` lists every such
  field with the largest value the library admits; validation admits that value and refuses the next admissible one, or -- where another kernel serves the
  wider stride -- the plan query moves the launch there.  ``UNBOUNDED`` lists the fields whose addresses are formed in 64 bits throughout; together the two
  cover every ``ld*`` / ``*_hs`` / ``*_bs`` field of every args struct, so a new field fails here until someone reads its kernel and classifies it.
* ``svdq_quantize_plan`` around the fast quantiser's 2 GiB rule (its x is read through a buffer descriptor with 32-bit byte offsets).

The addresses in the args structs are made up: validation and the plan queries look at alignment and NULL, never at what a pointer points to."""
import ast
import ctypes as C
import inspect
import math
import re

import pytest
import torch

from nunchaku_amd import _lib
from tests import test_gpu_hot_instantiations as T
from tests.test_gemm_plan import CUS, WS_BASE, plan_args

I32_MAX = 2 ** 31 - 1
U32 = 2 ** 32 - 1  # the largest 32-bit byte offset


# ---- 1. the finite reaches ------------------------------------------------------------------------------------------------------------
def _attention_args(**kw):
    a = _lib.AttentionArgs()
    a.q = a.k = a.vt = a.out = 4096
    a.L, a.H, a.head_dim, a.ldq, a.ldk, a.ldo, a.ldvt = 256, 2, 128, 768, 768, 256, 256
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _attention_probe(lib, field, value):
    """validation alone: q is misaligned, the check behind the reach checks -- an admitted stride gets that refusal (SVDQ_E_INVALID, another message)"""
    rc = lib.svdq_attention(C.byref(_attention_args(q=4096 + 2, **{field: value})), None)
    msg = lib.svdq_last_error()
    return ("admitted" if rc == 1 and b"16-byte aligned" in msg else "refused" if rc == 2 else "other"), msg


def _gemm_ldvt_probe(lib, field, value):
    """the plan query validates exactly as the launch does"""
    a = plan_args(512, 768, 256, _lib.FUSE_RMSNORM_ROPE, 0, 32, 0, _lib.LORA_ACT_F32, WS_BASE, 0, 0, _lib.SVDQ_BF16, lib=lib)
    a.out_vt = 0x63000000
    setattr(a, field, value)
    out = (C.c_int32 * 8)()
    rc = lib.svdq_gemm_plan(C.byref(a), CUS, out)
    return ("admitted" if rc == 0 else "refused" if rc == 2 else "other"), lib.svdq_last_error()


def _gemm_ldo_probe(lib, field, value):
    """geometry 8 asks for the wave-tile kernel by name; beyond its reach the launch takes the 8-wave kernel (64-bit row addresses) instead: "moved" """
    assert field == "ldo"
    res = set()
    for R in (0, 32):
        a = plan_args(512, 512, 256, _lib.FUSE_NONE, 8, R, 0, _lib.LORA_ACT_F32, WS_BASE, 0, 0, _lib.SVDQ_BF16, lib=lib)
        a.ldo = value
        out = (C.c_int32 * 8)()
        assert lib.svdq_gemm_plan(C.byref(a), CUS, out) == 0, lib.svdq_last_error()
        res.add("admitted" if out[1] == 6 else "moved")  # variant 6: wave_tile_128
    assert len(res) == 1
    return res.pop(), b"ldo"


# (entry point, args struct, field, largest admitted value, step to the next admissible value, the 32-bit byte offset that limits it as a function of the
#  field -- it fits 32 bits at the limit and not one step beyond --, what lies beyond, probe)
REACH = (
    ("svdq_attention", _lib.AttentionArgs, "ldk", 33554424, 8, lambda ld: 128 * ld, "refused", _attention_probe),               # attention.hip: kstride
    ("svdq_attention", _lib.AttentionArgs, "ldvt", 16909312, 8, lambda ld: 254 * ld + 112, "refused", _attention_probe),        # attention.hip: voff / vdma
    ("svdq_gemm_w4a4", _lib.GemmArgs, "ldvt", 429496716, 2, lambda ld: 10 * ld + 124, "refused", _gemm_ldvt_probe),             # gemm_w4a4.hip: lane_off
    ("svdq_gemm_w4a4", _lib.GemmArgs, "ldo", 16909316, 4, lambda ld: 254 * ld + 16, "moved", _gemm_ldo_probe),                  # gemm_w4a4.hip: e_off + 3 row tiles
)
# The quantiser's ldx / ldx2 are bounded for the fast kernel only, by products (M_pad * ld * 2, R * K * 2 < 0x7fffffff): section 3 below.
# Fields every kernel multiplies in 64 bits ((size_t)row * ld, (long long)b * bs): limited by the field's own width alone.
UNBOUNDED = (
    ("QuantizeArgs", "ldx"), ("QuantizeArgs", "ldx2"),
    ("ResidualArgs", "ld"), ("ResidualDiffArgs", "ld"), ("ModulatedDiffArgs", "ld"),
    ("IpAttentionArgs", "ldq"), ("IpAttentionArgs", "ldk"), ("IpAttentionArgs", "ldv"), ("IpAttentionArgs", "ldo"),
    ("LinearAttentionArgs", "q_bs"), ("LinearAttentionArgs", "kv_bs"), ("LinearAttentionArgs", "out_bs"),
    ("LinearAttentionArgs", "ldq"), ("LinearAttentionArgs", "ldkv"), ("LinearAttentionArgs", "ldo"),
    ("Dwconv3x3Args", "x_bs"), ("Dwconv3x3Args", "out_bs"), ("Dwconv3x3Args", "ldx"), ("Dwconv3x3Args", "ldo"),
    ("AttentionArgs", "q_hs"), ("AttentionArgs", "k_hs"), ("AttentionArgs", "vt_hs"), ("AttentionArgs", "o_hs"), ("AttentionArgs", "ldq"), ("AttentionArgs", "ldo"),
    ("GemvAwqArgs", "ldx"), ("GemmAwqArgs", "ldx"),
    ("CrossAttentionArgs", "ldq"), ("CrossAttentionArgs", "ldk"), ("CrossAttentionArgs", "ldv"), ("CrossAttentionArgs", "ldo"),
    ("AttentionD64Args", "q_bs"), ("AttentionD64Args", "k_bs"), ("AttentionD64Args", "v_bs"), ("AttentionD64Args", "out_bs"),
    ("AttentionD64Args", "ldq"), ("AttentionD64Args", "ldk"), ("AttentionD64Args", "ldv"), ("AttentionD64Args", "ldo"),
    ("SanaGlueArgs", "timestep_bs"), ("SanaGlueArgs", "ld_res"), ("SanaGlueArgs", "ld_a"), ("SanaGlueArgs", "ld_out"), ("SanaGlueArgs", "ld_mod"),
    ("SandwichNormArgs", "gate_bs"), ("SandwichNormArgs", "scale_bs"),
    ("SandwichNormArgs", "ld_res"), ("SandwichNormArgs", "ld_a"), ("SandwichNormArgs", "ld_out"), ("SandwichNormArgs", "ld_mod"),
    ("QkNormRopeArgs", "ld"), ("QkNormRopeArgs", "ldvt"),
    ("PulidCaArgs", "ldx"), ("PulidCaArgs", "ldo"),
)
STRIDE_FIELD = re.compile(r"^(ld\w*|\w+_hs|\w+_bs)$")


def _structs():
    return {name: cls for name, cls in vars(_lib).items() if isinstance(cls, type) and issubclass(cls, C.Structure) and cls is not C.Structure}


@pytest.mark.parametrize("row", REACH, ids=lambda r: f"{r[0]}-{r[2]}")
def test_the_reach_is_admitted_and_the_next_value_is_not(built_lib, row):
    entry, cls, field, limit, step, offset, beyond, probe = row
    lib = _lib.load()
    # the table's own arithmetic: the limit is the last admissible value whose limiting byte offset fits 32 bits
    assert limit % step == 0 and offset(limit) <= U32 < offset(limit + step), (field, offset(limit), offset(limit + step))
    got, msg = probe(lib, field, limit)
    assert got == "admitted", (entry, field, limit, got, msg)
    got, msg = probe(lib, field, limit + step)
    assert got == beyond, (entry, field, limit + step, got, msg)
    if beyond == "refused":
        text = msg.decode()
        assert f"{field}={limit + step}" in text and str(limit) in text and entry in text, text
    # far beyond, up to the field's own width
    got, msg = probe(lib, field, (I32_MAX // step) * step)
    assert got == beyond, (entry, field, got, msg)


def test_every_stride_field_is_classified():
    """every ld* / *_hs / *_bs field of every args struct is in REACH or in UNBOUNDED, and neither names a field that does not exist"""
    have = {(name, f) for name, cls in _structs().items() for f, _ in cls._fields_ if STRIDE_FIELD.match(f)}
    bounded = {(cls.__name__, field) for _, cls, field, *_ in REACH}
    assert len(set(UNBOUNDED)) == len(UNBOUNDED) and not bounded & set(UNBOUNDED)
    assert not have - bounded - set(UNBOUNDED), f"unclassified stride fields (read the kernel, then add them to REACH or UNBOUNDED): {sorted(have - bounded - set(UNBOUNDED))}"
    assert not (bounded | set(UNBOUNDED)) - have, f"classified, but no such field: {sorted((bounded | set(UNBOUNDED)) - have)}"
    assert len(have) == 58


def test_the_header_states_a_reach_for_every_entry_point_with_a_stride():
    import os

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svdq_amd.h")).read()
    for entry in ("svdq_quantize_w4a4_act_fuse_lora", "svdq_gemm_w4a4", "svdq_attention", "svdq_residual_gate_stats", "svdq_residual_diff", "svdq_modulated_diff",
                  "svdq_ip_attention", "svdq_linear_attention", "svdq_dwconv3x3", "svdq_cross_attention", "svdq_attention_d64", "svdq_sana_glue",
                  "svdq_sandwich_norm", "svdq_qk_norm_rope", "svdq_pulid_ca", "svdq_gemv_awq", "svdq_gemm_awq"):
        m = re.search(r"/\* Addressing reach((?:(?!\*/).)*)\*/\s*int " + entry + r"\(", src, flags=re.S)
        assert m, f"{entry}: no 'Addressing reach' comment in front of its declaration"
    for _, _, field, limit, *_ in REACH:
        assert str(limit) in src, (field, limit)


# ---- 2. the Python wrappers: nothing reaches a 32-bit field unchecked -------------------------------------------------------------------
BAD_STRIDES = (2 ** 31, 2 ** 32 + 16)  # the first turns negative in a c_int32, the second becomes 16


def test_what_ctypes_does_without_the_helper():
    a = _lib.AttentionArgs()
    a.ldq = 2 ** 32 + 16
    assert a.ldq == 16
    a.ldq = 2 ** 31 + 8
    assert a.ldq < 0


def test_the_helpers():
    from nunchaku_amd import _C

    for v in (0, 1, -1, I32_MAX, -2 ** 31):
        assert _C._i32("op", "x.stride(0)", v) == v
    for v in BAD_STRIDES + (2 ** 31 + 8, -2 ** 31 - 1, 2 ** 63):
        with pytest.raises(ValueError, match=rf"op: x\.stride\(0\)={v} does not fit"):
            _C._i32("op", "x.stride(0)", v)
    for v in (0, 2 ** 32 + 16, 2 ** 63 - 1, -2 ** 63):
        assert _C._i64("op", "q batch stride", v) == v
    for v in (2 ** 63, -2 ** 63 - 1):
        with pytest.raises(ValueError, match=r"op: q batch stride=-?\d+ does not fit"):
            _C._i64("op", "q batch stride", v)


class _Stand:
    """What a wrapper reads of a tensor before it marshals: shape, strides, dtype, device kind, an address.  No storage: a view with a row stride of 2^32
    elements would need 8 GiB."""

    def __init__(self, shape, strides=None, dtype=torch.bfloat16):
        self.shape = torch.Size(shape)
        if strides is None:
            strides, n = [], 1
            for s in reversed(shape):
                strides.insert(0, n)
                n *= s
        self._strides, self.dtype, self.is_cuda, self.device = tuple(strides), dtype, True, torch.device("cpu")

    def dim(self):
        return len(self.shape)

    def stride(self, i=None):
        return self._strides if i is None else self._strides[i]

    def numel(self):
        return math.prod(self.shape)

    def element_size(self):
        return torch.empty((), dtype=self.dtype).element_size()

    def is_contiguous(self):
        return self._strides == _Stand(self.shape)._strides

    def data_ptr(self):
        return 1 << 20

    _svdq_amd = True  # (a weight-side stand-in is in the kernel layout: no conversion on use)

    def reshape(self, *shape):
        shape = tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else shape
        if -1 in shape:
            shape = tuple(self.numel() // -math.prod(shape) if s == -1 else s for s in shape)
        assert tuple(shape) == tuple(self.shape), "the stand-ins are only reshaped to the shape they have"
        return self

    def unsqueeze(self, i):
        assert i == 0
        return _Stand((1,) + tuple(self.shape), (self.numel(),) + self._strides, self.dtype)


def _no_side_paths(monkeypatch):
    """what a wrapper does besides marshalling and needs a device or a storage for: the GEMM's stream workspace, the cached tap image of the convolution's weight"""
    from nunchaku_amd import _C

    monkeypatch.setattr(_C._Ops, "gemm_use_workspace", False)
    monkeypatch.setattr(_C, "_cached_conversion", lambda t, kind, convert, table=None: t)


def _wrapper_calls(ld):
    """{name: call} -- every wrapper with a caller-visible stride, one call per tensor whose stride is `ld`"""
    from nunchaku_amd._C import ops

    S, f32 = _Stand, torch.float32
    row = lambda wide: S((4, 256), (ld if wide else 256, 1))
    calls = {
        "residual_gate_stats": lambda: ops.residual_gate_stats(row(1), row(1), None, None, row(1), None),
        "residual_gate_stats (meta tensors)": lambda: ops.residual_gate_stats(*(torch.empty_strided((4, 256), (ld, 1), dtype=torch.bfloat16, device="meta"),) * 2,
                                                                              None, None, None, None),
        "residual_diff": lambda: ops.residual_diff(row(1), row(1), None, row(1)),
        "modulated_diff": lambda: ops.modulated_diff(row(1), S((4, 2), dtype=f32), S((256,)), S((256,)), None, row(1)),
        "sana_glue": lambda: ops.sana_glue(row(0), None, None, None, None, row(0), None, None, 4, 256, 256, (256, 0, ld, 0)),
        "sandwich_norm": lambda: ops.sandwich_norm(row(0), row(0), S((256,)), None, None, None, row(0), None, None, 4, 256, (256, ld, 256, 0)),
        "qk_norm_rope qkv": lambda: ops.qk_norm_rope(S((128, 384), (ld, 1)), None, None, None, S((128, 128)), None, 128, 128, 1),
        "qk_norm_rope vt": lambda: ops.qk_norm_rope(S((128, 384)), None, None, None, S((128, 128), (ld, 1)), None, 128, 128, 1),
        "pulid_ca x": lambda: ops.pulid_ca(S((4, 128), (ld, 1)), S((4, 2), dtype=f32), S((32, 128)), S((32,), dtype=f32), S((32,), dtype=f32), S((32, 128)),
                                           S((4, 32)), S((4, 128)), 4),
        "pulid_ca out": lambda: ops.pulid_ca(S((4, 128)), S((4, 2), dtype=f32), S((32, 128)), S((32,), dtype=f32), S((32,), dtype=f32), S((32, 128)),
                                             S((4, 32)), S((4, 128), (ld, 1)), 4),
    }
    lhd = lambda wide, L=128, H=2, D=128: S((L, H, D), (ld if wide else H * D, D, 1))
    for i, name in enumerate(("q", "k", "out")):
        t = [lhd(i == j) for j in range(3)]
        calls[f"attention {name}"] = lambda t=t: ops.attention(t[0], t[1], S((2, 128, 128)), t[2], 1.0)
    calls["attention vt"] = lambda: ops.attention(lhd(0), lhd(0), S((2, 128, 128), (128 * 128, ld, 1)), lhd(0), 1.0)
    calls["attention head stride (64-bit)"] = lambda: ops.attention(S((128, 2, 128), (256, 2 ** 63, 1)), lhd(0), S((2, 128, 128)), lhd(0), 1.0)
    for i, name in enumerate(("q", "k", "v", "out")):
        kv = lambda wide: S((16, 256), (ld if wide else 256, 1))
        calls[f"ip_attention {name}"] = lambda i=i, kv=kv: ops.ip_attention(lhd(i == 0, 8), kv(i == 1), kv(i == 2), lhd(i == 3, 8), 1.0)
        b4 = lambda wide, rows, D: S((2, rows, 2, D), (rows * (ld if wide else 2 * D), ld if wide else 2 * D, D, 1))
        calls[f"attention_d64 {name}"] = lambda i=i, b4=b4: ops.attention_d64(b4(i == 0, 8, 64), b4(i == 1, 16, 64), b4(i == 2, 16, 64), b4(i == 3, 8, 64), 1.0)
        ck = lambda wide: S((32, 144), (ld if wide else 144, 1))
        ints = S((2,), dtype=torch.int32)
        calls[f"cross_attention {name}"] = lambda i=i, b4=b4, ck=ck, ints=ints: ops.cross_attention(b4(i == 0, 8, 72), ck(i == 1), ck(i == 2), b4(i == 3, 8, 72),
                                                                                                   ints, ints, 16, 1.0)
    M_pad, K = 256, 128
    codes = lambda k: S((M_pad, k * 3 // 4), dtype=torch.uint8)
    calls["quantize_w4a4_act_fuse_lora"] = lambda: ops.quantize_w4a4_act_fuse_lora(S((200, K), (ld, 1)), codes(K), S((K // 64, M_pad)), None, None, None)
    calls["quantize_w4a4_act_fuse_lora second"] = lambda: ops.quantize_w4a4_act_fuse_lora(S((256, K)), S((512, K * 3 // 4), dtype=torch.uint8), S((K // 64, 512)), None, None,
                                                                                        None, second=dict(input=S((44, K), (ld, 1))))
    N = 384
    calls["gemm_w4a4 out_vt"] = lambda: ops.gemm_w4a4(
        codes(K), S((N, K * 3 // 4), dtype=torch.uint8), S((M_pad, N)), None, S((K // 64, M_pad)), S((K // 64, N)), None, None, None, None, None, None,
        S((128,)), S((128,)), S((M_pad, 128), dtype=f32), None, None, None, None, False, None, False, False, None, None, None, None, None, 0,
        out_vt=S((N // 3, M_pad), (ld, 1)))
    calls["gemv_awq"] = lambda: ops.gemv_awq(S((8, 64), (ld, 1)), S((16, 32), dtype=torch.int32), S((1, 64)), S((1, 64)), 8, 64, 64, 64)
    calls["gemm_awq"] = lambda: ops.gemm_awq(S((40, 128), (ld, 1)), S((16, 128), dtype=torch.int16), S((1, 64)), S((1, 64)))
    px = lambda wide: S((1, 5, 7, 64), (35 * (ld if wide else 64), 7 * (ld if wide else 64), ld if wide else 64, 1))
    calls["dwconv3x3 x"] = lambda: ops.dwconv3x3(px(1), S((64, 3, 3, 1)), None, px(0))
    calls["dwconv3x3 out"] = lambda: ops.dwconv3x3(px(0), S((64, 3, 3, 1)), None, px(1))
    la = lambda wide, D: S((2, 8, 2, D), (8 * (ld if wide else 2 * D), ld if wide else 2 * D, D, 1))
    for i, name in enumerate(("q", "kv", "out")):
        calls[f"linear_attention {name}"] = lambda i=i: ops.linear_attention(la(i == 0, 32), la(i == 1, 64), la(i == 2, 32))
    return calls


@pytest.mark.parametrize("ld", BAD_STRIDES)
def test_every_wrapper_refuses_a_stride_that_does_not_fit_before_the_library_is_called(built_lib, monkeypatch, ld):
    lib = _lib.load()
    _no_side_paths(monkeypatch)

    def reached(name):
        def fn(*a, **k):
            pytest.fail(f"{name} was called with a stride that does not fit its field")
        return fn

    for name in _lib.EXPORTS:
        if name not in ("svdq_last_error", "svdq_abi_version"):
            monkeypatch.setattr(lib, name, reached(name), raising=True)
    for name, call in _wrapper_calls(ld).items():
        with pytest.raises(ValueError, match=r"does not fit the library's (32|64)-bit field"):
            call()
        print("refused:", name)
    assert len(_wrapper_calls(ld)) == 37


def test_the_stand_in_calls_reach_the_library_with_strides_that_fit(built_lib, monkeypatch):
    """the same calls with a stride that fits get as far as the library: it is the stride, nothing else about the stand-ins, that the test above sees refused"""
    lib = _lib.load()

    class Reached(Exception):
        pass

    def fn(*a, **k):
        raise Reached

    for name in _lib.EXPORTS:
        if name.startswith("svdq_") and name not in ("svdq_last_error", "svdq_abi_version"):
            monkeypatch.setattr(lib, name, fn, raising=True)
    from nunchaku_amd import _C

    _no_side_paths(monkeypatch)
    monkeypatch.setattr(_C, "_stream", lambda: 0)  # (no device here: the stream handle is an argument of the call that is never made)
    for name, call in _wrapper_calls(2 ** 20).items():
        if "64-bit" in name or "meta" in name:
            continue
        with pytest.raises(Reached):
            call()


# what a wrapper may put into a stride or extent field of an args struct
EXTENT_FIELD = re.compile(r"^(M|M2|M_pad|N|K|R|R2|r|T|B|H|W|C|C_pad|L|L_pad|Nrows|max_keys|head_dim|split_rows)$")


def test_every_stride_and_extent_assignment_in_the_wrappers_is_a_checked_call():
    """By inspection of nunchaku_amd/_C.py: whatever is assigned to ``a.<field>`` / ``args.<field>`` with a stride name (ld*, *_hs, *_bs) or an extent name is
    a call of ``_i32`` / ``_i64`` (or of ``_row_view`` / ``_second_rows``, which return nothing but such calls), a generator of such calls, an integer literal,
    or another field of the same struct.  Tuple assignments are matched element by element."""
    from nunchaku_amd import _C

    tree = ast.parse(inspect.getsource(_C))
    checked = {"_i32", "_i64", "_row_view", "_second_rows"}

    def ok(v):
        if isinstance(v, ast.Call) and isinstance(v.func, ast.Name):
            return v.func.id in checked
        if isinstance(v, ast.GeneratorExp):
            return ok(v.elt)
        if isinstance(v, ast.Constant):
            return type(v.value) is int
        return isinstance(v, ast.Attribute) and isinstance(v.value, ast.Name) and v.value.id in ("a", "args")

    def pairs(target, value):
        if isinstance(target, ast.Tuple) and isinstance(value, ast.Tuple) and len(value.elts) == len(target.elts):
            for t, v in zip(target.elts, value.elts):
                yield from pairs(t, v)
        elif isinstance(target, ast.Tuple):
            for t in target.elts:
                yield from pairs(t, value)
        else:
            yield target, value

    seen, bad = set(), []
    for node in (n for n in ast.walk(tree) if isinstance(n, ast.Assign)):
        for target in node.targets:
            for t, v in pairs(target, node.value):
                if isinstance(t, ast.Attribute) and isinstance(t.value, ast.Name) and t.value.id in ("a", "args") and (STRIDE_FIELD.match(t.attr) or EXTENT_FIELD.match(t.attr)):
                    seen.add(t.attr)
                    if not ok(v):
                        bad.append(f"line {node.lineno}: {ast.unparse(t)} = {ast.unparse(v)}")
    for fn in (n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name in ("_row_view", "_second_rows")):
        for ret in (n for n in ast.walk(fn) if isinstance(n, ast.Return)):
            elts = ret.value.elts if isinstance(ret.value, ast.Tuple) else [ret.value]
            bad += [f"{fn.name} returns {ast.unparse(e)}" for e in elts if not (ok(e) or isinstance(e, ast.Subscript))]  # (the dtype code: _DT[...])
    assert not bad, "\n".join(bad)
    strides = {f for cls in _structs().values() for f, _ in cls._fields_ if STRIDE_FIELD.match(f)}
    assert strides <= seen, f"stride fields no wrapper assigns: {sorted(strides - seen)}"


# ---- 3. svdq_quantize_plan around the fast kernel's 2 GiB line ----------------------------------------------------------------------------
M_PAD, K = 256, 384
LINE = 2 ** 22  # M_pad * ld * 2 = 2^31 bytes at M_pad = 256


@pytest.mark.parametrize("R", (0, 32, 96))
def test_the_quantiser_leaves_the_fast_kernel_at_2_gib(built_lib, R):
    plan = lambda **kw: T.quant_plan(R, True, False, False, kw.pop("grouped", False), "f32", 300 if kw.get("grouped_m") else 200, K, M_PAD, **kw)
    below, at = plan(ldx=LINE - 8), plan(ldx=LINE)
    assert below["family"] == "fast" and below["sel"] == (8 if R > 32 else 0) | (4 if R else 0) | 1
    assert at["family"] == "general" and at["sel"] == math.ceil(R / 32) + (R > 64)  # rank classes 0, 1, (2,) 4: ceil(96 / 32) = 3 runs class 4
    # everything else about the launch is the same on both sides of the line
    assert {k: v for k, v in below.items() if k not in ("family", "sel")} == {k: v for k, v in at.items() if k not in ("family", "sel")}
    assert (below["cpw"], below["slices"], below["grid"], below["lora_act_add"]) == (4, 1, M_PAD // 32, 0)
    # the last stride of the fast kernel exactly: M_pad * ld * 2 < 0x7fffffff, ld a multiple of 4
    assert plan(ldx=LINE - 4)["family"] == "fast"
    # the same pair on the second stream's stride of a grouped launch whose first stride is small (M_pad = 512: 256 rows + 44)
    grouped = lambda ldx2: T.quant_plan(R, True, False, False, True, "f32", 300, K, 512, ldx2=ldx2)
    assert grouped(LINE // 2 - 8)["family"] == "fast" and grouped(LINE // 2)["family"] == "general"
    assert grouped(K)["family"] == "fast"


def test_the_lora_down_clause_at_its_own_line(built_lib):
    """R * K * 2 < 0x7fffffff guards the fast kernel's descriptor over lora_down.  At rank 128 its line is K = 2^23.  The grid rule gets there first: the fast
    kernel needs cpw = 4, which the smallest launch (M_pad = 256, 8 row tiles) keeps only up to K = 2^19 -- so on both sides of the clause's line the launch is
    the general kernel's already, and below K = 2^19 the largest rank of the fast kernel stays 2^4 short of the line.  The clause cannot wrap and cannot be
    reached: both are pinned here, so a change of the grid rule that exposes it meets this test."""
    for Kbig in (2 ** 23 - 128, 2 ** 23):
        pl = T.quant_plan(128, True, False, False, False, "f32", 200, Kbig, M_PAD)
        assert pl["family"] == "general" and pl["cpw"] > 4, (Kbig, pl)
    pl = T.quant_plan(160, True, False, False, False, "f32", 200, 2 ** 19, M_PAD)
    assert pl["family"] == "fast" and pl["cpw"] == 4 and 160 * 2 ** 19 * 2 * 8 < 0x7fffffff, pl
    assert T.quant_plan(160, True, False, False, False, "f32", 200, 2 ** 19 + 128, M_PAD)["cpw"] == 8


def _former_quant_grid(M_pad: int, K: int):
    """(chunks per workgroup, K slices) as tests/test_gpu_hot_instantiations.py restated launch_quantize's rule before the library answered"""
    KP, tiles, cpw = K // 128, M_pad // 32, 4
    while cpw < KP and tiles * math.ceil(KP / cpw) > 8192:
        cpw *= 2
    if cpw > KP:
        cpw = (KP + 3) // 4 * 4
    return cpw, math.ceil(KP / cpw)


def _former_quant_instantiation(case):
    R, smooth, ln, glu, _, _, M, K, pad = case
    cpw, _ = _former_quant_grid(math.ceil(M / pad) * pad, K)
    if not glu and R <= 160 and cpw == 4:
        return "quantize_kernel_v2", (int(R > 0), int(ln), int(smooth), int(R > 32))
    rt = math.ceil(R / 32)
    return "quantize_kernel", (0 if rt == 0 else 1 if rt <= 1 else 2 if rt <= 2 else 4 if rt <= 4 else 8, 1, int(glu))


def test_the_plan_agrees_with_the_former_restatement_on_the_whole_case_table(built_lib):
    assert len(T.QUANT_CASES) == 32
    for case in T.QUANT_CASES:
        R, smooth, ln, glu, grouped, fmt, M, K_, pad = case
        M_pad = math.ceil(M / pad) * pad
        pl = T.quant_plan(R, smooth, ln, glu, grouped, fmt, M, K_, M_pad)
        assert (pl["cpw"], pl["slices"]) == _former_quant_grid(M_pad, K_) == T.quant_grid(M_pad, K_), case
        assert T.quant_instantiation(case) == _former_quant_instantiation(case), case
        assert pl["grid"] == M_pad // 32 * pl["slices"] and pl["glu"] == glu
        assert pl["lora_act_add"] == (pl["slices"] > 1) + 2 * (fmt != "f32") and pl["memset"] == (R > 0 and pl["slices"] > 1)


def test_the_plan_query_refuses_what_the_launch_refuses(built_lib):
    lib = _lib.load()
    out = (C.c_int32 * 8)(*([-1] * 8))
    assert lib.svdq_quantize_plan(None, out) == 1 and b"NULL" in lib.svdq_last_error()
    a = _lib.QuantizeArgs()
    a.x, a.act, a.ascales = 16, 16, 16
    a.M, a.M_pad, a.K, a.ldx = 10, 100, 128, 128
    for fn in (lambda: lib.svdq_quantize_plan(C.byref(a), out), lambda: lib.svdq_quantize_w4a4_act_fuse_lora(C.byref(a), None)):
        assert fn() == 1 and b"M_pad" in lib.svdq_last_error()
    a.M_pad, a.fp4 = 256, 1
    assert lib.svdq_quantize_plan(C.byref(a), out) == 2 and list(out) == [-1] * 8
    a.fp4 = 0
    assert lib.svdq_quantize_plan(C.byref(a), None) == 1
    assert lib.svdq_quantize_plan(C.byref(a), out) == 0 and list(out) == [0, 0, 4, 1, 0, 8, 0, 0]
