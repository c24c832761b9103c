"""PuLID without a GPU: the C ABI of svdq_pulid_ca (declaration, layout, export, validation), the fold against the reference composition in
float64, the kernel's rounding points restated on the CPU against the 16-bit torch-op sequence, the module tree, the loader and the engine
hook's torch-op arm on a toy model."""

import ctypes as C
import json
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from nunchaku_amd import _lib
from nunchaku_amd.models import pulid
from nunchaku_amd.models.flux import FluxTransformerAMD
from tests import pulid_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_bindings_sources_and_kernel_name_agree():
    text = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    assert re.search(r"^typedef struct svdq_pulid_ca_args \{", text, re.M)
    assert re.search(r"^int svdq_pulid_ca\(const svdq_pulid_ca_args \*args, void \*stream\);", text, re.M)
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M)
    assert _lib.ABI_VERSION == 24 and "svdq_pulid_ca" in _lib.EXPORTS
    from nunchaku_amd import build
    from nunchaku_amd._C import ops

    assert "pulid_ca.hip" in build.SOURCES and callable(ops.pulid_ca)
    src = open(os.path.join(ROOT, "nunchaku_amd", "csrc", "pulid_ca.hip")).read()
    kernels = re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)
    assert kernels and all(re.fullmatch(r"pulid_\w+_kernel", k) for k in kernels), kernels  # (the ledgers count other names)
    from nunchaku_amd import ops as public_ops

    assert callable(public_ops.pulid_ca)


def test_struct_layout_matches_header(built_lib, tmp_path):
    cname, cls = "svdq_pulid_ca_args", _lib.PulidCaArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "svdq_amd.h")}"', "int main(void) {",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"offsetof({cname}, {f})"


def test_exported_and_validation_errors_are_returned(built_lib):
    """every refusal comes back before a launch (there is no GPU here: a launch would be a HIP error, code 3)"""
    lib = _lib.load()
    assert hasattr(C.CDLL(built_lib), "svdq_pulid_ca") and lib.svdq_abi_version() == 24
    call = lambda a: (lib.svdq_pulid_ca(C.byref(a), None), lib.svdq_last_error())
    assert lib.svdq_pulid_ca(None, None) == 1 and b"NULL" in lib.svdq_last_error()
    pointers = ("x", "stats", "a_fold", "colsum", "cbias", "b_fold", "probs", "out")

    def good():
        a = _lib.PulidCaArgs()
        for i, name in enumerate(pointers):
            setattr(a, name, 4096 * (i + 1))
        a.ldx, a.ldo, a.T, a.C, a.H, a.N, a.dtype, a.out_scale = 264, 256, 33, 256, 4, 5, 0, 1.0
        return a

    for ptr in pointers:
        a = good()
        setattr(a, ptr, None)
        rc, msg = call(a)
        assert rc == 1 and b"are required" in msg, (ptr, msg)
    for ptr in pointers + ("acc", "o_acc"):
        a = good()
        setattr(a, ptr, (getattr(a, ptr) or 65536) + (4 if ptr == "stats" else 8))
        rc, msg = call(a)
        assert rc == 1 and b"aligned" in msg, (ptr, msg)
    for ld in ("ldx", "ldo"):
        a = good()
        setattr(a, ld, 248)
        rc, msg = call(a)
        assert rc == 1 and b"at least C = 256" in msg
        setattr(a, ld, 260)
        rc, msg = call(a)
        assert rc == 1 and b"multiple of 8" in msg
    for field in ("T", "C", "H"):
        a = good()
        setattr(a, field, 0)
        rc, msg = call(a)
        assert rc == 1 and b">= 1" in msg
    for c in (64, 192, 200):
        a = good()
        a.C, a.ldx, a.ldo = c, 512, 512
        rc, msg = call(a)
        assert rc == 2 and b"multiples of 128" in msg, (c, msg)
    for h in (1, 2, 6):
        a = good()
        a.H = h
        rc, msg = call(a)
        assert rc == 2 and b"multiples of 4" in msg, (h, msg)
    a = good()
    a.H = 20
    rc, msg = call(a)
    assert rc == 2 and b"at most 512" in msg
    for n, code in ((0, 1), (-1, 1), (33, 2)):
        a = good()
        a.N = n
        rc, msg = call(a)
        assert rc == code and b"N=" in msg, (n, msg)
    a = good()
    a.dtype = 7
    rc, msg = call(a)
    assert rc == 1 and b"dtype" in msg
    for s in (float("inf"), float("-inf"), float("nan")):
        a = good()
        a.out_scale = s
        rc, msg = call(a)
        assert rc == 1 and b"out_scale" in msg


def test_wrapper_refuses_cpu_tensors_and_mismatched_shapes(built_lib):
    from nunchaku_amd._C import ops

    bf = torch.bfloat16
    x, a = torch.zeros(8, 256, dtype=bf), torch.zeros(128, 256, dtype=bf)
    st, v, pr = torch.zeros(8, 2), torch.zeros(128), torch.zeros(8, 128, dtype=bf)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ops.pulid_ca(x, st, a, v, v, a, pr, torch.zeros_like(x), 5)
    with pytest.raises(ValueError, match="share one 16-bit dtype"):
        ops.pulid_ca(x, st, a.half(), v, v, a, pr, torch.zeros_like(x), 5)
    with pytest.raises(ValueError, match=r"a_fold must be a contiguous \[H \* 32, C\]"):
        ops.pulid_ca(x, st, a[:100], v, v, a, pr, torch.zeros_like(x), 5)
    with pytest.raises(ValueError, match="probs must be"):
        ops.pulid_ca(x, st, a, v, v, a, pr[:, :64], torch.zeros_like(x), 5)
    with pytest.raises(ValueError, match="stats must be"):
        ops.pulid_ca(x, st.double(), a, v, v, a, pr, torch.zeros_like(x), 5)


# ---- the fold -----------------------------------------------------------------------------------------------------------------------
DIM, HEADS, KV, DH = 256, 4, 64, 32


def _case(tokens, dtype=torch.bfloat16, seed=0, T=40):
    g = torch.Generator().manual_seed(100 + seed)
    mod = ref.make_module(DIM, HEADS, KV, DH, seed=seed, dtype=dtype)
    x = torch.randn(1, tokens, KV, generator=g).to(dtype)
    lat = ref.stream_inputs(T, DIM, seed, dtype)
    return mod, x, lat


@pytest.mark.parametrize("tokens", [5, 32])
def test_fold_equals_the_reference_composition_in_float64(tokens):
    mod, x, lat = _case(tokens)
    assert (mod.norm2.weight.float() - 1).abs().max() > 0.1 and mod.norm2.bias.float().abs().max() > 0.05  # both non-trivial
    want, got = ref.compose64(mod, x, lat), ref.folded64(mod, x, lat)
    assert want.shape == got.shape == (lat.shape[0], DIM)
    rel = ((got - want).abs().max() / want.abs().max()).item()
    print(f"tokens {tokens}: folded vs composed, float64: {rel:.3g}")
    assert rel <= 1e-9


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("tokens", [5, 32])
def test_rounding_points_stay_within_the_envelope_of_the_torch_op_sequence(tokens, dtype):
    """the kernel's rounding points (fold rounded once, 16-bit probabilities, two output roundings) against float64: max and mean error at
    most 1.5 x those of the module's own 16-bit torch-op sequence on the same inputs (the margin of the GPU accuracy test)"""
    td = ref.TD[dtype]
    mod, x, lat = _case(tokens, td, seed=1)
    want = ref.compose64(mod, x, lat)
    fold = mod.fold(x)
    assert fold.tokens == tokens and fold.a_fold.shape == (HEADS * 32, DIM) and fold.a_fold.dtype == td
    assert torch.equal(fold.colsum, fold.a_fold.float().sum(-1))  # over the ROUNDED keys
    rows = fold.a_fold.view(HEADS, 32, DIM)
    assert (rows[:, tokens:] == 0).all() and (fold.b_fold.view(HEADS, 32, DIM)[:, tokens:] == 0).all()
    out, probs = ref.kernel_ref(lat, fold)
    assert (probs.view(-1, HEADS, 32)[:, :, tokens:] == 0).all()
    assert (probs.float().view(-1, HEADS, 32).sum(-1) - 1).abs().max() < 32 * (2.0 ** -8 if dtype == "bf16" else 2.0 ** -11)
    with torch.no_grad():
        torch16 = mod(x, lat[None])[0]
    err = (out.double() - want).abs()
    err16 = (torch16.double() - want).abs()
    print(f"tokens {tokens} {dtype}: restatement max {err.max():.3g} mean {err.mean():.3g}; torch ops max {err16.max():.3g} mean {err16.mean():.3g}")
    assert err.max() <= 1.5 * err16.max() and err.mean() <= 1.5 * err16.mean()


def test_exp_restatement_is_accurate_and_cuts_off():
    d = torch.cat([torch.linspace(-80, 0, 4001), torch.tensor([-80.5, -100.0, -1e4, float("-inf")])])
    e = ref.exp_ref(d)
    want = torch.exp(d[:4001].double())
    assert ((e[:4001].double() - want).abs() / want).max() < 2.0 ** -21
    assert (e[4001:] == 0).all() and e[4000] == 1.0


def test_fold_is_cached_per_tensor_object_and_version():
    mod, x, _ = _case(5)
    calls = []
    make = mod._make_fold
    mod._make_fold = lambda t: (calls.append(1), make(t))[1]
    f = mod.fold(x)
    assert mod.fold(x) is f and len(calls) == 1
    x.mul_(2)
    assert mod.fold(x) is not f and len(calls) == 2
    mod.fold(x.clone())
    assert len(calls) == 3
    with torch.inference_mode():
        inf = torch.randn(1, 5, KV).bfloat16()
    mod.fold(inf), mod.fold(inf)
    assert len(calls) == 5
    mod.load_state_dict(mod.state_dict())  # new weights: the entry is dropped
    assert mod._fold_cache is None
    with pytest.raises(NotImplementedError, match="33 identity tokens"):
        mod.fold(torch.zeros(1, 33, KV, dtype=torch.bfloat16))


# ---- module tree, loader ------------------------------------------------------------------------------------------------------------
def test_child_names_and_shapes_equal_the_reference_modules():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pulid_ca_keys.json")))
    with torch.device("meta"):
        mod = pulid.PerceiverAttentionCA()
    assert {k: list(v.shape) for k, v in mod.state_dict().items()} == golden
    assert [n for n, _ in mod.named_children()] == ["norm1", "norm2", "to_q", "to_kv", "to_out"]
    from nunchaku.models.pulid.encoders_transformer import PerceiverAttentionCA
    from nunchaku.models.pulid.pulid_forward import pulid_forward

    assert PerceiverAttentionCA is pulid.PerceiverAttentionCA and pulid_forward is pulid.pulid_forward


class Shell(nn.Module):
    """a transformer as the loader sees it: blocks to count, a width, a dtype and a device"""

    def __init__(self, joint=19, single=38, dim=3072):
        super().__init__()
        self.transformer_blocks = nn.ModuleList([nn.Identity() for _ in range(joint)])
        self.single_transformer_blocks = nn.ModuleList([nn.Identity() for _ in range(single)])
        self.proj_out = nn.Linear(dim, 8, dtype=torch.bfloat16, device="meta")
        self.dim, self.dtype_ = dim, torch.bfloat16


def test_attach_loads_twenty_modules_strictly_and_ignores_the_encoder(tmp_path):
    sd = ref.module_state_dict(20, 128, 1, 32, seed=3)
    e = Shell(dim=128)
    e.proj_out = nn.Linear(128, 8, dtype=torch.bfloat16)
    assert pulid.pulid_module_count(e) == 20
    mods = pulid.attach_pulid(e, sd)
    assert e.pulid_ca is mods and len(mods) == 20 and isinstance(mods, nn.ModuleList)
    for k, m in enumerate(mods):
        assert m.heads == 1 and m.to_kv.weight.shape == (256, 32)
        for name, t in m.state_dict().items():
            assert torch.equal(t, sd[f"pulid_ca.{k}.{name}"])
    assert not any("encoder" in k for k in e.state_dict())
    from safetensors.torch import save_file

    save_file(sd, str(tmp_path / "pulid_flux_v0.9.1.safetensors"))
    assert len(pulid.attach_pulid(e, tmp_path)) == 20 and len(pulid.attach_pulid(e, str(tmp_path / "pulid_flux_v0.9.1.safetensors"))) == 20
    with pytest.raises(ValueError, match="has 20 modules, the transformer needs 3"):
        pulid.attach_pulid(Shell(2, 5, 128), sd)
    extra = dict(sd)
    extra["pulid_ca.7.to_q.bias"] = torch.zeros(128)
    with pytest.raises(RuntimeError, match="Unexpected key"):  # strict=True
        pulid.attach_pulid(e, extra)
    missing = {k: v for k, v in sd.items() if k != "pulid_ca.4.norm2.bias"}
    with pytest.raises(RuntimeError, match="Missing key"):
        pulid.attach_pulid(e, missing)
    with pytest.raises(KeyError, match="not a PuLID file"):
        pulid.attach_pulid(e, {"pulid_encoder.latents": torch.zeros(2)})
    wide = ref.module_state_dict(20, 256, 1, 32)
    with pytest.raises(ValueError, match="256 channels, the transformer has 128"):
        pulid.attach_pulid(e, wide)
    assert pulid.detach_pulid(e) is e and getattr(e, "pulid_ca", None) is None
    pulid.detach_pulid(e)  # twice is fine


# ---- engine hook, torch-op arm ------------------------------------------------------------------------------------------------------
class _Attn:
    attention_impl, head_dim = "sdpa", 128


class _Joint(nn.Module):
    def __init__(self, log, i):
        super().__init__()
        self.log, self.i, self.attn = log, i, _Attn()

    def forward(self, hidden, enc, temb_act, rot, stats=None, mods=None, kv_valid=None, keep_input=False):
        self.log.append(("joint", self.i))
        return enc * 0.5 + 0.25, hidden * 0.75 + enc.mean() + 0.125 * (self.i + 1), None


class _Single(nn.Module):
    def __init__(self, log, i):
        super().__init__()
        self.log, self.i, self.attn = log, i, _Attn()

    def forward(self, hidden, temb_act, rot, stats=None, mods=None, kv_valid=None, keep_input=False):
        self.log.append(("single", self.i))
        return hidden * 0.75 + 0.0625 * (self.i + 1), None


T_IMG, T_TXT = 6, 3


def _toy(log):
    """2 joint + 5 single blocks -- the smallest model on which modules 0, 1 and 2 apply at joint block 0 and single blocks 0 and 4 --
    with the engine's own embedders and tail, and blocks that are plain arithmetic"""
    torch.manual_seed(0)
    m = FluxTransformerAMD(num_layers=0, num_single_layers=0, dim=128, heads=1, in_channels=16, joint_attention_dim=32,
                           pooled_projection_dim=16, torch_dtype=torch.float32, device="cpu")
    for p in m.parameters():
        nn.init.normal_(p, std=0.1)
    m.transformer_blocks = nn.ModuleList([_Joint(log, i) for i in range(2)])
    m.single_transformer_blocks = nn.ModuleList([_Single(log, i) for i in range(5)])
    m.fused_norm = False
    sd = ref.module_state_dict(3, 128, 1, 32, seed=5, dtype=torch.float32)
    for k in range(3):
        sd[f"pulid_ca.{k}.to_out.weight"].zero_()
    pulid.attach_pulid(m, sd)
    for k, mod in enumerate(m.pulid_ca):
        mod.register_forward_hook(lambda mod, args, out, k=k: log.append(("pulid", k, tuple(args[1].shape))))
    g = torch.Generator().manual_seed(1)
    inputs = (torch.randn(1, T_IMG, 16, generator=g), torch.randn(1, T_TXT, 32, generator=g), torch.randn(1, 16, generator=g),
              torch.tensor([0.5]), torch.zeros(T_IMG, 3), torch.zeros(T_TXT, 3), torch.tensor([3.5]))
    return m, inputs


@torch.no_grad()
def test_engine_applies_modules_0_1_2_at_joint_0_and_singles_0_and_4():
    log = []
    m, inputs = _toy(log)
    emb = torch.randn(1, 4, 32, generator=torch.Generator().manual_seed(2))
    plain = m.engine_forward(*inputs)
    assert [e for e in log if e[0] == "pulid"] == []
    del log[:]
    zero = m.engine_forward(*inputs, id_embeddings=emb, id_weight=0.7)
    shape = (1, T_IMG, 128)  # the image rows alone, in the joined stream too
    assert log == [("joint", 0), ("pulid", 0, shape), ("joint", 1), ("single", 0), ("pulid", 1, shape), ("single", 1), ("single", 2),
                   ("single", 3), ("single", 4), ("pulid", 2, shape)]
    assert torch.equal(zero, plain)  # every to_out is zero: nothing is added
    outs = []
    for k in range(3):  # one module's to_out non-zero at a time: each of the three changes the result, each differently
        w = m.pulid_ca[k].to_out.weight
        w.copy_(torch.randn(w.shape, generator=torch.Generator().manual_seed(10 + k)) * 0.1)
        outs.append(m.engine_forward(*inputs, id_embeddings=emb, id_weight=0.7))
        assert not torch.allclose(outs[-1], plain, atol=1e-4), k
        assert torch.equal(m.engine_forward(*inputs, id_embeddings=emb, id_weight=0.0), plain), k  # the strength multiplies what it adds
        w.zero_()
    assert not torch.allclose(outs[0], outs[1], atol=1e-4) and not torch.allclose(outs[1], outs[2], atol=1e-4)
    # the reference's signature, bound as the forward; the gates compare on the host
    pulid.apply_pulid_forward(m)
    m.pulid_ca[2].to_out.weight.copy_(torch.randn(128, 128, generator=torch.Generator().manual_seed(12)) * 0.1)
    kw = dict(encoder_hidden_states=inputs[1], pooled_projections=inputs[2], timestep=inputs[3], img_ids=inputs[4], txt_ids=inputs[5],
              guidance=inputs[6], return_dict=False)
    on = m(inputs[0], emb, 0.7, **kw)[0]
    assert torch.equal(on, outs[2])
    assert torch.equal(m(inputs[0], emb, 0.7, start_timestep=0.6, **kw)[0], plain)  # 0.6 > t = 0.5: not yet
    assert torch.equal(m(inputs[0], emb, 0.7, end_timestep=0.4, **kw)[0], plain)    # 0.4 < t: no longer
    assert torch.equal(m(inputs[0], emb, 0.7, start_timestep=0.5, end_timestep=0.5, **kw)[0], on)
    assert torch.equal(m(inputs[0], None, None, **kw)[0], plain)


@torch.no_grad()
def test_each_refusal_raises():
    m, inputs = _toy([])
    emb = torch.zeros(1, 4, 32)
    two = tuple(torch.cat([t, t]) if i in (0, 1, 2) else t for i, t in enumerate(inputs))
    with pytest.raises(ValueError, match="batch 1 only"):
        m.engine_forward(*two, id_embeddings=emb)
    m._is_cached, m.residual_diff_threshold_multi = True, 0.12
    with pytest.raises(NotImplementedError, match="First-Block Cache"):
        m.engine_forward(*inputs, id_embeddings=emb)
    m.residual_diff_threshold_multi = -1.0  # switched off: runs
    m.engine_forward(*inputs, id_embeddings=emb)
    m._is_cached = False
    m.cnt = 0  # (TeaCache's state on the model)
    with pytest.raises(NotImplementedError, match="TeaCache"):
        m.engine_forward(*inputs, id_embeddings=emb)
    del m.cnt
    m.offload = True
    with pytest.raises(NotImplementedError, match="offloaded"):
        m.engine_forward(*inputs, id_embeddings=emb)
    m.offload = False
    mods = m.pulid_ca
    m.pulid_ca = nn.ModuleList(list(mods)[:2])
    with pytest.raises(ValueError, match="2 PuLID modules are attached, the transformer needs 3"):
        m.engine_forward(*inputs, id_embeddings=emb)
    pulid.detach_pulid(m)
    with pytest.raises(ValueError, match="no PuLID modules are attached"):
        m.engine_forward(*inputs, id_embeddings=emb)
    m.engine_forward(*inputs)  # without embeddings nothing is asked of the modules
