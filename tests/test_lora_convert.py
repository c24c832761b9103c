"""diffusers / PEFT LoRA -> engine factors (nunchaku_amd/lora/flux.py): index work on the logical factors, checked with dense
linear algebra in float64.  The factors are small integers, so every product and sum below is exact and ``torch.equal`` is
the right comparison whatever the summation order (alpha / r is a power of two for the same reason)."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from nunchaku_amd import _lib
from nunchaku_amd.lora import flux as lora_flux
from nunchaku_amd.models.flux import FluxTransformerAMD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM, IN_CH = 256, 64


def _model():
    return FluxTransformerAMD(num_layers=1, num_single_layers=1, dim=DIM, heads=2, in_channels=IN_CH, joint_attention_dim=128,
                              pooled_projection_dim=64, device="cpu")


def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).double()


def make_peft_lora(seed=0, prefix="transformer."):
    """A synthetic PEFT dict for the 1 joint + 1 single block engine: ranks 4 and 16, one alpha, q/k/v with k missing, a single block's
    proj_out, one modulation layer, x_embedder, a bias delta.  Returns (state dict, {diffusers module: delta W float64})."""
    g = torch.Generator().manual_seed(seed)
    J, S = "transformer_blocks.0", "single_transformer_blocks.0"
    shapes = {  # module: (out, in, r)
        f"{J}.attn.to_q": (DIM, DIM, 4), f"{J}.attn.to_v": (DIM, DIM, 4),  # to_k missing
        f"{J}.attn.add_q_proj": (DIM, DIM, 16), f"{J}.attn.add_k_proj": (DIM, DIM, 16), f"{J}.attn.add_v_proj": (DIM, DIM, 16),
        f"{J}.attn.to_out.0": (DIM, DIM, 4), f"{J}.attn.to_add_out": (DIM, DIM, 4),
        f"{J}.ff.net.0.proj": (4 * DIM, DIM, 16), f"{J}.ff.net.2": (DIM, 4 * DIM, 4),
        f"{J}.ff_context.net.0.proj": (4 * DIM, DIM, 4), f"{J}.ff_context.net.2": (DIM, 4 * DIM, 4),
        f"{J}.norm1.linear": (6 * DIM, DIM, 4),
        f"{S}.attn.to_q": (DIM, DIM, 4), f"{S}.attn.to_k": (DIM, DIM, 16), f"{S}.attn.to_v": (DIM, DIM, 4),
        f"{S}.proj_mlp": (4 * DIM, DIM, 4), f"{S}.proj_out": (DIM, 5 * DIM, 16), f"{S}.norm.linear": (3 * DIM, DIM, 16),
        "x_embedder": (DIM, IN_CH, 4), "proj_out": (IN_CH, DIM, 4),
    }
    alphas = {f"{J}.ff.net.0.proj": 8.0, f"{S}.attn.to_k": 32.0}  # alpha / r = 1/2 and 2
    sd, dw = {}, {}
    for name, (o, i, r) in shapes.items():
        A, B = _ints(g, r, i), _ints(g, o, r)
        sd[f"{prefix}{name}.lora_A.weight"], sd[f"{prefix}{name}.lora_B.weight"] = A, B
        dw[name] = B @ A
        if name in alphas:
            sd[f"{prefix}{name}.alpha"] = torch.tensor(alphas[name])
            dw[name] = dw[name] * (alphas[name] / r)
    sd[f"{prefix}proj_out.diff_b"] = _ints(g, IN_CH)
    return sd, dw


def engine_delta_w(eng, name):
    down, up = eng[name]
    return up.double() @ down.double()


def check_engine_lora(eng, dw):
    """every target's delta W, rebuilt from what the engine layers were handed, against the source's"""
    J, S = "transformer_blocks.0", "single_transformer_blocks.0"
    # fused QKV: block-diagonal up over concatenated down
    for tgt, members in ((f"{J}.attn.to_qkv", [f"{J}.attn.to_q", f"{J}.attn.to_k", f"{J}.attn.to_v"]),
                         (f"{J}.attn.add_qkv_proj", [f"{J}.attn.add_q_proj", f"{J}.attn.add_k_proj", f"{J}.attn.add_v_proj"]),
                         (f"{S}.attn.to_qkv", [f"{S}.attn.to_q", f"{S}.attn.to_k", f"{S}.attn.to_v"])):
        full = engine_delta_w(eng, tgt)
        assert full.shape == (3 * DIM, DIM)
        for i, m in enumerate(members):
            want = dw[m] if m in dw else torch.zeros(DIM, DIM, dtype=torch.float64)
            assert torch.equal(full[i * DIM:(i + 1) * DIM], want), m
    # a single block's proj_out: [attention | mlp] input split over the two projections the engine adds
    full = torch.cat([engine_delta_w(eng, f"{S}.attn.to_out"), engine_delta_w(eng, f"{S}.mlp_fc2")], dim=1)
    assert torch.equal(full, dw[f"{S}.proj_out"])
    assert torch.equal(eng[f"{S}.attn.to_out"][1], eng[f"{S}.mlp_fc2"][1])
    # same names
    for src, tgt in ((f"{J}.attn.to_out.0", None), (f"{J}.attn.to_add_out", None), (f"{J}.ff.net.0.proj", None), (f"{J}.ff.net.2", None),
                     (f"{J}.ff_context.net.0.proj", None), (f"{J}.ff_context.net.2", None), (f"{J}.norm1.linear", None),
                     (f"{S}.proj_mlp", f"{S}.mlp_fc1"), (f"{S}.norm.linear", None), ("x_embedder", None), ("proj_out", None)):
        assert torch.equal(engine_delta_w(eng, tgt or src), dw[src]), src


def test_every_target_rebuilds_the_source_delta_w():
    sd, dw = make_peft_lora()
    model = _model()
    eng = lora_flux.to_engine_lora(sd, model)
    check_engine_lora(eng, dw)
    down, up = eng["transformer_blocks.0.attn.to_qkv"]
    assert down.shape == (8, DIM) and up.shape == (3 * DIM, 8)  # k missing: its ranks are not there at all
    assert not up[DIM:2 * DIM].any() and not up[:DIM, 4:].any() and not up[2 * DIM:, :4].any()
    mods = dict(model.named_modules())
    assert all(k in mods or (k.endswith(".bias") and k[:-5] in mods) for k in eng)  # engine names, taken from the model
    assert torch.equal(eng["proj_out.bias"], sd["transformer.proj_out.diff_b"])
    # the modulation layer's up keeps the checkpoint's interleaved row order (out_chunks is the kernel's business)
    assert torch.equal(eng["transformer_blocks.0.norm1.linear"][1], sd["transformer.transformer_blocks.0.norm1.linear.lora_B.weight"])
    # bare keys give the same
    bare = lora_flux.to_engine_lora({k[len("transformer."):]: v for k, v in sd.items()}, model)
    assert bare.keys() == eng.keys() and all(torch.equal(bare[k][0], eng[k][0]) and torch.equal(bare[k][1], eng[k][1]) for k in eng if not k.endswith(".bias"))


def test_x_embedder_narrower_than_the_model_is_zero_padded():
    g = torch.Generator().manual_seed(3)
    A, B = _ints(g, 4, IN_CH - 16), _ints(g, DIM, 4)
    eng = lora_flux.to_engine_lora({"x_embedder.lora_A.weight": A, "x_embedder.lora_B.weight": B}, _model())
    full = engine_delta_w(eng, "x_embedder")
    assert torch.equal(full[:, :IN_CH - 16], B @ A) and not full[:, IN_CH - 16:].any()


def test_compose_lora_is_the_weighted_sum():
    sd1, dw1 = make_peft_lora(seed=1)
    sd2, dw2 = make_peft_lora(seed=2, prefix="")
    del sd2["single_transformer_blocks.0.proj_mlp.lora_A.weight"], sd2["single_transformer_blocks.0.proj_mlp.lora_B.weight"]
    del dw2["single_transformer_blocks.0.proj_mlp"]
    comp = lora_flux.compose_lora([(sd1, 0.5), (sd2, -1.25)])
    assert not any(k.endswith(".alpha") for k in comp)
    want = {k: 0.5 * dw1[k] - 1.25 * dw2.get(k, 0) for k in dw1}
    eng = lora_flux.to_engine_lora(comp, _model())
    got = {}
    for k in dw1:  # per diffusers module, from the composed PEFT dict itself
        got[k] = comp[f"{k}.lora_B.weight"] @ comp[f"{k}.lora_A.weight"]
        assert comp[f"{k}.lora_A.weight"].shape[0] == (sd1[f"transformer.{k}.lora_A.weight"].shape[0] + (sd2[f"{k}.lora_A.weight"].shape[0] if k in dw2 else 0))
        # float64 rounding: the strengths are folded into B before the product (values are O(1e3), spacing 2e-13)
        assert (got[k] - want[k]).abs().max() <= 1e-9, k
    check = {k: got[k] for k in got}
    check_engine_lora(eng, check)  # and the composed dict converts like any other
    assert torch.equal(eng["proj_out.bias"], 0.5 * sd1["transformer.proj_out.diff_b"] - 1.25 * sd2["proj_out.diff_b"])


def test_file_by_path_equals_its_dict(tmp_path):
    from safetensors.torch import save_file

    sd, _ = make_peft_lora()
    sd = {k: v.float().contiguous() for k, v in sd.items()}
    path = tmp_path / "lora.safetensors"
    save_file(sd, str(path))
    model = _model()
    a = lora_flux.to_engine_lora(lora_flux.load_state_dict(path), model)  # os.PathLike
    b = lora_flux.to_engine_lora(lora_flux.load_state_dict(str(path)), model)
    c = lora_flux.to_engine_lora(sd, model)
    assert a.keys() == b.keys() == c.keys()
    for k in c:
        for x, y, z in zip(*[(d[k],) if torch.is_tensor(d[k]) else d[k] for d in (a, b, c)]):
            assert torch.equal(x, z) and torch.equal(y, z), k


def test_model_entry_point_by_path_merges_dense_layers_and_resets(tmp_path):
    """update_lora_params(path) on the CPU reaches the unquantised layers (merged) and the AWQ modulation layers (factors kept in kernel layout, ranks
    padded to 16); the W4A4 layers need the GPU for their layout and are left out of this file (tests/test_gpu_lora.py covers them)."""
    from safetensors.torch import save_file

    sd, dw = make_peft_lora()
    keep = ("x_embedder", "proj_out", "transformer_blocks.0.norm1.linear", "single_transformer_blocks.0.norm.linear")
    sd = {k: v.float().contiguous() for k, v in sd.items()
          if k[len("transformer."):].rsplit(".lora_", 1)[0] in keep or k == "transformer.proj_out.diff_b"}
    path = tmp_path / "dense.safetensors"
    save_file(sd, str(path))
    model = _model()
    with torch.no_grad():
        for p in (model.x_embedder.weight, model.proj_out.weight, model.proj_out.bias):
            p.copy_(torch.randn(p.shape))
    w0, b0 = model.x_embedder.weight.data.clone(), model.proj_out.bias.data.clone()
    model.update_lora_params(str(path), strength=0.5)
    want = (w0.float() + 0.5 * dw["x_embedder"].float()).to(w0.dtype)
    assert torch.equal(model.x_embedder.weight.data, want)
    assert torch.equal(model.proj_out.bias.data, (b0.float() + 0.5 * sd["transformer.proj_out.diff_b"]).to(b0.dtype))
    mod = model.transformer_blocks[0].norm1.linear
    assert mod._lora is not None and mod._lora.down.shape == (16, DIM) and mod._lora.up.shape == (6 * DIM, 16) and mod._lora.strength == 0.5
    assert not mod._lora.down[4:].any() and torch.equal(mod._lora.up[:, :4].double(), sd["transformer.transformer_blocks.0.norm1.linear.lora_B.weight"].double())
    assert model.single_transformer_blocks[0].norm.linear._lora.rank == 16 and model.transformer_blocks[0].norm1_context.linear._lora is None
    model.set_lora_strength(-2.0)
    assert torch.equal(model.x_embedder.weight.data, (w0.float() - 2.0 * dw["x_embedder"].float()).to(w0.dtype)) and mod._lora.strength == -2.0
    model.reset_lora()
    assert torch.equal(model.x_embedder.weight.data, w0) and torch.equal(model.proj_out.bias.data, b0) and mod._lora is None
    # the per-layer form keeps working
    model.update_lora_params({"x_embedder": (sd["transformer.x_embedder.lora_A.weight"], sd["transformer.x_embedder.lora_B.weight"])})
    assert torch.equal(model.x_embedder.weight.data, (w0.float() + dw["x_embedder"].float()).to(w0.dtype))
    model.reset_lora()


def test_unsupported_and_unknown_keys():
    model = _model()
    z = torch.zeros(4, 4)
    for sd in ({"transformer_blocks.0.attn.to_qkv.lora_down": z}, {"transformer_blocks.0.mlp_fc1.lora_up": z}, {"x.qweight": z}):
        with pytest.raises(NotImplementedError, match="diffusers / PEFT"):
            lora_flux.to_engine_lora(sd, model)
        with pytest.raises(NotImplementedError, match="diffusers / PEFT"):
            model.update_lora_params(sd)
    with pytest.raises(KeyError, match="to_q.lora_C"):
        lora_flux.to_engine_lora({"transformer_blocks.0.attn.to_q.lora_A.weight": torch.zeros(4, DIM), "transformer_blocks.0.attn.to_q.lora_C.weight": z}, model)
    with pytest.raises(KeyError, match="transformer_blocks.7"):
        model.update_lora_params({"transformer_blocks.7.attn.to_q.lora_A.weight": torch.zeros(4, DIM), "transformer_blocks.7.attn.to_q.lora_B.weight": torch.zeros(DIM, 4)})
    with pytest.raises(KeyError):
        model.update_lora_params({"no.such.module": (z, z)})


def test_total_rank_limits():
    model = _model()  # checkpoint rank 32: a fused QKV at LoRA rank r runs at 32 + 3 * pad16(r)
    ok = {f"transformer_blocks.0.attn.{p}.lora_{ab}.weight": torch.zeros((48, DIM) if ab == "A" else (DIM, 48)) for p in ("to_q", "to_k", "to_v") for ab in "AB"}
    assert lora_flux.to_engine_lora(ok, model)["transformer_blocks.0.attn.to_qkv"][0].shape[0] == 144  # 32 + 144 = 176
    bad = {f"transformer_blocks.0.attn.{p}.lora_{ab}.weight": torch.zeros((49, DIM) if ab == "A" else (DIM, 49)) for p in ("to_q", "to_k", "to_v") for ab in "AB"}
    with pytest.raises(ValueError, match=r"32 \+ 160 = 192.*176"):
        lora_flux.to_engine_lora(bad, model)
    mod = {"transformer_blocks.0.norm1.linear.lora_A.weight": torch.zeros(129, DIM), "transformer_blocks.0.norm1.linear.lora_B.weight": torch.zeros(6 * DIM, 129)}
    with pytest.raises(ValueError, match="128"):
        lora_flux.to_engine_lora(mod, model)
    lin = model.transformer_blocks[0].norm1.linear
    with pytest.raises(ValueError, match="128"):
        lin.set_lora(torch.zeros(129, DIM), torch.zeros(6 * DIM, 129))
    lin._offloaded = True
    with pytest.raises(RuntimeError, match="host memory"):
        lin.set_lora(torch.zeros(4, DIM), torch.zeros(6 * DIM, 4))


def test_nunchaku_package_reexports():
    import nunchaku.lora.flux as shim

    assert shim.to_engine_lora is lora_flux.to_engine_lora and shim.compose_lora is lora_flux.compose_lora


def test_gemv_lora_args_layout_matches_header(built_lib, tmp_path):
    cls = _lib.GemvLoraArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "svdq_amd.h")}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(svdq_gemv_lora_args));']
    for f, _ in cls._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(svdq_gemv_lora_args, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "lora_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "lora_layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def test_gemv_lora_validation_returns_codes(built_lib):
    lib = _lib.load()
    assert lib.svdq_abi_version() == 24
    assert lib.svdq_gemv_awq_lora_batched(None, 1, None) == 1

    def args(r=16, N=384, K=256):
        a = _lib.GemvLoraArgs()
        a.x = a.down = a.up = a.out = a.t = 1 << 20  # never dereferenced: validation fails first
        a.strength, a.r, a.N, a.K, a.dtype, a.out_chunks = 1.0, r, N, K, _lib.SVDQ_BF16, 6
        return a

    for r in (24, 0, 144):
        a = args(r=r)
        assert lib.svdq_gemv_awq_lora_batched(C.byref(a), 1, None) == 1 and b"multiple of 16" in lib.svdq_last_error()
    a = args(N=100)
    assert lib.svdq_gemv_awq_lora_batched(C.byref(a), 1, None) == 1 and b"out_chunks" in lib.svdq_last_error()
    a = args()
    assert lib.svdq_gemv_awq_lora_batched(C.byref(a), 81, None) == 1 and b"count" in lib.svdq_last_error()
