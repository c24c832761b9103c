"""GPU tests of the LoRA path: the low-rank branch of the AWQ GEMV (svdq_gemv_awq_lora_batched), AWQW4A16Linear.set_lora, and
update_lora_params(<diffusers / PEFT file>) on the tiny engine.

Kernel tolerance (the issue's).  The numpy twin below applies the kernel's three rounding points with float64 sums:
    t = round16(down @ x);  d = round16(strength * up @ t);  out = round16(out + d)
and the kernel's out is held to ONE 16-bit step of the twin's out, end to end (the twin's own t; nothing of the kernel's enters the
expectation).  t (the kernel's scratch) is held to one step of the twin's t as well.  The kernel forms its sums in fp64 and rounds once, so
on an MI355X every case is in fact bit-equal to the twin; with fp32 sums one element (fp16, N = 384, r = 128, where out and d nearly cancel)
was two steps of out off -- a d one step of d off -- which is why the kernel does not use them."""
import os

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests.helpers import TORCH_DT, assert_close_16, f32, t16

pytestmark = pytest.mark.gpu

K = 256


@pytest.fixture(autouse=True)
def _need_gpu(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def round16_f64(v: np.ndarray, dtype: str) -> np.ndarray:
    """float64 -> nearest 16-bit value (ties to even) in ONE rounding, as float64"""
    v = np.asarray(v, np.float64)
    if dtype == "fp16":
        return v.astype(np.float16).astype(np.float64)
    _, e = np.frexp(v)  # |v| = m * 2^e, m in [0.5, 1): 8 significant bits -> step 2^(e - 8)
    q = np.ldexp(1.0, e - 8)
    return np.round(v / q) * q  # np.round: half to even; the values here are far from bf16's subnormals and overflow


def step16(v: np.ndarray, dtype: str) -> np.ndarray:
    """the 16-bit spacing at |v|"""
    _, e = np.frexp(np.maximum(np.abs(v), 1e-30))
    return np.ldexp(1.0, e - 8) if dtype == "bf16" else np.ldexp(1.0, np.maximum(e - 1, -14) - 10)


def perm(n: int, c: int) -> np.ndarray:
    """position of logical output j in the GEMV's de-interleaved layout"""
    j = np.arange(n)
    return (j % c) * (n // c) + j // c if c > 1 else j


def twin_t(x, down, dtype):
    return round16_f64(down.astype(np.float64) @ x.astype(np.float64), dtype)


def twin_out(out0, t, up, strength, chunks, dtype):
    """(expected out, d in out's layout) from the 16-bit t"""
    d = round16_f64(np.float64(np.float32(strength)) * (up.astype(np.float64) @ t.astype(np.float64)), dtype)
    dp = np.empty_like(d)
    dp[perm(len(d), chunks)] = d
    return round16_f64(out0.astype(np.float64) + dp, dtype), dp


def _awq_layer(N, dtype, seed, chunks, fixture_codes=None):
    from nunchaku_amd.models.linear import AWQW4A16Linear

    rng = np.random.default_rng(seed)
    w = O.round16(rng.standard_normal((N, K)).astype(np.float32) * 0.05, dtype)
    q, s, z = O.awq_quantize_ref(w, dtype)
    if fixture_codes is not None:
        q = fixture_codes
    bias = O.round16(rng.standard_normal(N).astype(np.float32) * 0.1, dtype)
    lin = AWQW4A16Linear(K, N, torch_dtype=TORCH_DT[dtype], device="cuda")
    lin.load_state_dict({"qweight": torch.from_numpy(O.pack_awq_w4_ref(q)), "wscales": t16(s, dtype), "wzeros": t16(z, dtype), "bias": t16(bias, dtype)})
    lin.out_chunks = chunks
    return lin


def _factors(N, r, dtype, seed):
    rng = np.random.default_rng(seed)
    down = O.round16(rng.standard_normal((r, K)).astype(np.float32) / np.sqrt(K), dtype)
    up = O.round16(rng.standard_normal((N, r)).astype(np.float32) * (0.5 / np.sqrt(r)), dtype)
    return down, up


@pytest.fixture(scope="module")
def fixture_codes(golden_dir):
    """the 4-bit codes of tests/golden/qweight_256x384.npz as the [N = 384, K = 256] AWQ weight (codes 0 .. 15)"""
    logical = np.load(os.path.join(golden_dir, "qweight_256x384.npz"))["logical"]
    assert logical.shape == (256, 384)
    return np.ascontiguousarray((logical.T.astype(np.int16) & 15).astype(np.uint8))


@pytest.mark.parametrize("chunks", [1, 6])
@pytest.mark.parametrize("r", [16, 32, 128])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gemv_lora_kernel_matches_the_twin(dtype, r, chunks, fixture_codes):
    from nunchaku_amd.ops.gemv import awq_gemv_w4a16_batched

    # three layers of different N and rank with a LoRA and one without, in one batched launch (the LoRA launch covers the three)
    spec = [(384, r, chunks, 0.75), (768, {16: 48, 32: 128, 128: 16}[r], chunks, -1.5), (128, {16: 32, 32: 16, 128: 64}[r], 1, 0.3), (384, 0, chunks, 0.0)]
    layers = [_awq_layer(N, dtype, 10 + i, c, fixture_codes if i == 0 else None) for i, (N, _, c, _) in enumerate(spec)]
    x = O.round16(np.random.default_rng(5).standard_normal((1, K)).astype(np.float32), dtype)
    tx = t16(x, dtype)
    base = [o.clone() for o in awq_gemv_w4a16_batched(tx, layers)]
    facs = []
    for i, (lin, (N, rr, c, s)) in enumerate(zip(layers, spec)):
        facs.append(_factors(N, rr, dtype, 20 + i) if rr else None)
        if rr:
            lin.set_lora(t16(facs[-1][0], dtype), t16(facs[-1][1], dtype), strength=s)
    got = [o.clone() for o in awq_gemv_w4a16_batched(tx, layers)]
    again = awq_gemv_w4a16_batched(tx, layers)
    for lin, (N, rr, c, s), fac, b, g, g2 in zip(layers, spec, facs, base, got, again):
        assert torch.equal(g, g2), "two launches on the same inputs differ"
        if not rr:
            assert torch.equal(g, b), "an entry without a LoRA was touched"
            continue
        down, up = fac
        t_ref, t_got = twin_t(x[0], down, dtype), f32(lin._lora.t).astype(np.float64)
        assert (np.abs(t_got - t_ref) <= step16(t_ref, dtype)).all(), "t: more than one 16-bit step from the twin"
        exp, _ = twin_out(f32(b)[0], t_ref, up, s, c, dtype)  # the twin end to end, from its own t
        err = np.abs(f32(g)[0].astype(np.float64) - exp)
        print(f"gemv_lora {dtype} N={N} r={rr} chunks={c}: t off the twin: {int((t_got != t_ref).sum())} of {rr}; out off the twin: {int((err != 0).sum())} of {N}, "
              f"beyond one step: {int((err > step16(exp, dtype)).sum())}, worst {float((err / step16(exp, dtype)).max()):.2f} steps")
        assert (err <= step16(exp, dtype)).all(), f"N={N} r={rr}: more than one 16-bit step of out from the twin"
        assert not torch.equal(g, b)
    # strength 0: out bit-unchanged (the branch still runs)
    for lin in layers:
        if lin._lora is not None:
            lin.set_lora_strength(0.0)
    for o, b in zip(awq_gemv_w4a16_batched(tx, layers), base):
        assert torch.equal(o, b)


def test_gemv_lora_rejects_rank_24():
    from nunchaku_amd.ops.gemv import awq_gemv_lora_batched
    from types import SimpleNamespace

    x = torch.zeros(K, dtype=torch.bfloat16, device="cuda")
    lo = SimpleNamespace(down=torch.zeros(24, K, dtype=torch.bfloat16, device="cuda"), up=torch.zeros(384, 24, dtype=torch.bfloat16, device="cuda"),
                         t=torch.zeros(24, dtype=torch.bfloat16, device="cuda"), strength=1.0)
    out = torch.ones(384, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="multiple of 16"):  # SVDQ_E_INVALID
        awq_gemv_lora_batched(x, [(lo, out, 6)])
    assert bool((out == 1).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_layer_forward_equals_the_batched_path_and_reset_restores(dtype, fixture_codes):
    from nunchaku_amd.ops.gemv import awq_gemv_w4a16_batched

    lin = _awq_layer(384, dtype, 3, 6, fixture_codes)
    x = t16(np.random.default_rng(6).standard_normal((1, K)).astype(np.float32), dtype)
    y0 = lin(x).clone()
    down, up = _factors(384, 20, dtype, 7)  # rank 20: padded to 32 by set_lora
    lin.set_lora(t16(down, dtype), t16(up, dtype), strength=1.25)
    assert lin._lora.down.shape == (32, K) and lin._lora.up.shape == (384, 32)
    y1 = lin(x).clone()
    assert not torch.equal(y1, y0)
    assert torch.equal(y1, awq_gemv_w4a16_batched(x, [lin])[0])
    # the logical update, loosely (the exact statement is the kernel test's): y1 - y0 = strength * up @ (down @ x) in the GEMV's layout
    delta = np.zeros(384)
    delta[perm(384, 6)] = 1.25 * (up.astype(np.float64) @ (down.astype(np.float64) @ f32(x)[0].astype(np.float64)))
    assert np.abs((f32(y1)[0] - f32(y0)[0]) - delta).max() <= 0.02 * np.abs(delta).max() + 2.0 ** -7 * np.abs(f32(y0)).max()
    # several rows (the reference's M <= 8): row by row through the same kernel
    x3 = t16(np.random.default_rng(8).standard_normal((3, K)).astype(np.float32), dtype)
    y3 = lin(x3)
    for i in range(3):
        assert torch.equal(y3[i], lin(x3[i:i + 1])[0])
    lin.reset_lora()
    assert lin._lora is None and torch.equal(lin(x), y0)


def test_more_than_80_lora_entries_are_split_into_launches():
    """84 layers with a LoRA: the wrapper issues two calls (80 + 4 entries, SVDQ_GEMV_BATCH_MAX); every layer equals its own single-layer forward"""
    from nunchaku_amd.ops.gemv import awq_gemv_w4a16_batched

    dtype = "bf16"
    layers = []
    for i in range(84):
        lin = _awq_layer(*[(192, dtype, 40, 6), (64, dtype, 41, 1), (384, dtype, 42, 3)][i % 3])
        down, up = _factors(lin.out_features, 16 if i % 2 else 32, dtype, 50 + i)
        layers.append(lin.set_lora(t16(down, dtype), t16(up, dtype), strength=0.5 + 0.01 * i))
    x = t16(np.random.default_rng(9).standard_normal((1, K)).astype(np.float32), dtype)
    outs = awq_gemv_w4a16_batched(x, layers)
    for i in (0, 1, 41, 79, 80, 81, 83):  # both sides of the split
        assert torch.equal(outs[i], layers[i](x)), i
    layers[82].reset_lora()
    assert not torch.equal(outs[82], layers[82](x))


def _qwen(layers=2):
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    return NunchakuQwenImageTransformer2DModel(num_layers=layers, num_attention_heads=2, attention_head_dim=128, in_channels=64,
                                               out_channels=16, joint_attention_dim=128, rank=32, device="cuda").init_synthetic_(seed=5).eval()


def test_qwen_modulation_launches_take_the_lora_branch():
    """Qwen-Image: the batched modulation launch (layer stand-ins that carry ``_lora``) and the per-block launch (``add_lora_(..., out_chunks=6)``) add the
    same low-rank update, bit for bit; reset_lora restores the model."""
    from nunchaku_amd import mode

    g = torch.Generator(device="cuda").manual_seed(9)
    lat = torch.randn(1, 256, 64, device="cuda", generator=g).bfloat16()
    enc = torch.randn(1, 256, 128, device="cuda", generator=g).bfloat16()
    t = torch.tensor([0.6], device="cuda")
    model = _qwen(2)
    dim = model.inner_dim
    rng = torch.Generator().manual_seed(1)
    targets = [model.transformer_blocks[0].img_mod[1], model.transformer_blocks[1].txt_mod[1]]
    with torch.no_grad(), mode.deterministic_mode():
        ref = model(lat, enc, None, t, [(1, 16, 16)]).sample.clone()
        for lin in targets:
            lin.set_lora(torch.randn(8, dim, generator=rng) / dim ** 0.5, torch.randn(6 * dim, 8, generator=rng) * 0.2, strength=1.0)
        assert model.batched_mods
        y = model(lat, enc, None, t, [(1, 16, 16)]).sample.clone()
        assert bool(torch.isfinite(y.float()).all()) and not torch.equal(y, ref)
        model.batched_mods = False
        try:
            assert torch.equal(model(lat, enc, None, t, [(1, 16, 16)]).sample, y)
        finally:
            model.batched_mods = True
        for lin in targets:
            lin.reset_lora()
        assert torch.equal(model(lat, enc, None, t, [(1, 16, 16)]).sample, ref)


def test_offloaded_blocks_refuse_a_lora_on_their_awq_layers():
    """CPUOffloadManager: a LoRA on the modulation projection of a block that moves to host memory is dropped with a warning, set_lora on it raises until the
    offload is undone; a resident block's layer still takes one."""
    model = _qwen(3)
    dim = model.inner_dim
    down, up = torch.zeros(4, dim), torch.zeros(6 * dim, 4)
    last = model.transformer_blocks[2].img_mod[1]
    last.set_lora(down, up)
    with pytest.warns(RuntimeWarning, match="AWQW4A16Linear"):
        model.set_offload(True, num_blocks_on_gpu=1, num_slots=2)
    try:
        assert last._lora is None and last._offloaded
        with pytest.raises(RuntimeError, match="host memory"):
            last.set_lora(down, up)
        first = model.transformer_blocks[0].img_mod[1]
        assert not first._offloaded
        first.set_lora(down, up).reset_lora()
    finally:
        model.set_offload(False)
    assert not last._offloaded
    last.set_lora(down, up).reset_lora()


# ---- the model ------------------------------------------------------------------------------------------------------------------------------

DIM = 256


def _tiny():
    from nunchaku_amd.models.flux import FluxTransformerAMD

    return FluxTransformerAMD(num_layers=1, num_single_layers=1, dim=DIM, heads=2, in_channels=64, joint_attention_dim=128,
                              pooled_projection_dim=64, device="cuda").init_synthetic_(seed=0).eval()


def _inputs():
    side, t_txt = 16, 128
    g = torch.Generator(device="cuda").manual_seed(0)
    lat = torch.randn(1, side * side, 64, device="cuda", generator=g).bfloat16()
    enc = torch.randn(1, t_txt, 128, device="cuda", generator=g).bfloat16()
    pooled = torch.randn(1, 64, device="cuda", generator=g).bfloat16()
    img_ids = torch.zeros(side * side, 3, device="cuda")
    img_ids[:, 1] = torch.arange(side, device="cuda").repeat_interleave(side)
    img_ids[:, 2] = torch.arange(side, device="cuda").repeat(side)
    return lat, enc, pooled, torch.tensor([0.5], device="cuda"), img_ids, torch.zeros(t_txt, 3, device="cuda"), torch.tensor([3.5], device="cuda")


def _peft_lora(seed=0):
    """bf16-exact factors for a few layers of every kind; (PEFT dict, {module: (A, B_with_alpha)})"""
    g = torch.Generator().manual_seed(seed)
    J, S = "transformer_blocks.0", "single_transformer_blocks.0"
    shapes = {f"{J}.attn.to_q": (DIM, DIM, 4), f"{J}.attn.to_v": (DIM, DIM, 4),
              f"{J}.attn.add_q_proj": (DIM, DIM, 16), f"{J}.attn.add_k_proj": (DIM, DIM, 16), f"{J}.attn.add_v_proj": (DIM, DIM, 16),
              f"{J}.attn.to_out.0": (DIM, DIM, 4), f"{J}.ff.net.0.proj": (4 * DIM, DIM, 16), f"{J}.ff_context.net.2": (DIM, 4 * DIM, 4),
              f"{J}.norm1.linear": (6 * DIM, DIM, 4), f"{S}.norm.linear": (3 * DIM, DIM, 16),
              f"{S}.attn.to_q": (DIM, DIM, 4), f"{S}.attn.to_k": (DIM, DIM, 4), f"{S}.attn.to_v": (DIM, DIM, 4),
              f"{S}.proj_mlp": (4 * DIM, DIM, 4), f"{S}.proj_out": (DIM, 5 * DIM, 16), "x_embedder": (DIM, 64, 4)}
    sd, fac = {}, {}
    for name, (o, i, r) in shapes.items():
        A = (torch.randn(r, i, generator=g) / i ** 0.5).bfloat16().float()
        B = (torch.randn(o, r, generator=g) * (0.5 / r ** 0.5)).bfloat16().float()
        sd[f"transformer.{name}.lora_A.weight"], sd[f"transformer.{name}.lora_B.weight"] = A, B
        fac[name] = (A, B)
    sd[f"transformer.{J}.ff.net.0.proj.alpha"] = torch.tensor(8.0)  # alpha / r = 1/2: exact in bf16
    fac[f"{J}.ff.net.0.proj"] = (fac[f"{J}.ff.net.0.proj"][0], fac[f"{J}.ff.net.0.proj"][1] * 0.5)
    return sd, fac


def _attach_by_hand(model, fac, strength):
    """the same LoRA through the per-layer calls: fused factors built here, dense layers merged here"""
    J, S = "transformer_blocks.0", "single_transformer_blocks.0"
    jb, sb = model.transformer_blocks[0], model.single_transformer_blocks[0]

    def qkv(names):
        present = [(i, fac[n]) for i, n in enumerate(names) if n in fac]
        down = torch.cat([a for _, (a, _) in present])
        up = torch.zeros(3 * DIM, down.shape[0])
        r0 = 0
        for i, (a, b) in present:
            up[i * DIM:(i + 1) * DIM, r0:r0 + a.shape[0]] = b
            r0 += a.shape[0]
        return down, up

    jb.attn.to_qkv.set_lora(*qkv([f"{J}.attn.to_q", f"{J}.attn.to_k", f"{J}.attn.to_v"]), strength)
    jb.attn.add_qkv_proj.set_lora(*qkv([f"{J}.attn.add_q_proj", f"{J}.attn.add_k_proj", f"{J}.attn.add_v_proj"]), strength)
    jb.attn.to_out[0].set_lora(*fac[f"{J}.attn.to_out.0"], strength)
    jb.ff.net[0].proj.set_lora(*fac[f"{J}.ff.net.0.proj"], strength)
    jb.ff_context.net[2].set_lora(*fac[f"{J}.ff_context.net.2"], strength)
    jb.norm1.linear.set_lora(*fac[f"{J}.norm1.linear"], strength)
    sb.norm.linear.set_lora(*fac[f"{S}.norm.linear"], strength)
    sb.attn.to_qkv.set_lora(*qkv([f"{S}.attn.to_q", f"{S}.attn.to_k", f"{S}.attn.to_v"]), strength)
    sb.mlp_fc1.set_lora(*fac[f"{S}.proj_mlp"], strength)
    A, B = fac[f"{S}.proj_out"]
    sb.attn.to_out.set_lora(A[:, :DIM], B, strength)
    sb.mlp_fc2.set_lora(A[:, DIM:], B, strength)
    A, B = fac["x_embedder"]
    w = model.x_embedder.weight
    w.data = (w.data.float() + strength * (B.cuda() @ A.cuda())).to(w.dtype)


def test_update_lora_params_from_a_peft_file(tmp_path):
    from safetensors.torch import save_file

    from nunchaku_amd import mode

    sd, fac = _peft_lora()
    path = tmp_path / "lora.safetensors"
    save_file({k: v.contiguous() for k, v in sd.items()}, str(path))
    model, args = _tiny(), _inputs()
    with torch.no_grad(), mode.deterministic_mode("strict"):
        y0 = model(*args).clone()
        assert torch.equal(model(*args), y0)  # the mode's promise, on which the comparisons below rest
        model.update_lora_params(str(path), strength=0.8)
        assert model.transformer_blocks[0].attn.to_qkv.rank == 32 + 16 and model.transformer_blocks[0].attn.add_qkv_proj.rank == 32 + 48
        assert model.transformer_blocks[0].norm1.linear._lora.strength == 0.8 and model.transformer_blocks[0].norm1_context.linear._lora is None
        y1 = model(*args).clone()
        assert bool(torch.isfinite(y1.float()).all()) and not torch.equal(y1, y0)
        model.set_lora_strength(0.0)  # the widened branches still run: the existing runtime-LoRA test's bound (tests/test_gpu_parity.py)
        assert_close_16(f32(model(*args)), f32(y0), "bf16", "strength 0", max_bad_frac=2e-3)
        model.reset_lora()
        assert torch.equal(model(*args), y0)
        hand = _tiny()
        assert torch.equal(hand(*args), y0)
        _attach_by_hand(hand, fac, 0.8)
        assert torch.equal(hand(*args), y1)
        # the state dict of the same file gives the same
        model.update_lora_params(sd, strength=0.8)
        assert torch.equal(model(*args), y1)
