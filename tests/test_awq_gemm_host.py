"""Host side of the AWQ W4A16 GEMM (group 128) and of the 4-bit T5 encoder: the tinychat packer against fixtures from the
reference's own converter, W4Linear's state-dict spec, the C ABI struct and its validation (no launch), and the encoder's
checkpoint round trip on CPU (no forward)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from nunchaku_amd import _lib
from nunchaku_amd.models.text_encoders import W4Linear, ceil_num_groups, convert_to_tinychat_w4x16y16_linear_weight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _fixture(name):
    d = np.load(os.path.join(GOLDEN, name))
    return {k: d[k] for k in d.files}


def _bf16(u16: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(u16.astype(np.uint16).view(np.int16)).view(torch.bfloat16)


@pytest.mark.parametrize("name", ["awq128_64x640.npz", "awq128_256x1024.npz"])
def test_packer_reproduces_reference_converter(name):
    g = _fixture(name)
    N, K = g["codes"].shape
    G = K // 128
    scale, zero = torch.from_numpy(g["scale"]).bfloat16(), torch.from_numpy(g["zero"]).bfloat16()
    w = (torch.from_numpy(g["codes"].astype(np.float32)).view(N, G, 128) * scale.float().view(N, G, 1) - zero.float().view(N, G, 1)).view(N, K).bfloat16()
    qw, sc, zr = convert_to_tinychat_w4x16y16_linear_weight(w, scale, zero, group_size=128)
    assert qw.dtype == torch.int16 and torch.equal(qw, torch.from_numpy(g["qweight"]))
    assert sc.shape == (int(g["ceil_num_groups"]), N)
    # bit for bit, the zero padding rows (K = 640: 5 groups padded to 8) included
    assert torch.equal(sc.view(torch.int16), _bf16(g["scales"]).view(torch.int16))
    assert torch.equal(zr.view(torch.int16), _bf16(g["scaled_zeros"]).view(torch.int16))


def test_ceil_num_groups_matches_reference_table():
    spec = json.load(open(os.path.join(GOLDEN, "awq128_w4linear_spec.json")))
    assert len(spec["ceil_num_groups"]) >= 20
    for k, g, want in spec["ceil_num_groups"]:
        assert ceil_num_groups(k, g, 4) == want, (k, g)
    with pytest.raises(NotImplementedError):
        ceil_num_groups(96 * 4, 96)


def test_w4linear_state_dict_matches_reference_spec():
    spec = json.load(open(os.path.join(GOLDEN, "awq128_w4linear_spec.json")))["W4Linear(640, 256, group_size=128, dtype=bfloat16)"]
    for bias in (False, True):
        m = W4Linear(640, 256, bias=bias, group_size=128, dtype=torch.bfloat16, device="cpu")
        got = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
        assert got == spec[f"bias={bias}"]
        assert m.weight_bits == 4 and m.interleave == 4 and m.weight.dtype == torch.bfloat16 and "weight" not in m.state_dict()


def test_from_linear_dequantises_to_its_own_grid():
    """W4Linear.from_linear (asymmetric min / max per group): restating w = q * scale + scaled_zero from the packed buffers gives back the
    grid weights the converter was handed, to one bf16 rounding"""
    torch.manual_seed(0)
    lin = torch.nn.Linear(640, 128, bias=True).bfloat16()
    q = W4Linear.from_linear(lin, group_size=128)
    w16 = dequantise(q.qweight, q.scales, q.scaled_zeros, 640)
    assert w16.shape == (128, 640)
    err = (w16.float() - lin.weight.float()).abs().max().item()
    assert err <= 0.6 * (q.scales[:5].float().max().item()) + 1e-3
    assert torch.equal(q.bias, lin.bias.data)


def unpack_codes(qweight: torch.Tensor, K: int) -> torch.Tensor:
    """[N/4, K] int16 (tinychat order) -> codes [N, K] (int64); an independent restatement of the layout"""
    w = qweight.to(torch.int32) & 0xFFFF
    n4 = w.shape[0]
    w = w.view(n4, K // 64, 4, 2, 8)  # [rg][chunk][row][half][j]
    nib = torch.stack([(w >> (4 * e)) & 15 for e in range(4)], dim=4)  # [rg][chunk][row][half][e][j]: input 32 half + 8 e + j
    return nib.permute(0, 2, 1, 3, 4, 5).reshape(n4 * 4, K).long()


def dequantise(qweight, scales, zeros, K) -> torch.Tensor:
    """w16 = round16(q * scale + scaled_zero): the fma in float64 (exact), one rounding to the buffers' dtype (on the buffers' device)"""
    codes = unpack_codes(qweight, K).double()
    G = K // 128
    s = scales[:G].double().t().repeat_interleave(128, dim=1)
    z = zeros[:G].double().t().repeat_interleave(128, dim=1)
    return (codes * s + z).to(scales.dtype)


def test_unpack_restatement_inverts_the_fixture():
    g = _fixture("awq128_64x640.npz")
    assert torch.equal(unpack_codes(torch.from_numpy(g["qweight"]), 640), torch.from_numpy(g["codes"].astype(np.int64)))


def test_gemm_awq_args_layout_matches_header(built_lib, tmp_path):
    cls = _lib.GemmAwqArgs
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{os.path.join(ROOT, "include", "svdq_amd.h")}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(svdq_gemm_awq_args));']
    for f, _ in cls._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(svdq_gemm_awq_args, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "awq_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "awq_layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def _args(M=512, N=4096, K=4096, group=128):
    a = _lib.GemmAwqArgs()
    a.x = a.qweight = a.scales = a.scaled_zeros = a.out = 1 << 20  # never dereferenced: validation fails first
    a.M, a.N, a.K, a.ldx, a.group_size, a.dtype = M, N, K, K, group, _lib.SVDQ_BF16
    return a


def test_gemm_awq_validation_returns_codes(built_lib):
    lib = _lib.load()
    assert lib.svdq_gemm_awq(None, None) == 1
    a = _args(K=4160)
    assert lib.svdq_gemm_awq(C.byref(a), None) == 1 and b"multiple of 128" in lib.svdq_last_error()
    a = _args(group=64)
    assert lib.svdq_gemm_awq(C.byref(a), None) == 2 and b"group_size" in lib.svdq_last_error()
    a = _args(N=4096 + 32)
    assert lib.svdq_gemm_awq(C.byref(a), None) == 1 and b"multiple of 64" in lib.svdq_last_error()
    a = _args(M=0)
    assert lib.svdq_gemm_awq(C.byref(a), None) == 1
    # M = 8: 32 output tiles, the planner splits K = 4096 into 8 slices of fp32 partial tiles
    need = lib.svdq_gemm_awq_workspace_bytes(8, 4096, 4096)
    assert need == 8 * 8 * 4096 * 4
    a = _args(M=8)
    a.workspace, a.workspace_bytes = 1 << 20, need - 16
    assert lib.svdq_gemm_awq(C.byref(a), None) == 1 and b"workspace" in lib.svdq_last_error()
    # a launch that fills the chip without a split needs none
    assert lib.svdq_gemm_awq_workspace_bytes(1024, 4096, 4096) == 0
    assert lib.svdq_gemm_awq_workspace_bytes(512, 4096, 4096) == 2 * 512 * 4096 * 4


def test_ops_gemm_awq_rejects_cpu_tensors_and_bad_shapes():
    from nunchaku_amd._C import ops

    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    qw = torch.zeros(16, 256, dtype=torch.int16)
    sc = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gemm_awq(x, qw, sc, sc)
    with pytest.raises(ValueError):
        ops.gemm_awq(x, torch.zeros(16, 128, dtype=torch.int16), sc, sc)
    with pytest.raises(ValueError):
        ops.gemm_awq(x.half(), qw, sc, sc)


@pytest.mark.parametrize("shape", [(4096, 4096), (4096, 10240), (10240, 4096)])
def test_w4linear_bytes_at_t5_xxl_shapes(shape):
    K, N = shape
    m = W4Linear(K, N, bias=False, group_size=128, dtype=torch.bfloat16, device="meta")
    nbytes = sum(b.numel() * b.element_size() for b in m.buffers())
    assert m.scales.shape[0] == K // 128  # no padding rows at these K
    assert nbytes <= 0.27 * (N * K * 2)
    assert nbytes == N * K // 2 + 2 * (K // 128) * N * 2


# ---- the encoder: a tiny random T5 checkpoint written the way the quantised T5 files are (safetensors + 'config' metadata) ------------------

TINY_T5 = dict(vocab_size=128, d_model=256, d_kv=64, d_ff=640, num_layers=2, num_heads=4, feed_forward_proj="gated-gelu",
               relative_attention_num_buckets=32, relative_attention_max_distance=128, dropout_rate=0.0, is_encoder_decoder=False,
               use_cache=False)


def write_tiny_t5_checkpoint(path, dtype=torch.bfloat16, seed=0):
    """A random T5 encoder with every nn.Linear quantised by W4Linear.from_linear (group 128); returns (path, dense model whose linear weights
    are the dequantised w16, names of the quantised linears)"""
    transformers = pytest.importorskip("transformers")
    from safetensors.torch import save_file

    torch.manual_seed(seed)
    cfg = transformers.T5Config(**TINY_T5)
    dense = transformers.T5EncoderModel(cfg).to(dtype).eval()
    with torch.no_grad():
        for p in dense.parameters():  # T5's init scales some weights to ~1e-3 of the others: keep all of them O(1 / sqrt(fan_in))
            p.copy_(torch.randn_like(p.float()).mul(0.05).to(dtype))
    state, quantised = {}, []
    for name, mod in dense.named_modules():
        if isinstance(mod, torch.nn.Linear):
            q = W4Linear.from_linear(mod, group_size=128)
            for k, v in q.state_dict().items():
                state[f"{name}.{k}"] = v.contiguous()
            with torch.no_grad():
                mod.weight.copy_(dequantise(q.qweight, q.scales, q.scaled_zeros, mod.in_features))
            quantised.append(name)
    for k, v in dense.state_dict().items():
        if k.rsplit(".", 1)[0] not in quantised:
            state[k] = v.clone().contiguous()
    save_file(state, str(path), metadata={"config": json.dumps(cfg.to_dict())})
    return path, dense, quantised


def test_t5_encoder_loads_tiny_checkpoint_strictly(tmp_path):
    pytest.importorskip("transformers")
    from nunchaku import NunchakuT5EncoderModel

    path, dense, quantised = write_tiny_t5_checkpoint(tmp_path / "t5.safetensors")
    model = NunchakuT5EncoderModel.from_pretrained(str(path), device="cpu")
    swapped = sorted(n for n, m in model.named_modules() if isinstance(m, W4Linear))
    assert swapped == sorted(quantised) and len(swapped) == 2 * (4 + 3)  # q, k, v, o + wi_0, wi_1, wo per layer
    assert not any(isinstance(m, torch.nn.Linear) for m in model.modules())
    wo = model.encoder.block[0].layer[1].DenseReluDense.wo
    assert wo.scales.shape == (8, 256) and wo.weight.dtype == torch.bfloat16  # d_ff = 640: 5 groups padded to 8
    sd = model.state_dict()
    assert torch.equal(sd["encoder.final_layer_norm.weight"], dense.state_dict()["encoder.final_layer_norm.weight"])
    with pytest.raises(FileNotFoundError):
        NunchakuT5EncoderModel.from_pretrained("google/t5-v1_1-xxl", device="cpu")


def test_import_nunchaku_does_not_import_transformers():
    code = "import sys, nunchaku, nunchaku.models.text_encoders; assert 'transformers' not in sys.modules, 'transformers imported eagerly'"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")
def test_gemm_awq_kernel_resources(built_lib):
    """gemm_awq_kernel<DT, BM>: no scratch; the 128-row tile fits two workgroups per CU (<= 256 VGPRs, 2 x 68 KB of LDS); 32 MFMAs per K-step
    and wave at BM = 128, a quarter of that at BM = 32 (one 32 x 32 tile per wave)"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    res = mod.kernel_resources(_lib.lib_path(), "gemm_awq")
    assert len(res) == 8, sorted(res)  # bf16 / fp16 x BM 32, 64, 128 + the two reduction kernels
    for name, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 256 and r["group_segment_fixed_size"] <= 69632, (name, r)
    funcs = mod.disassemble(_lib.lib_path())
    mfma = {n: sum(1 for ln in ins if ln.startswith("v_mfma_f32_32x32x16")) for n, ins in funcs.items() if "gemm_awq_kernel" in n}
    assert len(mfma) == 6
    for n, c in mfma.items():
        assert c == (32 if "Li128E" in n else 16 if "Li64E" in n else 8), (n, c)
