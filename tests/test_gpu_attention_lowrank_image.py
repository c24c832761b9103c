"""The attention epilogue's fused quantiser at rank 16 / 32 on the fragment image of its low-rank factor (``svdq_pack_lora_down`` at one rank block,
``svdq_attention_args.qlora_down_packed(2)``): the factor is requested once per task as lane-contiguous 16-byte loads instead of row-per-lane 8-byte
loads per row tile, and the normalised rows are rounded once for both the low-rank MFMAs and the quantiser.  A pure re-layout: codes and scales stay
bit-equal to a separate quantiser launch on the kernel's own 16-bit output, ``lora_act`` is bit-equal with and without the image at the deterministic
level ``strict`` and within the quantiser rows' bound of tests/test_gpu_hot_instantiations.py, ``2e-5 (|x'| @ |D|) + 1e-6`` per element, otherwise.

fp16: the bound only holds because the low-rank MFMAs read the 16-bit output itself.  Until this file existed the pass formed its A operand as
``(T)(o * inv)``, which the fp16 build compiled to a multiply and a packed conversion -- a second rounding, one fp16 step from the stored output on
~1e-4 of the elements: ``worst err / bound = 1.25`` at L = 256, H = 2, rank 32.  Both operand paths now round once (``pack2_scaled``), so fp16
``lora_act`` moved in its last bits against earlier builds; bf16 did not.

Shapes are the smallest at which this code can go wrong: L = 256 is one task per head and four KV tiles (the shortest run of the generated loop: first
tile, one loop pair, last tile), L = 512 two tasks; H = 3 makes K = 384 (no multiple of 256: the image's own shape rule, whole heads); rank 16 is the
zero-padded image.  The CPU tests restate the layout in numpy and run the host-side size / validation code under the host sanitizers as a stand-alone
program (nothing is loaded into Python under a sanitizer)."""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests.helpers import TORCH_DT, f32, make_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the image layout, restated: [N / 16 units][nb rank blocks][64 lanes][8]; lane (rank & 31, h), slot j <- column 16 unit + 8 (j >> 2) + 4 h + (j & 3) ----
def pack_image_np(ld: np.ndarray) -> np.ndarray:
    """rank-major [R][N] 16-bit patterns -> the image (ranks >= R: zeros)"""
    R, N = ld.shape
    nb = (R + 31) // 32
    img = np.zeros((N // 16, nb, 64, 8), dtype=ld.dtype)
    unit, b, lane, j = np.meshgrid(np.arange(N // 16), np.arange(nb), np.arange(64), np.arange(8), indexing="ij")
    rank = 32 * b + (lane & 31)
    col = 16 * unit + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)
    live = rank < R
    img[live] = ld[rank[live], col[live]]
    return img


def unpack_image_np(img: np.ndarray, R: int) -> np.ndarray:
    units, nb = img.shape[:2]
    ld = np.zeros((R, units * 16), dtype=img.dtype)
    unit, b, lane, j = np.meshgrid(np.arange(units), np.arange(nb), np.arange(64), np.arange(8), indexing="ij")
    rank = 32 * b + (lane & 31)
    col = 16 * unit + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)
    live = rank < R
    ld[rank[live], col[live]] = img[live]
    return ld


@pytest.mark.parametrize("N", [256, 3072])
@pytest.mark.parametrize("R", [16, 32])
def test_image_is_a_permutation_and_holds_what_the_row_loads_fetch(R, N):
    """Pack then unpack is the identity, and fragment (head, step, lane) holds exactly the eight values the epilogue's two 8-byte loads fetch without the
    image (finish_rows' lowrank_pass: rank row ``lr``, columns ``head * 128 + dt * 32 + qq * 16 + h * 4 + (0 .. 3)`` and the same ``+ 8``; lanes with
    ``lr >= R`` feed zeros)."""
    rng = np.random.default_rng(R + N)
    ld = rng.integers(1, 65536, size=(R, N), dtype=np.uint16)
    img = pack_image_np(ld)
    assert img.shape == (N // 16, 1, 64, 8) and img.nbytes == (N // 16) * 1024
    assert np.array_equal(unpack_image_np(img, R), ld)
    assert np.count_nonzero(img) == R * N
    flat = ld.reshape(-1)
    for head in range(N // 128):
        for step in range(8):
            dt, qq = step >> 1, step & 1
            for lane in range(64):
                lr, h = lane & 31, lane >> 5
                if lr < R:
                    src = lr * N + head * 128 + dt * 32 + qq * 16 + h * 4  # `ld + (rank0 + lr) * K + dt * 32 + qq * 16 + h * 4`, ld offset by head * 128
                    want = np.concatenate([flat[src:src + 4], flat[src + 8:src + 12]])  # w0, w1 -> wv[0 .. 3], wv[4 .. 7]
                else:
                    want = np.zeros(8, dtype=np.uint16)
                assert np.array_equal(img[head * 8 + step, 0, lane], want), (head, step, lane)


def test_host_side_sizes_and_validation_under_the_host_sanitizers(tmp_path):
    """tools/lowrank_image_host_check.cpp (a stand-alone program over nunchaku_amd/csrc/lowrank_image_host.h, the header svdq_pack_lora_down and its
    ``_bytes`` query are built from) with AddressSanitizer and UBSan: sizes, argument validation, index arithmetic within the queried size."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lowrank_image_host_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "lowrank_image_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr


# =================================================================== GPU ===================================================================
@pytest.fixture
def gpu(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from nunchaku_amd._C import _Ops

    saved = (_Ops.attention_geometry, _Ops.attention_use_workspace, _Ops.attention_lowrank_image)
    yield _Ops
    _Ops.attention_geometry, _Ops.attention_use_workspace, _Ops.attention_lowrank_image = saved


_LAYERS = {}


def _layer(K, R, seed, dtype):
    """(oracle layer, module): computed once per shape and shared, never modified"""
    key = (K, R, seed, dtype)
    if key not in _LAYERS:
        lay = O.make_svdq_layer(K, 128, R, seed=seed, dtype=dtype, cheap=True)
        _LAYERS[key] = (lay, make_module(lay, dtype))
    return _LAYERS[key]


def _inputs(L, H, dtype, prescaled, seed=3):
    from nunchaku_amd.ops.attention import q_prescale

    td = TORCH_DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(seed + L + H)
    qkv = torch.randn(L, 3 * H * 128, device="cuda", generator=g).to(td)
    if prescaled:
        qkv[:, : H * 128] = (qkv[:, : H * 128].float() * q_prescale(128)).to(td)
    return qkv, qkv[:, 2 * H * 128:].t().contiguous()


def _image_of(lin):
    """the cached fragment image of the module's low-rank factor (None: no launch has built one)"""
    from nunchaku_amd import _C

    per = _C._epilogue_images.get(lin.proj_down) or {}
    hits = [v[1] for k, v in per.items() if k[0] == "frag_down"]
    return hits[0] if hits else None


def _fused(qkv, vt, H, lin, lin_first=None, **kw):
    from nunchaku_amd.ops.attention import attention_packed_quantized

    got = attention_packed_quantized(qkv, vt, H, lin, lin_first=lin_first, split_rows=256 if lin_first is not None else 0, **kw)
    assert got is not None
    return got


def _check_against_separate_quantiser(got, o, streams, dtype):
    """streams: [(row0, row1, oracle layer, module)].  Codes and scales bit-equal to module.quantize(o rows); lora_act within 2e-5 (|o| @ |D|) + 1e-6 of the
    float64 product of the kernel's own 16-bit output with the factor."""
    from nunchaku_amd import layout, mode

    K = o.shape[1]
    la = f32(mode.lora_act_to_float(got[2]) if got[2].dtype == torch.int64 else got[2]).astype(np.float64)
    codes, scales = layout.unpack_act(got[0], K), layout.unpack_scales(got[1], o.shape[0])
    for r0, r1, lay, lin in streams:
        ref = lin.quantize(o[r0:r1])
        assert torch.equal(codes[r0:r1], layout.unpack_act(ref[0], K)), f"rows {r0} .. {r1}: codes differ from a separate quantiser launch"
        assert torch.equal(scales[:, r0:r1], layout.unpack_scales(ref[1], r1 - r0)), f"rows {r0} .. {r1}: scales differ from a separate quantiser launch"
        x = f32(o[r0:r1]).astype(np.float64)
        D = np.asarray(lay["proj_down"], dtype=np.float64)  # [K][R]
        bound = 2e-5 * (np.abs(x) @ np.abs(D)) + 1e-6
        err = np.abs(la[r0:r1] - x @ D)
        print(f"lora_act rows {r0} .. {r1}: worst err / bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound), f"lora_act rows {r0} .. {r1}: worst err / bound = {(err / bound).max():.2f}"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("R", [32, 16])
@pytest.mark.parametrize("H", [2, 3])
@pytest.mark.parametrize("L", [256, 512])
def test_fused_quantiser_on_the_image_matches_a_separate_quantiser_launch(gpu, L, H, R, dtype):
    """The 4 x 64 kernel on the plain grid (Q prescaled: the step's kernel) with the image: codes / scales bit-equal, lora_act within the quantiser rows'
    bound; the image the launch cached is the numpy restatement's."""
    from nunchaku_amd._C import ops
    from nunchaku_amd.ops.attention import attention_packed

    lay, lin = _layer(H * 128, R, 2, dtype)
    qkv, vt = _inputs(L, H, dtype, True)
    o = attention_packed(qkv, vt, H, q_prescaled=True)
    got = _fused(qkv, vt, H, lin, q_prescaled=True)
    plan = ops.attention_last_plan()
    assert plan["geometry"] == 2 and plan["persistent_groups"] == 0 and not plan["split_lowrank"], plan
    img = _image_of(lin)
    assert img is not None, "a rank <= 32 launch builds and caches the factor's fragment image"
    ld = lin.proj_down.detach().view(torch.int16).cpu().numpy().view(np.uint16).reshape(R, H * 128)  # kernel layout: the bytes are rank-major [R][K]
    assert np.array_equal(img.cpu().numpy().view(np.uint16).reshape(-1), pack_image_np(ld).reshape(-1)), "svdq_pack_lora_down at one rank block"
    _check_against_separate_quantiser(got, o, [(0, L, lay, lin)], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("R", [32, 16])
def test_image_and_row_loads_give_the_same_bits(gpu, R, dtype):
    """The same launch with and without the image at the deterministic level ``strict`` (Q31.32 integer atomics: no summation order): codes, scales and
    lora_act bit-equal -- the operand path is a pure re-layout, the MFMA chain per head is the same.  And the kernel reads the image, not the rows: with
    the cached image zeroed the low-rank sums are zero while codes and scales stay."""
    from nunchaku_amd import _C, mode

    L, H = 512, 3
    lay, lin = _layer(H * 128, R, 2, dtype)
    qkv, vt = _inputs(L, H, dtype, True)
    with mode.deterministic_mode("strict"):
        with_img = _fused(qkv, vt, H, lin, q_prescaled=True)
        gpu.attention_lowrank_image = False
        without = _fused(qkv, vt, H, lin, q_prescaled=True)
        gpu.attention_lowrank_image = True
        assert with_img[2].dtype == torch.int64 and with_img[2].any()
        for a, b, what in zip(with_img, without, ("codes", "scales", "lora_act")):
            assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} elements differ between the image and the row loads"
        img = _image_of(lin)
        keep = img.clone()
        try:
            img.zero_()
            zeroed = _fused(qkv, vt, H, lin, q_prescaled=True)
        finally:
            img.copy_(keep)
        assert not zeroed[2].any(), "the launch did not read the fragment image"
        assert torch.equal(zeroed[0], with_img[0]) and torch.equal(zeroed[1], with_img[1])
        assert torch.equal(_fused(qkv, vt, H, lin, q_prescaled=True)[2], with_img[2])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_two_streams_use_both_images_and_split_at_the_task_boundary(gpu, dtype):
    """L = 512, qsplit_rows = 256, different smooth / lora_down per stream: each stream's rows against its own module; zeroing ONE stream's cached image
    zeroes exactly that stream's rows of lora_act (the split sits at row 256, a whole task: wave-uniform)."""
    from nunchaku_amd import mode
    from nunchaku_amd.ops.attention import attention_packed

    L, H, R = 512, 2, 32
    (laya, la), (layb, lb) = _layer(H * 128, R, 1, dtype), _layer(H * 128, R, 2, dtype)
    qkv, vt = _inputs(L, H, dtype, True)
    o = attention_packed(qkv, vt, H, q_prescaled=True)
    got = _fused(qkv, vt, H, lb, lin_first=la, q_prescaled=True)
    assert _image_of(la) is not None and _image_of(lb) is not None
    _check_against_separate_quantiser(got, o, [(0, 256, laya, la), (256, 512, layb, lb)], dtype)
    with mode.deterministic_mode("strict"):
        full = _fused(qkv, vt, H, lb, lin_first=la, q_prescaled=True)[2]
        for lin, dead, live in ((la, slice(0, 256), slice(256, 512)), (lb, slice(256, 512), slice(0, 256))):
            img = _image_of(lin)
            keep = img.clone()
            try:
                img.zero_()
                part = _fused(qkv, vt, H, lb, lin_first=la, q_prescaled=True)[2]
            finally:
                img.copy_(keep)
            assert not part[dead].any() and torch.equal(part[live], full[live]), "each stream reads its own image, split at row 256"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kernel", ["geometry1-raw-q", "geometry1-persistent", "geometry2-persistent", "geometry2-key-mask"])
def test_the_other_kernels_that_share_the_epilogue(gpu, kernel, dtype):
    """finish_rows is shared: the 8-wave x 32-row kernel on a raw, unprescaled Q (plain grid and persistent schedule), the 4 x 64 kernel on its persistent
    schedule, and the masked 4 x 64 kernel with ``kv_len0`` no multiple of 64.  Same checks, and bit-equal to the row loads at ``strict``.
    (The fused quantiser needs L % 256 == 0 -- its rows are F6 chunks of 256-row tasks -- so the 4-wave workgroup of L = 384 never runs it: refused below.)"""
    from nunchaku_amd import mode
    from nunchaku_amd._C import ops
    from nunchaku_amd.ops.attention import attention_packed, attention_packed_quantized

    L, H, R = 512, 3, 32
    lay, lin = _layer(H * 128, R, 2, dtype)
    geometry, prescaled, ws, kv = {"geometry1-raw-q": (1, False, False, None), "geometry1-persistent": (1, False, True, None),
                                   "geometry2-persistent": (2, True, True, None), "geometry2-key-mask": (0, True, True, (200,))}[kernel]
    qkv, vt = _inputs(L, H, dtype, prescaled)
    gpu.attention_geometry, gpu.attention_use_workspace = geometry, ws
    o = attention_packed(qkv, vt, H, q_prescaled=prescaled, kv_valid=kv)
    got = _fused(qkv, vt, H, lin, q_prescaled=prescaled, kv_valid=kv)
    plan = ops.attention_last_plan()
    ops.attention_workspace_status()
    assert plan["geometry"] == (2 if kernel.startswith("geometry2") else 1), plan
    assert plan["masked_geometry2"] == (kv is not None), plan
    if kernel.endswith("persistent"):
        assert plan["persistent_groups"] > 0, plan
    _check_against_separate_quantiser(got, o, [(0, L, lay, lin)], dtype)
    with mode.deterministic_mode("strict"):
        a = _fused(qkv, vt, H, lin, q_prescaled=prescaled, kv_valid=kv)
        gpu.attention_lowrank_image = False
        b = _fused(qkv, vt, H, lin, q_prescaled=prescaled, kv_valid=kv)
    for x, y, what in zip(a, b, ("codes", "scales", "lora_act")):
        assert torch.equal(x, y), f"{what}: the image and the row loads differ"
    if kernel == "geometry1-raw-q":
        q384, vt384 = _inputs(384, H, dtype, False)
        assert attention_packed_quantized(q384, vt384, H, lin) is None


@pytest.mark.gpu
def test_cached_image_follows_writes_to_the_factor(gpu):
    """The image is cached per (storage, offset, shape, version) like the rank 48 .. 160 images: a ``copy_`` into the parameter (what an offload slot load and
    a weight broadcast do: the version moves) re-packs on the next launch, a write through ``.data`` needs ``_C.invalidate``; either way the launch after
    the write equals, bit for bit at ``strict``, the launch of a module that always held those weights.  Until invalidated, a ``.data`` write is not seen."""
    from nunchaku_amd import _C, mode

    L, H, R, dtype = 256, 2, 32, "bf16"
    lay_a = O.make_svdq_layer(H * 128, 128, R, seed=5, dtype=dtype, cheap=True)
    mine = make_module(lay_a, dtype)                   # this test's own module: it is written to
    _, other = _layer(H * 128, R, 2, dtype)
    qkv, vt = _inputs(L, H, dtype, True)
    with mode.deterministic_mode("strict"), torch.no_grad():
        first = _fused(qkv, vt, H, mine, q_prescaled=True)[2].clone()
        other._ensure_layout()
        keep = mine.proj_down.detach().clone()
        smooth_keep = mine.smooth_factor.detach().clone()
        mine.smooth_factor.copy_(other.smooth_factor)
        mine.proj_down.copy_(other.proj_down)          # version bump
        want = _fused(qkv, vt, H, other, q_prescaled=True)
        got = _fused(qkv, vt, H, mine, q_prescaled=True)
        for a, b in zip(got, want):
            assert torch.equal(a, b), "after copy_ the launch must read a fresh image"
        assert not torch.equal(got[2], first), "the write must change the low-rank sums (else the test shows nothing)"
        mine.smooth_factor.copy_(smooth_keep)
        mine.proj_down.data.copy_(keep)                # no version bump: the cache cannot see it
        stale = _fused(qkv, vt, H, mine, q_prescaled=True)[2]
        assert torch.equal(stale, got[2]), "a .data write without invalidate() is served the cached image (documented contract)"
        _C.invalidate(mine.proj_down)
        assert torch.equal(_fused(qkv, vt, H, mine, q_prescaled=True)[2], first)
