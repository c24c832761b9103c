"""Every instantiation of the three kernels on the hot path -- the W4A4 GEMM (gemm_w4a4_kernel, gemm_w4a4_wt128_kernel, lowrank_down_split_kernel),
the activation quantiser (quantize_kernel, quantize_kernel_v2) and attention (attention_kernel, attention_kernel64) -- launched in both dtypes and
held to the oracle.  The case tables are module-level constants: tests/test_hot_ledger.py compares the instantiations they claim with the ones the
built library holds.

* GEMM and attention rows carry the key of the instantiation they claim, and every launch asserts that ``ops.gemm_last_plan()`` /
  ``ops.attention_last_plan()`` report that key: the claim is witnessed by the dispatch code itself.  (A GEMM key needs no launch to be read:
  ``svdq_gemm_plan`` answers from the same ``plan_gemm`` without a GPU, and tests/test_gemm_plan.py pins its answers there; here the key is
  read off the launch whose output is checked.)
* The quantiser's rows state their instantiation through ``quant_instantiation`` below, which asks ``svdq_quantize_plan``: the host function
  ``quantize_plan`` of csrc/quantize.hip, which ``launch_quantize`` consumes and beside which it decides nothing.  What
  remains restated here is the 4- / 8-wave choice of attention_kernel (``L % 256``), which the attention plan does not report: if the launcher changes
  that rule and the table is not changed with it, a row is counted for a kernel it no longer launches.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests.helpers import TORCH_DT, ULP16, assert_close_16, attn_softmax64, checked_codes, f32, make_module, t16

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "fp16")
STEP16 = {"bf16": 2.0 ** -7, "fp16": 2.0 ** -10}  # one 16-bit step, relative

# ---- the GEMM table -------------------------------------------------------------------------------------------------------------------
# (fuse, geometry, lora_act format, R, R2, M, K, N, workspace, key) with key = (tile rows, plan variant, fixed-point accumulators).
# How a key maps to gemm_w4a4_kernel<DT, FUSE, NW, LAQ, CARRY, RALL, HYB, SPLIT>: ``gemm_instantiations``.
FUSES = ("none", "silu", "gelu_quant", "rmsnorm_rope")  # SVDQ_FUSE_* 0 .. 3
M_SMALL = 300                                           # two 256-row blocks, the second ragged
ROWRUN_M, ROWRUN_K, ROWRUN_N = 1800, 128, 8192          # M_pad = 2048: (M_pad / 256) * (N / 128) = 512 = 2 * 256 CUs, the smallest shape with row runs


def _n(fuse, wide=False):
    return 768 if fuse == "rmsnorm_rope" else 1024 if wide else 512


def _r2(fuse, r2):
    return r2 if fuse == "gelu_quant" else 0


GEMM_CASES = tuple(
    # plain: every epilogue on both tile heights, fp32 and fixed-point low-rank accumulators, rank 32.  GELU_QUANT with an fp32 next-layer branch on 256-row
    # tiles is the carry kernel's, so that row has none (R2 = 0); the other three GELU_QUANT rows project down to rank 32 with per-tile atomics
    [(f, g, fmt, 32, _r2(f, 0 if (g, fmt) == (1, "f32") else 32), M_SMALL, 256, _n(f), True, (256 if g == 1 else 128, "plain", fmt != "f32"))
     for f in FUSES for g in (1, 3) for fmt in ("f32", "q32")]
    # all-rank: rank 64 with a workspace (256 rows: lora_up staged in LDS + packed lora_act_in; 128 rows: both packed).  GELU_QUANT: next rank 64 where
    # no row runs apply and (explicit geometry) no split: the per-tile atomics over two passes of 32 ranks
    + [(f, g, "f32", 64, _r2(f, 64), M_SMALL, 384, _n(f, True), True, (256 if g == 1 else 128, "all_rank", False)) for f in FUSES for g in (1, 3)]
    + [
        ("gelu_quant", 1, "f32", 32, 32, M_SMALL, 256, 512, True, (256, "carry", False)),            # four column tiles per row block: the carry sums
        ("gelu_quant", 1, "f32", 32, 16, M_SMALL, 256, 512, False, (256, "carry", False)),           # rank 16 (half the carry's lanes idle), no workspace
        ("gelu_quant", 1, "q32_runs", 32, 32, ROWRUN_M, ROWRUN_K, ROWRUN_N, True, (256, "carry", True)),
        ("gelu_quant", 1, "f32", 32, 48, ROWRUN_M, ROWRUN_K, ROWRUN_N, True, (256, "hybrid_carry", False)),
        ("gelu_quant", 1, "f32", 32, 80, ROWRUN_M, ROWRUN_K, ROWRUN_N, True, (256, "hybrid_carry", False)),
        ("gelu_quant", 6, "f32", 32, 48, M_SMALL, 256, 512, True, (128, "solo_carry", False)),
        ("gelu_quant", 6, "f32", 32, 128, M_SMALL, 256, 512, True, (128, "solo_carry", False)),
    ]
    # split down: the all-rank kernel stores 16-bit fragments, lowrank_down_split_kernel<DT, NB = ceil(R2 / 32)> contracts them: NB = 2, 3, 4, 5
    + [("gelu_quant", 7, "f32", 64, r2, M_SMALL, 256, 512, True, (256, "split_down", False)) for r2 in (64, 96, 128, 160)]
    + [("none", 8, "f32", r, 0, M_SMALL, 256, 512, True, (256, "wave_tile_128", False)) for r in (0, 32)]
)
DET_LEVEL = {"f32": False, "q32": "strict", "q32_runs": "runs"}

# Elements of a row of the 16-bit GELU output that the GPU (exp2 / rcp GELU, fp32 accumulation order of the pre-activation) rounds one 16-bit step away
# from the oracle's, by the row's width N: {(dtype, N): allowance} = twice the worst row measured on an MI355X (``test_gemm_case``'s docstring)
H_STEPS_ALLOWED = {("bf16", 512): 4, ("bf16", 1024): 16, ("bf16", 8192): 6, ("fp16", 512): 10, ("fp16", 1024): 22, ("fp16", 8192): 16}


def gemm_instantiations(case) -> set:
    """the template arguments behind a row's key, without DT: {(kernel, args)} (GemmPlan's switches, launch_variant of csrc/gemm_w4a4.hip)"""
    fuse, _, _, _, r2, *_, (rows, variant, laq) = case
    if variant == "wave_tile_128":
        return {("gemm_w4a4_wt128_kernel", ())}
    carry, rall, hyb, split = {"plain": (0, 0, 0, 0), "carry": (1, 0, 0, 0), "all_rank": (0, 1, 0, 0), "hybrid_carry": (1, 0, 1, 0), "solo_carry": (1, 0, 0, 0),
                               "split_down": (0, 1, 0, 1)}[variant]
    out = {("gemm_w4a4_kernel", (FUSES.index(fuse), 8 if rows == 256 else 4, int(laq), carry, rall, hyb, split))}
    if variant == "split_down":
        out.add(("lowrank_down_split_kernel", (math.ceil(r2 / 32),)))
    return out


# ---- the quantiser table --------------------------------------------------------------------------------------------------------------
# (R, smooth given, LayerNorm front end, fuse_glu, grouped second stream, lora_act format, M, K, pad_size)
QUANT_M, QUANT_K = 300, 384
LARGE_GRID = (600, 1152, 87552)     # 2736 row tiles x 3 slices > 8192: cpw = 8, two K slices (the atomics path of the general kernel), ~75 MB of outputs
BEYOND_8192_TILES = (300, 128, 262400)  # 8200 row tiles: the doubling of cpw used not to end here (csrc/quantize.hip, launch_quantize)
QUANT_CASES = tuple(
    # the fast path: all 12 of quantize_kernel_v2<DT, LORA, LN, SMOOTH, MULTI>
    [(R, sm, ln, False, False, "f32", QUANT_M, QUANT_K, 256) for R in (0, 32, 96) for sm in (False, True) for ln in (False, True)]
    # ... five of them again as the grouped launch (a second stream with its own input and parameter set behind 256 rows of the first), rank 96 with LayerNorm among them
    + [(R, sm, ln, False, True, "f32", QUANT_M, QUANT_K, 256) for R, sm, ln in ((96, True, True), (96, False, True), (96, True, False), (32, True, True), (0, True, False))]
    + [(R, True, False, False, False, "q32", QUANT_M, QUANT_K, 256) for R in (32, 96)]
    # fuse_glu: quantize_kernel<DT, RT32 = 0, 1, 2, 4, 8, 1, true>
    + [(R, True, False, True, False, "f32", QUANT_M, QUANT_K, 256) for R in (0, 32, 64, 128, 176)]
    # the general kernel without GLU: rank 176 at the small shape, ranks 0 .. 128 where the grid rule leaves the fast path (cpw = 8)
    + [(176, True, False, False, False, fmt, QUANT_M, QUANT_K, 256) for fmt in ("f32", "q32")]
    + [(R, True, False, False, False, "f32") + LARGE_GRID for R in (0, 32, 64, 128)]
    + [(64, True, False, False, False, "q32") + LARGE_GRID]
    + [(32, True, False, False, False, "f32") + BEYOND_8192_TILES]
)


def quant_plan(R, smooth, ln, glu, grouped, fmt, M, K, M_pad, ldx=None, ldx2=None) -> dict:
    """``svdq_quantize_plan`` for a launch of this shape: what ``launch_quantize`` consumes (csrc/quantize.hip, ``quantize_plan``), from the library itself, host
    only.  The addresses are made up (aligned, never dereferenced: the query validates and decides, nothing else).  ``grouped``: 256 rows of the first stream,
    the rest in a second one, as ``test_quantize_case`` launches it.  ``ldx`` / ``ldx2``: row strides of the inputs (default: contiguous)."""
    import ctypes as C

    from nunchaku_amd import _lib

    a, base = _lib.QuantizeArgs(), 1 << 20
    a.x, a.act, a.ascales = base, 2 * base, 3 * base
    a.smooth = 4 * base if smooth else None
    a.lora_down, a.lora_act = (5 * base, 6 * base) if R else (None, None)
    if ln:
        a.ln_stats, a.mod_scale, a.mod_shift = 7 * base, 8 * base, 9 * base
    a.M, a.M_pad, a.K, a.R = (256 if grouped else M), M_pad, K, R
    a.ldx = (2 * K if glu else K) if ldx is None else ldx
    a.fuse_glu = int(glu)
    a.lora_act_format = {"f32": _lib.LORA_ACT_F32, "q32": _lib.LORA_ACT_Q32}[fmt]
    if grouped:
        a.x2, a.M2, a.ldx2, a.split_rows = 10 * base, M - 256, (K if ldx2 is None else ldx2), 256
        a.smooth2 = 11 * base if smooth else None
        a.lora_down2 = 12 * base if R else None
        if ln:
            a.ln_stats2, a.mod_scale2, a.mod_shift2 = 13 * base, 14 * base, 15 * base
    out = (C.c_int32 * 8)()
    lib = _lib.load()
    rc = lib.svdq_quantize_plan(C.byref(a), out)
    assert rc == 0, (rc, lib.svdq_last_error().decode())
    return {"family": ("fast", "general")[out[0]], "sel": out[1], "cpw": out[2], "slices": out[3], "lora_act_add": out[4], "grid": out[5], "glu": bool(out[6]),
            "memset": bool(out[7])}


def quant_grid(M_pad: int, K: int):
    """(chunks per workgroup, K slices) of launch_quantize, as the library's plan states them (they depend on M_pad and K alone)"""
    pl = quant_plan(0, False, False, False, False, "f32", M_pad, K, M_pad)
    return pl["cpw"], pl["slices"]


def quant_instantiation(case):
    """The instantiation ``svdq_quantize_plan`` names for a row: ("quantize_kernel_v2", (LORA, LN, SMOOTH, MULTI)) for the fast family, its switch set spelt
    out; ("quantize_kernel", (RT32 class, 1, GLU)) for the general one"""
    R, smooth, ln, glu, grouped, fmt, M, K, pad = case
    pl = quant_plan(R, smooth, ln, glu, grouped, fmt, M, K, math.ceil(M / pad) * pad)
    sel = pl["sel"]
    if pl["family"] == "fast":
        return "quantize_kernel_v2", (sel >> 2 & 1, sel >> 1 & 1, sel & 1, sel >> 3 & 1)
    return "quantize_kernel", (sel, 1, int(pl["glu"]))


# ---- the attention table --------------------------------------------------------------------------------------------------------------
# (L, geometry, workspace, Q prescaled, kv_valid, key) with key = (kernel, template arguments without DT); H = 2
ATTN_H = 2
ATTN_CASES = (
    (384, 0, True, False, None, ("attention_kernel", (4, 0))),          # L % 256 != 0: the 4-wave kernel on the plain grid
    (512, 1, False, False, None, ("attention_kernel", (8, 0))),
    (512, 1, True, False, None, ("attention_kernel", (8, 1))),          # 4 tasks on 256 CUs: the persistent schedule splits them along the keys
    (512, 0, True, True, None, ("attention_kernel64", (0, 0))),         # automatic: a prescaled Q runs geometry 2 on the plain grid
    (512, 2, True, True, None, ("attention_kernel64", (1, 0))),         # explicit geometry 2 takes the workspace
    (512, 0, True, True, (300,), ("attention_kernel64", (0, 1))),       # key mask: four fully real 64-key tiles, one partly real, three padded
)


def attn_plan_key(L: int, plan: dict):
    """the instantiation a reported plan stands for (the 4- / 8-wave choice restated: csrc/attention.hip, ``nw = L % 256 == 0 ? 8 : 4``)"""
    if plan["geometry"] == 2:
        return "attention_kernel64", (int(plan["persistent_groups"] > 0), int(plan["masked_geometry2"]))
    return "attention_kernel", (8 if L % 256 == 0 else 4, int(plan["persistent_groups"] > 0))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nunchaku_amd import _lib

    _lib.load()


# =======================================================================================================================================
# 1. GEMM
# =======================================================================================================================================
@functools.lru_cache(maxsize=None)
def _layer(K, N, R, seed, dtype):
    return O.make_svdq_layer(K, N, R, seed=seed, dtype=dtype, cheap=True)


@functools.lru_cache(maxsize=None)
def _acts(M, K, seed, dtype):
    return O.make_activations(M, K, seed=seed, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _rope(M_pad, dtype):
    rng = np.random.default_rng(12)
    nq = O.round16((1 + 0.1 * rng.standard_normal(128)).astype(np.float32), dtype)
    nk = O.round16((1 + 0.1 * rng.standard_normal(128)).astype(np.float32), dtype)
    ang = rng.uniform(0, 6.28, (M_pad, 64)).astype(np.float32)
    return nq, nk, np.stack([np.sin(ang), np.cos(ang)], axis=-1).astype(np.float32)


def _sample_rows(M):
    """rows the oracle is run on: all of a small launch; of a large one both ends, every 256-row block edge region and a random handful"""
    if M <= 512:
        return None
    edge = [r for b in range(0, M, 256) for r in (b, b + 31, b + 128, b + 255) if r < M]
    return np.array(sorted(set(edge + [M - 1] + np.random.default_rng(0).integers(0, M, 24).tolist())))


class _GemmRun:
    """The operands of a table row on the GPU (quantised once), its launch, and the oracle's view of the operands the launch consumed."""

    def __init__(self, case, dtype):
        from nunchaku_amd import mode

        self.case, self.dtype = case, dtype
        fuse, self.geometry, fmt, R, R2, M, K, N, self.ws, self.key = case
        self.L1 = _layer(K, N, max(R, 16), 100 + K + N + R, dtype)  # (R = 0: a rank-16 layer launched without its low-rank branch)
        self.x = _acts(M, K, 7 + M + K, dtype)
        self.m1 = make_module(self.L1, dtype)
        self.m1._ensure_layout()
        self.M_pad = math.ceil(M / 256) * 256
        self.L2 = self.m2 = None
        if fuse == "gelu_quant":
            self.L2 = _layer(N, 128, max(R2, 16), 200 + N + R2, dtype)
            self.m2 = make_module(self.L2, dtype, act_unsigned=True)
            self.m2._ensure_layout()
        self.level = DET_LEVEL[fmt]
        with mode.deterministic_mode(self.level):
            self.qx, self.asc, self.la = self.m1.quantize(t16(self.x, dtype))
        assert self.la.dtype == (torch.float32 if fmt == "f32" else torch.int64)

    def launch(self, geometry=None, R=None):
        """-> (outputs, plan); outputs: (out,) or (qout, oscales, lora_act_out | None)"""
        from nunchaku_amd import layout, mode
        from nunchaku_amd._C import _Ops, ops
        from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda

        fuse, _, fmt, R0, R2, M, K, N, ws, _ = self.case
        R = R0 if R is None else R
        m1, m2, td, M_pad = self.m1, self.m2, TORCH_DT[self.dtype], self.M_pad
        kw = dict(act=self.qx, wgt=m1.qweight, ascales=self.asc, wscales=m1.wscales, bias=m1.bias)
        if R:
            kw.update(lora_act_in=self.la, lora_up=m1.proj_up)
        lh = None
        if fuse == "gelu_quant":
            qh = torch.empty(layout.act_image_shape(M_pad, N), dtype=torch.uint8, device="cuda")
            sh = torch.empty(N // 64, M_pad, dtype=td, device="cuda")
            kw.update(qout=qh, oscales=sh, smooth_factor=m2.smooth_factor)
            if R2:  # junk in the accumulators: the op has to clear them
                lh = torch.full((M_pad, R2), 3.0, dtype=torch.float32, device="cuda") if fmt == "f32" else torch.full((M_pad, R2), 12345, dtype=torch.int64, device="cuda")
                kw.update(lora_down=m2.proj_down, lora_act_out=lh)
            outs = (qh, sh, lh)
        else:
            out = torch.empty(M, N, dtype=td, device="cuda")
            kw.update(out=out, fuse_silu=fuse == "silu")
            if fuse == "rmsnorm_rope":
                nq, nk, rot = _rope(M_pad, self.dtype)
                kw.update(norm_q=t16(nq, self.dtype), norm_k=t16(nk, self.dtype), rotary_emb=torch.from_numpy(O.pack_rotemb_ref(rot)).cuda().view(M_pad, 128))
            outs = (out,)
        saved = (_Ops.gemm_geometry, _Ops.gemm_use_workspace)
        _Ops.gemm_geometry, _Ops.gemm_use_workspace = self.geometry if geometry is None else geometry, ws
        try:
            with mode.deterministic_mode(self.level):
                svdq_gemm_w4a4_cuda(**kw)
            plan = ops.gemm_last_plan()
        finally:
            _Ops.gemm_geometry, _Ops.gemm_use_workspace = saved
        return outs, plan

    def consumed(self, rows=None):
        """(codes, scales, lora_act) the launch read, as the oracle takes them -- the quantiser's codes checked against the oracle on the way"""
        from nunchaku_amd import mode

        q, a = checked_codes(self.qx, self.asc, self.x, self.L1["smooth"], self.dtype, rows=rows)
        la = mode.lora_act_to_float(self.la).cpu().numpy()
        return q, a, la if rows is None else la[rows]


def _plan_key(plan):
    return plan["tile_rows"], plan["variant"]


def _lora_act_out_bound(h, D, dtype, steps):
    """per element: the fp32-order term of test_quantize_codes_and_scales on the oracle's 16-bit GELU output ``h``, plus ``steps`` elements of the row one 16-bit
    step off, each worth at most max_k |h_k D_kr| (as test_quantize_fuse_glu builds it)"""
    big = np.max(np.abs(h)[:, :, None] * np.abs(D)[None, :, :], axis=1) if steps else 0.0
    return 2e-5 * (np.abs(h) @ np.abs(D)) + 1e-6 + steps * STEP16[dtype] * big


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: "-".join(str(v) for v in c[:9]))
def test_gemm_case(case, dtype):
    """One row of GEMM_CASES: the plan the library reports is the key the row claims; the output against the oracle on the operands the launch consumed, at
    the tolerances tests/test_gpu_parity.py uses for the epilogue (plain: 1 ulp; SiLU: 1 ulp but 2e-3 of the elements, 2 ulp all; RMSNorm + RoPE: V 1 ulp,
    Q / K 2 ulp but 2e-3; GELU_QUANT: codes +-1 on < 5e-3, scales one step on < 5e-3).

    GELU_QUANT with a next-layer branch: lora_act_out per element within ``_lora_act_out_bound`` -- not within 2e-3 of the largest sum, inside which a dropped
    column tile of a long run can hide -- after a second launch into the same buffer too (the carry left clean, the accumulators cleared); the fixed-point
    formats to the same bound and bit-equal between the two launches.  The bound's second term counts elements of the 16-bit GELU output one step away from
    the oracle's.  Measured on an MI355X against the oracle at this table's shapes, on the 16-bit image the split-down launch stores (rank 64 -> 64; all 300
    rows at N = 512 and 1024, the 54 sampled rows at N = 8192), differing elements in the worst row: bf16 2 / 8 / 3 at N = 512 / 1024 / 8192, fp16 5 / 11 / 8
    (mean per row 0.04 / 0.15 / 0.17 and 0.25 / 0.87 / 4.2; none further than one step of its own size, or, next to zero, 2^-10 absolute).
    ``H_STEPS_ALLOWED`` is twice that: 4 / 16 / 6 and 10 / 22 / 16."""
    from nunchaku_amd import layout, mode

    fuse, geometry, fmt, R, R2, M, K, N, ws, key = case
    run = _GemmRun(case, dtype)
    outs, plan = run.launch()
    assert _plan_key(plan) == key[:2], f"claimed {key}, launched {plan}"
    if key[1] in ("carry", "hybrid_carry") and M > 512:
        assert plan["rowrun"] > 0, plan
    rows = _sample_rows(M)
    q, a, la = run.consumed(rows)
    L1, L2 = run.L1, run.L2
    sel = slice(0, M) if rows is None else rows
    kw = dict(dtype=dtype, bias=L1["bias"])
    if R:
        kw.update(lora_act_in=la, lora_up=L1["proj_up"])
    if fuse == "rmsnorm_rope":
        nq, nk, rot = _rope(run.M_pad, dtype)
        kw.update(norm_q=nq, norm_k=nk, rot=rot)
    if fuse == "gelu_quant":
        kw.update(next_smooth=L2["smooth"], next_lora_down=L2["proj_down"] if R2 else None)
    ref = O.gemm_w4a4(q, a, L1["qweight"], L1["wscales"], fuse=fuse, **kw)
    if fuse != "gelu_quant":
        got = f32(outs[0])
        want = ref["out"][:M]
        if fuse == "none":
            assert_close_16(got, want, dtype, f"{case}")
        elif fuse == "silu":
            assert_close_16(got, want, dtype, "silu", max_bad_frac=2e-3, ulps=1.0)
            assert_close_16(got, want, dtype, "silu(2ulp)", ulps=2.0)
        else:
            assert_close_16(got[:, 2 * N // 3:], want[:, 2 * N // 3:], dtype, "V")
            assert_close_16(got[:, : 2 * N // 3], want[:, : 2 * N // 3], dtype, "QK", max_bad_frac=2e-3, ulps=2.0)
        return
    qh, sh, lh = outs
    codes = layout.unpack_act(qh, N, unsigned=True).cpu().numpy()[sel]
    want_codes = ref["qout"][:M] if rows is None else ref["qout"]
    diff = np.abs(codes.astype(int) - want_codes.astype(int))
    assert diff.max() <= 1 and (diff != 0).mean() < 5e-3, f"codes: {(diff != 0).mean():.2e} differ, max {diff.max()}"
    s_got = f32(layout.unpack_scales(sh, run.M_pad))[:, sel]
    s_ref = ref["oscales"][:, :M] if rows is None else ref["oscales"]
    assert (s_got != s_ref).mean() < 5e-3 and np.allclose(s_got, s_ref, rtol=2 ** -6), f"scales: {(s_got != s_ref).mean():.2e} differ"
    if not R2:
        return
    h = ref["g16"][:M] if rows is None else ref["g16"]
    la_ref = ref["lora_act_out"][:M] if rows is None else ref["lora_act_out"]
    bound = _lora_act_out_bound(h, L2["proj_down"], dtype, H_STEPS_ALLOWED[(dtype, N)])
    first = lh.clone()
    outs2, _ = run.launch()
    for name, t in (("first launch", first), ("second launch", outs2[2])):
        got = mode.lora_act_to_float(t).cpu().numpy()
        assert got.shape[1] == R2
        err = np.abs(got[sel].astype(np.float64) - la_ref)
        print(f"lora_act_out {name}: worst err / bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound), f"lora_act_out, {name}: worst err / bound = {(err / bound).max():.2f} at {np.unravel_index((err / bound).argmax(), err.shape)}"
    if fmt != "f32":
        assert torch.equal(first, outs2[2]), "fixed-point lora_act_out differs between two launches"
    assert torch.equal(qh, outs2[0]) and torch.equal(sh, outs2[1]), "codes and scales differ between two launches"


def _pairs(variant_a, variant_b):
    """table rows that differ in geometry alone (and, GELU_QUANT, in the next-layer rank, which the codes do not depend on)"""
    same = lambda a, b: a[0] == b[0] and a[2:4] == b[2:4] and a[5:9] == b[5:9]
    return [(a, b) for a in GEMM_CASES for b in GEMM_CASES if a[9][1] == variant_a and b[9][1] == variant_b and a[1] == 1 and b[1] != 1 and same(a, b)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_tile_heights_are_bit_equal(dtype):
    """include/svdq_amd.h: launches that are not split along K compute every output element with the same operations in the same order on 256 x 128 and on
    128 x 128 tiles.  K = 256 / 384 has too few K-steps for a split; the low-rank accumulators are an INPUT here (one quantiser run per pair), so their
    format does not matter.  Every plain and all-rank pair of the table, 16-bit outputs or codes and scales bit for bit."""
    pairs = _pairs("plain", "plain") + _pairs("all_rank", "all_rank")
    assert len(pairs) == 12
    for a, b in pairs:
        run = _GemmRun(a, dtype)
        (oa, pa), (ob, pb) = run.launch(), run.launch(geometry=b[1])
        assert (pa["tile_rows"], pb["tile_rows"]) == (256, 128) and pa["streamk_groups"] == pb["streamk_groups"] == 0, (pa, pb)
        for ta, tb in zip(oa[:2], ob[:2]):
            assert torch.equal(ta, tb), f"{a[:4]}: geometry {b[1]} vs 1: {(ta != tb).float().mean():.2e} of the elements differ"


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_wave_tile_is_bit_equal_to_the_8_wave_kernel(dtype):
    for case in GEMM_CASES:
        if case[9][1] == "wave_tile_128":
            run = _GemmRun(case, dtype)
            (o8, p8), (o1, p1) = run.launch(), run.launch(geometry=1)
            assert p8["variant"] == "wave_tile_128" and _plan_key(p1) == (256, "plain"), (p8, p1)
            assert torch.equal(o8[0], o1[0]), f"rank {case[3]}: geometry 8 vs 1: {(o8[0] != o1[0]).float().mean():.2e} of the elements differ"


# =======================================================================================================================================
# 2. quantiser
# =======================================================================================================================================
def _ln_params(K, dtype, seed):
    rng = np.random.default_rng(seed)
    return O.round16(1 + rng.standard_normal(K).astype(np.float32) * 0.3, dtype), O.round16(rng.standard_normal(K).astype(np.float32) * 0.2, dtype)


class _QuantStream:
    """one input with its parameter set: the tensors the op takes and the oracle's 16-bit input to the projection ``xp`` (after LayerNorm / GLU)"""

    def __init__(self, R, smooth, ln, glu, M, K, dtype, seed):
        self.L = _layer(K, 128, max(R, 16), 300 + K + R + seed, dtype)
        self.mod = make_module(self.L, dtype)
        self.mod._ensure_layout()
        self.smooth = self.L["smooth"] if smooth else None
        self.D = self.L["proj_down"] if R else None
        if glu:
            self.x = O.round16(np.random.default_rng(seed).standard_normal((M, 2 * K)).astype(np.float32) * 1.5, dtype)
            self.xp = O.glu_pairs(self.x, dtype)
        else:
            self.x = O.round16(_acts(M, K, seed, dtype) * 2 + 0.5, dtype) if ln else _acts(M, K, seed, dtype)
            self.xp = self.x
        self.xt = t16(self.x, dtype)
        self.ln = None
        if ln:
            scale, shift = _ln_params(K, dtype, seed)
            stats = O.ln_stats_ref(self.x)
            self.xp = O.ln_mod_ref(self.x, stats, scale, shift, dtype)
            self.ln = (torch.from_numpy(stats).cuda(), t16(scale, dtype), t16(shift, dtype))

    def args(self):
        d = dict(smooth=self.mod.smooth_factor if self.smooth is not None else None, lora_down=self.mod.proj_down if self.D is not None else None)
        if self.ln:
            d.update(ln_stats=self.ln[0], mod_scale=self.ln[1], mod_shift=self.ln[2])
        return d


def _quant_launch(streams, R, glu, fmt, K, M_pad, dtype, plain_input=None):
    """-> (code image, scale image, lora_act | None).  ``plain_input``: quantise this 16-bit tensor with the first stream's smooth / lora_down, no front end."""
    from nunchaku_amd._C import ops

    act = torch.empty(M_pad, K * 3 // 4, dtype=torch.uint8, device="cuda")
    asc = torch.empty(K // 64, M_pad, dtype=TORCH_DT[dtype], device="cuda")
    la = None
    if R:  # junk: the op clears what it accumulates into, and writes the rest
        la = torch.full((M_pad, R), 3.0, dtype=torch.float32, device="cuda") if fmt == "f32" else torch.full((M_pad, R), 12345, dtype=torch.int64, device="cuda")
    a0 = streams[0].args()
    if plain_input is not None:
        ops.quantize_w4a4_act_fuse_lora(plain_input, act, asc, a0["lora_down"], la, a0["smooth"])
        return act, asc, la
    second = None
    if len(streams) == 2:
        second = dict(input=streams[1].xt, **streams[1].args())
    ops.quantize_w4a4_act_fuse_lora(streams[0].xt, act, asc, a0["lora_down"], la, a0["smooth"], glu, False, ln_stats=a0.get("ln_stats"), mod_scale=a0.get("mod_scale"),
                                    mod_shift=a0.get("mod_shift"), second=second)
    return act, asc, la


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", QUANT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_quantize_case(case, dtype):
    """One row of QUANT_CASES.  Codes and scales through ``checked_codes`` (approximation envelope, flip budget against the IEEE oracle) on the oracle's 16-bit
    input to the projection x' (the LayerNorm front end's output where there is one); padded rows code 0, scale 0; lora_act per element within
    2e-5 (|x'| @ |D|) + 1e-6, the LayerNorm and grouped rows included; a fixed-point lora_act bit-equal between two launches.  A LayerNorm row's codes and
    scales are bit-equal to the stand-alone quantiser's on the oracle's LayerNorm output; a large-grid row's real rows are bit-equal to the same rows quantised
    with pad_size = 256 (which gets the oracle checks), everything behind them zero.
    fuse_glu rows: silu runs on the hardware exp2 / rcp, so an input element may land one 16-bit step from the oracle's -- they get the assertions of
    test_gpu_parity.test_quantize_fuse_glu (codes +-1 on <= 1 %, scales one step on <= 2 %, four such elements per row in the lora_act bound)."""
    from nunchaku_amd import layout, mode

    R, smooth, ln, glu, grouped, fmt, M, K, pad = case
    M_pad = math.ceil(M / pad) * pad
    large = pad != 256
    if grouped:
        streams = [_QuantStream(R, smooth, ln, glu, 256, K, dtype, 41), _QuantStream(R, smooth, ln, glu, M - 256, K, dtype, 42)]
    else:
        streams = [_QuantStream(R, smooth, ln, glu, M, K, dtype, 41)]
    s0 = streams[0]
    act, asc, la = _quant_launch(streams, R, glu, fmt, K, M_pad, dtype)
    if fmt != "f32":
        act2, asc2, la2 = _quant_launch(streams, R, glu, fmt, K, M_pad, dtype)
        assert torch.equal(la, la2) and torch.equal(act, act2) and torch.equal(asc, asc2), "fixed-point lora_act differs between two launches"
    codes_t, scales_t = layout.unpack_act(act, K), layout.unpack_scales(asc, M_pad)
    assert not codes_t[M:].any() and not scales_t[:, M:].any(), "padded rows: code 0, scale 0"
    la_t = None if la is None else mode.lora_act_to_float(la)
    if large:
        small_pad = math.ceil(M / 256) * 256
        assert quant_grid(M_pad, K) != quant_grid(small_pad, K) or M_pad > 262144
        sact, sasc, sla = _quant_launch(streams, R, glu, fmt, K, small_pad, dtype)
        assert torch.equal(codes_t[:small_pad], layout.unpack_act(sact, K)), "large grid: codes differ from the pad_size = 256 launch"
        assert torch.equal(scales_t[:, :small_pad], layout.unpack_scales(sasc, small_pad)), "large grid: scales differ from the pad_size = 256 launch"
        if la_t is not None:
            assert not la_t[small_pad:].any(), "large grid: lora_act of the padded rows"
            la_t = la_t[:small_pad]
        act, asc, M_pad = sact, sasc, small_pad
    la_got = None if la_t is None else la_t.cpu().numpy().astype(np.float64)
    if glu:
        q_ref, asc_ref, _ = O.quantize_w4a4_act_fuse_lora(s0.x, s0.smooth, None, dtype, fuse_glu=True)
        codes = layout.unpack_act(act, K).cpu().numpy().astype(np.int32)
        diff = np.abs(codes - q_ref)
        assert diff.max() <= 1 and (diff != 0).mean() <= 0.01, f"{(diff != 0).sum()} of {diff.size} codes differ (max {diff.max()})"
        sc = f32(layout.unpack_scales(asc, M_pad))
        assert np.all(np.abs(sc - asc_ref) <= np.abs(asc_ref) * STEP16[dtype] + 1e-30) and (sc != asc_ref).mean() <= 0.02
    else:
        x_all = np.concatenate([s.xp for s in streams])
        row0 = 0
        for s in streams:
            n = s.xp.shape[0]
            checked_codes(act, asc, x_all, s.smooth, dtype, rows=np.arange(row0, row0 + n))
            row0 += n
    if ln and not grouped:
        sact, sasc, _ = _quant_launch(streams, R, glu, fmt, K, M_pad, dtype, plain_input=t16(s0.xp, dtype))
        assert torch.equal(act, sact) and torch.equal(asc, sasc), "LayerNorm front end: not the stand-alone quantiser's codes on the oracle's LayerNorm output"
    if R:
        row0 = 0
        for s in streams:
            n = s.xp.shape[0]
            xa, Da = np.abs(s.xp).astype(np.float64), np.abs(s.D).astype(np.float64)
            bound = 2e-5 * (xa @ Da) + 1e-6
            if glu:
                bound += 4 * STEP16[dtype] * np.max(xa[:, :, None] * Da[None, :, :], axis=1)
            err = np.abs(la_got[row0:row0 + n] - s.xp.astype(np.float64) @ s.D.astype(np.float64))
            print(f"lora_act rows {row0} .. {row0 + n}: worst err / bound = {(err / bound).max():.3f}")
            assert np.all(err <= bound), f"lora_act rows {row0} .. {row0 + n}: worst err / bound = {(err / bound).max():.2f}"
            row0 += n
        assert np.all(np.abs(la_got[M:]) <= 1e-6), "lora_act of the padded rows"


# =======================================================================================================================================
# 3. attention
# =======================================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: f"L{c[0]}-g{c[1]}-ws{int(c[2])}-pre{int(c[3])}-{'mask' if c[4] else 'all'}")
def test_attention_case(case, dtype):
    """One row of ATTN_CASES: the reported plan stands for the claimed kernel; the output against the float64 softmax over the same 16-bit values (real keys
    only), at the bar of tests/test_gpu_attention.py: 3 * 2^-8 (bf16) / 3 * 2^-11 (fp16) of max |out|.  The padded keys of the masked row are larger
    than the real ones: counted, they would take the softmax over."""
    from nunchaku_amd._C import _Ops, ops
    from nunchaku_amd.ops.attention import attention_packed, q_prescale

    L, geometry, ws, prescaled, valid, key = case
    H, td = ATTN_H, TORCH_DT[dtype]
    g = torch.Generator(device="cuda").manual_seed(L + 10 * geometry)
    qkv = torch.randn(L, 3 * H * 128, device="cuda", generator=g).to(td)
    qkv[: L // 2, : H * 128] *= 4.0  # peaky rows
    real = None
    if valid is not None:
        real = np.zeros(L, dtype=bool)
        real[: valid[0]] = True
        qkv[valid[0]:, H * 128:] *= 3.0
    c = 1.0 / math.sqrt(128.0) * 1.4426950408889634
    if prescaled:
        qkv[:, : H * 128] = (qkv[:, : H * 128].float() * q_prescale(128)).to(td)
        c = 1.0
    vt = qkv[:, 2 * H * 128:].t().contiguous()
    saved = (_Ops.attention_geometry, _Ops.attention_use_workspace)
    _Ops.attention_geometry, _Ops.attention_use_workspace = geometry, ws
    try:
        out = attention_packed(qkv, vt, H, q_prescaled=prescaled, kv_valid=valid)
        plan = ops.attention_last_plan()
        ops.attention_workspace_status()
    finally:
        _Ops.attention_geometry, _Ops.attention_use_workspace = saved
    assert attn_plan_key(L, plan) == key, f"claimed {key}, launched {plan}"
    x = f32(qkv).reshape(L, 3, H, 128)
    got = f32(out).reshape(L, H, 128)
    for h in range(H):
        ref, _ = attn_softmax64(x[:, 0, h], x[:, 1, h], x[:, 2, h], c, real)
        err = np.abs(got[:, h] - ref).max()
        tol = 3 * ULP16[dtype] * np.abs(ref).max()
        print(f"head {h}: err / tol = {err / tol:.3f}")
        assert np.isfinite(got[:, h]).all() and err <= tol, f"head {h}: attention error {err:.3g} > {tol:.3g}"


def test_attention_refuses_lengths_that_are_no_multiple_of_128():
    """(L = 320 has no kernel: the 4-wave workgroup covers 128 query rows)"""
    from nunchaku_amd.ops.attention import attention_packed

    qkv = torch.zeros(320, 3 * ATTN_H * 128, dtype=torch.bfloat16, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        attention_packed(qkv, qkv[:, 2 * ATTN_H * 128:].t().contiguous(), ATTN_H)
