"""The launches whose state outlives them in a caller-owned workspace (include/svdq_amd.h: ``svdq_gemm_args.workspace``, ``svdq_attention_args.workspace``, the
scratch-only kinds of ``nunchaku_amd._C._PLAIN_KINDS``), one row per schedule class, at the smallest shape at which the class exists on 256 compute units.

tests/test_workspace_cases.py replays every row on the host (no GPU) and asserts that it is what its name says; tests/test_gpu_workspace_hygiene.py launches
the rows through the process's own cached workspaces and asserts the contract: counters back at zero, no byte read that the launch did not write, no
dependence on the launch before.

A row knows how to ``build(seed, dtype)`` its operands (device tensors, kept by the caller), how to ``run(operands)`` -- the launch, asynchronous on the current
stream, returning the tensors it is judged on -- and which of them are compared bit for bit (``exact``) and which are fp32 sums of atomics held to the bound
of the existing test of that path against the same oracle (``bounded``: the header says which outputs depend on the order of arrival).

Shapes (``streamk_groups_for`` / ``attention_groups_for``, csrc/gemm_w4a4.hip and csrc/attention.hip): a remainder of R tiles is split two ways when
``R * KP / (2 R) + 10 < 0.85 KP``, i.e. from KP = 29 K-steps: K = 3712 is the smallest K that splits, K = 128 never does; the tile queue needs more 128 x 128
tiles than the 512 workgroup slots; attention goes persistent for L % 256 == 0 whenever the tasks are no whole rounds of compute units."""

from __future__ import annotations

import contextlib
import ctypes as C
import math

import numpy as np

CUS = 256
GEMM_HEADER_BYTES, ATTENTION_HEADER_BYTES = 8192, 4096  # 2048 / 1024 int32 words: counters, error word, ticket counters -- all a test ever reads of a header
DTYPES = ("bf16", "fp16")
FUSE = {"none": 0, "silu": 1, "gelu_quant": 2, "rmsnorm_rope": 3}
CHAIN = ("sk256-3tiles", "dyn", "sk128", "att-24wg", "att-g2")  # the back-to-back and graph-replay tests queue these, in this order

# fill patterns for everything behind a header ("poison"), as 32-bit words: zeros; NaN read as fp32 and as either 16-bit half in both formats; fp32 1e30,
# whose halves 0x7149 / 0xf2ca are finite in bf16 (1e30, -8e30) and fp16 (10824, -13904)
POISON = {"zero": 0, "nan": 0x7FC07FC0, "finite": 0x7149F2CA}


def poison(buf, header_bytes: int, pattern: str) -> None:
    """fill ``buf`` (the uint8 tensor of a workspace) behind its header; stream-ordered like the launches"""
    n = (buf.numel() - header_bytes) // 4 * 4
    if n > 0:
        buf[header_bytes:header_bytes + n].view(_torch().int32).fill_(POISON[pattern])


def first_nonzero_word(buf, header_bytes: int):
    """index of the first non-zero int32 word of the header, or None"""
    import torch

    nz = torch.nonzero(buf[:header_bytes].view(torch.int32))
    return None if nz.numel() == 0 else int(nz[0])


def _torch():
    import torch

    return torch


def _td(dtype):
    import torch

    return {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]


def _gen(name: str, seed: int, dtype: str):
    import torch

    return torch.Generator(device="cuda").manual_seed(1000003 * seed + 101 * sum(name.encode()) + (dtype == "fp16"))


@contextlib.contextmanager
def _ops_set(**kw):
    """attributes of nunchaku_amd._C._Ops for the duration of a launch (no synchronisation)"""
    from nunchaku_amd._C import _Ops

    saved = {k: getattr(_Ops, k) for k in kw}
    for k, v in kw.items():
        setattr(_Ops, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(_Ops, k, v)


class Case:
    kind = "gemm"
    exact: tuple = ()
    bounded: tuple = ()

    def __init__(self, name: str, cls: str):
        self.name, self.cls = name, cls

    def __repr__(self):
        return self.name

    def header_bytes(self) -> int:
        return {"gemm": GEMM_HEADER_BYTES, "attention": ATTENTION_HEADER_BYTES}.get(self.kind, 0)

    def last_plan(self) -> dict:
        from nunchaku_amd._C import ops

        return ops.gemm_last_plan() if self.kind == "gemm" else ops.attention_last_plan() if self.kind == "attention" else {}

    def status(self) -> None:
        """the library's status query of this kind's workspace on the current stream (synchronises; raises when an owner gave up)"""
        from nunchaku_amd._C import ops

        if self.kind == "gemm":
            ops.gemm_workspace_status()
        elif self.kind == "attention":
            ops.attention_workspace_status()

    def check_plan(self, plan: dict) -> None:
        pass

    def check_bounded(self, operands: dict, outputs: dict) -> None:
        pass


# =====================================================================================================================================================
# W4A4 GEMM
# =====================================================================================================================================================
class GemmCase(Case):
    """A launch on random operands made on the device: the quantiser's own images of a random input, a random weight image, random scales and low-rank
    factors in the kernel layout.  Judged bit for bit, so no oracle is needed: every output is a function of the operands alone."""

    kind = "gemm"

    def __init__(self, name, cls, geometry, M_pad, N, K, R=32, fuse="none", q32=False, grouped=False, variant="plain", tile_rows=256, streamk=True,
                 dynamic=False, replay_geometry=1):
        super().__init__(name, cls)
        self.geometry, self.M_pad, self.N, self.K, self.R, self.fuse, self.q32, self.grouped = geometry, M_pad, N, K, R, fuse, q32, grouped
        self.variant, self.tile_rows, self.streamk, self.dynamic, self.replay_geometry = variant, tile_rows, streamk, dynamic, replay_geometry
        self.exact = ("out", "out_vt") if fuse == "rmsnorm_rope" else ("out",)

    # ---- host side ----
    def plan_row(self, dtype_code: int):
        """the row tests/test_gemm_plan.plan_args takes (workspace: the size svdq_gemm_workspace_bytes_for answers)"""
        return (self.M_pad, self.N, self.K, FUSE[self.fuse], self.geometry, self.R, 0, 1 if self.q32 else 0, 2, int(self.grouped), 0, dtype_code)

    def check_plan(self, plan):
        want = dict(variant=self.variant, tile_rows=self.tile_rows, dynamic_queue=self.dynamic)
        got = {k: plan[k] for k in want}
        assert got == want and (plan["streamk_groups"] > 0) == self.streamk, f"{self.name}: meant for {want}, stream-K {self.streamk}; launched {plan}"

    # ---- device side ----
    def build(self, seed, dtype):
        import torch

        from nunchaku_amd import layout
        from nunchaku_amd._C import mark_amd, ops

        g, td = _gen(self.name, seed, dtype), _td(dtype)
        M, N, K, R = self.M_pad, self.N, self.K, self.R
        rn = lambda *s, scale=1.0: mark_amd((torch.randn(*s, device="cuda", generator=g) * scale).to(td))
        x = rn(M, K)
        smooth = mark_amd((torch.rand(K, device="cuda", generator=g) + 0.5).to(td))
        o = dict(act=torch.empty(layout.act_image_shape(M, K), dtype=torch.uint8, device="cuda"), ascales=torch.empty(K // 64, M, dtype=td, device="cuda"),
                 lora_act=torch.empty(M, R, dtype=torch.int64 if self.q32 else torch.float32, device="cuda"))
        ops.quantize_w4a4_act_fuse_lora(x, o["act"], o["ascales"], rn(K, R, scale=0.05), o["lora_act"], smooth)
        for suffix in ("", "2") if self.grouped else ("",):
            codes = torch.randint(-128, 128, (N, K // 2), device="cuda", generator=g, dtype=torch.int16).to(torch.int8)
            o["wgt" + suffix] = layout.repack_qweight(codes)
            o["wscales" + suffix] = mark_amd((torch.rand(K // 64, N, device="cuda", generator=g) * 0.02 + 0.005).to(td))
            o["bias" + suffix] = rn(N, scale=0.1)
            o["lora_up" + suffix] = rn(N, R, scale=0.05)
            if self.fuse == "rmsnorm_rope":
                o["norm_q" + suffix] = mark_amd((torch.rand(128, device="cuda", generator=g) + 0.5).to(td))
                o["norm_k" + suffix] = mark_amd((torch.rand(128, device="cuda", generator=g) + 0.5).to(td))
        if self.fuse == "rmsnorm_rope":
            ang = torch.rand(M, 64, device="cuda", generator=g) * 6.28
            o["rotary_emb"] = torch.stack([torch.sin(ang), torch.cos(ang)], dim=-1).reshape(M, 128).contiguous()
        return o

    def run(self, o):
        import torch

        from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda

        td = o["ascales"].dtype
        out = torch.zeros(self.M_pad, self.N, dtype=td, device="cuda")
        kw = dict(act=o["act"], wgt=o["wgt"], out=out, ascales=o["ascales"], wscales=o["wscales"], lora_act_in=o["lora_act"], lora_up=o["lora_up"], bias=o["bias"])
        res = {"out": out}
        if self.fuse == "rmsnorm_rope":
            from nunchaku_amd.ops.attention import q_prescale

            res["out_vt"] = torch.zeros(self.N // 3, self.M_pad, dtype=td, device="cuda")
            kw.update(norm_q=o["norm_q"], norm_k=o["norm_k"], rotary_emb=o["rotary_emb"], out_vt=res["out_vt"], q_scale=q_prescale(128))
        if self.grouped:
            kw.update(split_rows=256, second=dict(wgt=o["wgt2"], wscales=o["wscales2"], bias=o["bias2"], lora_up=o["lora_up2"],
                                                  norm_q=o.get("norm_q2"), norm_k=o.get("norm_k2")))
        with _ops_set(gemm_geometry=self.geometry, gemm_use_workspace=True):
            svdq_gemm_w4a4_cuda(**kw)
        return res


class GeluQuantCase(Case):
    """A GELU_QUANT launch whose next-layer low-rank sums can only be fp32 (the split down projection and the solo-carry kernel take no fixed-point
    accumulators; include/svdq_amd.h, ``geometry``: "lora_act_out differs by fp32 summation order"): the operands and the bound of
    tests/test_gpu_parity.py::test_gelu_quant_next_low_rank_down_by_rank -- an oracle layer pair at M = 300, 256 -> 1024 -> 256, own rank 128 -- with the
    fragment images packed by the launch into the workspace tail (``cache_packed_lowrank`` off), so that the tail is what the kernels read.  Codes and
    scales bit for bit; ``lora_act`` within ``2e-3 max|ref| + 1e-4`` of the oracle on the operands the launch consumed, and finite.  That bound is the
    bf16 test's; the fp16 sums carry a 16-bit GELU output rounded eight times finer, so it holds for them a fortiori."""

    kind = "gemm"
    exact, bounded = ("qout", "oscales"), ("lora_act",)
    M, C, Hd, R1 = 300, 256, 1024, 128

    def __init__(self, name, cls, geometry, R2, variant, tile_rows):
        super().__init__(name, cls)
        self.geometry, self.R2, self.variant, self.tile_rows = geometry, R2, variant, tile_rows
        self.M_pad, self.N, self.K, self.R = 512, self.Hd, self.C, self.R1

    def plan_row(self, dtype_code: int):
        return (self.M_pad, self.N, self.K, FUSE["gelu_quant"], self.geometry, self.R, self.R2, 0, 2, 0, 0, dtype_code)

    def check_plan(self, plan):
        assert plan["variant"] == self.variant and plan["tile_rows"] == self.tile_rows and plan["lora_act_packed"], f"{self.name}: launched {plan}"

    def build(self, seed, dtype):
        from oracle import svdq_oracle as O
        from tests.helpers import checked_codes, make_module, t16

        fc1 = O.make_svdq_layer(self.C, self.Hd, self.R1, seed=31 + 10 * seed, dtype=dtype, cheap=True)
        fc2 = O.make_svdq_layer(self.Hd, self.C, self.R2, seed=32 + 10 * seed, dtype=dtype, cheap=True)
        x = O.make_activations(self.M, self.C, seed=33 + 10 * seed, dtype=dtype)
        m1, m2 = make_module(fc1, dtype), make_module(fc2, dtype, act_unsigned=True)
        m2._ensure_layout()
        qx, asc, la = m1.quantize(t16(x, dtype))
        q, a = checked_codes(qx, asc, x, fc1["smooth"], dtype)
        l_ = O.quantize_w4a4_act_fuse_lora(x, None, fc1["proj_down"], dtype)[2]
        ref = O.gemm_w4a4(q, a, fc1["qweight"], fc1["wscales"], dtype=dtype, bias=fc1["bias"], lora_act_in=l_, lora_up=fc1["proj_up"], fuse="gelu_quant",
                          next_smooth=fc2["smooth"], next_lora_down=fc2["proj_down"])
        return dict(m1=m1, m2=m2, act=qx, ascales=asc, lora_act=la, la_ref=ref["lora_act_out"][: self.M])

    def run(self, o):
        import torch

        from nunchaku_amd import layout
        from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda

        m1, m2, td = o["m1"], o["m2"], o["ascales"].dtype
        qh = torch.zeros(layout.act_image_shape(self.M_pad, self.Hd), dtype=torch.uint8, device="cuda")
        sh = torch.zeros(self.Hd // 64, self.M_pad, dtype=td, device="cuda")
        lh = torch.full((self.M_pad, self.R2), 3.0, dtype=torch.float32, device="cuda")  # (the op clears it)
        with _ops_set(gemm_geometry=self.geometry, gemm_use_workspace=True, cache_packed_lowrank=False):
            svdq_gemm_w4a4_cuda(act=o["act"], wgt=m1.qweight, qout=qh, ascales=o["ascales"], wscales=m1.wscales, oscales=sh, lora_act_in=o["lora_act"],
                                lora_up=m1.proj_up, lora_down=m2.proj_down, lora_act_out=lh, bias=m1.bias, smooth_factor=m2.smooth_factor)
        return {"qout": qh, "oscales": sh, "lora_act": lh}

    def check_bounded(self, o, res):
        got, ref = res["lora_act"].cpu().numpy(), o["la_ref"]
        assert np.isfinite(got).all(), f"{self.name}: lora_act_out is not finite"
        err, bound = np.abs(got[: self.M] - ref).max(), 2e-3 * np.abs(ref).max() + 1e-4
        assert got.shape[1] == self.R2 and err <= bound, f"{self.name}: lora_act_out off the oracle by {err:.3e}, bound {bound:.3e}"


class AllRankCase(GemmCase):
    """plain epilogue at rank 128: the all-rank kernel reads lora_act_in as the fragment image a pack kernel writes into the workspace tail"""

    def check_plan(self, plan):
        super().check_plan(plan)
        assert plan["lora_act_packed"], f"{self.name}: launched {plan}"

    def run(self, o):
        with _ops_set(cache_packed_lowrank=False):
            return super().run(o)


# =====================================================================================================================================================
# attention
# =====================================================================================================================================================
class AttentionCase(Case):
    kind = "attention"

    def __init__(self, name, cls, geometry, L, H, prescaled=False, kv_valid=None, qR=0, q32=False, split=False):
        super().__init__(name, cls)
        self.geometry, self.L, self.H, self.prescaled, self.kv_valid, self.qR, self.q32, self.split = geometry, L, H, prescaled, kv_valid, qR, q32, split
        self.exact = ("qact", "qscales") + (("lora_act",) if q32 else ()) if qR else ("out",)
        self.bounded = ("lora_act",) if qR and not q32 else ()

    def args(self, lib_mod, workspace_bytes=0):
        """svdq_attention_args for the host-side queries (made-up aligned addresses: none is dereferenced)"""
        a = lib_mod.AttentionArgs()
        a.q, a.k, a.vt, a.out = 0x10000000, 0x20000000, 0x30000000, 0x40000000
        a.L, a.H, a.head_dim, a.dtype, a.geometry, a.q_prescaled = self.L, self.H, 128, 0, self.geometry, int(self.prescaled)
        if self.kv_valid:
            a.kv_len0, a.kv_start1, a.kv_end1 = self.kv_valid
        if self.qR:
            a.qact, a.qscales, a.qlora_act, a.qsmooth, a.qlora_down, a.qR = 0x50000000, 0x51000000, 0x52000000, 0x53000000, 0x54000000, self.qR
            a.qlora_act_format = 1 if self.q32 else 0
        a.workspace, a.workspace_bytes = (0x100000000, workspace_bytes) if workspace_bytes else (0, 0)
        return a

    def check_plan(self, plan):
        assert plan["geometry"] == max(self.geometry, 1) and plan["persistent_groups"] > 0 and not plan["masked_geometry2"] and \
            plan["split_lowrank"] == self.split, f"{self.name}: launched {plan}"

    def build(self, seed, dtype):
        import torch

        from nunchaku_amd._C import mark_amd
        from nunchaku_amd.ops.attention import q_prescale

        g, td, L, H = _gen(self.name, seed, dtype), _td(dtype), self.L, self.H
        qkv = torch.randn(L, 3 * H * 128, device="cuda", generator=g)
        if self.prescaled:
            qkv[:, : H * 128] *= q_prescale(128)
        qkv = qkv.to(td)
        o = dict(qkv=qkv, vt=qkv[:, 2 * H * 128:].t().contiguous())
        if self.qR:
            K = H * 128
            o["smooth"] = mark_amd((torch.rand(K, device="cuda", generator=g) + 0.5).to(td))
            o["lora_down"] = mark_amd((torch.randn(K, self.qR, device="cuda", generator=g) * 0.05).to(td))  # the bytes are rank-major [R][K]
            if self.bounded:
                # the oracle of tests/test_gpu_attention_lowrank_image.py: the kernel's own 16-bit output -- a launch without the quantiser on the same
                # schedule, once per operands -- times the factor, in float64
                x = self._launch(o, quant=False)["out"].float().cpu().numpy().astype(np.float64)
                D = o["lora_down"].float().cpu().numpy().astype(np.float64).reshape(self.qR, K).T
                o["la_ref"], o["la_bound"] = x @ D, 2e-5 * (np.abs(x) @ np.abs(D)) + 1e-6
        return o

    def _launch(self, o, quant):
        import torch

        from nunchaku_amd._C import ops

        L, H, td = self.L, self.H, o["qkv"].dtype
        q, k = o["qkv"][:, : H * 128].unflatten(1, (H, 128)), o["qkv"][:, H * 128: 2 * H * 128].unflatten(1, (H, 128))
        res, out, qd = {}, None, None
        if quant:
            K = H * 128
            res = {"qact": torch.zeros(L, K * 3 // 4, dtype=torch.uint8, device="cuda"), "qscales": torch.zeros(K // 64, L, dtype=td, device="cuda"),
                   "lora_act": torch.zeros(L, self.qR, dtype=torch.int64 if self.q32 else torch.float32, device="cuda")}
            qd = dict(act=res["qact"], ascales=res["qscales"], lora_act=res["lora_act"], R=self.qR, smooth=o["smooth"], lora_down=o["lora_down"])
        else:
            out = res["out"] = torch.zeros(L, H * 128, dtype=td, device="cuda")
        # (the split fused quantiser packs its factor into the workspace, in front of the row image, when the caller brings no image of its own)
        with _ops_set(attention_geometry=self.geometry, attention_use_workspace=True, attention_split_lowrank=True, cache_packed_lowrank=not self.split):
            ops.attention(q, k, o["vt"].unflatten(0, (H, 128)), None if out is None else out.unflatten(1, (H, 128)), 1.0 / math.sqrt(128), None, qd,
                          kv_valid=self.kv_valid, q_prescaled=self.prescaled)
        return res

    def run(self, o):
        return self._launch(o, quant=bool(self.qR))

    def check_bounded(self, o, res):
        got = res["lora_act"].float().cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), f"{self.name}: qlora_act is not finite"
        ratio = (np.abs(got - o["la_ref"]) / o["la_bound"]).max()
        assert ratio <= 1.0, f"{self.name}: qlora_act: worst err / bound = {ratio:.2f}"


# =====================================================================================================================================================
# scratch-only kinds
# =====================================================================================================================================================
class AwqCase(Case):
    kind = "awq"
    exact = ("out",)

    def __init__(self, name, cls, splits):
        from tests.test_gpu_dispatch_classes import AWQ_GEMM_CASES

        super().__init__(name, cls)
        self.splits = splits
        self.M, self.N, self.K, _ = [c for c in AWQ_GEMM_CASES if c[3] == splits][0]

    def build(self, seed, dtype):
        import torch

        from tests.test_gpu_dispatch_classes import awq_gemm_layer

        td = _td(dtype)
        qw, sc, zr = awq_gemm_layer(self.N, self.K, td, seed=seed * 131 + self.M + self.N + self.K)
        g = torch.Generator().manual_seed(seed * 17 + self.K)
        return dict(qw=qw, sc=sc, zr=zr, bias=(torch.randn(self.N, generator=g) * 0.1).to(td).cuda(), x=torch.randn(self.M, self.K, generator=g).to(td).cuda())

    def run(self, o):
        from nunchaku_amd._C import ops

        return {"out": ops.gemm_awq(o["x"], o["qw"], o["sc"], o["zr"], o["bias"])}


class LinearAttentionCase(Case):
    kind = "linear_attention"
    exact = ("out", "vk")

    def __init__(self, name, cls, B, T, H):
        super().__init__(name, cls)
        self.B, self.T, self.H = B, T, H

    def args(self, lib_mod):
        a = lib_mod.LinearAttentionArgs()
        a.B, a.T, a.H, a.head_dim, a.dtype, a.eps = self.B, self.T, self.H, 32, 0, 1e-6
        a.kv, a.ldkv, a.kv_bs = 0x10000000, 3 * self.H * 32, self.T * 3 * self.H * 32
        a.q, a.ldq, a.q_bs, a.out, a.ldo, a.out_bs = 0x20000000, 3 * self.H * 32, self.T * 3 * self.H * 32, 0x30000000, self.H * 32, self.T * self.H * 32
        return a

    def build(self, seed, dtype):
        import torch

        return dict(qkv=torch.randn(self.B, self.T, 3 * self.H * 32, device="cuda", generator=_gen(self.name, seed, dtype)).to(_td(dtype)))

    def run(self, o):
        from nunchaku_amd.ops.attention import linear_attention

        out, vk = linear_attention(o["qkv"], self.H, return_vk=True)
        return {"out": out, "vk": vk}


# =====================================================================================================================================================
# the table: one row per class
# =====================================================================================================================================================
CLASSES = ("sk256-1tile", "sk256-3tiles", "sk256-rounds", "sk128", "sk-wave-tile", "sk-q32", "sk-grouped", "dyn", "dyn-stagger", "all-rank", "split-down",
           "solo-carry", "rope-sk", "att-2wg", "att-24wg", "att-g2", "att-mask", "att-q32r", "att-split", "awq-split-2", "awq-split-4", "awq-split-16",
           "litela-chunks")


def _table():
    return (
        GemmCase("sk256-1tile", "sk256-1tile", 1, 256, 128, 3712),
        GemmCase("sk256-3tiles", "sk256-3tiles", 1, 256, 384, 3712),
        GemmCase("sk256-rounds", "sk256-rounds", 1, 768, 11008, 3712),               # 258 tiles on 256 slots: one whole round, tiles 256 and 257 split
        GemmCase("sk128", "sk128", 3, 256, 128, 3712, tile_rows=128, replay_geometry=2),
        GemmCase("sk-wave-tile", "sk-wave-tile", 8, 256, 128, 3712, variant="wave_tile_128"),
        GemmCase("sk-q32", "sk-q32", 1, 256, 384, 3712, q32=True),
        GemmCase("sk-grouped", "sk-grouped", 1, 512, 128, 3712, grouped=True),
        GemmCase("dyn", "dyn", 2, 1024, 8320, 128, tile_rows=128, streamk=False, dynamic=True, replay_geometry=2),   # 520 tiles of 128 x 128 on 512 slots
        GemmCase("dyn-stagger", "dyn-stagger", 4, 1024, 8320, 128, tile_rows=128, streamk=False, dynamic=True, replay_geometry=2),
        AllRankCase("all-rank", "all-rank", 0, 256, 256, 128, R=128, variant="all_rank", streamk=False),
        GeluQuantCase("split-down", "split-down", 7, 128, "split_down", 256),
        GeluQuantCase("solo-carry", "solo-carry", 6, 48, "solo_carry", 128),
        GemmCase("rope-sk", "rope-sk", 1, 256, 384, 3712, fuse="rmsnorm_rope"),
        AttentionCase("att-2wg", "att-2wg", 1, 256, 1),
        AttentionCase("att-24wg", "att-24wg", 1, 512, 3),
        AttentionCase("att-g2", "att-g2", 2, 512, 3, prescaled=True),
        AttentionCase("att-mask", "att-mask", 1, 512, 3, kv_valid=(300, 384, 500)),
        AttentionCase("att-q32r", "att-q32r", 0, 512, 3, qR=32, q32=True),
        AttentionCase("att-split", "att-split", 0, 512, 2, qR=128, split=True),       # H * 128 = 256: the split's shape rule
        AwqCase("awq-split-2", "awq-split-2", 2),
        AwqCase("awq-split-4", "awq-split-4", 4),
        AwqCase("awq-split-16", "awq-split-16", 16),
        LinearAttentionCase("litela-chunks", "litela-chunks", 2, 600, 2),              # three chunks of 256 tokens per batch element, the last ragged
    )


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
KINDS = ("gemm", "attention", "awq", "linear_attention")


def of_kind(kind: str):
    return tuple(c for c in CASES if c.kind == kind)


# ---- host-side replays (tests/test_workspace_cases.py) ----------------------------------------------------------------------------------------------
def gemm_segments(case) -> np.ndarray:
    """records {position, tile, kp0, kp1, partial slot or -1, contributors the owner waits for} of svdq_gemm_schedule_ex on 256 compute units"""
    from nunchaku_amd import _lib

    lib = _lib.load()
    n = lib.svdq_gemm_schedule_ex(case.M_pad, case.N, case.K, CUS, 1, case.replay_geometry, None, 0)
    assert n > 0, (case, n)
    buf = (C.c_int32 * (6 * n))()
    assert lib.svdq_gemm_schedule_ex(case.M_pad, case.N, case.K, CUS, 1, case.replay_geometry, buf, n) == n
    return np.frombuffer(buf, dtype=np.int32).reshape(n, 6).copy()
