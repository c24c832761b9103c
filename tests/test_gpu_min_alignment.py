"""Every entry point at the smallest alignment its validation admits, on the GPU.

tests/test_alignment_contract.py pins on the host what validation admits (its ``LEDGER``).  Here each launch runs twice: once as the wrapper marshals it
(torch allocates 256-byte aligned, contiguous or strided by multiples of 8), once with EVERY operand the ledger admits below 16 bytes moved to its admitted
minimum at the same time -- into a fresh buffer, ``admitted alignment`` bytes behind a 256-byte boundary, so an 8-byte operand sits at an address = 8
(mod 16) -- and every strided operand given its smallest admitted non-contiguous stride (``ldo = N + 4``, ``ldx = K + 4``, ``ldvt = M_pad + 2``).  The
args struct is retargeted on its way into the library (``tests.helpers.retargeted``), so the wrapper, the plan and every other operand are the aligned
launch's.  A moved launch asserts, in the edit itself, that it moved every operand of the ledger that the launch passes.

What is asserted: every output of the moved launch equals the aligned launch's bit for bit -- except fp32 low-rank sums added with atomics, which the
header documents as order-dependent and which get the oracle gate of the row's own test; the fixed-point (q32) rows give bit equality of those sums too.
A moved output lives in a buffer of a sentinel (a NaN payload no kernel produces) with a guard in front of and behind it: the number of elements that
differ from the sentinel afterwards must be the operand's element count -- and what the aligned launch wrote into the wrapper's own buffer, prefilled
with the same sentinel -- so a store outside the footprint is counted.  A moved input must still hold what was copied in.

The aligned launch is not held to the oracle again: every case names the test that does that for the same launch.  No tolerance here is new."""
import math

import numpy as np
import pytest
import torch

from oracle import svdq_oracle as O
from tests import test_gpu_dispatch_classes as D
from tests import test_gpu_hot_instantiations as T
from tests.helpers import TORCH_DT, retargeted, t16
from tests.test_alignment_contract import below_16

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "fp16")
GUARD = 256                                   # bytes of sentinel in front of and behind a moved operand
SENT = {2: 0x7FA5, 4: 0x7FA5A5A5}             # per counting granule (bytes): a NaN with a payload as 16-bit, as fp32 and as either half of a Q31.32 word
INT = {2: torch.int16, 4: torch.int32}
Q, G, A = "svdq_quantize_w4a4_act_fuse_lora", "svdq_gemm_w4a4", "svdq_attention"
STAYS = {"status"}                            # the host-visible status word is the wrapper's pinned tensor, polled by the wrapper: it stays where it is


@pytest.fixture(autouse=True)
def _gpu(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"


# ---- device memory at an address of the args struct -------------------------------------------------------------------------------------------
class _Raw:
    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}


def alias(ptr: int, rows: int, row_bytes: int, ld_bytes: int) -> torch.Tensor:
    """uint8 [rows, row_bytes] view of the device memory at ``ptr`` (memory a live tensor of the launch owns)"""
    span = (rows - 1) * ld_bytes + row_bytes
    t = torch.as_tensor(_Raw(ptr, span), device="cuda")
    assert t.data_ptr() == ptr and t.dtype == torch.uint8 and t.numel() == span
    return t.as_strided((rows, row_bytes), (ld_bytes, 1))


def _typed(view: torch.Tensor, granule: int) -> torch.Tensor:
    return view.view(INT[granule])


class Window:
    """a fresh buffer of the sentinel with a [rows, row_bytes] operand ``off`` bytes behind a 256-byte boundary, GUARD bytes of sentinel on either side"""

    def __init__(self, rows, row_bytes, ld_bytes, off, granule):
        span = (rows - 1) * ld_bytes + row_bytes
        assert off % granule == 0 and span % granule == 0 and ld_bytes % granule == 0
        total = -(-(GUARD + off + span + GUARD) // 4) * 4
        self.granule = granule
        self.buf = torch.full((total // granule,), SENT[granule], dtype=INT[granule], device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + GUARD + off
        self.view = self.buf.view(torch.uint8)[GUARD + off:GUARD + off + span].as_strided((rows, row_bytes), (ld_bytes, 1))

    def changed(self) -> int:
        return int((self.buf != SENT[self.granule]).sum())


def Op(kind, nbytes, granule=2, rows=1, ld=None, new_ld=None, off=None, live=None):
    """one operand of a spec: kind "in" | "out" | "acc" (read and written: the moved copy starts from what the wrapper's buffer holds); ``nbytes`` per row;
    ``ld``: the struct's stride field (16-bit elements), ``new_ld``: the stride of the moved operand; ``off``: where the admitted alignment depends on a
    mode (the Q31.32 sums: 8 bytes), else the ledger's; ``live``: elements a launch writes where that is not all of them"""
    return dict(kind=kind, row_bytes=nbytes, granule=granule, rows=rows, ld=ld, new_ld=new_ld, off=off, live=live)


class Launch:
    """The edit of one launch (``retargeted(..., edit=...)``).  ``move=False``: the aligned launch -- records where its outputs are and prefills them with the
    sentinel; ``move=True``: every operand of ``spec(a)`` that is given moves to the ledger's alignment.  ``also(a)``: further changes to the struct, for both.
    ``collect()`` (while the launch's tensors are alive) keeps a copy of every output and the count of what was written."""

    def __init__(self, entry, spec, move, also=None, stays=()):
        self.entry, self.spec, self.move, self.also, self.stays = entry, spec, move, also, set(stays) | STAYS
        self.ops, self.plan = {}, None

    def __call__(self, a, i=0):
        if self.also:
            self.also(a)
        low = below_16(self.entry)
        done = set()
        for field, op in self.spec(a).items():
            ptr = getattr(a, field)
            if not ptr or op is None:
                continue
            done.add(field)
            old_ld = getattr(a, op["ld"]) * 2 if op["ld"] else op["row_bytes"]
            src = alias(ptr, op["rows"], op["row_bytes"], old_ld)
            rec = dict(op, src=src, win=None, snap=None if op["kind"] == "out" else src.clone())  # (an input may be a temporary of the wrapper)
            if self.move:
                off = op["off"] or low[field]
                assert off >= low[field]
                w = rec["win"] = Window(op["rows"], op["row_bytes"], op["new_ld"] * 2 if op["ld"] else op["row_bytes"], off, op["granule"])
                if op["kind"] != "out":
                    w.view.copy_(src)
                setattr(a, field, w.ptr)
                if op["ld"]:
                    setattr(a, op["ld"], op["new_ld"])
                assert getattr(a, field) % (2 * off) == off, "the moved operand is aligned to its minimum and to nothing coarser"
            elif op["kind"] == "out":
                _typed(src, op["granule"]).fill_(SENT[op["granule"]])
            self.ops[(i, field)] = rec
        if self.move:  # everything the ledger admits below 16 bytes and this launch passes has moved
            given = {f for f in low if getattr(a, f)} - self.stays
            assert done >= given, f"{self.entry}: not moved: {sorted(given - done)}"
        if self.entry == Q:
            import ctypes as C

            from nunchaku_amd import _lib

            out = (C.c_int32 * 8)()
            assert _lib.load().svdq_quantize_plan(C.byref(a), out) == 0
            self.plan = ("fast", "general")[out[0]]

    def collect(self):
        for rec in self.ops.values():
            w = rec["win"]
            rec["bytes"] = (w.view if w is not None else rec["src"]).clone()
            # elements that differ from the sentinel: over the whole buffer of a moved operand (guards and gaps included), over the operand of an aligned one
            rec["count"] = w.changed() if w is not None else int((_typed(rec["src"], rec["granule"]) != SENT[rec["granule"]]).sum())
            rec["src"] = None

    def bytes_of(self, key):
        return self.ops[key]["bytes"]


def run_pair(monkeypatch, symbol, launch, spec, entry=None, also=None, stays=()):
    """-> (aligned edit, moved edit, what the aligned launch returned, what the moved launch returned).  ``launch`` returns every output tensor it
    allocates, so that none is freed before it has been read."""
    entry = entry or symbol
    al, mv = Launch(entry, spec, False, also, stays), Launch(entry, spec, True, also, stays)
    res_a = retargeted(monkeypatch, symbol, launch, edit=al)
    al.collect()
    res_m = retargeted(monkeypatch, symbol, launch, edit=mv)
    mv.collect()
    assert al.ops.keys() == mv.ops.keys() and mv.ops, "the two launches passed different operands"
    return al, mv, res_a, res_m


def assert_same(al, mv, what, gated=()):
    """every operand of the pair: inputs still hold what was copied in and nothing else was written near them; outputs bit-equal, with as many elements
    written as the aligned launch wrote and as the operand has (``gated``: fields compared by the caller; their footprint is still counted)"""
    for key, rec in mv.ops.items():
        ra, size = al.ops[key], rec["rows"] * rec["row_bytes"] // rec["granule"]
        if rec["kind"] == "in":
            assert torch.equal(rec["bytes"], rec["snap"]) and rec["count"] == size, f"{what}: input {key} or its surroundings were written"
            continue
        if rec["kind"] == "out":
            live = rec["live"] if rec["live"] is not None else size
            assert rec["count"] == ra["count"] == live, f"{what}: {key}: {rec['count']} elements written, the aligned launch wrote {ra['count']}, the operand has {live}"
        else:
            assert rec["count"] == size, f"{what}: {key}: {rec['count']} elements differ from the sentinel around an operand of {size}"
        if key[1] in gated:
            continue
        assert torch.equal(ra["bytes"], rec["bytes"]), f"{what}: {key}: {int((ra['bytes'] != rec['bytes']).sum())} of {rec['bytes'].numel()} bytes differ from the aligned launch"


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# =======================================================================================================================================
# 1. the quantiser
# =======================================================================================================================================
def _quant_spec(a):
    K2, f32w = a.K * 2, 8 if a.lora_act_format else 4
    vec = lambda: Op("in", K2)
    return {
        "x": None if a.fuse_glu else Op("in", K2, rows=a.M, ld="ldx", new_ld=a.K + 4),   # (fuse_glu reads x in 16-byte pieces: validated, it stays)
        "smooth": vec(), "mod_scale": vec(), "mod_shift": vec(), "lora_down": Op("in", a.R * K2), "ln_stats": Op("in", a.M * 8, 4),
        "x2": Op("in", K2, rows=a.M2, ld="ldx2", new_ld=a.K + 4),
        "smooth2": vec(), "mod_scale2": vec(), "mod_shift2": vec(), "lora_down2": Op("in", a.R * K2), "ln_stats2": Op("in", a.M2 * 8, 4),
        "ascales": Op("out", (a.K // 64) * a.M_pad * 2),
        "lora_act": Op("out", a.M_pad * a.R * f32w, 4, off=f32w),   # (one K slice at these shapes: plain stores of every element, no atomics)
    }


QUANT_ROWS = (  # rows of T.QUANT_CASES and the family svdq_quantize_plan names for them, aligned and moved alike
    ((32, True, True, False, False, "f32", T.QUANT_M, T.QUANT_K, 256), "fast"),      # one slab of lora_down by 16-byte LDS-DMA
    ((96, True, True, False, False, "f32", T.QUANT_M, T.QUANT_K, 256), "fast"),      # MULTI: three slabs
    ((96, True, True, False, True, "f32", T.QUANT_M, T.QUANT_K, 256), "fast"),       # grouped: both parameter sets
    ((32, True, False, True, False, "f32", T.QUANT_M, T.QUANT_K, 256), "general"),   # fuse_glu: x stays, the vectors move
    ((176, True, False, False, False, "f32", T.QUANT_M, T.QUANT_K, 256), "general"),
    ((32, True, False, False, False, "q32", T.QUANT_M, T.QUANT_K, 256), "fast"),
)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row", QUANT_ROWS, ids=lambda r: "-".join(str(v) for v in r[0][:6]))
def test_quantize(row, dtype, monkeypatch):
    """rows of QUANT_CASES: tests/test_gpu_hot_instantiations.py::test_quantize_case holds the aligned launch to the oracle.  x at + 8 bytes with ldx = K + 4
    (every second row starts at 8 mod 16), smooth, lora_down, the LayerNorm operands and the second set at + 8, ascales at + 2, lora_act at + 4 (fp32)
    / + 8 (Q31.32): codes, scales and low-rank sums bit for bit."""
    case, family = row
    assert case in T.QUANT_CASES
    R, smooth, ln, glu, grouped, fmt, M, K, pad = case
    M_pad = math.ceil(M / pad) * pad
    if grouped:
        streams = [T._QuantStream(R, smooth, ln, glu, 256, K, dtype, 41), T._QuantStream(R, smooth, ln, glu, M - 256, K, dtype, 42)]
    else:
        streams = [T._QuantStream(R, smooth, ln, glu, M, K, dtype, 41)]
    pl = T.quant_plan(R, smooth, ln, glu, grouped, fmt, M, K, M_pad)
    assert pl["family"] == family and pl["slices"] == 1 and not pl["lora_act_add"] & 1
    al, mv, res_a, res_m = run_pair(monkeypatch, Q, lambda: T._quant_launch(streams, R, glu, fmt, K, M_pad, dtype), _quant_spec, stays=("x",) if glu else ())
    assert al.plan == mv.plan == family, f"aligned: {al.plan}, moved: {mv.plan}, the table row: {family}"
    assert same_bits(res_a[0], res_m[0]), "codes differ from the aligned launch"
    assert_same(al, mv, f"quantise {case} {dtype}")
    moved = {f for _, f in mv.ops}
    assert {"smooth", "lora_down", "ascales", "lora_act"} <= moved and ("x" in moved) != glu and ("ln_stats" in moved) == ln and ("lora_down2" in moved) == grouped


# =======================================================================================================================================
# 2. the W4A4 GEMM
# =======================================================================================================================================
def _gemm_spec(a):
    N2, acc = a.N * 2, 8 if a.lora_act_format else 4
    vec, down = (lambda: Op("in", N2)), (lambda: Op("in", a.R2 * N2))
    return {
        # (with out_vt the V columns of out stay unwritten: sentinel in both launches)
        "out": Op("out", N2, rows=a.M, ld="ldo", new_ld=a.N + 4, live=a.M * a.N * 2 // 3 if a.out_vt else None),
        "bias": vec(), "bias2": vec(), "next_smooth": vec(), "next_smooth2": vec(), "next_lora_down": down(), "next_lora_down2": down(),
        "norm_q": Op("in", 256), "norm_k": Op("in", 256), "norm_q2": Op("in", 256), "norm_k2": Op("in", 256),
        "lora_act_out": Op("acc", a.M_pad * a.R2 * acc, 4),
        "oscales": Op("out", (a.N // 64) * a.M_pad * 2),
        "out_vt": Op("out", a.M * 2, rows=a.N // 3, ld="ldvt", new_ld=a.M_pad + 2),
    }


def _gemm_row(fuse, geometry, fmt, variant, R=None, R2=None, M=T.M_SMALL):
    rows = [c for c in T.GEMM_CASES if c[0] == fuse and c[1] == geometry and c[2] == fmt and c[9][1] == variant and c[5] == M
            and (R is None or c[3] == R) and (R2 is None or c[4] == R2)]
    assert len(rows) >= 1, (fuse, geometry, fmt, variant, R, R2, M)
    return rows[0]


GEMM_ROWS = tuple(
    # (256, plain) and (128, plain) for each epilogue; GELU_QUANT with fixed-point sums: bit equality of lora_act_out
    [_gemm_row(f, g, "q32" if f == "gelu_quant" else "f32", "plain") for f in T.FUSES for g in (1, 3)]
    + [_gemm_row("gelu_quant", 1, "f32", "all_rank"), _gemm_row("none", 3, "f32", "all_rank")]
    + [_gemm_row("gelu_quant", 1, "f32", "carry", R2=32), _gemm_row("gelu_quant", 6, "f32", "solo_carry", R2=48),
       _gemm_row("gelu_quant", 7, "f32", "split_down", R2=64), _gemm_row("none", 8, "f32", "wave_tile_128", R=0),
       _gemm_row("none", 8, "f32", "wave_tile_128", R=32), _gemm_row("gelu_quant", 1, "f32", "hybrid_carry", R2=48, M=T.ROWRUN_M)]
)
assert len(set(GEMM_ROWS)) == 16 and {(c[9][0], c[9][1]) for c in GEMM_ROWS} == \
    {(256, "plain"), (128, "plain"), (256, "all_rank"), (128, "all_rank"), (256, "carry"), (128, "solo_carry"), (256, "split_down"), (256, "wave_tile_128"),
     (256, "hybrid_carry")}


def _lora_act_out_gate(run, launches, what):
    """the gate of tests/test_gpu_hot_instantiations.py::test_gemm_case on fp32 low-rank sums: per element within ``_lora_act_out_bound`` of the oracle on the
    operands the launch consumed.  ``launches``: {name: lora_act_out [M_pad, R2] as numpy}"""
    fuse, _, fmt, R, R2, M, K, N, _, _ = run.case
    rows = T._sample_rows(M)
    q, a, la = run.consumed(rows)
    L1, L2 = run.L1, run.L2
    ref = O.gemm_w4a4(q, a, L1["qweight"], L1["wscales"], fuse=fuse, dtype=run.dtype, bias=L1["bias"], lora_act_in=la, lora_up=L1["proj_up"],
                      next_smooth=L2["smooth"], next_lora_down=L2["proj_down"])
    h = ref["g16"][:M] if rows is None else ref["g16"]
    la_ref = ref["lora_act_out"][:M] if rows is None else ref["lora_act_out"]
    bound = T._lora_act_out_bound(h, L2["proj_down"], run.dtype, T.H_STEPS_ALLOWED[(run.dtype, N)])
    sel = slice(0, M) if rows is None else rows
    for name, got in launches.items():
        err = np.abs(got[sel].astype(np.float64) - la_ref)
        print(f"{what} {name}: lora_act_out worst err / bound = {(err / bound).max():.3f}")
        assert got.shape[1] == R2 and np.all(err <= bound), f"{what} {name}: lora_act_out worst err / bound = {(err / bound).max():.2f}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", GEMM_ROWS, ids=lambda c: "-".join(str(v) for v in c[:9]))
def test_gemm(case, dtype, monkeypatch):
    """rows of GEMM_CASES, one per plan key: tests/test_gpu_hot_instantiations.py::test_gemm_case holds the aligned launch to the oracle.  out at + 8 bytes with
    ldo = N + 4 (rows alternate between 8 and 0 mod 16: the 16-byte stores of the epilogues), bias, next_smooth, next_lora_down, norm_q, norm_k and lora_act_out
    at + 8, oscales at + 2; the RMSNorm + RoPE rows also write V transposed to out_vt at + 4 bytes with ldvt = M_pad + 2.  16-bit outputs, codes and scales
    and fixed-point sums bit for bit; fp32 lora_act_out (atomics) within test_gemm_case's bound of the oracle."""
    fuse, geometry, fmt, R, R2, M, K, N, ws, key = case
    run = T._GemmRun(case, dtype)
    also = None
    if fuse == "rmsnorm_rope":
        # out_vt is not among the wrapper's operands of this row: both launches get it -- 16-byte aligned with ldvt = M_pad in the aligned one
        vt_ref = Window(N // 3, run.M_pad * 2, run.M_pad * 2, 0, 2)

        def also(a):
            a.out_vt, a.ldvt = vt_ref.ptr, run.M_pad
    al, mv, (outs_a, plan_a), (outs_m, plan_m) = run_pair(monkeypatch, G, run.launch, _gemm_spec, also=also)
    assert T._plan_key(plan_a) == T._plan_key(plan_m) == key[:2], f"the table row claims {key}; aligned {plan_a}, moved {plan_m}"
    assert plan_a == plan_m
    what = f"gemm {case[:9]} {dtype}"
    moved = {f for _, f in mv.ops}
    if fuse == "gelu_quant":
        assert same_bits(outs_a[0], outs_m[0]), f"{what}: codes differ from the aligned launch"
        assert {"bias", "next_smooth", "oscales"} <= moved and ("lora_act_out" in moved) == (R2 > 0) == ("next_lora_down" in moved)
        assert_same(al, mv, what, gated=("lora_act_out",) if fmt == "f32" else ())
        if R2 and fmt == "f32":
            _lora_act_out_gate(run, {name: L.bytes_of((0, "lora_act_out")).view(torch.float32).view(run.M_pad, R2).cpu().numpy()
                                     for name, L in (("aligned", al), ("moved", mv))}, what)
    elif fuse == "rmsnorm_rope":
        assert {"out", "bias", "norm_q", "norm_k", "out_vt"} <= moved
        assert_same(al, mv, what)
        # the aligned launch's V^T is the V columns of the row's launch without out_vt (the one test_gemm_case holds to the oracle), transposed
        (plain,), _ = run.launch()
        torch.cuda.synchronize()
        vt = al.bytes_of((0, "out_vt")).view(TORCH_DT[dtype])
        assert same_bits(vt, plain[:, 2 * N // 3:].t()), f"{what}: out_vt is not the V columns transposed"
        qk = al.bytes_of((0, "out")).view(TORCH_DT[dtype])[:, :2 * N // 3]
        assert same_bits(qk, plain[:, :2 * N // 3]), f"{what}: Q and K differ from the launch without out_vt"
    else:
        assert {"out", "bias"} <= moved
        assert_same(al, mv, what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_grouped(dtype, monkeypatch):
    """a grouped launch (wgt2): RMSNorm + RoPE on 512 rows, the second set for rows >= 256, with out, out_vt, bias(2), norm_q(2) and norm_k(2) moved.  Grouped
    launches are held to separate launches -- and those to the oracle -- by tests/test_gpu_fused_norm.py::test_grouped_launches_match_separate_calls and
    tests/test_gpu_dual_stream.py; the operands are those of tests/workspace_cases.py's grouped row at a K without a stream-K split."""
    from nunchaku_amd._C import ops
    from tests import workspace_cases as W

    case = W.GemmCase("grouped-rope", "min-alignment", 1, 512, 384, 256, fuse="rmsnorm_rope", grouped=True, streamk=False)
    o = case.build(5, dtype)
    plans = []

    def launch():
        res = case.run(o)
        plans.append(ops.gemm_last_plan())
        return res

    al, mv, res_a, res_m = run_pair(monkeypatch, G, launch, _gemm_spec)
    for p in plans:
        case.check_plan(p)
    assert plans[0] == plans[1]
    moved = {f for _, f in mv.ops}
    assert moved == {"out", "out_vt", "bias", "bias2", "norm_q", "norm_k", "norm_q2", "norm_k2"}, moved
    assert_same(al, mv, f"grouped gemm {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_grouped_gelu_quant(dtype, monkeypatch):
    """the (128, plain) GELU_QUANT row with fixed-point sums as a grouped launch: rows >= 256 take a second weight set, whose bias2, next_smooth2 and
    next_lora_down2 move with the first set's vectors, oscales and lora_act_out.  Bit for bit against the aligned grouped launch, the low-rank sums included;
    grouped launches are held to separate ones by tests/test_gpu_fused_norm.py::test_flux_transformer_grouped_vs_separate_launches."""
    from nunchaku_amd import layout, mode
    from nunchaku_amd._C import ops
    from nunchaku_amd.ops.gemm import svdq_gemm_w4a4_cuda
    from tests.helpers import make_module
    from tests.workspace_cases import _ops_set

    case = _gemm_row("gelu_quant", 3, "q32", "plain")
    fuse, geometry, fmt, R, R2, M, K, N, ws, key = case
    run = T._GemmRun(case, dtype)
    m1, m2, td, M_pad = run.m1, run.m2, TORCH_DT[dtype], run.M_pad
    m1b = make_module(T._layer(K, N, R, 901, dtype), dtype)
    m2b = make_module(T._layer(N, 128, R2, 902, dtype), dtype, act_unsigned=True)
    m1b._ensure_layout()
    m2b._ensure_layout()
    second = dict(wgt=m1b.qweight, wscales=m1b.wscales, bias=m1b.bias, lora_up=m1b.proj_up, smooth_factor=m2b.smooth_factor, lora_down=m2b.proj_down)
    plans = []

    def launch():
        qh = torch.empty(layout.act_image_shape(M_pad, N), dtype=torch.uint8, device="cuda")
        sh = torch.empty(N // 64, M_pad, dtype=td, device="cuda")
        lh = torch.full((M_pad, R2), 12345, dtype=torch.int64, device="cuda")  # (junk: the op clears it)
        with _ops_set(gemm_geometry=geometry, gemm_use_workspace=ws), mode.deterministic_mode(run.level):
            svdq_gemm_w4a4_cuda(act=run.qx, wgt=m1.qweight, ascales=run.asc, wscales=m1.wscales, bias=m1.bias, lora_act_in=run.la, lora_up=m1.proj_up, qout=qh,
                                oscales=sh, smooth_factor=m2.smooth_factor, lora_down=m2.proj_down, lora_act_out=lh, split_rows=256, second=second)
        plans.append(ops.gemm_last_plan())
        return qh, sh, lh

    al, mv, res_a, res_m = run_pair(monkeypatch, G, launch, _gemm_spec)
    assert plans[0] == plans[1] and T._plan_key(plans[0]) == key[:2], plans
    assert {f for _, f in mv.ops} == {"bias", "bias2", "next_smooth", "next_smooth2", "next_lora_down", "next_lora_down2", "oscales", "lora_act_out"}
    assert same_bits(res_a[0], res_m[0]), "codes differ from the aligned launch"
    assert_same(al, mv, f"grouped GELU_QUANT gemm {dtype}")
    # the second set is in use: rows >= 256 differ from the launch with one weight set
    (qh1, _, _), _ = run.launch()
    torch.cuda.synchronize()
    rows = layout.unpack_act(res_a[0], N, unsigned=True)
    assert torch.equal(rows[:256], layout.unpack_act(qh1, N, unsigned=True)[:256]) and not torch.equal(rows[256:M], layout.unpack_act(qh1, N, unsigned=True)[256:M])


# =======================================================================================================================================
# 3. attention with the fused quantiser
# =======================================================================================================================================
def _attn_spec(a):
    K2, acc = a.H * 128 * 2, 8 if a.qlora_act_format else 4
    return {
        "qsmooth": Op("in", K2), "qsmooth2": Op("in", K2), "qlora_down": Op("in", a.qR * K2), "qlora_down2": Op("in", a.qR * K2),
        "qscales": Op("out", (a.H * 128 // 64) * a.L * 2), "qlora_act": Op("acc", a.L * a.qR * acc, 4, off=acc),
    }


class _Attn:
    """the operands and the launch of tests/workspace_cases.py's AttentionCase, with an optional second parameter set for rows >= 256"""

    def __init__(self, L, H, qR, q32, joint, dtype):
        from nunchaku_amd._C import mark_amd
        from tests import workspace_cases as W

        self.case = W.AttentionCase(f"min-alignment-L{L}", "min-alignment", 1, L, H, qR=qR, q32=q32)
        self.o = self.case.build(7, dtype)
        self.L, self.H, self.qR, self.q32, self.joint = L, H, qR, q32, joint
        if joint:
            g, td, K = torch.Generator(device="cuda").manual_seed(99), TORCH_DT[dtype], H * 128
            self.o["smooth2"] = mark_amd((torch.rand(K, device="cuda", generator=g) + 0.5).to(td))
            self.o["lora_down2"] = mark_amd((torch.randn(K, qR, device="cuda", generator=g) * 0.05).to(td))
        self.plans = []

    def launch(self):
        from nunchaku_amd._C import ops
        from tests.workspace_cases import _ops_set

        o, L, H = self.o, self.L, self.H
        td, K = o["qkv"].dtype, H * 128
        q, k = o["qkv"][:, :K].unflatten(1, (H, 128)), o["qkv"][:, K:2 * K].unflatten(1, (H, 128))
        res = {"qact": torch.zeros(L, K * 3 // 4, dtype=torch.uint8, device="cuda"), "qscales": torch.zeros(K // 64, L, dtype=td, device="cuda"),
               "lora_act": torch.zeros(L, self.qR, dtype=torch.int64 if self.q32 else torch.float32, device="cuda")}
        qd = dict(act=res["qact"], ascales=res["qscales"], lora_act=res["lora_act"], R=self.qR, smooth=o["smooth"], lora_down=o["lora_down"])
        if self.joint:
            qd.update(smooth2=o["smooth2"], lora_down2=o["lora_down2"], split_rows=256)
        with _ops_set(attention_geometry=1, attention_use_workspace=True, attention_split_lowrank=True, cache_packed_lowrank=True):
            ops.attention(q, k, o["vt"].unflatten(0, (H, 128)), None, 1.0 / math.sqrt(128), None, qd)
            self.plans.append(ops.attention_last_plan())
            ops.attention_workspace_status()
        return res


ATTN_RUNS = (  # (L, q32, joint, the launch keeps the fragment image of the factor)
    (256, False, False, False),   # the path that reads qlora_down itself, 8 bytes at a time
    (256, True, False, False),    # ... with fixed-point sums: bit equality
    (256, False, False, True),    # the image: qlora_down is not read, qsmooth is
    (512, True, True, False),     # both parameter sets (a split needs 256 rows on either side: L = 512 is the smallest such launch)
)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,q32,joint,image", ATTN_RUNS, ids=lambda v: str(v))
def test_attention_fused_quantiser(L, q32, joint, image, dtype, monkeypatch):
    """H = 2, qR = 32, 8 waves on the persistent schedule (the (8, 1) row of ATTN_CASES, with the quantiser of
    tests/test_gpu_attention.py::test_attention_fused_output_quantiser, which holds codes and scales to the stand-alone quantiser bit for bit and the
    low-rank sums to it; tests/test_gpu_attention_lowrank_image.py holds image and row loads to each other).  qsmooth(2), qlora_down(2) at + 8 bytes,
    qscales at + 2, qlora_act at + 4 (fp32) / + 8 (Q31.32).  fp32 sums over the heads are atomics: both launches within the bound of
    tests/workspace_cases.py (2e-5 |x| @ |D| + 1e-6 around the kernel's own 16-bit output times the factor)."""
    at = _Attn(L, 2, 32, q32, joint, dtype)

    def also(a):
        if not image:
            a.qlora_down_packed = a.qlora_down_packed2 = None
    al, mv, res_a, res_m = run_pair(monkeypatch, A, at.launch, _attn_spec, also=also)
    assert at.plans[0] == at.plans[1] and T.attn_plan_key(L, at.plans[0]) == ("attention_kernel", (8, 1)), at.plans
    what = f"attention L={L} q32={q32} joint={joint} image={image} {dtype}"
    assert same_bits(res_a["qact"], res_m["qact"]), f"{what}: codes differ from the aligned launch"
    assert {f for _, f in mv.ops} == {"qsmooth", "qlora_down", "qscales", "qlora_act"} | ({"qsmooth2", "qlora_down2"} if joint else set())
    assert_same(al, mv, what, gated=() if q32 else ("qlora_act",))
    if not q32:
        for name, Lc in (("aligned", al), ("moved", mv)):
            got = Lc.bytes_of((0, "qlora_act")).view(torch.float32).view(L, 32)
            at.case.check_bounded(at.o, {"lora_act": got})


# =======================================================================================================================================
# 4. the row passes, qk_norm_rope, pulid_ca: the fp32 buffers at + 8, rstd at + 4
# =======================================================================================================================================
ROW_M, ROW_C = D.ROW_M, D.ROW_WIDTHS[1]   # 6 rows of 200 columns: one full workgroup and half of one, a ragged pass
pairs = lambda rows: Op("out", rows * 8, 4)


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_gate_stats(dtype, monkeypatch):
    """tests/test_gpu_dispatch_classes.py::test_residual_gate_stats_every_width_class (and ..._grouped_...) hold these launches to residual_gate_ref"""
    from nunchaku_amd._C import ops

    probs = []
    for i, M in enumerate(D.ROW_M_PAIR):
        res, a, _, gate = D._row_inputs(M, ROW_C, dtype, seed=11 + i)
        probs.append((t16(res, dtype), t16(a, dtype), t16(gate, dtype), M))

    def launch(grouped):
        def fn():
            work = [(r.clone(), a, None, g, None, torch.zeros(M, 2, device="cuda")) for r, a, g, M in probs]
            (r1, a1, _, g1, _, s1), (r2, a2, _, g2, _, s2) = work
            ops.residual_gate_stats(r1, a1, None, g1, r1, s1, second=(r2, a2, None, g2, r2, s2) if grouped else None)
            return (r1, r2, s1, s2) if grouped else (r1, s1)
        return fn

    spec = lambda a: {"stats": pairs(a.M), "stats2": pairs(a.M2)}
    for grouped in (False, True):
        al, mv, res_a, res_m = run_pair(monkeypatch, "svdq_residual_gate_stats", launch(grouped), spec)
        n = 2 if grouped else 1  # (the statistics of the moved launch are in its windows: the wrapper's tensors behind them are not written)
        assert all(same_bits(x, y) for x, y in zip(res_a[:n], res_m[:n])) and {f for _, f in mv.ops} == ({"stats", "stats2"} if grouped else {"stats"})
        assert_same(al, mv, f"residual_gate_stats grouped={grouped} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_residual_diff_and_modulated_diff(dtype, monkeypatch):
    """tests/test_gpu_dispatch_classes.py::test_residual_diff_every_width_class and ::test_modulated_diff_every_width_class hold these launches to their
    restatements; partials and result at + 8, the statistics modulated_diff reads at + 8"""
    from nunchaku_amd._C import ops

    prev, base, cur = D._diff_inputs(ROW_M, ROW_C, dtype, seed=31)

    def diff():
        out, partials, result = torch.zeros_like(cur), torch.zeros(ROW_M, 2, device="cuda"), torch.zeros(8, device="cuda")
        ops.residual_diff(cur, base, prev, out, partials=partials, result=result)
        return (out, partials, result)

    spec = lambda a: {"partials": pairs(a.M + a.M2), "result": Op("out", 32, 4)}
    al, mv, res_a, res_m = run_pair(monkeypatch, "svdq_residual_diff", diff, spec)
    assert same_bits(res_a[0], res_m[0]) and {f for _, f in mv.ops} == {"partials", "result"}
    assert_same(al, mv, f"residual_diff {dtype}")

    rng = np.random.default_rng(41)
    x = t16(O.round16((3.0 + 0.5 * rng.standard_normal((ROW_M, ROW_C))).astype(np.float32), dtype), dtype)
    scale = t16(O.round16(1 + 0.3 * rng.standard_normal(ROW_C).astype(np.float32), dtype), dtype)
    shift = t16(O.round16(0.5 * rng.standard_normal(ROW_C).astype(np.float32), dtype), dtype)
    stats = torch.zeros(ROW_M, 2, device="cuda")
    ops.residual_gate_stats(x, None, None, None, None, stats)

    def mod():
        out, partials, result = torch.zeros_like(x), torch.zeros(ROW_M, 2, device="cuda"), torch.zeros(8, device="cuda")
        ops.modulated_diff(x, stats, scale, shift, prev, out, partials=partials, result=result)
        return (out, partials, result)

    spec = lambda a: {"stats": Op("in", a.M * 8, 4), "partials": pairs(a.M), "result": Op("out", 32, 4)}
    al, mv, res_a, res_m = run_pair(monkeypatch, "svdq_modulated_diff", mod, spec)
    assert same_bits(res_a[0], res_m[0]) and {f for _, f in mv.ops} == {"stats", "partials", "result"}
    assert_same(al, mv, f"modulated_diff {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_sandwich_norm_and_qk_norm_rope(dtype, monkeypatch):
    """tests/test_gpu_zimage_ops.py holds both to tests/zimage_ref.py bit for bit (sandwich: B, T = 2, 5 at C = 256; qk_norm_rope: T = 65, H = 3, L = 128);
    the reciprocal RMS values at + 8 (stats) and + 4 (rstd)"""
    from nunchaku_amd.ops import qk_norm_rope, sandwich_norm
    from tests import test_gpu_zimage_ops as ZO

    C = 256
    g = torch.Generator().manual_seed(C + 1)
    res, a = ZO._rand16((ZO.B, ZO.T, C), dtype, g).cuda(), ZO._rand16((ZO.B, ZO.T, C), dtype, g, 3.0).cuda()
    w, s = ZO._rand16((C,), dtype, g, 0.2, 1.0).cuda(), ZO._rand16((ZO.B, C), dtype, g, 0.3, 1.0).cuda()

    def sandwich():
        return sandwich_norm(res, a, w_post=w, gate=s, w_pre=w, scale=s, want_stats=True)

    al, mv, res_a, res_m = run_pair(monkeypatch, "svdq_sandwich_norm", sandwich, lambda a: {"stats": pairs(a.M)})
    assert all(same_bits(x, y) for x, y in zip(res_a[:2], res_m[:2])) and {f for _, f in mv.ops} == {"stats"}
    assert_same(al, mv, f"sandwich_norm {dtype}")

    T_, H, L = 65, 3, 128
    qkv, wq, wk, fc = ZO._qk_inputs(T_, H, L, dtype, seed=T_ * 10 + H)

    def qk():
        buf = qkv.cuda()
        vt = torch.zeros(H * 128, L + 128, dtype=qkv.dtype, device="cuda")
        _, rstd = qk_norm_rope(buf[:, :3 * H * 128], H, T_, vt=vt, want_rstd=True, norm_q=wq.cuda(), norm_k=wk.cuda(), freqs_cis=fc.cuda())
        return (buf, vt, rstd)

    al, mv, res_a, res_m = run_pair(monkeypatch, "svdq_qk_norm_rope", qk, lambda a: {"rstd": Op("out", a.T * 2 * a.H * 4, 4)})
    assert all(same_bits(x, y) for x, y in zip(res_a[:2], res_m[:2])) and {f for _, f in mv.ops} == {"rstd"}
    assert_same(al, mv, f"qk_norm_rope {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_sana_glue_and_pulid_ca(dtype, monkeypatch):
    """tests/test_gpu_sana_block.py::test_one_case_per_width_class holds the glue launch (2 x 3 rows, C = 376 of 512) to tests/sana_glue_ref.py,
    tests/test_gpu_pulid.py::test_each_stage_equals_the_restatement_from_its_own_input the identity cross-attention (T = 33, C = 256, H = 4, N = 5) to
    tests/pulid_ref.py; their row statistics at + 8: written by the one, read by the other"""
    from nunchaku_amd.ops import sana_glue
    from nunchaku_amd.ops.attention import pulid_ca
    from nunchaku_amd.ops.elementwise import residual_gate_stats
    from tests import pulid_ref
    from tests import test_gpu_pulid as PU
    from tests import test_gpu_sana_block as SB

    C_pad = 512
    inp = SB._inputs(2, 3, C_pad - 136, dtype, seed=1)
    d = SB.Device(inp, C_pad, dtype, used_rows=[5, SB.MSA[0], SB.MSA[1]])

    def glue():
        (_, out), (_, out_mod) = d.buffer(), d.buffer()
        _, _, stats = sana_glue(d.res, d.a, timestep=d.ts, gate_table=d.gtab, gate_row=5, mod_table=d.mtab, scale_row=SB.MSA[1], shift_row=SB.MSA[0],
                                channels=d.C, pad_to=C_pad, out=out, out_mod=out_mod, want_stats=True)
        return (out, out_mod, stats)

    al, mv, res_a, res_m = run_pair(monkeypatch, "svdq_sana_glue", glue, lambda a: {"stats": pairs(a.B * a.T)})
    assert all(same_bits(x, y) for x, y in zip(res_a[:2], res_m[:2])) and {f for _, f in mv.ops} == {"stats"}
    assert_same(al, mv, f"sana_glue {dtype}")

    Tn, C, H, N = 33, 256, 4, 5
    _, _, fold = PU._fold(C, H, N, dtype)
    x = pulid_ref.stream_inputs(Tn, C, Tn + N, PU.TD[dtype], "cuda", ld=C + 64)
    stats = residual_gate_stats(x, eps=1e-5)[1]

    def pulid():
        out = torch.zeros(Tn, C, dtype=PU.TD[dtype], device="cuda")
        _, probs = pulid_ca(x, fold, out_scale=0.7, stats=stats, out=out, return_probs=True)
        return (out, probs)

    al, mv, res_a, res_m = run_pair(monkeypatch, "svdq_pulid_ca", pulid, lambda a: {"stats": Op("in", a.T * 8, 4)})
    assert all(same_bits(x_, y) for x_, y in zip(res_a, res_m)) and {f for _, f in mv.ops} == {"stats"}
    assert_same(al, mv, f"pulid_ca {dtype}")


# =======================================================================================================================================
# 5. AWQ: scales, zeros, bias, out (and t) at the ledger's minimum: + 2 bytes, out of the GEMM at + 8
# =======================================================================================================================================
def _gemv_spec(a):
    groups = (a.K // 64) * a.N * 2
    return {"scales": Op("in", groups), "zeros": Op("in", groups), "bias": Op("in", a.N * 2), "out": Op("out", a.M * a.N * 2)}


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_awq(dtype, monkeypatch):
    """M = 1 (the LDS path) and M = 2 (the row-group path) at N = 20, K = 576, and a batched launch of two entries:
    tests/test_gpu_dispatch_classes.py::test_gemv_awq_every_m_and_both_single_row_paths holds the single launches to the oracle,
    ::test_gemv_awq_batched_ragged_entry_and_row_group_path the batched one to them"""
    from nunchaku_amd.ops.gemv import awq_gemv_w4a16_batched, awq_gemv_w4a16_cuda
    from tests.test_gpu_awq import _layer

    N, K = D.GEMV_SHAPES[0]
    q, s, z, bias = _layer(N, K, dtype, seed=N + K)
    kern, ts, tz, tb = torch.from_numpy(O.pack_awq_w4_ref(q)).cuda(), t16(s, dtype), t16(z, dtype), t16(bias, dtype)
    for m in (1, 2):
        x = t16(O.round16(np.random.default_rng(7 + m).standard_normal((m, K)).astype(np.float32), dtype), dtype)
        al, mv, _, _ = run_pair(monkeypatch, "svdq_gemv_awq", lambda: awq_gemv_w4a16_cuda(x, kern, ts, tz, m, N, K, bias=tb), _gemv_spec)
        assert {f for _, f in mv.ops} == {"scales", "zeros", "bias", "out"}
        assert_same(al, mv, f"gemv_awq M={m} {dtype}")
    layers = []
    for i, (n, chunks) in enumerate(D.GEMV_BATCHED_ENTRIES[:2]):
        lin = D._cheap_gemv_layer(n, 256, dtype, seed=300 + i)
        lin.out_chunks = chunks
        layers.append(lin)
    x = t16(np.random.default_rng(256).standard_normal((1, 256)).astype(np.float32), dtype)
    al, mv, _, _ = run_pair(monkeypatch, "svdq_gemv_awq_batched", lambda: awq_gemv_w4a16_batched(x, layers), _gemv_spec)
    assert {k for k in mv.ops} == {(i, f) for i in (0, 1) for f in ("scales", "zeros", "bias", "out")}
    assert_same(al, mv, f"gemv_awq_batched {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemv_awq_lora(dtype, monkeypatch):
    """r = 16 on N = 64, K = 256: tests/test_gpu_lora.py::test_gemv_lora_kernel_matches_the_twin holds the branch to its float64 twin; out (read, updated,
    written) and the scratch t at + 2 bytes"""
    from nunchaku_amd.ops.gemv import awq_gemv_w4a16_batched

    N, K, r = 64, 256, 16
    lin = D._cheap_gemv_layer(N, K, dtype, seed=300)
    rng = np.random.default_rng(20)
    down = O.round16(rng.standard_normal((r, K)).astype(np.float32) / np.sqrt(K), dtype)
    up = O.round16(rng.standard_normal((N, r)).astype(np.float32) * (0.5 / np.sqrt(r)), dtype)
    lin.set_lora(t16(down, dtype), t16(up, dtype), strength=0.75)
    x = t16(np.random.default_rng(5).standard_normal((1, K)).astype(np.float32), dtype)
    spec = lambda a: {"out": Op("acc", a.N * 2), "t": Op("out", a.r * 2)}
    al, mv, _, _ = run_pair(monkeypatch, "svdq_gemv_awq_lora_batched", lambda: awq_gemv_w4a16_batched(x, [lin]), spec)
    assert {f for _, f in mv.ops} == {"out", "t"}
    assert_same(al, mv, f"gemv_awq_lora {dtype}")
    # the branch did something: out is not the plain GEMV's
    lin.set_lora_strength(0.0)
    plain = awq_gemv_w4a16_batched(x, [lin])[0]
    assert not same_bits(mv.bytes_of((0, "out")).view(TORCH_DT[dtype]).view(1, N), plain)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,split", [(7, 256, 640, False), (8, 4096, 4096, True)])
def test_gemm_awq(M, N, K, split, dtype, monkeypatch):
    """two shapes of tests/test_gpu_awq_gemm.py::test_parity_with_float64_restatement, which holds them to the float64 restatement: (7, 256, 640) runs
    without a K-split, (8, 4096, 4096) splits K -- only then the reduce kernel runs, which stores out four elements (8 bytes) at a time.  out at
    + 8 bytes; scales, scaled_zeros and bias at + 2"""
    from nunchaku_amd import _lib
    from tests.test_gpu_awq_gemm import DT, gemm, make_layer

    planned = int(_lib.load().svdq_gemm_awq_workspace_bytes(M, N, K)) // (4 * M * N) or 1
    assert (planned > 1) == split, f"the planner splits ({M}, {N}, {K}) {planned} ways"
    qw, sc, zr = make_layer(N, K, DT[dtype], seed=M + N + K)
    x = torch.randn(M, K, device="cuda", generator=torch.Generator(device="cuda").manual_seed(M)).to(DT[dtype])
    bias = torch.randn(N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(N)).to(DT[dtype])
    groups = lambda a: Op("in", (a.K // 128) * a.N * 2)
    spec = lambda a: {"scales": groups(a), "scaled_zeros": groups(a), "bias": Op("in", a.N * 2), "out": Op("out", a.M * a.N * 2)}
    al, mv, _, _ = run_pair(monkeypatch, "svdq_gemm_awq", lambda: gemm(x, qw, sc, zr, bias=bias), spec)
    assert {f for _, f in mv.ops} == {"scales", "scaled_zeros", "bias", "out"}
    assert_same(al, mv, f"gemm_awq {M}x{N}x{K} {dtype}")
