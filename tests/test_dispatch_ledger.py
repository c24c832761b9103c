"""A ledger over the shape-class dispatch of the small kernels: the template instantiations the built library holds (kernel names in the
code objects' metadata notes, tools/isa_stats.kernel_resources -- names only, no instruction is looked at) against the classes the case
tables of tests/test_gpu_dispatch_classes.py reach.  Whoever adds an instantiation (NV = 10, BM = 256) gets a failing test that names the
one without a case; whoever drops a table row gets one that names the instantiation left unlaunched.

Its limit: it trusts the class rules restated below (``CLASS_RULES``).  If a launcher changes how it maps a shape to an instantiation and
the rule here is not changed with it, the ledger reports "reached" for a kernel the tables no longer launch.  The rules live in
csrc/row_pass.h (``for_row_class``: ``(C + 511) / 512``, for the three row kernels), gemv_awq.hip (``M``), gemm_awq.hip (``awq_plan``) and
ip_attention.hip (``(N + 31) / 32``)."""
import math
import os
import re

import pytest

from tests import test_gpu_dispatch_classes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")

ROW_CLASS = lambda C: math.ceil(C / 512)
CLASS_RULES = {  # kernel -> (instantiations compiled, the variants its tables reach)
    "residual_kernel": (24, lambda: {ROW_CLASS(C) for C in T.ROW_WIDTHS}),
    "residual_diff_kernel": (24, lambda: {ROW_CLASS(C) for C in T.ROW_WIDTHS}),
    "modulated_diff_kernel": (24, lambda: {ROW_CLASS(C) for C in T.ROW_WIDTHS}),
    "gemv_awq_kernel": (16, lambda: {M for M, _, _ in T.GEMV_SINGLE}),
    "gemm_awq_kernel": (6, lambda: {32 if M <= 32 else 64 if M <= 64 else 128 for M, _, _, _ in T.AWQ_GEMM_CASES}),
    "ip_attention_kernel": (16, lambda: {math.ceil(N / 32) for _, _, N in T.IP_CASES + T.IP_PROBE_COVERED + T.IP_MULTI_TILE}),
}
DT = {0: "bf16", 1: "fp16"}  # SVDQ_BF16, SVDQ_FP16: every table runs both (tests loop or parametrise over T.DTYPES)


@pytest.fixture(scope="module")
def kernel_names(built_lib):
    import importlib.util

    spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from nunchaku_amd import _lib

    return sorted(mod.kernel_resources(_lib.lib_path(), "_kernel"))


def compiled(names, kernel: str) -> set:
    """{(dtype, variant)} of ``kernel<DT, V>`` from the Itanium names: <length>kernel I Li<dt>E Li<v>E E"""
    found = [re.search(rf"(?<!\d){len(kernel)}{kernel}ILi(\d+)ELi(\d+)EE", n) for n in names]
    return {(int(m.group(1)), int(m.group(2))) for m in found if m}


def reached(kernel: str) -> set:
    return {(dt, v) for dt in DT for v in CLASS_RULES[kernel][1]()}


def test_the_tables_run_both_dtypes():
    assert tuple(T.DTYPES) == tuple(DT.values())


@pytest.mark.parametrize("kernel", sorted(CLASS_RULES))
def test_every_instantiation_has_a_case(kernel_names, kernel):
    have, want = compiled(kernel_names, kernel), reached(kernel)
    fmt = lambda s: ", ".join(f"{kernel}<{DT.get(dt, dt)}, {v}>" for dt, v in sorted(s))
    assert len(have) == CLASS_RULES[kernel][0], f"{kernel}: {len(have)} instantiations in the library, the ledger knows {CLASS_RULES[kernel][0]}: {fmt(have)}"
    assert not have - want, f"compiled and dispatched, but no case table launches: {fmt(have - want)}"
    assert not want - have, f"the case tables expect instantiations the library does not hold: {fmt(want - have)}"


def test_all_110_instantiations_are_reached(kernel_names):
    total = sum(len(compiled(kernel_names, k) & reached(k)) for k in CLASS_RULES)
    print(f"dispatch ledger: {total} instantiations compiled and reached by the case tables")
    assert total == 110


def test_the_tables_keep_their_edge_cases():
    """what a class needs besides being reached: the row kernels a full AND a ragged last pass per class, the image-prompt kernel a full AND a
    ragged last key tile for the classes that had no case before, the GEMV every M at every shape, the GEMM every split count"""
    for nv in T.ROW_NV:
        mine = [C for C in T.ROW_WIDTHS if ROW_CLASS(C) == nv]
        assert any(C % 512 == 0 for C in mine) and any(C % 512 and C % 512 < 512 - 8 for C in mine), f"NV = {nv}: widths {mine}"
    for nkt in (3, 5, 6):
        mine = [N for _, _, N in T.IP_CASES if math.ceil(N / 32) == nkt]
        assert any(N % 32 == 0 for N in mine) and any(N % 32 for N in mine), f"NKT = {nkt}: key counts {mine}"
    assert {math.ceil(N / 32) for _, _, N in T.IP_PROBE_COVERED} == {1, 2, 4, 7, 8}, "the selection probe on the classes test_gpu_ip_attention launches"
    assert {T.ip_grid(*c)[1:] for c in T.IP_MULTI_TILE} == {(2, 2), (1, 3)}, "the tile loop with two workgroups per head and with one"
    assert {(m, n, k) for n, k in T.GEMV_SHAPES for m in range(1, 9)} <= set(T.GEMV_SINGLE), "every M at the ragged-N and at the one-chunk shape"
    assert {(1, 64, 8192), (1, 64, 8256)} <= set(T.GEMV_SINGLE) and set(T.GEMV_BATCHED_K) == {256, 8256}, "both M = 1 paths, single and batched"
    assert {s for _, _, _, s in T.AWQ_GEMM_CASES} == {1, 2, 4, 16} and any(K == 128 for _, _, K, _ in T.AWQ_GEMM_CASES), "split counts, one K-step"
    assert sum(1 for M, _, _, _ in T.AWQ_GEMM_CASES if 32 < M <= 64) == 3, "BM = 64: unsplit, two uneven slices, four slices"
