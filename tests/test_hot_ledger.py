"""A ledger over the kernels on the hot path, as tests/test_dispatch_ledger.py is over the small ones: the template instantiations of the W4A4 GEMM, the
activation quantiser and attention that the built library holds (kernel names in the code objects' metadata notes, tools/isa_stats.kernel_resources --
names only, no instruction is looked at) against the instantiations the case tables of tests/test_gpu_hot_instantiations.py claim.  Whoever adds an
instantiation gets a failing test that names the one without a case; whoever drops a table row gets one that names the instantiation left unlaunched.

GEMM, quantiser and attention rows are witnessed by the library: every GEMM and attention launch asserts the plan it reports (the GEMM's plan is the host
function plan_gemm, which svdq_gemm_plan also answers without a GPU: tests/test_gemm_plan.py), and the quantiser rows ask svdq_quantize_plan, the host function
launch_quantize consumes (``quant_instantiation``; tests/test_addressing_reach.py pins its answers around the fast kernel's 2 GiB rule).  Its limit: the
4- / 8-wave attention kernels go through ``L % 256``, a restatement; if the launcher changes that rule and the table is not changed with it, the ledger reports
"reached" for a kernel the tables no longer launch."""
import math
import os
import re

import pytest

from tests import test_gpu_hot_instantiations as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"), reason="needs llvm-objdump")

I, B = r"Li(\d+)E", r"Lb([01])E"  # an int / a bool template argument in an Itanium name
KERNELS = {  # kernel -> (template arguments after DT, instantiations compiled)
    "gemm_w4a4_kernel": (I + I + B * 5, 58),        # FUSE, NW, LAQ, CARRY, RALL, HYB, SPLIT
    "gemm_w4a4_wt128_kernel": ("", 2),
    "lowrank_down_split_kernel": (I, 8),            # NB
    "quantize_kernel": (I + I + B, 20),             # RT32, OCC, GLU
    "quantize_kernel_v2": (B * 4, 24),              # LORA, LN, SMOOTH, MULTI
    "attention_kernel": (I + B, 6),                 # NW, PERSIST
    "attention_kernel64": (B + B, 6),               # PERSIST, MASK
}
DT = {0: "bf16", 1: "fp16"}  # SVDQ_BF16, SVDQ_FP16: every table is parametrised over T.DTYPES


@pytest.fixture(scope="module")
def kernel_names(built_lib):
    import importlib.util

    spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from nunchaku_amd import _lib

    return sorted(mod.kernel_resources(_lib.lib_path(), "_kernel"))


def compiled(names, kernel: str) -> set:
    """{(dtype, template arguments)} of ``kernel<DT, ...>``: <length>kernel I Li<dt>E ... E (the length prefix keeps ip_attention_kernel and its like out)"""
    found = [re.search(rf"(?<!\d){len(kernel)}{kernel}ILi(\d+)E{KERNELS[kernel][0]}E", n) for n in names]
    return {(int(m.group(1)), tuple(int(g) for g in m.groups()[1:])) for m in found if m}


def claimed(tables=T) -> dict:
    """kernel -> {template arguments} the case tables claim (the tables run every row in every dtype)"""
    out = {k: set() for k in KERNELS}
    for case in tables.GEMM_CASES:
        for kernel, args in tables.gemm_instantiations(case):
            out[kernel].add(args)
    for case in tables.QUANT_CASES:
        kernel, args = tables.quant_instantiation(case)
        out[kernel].add(args)
    for case in tables.ATTN_CASES:
        out[case[5][0]].add(case[5][1])
    return out


def reached(kernel: str, tables=T) -> set:
    return {(dt, args) for dt in DT for args in claimed(tables)[kernel]}


def fmt(kernel, s) -> str:
    return ", ".join(f"{kernel}<{', '.join([DT.get(dt, str(dt))] + [str(a) for a in args])}>" for dt, args in sorted(s))


def check(kernel, have, want):
    """the three ways the ledger fails, each naming the instantiation"""
    assert len(have) == KERNELS[kernel][1], f"{kernel}: {len(have)} instantiations in the library, the ledger knows {KERNELS[kernel][1]}: {fmt(kernel, have)}"
    assert not have - want, f"compiled and dispatched, but no case table launches: {fmt(kernel, have - want)}"
    assert not want - have, f"the case tables claim instantiations the library does not hold: {fmt(kernel, want - have)}"


def test_the_tables_run_both_dtypes():
    assert tuple(T.DTYPES) == tuple(DT.values())


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_every_instantiation_has_a_case(kernel_names, kernel):
    check(kernel, compiled(kernel_names, kernel), reached(kernel))


def test_all_124_instantiations_are_reached(kernel_names):
    total = sum(len(compiled(kernel_names, k) & reached(k)) for k in KERNELS)
    print(f"hot-path ledger: {total} instantiations compiled and reached by the case tables")
    assert [KERNELS[k][1] for k in KERNELS] == [58, 2, 8, 20, 24, 6, 6] and total == 124


def test_the_ledger_names_what_is_missing(kernel_names):
    """the ledger's own failure modes: a table without one of its rows, and a library with one more instantiation, each reported by name"""
    class Without:  # the tables minus the only NB = 3 row
        DTYPES, QUANT_CASES, ATTN_CASES = T.DTYPES, T.QUANT_CASES, T.ATTN_CASES
        GEMM_CASES = tuple(c for c in T.GEMM_CASES if not (c[9][1] == "split_down" and c[4] == 96))
        gemm_instantiations, quant_instantiation = staticmethod(T.gemm_instantiations), staticmethod(T.quant_instantiation)

    k = "lowrank_down_split_kernel"
    with pytest.raises(AssertionError, match=r"no case table launches: lowrank_down_split_kernel<bf16, 3>, lowrank_down_split_kernel<fp16, 3>"):
        check(k, compiled(kernel_names, k), reached(k, Without))
    more = kernel_names + ["_ZN4svdq25lowrank_down_split_kernelILi0ELi6EEEvPKNS_4HalfIXT_EE2V8ES5_S5_Pfiiii"]
    with pytest.raises(AssertionError, match=r"9 instantiations in the library, the ledger knows 8"):
        check(k, compiled(more, k), reached(k))
    k = "attention_kernel64"
    more = [n.replace("18attention_kernel64ILi0ELb0ELb1E", "18attention_kernel64ILi0ELb1ELb1E") for n in kernel_names]
    with pytest.raises(AssertionError, match=r"no case table launches: attention_kernel64<bf16, 1, 1>"):
        check(k, compiled(more, k), reached(k))

    class Beyond(Without):  # ... plus a row that claims a masked persistent kernel, which does not exist
        GEMM_CASES = T.GEMM_CASES
        ATTN_CASES = T.ATTN_CASES + ((512, 2, True, True, (300,), ("attention_kernel64", (1, 1))),)

    with pytest.raises(AssertionError, match=r"library does not hold: attention_kernel64<bf16, 1, 1>, attention_kernel64<fp16, 1, 1>"):
        check(k, compiled(kernel_names, k), reached(k, Beyond))


def test_every_table_row_counts():
    """no row of the GEMM and attention tables can go without the ledger noticing, but for the rows kept for a second shape of one instantiation"""
    spare = {"gemm": 0, "attention": 0}
    for i, case in enumerate(T.GEMM_CASES):
        rest = T.GEMM_CASES[:i] + T.GEMM_CASES[i + 1:]
        spare["gemm"] += all(inst in {x for c in rest for x in T.gemm_instantiations(c)} for inst in T.gemm_instantiations(case))
    for i, case in enumerate(T.ATTN_CASES):
        spare["attention"] += any(c[5] == case[5] for c in T.ATTN_CASES[:i] + T.ATTN_CASES[i + 1:])
    # carry: rank 32 with and rank 16 without a workspace; hybrid carry: rank 48 and 80; solo carry: rank 48 and 128; wave tile: rank 0 and 32
    assert spare == {"gemm": 8, "attention": 0}, spare


def test_the_tables_keep_their_edge_cases():
    """what an instantiation needs besides being reached"""
    gemm = T.GEMM_CASES
    assert all(c[5] % 256 for c in gemm), "every GEMM row has a ragged last row block"
    assert all(c[5] > 256 for c in gemm), "... and more than one row block"
    assert {math.ceil(c[4] / 32) for c in gemm if c[9][1] == "split_down"} == {2, 3, 4, 5}, "every NB of the split kernel"
    assert {c[3] for c in gemm if c[9][1] == "wave_tile_128"} == {0, 32}
    assert all(c[7] // 128 >= 4 for c in gemm if "carry" in c[9][1]), "a carry sums at least four column tiles per row block"
    rowrun = [c for c in gemm if c[5] > 512]
    assert {c[9][1:] for c in rowrun} == {("carry", True), ("hybrid_carry", False)} and all((math.ceil(c[5] / 256) * 256 // 256) * (c[7] // 128) >= 512 for c in rowrun)
    assert {c[2] for c in gemm} == {"f32", "q32", "q32_runs"}
    quant = T.QUANT_CASES
    assert all(c[6] % 256 for c in quant), "every quantiser row has a ragged M"
    large = [c for c in quant if c[8] == T.LARGE_GRID[2]]
    assert {c[0] for c in large} == {0, 32, 64, 128} and all(T.quant_grid(c[8], c[7]) == (8, 2) for c in large), "the multi-slice large-grid rows of the general kernel"
    assert any(c[8] > 262144 and T.quant_instantiation(c)[0] == "quantize_kernel_v2" for c in quant), "more than 8192 row tiles"
    assert sum(1 for c in quant if c[4]) == 5 and any(c[4] and c[0] == 96 and c[2] for c in quant), "the grouped rows"
    assert {c[0] for c in quant if c[3]} == {0, 32, 64, 128, 176}, "fuse_glu at every rank class"
    assert any(c[5] == "q32" for c in quant)
    attn = T.ATTN_CASES
    assert any(c[0] % 256 for c in attn) and any(c[4] for c in attn) and T.ATTN_H == 2
