"""tests/workspace_cases.py replayed on the host for 256 compute units (svdq_gemm_schedule_ex, svdq_gemm_plan, svdq_attention_schedule, svdq_attention_plan and
the workspace-size queries; no GPU): every row is the schedule class its name says, and no class has lost its row.  A row that stops being its class --
a changed heuristic, a moved threshold -- fails here by name: move the row to the smallest shape that is the class again, do not relax the assertion."""
import ctypes as C

import numpy as np
import pytest

from nunchaku_amd import _lib
from tests import workspace_cases as W
from tests.test_gemm_plan import plan_args

DT_CODES = (_lib.SVDQ_BF16, _lib.SVDQ_FP16)


def test_the_table_keeps_one_row_per_class():
    assert tuple(c.cls for c in W.CASES) == W.CLASSES and len(set(W.CLASSES)) == len(W.CLASSES)
    assert {c.kind for c in W.CASES} == set(W.KINDS)
    assert all(name in W.BY_NAME for name in W.CHAIN)
    from nunchaku_amd import _C

    assert set(_C._PLAIN_KINDS) == {"awq", "linear_attention"}, "a new scratch-only kind needs a row"


def _gemm_plan(lib, case, dt):
    a = plan_args(*case.plan_row(dt), lib=lib)
    out = (C.c_int32 * 8)()
    assert lib.svdq_gemm_plan(C.byref(a), W.CUS, out) == 0, lib.svdq_last_error()
    from nunchaku_amd._C import _Ops

    return {"tile_rows": out[0], "variant": _Ops.PLAN_VARIANTS[out[1]], "grid": out[2], "streamk_groups": out[3], "rowrun": out[4],
            "lora_act_packed": bool(out[5]), "lora_up_packed": bool(out[6]), "dynamic_queue": bool(out[7])}


@pytest.mark.parametrize("case", W.of_kind("gemm"), ids=repr)
def test_gemm_rows_are_the_class_they_are_named_for(built_lib, case):
    lib = _lib.load()
    for dt in DT_CODES:
        plan = _gemm_plan(lib, case, dt)
        case.check_plan(plan)  # the assertion the GPU tests make on svdq_gemm_last_plan
    if isinstance(case, W.GeluQuantCase):
        assert (plan["variant"] == "split_down") == (case.name == "split-down")
        a = plan_args(*case.plan_row(DT_CODES[0]), lib=lib)
        grows = lib.svdq_gemm_workspace_bytes_for(C.byref(a)) > lib.svdq_gemm_workspace_bytes()
        assert grows == (case.name == "split-down"), "the split down projection is the launch that asks for a larger workspace"
        return
    seg = W.gemm_segments(case)
    KP, tile = case.K // 128, (256 if case.replay_geometry == 1 else 128)
    tiles, slots = (case.M_pad // tile) * (case.N // 128), W.CUS * case.replay_geometry
    assert tile == plan["tile_rows"]
    partial = seg[(seg[:, 2] > 0) | (seg[:, 3] < KP)]
    if case.streamk:
        assert len(partial) > 0, "no tile is split along K"
        owners = partial[partial[:, 3] == KP]
        assert len(owners) > 0 and (owners[:, 5] >= 1).all(), "every owner of a split tile waits for at least one contributor"
        assert (partial[partial[:, 3] < KP][:, 4] >= 0).all(), "a contributor publishes into a slab"
        assert plan["grid"] == seg[:, 0].max() + 1
    else:
        assert len(partial) == 0 and plan["streamk_groups"] == 0
    if case.name == "sk256-1tile":
        assert tiles == 1 and plan["grid"] == 2
    if case.name in ("sk256-3tiles", "sk-q32", "rope-sk"):
        assert tiles == 3 and len(np.unique(partial[:, 1])) == 3
    if case.name == "sk256-rounds":
        grid = plan["grid"]
        assert tiles > slots and (partial[:, 1] >= grid).any(), "a split tile whose id is not its flag index"
        assert (np.bincount(seg[:, 1], minlength=tiles) == 1)[: tiles - tiles % slots].all(), "the whole rounds run whole tiles"
    if case.name == "sk128":
        assert tiles == 2 and plan["tile_rows"] == 128
    if case.name == "sk-grouped":
        assert tiles == 2 and case.grouped
    if case.name.startswith("dyn"):
        assert tiles > slots and plan["dynamic_queue"] and plan["grid"] == slots
        assert case.K == 128, "one K-step: nothing to split"
    if case.name == "all-rank":
        assert plan["lora_act_packed"] and not plan["lora_up_packed"]


def test_stream_k_starts_at_3712(built_lib):
    """the hand-derived threshold of the table: K = 3712 is the smallest K at which a remainder tile is split, K = 3072 never splits"""
    lib = _lib.load()
    splits = lambda K: lib.svdq_gemm_schedule_ex(256, 128, K, W.CUS, 1, 1, None, 0) > 1
    assert splits(3712) and not splits(3584) and not splits(3072)


@pytest.mark.parametrize("case", W.of_kind("attention"), ids=repr)
def test_attention_rows_are_the_class_they_are_named_for(built_lib, case):
    lib = _lib.load()
    n = lib.svdq_attention_schedule(case.L, case.H, W.CUS, None, 0)
    assert n > 0, "runs on the plain grid"
    buf = (C.c_int32 * (6 * n))()
    assert lib.svdq_attention_schedule(case.L, case.H, W.CUS, buf, n) == n
    seg = np.ctypeslib.as_array(buf).reshape(n, 6)
    contributors = seg[seg[:, 4] >= 0]
    assert len(contributors) > 0 and (contributors[:, 2] > 0).all(), "no contributor record"
    assert (seg[(seg[:, 4] < 0) & (seg[:, 3] < case.L // 64)][:, 5] >= 0).all(), "an owner of a split task names its last contributor"
    groups = int(seg[:, 0].max()) + 1
    assert groups == {"att-2wg": 2, "att-24wg": 24}.get(case.name, groups)
    plan = (C.c_int32 * 4)()
    a = case.args(_lib)
    assert lib.svdq_attention_plan(C.byref(a), plan) == 0, lib.svdq_last_error()
    assert plan[0] == max(case.geometry, 1) and plan[1] == 0, list(plan)
    base = lib.svdq_attention_workspace_bytes()
    want = lib.svdq_attention_workspace_bytes_for(C.byref(a))
    assert (want > base) == case.split, "the split fused quantiser is the launch that asks for room behind the slabs"
    if case.split:
        assert (case.H * 128) % 256 == 0 and 48 <= case.qR <= 160
        assert want - base >= case.L * case.H * 128 * 2, "packed factor + the 16-bit row image"
    if case.name == "att-mask":
        assert case.kv_valid is not None and case.geometry == 1
    if case.name == "att-g2":
        assert case.prescaled and case.geometry == 2 and case.kv_valid is None and case.L % 256 == 0


def test_plain_scratch_rows_use_their_scratch(built_lib):
    lib = _lib.load()
    for case in W.of_kind("awq"):
        assert int(lib.svdq_gemm_awq_workspace_bytes(case.M, case.N, case.K)) // (4 * case.M * case.N) == case.splits, case
    assert {c.splits for c in W.of_kind("awq")} == {2, 4, 16}
    for case in W.of_kind("linear_attention"):
        assert case.T > 256 and case.T % 256, "more than one chunk, the last ragged"
        assert lib.svdq_linear_attention_workspace_bytes(C.byref(case.args(_lib))) >= case.B * case.H * math_ceil(case.T, 256) * 33 * 32 * 4


def math_ceil(a, b):
    return -(-a // b)
