"""svdq_gemm_plan: which kernel, grid, schedule and packed images a W4A4 GEMM launch takes -- host only, no GPU needed.

tests/golden/gemm_plans.npz holds the dispatch of commit e26481b (the parent of the change that gave the rule its one home, plan_gemm), recorded on a machine
without a GPU: there device_cus() answers 256, the MI355X's count, so every row is a decision for cus = 256.  That recording had to call svdq_gemm_w4a4 itself with
made-up addresses and read svdq_gemm_last_plan (harmless only where no device exists: the launch fails after the dispatch ran).  Since svdq_gemm_plan exists the
table is regenerated safely anywhere: `python tests/test_gemm_plan.py` sweeps the same axes through the query and rewrites the file -- do that, and read the
diff of the class counts it prints, when a rule or threshold is changed on purpose.

Columns (int32): the twelve inputs COLUMNS[:12], then the eight words of svdq_gemm_last_plan {tile rows, variant, grid, stream-K groups, row-run length,
lora_act_in packed, lora_up packed, dynamic tile queue}."""
import ctypes as C
import itertools
import os

import numpy as np

from nunchaku_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plans.npz")
COLUMNS = ("M_pad", "N", "K", "fuse", "geometry", "R", "R2", "lora_act_format", "workspace", "grouped", "caller_packed", "dtype",
           "tile_rows", "variant", "grid", "sk_gs", "rowrun", "la_packed", "lu_packed", "dynamic")
CUS = 256
WS_NONE, WS_BASE, WS_FOR = 0, 1, 2  # no workspace | svdq_gemm_workspace_bytes() | svdq_gemm_workspace_bytes_for(args)

# the sweep: small, 1296 tiles (the geometry-2 rule), long K (stream-K, the wave tile) on both sides of its K = 8192 threshold, the grouped Qwen-Image fc1,
# N % 256 != 0 (no split down projection), fewer tiles than CUs, a partial last round
SHAPES = [(256, 128, 128), (4608, 9216, 3072), (4608, 3072, 12288), (6400, 12288, 3072), (4608, 12288, 3072), (4096, 3072, 3072), (512, 3072, 12288),
          (4608, 3200, 3072), (4608, 3072, 8192), (4608, 3072, 7168), (2560, 1152, 2048)]
RANKS = [(0, 0), (32, 0), (0, 32), (32, 32), (16, 16), (48, 48), (64, 64), (96, 96), (128, 128), (160, 160), (176, 176), (256, 256), (128, 32), (32, 128),
         (128, 48), (48, 96), (128, 160)]


def plan_args(M_pad, N, K, fuse, geometry, R, R2, fmt, workspace, grouped, caller_packed, dtype, lib=None):
    """svdq_gemm_args of a row: made-up aligned addresses (the plan reads their alignment and which are NULL, never what they point to)"""
    lib = lib or _lib.load()
    a = _lib.GemmArgs()
    a.act, a.wgt, a.ascales, a.wscales = 0x10000000, 0x20000000, 0x30000000, 0x31000000
    a.M, a.M_pad, a.N, a.K, a.R, a.R2, a.ldo = M_pad - 3, M_pad, N, K, R, R2, N
    a.dtype, a.fuse, a.geometry, a.lora_act_format = dtype, fuse, geometry, fmt
    if R > 0:
        a.lora_act_in, a.lora_up = 0x40000000, 0x41000000
    if fuse == _lib.FUSE_GELU_QUANT:
        a.qout, a.oscales, a.next_smooth = 0x50000000, 0x51000000, 0x52000000
        if R2 > 0:
            a.next_lora_down, a.lora_act_out = 0x53000000, 0x54000000
    else:
        a.out = 0x60000000
    if fuse == _lib.FUSE_RMSNORM_ROPE:
        a.norm_q, a.norm_k, a.rotary_emb = 0x61000000, 0x61001000, 0x62000000
    if grouped:
        a.wgt2, a.wscales2, a.split_rows = 0x70000000, 0x71000000, 256
        a.lora_up2 = 0x72000000 if R > 0 else 0
        if fuse == _lib.FUSE_GELU_QUANT:
            a.next_smooth2 = 0x73000000
            a.next_lora_down2 = 0x74000000 if R2 > 0 else 0
        if fuse == _lib.FUSE_RMSNORM_ROPE:
            a.norm_q2, a.norm_k2 = 0x75000000, 0x75001000
    if caller_packed:
        a.lora_up_packed = 0x78000000 if R > 0 else 0
        if fuse == _lib.FUSE_GELU_QUANT and R2 > 0:
            a.next_lora_down_packed = 0x79000000
            a.next_lora_down_packed2 = 0x7a000000 if grouped else 0
    if workspace != WS_NONE:
        a.workspace = 0x100000000
        a.workspace_bytes = lib.svdq_gemm_workspace_bytes() if workspace == WS_BASE else lib.svdq_gemm_workspace_bytes_for(C.byref(a))
    return a


def sweep():
    """every input row of the table.  Three full crosses -- the thinning keeps every variant x tile height and every combination of the three flags (asserted
    below): all of shape x fuse x geometry x ranks x workspace for the default format, one weight set, bf16; the format, grouped and caller-packed axes crossed
    with each other on the geometries a model run or a test asks for by name (0, 6, 7, 8); fp16 on geometry 0."""
    for (M_pad, N, K), fuse, (R, R2), ws in itertools.product(SHAPES, range(4), RANKS, (WS_NONE, WS_BASE, WS_FOR)):
        for geometry in range(9):
            yield M_pad, N, K, fuse, geometry, R, R2, _lib.LORA_ACT_F32, ws, 0, 0, _lib.SVDQ_BF16
        for geometry, fmt, grouped, packed in itertools.product((0, 6, 7, 8), range(3), (0, 1), (0, 1)):
            if fmt or grouped or packed:
                yield M_pad, N, K, fuse, geometry, R, R2, fmt, ws, grouped, packed, _lib.SVDQ_BF16
        yield M_pad, N, K, fuse, 0, R, R2, _lib.LORA_ACT_F32, ws, 0, 0, _lib.SVDQ_FP16


def query(lib, row, cus=CUS):
    out = (C.c_int32 * 8)()
    rc = lib.svdq_gemm_plan(C.byref(plan_args(*row, lib=lib)), cus, out)
    return rc, list(out)


def test_every_recorded_launch_still_takes_the_kernel_grid_and_images_it_took(built_lib):
    """tests/golden/gemm_plans.npz: dispatch of parent commit e26481b at cus = 256 (module docstring); svdq_gemm_plan must give the same eight words for every row"""
    lib = _lib.load()
    table = np.load(GOLDEN)["plans"]
    assert table.dtype == np.int32 and table.shape[1] == len(COLUMNS) and len(table) > 30000
    # what the table must reach to mean anything: every variant at each tile height it exists at, every combination of the two packed flags and the queue flag
    classes = {(int(v), int(t)) for t, v in np.unique(table[:, 12:14], axis=0)}
    assert classes == {(0, 256), (0, 128), (1, 256), (2, 256), (2, 128), (3, 256), (4, 128), (5, 256), (6, 256)}
    flags = {tuple(int(x) for x in f) for f in np.unique(table[:, 17:20], axis=0)}
    assert flags == {(0, 0, 0), (0, 0, 1), (1, 0, 0), (1, 1, 0), (1, 1, 1)}  # (lora_up is packed only beside lora_act_in; the solo-carry kernel has no queue)
    bad = []
    for row in table.tolist():
        rc, plan = query(lib, row[:12])
        if rc != 0 or plan != row[12:]:
            bad.append((dict(zip(COLUMNS, row)), rc, plan))
    assert not bad, f"{len(bad)} of {len(table)} launches changed their plan; first: {bad[0]}"


def test_the_plan_query_refuses_what_the_launch_refuses(built_lib):
    lib = _lib.load()
    ok = (4608, 3072, 3072, _lib.FUSE_NONE, 0, 32, 0, 0, WS_BASE, 0, 0, _lib.SVDQ_BF16)
    out = (C.c_int32 * 8)(*([-1] * 8))

    def both(**kw):
        a = plan_args(*ok, lib=lib)
        for k, v in kw.items():
            setattr(a, k, v)
        rc = lib.svdq_gemm_plan(C.byref(a), CUS, out)
        msg = lib.svdq_last_error()
        # (without a device the launch of a valid call fails with SVDQ_E_HIP after validation; with one, made-up addresses must not be launched)
        assert rc == 0 or lib.svdq_gemm_w4a4(C.byref(a), None) == rc
        return rc, msg

    assert both()[0] == 0 and list(out)[:2] == [256, 0]
    for kw, word in ((dict(M_pad=4608 + 128), b"M_pad"), (dict(R=24), b"R=24"), (dict(fuse=_lib.FUSE_RMSNORM_ROPE, norm_q=0x1000, norm_k=0x2000, rotary_emb=0x3000, N=3200, ldo=3200), b"3*128"),
                     (dict(lora_up=0x41000008), b"16-byte aligned"), (dict(geometry=9), b"geometry"), (dict(act=0), b"required"), (dict(variant=1), b"variant"),
                     (dict(wgt2=0x70000000), b"grouped"), (dict(workspace_bytes=-1), b"workspace")):
        out[:] = [-1] * 8
        rc, msg = both(**kw)
        assert rc == 1 and word in msg and list(out) == [-1] * 8, (kw, rc, msg)
    assert lib.svdq_gemm_plan(None, CUS, out) == 1 and lib.svdq_gemm_plan(C.byref(plan_args(*ok, lib=lib)), CUS, None) == 1
    assert lib.svdq_gemm_plan(C.byref(plan_args(*ok, lib=lib)), -8, out) == 1 and lib.svdq_gemm_plan(C.byref(plan_args(*ok, lib=lib)), 257, out) == 1
    # cus = 0: the device's count (256 where there is none); a smaller chip gets a smaller grid
    assert query(lib, ok, 0)[0] == 0
    assert query(lib, ok, 64)[1][2] <= 64 < query(lib, ok, 256)[1][2]


def test_the_plan_is_split_down_exactly_where_the_workspace_query_adds_the_image(built_lib):
    """the rows of test_host_logic.py::test_gemm_workspace_bytes_for_the_split_low_rank_down: a workspace of svdq_gemm_workspace_bytes_for() bytes runs the split
    low-rank down projection (variant 5) exactly when that size exceeds the base -- one predicate answers both"""
    lib = _lib.load()
    base = lib.svdq_gemm_workspace_bytes()
    out = (C.c_int32 * 8)()
    rows = [dict(), dict(R2=160, R=144), dict(M_pad=6400, grouped=1), dict(R2=64), dict(R2=48, R=48), dict(R2=32), dict(R2=176), dict(R=32), dict(R=176),
            dict(M_pad=256, N=1024), dict(M_pad=256, N=1024, geometry=7), dict(N=12288 + 128), dict(geometry=1), dict(geometry=6), dict(fmt=_lib.LORA_ACT_Q32),
            dict(fuse=_lib.FUSE_NONE)]
    grew = 0
    for kw in rows:
        row = dict(M_pad=4608, N=12288, K=3072, fuse=_lib.FUSE_GELU_QUANT, geometry=0, R=128, R2=128, fmt=_lib.LORA_ACT_F32, workspace=WS_FOR, grouped=0,
                   caller_packed=0, dtype=_lib.SVDQ_BF16)
        row.update(kw)
        a = plan_args(**row, lib=lib)
        assert lib.svdq_gemm_plan(C.byref(a), CUS, out) == 0
        assert (out[1] == 5) == (a.workspace_bytes > base), (kw, list(out))
        grew += a.workspace_bytes > base
        a.workspace_bytes = base  # the base size is never an error: the same launch without the image takes another kernel
        assert lib.svdq_gemm_plan(C.byref(a), CUS, out) == 0 and out[1] != 5
    assert grew == 6


def _regenerate():
    lib = _lib.load()
    rows = []
    for row in sweep():
        rc, plan = query(lib, row)
        if rc == 0:
            rows.append(list(row) + plan)
    table = np.array(rows, np.int32)
    np.savez_compressed(GOLDEN, plans=table)
    for (t, v), n in zip(*np.unique(table[:, 12:14], axis=0, return_counts=True)):
        print(f"variant {v} on {t}-row tiles: {n} rows")
    print(f"{len(table)} rows, {os.path.getsize(GOLDEN)} bytes -> {GOLDEN}")


if __name__ == "__main__":
    _regenerate()
