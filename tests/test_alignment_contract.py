"""The alignment every entry point admits, pinned on the host -- no GPU, nothing is launched.

``LEDGER`` has a row for every pointer and every stride field of the args structs of the entry points in ``ENTRY_POINTS``: the alignment validation admits
(bytes for a pointer, elements for a stride) and the widest access the kernels make through the field, with the source line that shows it (read, not
measured; ``test_the_cited_lines_say_what_the_ledger_says`` keeps the citations from rotting).  For each row validation admits the field at exactly that
alignment and refuses it at half of it.  The addresses are made up and never dereferenced: the plan queries (``svdq_gemm_plan``, ``svdq_quantize_plan``)
validate as the launch does and launch nothing; the other entry points are called with one argument that validation looks at AFTER the alignment and
refuses (an unknown dtype, a row width without an instantiation, ``reserved = 1``, ...), so an admitted alignment is seen as that later refusal.  Nothing
here can reach a launch: a probe that came back with anything but a refusal fails the test.

``WIDER`` lists the rows whose widest access exceeds what is admitted.  They are the accesses tests/test_gpu_min_alignment.py exists for; DESIGN.md
section 7 ("Alignment") says what an MI355X did with them.

Out of scope, as everything they touch must be 16-byte aligned with strides that are multiples of 8: svdq_dwconv3x3, svdq_linear_attention,
svdq_cross_attention, svdq_ip_attention, svdq_attention_d64 (key offsets and counts: their natural 4 bytes), and the load-time repack / pack utilities."""
import ctypes as C
import os
import re

import pytest

from nunchaku_amd import _lib
from tests.test_gemm_plan import CUS, WS_BASE, plan_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nunchaku_amd", "csrc")

ENTRY_POINTS = {  # entry point -> its args struct
    "svdq_quantize_w4a4_act_fuse_lora": _lib.QuantizeArgs, "svdq_gemm_w4a4": _lib.GemmArgs, "svdq_attention": _lib.AttentionArgs,
    "svdq_residual_gate_stats": _lib.ResidualArgs, "svdq_residual_diff": _lib.ResidualDiffArgs, "svdq_modulated_diff": _lib.ModulatedDiffArgs,
    "svdq_sandwich_norm": _lib.SandwichNormArgs, "svdq_sana_glue": _lib.SanaGlueArgs, "svdq_qk_norm_rope": _lib.QkNormRopeArgs,
    "svdq_pulid_ca": _lib.PulidCaArgs, "svdq_gemv_awq": _lib.GemvAwqArgs, "svdq_gemv_awq_batched": _lib.GemvAwqArgs,
    "svdq_gemv_awq_lora_batched": _lib.GemvLoraArgs, "svdq_gemm_awq": _lib.GemmAwqArgs,
}
NOT_DEVICE = {("svdq_gemm_w4a4", "lora_scales")}  # a HOST pointer to floats: read by the launcher, never by a kernel
STRIDE_FIELD = re.compile(r"^(ld\w*|\w+_hs|\w+_bs)$")

# ---- the ledger ---------------------------------------------------------------------------------------------------------------------------
# (entry point, field, admitted alignment, widest access in bytes, (file under csrc, line, text on that line) or None)
# A stride's alignment is in elements and its "access" the bytes of the widest access made at a row start.  None: the validator asks for 16 bytes, the widest
# vector access there is.
LEDGER = []


def _rows(entry, align, fields, widest, where=None):
    for f in fields.split():
        LEDGER.append((entry, f, align, widest, where))


Q = "svdq_quantize_w4a4_act_fuse_lora"
_rows(Q, 16, "act", 16, ("quantize.hip", 237, "uint4"))
_rows(Q, 8, "x x2", 8, ("quantize.hip", 440, "raw_buffer_load_b64"))                    # general kernel: u16x4, quantize.hip:102 (fuse_glu: 16, validated)
_rows(Q, 8, "smooth smooth2", 8, ("quantize.hip", 105, "u16x4"))                         # fast kernel: 4 bytes, quantize.hip:452
_rows(Q, 8, "lora_down lora_down2", 16, ("quantize.hip", 448, "raw_ptr_buffer_load_lds"))  # fast kernel: 16-byte LDS-DMA; general kernel: u16x4, quantize.hip:119
_rows(Q, 8, "ln_stats ln_stats2", 8, ("quantize.hip", 459, "float2"))
_rows(Q, 8, "mod_scale mod_shift mod_scale2 mod_shift2", 8, ("quantize.hip", 110, "u16x4"))
_rows(Q, 4, "lora_act", 4, ("svdq_common.h", 125, "unsafeAtomicAdd((float *)"))          # (Q31.32 formats: 8 bytes, validated: svdq_common.h:122)
_rows(Q, 2, "ascales", 2, ("quantize.hip", 550, "f2h<T>(scale)"))
_rows(Q, 4, "ldx ldx2", 8, ("quantize.hip", 421, "ldx"))

G = "svdq_gemm_w4a4"
_rows(G, 16, "act wgt ascales wscales lora_act_in lora_up qout rotary_emb workspace wgt2 wscales2 lora_up2", 16)
_rows(G, 16, "lora_up_packed next_lora_down_packed next_lora_down_packed2", 16, ("gemm_w4a4.hip", 897, "const V8 *lap"))
_rows(G, 8, "out", 16, ("gemm_w4a4.hip", 1351, "reinterpret_cast<v4i *>(orow"))         # wave-tile kernel: gemm_epi3.inc:393, global_store_dwordx4
_rows(G, 8, "bias bias2", 4, ("gemm_loop2.inc", 170, "global_load_lds_dword v70, s[92:93]"))  # elsewhere one element: gemm_w4a4.hip:724, gemm_loop3.inc:31
_rows(G, 8, "next_smooth next_smooth2", 8, ("gemm_w4a4.hip", 830, "u16x4"))
_rows(G, 8, "next_lora_down next_lora_down2", 8, ("gemm_w4a4.hip", 838, "u16x4"))       # split down: lowrank_split.h:32, u16x4
_rows(G, 8, "lora_act_out", 4, ("gemm_w4a4.hip", 1385, "unsafeAtomicAdd"))               # (Q31.32 formats: 8-byte integer atomics, gemm_w4a4.hip:1382)
_rows(G, 8, "norm_q norm_k norm_q2 norm_k2", 8, ("gemm_w4a4.hip", 998, "u16x4"))
_rows(G, 4, "out_vt", 4, ("gemm_w4a4.hip", 1314, "reinterpret_cast<unsigned *>(dst)"))
_rows(G, 4, "status", 4, ("gemm_w4a4.hip", 655, "__hip_atomic_store(p.status"))
_rows(G, 2, "oscales", 2, ("gemm_w4a4.hip", 1158, "p.oscales"))
_rows(G, 4, "ldo", 16, ("gemm_w4a4.hip", 1326, "p.ldo"))
_rows(G, 2, "ldvt", 4, ("gemm_w4a4.hip", 1301, "p.ldvt"))

A = "svdq_attention"
_rows(A, 16, "q k vt out zero_ptr qact workspace qlora_down_packed qlora_down_packed2", 16)
_rows(A, 8, "qsmooth qsmooth2", 8, ("attention.hip", 163, "u16x4"))
_rows(A, 8, "qlora_down qlora_down2", 8, ("attention.hip", 281, "u16x4"))                # split: lowrank_split.h:32, u16x4
_rows(A, 4, "qlora_act", 4, ("attention.hip", 303, "lora_act_add(p.qlora_act"))          # (Q31.32 formats: 8 bytes, validated)
_rows(A, 4, "status", 4, ("attention.hip", 612, "__hip_atomic_store(p.status"))
_rows(A, 2, "qscales", 2, ("attention.hip", 234, "p.qscales["))
_rows(A, 8, "ldq ldk ldvt ldo q_hs k_hs vt_hs o_hs", 16)

_rows("svdq_residual_gate_stats", 16, "res a b gate out zero_ptr res2 a2 b2 gate2 out2", 16, ("row_pass.h", 39, "u16x8"))
_rows("svdq_residual_gate_stats", 8, "stats stats2", 4, ("residual.hip", 90, "stats[2 * (size_t)row] = mean"))
_rows("svdq_residual_gate_stats", 8, "ld", 16)
_rows("svdq_residual_diff", 16, "cur base prev out_res cur2 base2 prev2 out_res2", 16, ("row_pass.h", 39, "u16x8"))
_rows("svdq_residual_diff", 8, "partials", 4, ("row_pass.h", 71, "partials[2 * (size_t)row] = sd"))
_rows("svdq_residual_diff", 8, "result", 4, ("residual_diff.hip", 65, "result->sum_diff = sd"))
_rows("svdq_residual_diff", 8, "ld", 16)
_rows("svdq_modulated_diff", 16, "x mod_scale mod_shift prev out_mod", 16, ("row_pass.h", 39, "u16x8"))
_rows("svdq_modulated_diff", 8, "stats", 8, ("modulated_diff.hip", 27, "float2"))
_rows("svdq_modulated_diff", 8, "partials", 4, ("row_pass.h", 71, "partials[2 * (size_t)row] = sd"))
_rows("svdq_modulated_diff", 8, "result", 4, ("residual_diff.hip", 65, "result->sum_diff = sd"))
_rows("svdq_modulated_diff", 8, "ld", 16)
_rows("svdq_sandwich_norm", 16, "res a w_post gate w_pre scale out out_mod", 16, ("row_pass.h", 39, "u16x8"))
_rows("svdq_sandwich_norm", 8, "stats", 4, ("sandwich_norm.hip", 96, "stats[2 * (size_t)row] = rstd_a"))
_rows("svdq_sandwich_norm", 8, "ld_res ld_a ld_out ld_mod gate_bs scale_bs", 16)
_rows("svdq_sana_glue", 16, "res a timestep gate_table mod_table out out_mod", 16, ("row_pass.h", 39, "u16x8"))
_rows("svdq_sana_glue", 8, "stats", 4, ("sana_glue.hip", 98, "stats[2 * (size_t)row] = mean"))
_rows("svdq_sana_glue", 8, "ld_res ld_a ld_out ld_mod timestep_bs", 16)
_rows("svdq_qk_norm_rope", 16, "qkv norm_q norm_k freqs vt", 16, ("row_pass.h", 39, "u16x8"))
_rows("svdq_qk_norm_rope", 4, "rstd", 4, ("qk_norm_rope.hip", 73, "rstd_out["))
_rows("svdq_qk_norm_rope", 8, "ld ldvt", 16)
_rows("svdq_pulid_ca", 16, "x a_fold colsum cbias b_fold probs out acc o_acc", 16, ("pulid_ca.hip", 198, "const v4f cs"))
_rows("svdq_pulid_ca", 8, "stats", 4, ("pulid_ca.hip", 184, "p.stats[2 * row]"))
_rows("svdq_pulid_ca", 8, "ldx ldo", 16)
for _e in ("svdq_gemv_awq", "svdq_gemv_awq_batched"):
    _rows(_e, 16, "x qweight", 16, ("gemv_awq.hip", 152, "const v4i *"))
    _rows(_e, 2, "scales zeros", 2, ("gemv_awq.hip", 153, "scales[(size_t)c * N + n]"))
    _rows(_e, 2, "bias", 2, ("gemv_awq.hip", 183, "bias[n]"))
    _rows(_e, 2, "out", 2, ("gemv_awq.hip", 185, "out[no]"))
    _rows(_e, 8, "ldx", 16, ("gemv_awq.hip", 241, "u16x8"))
_rows("svdq_gemv_awq_lora_batched", 16, "x down up", 16, ("gemv_awq_lora.hip", 60, "u16x8"))
_rows("svdq_gemv_awq_lora_batched", 2, "out", 2, ("gemv_awq_lora.hip", 102, "e.out[no]"))
_rows("svdq_gemv_awq_lora_batched", 2, "t", 2, ("gemv_awq_lora.hip", 75, "e.t[j]"))
_rows("svdq_gemm_awq", 16, "x qweight workspace", 16, ("gemm_awq.hip", 133, "const v4i *"))
_rows("svdq_gemm_awq", 8, "out", 8, ("gemm_awq.hip", 222, "reinterpret_cast<u16x4 *>(out + idx)"))  # without a K-split: one element, gemm_awq.hip:199
_rows("svdq_gemm_awq", 2, "scales scaled_zeros", 2, ("gemm_awq.hip", 137, "scales[(size_t)kb * N + qn]"))
_rows("svdq_gemm_awq", 2, "bias", 2, ("gemm_awq.hip", 219, "bias[n + t]"))
_rows("svdq_gemm_awq", 8, "ldx", 16, ("gemm_awq.hip", 133, "const v4i *"))
LEDGER = tuple(LEDGER)

# rows whose widest access is wider than what is admitted (everything else: widest <= admitted, asserted below)
WIDER = {(Q, "lora_down"), (Q, "lora_down2"), (G, "out"), (G, "ldo")}


def admitted(entry: str, field: str) -> int:
    """the ledger's alignment of a field (tests/test_gpu_min_alignment.py moves operands by it)"""
    hit = [r[2] for r in LEDGER if r[:2] == (entry, field)]
    assert len(hit) == 1, (entry, field, hit)
    return hit[0]


def below_16(entry: str):
    """the pointer fields of an entry point that validation admits below 16 bytes -> {field: bytes}"""
    return {f: al for e, f, al, _, _ in LEDGER if e == entry and al < 16 and not STRIDE_FIELD.match(f)}


# ---- probes: (args with made-up addresses in which every pointer is given, call -> "admitted" | "refused") ------------------------------------
P = 1 << 20  # made-up addresses: multiples of 1 MiB


def _fill_pointers(a, skip=()):
    for i, (name, typ) in enumerate(type(a)._fields_):
        if typ is C.c_void_p and name not in skip:
            setattr(a, name, (i + 1) * P)
    return a


def _verdict(rc, msg, admitted_rc, admitted_word, refused_words):
    """admitted: the refusal of the argument that is looked at after every alignment; refused: SVDQ_E_INVALID naming an alignment"""
    if rc == admitted_rc and admitted_word in msg:
        return "admitted"
    if rc == 1 and any(w in msg for w in refused_words):
        return "refused"
    return f"unexpected: rc={rc} {msg!r}"


ALIGN_WORDS = (b"aligned", b"multiple of 4", b"multiple of 8", b"multiples of 8", b"even ldvt")


def _quantize_args():
    a = _fill_pointers(_lib.QuantizeArgs())
    a.M, a.M_pad, a.K, a.R, a.ldx, a.dtype = 256, 512, 384, 32, 384, _lib.SVDQ_BF16
    a.M2, a.ldx2, a.split_rows = 44, 384, 256
    return a


def _quantize_probe(lib, a):
    out = (C.c_int32 * 8)()
    rc = lib.svdq_quantize_plan(C.byref(a), out)
    return _verdict(rc, b"plan" if rc == 0 else lib.svdq_last_error(), 0, b"plan", ALIGN_WORDS)


def _gemm_args():
    lib = _lib.load()
    a = plan_args(512, 768, 256, _lib.FUSE_RMSNORM_ROPE, 0, 32, 0, _lib.LORA_ACT_F32, WS_BASE, 1, 1, _lib.SVDQ_BF16, lib=lib)
    given = {name for name, _ in _lib.GemmArgs._fields_ if getattr(a, name, None)}
    for i, (name, typ) in enumerate(_lib.GemmArgs._fields_):
        if typ is C.c_void_p and name not in given:  # (the pointers the RMSNorm + RoPE row does not use are looked at all the same)
            setattr(a, name, 0x200000000 + i * P)
    a.ldvt = a.M_pad
    return a


def _gemm_probe(lib, a):
    out = (C.c_int32 * 8)()
    rc = lib.svdq_gemm_plan(C.byref(a), CUS, out)
    return _verdict(rc, b"plan" if rc == 0 else lib.svdq_last_error(), 0, b"plan", ALIGN_WORDS)


def _attention_args():
    a = _fill_pointers(_lib.AttentionArgs())
    a.L, a.H, a.head_dim, a.dtype, a.scale = 512, 2, 128, _lib.SVDQ_BF16, 1.0
    a.ldq, a.ldk, a.ldo, a.ldvt, a.q_hs, a.k_hs, a.o_hs, a.vt_hs = 768, 768, 256, 512, 128, 128, 128, 128 * 512
    a.qR, a.qsplit_rows, a.zero_bytes, a.workspace_bytes = 32, 256, 16, 0
    a.reserved = 1  # looked at behind every alignment: "reserved must be 0"
    return a


def _launch_probe(symbol, rc_ok, word, batched=False):
    def probe(lib, a):
        fn = getattr(lib, symbol)
        rc = fn(C.byref(a), 1, None) if batched else fn(C.byref(a), None)
        return _verdict(rc, lib.svdq_last_error(), rc_ok, word, ALIGN_WORDS)
    return probe


NO_CLASS = 4608  # ceil(C / 512) = 9: a row width without an instantiation, refused (SVDQ_E_UNSUPPORTED) after everything else passed and before a launch


def _residual_args():
    a = _fill_pointers(_lib.ResidualArgs())
    a.M, a.M2, a.C, a.ld, a.dtype, a.eps, a.zero_bytes = 4, 4, NO_CLASS, NO_CLASS, _lib.SVDQ_BF16, 1e-6, 16
    return a


def _residual_diff_args():
    a = _fill_pointers(_lib.ResidualDiffArgs())
    a.M, a.M2, a.C, a.ld, a.dtype = 4, 4, NO_CLASS, NO_CLASS, _lib.SVDQ_BF16
    return a


def _modulated_diff_args():
    a = _fill_pointers(_lib.ModulatedDiffArgs())
    a.M, a.C, a.ld, a.dtype = 4, NO_CLASS, NO_CLASS, _lib.SVDQ_BF16
    return a


def _sandwich_args():
    a = _fill_pointers(_lib.SandwichNormArgs())
    a.M, a.T, a.C, a.dtype, a.eps = 4, 2, NO_CLASS, _lib.SVDQ_BF16, 1e-6
    a.ld_res = a.ld_a = a.ld_out = a.ld_mod = a.gate_bs = a.scale_bs = NO_CLASS
    return a


def _sana_args():
    a = _fill_pointers(_lib.SanaGlueArgs())
    a.B, a.T, a.C, a.C_pad, a.dtype = 1, 4, 512, 512, _lib.SVDQ_BF16
    a.ld_res = a.ld_a = a.ld_out = a.ld_mod = 512
    a.timestep_bs, a.gate_row, a.scale_row, a.shift_row = 6 * 512, 0, 1, 2
    a.eps = -1.0  # looked at last: "eps must be finite and not negative"
    return a


def _qk_args():
    a = _fill_pointers(_lib.QkNormRopeArgs())
    a.T, a.L_pad, a.H, a.head_dim, a.ld, a.ldvt, a.dtype = 128, 128, 1, 128, 384, 128, _lib.SVDQ_BF16
    a.eps = -1.0
    return a


def _pulid_args():
    a = _fill_pointers(_lib.PulidCaArgs())
    a.T, a.C, a.H, a.N, a.ldx, a.ldo, a.dtype = 4, 128, 4, 4, 128, 128, _lib.SVDQ_BF16
    a.out_scale = float("inf")  # looked at behind the alignments: "out_scale must be finite"
    return a


def _gemv_args():
    a = _fill_pointers(_lib.GemvAwqArgs())
    a.M, a.N, a.K, a.ldx, a.group_size = 1, 64, 64, 64, 64
    a.dtype = 99  # looked at behind the alignments: "unknown dtype"
    return a


def _gemv_lora_args():
    a = _fill_pointers(_lib.GemvLoraArgs())
    a.r, a.N, a.K, a.strength, a.dtype = 16, 64, 64, 1.0, 99
    return a


def _gemm_awq_args():
    a = _fill_pointers(_lib.GemmAwqArgs())
    a.M, a.N, a.K, a.ldx, a.group_size, a.dtype = 4, 64, 128, 128, 128, _lib.SVDQ_BF16
    a.workspace_bytes = -1  # looked at last: "workspace of -1 bytes"
    return a


PROBES = {
    "svdq_quantize_w4a4_act_fuse_lora": (_quantize_args, _quantize_probe),
    "svdq_gemm_w4a4": (_gemm_args, _gemm_probe),
    "svdq_attention": (_attention_args, _launch_probe("svdq_attention", 1, b"reserved must be 0")),
    "svdq_residual_gate_stats": (_residual_args, _launch_probe("svdq_residual_gate_stats", 2, b"ceil(C/512)")),
    "svdq_residual_diff": (_residual_diff_args, _launch_probe("svdq_residual_diff", 2, b"ceil(C/512)")),
    "svdq_modulated_diff": (_modulated_diff_args, _launch_probe("svdq_modulated_diff", 2, b"ceil(C/512)")),
    "svdq_sandwich_norm": (_sandwich_args, _launch_probe("svdq_sandwich_norm", 2, b"ceil(C/512)")),
    "svdq_sana_glue": (_sana_args, _launch_probe("svdq_sana_glue", 1, b"eps must be finite")),
    "svdq_qk_norm_rope": (_qk_args, _launch_probe("svdq_qk_norm_rope", 1, b"eps must be finite")),
    "svdq_pulid_ca": (_pulid_args, _launch_probe("svdq_pulid_ca", 1, b"out_scale must be finite")),
    "svdq_gemv_awq": (_gemv_args, _launch_probe("svdq_gemv_awq", 1, b"unknown dtype")),
    "svdq_gemv_awq_batched": (_gemv_args, _launch_probe("svdq_gemv_awq_batched", 1, b"unknown dtype", batched=True)),
    "svdq_gemv_awq_lora_batched": (_gemv_lora_args, _launch_probe("svdq_gemv_awq_lora_batched", 1, b"unknown dtype", batched=True)),
    "svdq_gemm_awq": (_gemm_awq_args, _launch_probe("svdq_gemm_awq", 1, b"workspace of")),
}


def _moved(a, field, by):
    setattr(a, field, getattr(a, field) + by)
    return a


# ---- tests ----------------------------------------------------------------------------------------------------------------------------------
def test_every_pointer_and_stride_field_has_a_row():
    """against the ctypes structs: a new field fails here until someone reads its kernels and gives it a row"""
    have = {(e, name) for e, cls in ENTRY_POINTS.items() for name, typ in cls._fields_
            if typ is C.c_void_p or (isinstance(typ, type) and issubclass(typ, C._Pointer)) or STRIDE_FIELD.match(name)}
    rows = {r[:2] for r in LEDGER}
    assert len(rows) == len(LEDGER), "a field has two rows"
    assert not have - rows - NOT_DEVICE, f"no row for: {sorted(have - rows - NOT_DEVICE)}"
    assert not (rows | NOT_DEVICE) - have, f"a row for a field that does not exist: {sorted((rows | NOT_DEVICE) - have)}"
    assert set(PROBES) == set(ENTRY_POINTS) == {r[0] for r in LEDGER}
    assert len(LEDGER) == 182


@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
def test_every_field_is_admitted_at_its_alignment_and_refused_at_half_of_it(built_lib, entry):
    lib = _lib.load()
    make, probe = PROBES[entry]
    assert probe(lib, make()) == "admitted", f"{entry}: the probe's own arguments"
    for e, field, align, _, _ in LEDGER:
        if e != entry:
            continue
        assert align in (2, 4, 8, 16) and getattr(make(), field) % 16 == 0, (entry, field)
        got = probe(lib, _moved(make(), field, align))
        assert got == "admitted", f"{entry}.{field} at {align}: {got}"
        got = probe(lib, _moved(make(), field, align // 2))
        assert got == "refused", f"{entry}.{field} at {align // 2}: {got}"
        got = probe(lib, _moved(make(), field, align + align // 2))
        assert got == "refused", f"{entry}.{field} at {align + align // 2}: {got}"


def test_the_lines_that_depend_on_a_mode(built_lib):
    """the Q31.32 low-rank sums are 64-bit integers; fuse_glu reads x in 16-byte pieces"""
    lib = _lib.load()
    for fmt in (_lib.LORA_ACT_Q32, _lib.LORA_ACT_Q32_RUNS):
        a = _quantize_args()
        a.lora_act_format = fmt
        assert _quantize_probe(lib, _moved(a, "lora_act", 8)) == "admitted"
        a = _quantize_args()
        a.lora_act_format = fmt
        assert _quantize_probe(lib, _moved(a, "lora_act", 4)) == "refused"
        probe = PROBES["svdq_attention"][1]
        a = _attention_args()
        a.qlora_act_format = fmt
        assert probe(lib, _moved(a, "qlora_act", 8)) == "admitted"
        a = _attention_args()
        a.qlora_act_format = fmt
        assert probe(lib, _moved(a, "qlora_act", 4)) == "refused"

    def glu(**kw):
        a = _lib.QuantizeArgs()
        a.x, a.act, a.ascales, a.smooth = P, 2 * P, 3 * P, 4 * P
        a.M, a.M_pad, a.K, a.ldx, a.fuse_glu = 200, 256, 384, 768, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return _quantize_probe(lib, a)

    assert glu() == glu(x=P + 16) == glu(ldx=776) == "admitted"
    assert glu(x=P + 8) == glu(ldx=772) == "refused"


def test_only_the_listed_accesses_are_wider_than_what_is_admitted():
    for entry, field, align, widest, _ in LEDGER:
        unit = 2 if STRIDE_FIELD.match(field) else 1  # a stride of `align` 16-bit elements puts a row start on 2 * align bytes
        assert (widest > align * unit) == ((entry, field) in WIDER), (entry, field, align, widest)
    assert WIDER <= {r[:2] for r in LEDGER}


def test_the_cited_lines_say_what_the_ledger_says():
    for entry, field, _, _, where in LEDGER:
        if where is None:
            continue
        name, line, text = where
        lines = open(os.path.join(CSRC, name)).read().split("\n")
        assert line <= len(lines) and text in lines[line - 1], f"{entry}.{field}: {name}:{line} does not hold {text!r} (it holds {lines[line - 1].strip()[:120]!r})"


def test_the_header_states_the_alignment_of_every_field():
    """include/svdq_amd.h: an "Alignment of the operands of <entry point>" comment in front of the declaration, one line per alignment: `fields   N bytes` /
    `fields   N elements`; it names every field of the ledger, with the ledger's number"""
    src = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    for entry in ENTRY_POINTS:
        m = re.search(r"/\* Alignment of the operands of [\w ]*\b" + entry + r"\b((?:(?!\*/).)*)\*/", src, flags=re.S)
        assert m, f"{entry}: no 'Alignment of the operands of' comment"
        stated = {}
        for names, n, unit in re.findall(r"^ \*   ([\w, ]+?)\s{2,}(\d+) (bytes|elements)", m.group(1), flags=re.M):
            for f in names.split(", "):
                stated[f] = (int(n), unit)
        want = {f: (al, "elements" if STRIDE_FIELD.match(f) else "bytes") for e, f, al, _, _ in LEDGER if e == entry}
        assert stated == want, f"{entry}: header and ledger differ: {sorted(set(stated.items()) ^ set(want.items()))}"
        assert src.index(m.group(0)) < src.index("int " + entry + "(")


def test_aligned_launches_plan_as_before(built_lib):
    """no plan looks at the alignments below 16 bytes: moving every such operand of a launch to its minimum leaves the plan words as they were -- one row per
    quantiser family and GEMM plan key (the attention plan query does not look at pointers at all)"""
    from tests import test_gpu_hot_instantiations as T

    lib = _lib.load()
    assert T.quant_plan(32, True, True, False, False, "f32", 300, 384, 512) == \
        {"family": "fast", "sel": 7, "cpw": 4, "slices": 1, "lora_act_add": 0, "grid": 16, "glu": False, "memset": False}
    assert T.quant_plan(176, True, False, False, False, "f32", 300, 384, 512)["family"] == "general"
    for R, want in ((32, "fast"), (96, "fast"), (176, "general")):
        a = _quantize_args()
        a.R = R
        out, moved = (C.c_int32 * 8)(), (C.c_int32 * 8)()
        assert lib.svdq_quantize_plan(C.byref(a), out) == 0 and ("fast", "general")[out[0]] == want
        for f, al in below_16(Q).items():
            _moved(a, f, al)
        a.ldx, a.ldx2 = a.ldx + 4, a.ldx2 + 4
        assert lib.svdq_quantize_plan(C.byref(a), moved) == 0, lib.svdq_last_error()
        assert list(moved) == list(out), (R, list(out), list(moved))
    for fuse, geometry, R, R2 in ((_lib.FUSE_NONE, 1, 32, 0), (_lib.FUSE_NONE, 3, 32, 0), (_lib.FUSE_NONE, 8, 32, 0), (_lib.FUSE_SILU, 1, 64, 0),
                                  (_lib.FUSE_GELU_QUANT, 1, 32, 32), (_lib.FUSE_GELU_QUANT, 6, 32, 48), (_lib.FUSE_GELU_QUANT, 7, 64, 64),
                                  (_lib.FUSE_RMSNORM_ROPE, 1, 32, 0)):
        N = 768 if fuse == _lib.FUSE_RMSNORM_ROPE else 512
        a = plan_args(512, N, 256, fuse, geometry, R, R2, _lib.LORA_ACT_F32, 2, 0, 0, _lib.SVDQ_BF16, lib=lib)
        a.bias = 0x63000000
        out, moved = (C.c_int32 * 8)(), (C.c_int32 * 8)()
        assert lib.svdq_gemm_plan(C.byref(a), CUS, out) == 0, lib.svdq_last_error()
        for f, al in below_16(G).items():
            if getattr(a, f):
                _moved(a, f, al)
        a.ldo = a.ldo + 4 if a.out else a.ldo
        assert lib.svdq_gemm_plan(C.byref(a), CUS, moved) == 0, lib.svdq_last_error()
        assert list(moved) == list(out), (fuse, geometry, list(out), list(moved))
