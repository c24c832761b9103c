"""Build the HIP shared library in-tree (nunchaku_amd/csrc/libsvdq_amd.so) with hipcc for gfx950."""

import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libsvdq_amd.so")
SOURCES = ["repack.hip", "quantize.hip", "gemm_w4a4.hip", "attention.hip", "gemv_awq.hip", "gemv_awq_lora.hip", "gemm_awq.hip", "residual.hip", "residual_diff.hip", "modulated_diff.hip", "ip_attention.hip", "linear_attention.hip", "dwconv.hip", "cross_attention.hip", "sana_glue.hip", "attention_d64.hip", "sandwich_norm.hip", "qk_norm_rope.hip", "pulid_ca.hip", "qwen_rotary.hip"]
# -ffp-contract=off: the quantiser's arithmetic is specified operation by operation;
# the hot loop uses explicit fma.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared"]


def _stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    # every header and generated .inc file in csrc, whether listed anywhere or not: a forgotten one would leave a stale library in place
    deps = SOURCES + [f for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))] + [os.path.join("..", "..", "include", "svdq_amd.h")]
    return any(os.path.getmtime(os.path.join(CSRC, f)) > t for f in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *FLAGS, "-o", LIB, *SOURCES]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, cwd=CSRC, check=True)
    return LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))
