"""CPU restatement of ``svdq_sana_glue`` (include/svdq_amd.h), operation for operation, for the tests of SANA's block glue.

16-bit values are carried as float32 numpy arrays.  The LayerNorm statistics are an INPUT (``stats``): the kernel's fp32 sums run in the order
of its lanes, which a restatement cannot reproduce bit for bit and does not need to -- the GPU tests hold the kernel's statistics to the
float64 ones within 2e-6 and then feed them here, so that everything behind them can be compared with ``torch.equal``.

``one_op`` is the 16-bit result of ONE fp32 operation on 16-bit operands whose exact value is given in float64: bf16 rounds the fp32 result
(two roundings), fp16 rounds once -- the gfx950 backend folds the fp32 operation and the conversion into one v_fma_mix instruction, in
torch's half kernels and in this project's alike (oracle/svdq_oracle.py ``_round16_fma`` states the same rule for the FLUX glue)."""
import numpy as np
import torch

F32 = np.float32
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}  # the unit roundoff: half an ulp, relative
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def round16(x32: np.ndarray, dtype: str) -> np.ndarray:
    """float32 -> nearest-even 16-bit value, as float32"""
    t = torch.from_numpy(np.ascontiguousarray(x32, dtype=F32))
    return t.to(TORCH_DT[dtype]).float().numpy()


def one_op(exact64: np.ndarray, dtype: str) -> np.ndarray:
    if dtype == "fp16":
        with np.errstate(over="ignore"):
            return np.asarray(exact64, dtype=np.float64).astype(np.float16).astype(F32)
    with np.errstate(over="ignore"):
        return round16(np.asarray(exact64, dtype=np.float64).astype(F32), dtype)


def clip(x: np.ndarray, dtype: str) -> np.ndarray:
    return np.minimum(np.maximum(x, F32(-65504.0)), F32(65504.0)) if dtype == "fp16" else x


def mod_row(timestep: np.ndarray, table: np.ndarray, row: int, dtype: str) -> np.ndarray:
    """mod(tab, i)[b, c] = clip(round16(timestep[b, i, c] + tab[i, c]))  ->  [B, 1, C]"""
    return clip(one_op(timestep[:, row].astype(np.float64) + table[row].astype(np.float64)[None], dtype), dtype)[:, None, :]


def glue_residual(res, a, timestep, gate_table, gate_row, dtype: str) -> np.ndarray:
    """t [B, T, C]: res | clip(round16(a + res)) | clip(round16(round16(a * g) + res))"""
    if a is None:
        return np.asarray(res, dtype=F32)
    t = a.astype(np.float64)
    if gate_row is not None and gate_row >= 0:
        g = mod_row(timestep, gate_table, gate_row, dtype)
        t = one_op(t * g.astype(np.float64), dtype).astype(np.float64)
    return clip(one_op(t + res.astype(np.float64), dtype), dtype)


def glue_modulate(t, stats, timestep, mod_table, scale_row: int, shift_row: int, dtype: str) -> np.ndarray:
    """out_mod [B, T, C] = clip(round16(round16(n * s) + h)), n = round16((t - mean) * rstd), s = round16(mod(scale) + 1), h = mod(shift);
    stats [B * T, 2] float32 (mean, rstd); t - mean is an fp32 subtraction, its product with rstd is exact in float64"""
    B, T, _ = t.shape
    mean, rstd = stats[:, 0].astype(F32).reshape(B, T, 1), stats[:, 1].astype(F32).reshape(B, T, 1)
    n = one_op((t.astype(F32) - mean).astype(np.float64) * rstd.astype(np.float64), dtype)
    s = one_op(mod_row(timestep, mod_table, scale_row, dtype).astype(np.float64) + 1.0, dtype)
    h = mod_row(timestep, mod_table, shift_row, dtype)
    p = one_op(n.astype(np.float64) * s.astype(np.float64), dtype)
    return clip(one_op(p.astype(np.float64) + h.astype(np.float64), dtype), dtype)


def pad_cols(x: np.ndarray, C_pad: int) -> np.ndarray:
    out = np.zeros(x.shape[:-1] + (C_pad,), dtype=F32)
    out[..., : x.shape[-1]] = x
    return out


def sana_glue_ref(res, a=None, *, timestep=None, gate_table=None, gate_row=None, mod_table=None, scale_row=None, shift_row=None, stats=None,
                  C_pad=None, dtype="bf16"):
    """``(out [B, T, C_pad], out_mod [B, T, C_pad] or None)``; res / a [B, T, C], timestep [B, 6, C], tables [6, C]: float32 arrays that hold
    16-bit values; ``out_mod`` when ``mod_table`` is given (then ``stats`` is required)."""
    C = res.shape[-1]
    C_pad = (C + 127) // 128 * 128 if C_pad is None else C_pad
    t = glue_residual(res, a, timestep, gate_table, gate_row, dtype)
    m = None if mod_table is None else pad_cols(glue_modulate(t, stats, timestep, mod_table, scale_row, shift_row, dtype), C_pad)
    return pad_cols(t, C_pad), m


def stats64(t: np.ndarray, eps: float = 1e-6) -> np.ndarray:
    """[rows, 2] float32 (mean, 1 / sqrt(var + eps)), population variance in float64 (what oracle.ln_stats_ref computes)"""
    y = t.reshape(-1, t.shape[-1]).astype(np.float64)
    mean = y.mean(axis=1)
    var = ((y - mean[:, None]) ** 2).mean(axis=1)
    return np.stack([mean, 1.0 / np.sqrt(var + eps)], axis=1).astype(F32)


def to_torch(x32: np.ndarray, dtype: str) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=F32)).to(TORCH_DT[dtype])
