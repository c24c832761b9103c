"""CPU restatements of ``svdq_sandwich_norm`` and ``svdq_qk_norm_rope`` (include/svdq_amd.h), operation for operation, and the 16-bit torch-op
sequences they restate (diffusers' ``RMSNorm`` and ``ZImageTransformerBlock``, the reference's ``NunchakuZSingleStreamAttnProcessor``).

A restatement carries 16-bit values as float32 tensors; every operation is ONE fp32 torch operation followed by ``r16`` (round to the 16-bit
dtype and come back).  The reciprocal RMS values are an INPUT (``rstd``): the kernels' fp32 sums run in the order of their lanes, which a
restatement cannot reproduce bit for bit and does not need to -- the tests hold the kernel's values to a float64 evaluation and then feed them
here, so that everything behind them can be compared with ``torch.equal``; the CPU tests feed torch's own."""
import torch

TD = {"bf16": torch.bfloat16, "fp16": torch.float16}
EPS = 1e-5


def r16(x: torch.Tensor, dtype: str) -> torch.Tensor:
    return x.to(TD[dtype]).float()


# ---- the restatements -----------------------------------------------------------------------------------------------------------------
def rms(h: torch.Tensor, w: torch.Tensor, rstd: torch.Tensor, dtype: str) -> torch.Tensor:
    """round16(round16(h * rstd) * w); h [..., C], w [C], rstd [..., 1] float32"""
    return r16(r16(h * rstd, dtype) * w, dtype)


def sandwich_ref(res, a=None, *, w_post=None, gate=None, w_pre=None, scale=None, rstd_a=None, rstd_y=None, dtype="bf16"):
    """``(y, out_mod or None)``; res / a [B, T, C], gate / scale [B, C], weights [C]: float32 tensors that hold 16-bit values;
    rstd_a / rstd_y [B, T, 1] float32.  ``out_mod`` when ``w_pre`` is given."""
    y = res
    if a is not None:
        n = rms(a, w_post, rstd_a, dtype)
        if gate is not None:
            n = r16(gate[:, None, :] * n, dtype)
        y = r16(res + n, dtype)
    m = None
    if w_pre is not None:
        m = rms(y, w_pre, rstd_y, dtype)
        if scale is not None:
            m = r16(m * scale[:, None, :], dtype)
    return y, m


def qk_ref(x, w=None, rstd=None, freqs=None, dtype="bf16"):
    """x [T, H, 128] float32 holding 16-bit values, w [128] or None, rstd [T, H, 1] float32, freqs [T, 64, 2] float32 (cos, sin) or None"""
    n = x if w is None else rms(x, w, rstd, dtype)
    if freqs is None:
        return n
    n0, n1 = n[..., 0::2], n[..., 1::2]
    c, s = freqs[:, None, :, 0], freqs[:, None, :, 1]
    o0 = r16(n0 * c - n1 * s, dtype)
    o1 = r16(n0 * s + n1 * c, dtype)
    return torch.stack([o0, o1], dim=-1).flatten(-2)


def rstd64(h: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """[..., 1] float64: 1 / sqrt(mean(h^2) + eps) evaluated in float64"""
    return 1.0 / torch.sqrt(h.double().pow(2).mean(-1, keepdim=True) + eps)


# ---- the 16-bit torch-op sequences (the specification) --------------------------------------------------------------------------------
def torch_rstd(x16: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    return torch.rsqrt(x16.to(torch.float32).pow(2).mean(-1, keepdim=True) + eps)


def torch_rmsnorm(x16: torch.Tensor, w16: torch.Tensor, eps: float = EPS, rstd: torch.Tensor | None = None) -> torch.Tensor:
    """diffusers' RMSNorm.forward with a 16-bit weight: ``x * rsqrt(var + eps)`` (fp32 by promotion), cast to the weight's dtype, ``* weight``"""
    x = x16 * (torch_rstd(x16, eps) if rstd is None else rstd)
    return x.to(w16.dtype) * w16


def torch_sandwich(res, a=None, *, w_post=None, gate=None, w_pre=None, scale=None, eps=EPS, rstd_a=None, rstd_y=None):
    """the block's glue as 16-bit torch operations; gate = tanh(gate_*), scale = 1 + scale_*, each [B, C]"""
    y = res
    if a is not None:
        n = torch_rmsnorm(a, w_post, eps, rstd_a)
        y = res + (gate.unsqueeze(1) * n if gate is not None else n)
    m = None
    if w_pre is not None:
        m = torch_rmsnorm(y, w_pre, eps, rstd_y)
        if scale is not None:
            m = m * scale.unsqueeze(1)
    return y, m


def torch_rope(x_in: torch.Tensor, freqs_cis: torch.Tensor) -> torch.Tensor:
    """the reference processor's apply_rotary_emb: x_in [B, T, H, 128] 16-bit, freqs_cis [B, T, 64] complex64"""
    x = torch.view_as_complex(x_in.float().reshape(*x_in.shape[:-1], -1, 2))
    x_out = torch.view_as_real(x * freqs_cis.unsqueeze(2)).flatten(3)
    return x_out.type_as(x_in)


def torch_qk(x16, w16=None, freqs_cis=None, eps=EPS, rstd=None):
    """x16 [B, T, H, 128]: norm_q / norm_k (an RMSNorm over the last axis) and the rotation, as the reference processor orders them"""
    n = x16 if w16 is None else torch_rmsnorm(x16, w16, eps, rstd)
    return n if freqs_cis is None else torch_rope(n, freqs_cis)
