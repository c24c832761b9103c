"""Z-Image's quantised block and ``ZImageBlockStack`` on the GPU, at (dim 256, 2 heads, hidden 512) and (384, 3, 1024), rank 32, both dtypes,
synthetic weights (``synthetic_codes_``), batch 1 and 2 at 77 and at 200 tokens (neither a multiple of 128), with and without modulation.

* The fused path is ``torch.equal`` to its composition from the public modules and the two new ops called one by one (every sandwich pass
  split into the pass that closes and the pass that opens): this pins the cross-block hand-off and the padding.
* Against the 16-bit torch-op reading of the block the comparison is relative.  The truth is the same composition with the glue in float64
  (``F.scaled_dot_product_attention`` on the real tokens, the ``SVDQW4A4Linear`` s as they are); the 16-bit torch-op composition's own
  maximum and mean error against it is measured, and the fused block's must stay within ``ERR_FACTOR`` of both.
* Keys behind a sample's real tokens are masked: NaN rows there change nothing.
* The launches of a two-block stack are counted."""

import math

import pytest
import torch
import torch.nn.functional as F

from tests import zimage_ref as Z

pytestmark = pytest.mark.gpu

TD = Z.TD
DTYPES = ["bf16", "fp16"]
SIZES = [(256, 2, 512), (384, 3, 1024)]
# the fused block's max and mean error against the float64-glue truth may be this many times the 16-bit torch-op composition's own: the
# factor covers rounding flips from rstd's last bit and the attention kernel's rounding of P.  Measured over the 32 cases below on one MI355X
# (every pair is in profiles/zimage.txt): max error fused 0.94-2.02 against torch 0.94-2.00 (worst ratio 1.07), mean error fused 0.084-0.268
# against torch 0.085-0.269 (worst ratio 1.004), at outputs up to 9.5 -- a rounding flip of the glue changes 4-bit codes of the next layer.
ERR_FACTOR = 1.5


@pytest.fixture
def strict_mode():
    from nunchaku_amd import mode

    with mode.deterministic_mode("strict"):
        yield


@torch.no_grad()
def _init_synthetic_(block, seed):
    """random weights in the checkpoint layout, as tests/test_gpu_sdxl_block.py draws them for a W4A4 layer; RMSNorm weights near 1"""
    from nunchaku_amd.models.linear import SVDQW4A4Linear, synthetic_codes_

    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda shape, scale: torch.randn(tuple(shape), generator=g, device="cuda") * scale
    for m in block.modules():
        if isinstance(m, SVDQW4A4Linear):
            K = m.in_features
            synthetic_codes_(m.qweight, m.wscales, K, g)
            m.smooth_factor.copy_(torch.rand((K,), generator=g, device="cuda") + 0.5)
            m.smooth_factor_orig.copy_(m.smooth_factor)
            m.proj_down.copy_(rnd(m.proj_down.shape, 0.5 / math.sqrt(K)))
            m.proj_up.copy_(rnd(m.proj_up.shape, 0.5 / math.sqrt(m.rank)))
        elif isinstance(m, torch.nn.Linear):
            m.weight.copy_(rnd(m.weight.shape, 1.0 / math.sqrt(m.in_features)))
            m.bias.copy_(rnd(m.bias.shape, 0.1))
        elif isinstance(m, torch.nn.RMSNorm):
            m.weight.copy_(1.0 + rnd(m.weight.shape, 0.1))
    return block


_BLOCKS = {}


def _blocks(dim, heads, hidden, dtype, modulation):
    """two blocks per size, dtype and kind, built once and left unchanged"""
    from nunchaku_amd.models.zimage import NunchakuZImageTransformerBlock

    key = (dim, dtype, modulation)
    if key not in _BLOCKS:
        _BLOCKS[key] = [_init_synthetic_(NunchakuZImageTransformerBlock(dim, heads, hidden, modulation=modulation, rank=32, torch_dtype=TD[dtype],
                                                                        device="cuda"), seed=dim + 2 * i + (dtype == "fp16")) for i in range(2)]
    return _BLOCKS[key]


def _acts(dim, Bn, T, dtype, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed + dim + T + Bn)
    x = torch.randn(Bn, T, dim, device="cuda", generator=g).to(TD[dtype])
    ang = torch.rand(Bn, T, 64, device="cuda", generator=g) * 6.2831853
    fc = torch.polar(torch.ones_like(ang), ang)
    adaln = torch.randn(Bn, 256, device="cuda", generator=g).to(TD[dtype])
    return x, fc, adaln


def _compose(blocks, x, counts, fc, adaln):
    """the stack from the public modules and ops, one operation per launch: no pass both closes and opens, nothing is handed across blocks"""
    from nunchaku_amd.ops import qk_norm_rope, sandwich_norm
    from nunchaku_amd.ops.attention import attention_packed

    Bn, T, C = x.shape
    L = (T + 127) // 128 * 128
    h = x.new_zeros(Bn, L, C)
    for b, n in enumerate(counts):
        h[b, :n] = x[b, :n]
    for blk in blocks:
        s_msa, g_msa, s_mlp, g_mlp = blk.modulate(adaln if blk.modulation else None)
        at = blk.attention
        _, hm, _ = sandwich_norm(h, w_pre=blk.attention_norm1.weight, scale=s_msa)
        qkv = at.to_qkv(hm)
        vt, o = torch.empty(Bn, C, L, dtype=x.dtype, device="cuda"), torch.empty(Bn, L, C, dtype=x.dtype, device="cuda")
        for b, n in enumerate(counts):
            qk_norm_rope(qkv[b], at.heads, n, norm_q=at.norm_q.weight, norm_k=at.norm_k.weight, freqs_cis=fc[b, :n], vt=vt[b])
            attention_packed(qkv[b], vt[b], at.heads, out=o[b], kv_valid=(n,) if n < L else None)
        a = at.to_out[0](o)
        h, _, _ = sandwich_norm(h, a, w_post=blk.attention_norm2.weight, gate=g_msa, out=True, out_mod=False)
        _, hm, _ = sandwich_norm(h, w_pre=blk.ffn_norm1.weight, scale=s_mlp)
        value, gate = blk.feed_forward.net[0].proj(hm).chunk(2, dim=-1)
        f = blk.feed_forward.net[2](value * F.silu(gate))
        h, _, _ = sandwich_norm(h, f, w_post=blk.ffn_norm2.weight, gate=g_mlp, out=True, out_mod=False)
    return h[:, :T]


@pytest.mark.parametrize("modulation", [True, False], ids=["mod", "plain"])
@pytest.mark.parametrize("Bn,T", [(1, 77), (1, 200), (2, 77), (2, 200)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,heads,hidden", SIZES)
def test_block_and_stack_equal_their_composition(dim, heads, hidden, dtype, Bn, T, modulation, strict_mode):
    from nunchaku_amd.models.zimage import ZImageBlockStack

    blocks = _blocks(dim, heads, hidden, dtype, modulation)
    x, fc, adaln = _acts(dim, Bn, T, dtype)
    ad = adaln if modulation else None
    y = blocks[0](x, None, fc, ad)
    assert y.shape == x.shape and y.dtype == TD[dtype] and torch.isfinite(y).all() and (y.float() - x.float()).abs().max() > 0.01
    assert torch.equal(blocks[0](x, None, fc, ad), y)                                                 # a second call
    assert torch.equal(y, _compose(blocks[:1], x, [T] * Bn, fc, ad))
    y2 = ZImageBlockStack(blocks)(x, None, fc, ad)
    assert torch.isfinite(y2).all() and torch.equal(y2, _compose(blocks, x, [T] * Bn, fc, ad))
    assert torch.equal(y2, blocks[1](y.contiguous(), None, fc, ad))                                   # the hand-off changes no bit
    if modulation:   # the modulation is looked at, per sample
        assert not torch.equal(blocks[0](x, None, fc, adaln.flip(0) if Bn > 1 else -adaln), y)
    # the attention module alone, through the reference's processor signature
    at = blocks[0].attention
    s_msa = blocks[0].modulate(ad)[0]
    from nunchaku_amd.ops import sandwich_norm

    _, hm, _ = sandwich_norm(x, w_pre=blocks[0].attention_norm1.weight, scale=s_msa)
    out = at(hm, attention_mask=None, freqs_cis=fc)
    assert out.shape == x.shape and torch.isfinite(out).all()
    assert not torch.equal(out, at(hm, freqs_cis=None))                                               # (the rotation is applied)


def _reading(blk, x, fc, adaln, dt):
    """the block as diffusers computes it, the glue in ``dt`` (the 16-bit dtype: the torch-op reading; float64: the truth), the attention
    ``F.scaled_dot_product_attention`` in ``dt``, the SVDQW4A4Linear s as they are (16-bit in, 16-bit out)"""
    low = x.dtype
    lin = lambda m, t: m(t.to(low)).to(dt)

    def rms(t, norm):
        if dt == torch.float64:
            return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + norm.eps) * norm.weight.double()
        return Z.torch_rmsnorm(t, norm.weight, norm.eps)

    def rope(t):
        if dt == torch.float64:
            c = torch.view_as_complex(t.reshape(*t.shape[:-1], -1, 2))
            return torch.view_as_real(c * fc.to(torch.complex128).unsqueeze(2)).flatten(3)
        return Z.torch_rope(t, fc)

    s_msa = g_msa = s_mlp = g_mlp = None
    if blk.modulation:
        scale_msa, gate_msa, scale_mlp, gate_mlp = blk.adaLN_modulation(adaln).unsqueeze(1).to(dt).chunk(4, dim=-1)
        s_msa, g_msa, s_mlp, g_mlp = 1.0 + scale_msa, gate_msa.tanh(), 1.0 + scale_mlp, gate_mlp.tanh()
    at = blk.attention
    h = x.to(dt)
    n = rms(h, blk.attention_norm1)
    q, k, v = lin(at.to_qkv, n * s_msa if s_msa is not None else n).chunk(3, dim=-1)
    q, k, v = (t.unflatten(-1, (at.heads, -1)) for t in (q, k, v))
    q, k = rope(rms(q, at.norm_q)), rope(rms(k, at.norm_k))
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2).flatten(2, 3)
    a = rms(lin(at.to_out[0], o), blk.attention_norm2)
    h = h + (g_msa * a if g_msa is not None else a)
    n = rms(h, blk.ffn_norm1)
    value, gate = lin(blk.feed_forward.net[0].proj, n * s_mlp if s_mlp is not None else n).chunk(2, dim=-1)
    f = rms(lin(blk.feed_forward.net[2], value * F.silu(gate)), blk.ffn_norm2)
    return h + (g_mlp * f if g_mlp is not None else f)


@pytest.mark.parametrize("modulation", [True, False], ids=["mod", "plain"])
@pytest.mark.parametrize("Bn,T", [(1, 77), (1, 200), (2, 77), (2, 200)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,heads,hidden", SIZES)
def test_fused_block_is_as_close_to_the_float64_glue_as_the_torch_op_reading(dim, heads, hidden, dtype, Bn, T, modulation, strict_mode):
    blk = _blocks(dim, heads, hidden, dtype, modulation)[0]
    x, fc, adaln = _acts(dim, Bn, T, dtype, seed=1)
    ad = adaln if modulation else None
    with torch.no_grad():
        truth = _reading(blk, x, fc, ad, torch.float64)
        torch16 = _reading(blk, x, fc, ad, TD[dtype])
        fused = blk(x, None, fc, ad)
    assert torch16.dtype == TD[dtype] and torch.isfinite(truth).all()
    e_torch, e_fused = (torch16.double() - truth).abs(), (fused.double() - truth).abs()
    pairs = (e_fused.max().item(), e_torch.max().item(), e_fused.mean().item(), e_torch.mean().item())
    print(f"zimage block dim={dim} {dtype} B={Bn} T={T} {'mod' if modulation else 'plain'}: max error fused {pairs[0]:.4g} / torch {pairs[1]:.4g}, "
          f"mean error fused {pairs[2]:.4g} / torch {pairs[3]:.4g}, max |truth| {truth.abs().max().item():.4g}")
    assert pairs[1] > 0 and pairs[3] > 0
    assert pairs[0] <= ERR_FACTOR * pairs[1], f"max error {pairs[0]:.4g} > {ERR_FACTOR} x {pairs[1]:.4g}"
    assert pairs[2] <= ERR_FACTOR * pairs[3], f"mean error {pairs[2]:.4g} > {ERR_FACTOR} x {pairs[3]:.4g}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim,heads,hidden", SIZES)
def test_rows_behind_the_real_tokens_are_masked(dim, heads, hidden, dtype, strict_mode):
    from nunchaku_amd.models.zimage import ZImageBlockStack

    blocks = _blocks(dim, heads, hidden, dtype, True)
    Bn, T, Tp = 2, 200, 230
    x, fc, adaln = _acts(dim, Bn, Tp, dtype, seed=2)
    want = ZImageBlockStack(blocks)(x[:, :T].contiguous(), None, fc[:, :T], adaln)                    # the unpadded call
    xp = x.clone()
    xp[:, T:] = float("nan")
    mask = torch.zeros(Bn, Tp, dtype=torch.bool, device="cuda")
    mask[:, :T] = True
    got = ZImageBlockStack(blocks)(xp, mask, fc, adaln)
    assert got.shape == xp.shape and torch.isfinite(got[:, :T]).all() and torch.equal(got[:, :T], want)
    # samples of different lengths: each against the composition with its own count
    mask[1, 150:] = False
    got = ZImageBlockStack(blocks)(xp, mask, fc, adaln)
    assert torch.isfinite(got[0, :T]).all() and torch.isfinite(got[1, :150]).all()
    ref = _compose(blocks, xp, [T, 150], fc, adaln)
    assert torch.equal(got[0, :T], ref[0, :T]) and torch.equal(got[1, :150], ref[1, :150])
    assert not torch.equal(got[1, :150], want[1, :150])                                                # (fewer keys: another result)
    for bad in (mask.float(), mask.flip(1)):
        with pytest.raises(NotImplementedError):
            blocks[0](xp, bad, fc, adaln)


def _prof_counts(fn):
    """-> (fn(), {"gemm": n, "quantize": n, "attention": n}): the library's launches while fn runs (svdq_prof_* event counters)"""
    import ctypes as C

    from nunchaku_amd import _lib
    lib = _lib.load()
    _lib.check(lib.svdq_prof_select((1 << 0) | (1 << 1) | (1 << 2)), "svdq_prof_select")
    _lib.check(lib.svdq_prof_enable(4096), "svdq_prof_enable")
    counts = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        for name, cls in (("gemm", 0), ("quantize", 1), ("attention", 2)):
            n, ms, work = C.c_int64(0), C.c_double(0), C.c_double(0)
            _lib.check(lib.svdq_prof_read(cls, C.byref(n), C.byref(ms), C.byref(work)), "svdq_prof_read")
            counts[name] = n.value
    finally:
        lib.svdq_prof_enable(0)
        lib.svdq_prof_select(0xFFFFFFFF)
    return out, counts


def test_launches_of_a_two_block_stack(strict_mode, monkeypatch):
    """B = 1, with modulation: one opening pass and two sandwich passes per block (behind the attention; behind the feed-forward, which opens the
    next block) = 5 ``svdq_sandwich_norm``, one ``svdq_qk_norm_rope`` and one ``svdq_attention`` per block, four quantiser and four GEMM launches
    per block as ``SVDQW4A4Linear`` makes them."""
    from nunchaku_amd.models import zimage

    blocks = _blocks(256, 2, 512, "bf16", True)
    x, fc, adaln = _acts(256, 1, 77, "bf16", seed=3)
    calls = {"sandwich_norm": 0, "qk_norm_rope": 0}
    for name in calls:
        real = getattr(zimage, name)
        monkeypatch.setattr(zimage, name, lambda *a, _real=real, _name=name, **k: (calls.__setitem__(_name, calls[_name] + 1), _real(*a, **k))[1])
    y, prof = _prof_counts(lambda: zimage.ZImageBlockStack(blocks)(x, None, fc, adaln))
    assert calls == {"sandwich_norm": 1 + 2 * 2, "qk_norm_rope": 2}
    assert prof == {"gemm": 8, "quantize": 8, "attention": 2}
    calls.update(sandwich_norm=0, qk_norm_rope=0)
    one, prof = _prof_counts(lambda: blocks[0](x, None, fc, adaln))
    assert calls == {"sandwich_norm": 3, "qk_norm_rope": 1} and prof == {"gemm": 4, "quantize": 4, "attention": 1}
