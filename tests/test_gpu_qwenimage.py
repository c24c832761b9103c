"""Qwen-Image block (BASELINE config 5) on the GPU: parity against a CPU twin that follows
the reference's op sequence (NunchakuQwenImageTransformerBlock + NunchakuQwenImageNaiveFA2Processor) with the numpy oracle
for every quantised operator; the fused path (RMSNorm + RoPE in the QKV epilogue, this library's attention kernel, grouped
launches) against the reference-op path on the GPU; and the layer-wise host offload against the resident model, bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import svdq_oracle as O
from tests.flux_ref import DT, psnr_rel, r16
from tests.helpers import reference_state_dict

pytestmark = pytest.mark.gpu


def _fill(model, seed=0, lowrank_energy=0.9):
    from nunchaku_amd.models.linear import AWQW4A16Linear, SVDQW4A4Linear

    torch.manual_seed(seed)
    layers = {}
    with torch.no_grad():
        for name, mod in model.named_modules():
            if isinstance(mod, SVDQW4A4Linear):
                L = O.make_svdq_layer(mod.in_features, mod.out_features, 32, seed=seed * 1000 + len(layers), dtype=DT, cheap=False,
                                      svd="randomized", lowrank_energy=lowrank_energy)
                layers[name] = L
                mod.load_state_dict({k: v.cuda() for k, v in reference_state_dict(L, DT).items()})
            elif isinstance(mod, AWQW4A16Linear):
                rng = np.random.default_rng(seed * 1000 + 500 + len(layers))
                w = O.round16(rng.standard_normal((mod.out_features, mod.in_features)).astype(np.float32) / mod.in_features ** 0.5, DT)
                q, s_, z_ = O.awq_quantize_ref(w, DT)
                bias = O.round16(rng.standard_normal(mod.out_features).astype(np.float32) * 0.02, DT)
                layers[name] = {"q": q, "s": s_, "z": z_, "bias": bias}
                mod.load_state_dict({"qweight": torch.from_numpy(O.pack_awq_w4_ref(q)).cuda(), "wscales": torch.from_numpy(s_).cuda().bfloat16(),
                                     "wzeros": torch.from_numpy(z_).cuda().bfloat16(), "bias": torch.from_numpy(bias).cuda().bfloat16()})
            elif isinstance(mod, torch.nn.Linear):
                mod.weight.copy_(torch.randn_like(mod.weight, dtype=torch.float32) / mod.in_features ** 0.5)
                mod.bias.copy_(torch.randn_like(mod.bias, dtype=torch.float32) * 0.02)
            elif isinstance(mod, torch.nn.RMSNorm):
                mod.weight.copy_(1 + 0.1 * torch.randn_like(mod.weight, dtype=torch.float32))
    return layers


class BlockTwin:
    """CPU forward of one Qwen-Image block, the reference's op sequence with one 16-bit rounding per torch op."""

    def __init__(self, block, layers, prefix=""):
        self.b, self.L, self.p = block, layers, prefix

    def svdq(self, name, x):
        return torch.from_numpy(O.svdq_linear(x.numpy(), self.L[self.p + name], DT, "fp32")["out"])

    def awq(self, name, x):
        L = self.L[self.p + name]
        return torch.from_numpy(O.awq_gemv_w4a16(x.numpy(), L["q"], L["s"], L["z"], DT, bias=L["bias"]))

    def mlp(self, name, x):
        return torch.from_numpy(O.fused_gelu_mlp(x.numpy(), self.L[self.p + name + ".net.0.proj"], self.L[self.p + name + ".net.2"], DT))

    @staticmethod
    def modulate(x, shift, scale, gate):
        n = r16(F.layer_norm(x, (x.shape[-1],), eps=1e-6))
        return r16(r16(n * r16(scale + 1.0)[None]) + shift[None]), gate

    @staticmethod
    def rms(x, w):  # nn.RMSNorm on a 16-bit tensor: fp32 inside, 16-bit out
        return r16(x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * w.float().cpu())

    @staticmethod
    def rot(x, cs):  # x [T, H, 128], cs [T, 64, (cos, sin)]
        xf = x.unflatten(-1, (-1, 2))
        c, s = cs[:, None, :, 0], cs[:, None, :, 1]
        return r16(torch.stack([xf[..., 0] * c - xf[..., 1] * s, xf[..., 0] * s + xf[..., 1] * c], dim=-1).flatten(-2))

    def forward(self, hidden, enc, temb, img_cs, txt_cs):
        b = self.b
        H = b.attn.heads
        ta = r16(F.silu(temb))
        im = self.awq("img_mod.1", ta).view(-1, 6).T  # rows: shift1 scale1 gate1 shift2 scale2 gate2
        tm = self.awq("txt_mod.1", ta).view(-1, 6).T
        ix, ig1 = self.modulate(hidden, im[0], im[1], im[2])
        tx, tg1 = self.modulate(enc, tm[0], tm[1], tm[2])

        def stream(x, proj, nq, nk, cs):
            q, k, v = (t.reshape(-1, H, 128) for t in self.svdq(proj, x).chunk(3, dim=-1))
            return self.rot(self.rms(q, nq.weight), cs), self.rot(self.rms(k, nk.weight), cs), v

        tq, tk, tv = stream(tx, "attn.add_qkv_proj", b.attn.norm_added_q, b.attn.norm_added_k, txt_cs)
        iq, ik, iv = stream(ix, "attn.to_qkv", b.attn.norm_q, b.attn.norm_k, img_cs)
        q, k, v = (torch.cat(p, 0).transpose(0, 1) for p in ((tq, iq), (tk, ik), (tv, iv)))
        o = r16((torch.softmax(q @ k.transpose(1, 2) / 128 ** 0.5, dim=-1) @ v).transpose(0, 1).reshape(-1, H * 128))
        tt = enc.shape[0]
        hidden = r16(hidden + r16(ig1[None] * self.svdq("attn.to_out.0", o[tt:])))
        enc = r16(enc + r16(tg1[None] * self.svdq("attn.to_add_out", o[:tt])))
        ix2, ig2 = self.modulate(hidden, im[3], im[4], im[5])
        hidden = r16(hidden + r16(ig2[None] * self.mlp("img_mlp", ix2)))
        tx2, tg2 = self.modulate(enc, tm[3], tm[4], tm[5])
        enc = r16(enc + r16(tg2[None] * self.mlp("txt_mlp", tx2)))
        return enc, hidden


def _block_inputs(dim, t_img, t_txt, seed=1, grid=None):
    from nunchaku_amd.models.qwenimage import qwen_rope_freqs

    g = torch.Generator().manual_seed(seed)
    side = int(t_img ** 0.5)
    grid = grid or (side, side)
    assert grid[0] * grid[1] == t_img
    hidden = r16(torch.randn(t_img, dim, generator=g))
    enc = r16(torch.randn(t_txt, dim, generator=g))
    temb = r16(torch.randn(1, dim, generator=g))
    img_f, txt_f = qwen_rope_freqs((1, grid[0], grid[1]), t_txt)
    return hidden, enc, temb, img_f, txt_f


@pytest.mark.parametrize("t_txt", [256, 128], ids=["grouped", "separate"])
def test_qwen_block_matches_the_reference_op_sequence(t_txt):
    from nunchaku_amd.models.qwenimage import NunchakuQwenAttention, NunchakuQwenImageTransformerBlock

    dim, t_img = 256, 256
    block = NunchakuQwenImageTransformerBlock(dim, 2, 128, device="cuda").eval()
    layers = _fill(block, seed=3)
    hidden, enc, temb, img_f, txt_f = _block_inputs(dim, t_img, t_txt)
    cs = lambda f: torch.stack([f.real.float(), f.imag.float()], dim=-1)
    with torch.no_grad():
        e_ref, h_ref = BlockTwin(block, layers).forward(hidden, enc, temb, cs(img_f), cs(txt_f))
        outs = {}
        for fused in (True, False):
            NunchakuQwenAttention.fused_qkv = fused
            try:
                e, h = block(hidden.cuda().bfloat16()[None], enc.cuda().bfloat16()[None], None, temb.cuda().bfloat16(),
                             (img_f.cuda(), txt_f.cuda()))
            finally:
                NunchakuQwenAttention.fused_qkv = True
            outs[fused] = (e[0].float().cpu(), h[0].float().cpu())
    for fused, (e, h) in outs.items():
        for name, got, ref in (("text", e, e_ref), ("image", h, h_ref)):
            psnr, rel = psnr_rel(got, ref)
            print(f"qwen block fused={fused} {name}: PSNR {psnr:.1f} dB rel {rel:.2e}")
            # measured 67.9 - 71.3 dB / 0.13 - 0.18 % (round 4); round 3 gated at 45 dB / 2 %
            assert torch.isfinite(got).all() and psnr > 60.0 and rel < 6e-3, (fused, name, psnr, rel)
    # the fused path (QKV epilogue + svdq attention, grouped when t_txt % 256 == 0) against the reference-op path on the GPU
    for i in range(2):
        psnr, _ = psnr_rel(outs[True][i], outs[False][i])
        assert psnr > 55.0, psnr


def _small_model(layers=4, rank=32):
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    return NunchakuQwenImageTransformer2DModel(num_layers=layers, num_attention_heads=2, attention_head_dim=128, in_channels=64,
                                               out_channels=16, joint_attention_dim=128, rank=rank, device="cuda").init_synthetic_(seed=5).eval()


def _fragment_images(blocks) -> dict:
    """(block, parameter, cache key) -> the cached MFMA-fragment image (nunchaku_amd._C._packed_fragments) of every low-rank factor of ``blocks``"""
    from nunchaku_amd import _C

    out = {}
    for i, b in enumerate(blocks):
        for name, p in b.named_parameters():
            for k, v in (_C._converted.get(p) or {}).items():
                if k[0].startswith("frag_") and (k[1], k[2]) == (p.storage_offset(), tuple(p.shape)):
                    out[(i, name, k)] = v[1]
    return out


def test_qwen_model_offload_auto_keeps_every_block_that_fits():
    """num_blocks_on_gpu="auto" (round 6): the reference's default of one resident block is sized for a 16-24 GB card; on a 288 GB part every block that fits in
    three quarters of the free memory stays resident -- for this small model all of them: nothing is offloaded, nothing crosses the link, the forward is the resident one
    bit for bit (deterministic mode), and an explicit count still offloads."""
    from nunchaku_amd import mode
    from nunchaku_amd.models.offload import CPUOffloadManager

    g = torch.Generator(device="cuda").manual_seed(9)
    lat = torch.randn(1, 256, 64, device="cuda", generator=g).bfloat16()
    enc = torch.randn(1, 256, 128, device="cuda", generator=g).bfloat16()
    t = torch.tensor([0.6], device="cuda")
    with torch.no_grad(), mode.deterministic_mode():
        model = _small_model(4)
        ref = model(lat, enc, None, t, [(1, 16, 16)]).sample.clone()
        fit = CPUOffloadManager.blocks_that_fit(list(model.transformer_blocks), "cuda", num_slots=2)
        assert fit == 4, fit
        model.set_offload(True, num_blocks_on_gpu="auto", num_slots=2)
        mgr = model.offload_manager
        assert mgr.num_blocks_on_gpu == 4 and mgr.n_offloaded == 0 and not mgr._images
        assert torch.equal(model(lat, enc, None, t, [(1, 16, 16)]).sample, ref)
        assert torch.equal(model(lat, enc, None, t, [(1, 16, 16)]).sample, ref)
        model.set_offload(False)
        assert torch.equal(model(lat, enc, None, t, [(1, 16, 16)]).sample, ref)
    with pytest.raises(ValueError):
        CPUOffloadManager(list(model.transformer_blocks), num_blocks_on_gpu="all")


_OFFLOAD_VARIANTS = [(False, 2, "nibbles"), (True, 2, "after-first-forward"), (False, 3, "three-slots")]


# rank 32 (no fragment images: the control) keeps the variants' plain ids; ranks 64 .. 160 use the fragment cache
@pytest.mark.parametrize("late,num_slots,rank", [pytest.param(late, slots, rank, id=name if rank == 32 else f"{name}-r{rank}")
                                                 for rank in (32, 64, 128, 160) for late, slots, name in _OFFLOAD_VARIANTS])
def test_qwen_model_offload_equals_resident(late, num_slots, rank):
    """set_offload(True): blocks live in pinned host memory (their tensors are views of one flat image each), a ring of device
    slots, copies on a side stream ahead of the compute.  In deterministic mode (fixed-point low-rank accumulation: no
    run-to-run noise) offloaded forwards must equal the resident model BIT FOR BIT -- over several forwards (the ring wraps and
    continues across forwards), whether offload is switched on before the first forward or after it (layers already repacked:
    their code tensors are converted back to nibbles for the link), with two or three slots.  After every block load the slot's
    parameters are compared with the host image bit for bit; after set_offload(False) the model runs resident again.

    Ranks 48 .. 160 keep MFMA-fragment images of the low-rank factors per (storage, version) (ABI 21, ``_C._packed_fragments``): every
    block load into a slot must re-pack them (a stale image runs the low-rank branch with the previous tenant's weights), the slot's
    cache entries are replaced rather than added, and a resident block's images are packed once.  The kernels read those images only
    with fp32 low-rank accumulators, whose run-to-run noise hides a stale image in the model's output, so before every load the images
    the cache would serve for the slot's outgoing tenant are compared with a fresh pack of the slot's weights.  Rank 32 uses no images:
    the control."""
    from nunchaku_amd import _C, layout, mode
    from nunchaku_amd.models.linear import SVDQW4A4Linear
    from tests.helpers import served_fragment_images

    g = torch.Generator(device="cuda").manual_seed(9)
    lat = torch.randn(1, 256, 64, device="cuda", generator=g).bfloat16()
    enc = torch.randn(1, 256, 128, device="cuda", generator=g).bfloat16()
    t = torch.tensor([0.6], device="cuda")
    n_blocks, nb = 6, 2
    with torch.no_grad(), mode.deterministic_mode():
        resident = _small_model(n_blocks, rank)
        ref = resident(lat, enc, None, t, [(1, 16, 16)]).sample.clone()
        assert torch.equal(resident(lat, enc, None, t, [(1, 16, 16)]).sample, ref), "deterministic mode: resident forwards differ"
        model = resident if late else _small_model(n_blocks, rank)  # same seed: same weights
        model.set_offload(True, num_blocks_on_gpu=nb, use_pin_memory=True, num_slots=num_slots)
        mgr = model.offload_manager
        assert len(mgr.buffer_blocks) == num_slots and mgr.n_offloaded == n_blocks - nb
        assert all(next(b.parameters()).is_cuda for b in mgr.blocks[:nb])
        for i in range(nb, n_blocks):  # host blocks: complete CPU modules whose tensors are views of ONE pinned image
            img = mgr._images[i]
            assert img.is_pinned() and not img.is_cuda
            lo, hi = img.data_ptr(), img.data_ptr() + img.numel()
            assert all(lo <= p.data_ptr() < hi and not p.is_cuda for p in mgr.blocks[i].parameters())
        fp6 = sum(m.qweight.numel() for m in mgr.buffer_blocks[0].modules() if isinstance(m, SVDQW4A4Linear))
        assert mgr.nibble_bytes() == fp6 * 2 // 3, "the link carries nibbles (2/3 of the FP6 image bytes), also for layers repacked before"

        # every load: the slot's parameters equal the host block's (code tensors: after re-expansion) bit for bit
        checked = []
        served = []  # (outgoing tenant, fragment images checked, parameters whose image is stale) before every load into a slot
        orig_load = mgr.load_block

        def checking_load(block_idx, non_blocking=True, slot=None):
            sl = mgr._slots[slot if slot is not None else (mgr._seq + block_idx - nb) % mgr.num_slots]
            if sl.tenant >= 0:  # its compute has been issued: what the cache serves for the slot must be the outgoing tenant's factors
                served.append((sl.tenant, *served_fragment_images(sl.module)))
            orig_load(block_idx, non_blocking, slot)
            if block_idx < nb or block_idx >= n_blocks:
                return
            torch.cuda.current_stream().synchronize()
            sl = mgr._slots[slot if slot is not None else (mgr._seq + block_idx - nb) % mgr.num_slots]
            assert sl.tenant == block_idx
            host = dict(mgr.blocks[block_idx].named_parameters())
            mods = dict(mgr.blocks[block_idx].named_modules())
            for name, p in sl.module.named_parameters():
                h = host[name]
                mn, _, tn = name.rpartition(".")
                if tn == "qweight" and isinstance(mods[mn], SVDQW4A4Linear):
                    assert torch.equal(p.data, layout.repack_qweight(h.data.cuda())), f"block {block_idx} {name}: FP6 image != expanded host nibbles"
                else:
                    assert torch.equal(p.data.cpu(), h.data), f"block {block_idx} {name}: slot != host image"
            checked.append(block_idx)

        mgr.load_block = checking_load
        got, slot_entries, resident_images = [], [], []
        for _ in range(3):
            got.append(model(lat, enc, None, t, [(1, 16, 16)]).sample.clone())
            slot_entries.append([len(_C._converted.get(s.flat) or {}) for s in mgr._slots])
            resident_images.append(_fragment_images(mgr.blocks[:nb]))
        torch.cuda.synchronize()
        mgr.load_block = orig_load
        assert mgr.forward_counter == 3 and mgr.current_block_idx == 0
        assert sorted(set(checked)) == list(range(nb, n_blocks)) and len(checked) >= 3 * (n_blocks - nb)
        for k, a in enumerate(got):
            assert torch.equal(a, ref), f"offloaded forward {k} (late={late}, slots={num_slots}) differs from the resident model: rel " \
                                        f"{((a.float() - ref.float()).norm() / ref.float().norm()).item():.3e}"
        # the fragment cache: a slot's entries are replaced by every new tenant, never added (bounded memory); resident blocks pack once
        assert slot_entries[0] == slot_entries[1] == slot_entries[2], f"cache entries per slot storage grew across forwards: {slot_entries}"
        stale = [(tenant, names) for tenant, _, names in served if names]
        assert not stale, f"rank {rank}: the cache served fragment images of another block's low-rank factors (tenant, parameters): {stale[:2]}"
        if rank == 32:
            assert not any(slot_entries[0]) and not resident_images[0], "rank 32 keeps no fragment images"
            assert not any(n for _, n, _ in served)
        else:
            assert all(slot_entries[0]) and resident_images[0], (slot_entries[0], len(resident_images[0]))
            assert len(served) >= 2 * (n_blocks - nb) and all(n for _, n, _ in served), [n for _, n, _ in served]
        for imgs in resident_images[1:]:
            assert imgs.keys() == resident_images[0].keys() and all(imgs[k] is v for k, v in resident_images[0].items()), \
                "a resident block's fragment images must be packed once and reused"
        # a host block is still a loadable module: its state dict is the checkpoint-layout state dict of the resident twin
        twin = _small_model(n_blocks, rank)
        sd_host = mgr.blocks[nb].state_dict()
        sd_twin = twin.transformer_blocks[nb].state_dict()
        assert set(sd_host) == set(sd_twin)
        for k in sd_twin:
            assert torch.equal(sd_host[k].cpu(), sd_twin[k].cpu()), f"host block state_dict {k}"
        # a second set_device (same device, forced) rebuilds the slots and keeps working
        mgr.set_device(mgr.device, force=True)
        assert torch.equal(model(lat, enc, None, t, [(1, 16, 16)]).sample, ref)
        # offload off: the blocks come back as ordinary GPU modules and the model runs resident
        model.set_offload(False)
        assert model.offload_manager is None and all(p.is_cuda for p in model.parameters())
        assert torch.equal(model(lat, enc, None, t, [(1, 16, 16)]).sample, ref), "forward after set_offload(False)"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_qwen_model_fused_passes_match_the_torch_op_blocks(dtype):
    """The model's fused path (LayerNorm + modulation inside the quantisers, gated residuals + statistics in one pass, grouped
    launches, attention-side quantiser, one batched modulation GEMV per step) against the reference's torch-op block sequence on
    the same weights: the fused passes restate the torch ops' 16-bit rounding points, so the two agree up to the W4A4 code-flip
    level of a last-bit difference (fp32 summation orders of the attention / low-rank sums differ between the two paths)."""
    from nunchaku_amd import mode
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    model = NunchakuQwenImageTransformer2DModel(num_layers=3, num_attention_heads=2, attention_head_dim=128, in_channels=64, out_channels=16,
                                                joint_attention_dim=128, torch_dtype=dtype, device="cuda").init_synthetic_(seed=5).eval()
    g = torch.Generator(device="cuda").manual_seed(4)
    lat = torch.randn(1, 256, 64, device="cuda", generator=g).to(dtype)
    enc = torch.randn(1, 256, 128, device="cuda", generator=g).to(dtype)
    t = torch.tensor([0.4], device="cuda")
    outs = {}
    with torch.no_grad(), mode.deterministic_mode():
        for fused in (True, False):
            NunchakuQwenImageTransformer2DModel.fused_norm = fused
            try:
                outs[fused] = model(lat, enc, None, t, [(1, 16, 16)]).sample.float()
                again = model(lat, enc, None, t, [(1, 16, 16)]).sample.float()
            finally:
                NunchakuQwenImageTransformer2DModel.fused_norm = True
            assert torch.equal(outs[fused], again), f"fused={fused}: two forwards differ in deterministic mode"
        NunchakuQwenImageTransformer2DModel.batched_mods = False
        try:
            per_block = model(lat, enc, None, t, [(1, 16, 16)]).sample.float()
        finally:
            NunchakuQwenImageTransformer2DModel.batched_mods = True
    assert torch.equal(per_block, outs[True]), "batched modulation GEMVs differ from the per-block ones"
    psnr, rel = psnr_rel(outs[True], outs[False])
    print(f"qwen model fused vs torch-op blocks ({dtype}): PSNR {psnr:.1f} dB rel {rel:.2e}")
    # deterministic mode: measured 52.0 dB (bf16) / 48.5 dB (fp16) on this 3-block model with uniform-random weights (the code-flip floor, see
    # tests/test_gpu_fused_norm.py); round 3 gated at 40 dB / 3 %
    assert torch.isfinite(outs[True]).all() and psnr > 45.0 and rel < 2.5e-2, (psnr, rel)


def test_qwen_controlnet_residuals_on_the_fused_path():
    """`controlnet_block_samples` (reference transformer_qwenimage.py:546-550: hidden += samples[block // ceil(blocks / samples)] behind every block):
    the fused path (the add and the next LayerNorm's statistics in one pass) against the torch-op block sequence with a plain 16-bit add, at a token
    count that is padded (300 image tokens -> 512 rows: the padded rows get a zero residual) and with fewer samples than blocks."""
    from nunchaku_amd import mode
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    model = NunchakuQwenImageTransformer2DModel(num_layers=3, num_attention_heads=2, attention_head_dim=128, in_channels=64, out_channels=16,
                                                joint_attention_dim=128, device="cuda").init_synthetic_(seed=6).eval()
    g = torch.Generator(device="cuda").manual_seed(9)
    lat = torch.randn(1, 300, 64, device="cuda", generator=g).bfloat16()
    enc = torch.randn(1, 40, 128, device="cuda", generator=g).bfloat16()
    ctrl = [torch.randn(1, 300, 256, device="cuda", generator=g).bfloat16() * 0.5 for _ in range(2)]  # blocks 0, 1 -> sample 0; block 2 -> sample 1
    t = torch.tensor([0.4], device="cuda")
    outs = {}
    with torch.no_grad(), mode.deterministic_mode():
        plain = model(lat, enc, None, t, [(1, 15, 20)]).sample.float()
        for fused in (True, False):
            NunchakuQwenImageTransformer2DModel.fused_norm = fused
            try:
                outs[fused] = model(lat, enc, None, t, [(1, 15, 20)], controlnet_block_samples=ctrl).sample.float()
            finally:
                NunchakuQwenImageTransformer2DModel.fused_norm = True
        # the torch-op blocks with the add done here, outside the model: what the reference's loop computes
        NunchakuQwenImageTransformer2DModel.fused_norm = False
        try:
            hooks, k = [], [0]

            def add(_m, _inp, out):
                i = k[0]
                k[0] += 1
                smp = torch.nn.functional.pad(ctrl[i // 2], (0, 0, 0, out[1].shape[1] - 300))
                return out[0], out[1] + smp
            for b in model.transformer_blocks:
                hooks.append(b.register_forward_hook(add))
            by_hand = model(lat, enc, None, t, [(1, 15, 20)]).sample.float()
        finally:
            for h in hooks:
                h.remove()
            NunchakuQwenImageTransformer2DModel.fused_norm = True
    assert plain.shape == (1, 300, 64) and torch.isfinite(outs[True]).all()
    assert torch.equal(outs[False], by_hand), "torch-op path: the model's ControlNet add differs from the reference loop's"
    assert not torch.equal(outs[True], plain)
    psnr, rel = psnr_rel(outs[True], outs[False])
    print(f"qwen controlnet fused vs torch-op blocks: PSNR {psnr:.1f} dB rel {rel:.2e}")
    assert psnr > 45.0 and rel < 2.5e-2, (psnr, rel)


def test_qwen_rope_tables():
    from nunchaku_amd.models.qwenimage import pack_qwen_rotary, qwen_rope_freqs

    img, txt = qwen_rope_freqs((1, 16, 16), 40)
    assert img.shape == (256, 64) and txt.shape == (40, 64) and img.dtype == torch.complex64
    assert torch.allclose(img.abs(), torch.ones(256, 64)) and torch.allclose(txt.abs(), torch.ones(40, 64))
    # centred positions: row h of the grid carries position h - 8 on the height axis (56 dims = 28 complex, after the 8 of the frame axis)
    assert torch.allclose(img[8 * 16, 8:36], torch.ones(28, dtype=torch.complex64), atol=1e-6)  # height position 0
    p = pack_qwen_rotary(img, txt)
    assert p["img"].shape == (1, 256, 128) and p["txt"].shape == (1, 256, 128) and p["all"].shape == (1, 512, 128)


def _launch_counts(fn):
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


def _attention_launches(fn):
    out, counts = _launch_counts(fn)
    return out, counts["attention"]


# the reference's own Qwen-Image quality gate runs 1664 x 928 (tests/v1/qwenimage/test_qwenimage.py:21,118): a 58 x 104 grid of
# 2 x 2 latent patches = 6032 image tokens, and a prompt's text length is arbitrary.  The block on padded streams ([text | pad | image | pad],
# padded keys masked by the attention kernel) against the twin of the reference's op sequence at the natural sizes.
@pytest.mark.parametrize("grid,t_txt", [((58, 104), 37), ((13, 20), 300)], ids=["1664x928", "320x208"])
def test_qwen_block_on_padded_streams_matches_the_reference_op_sequence(grid, t_txt):
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformerBlock, pack_qwen_rotary
    from nunchaku_amd.ops.attention import kv_valid_ranges

    dim, t_img = 256, grid[0] * grid[1]
    block = NunchakuQwenImageTransformerBlock(dim, 2, 128, device="cuda").eval()
    layers = _fill(block, seed=4)
    hidden, enc, temb, img_f, txt_f = _block_inputs(dim, t_img, t_txt, seed=2, grid=grid)
    cs = lambda f: torch.stack([f.real.float(), f.imag.float()], dim=-1)
    kv = kv_valid_ranges(t_txt, t_img)
    assert kv is not None and len(kv) == 3  # padding in the middle of the joint sequence
    pad = lambda x: F.pad(x.cuda().bfloat16(), (0, 0, 0, -x.shape[0] % 256))[None]
    with torch.no_grad():
        e_ref, h_ref = BlockTwin(block, layers).forward(hidden, enc, temb, cs(img_f), cs(txt_f))
        (e, h), launches = _attention_launches(lambda: block(pad(hidden), pad(enc), None, temb.cuda().bfloat16(),
                                                             pack_qwen_rotary(img_f.cuda(), txt_f.cuda()), kv_valid=kv))
    assert launches == 1, "the block did not run svdq_attention"
    for name, got, ref in (("text", e[0, :t_txt].float().cpu(), e_ref), ("image", h[0, :t_img].float().cpu(), h_ref)):
        psnr, rel = psnr_rel(got, ref)
        print(f"qwen block {grid} + {t_txt} tokens, padded streams, {name}: PSNR {psnr:.1f} dB rel {rel:.2e}")
        assert torch.isfinite(got).all() and psnr > 58.0 and rel < 6e-3, (name, psnr, rel)  # measured 64.7 - 68.6 dB
    assert torch.isfinite(e).all() and torch.isfinite(h).all()  # the padded rows stay finite (they are V^T columns of the next block)


@pytest.mark.parametrize("rank", [32, 64, 128], ids=["r32", "r64", "r128"])
def test_qwen_model_odd_token_counts_run_the_fused_path(rank):
    """The model pads both streams itself and keeps the fused path -- with the pipeline's real call signature (an all-ones
    ``encoder_hidden_states_mask``, ignored as the reference's processor ignores it) -- against the reference's torch-op block sequence with no
    padding anywhere.  Every rank takes the same launches since round 5 (rank > 32 used to leave the attention epilogue's quantiser, the
    staged epilogue operands and the quantiser's fast path): the launch counters of rank 64 / 128 (the reference's r128 checkpoints,
    tests/v1/qwenimage/test_qwenimage.py:20-26) equal rank 32's -- no stand-alone quantiser behind the attention, no extra GEMM."""
    from nunchaku_amd import mode
    from nunchaku_amd.models.qwenimage import NunchakuQwenAttention, NunchakuQwenImageTransformer2DModel

    layers, grid, t_txt = 2, (13, 20), 37
    model = NunchakuQwenImageTransformer2DModel(num_layers=layers, num_attention_heads=2, attention_head_dim=128, in_channels=64, out_channels=16,
                                                joint_attention_dim=128, rank=rank, device="cuda").init_synthetic_(seed=7).eval()
    g = torch.Generator(device="cuda").manual_seed(2)
    lat = torch.randn(1, grid[0] * grid[1], 64, device="cuda", generator=g).bfloat16()
    enc = torch.randn(1, t_txt, 128, device="cuda", generator=g).bfloat16()
    mask = torch.ones(1, t_txt, dtype=torch.long, device="cuda")
    t = torch.tensor([0.3], device="cuda")
    call = lambda: model(lat, enc, mask, t, [(1, grid[0], grid[1])], txt_seq_lens=[t_txt]).sample.float()
    with torch.no_grad(), mode.deterministic_mode():
        hot, counts = _launch_counts(call)
        assert counts["attention"] == layers, f"{counts['attention']} svdq_attention launches for {layers} blocks"
        if rank != 32:  # the same launches as the rank-32 model: nothing fell back to an unfused sequence
            m32 = NunchakuQwenImageTransformer2DModel(num_layers=layers, num_attention_heads=2, attention_head_dim=128, in_channels=64, out_channels=16,
                                                      joint_attention_dim=128, rank=32, device="cuda").init_synthetic_(seed=7).eval()
            _, c32 = _launch_counts(lambda: m32(lat, enc, mask, t, [(1, grid[0], grid[1])], txt_seq_lens=[t_txt]).sample)
            print(f"launches per step, rank 32: {c32}; rank {rank}: {counts}")
            assert counts == c32, (counts, c32)
            del m32
        assert torch.equal(hot, call())
        NunchakuQwenImageTransformer2DModel.padded_tokens, NunchakuQwenAttention.fused_qkv = False, False
        try:
            plain, launches = _attention_launches(call)
        finally:
            NunchakuQwenImageTransformer2DModel.padded_tokens, NunchakuQwenAttention.fused_qkv = True, True
        assert launches == 0
    assert hot.shape == plain.shape == (1, grid[0] * grid[1], 64) and torch.isfinite(hot).all()
    psnr, rel = psnr_rel(hot.cpu(), plain.cpu())
    print(f"qwen model rank {rank}, {grid} + {t_txt} tokens: padded fused path vs unpadded torch-op blocks {psnr:.1f} dB rel {rel:.2e}")
    assert psnr > 42.0 and rel < 3e-2, (psnr, rel)  # measured 45.9 - 46.1 dB: two op sequences on uniform-random weights (code-flip floor)
