"""CPU restatements for the IP-Adapter tests (test infrastructure): the fp32 reference of ``svdq_ip_attention`` and the twin of
tests/flux_ref.py with the adapter's step behind the joint block (reference: nunchaku/models/ip_adapter/utils.py:346-372,
src/FluxModel.cpp ``forward_layer_ip_adapter`` / ``get_q_heads``)."""
import torch
import torch.nn.functional as F

from tests.flux_ref import Ref, r16

PREFIX = "double_blocks."


def ip_attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float | None = None) -> torch.Tensor:
    """fp32 ``softmax(scale * q k^T) v`` per head: q [T, H*D], k / v [N, H*D] (any float dtype) -> [T, H*D] float32, unrounded"""
    T, N = q.shape[0], k.shape[0]
    D = q.shape[1] // heads
    qh, kh, vh = (t.float().reshape(-1, heads, D).transpose(0, 1) for t in (q, k, v))
    s = qh @ kh.transpose(1, 2) * (D ** -0.5 if scale is None else scale)
    o = torch.softmax(s, dim=-1) @ vh
    assert o.shape == (heads, T, D) and s.shape == (heads, T, N)
    return o.transpose(0, 1).reshape(T, heads * D)


def adapter_state_dict(num_blocks: int, cross_dim: int, dim: int, seed: int = 0, weight_scale: float = 1.0, dtype=torch.bfloat16) -> dict:
    """A synthetic IP-Adapter file's content with the reference's key names"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in range(num_blocks):
        for n in ("k", "v"):
            base = f"{PREFIX}{i}.processor.ip_adapter_double_stream_{n}_proj"
            sd[base + ".weight"] = (torch.randn(dim, cross_dim, generator=g) * (weight_scale / cross_dim ** 0.5)).to(dtype)
            sd[base + ".bias"] = (torch.randn(dim, generator=g) * 0.02).to(dtype)
    return sd


class IPARef(Ref):
    """``Ref`` with an IP-Adapter: ``sd`` is the adapter's state dict, ``embeds`` the image embeddings [..., cross_dim] (16-bit values),
    ``scale`` the strength (a Python float: torch multiplies a 16-bit tensor by it in fp32 and rounds once)."""

    def __init__(self, model, layers, sd, embeds, scale: float):
        super().__init__(model, layers)
        self.sd, self.embeds, self.scale = sd, embeds.float().reshape(-1, embeds.shape[-1]), float(scale)

    def ip_linear(self, i, n):
        base = f"{PREFIX}{i}.processor.ip_adapter_double_stream_{n}_proj"
        return r16(F.linear(self.embeds, self.sd[base + ".weight"].float(), self.sd[base + ".bias"].float()))

    def ip_step(self, hidden, control, mm, rot_img, i=0):
        """steps 1-5 behind joint block ``i``: the query from the block's OUTPUT (before the ControlNet residual), the residual, the add"""
        b = self.m.blocks[i]
        k_img, v_img = self.ip_linear(i, "k"), self.ip_linear(i, "v")
        name = f"transformer_blocks.{i}.attn.to_qkv"
        dim = hidden.shape[-1]
        ip_query = self.qkv(name, self.ln_mod(hidden, mm[1], mm[0]), b.attn.norm_q.weight, b.attn.norm_k.weight, rot_img)[:, :dim]
        if control is not None:
            hidden = r16(hidden + control)
        o = r16(ip_attention_ref(ip_query, k_img, v_img, b.attn.heads))
        s32 = torch.tensor(self.scale, dtype=torch.float32)
        return r16(hidden + r16(s32 * o))

    def forward(self, lat, enc, pooled, t, img_ids, txt_ids, g, control=None, control_single=None):
        """``Ref.forward`` (1 joint + 1 single block) with :meth:`ip_step` between the joint block and the ControlNet residual"""
        from nunchaku_amd.models.embeddings import flux_pos_embed
        from nunchaku_amd.models.flux import timestep_embedding
        m = self.m
        emb = lambda e, x: self.lin(e.linear_2, r16(F.silu(self.lin(e.linear_1, x))))
        hidden = self.lin(m.x_embedder, lat)
        temb = emb(m.time_embed, r16(timestep_embedding(r16(r16(t) * 1000))))
        if m.guidance_embed is not None:
            temb = r16(temb + emb(m.guidance_embed, r16(timestep_embedding(r16(r16(g) * 1000)))))
        temb = r16(temb + emb(m.text_embed, pooled))
        ta = r16(F.silu(temb))
        e = self.lin(m.context_embedder, enc)
        rot = flux_pos_embed(torch.cat([txt_ids, img_ids], 0), m.axes)[0, :, :, 0].numpy()
        tt = e.shape[0]
        b = m.blocks[0]
        mm = self.awq("transformer_blocks.0.norm1.linear", ta).view(-1, 6).T
        cc = self.awq("transformer_blocks.0.norm1_context.linear", ta).view(-1, 6).T
        n_h, n_e = self.ln_mod(hidden, mm[1], mm[0]), self.ln_mod(e, cc[1], cc[0])
        qkv = torch.cat([self.qkv("transformer_blocks.0.attn.add_qkv_proj", n_e, b.attn.norm_added_q.weight, b.attn.norm_added_k.weight, rot[:tt]),
                         self.qkv("transformer_blocks.0.attn.to_qkv", n_h, b.attn.norm_q.weight, b.attn.norm_k.weight, rot[tt:])])
        o = self.attend(qkv, b.attn.heads)
        a, ca = self.svdq("transformer_blocks.0.attn.to_out.0", o[tt:]), self.svdq("transformer_blocks.0.attn.to_add_out", o[:tt])
        hidden = r16(hidden + r16(mm[2][None] * a))
        hidden = r16(hidden + r16(mm[5][None] * self.mlp("transformer_blocks.0.ff.net.0.proj", "transformer_blocks.0.ff.net.2", self.ln_mod(hidden, mm[4], mm[3]))))
        e = r16(e + r16(cc[2][None] * ca))
        e = r16(e + r16(cc[5][None] * self.mlp("transformer_blocks.0.ff_context.net.0.proj", "transformer_blocks.0.ff_context.net.2", self.ln_mod(e, cc[4], cc[3]))))
        hidden = self.ip_step(hidden, control, mm, rot[tt:])  # the ControlNet residual of the block, then the adapter's add
        x = torch.cat([e, hidden])
        s = m.single_blocks[0]
        sm = self.awq("single_transformer_blocks.0.norm.linear", ta).view(-1, 3).T
        n = self.ln_mod(x, sm[1], sm[0])
        mlp = self.mlp("single_transformer_blocks.0.mlp_fc1", "single_transformer_blocks.0.mlp_fc2", n)
        att = self.svdq("single_transformer_blocks.0.attn.to_out",
                        self.attend(self.qkv("single_transformer_blocks.0.attn.to_qkv", n, s.attn.norm_q.weight, s.attn.norm_k.weight, rot), s.attn.heads))
        x = r16(x + r16(sm[2][None] * r16(att + mlp)))[tt:]
        if control_single is not None:
            x = r16(x + control_single)
        sc, sh = self.lin(m.norm_out_mod, ta).chunk(2, dim=-1)
        x = r16(r16(F.layer_norm(x, (x.shape[-1],), eps=1e-6)) * r16(1 + sc) + sh)
        return self.lin(m.proj_out, x)
