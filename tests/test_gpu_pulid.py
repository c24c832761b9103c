"""svdq_pulid_ca on the GPU: the folded identity cross-attention of PuLID.

Each stage of the kernel is held against its own input.  The two epilogues (the softmax with the LayerNorm in front of it; the output
rule) are restated operation by operation in tests/pulid_ref.py and must be BIT-EQUAL, starting from the accumulators the kernel hands
out (``acc``, ``o_acc``).  The order in which the matrix core adds an accumulator's terms is not restated on the CPU; the accumulators
are held to float64 within the bound of an fp32 sum of K exact products in ANY order, ``K * 2^-23 * sum|terms|`` (K = C for the scores,
K = H * 32 for the output; 16-bit x 16-bit products are exact in fp32; 2^-23, one unit in the last place per addition, holds whichever
way the matrix core's adder rounds).  Then the fused module against the float64 reference composition
next to the module's own 16-bit torch-op sequence, the structural properties, and the engine hook on a FLUX-shaped model."""


import pytest
import torch

from tests import pulid_ref as ref

pytestmark = pytest.mark.gpu

TD = ref.TD
U32 = 2.0 ** -23
# (T, C, H, N): one row; a partial tile and few tokens; one token and three row tiles; every head; the FLUX shape over nine row tiles; seven tokens
SHAPES = [(1, 128, 4, 32), (33, 256, 4, 5), (130, 256, 8, 1), (257, 384, 16, 32), (513, 3072, 16, 32), (129, 3072, 16, 7)]
_CACHE: dict = {}


def _fold(C, H, N, dtype, seed=0):
    """a module of width C with H heads (head dimension 32, kv_dim 64: the kernel sees the fold only) and its fold of N identity tokens"""
    mod = ref.make_module(C, H, 64, 32, seed=seed, dtype=TD[dtype], device="cuda")
    emb = torch.randn(1, N, 64, generator=torch.Generator().manual_seed(seed + 50)).to(TD[dtype]).cuda()
    return mod, emb, mod.fold(emb)


def _run(T, C, H, N, dtype, out_scale=1.0):
    """one call with strided x and out and both accumulators handed out; computed once per case and shared"""
    key = (T, C, H, N, dtype, out_scale)
    if key not in _CACHE:
        from nunchaku_amd.ops.attention import pulid_ca
        from nunchaku_amd.ops.elementwise import residual_gate_stats

        _, _, fold = _fold(C, H, N, dtype)
        x = ref.stream_inputs(T, C, T + N, TD[dtype], "cuda", ld=C + 64)
        assert x.stride(0) == C + 64
        stats = residual_gate_stats(x, eps=1e-5)[1]
        sentinel = -77.0
        big = torch.full((T + 3, C + 72), sentinel, dtype=TD[dtype], device="cuda")
        out = big[:T, 8:8 + C]
        acc = torch.empty(T, H * 32, dtype=torch.float32, device="cuda")
        o_acc = torch.empty(T, C, dtype=torch.float32, device="cuda")
        got, probs = pulid_ca(x, fold, out_scale=out_scale, stats=stats, out=out, return_probs=True, acc=acc, o_acc=o_acc)
        assert got is out
        assert (big[T:] == sentinel).all() and (big[:T, :8] == sentinel).all() and (big[:T, 8 + C:] == sentinel).all()
        _CACHE[key] = dict(fold=fold, x=x, stats=stats, out=out.clone(), probs=probs, acc=acc, o_acc=o_acc)
    return _CACHE[key]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("T,C,H,N", SHAPES)
def test_each_stage_equals_the_restatement_from_its_own_input(T, C, H, N, dtype):
    r = _run(T, C, H, N, dtype, out_scale=0.7)
    fold, x = r["fold"], r["x"]
    valid = (torch.arange(H * 32) % 32 < N)
    # stage 1, the matrix core: acc against float64 within K u sum|terms|, K = C
    xd, ad = x.double().cpu(), fold.a_fold.double().cpu()
    acc64, mag = xd @ ad.T, xd.abs() @ ad.abs().T
    err = (r["acc"].double().cpu() - acc64).abs()[:, valid]
    bound = (C * U32 * mag)[:, valid]
    print(f"({T},{C},{H},{N}) {dtype}: acc max error {err.max():.3g}, largest bound {bound.max():.3g}, worst ratio {(err / bound).max():.3g}")
    assert (err <= bound).all()
    # the scores that follow from it, against float64 from the same statistics: the same bound through rstd, plus the fp32 roundings of the
    # three epilogue operations on terms of size |mean colsum|, |acc| and |s|
    stats = r["stats"].double().cpu()
    s_k = stats[:, 1:2] * (r["acc"].double().cpu() - stats[:, 0:1] * fold.colsum.double().cpu()[None]) + fold.cbias.double().cpu()[None]
    s_64 = stats[:, 1:2] * (acc64 - stats[:, 0:1] * fold.colsum.double().cpu()[None]) + fold.cbias.double().cpu()[None]
    assert ((s_k - s_64).abs()[:, valid] <= (stats[:, 1:2] * C * U32 * mag)[:, valid] + 1e-12).all()
    # stage 1, the epilogue: bit-equal from the kernel's own accumulator
    want = ref.probs_from_acc(r["acc"], r["stats"], fold.colsum, fold.cbias, N, TD[dtype])
    assert torch.equal(r["probs"].cpu(), want), f"{(r['probs'].cpu() != want).sum().item()} of {want.numel()} probabilities differ"
    assert (r["probs"].cpu()[:, ~valid] == 0).all()
    # stage 2, the matrix core: o against float64 from the kernel's own probabilities, K = H * 32
    pd, bd = r["probs"].double().cpu(), fold.b_fold.double().cpu()
    o64, omag = pd @ bd, pd.abs() @ bd.abs()
    oerr = (r["o_acc"].double().cpu() - o64).abs()
    print(f"({T},{C},{H},{N}) {dtype}: o max error {oerr.max():.3g}, worst ratio {(oerr / (H * 32 * U32 * omag + 1e-30)).max():.3g}")
    assert (oerr <= H * 32 * U32 * omag + 1e-30).all()
    # stage 2, the epilogue: bit-equal from the kernel's own accumulator
    assert torch.equal(r["out"].cpu(), ref.out_from_o(r["o_acc"], 0.7, TD[dtype]))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("T,dim,heads,dim_head,kv_dim,N", [(257, 384, 16, 128, 64, 32), (129, 3072, 16, 128, 2048, 7), (513, 3072, 16, 128, 2048, 32)])
def test_fused_module_is_as_accurate_as_the_torch_op_sequence(T, dim, heads, dim_head, kv_dim, N, dtype):
    """Against the float64 reference composition the fused module's max and mean error are at most 1.5 x those of
    ``PerceiverAttentionCA.forward`` on the GPU in the same dtype on the same inputs (the margin of tests/test_gpu_zimage_block.py for a
    fused path against torch's).  Measured ratios: profiles/pulid.txt."""
    td = TD[dtype]
    mod = ref.make_module(dim, heads, kv_dim, dim_head, seed=3, dtype=td, device="cuda")
    emb = torch.randn(1, N, kv_dim, generator=torch.Generator().manual_seed(8)).to(td).cuda()
    lat = ref.stream_inputs(T, dim, 11, td, "cuda")
    with torch.no_grad():
        fused = mod.forward_fused(emb, lat).double().cpu()
        torch16 = mod(emb, lat[None])[0].double().cpu()
    want = ref.compose64(mod, emb, lat)
    e_f, e_t = (fused - want).abs(), (torch16 - want).abs()
    print(f"accuracy T={T} dim={dim} N={N} {dtype}: fused max {e_f.max():.4g} mean {e_f.mean():.4g}; torch ops max {e_t.max():.4g} mean {e_t.mean():.4g}; "
          f"ratios max {e_f.max() / e_t.max():.3f} mean {e_f.mean() / e_t.mean():.3f}  (|ref| max {want.abs().max():.3g})")
    assert torch.isfinite(fused).all()
    assert e_f.max() <= 1.5 * e_t.max() and e_f.mean() <= 1.5 * e_t.mean()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_two_calls_and_a_row_range_are_bit_equal(dtype):
    from nunchaku_amd.ops.attention import pulid_ca

    T, C, H, N = 257, 384, 16, 32
    r = _run(T, C, H, N, dtype)
    again, probs = pulid_ca(r["x"], r["fold"], stats=r["stats"], return_probs=True)
    assert torch.equal(again, r["out"]) and torch.equal(probs, r["probs"])
    a, b = 100, 203  # straddles the 64-row tiles at 128 and 192 and starts and ends inside one
    part, pp = pulid_ca(r["x"][a:b], r["fold"], stats=r["stats"][a:b].contiguous(), return_probs=True)
    assert torch.equal(part, r["out"][a:b]) and torch.equal(pp, r["probs"][a:b])
    # the statistics the op computes itself are the stats-only pass's
    assert torch.equal(pulid_ca(r["x"], r["fold"]), r["out"])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_rows_beyond_the_token_count_are_never_read(dtype):
    from nunchaku_amd.models.pulid import PulidFold
    from nunchaku_amd.ops.attention import pulid_ca

    T, C, H, N = 33, 256, 4, 5
    r = _run(T, C, H, N, dtype)
    f = r["fold"]
    a, b = f.a_fold.clone().view(H, 32, C), f.b_fold.clone().view(H, 32, C)
    a[:, N:], b[:, N:] = float("nan"), float("nan")
    colsum, cbias = f.colsum.clone().view(H, 32), f.cbias.clone().view(H, 32)
    colsum[:, N:], cbias[:, N:] = float("nan"), float("nan")
    dirty = PulidFold(a.view(H * 32, C), b.view(H * 32, C), colsum.view(-1), cbias.view(-1), N)
    out, probs = pulid_ca(r["x"], dirty, stats=r["stats"], return_probs=True)
    assert torch.isfinite(out).all() and torch.equal(out, r["out"]) and torch.equal(probs, r["probs"])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_a_dominant_key_takes_the_whole_probability(dtype):
    """One key per head ahead of the others by more than 40 in score -- by more than 100 here: exp(-40) = 4e-18 is an ordinary bf16
    number (the reference's ``softmax(weight.float()).type(dtype)`` keeps it too), so "exactly 0 elsewhere" needs the quotient below the
    format: the kernel's exponential is +0 below -80.  Head 0's lead comes through the data path (x . a - mean colsum), the others'
    through cbias."""
    from nunchaku_amd.models.pulid import PulidFold
    from nunchaku_amd.ops.attention import pulid_ca

    T, C, H, N = 70, 256, 4, 32
    td = TD[dtype]
    x = ref.stream_inputs(T, C, 4, td, "cuda")
    hot = (7 * 4 + 3) % C  # the outlier channel of stream_inputs
    g = torch.Generator().manual_seed(5)
    a = (torch.randn(H * 32, C, generator=g) * 0.01).to(td)
    star = [3, 32 + 31, 64 + 0, 96 + 17]
    a[star[0], hot] = 16.0
    cbias = torch.zeros(H * 32)
    for j in star[1:]:
        cbias[j] = 120.0
    b = torch.randn(H * 32, C, generator=g).to(td)
    fold = PulidFold(a.cuda(), b.cuda(), a.float().sum(-1).cuda(), cbias.cuda(), N)
    stats = ref.row_stats(x).cuda()
    s = stats[:, 1:2].double().cpu() * (x.double().cpu() @ a.double().T - stats[:, 0:1].double().cpu() * a.double().sum(-1)[None]) + cbias.double()[None]
    s = s.view(T, H, 32)
    lead = torch.stack([s[:, h, j % 32] - torch.cat([s[:, h, :j % 32], s[:, h, j % 32 + 1:]], dim=-1).max(-1).values for h, j in enumerate(star)], 1)
    assert lead.min() > 100, lead.min()
    out, probs = pulid_ca(x, fold, stats=stats, return_probs=True)
    want = torch.zeros(T, H * 32)
    want[:, star] = 1.0
    assert torch.equal(probs.float().cpu(), want)
    assert torch.equal(out.cpu(), b[star].float().sum(0).to(td).expand(T, C))  # four exact terms: the sum of the four value rows, rounded once


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_out_scale_zero_and_doubling(dtype):
    from nunchaku_amd.ops.attention import pulid_ca

    T, C, H, N = 33, 256, 4, 5
    r = _run(T, C, H, N, dtype)
    zero = pulid_ca(r["x"], r["fold"], out_scale=0.0, stats=r["stats"])
    assert (zero == 0).all()
    two = pulid_ca(r["x"], r["fold"], out_scale=2.0, stats=r["stats"])
    assert torch.isfinite(two).all() and torch.equal(two.float(), 2 * r["out"].float())  # exactly one doubling where nothing overflows


def test_unsupported_shapes_are_refused():
    from nunchaku_amd.models.pulid import PulidFold
    from nunchaku_amd.ops.attention import pulid_ca

    bf = torch.bfloat16
    z = lambda *s, dt=bf: torch.zeros(*s, dtype=dt, device="cuda")
    fold = lambda J, C, n=4: PulidFold(z(J, C), z(J, C), z(J, dt=torch.float32), z(J, dt=torch.float32), n)
    with pytest.raises(NotImplementedError, match="multiples of 128"):
        pulid_ca(z(8, 192), fold(128, 192))
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        pulid_ca(z(8, 128), fold(64, 128))
    with pytest.raises(NotImplementedError, match="at most 512"):
        pulid_ca(z(8, 128), fold(640, 128))
    with pytest.raises(NotImplementedError, match="at most 32"):
        pulid_ca(z(8, 128), fold(128, 128, 33))


# ---- the engine hook ----------------------------------------------------------------------------------------------------------------
def _count_pulid(fn):
    from nunchaku_amd._C import ops

    calls, orig = [], ops.pulid_ca

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    ops.pulid_ca = counted
    try:
        return fn(), len(calls)
    finally:
        del ops.pulid_ca  # (the instance attribute; the class's static method is uncovered again)


def test_engine_step_equals_the_step_composed_by_hand():
    """A FLUX-shaped model (dim 3072, 24 heads, random weights) of 2 joint + 5 single blocks -- the smallest on which modules 0, 1 and 2
    apply at joint block 0 and single blocks 0 and 4: three svdq_pulid_ca calls -- with 130 image and 37 text tokens, so both streams are
    padded.  In the deterministic mode: the default mode's low-rank sums use fp32 atomics, so two runs of one step differ in the last bits
    whatever this test does."""
    from nunchaku_amd import mode

    with torch.no_grad(), mode.deterministic_mode("strict"):
        _engine_step_equals_the_step_composed_by_hand()


def _engine_step_equals_the_step_composed_by_hand():
    from nunchaku_amd.models import pulid
    from nunchaku_amd.models.flux import FluxTransformerAMD
    from nunchaku_amd.ops.attention import pulid_ca
    from nunchaku_amd.ops.elementwise import residual_gate_stats
    from tests.flux_ref import synthetic_inputs

    model = FluxTransformerAMD(num_layers=2, num_single_layers=5, device="cuda").eval()
    model.init_synthetic_(seed=0)
    lat, enc, pooled, img_ids, txt_ids = synthetic_inputs((13, 10), 37, 4096, 768, seed=3)
    cuda = lambda t: t.cuda().bfloat16()[None]
    args = (cuda(lat), cuda(enc), pooled.cuda().bfloat16(), torch.tensor([0.6]).cuda(), img_ids.cuda(), txt_ids.cuda(), torch.tensor([3.5]).cuda())
    before = model.engine_forward(*args)
    pulid.attach_pulid(model, ref.module_state_dict(3, 3072, 16, 2048, seed=7, out_scale=2.0))
    assert len(model.pulid_ca) == 3 and model.pulid_fused
    assert torch.equal(model.engine_forward(*args), before)  # attached, no embeddings: no launch of the step changes
    emb = torch.randn(1, 32, 2048, generator=torch.Generator().manual_seed(9)).bfloat16().cuda()
    weight = 0.8

    checked = []

    def fresh_stats(name):
        def hook(mod, a, kw):
            hidden, stats = (a[0], a[4]) if name.startswith("joint") else (a[0], a[3])
            have = stats[0][0] if name.startswith("joint") else stats[0]
            assert torch.equal(have, residual_gate_stats(hidden.clone())[1]), name
            checked.append(name)
        return hook

    hooks = [model.blocks[1].register_forward_pre_hook(fresh_stats("joint 1"), with_kwargs=True),
             model.single_blocks[1].register_forward_pre_hook(fresh_stats("single 1"), with_kwargs=True)]
    try:
        got, calls = _count_pulid(lambda: model.engine_forward(*args, id_embeddings=emb, id_weight=weight))
    finally:
        for h in hooks:
            h.remove()
    assert calls == 3 and checked == ["joint 1", "single 1"]
    assert torch.isfinite(got).all() and not torch.equal(got, before)

    st = model._prologue(*args)
    nj, ns = len(model.blocks), len(model.single_blocks)
    model._launch_mods(st, range(nj), range(ns))
    for i in range(nj):
        st.enc, st.hidden, st.stats = model.blocks[i](st.hidden, st.enc, st.temb_act, st.rot, st.stats, mods=st.mods.get(("j", i)), kv_valid=st.kv_valid)
        if i % 2 == 0:
            o = pulid_ca(st.hidden, model.pulid_ca[i // 2].fold(emb), out_scale=weight)
            st.hidden, h_stats = residual_gate_stats(st.hidden, o)
            st.stats = ((h_stats, st.stats[0][1]), st.stats[1])
    assert st.hidden.shape[1] == 256 and st.enc.shape[1] == 256  # both streams padded
    model._join(st)
    for i in range(ns):
        st.hidden, st.stats = model.single_blocks[i](st.hidden, st.temb_act, st.rot[2], st.stats, mods=st.mods.get(("s", i)), kv_valid=st.kv_valid)
        if i % 4 == 0:
            img = st.hidden[:, st.p_txt:]
            o = pulid_ca(img, model.pulid_ca[1 + i // 4].fold(emb), out_scale=weight)
            _, i_stats = residual_gate_stats(img, o)
            st.stats[0][st.p_txt:] = i_stats
    by_hand = model._tail(st)
    assert torch.equal(got, by_hand)

    # the torch-op arm of the same step agrees (two 16-bit arithmetics of one computation), and detaching brings the plain step back
    model.pulid_fused = False
    try:
        torch_arm, calls_t = _count_pulid(lambda: model.engine_forward(*args, id_embeddings=emb, id_weight=weight))
    finally:
        del model.pulid_fused
    from tests.flux_ref import psnr_rel

    psnr = psnr_rel(got.float().cpu(), torch_arm.float().cpu())[0]
    print(f"engine: fused arm vs torch-op arm {psnr:.1f} dB; against the step without PuLID {psnr_rel(before.float().cpu(), torch_arm.float().cpu())[0]:.1f} dB")
    # leaving the computation out is further away than computing it in the other arithmetic
    assert calls_t == 0 and torch.isfinite(torch_arm).all() and psnr > psnr_rel(before.float().cpu(), torch_arm.float().cpu())[0] + 10.0
    pulid.detach_pulid(model)
    assert torch.equal(model.engine_forward(*args), before)
    with pytest.raises(ValueError, match="no PuLID modules"):
        model.engine_forward(*args, id_embeddings=emb)
