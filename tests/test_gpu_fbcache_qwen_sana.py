"""First-Block Cache for Qwen-Image and SANA on the GPU: three steps on one context (a miss that stores, a hit with ratio 0, a miss that
replaces), the decision's ratio against its CPU restatement, inert padding rows, CFG branches, SANA's batch fall-through, refusals.

Shapes: the smallest at which this can go wrong.  Qwen-Image: 4 blocks of 24 heads x 128, 300 image tokens and 40 (9) text tokens --
neither a multiple of 256, both streams padded.  SANA: the 0.6B block shape (36 heads x 32, 16 cross-attention heads), 3 blocks, a 16 x 16
grid, 300 text tokens with key counts (300, 37).  Bit equality is asserted in deterministic mode, as tests/test_gpu_fbcache.py does."""

from types import SimpleNamespace

import pytest
import torch

from tests.test_gpu_fbcache import DTYPES, _launch_counts

pytestmark = pytest.mark.gpu

THR = 0.12
LAYERS, T_IMG, GRID = 4, 300, (1, 15, 20)
FIRST, REST = "first_multi_hidden_states_residual", "multi_hidden_states_residual"


@pytest.fixture(autouse=True)
def _need_gpu(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


@pytest.fixture
def decisions(monkeypatch):
    """every decision taken while the test runs: (hit, ratio) as Python values, from the record the decision itself read"""
    from nunchaku_amd.caching import fbcache

    seen = []
    real = fbcache.are_two_tensors_similar

    def spy(*args, **kwargs):
        hit, ratio = real(*args, **kwargs)
        seen.append((bool(hit), float(ratio)))
        return hit, ratio

    monkeypatch.setattr(fbcache, "are_two_tensors_similar", spy)
    return seen


def restated_ratio(t1: torch.Tensor, t2: torch.Tensor) -> float:
    """the reference's formula on the CPU with its 16-bit rounding points (caching/fbcache.py:275-277)"""
    t1, t2 = t1.cpu(), t2.cpu()
    return ((t1 - t2).abs().mean() / t1.abs().mean()).item()


def ratio_bound(ratio: float, dt) -> float:
    """what tests/test_gpu_fbcache.py allows between the kernel's ratio and torch's: two means and a quotient, three 16-bit roundings of
    half a unit each (the fp32 sums run in another order) -- within four whole units"""
    return 4 * ratio * (2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11)


# ---- Qwen-Image ----------------------------------------------------------------------------------------------------------------------
_QWEN = {}


def _qwen(name):
    """one model per dtype, built once and left unchanged"""
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    if name not in _QWEN:
        _QWEN[name] = NunchakuQwenImageTransformer2DModel(
            num_layers=LAYERS, num_attention_heads=24, attention_head_dim=128, in_channels=64, out_channels=16, joint_attention_dim=128,
            torch_dtype=DTYPES[name], device="cuda").init_synthetic_(seed=3).eval()
    return _QWEN[name]


def _qwen_inputs(dt, seed, t_txt=40, timestep=0.6):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lat = torch.randn(1, T_IMG, 64, device="cuda", generator=g).to(dt)
    enc = torch.randn(1, t_txt, 128, device="cuda", generator=g).to(dt)
    return [lat, enc, None, torch.tensor([timestep], device="cuda"), [GRID]]


def _qwen_other_inputs(dt):
    """the inputs of a step that must be a miss: another seed AND another point of the schedule.  (Another seed alone gave a restated ratio
    of 0.155 on these synthetic weights -- LayerNorm in front of every projection makes the first block's residual follow its modulation,
    that is the timestep, much more than its input -- and 0.155 is not clear of the threshold.)"""
    return _qwen_inputs(dt, seed=6, timestep=0.15)


def _qwen_restated_hit(model, inputs, residual, first_blocks):
    """a hit step restated: the first blocks' image rows + the stored residual (torch's 16-bit add), the tail"""
    st = model._prologue(*inputs)
    model._launch_mods(st, 0, first_blocks)
    model._run_blocks(st, 0, first_blocks)
    st.hidden = torch.cat([st.hidden[:, :T_IMG] + residual, st.hidden[:, T_IMG:]], dim=1)
    return model._tail(st)


@pytest.fixture
def gemv_launches(monkeypatch):
    """the modulation GEMV launches of the Qwen-Image engine: projections per batched launch; a block that runs its own appends -1"""
    from nunchaku_amd.models import qwenimage

    seen = []
    batched, single = qwenimage.awq_gemv_w4a16_batched, qwenimage.awq_gemv_w4a16_cuda
    monkeypatch.setattr(qwenimage, "awq_gemv_w4a16_batched", lambda x, lins: (seen.append(len(lins)), batched(x, lins))[1])
    monkeypatch.setattr(qwenimage, "awq_gemv_w4a16_cuda", lambda *a, **k: (seen.append(-1), single(*a, **k))[1])
    return seen


@pytest.mark.parametrize("first_blocks", [1, 2])
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_qwen_three_steps(name, first_blocks, decisions, gemv_launches):
    from nunchaku.caching import fbcache
    from nunchaku_amd import mode

    dt, fb = DTYPES[name], first_blocks
    kw = dict(residual_diff_threshold=THR, first_blocks=fb)
    with torch.no_grad(), mode.deterministic_mode("strict"):
        model = _qwen(name)
        a, b = _qwen_inputs(dt, seed=5), _qwen_other_inputs(dt)
        ref_a, n_full = _launch_counts(lambda: model(*a).sample)
        ref_b = model(*b).sample
        assert gemv_launches == [2 * LAYERS] * 2
        # a non-positive threshold is the plain forward: no context needed
        assert torch.equal(model.forward_cached(*a, residual_diff_threshold=0.0, first_blocks=fb).sample, ref_a)
        assert torch.equal(model.forward_cached(*a, residual_diff_threshold=-1.0, first_blocks=fb, return_dict=False)[0], ref_a)
        ctx = fbcache.create_cache_context()
        with fbcache.cache_context(ctx):
            # step 1: nothing stored -- a miss that stores, equal to the plain forward; the other blocks' projections in a launch of their own
            del gemv_launches[:]
            assert torch.equal(model.forward_cached(*a, **kw).sample, ref_a)
            assert gemv_launches == [2 * fb, 2 * (LAYERS - fb)] and not decisions
            assert sorted(ctx.buffers) == [FIRST + "_0", REST + "_0"]
            first, rest = ctx.get_buffer(FIRST + "_0"), ctx.get_buffer(REST + "_0")
            assert first.shape == rest.shape == (1, T_IMG, 3072) and first.dtype == rest.dtype == dt  # the real image rows only
            first_bits, rest_bits = first.clone(), rest.clone()
            # step 2: identical inputs -- ratio exactly 0, a hit
            del gemv_launches[:]
            hit_out, n_hit = _launch_counts(lambda: model.forward_cached(*a, **kw).sample)
            assert decisions == [(True, 0.0)]
            assert gemv_launches == [2 * fb], "a hit launches the first blocks' modulation projections only"
            assert ctx.get_buffer(FIRST + "_0") is first and torch.equal(first, first_bits)  # a hit leaves the stored first residual alone
            assert ctx.get_buffer(REST + "_0") is rest and torch.equal(rest, rest_bits)
            assert torch.isfinite(hit_out.float()).all()
            # what the prologue, the first blocks and the tail launch, and nothing else
            want, n_want = _launch_counts(lambda: _qwen_restated_hit(model, a, rest, fb))
            assert torch.equal(hit_out, want)
            print(f"{name} first_blocks={fb}: launches hit {n_hit} first blocks alone {n_want} full step {n_full}")
            assert n_hit == n_want
            for k in ("gemm", "quantize", "attention"):
                assert 0 < n_hit[k] < n_full[k], k
            # step 3: inputs from another seed, at another timestep -- a miss, equal to the plain forward, both buffers replaced
            del gemv_launches[:], decisions[:]
            out_b = model.forward_cached(*b, **kw).sample
            new_first, new_rest = ctx.get_buffer(FIRST + "_0"), ctx.get_buffer(REST + "_0")
            assert new_first is not first and new_rest is not rest and torch.equal(first, first_bits)
            want_ratio = restated_ratio(first, new_first)
            print(f"{name} first_blocks={fb}: step 3 ratio: decision {decisions} CPU restatement {want_ratio}")
            assert want_ratio > 2 * THR, f"mis-constructed: the restated ratio {want_ratio} of step 3 is not above 2 x threshold"
            assert len(decisions) == 1 and decisions[0][0] is False
            assert abs(decisions[0][1] - want_ratio) <= ratio_bound(want_ratio, dt)
            assert gemv_launches == [2 * fb, 2 * (LAYERS - fb)]
            assert torch.equal(out_b, ref_b)
            assert sorted(ctx.buffers) == [FIRST + "_0", REST + "_0"]


def test_qwen_padding_rows_are_inert(decisions, monkeypatch):
    """The image stream has 212 padding rows behind its 300 real ones.  A hook poisons them with NaN right behind the first block: neither a
    zero nor a non-zero ratio moves, and the hit's output (the tail reads the real rows) stays bit for bit."""
    from nunchaku.caching import fbcache
    from nunchaku_amd import mode

    dt = torch.bfloat16
    with torch.no_grad(), mode.deterministic_mode("strict"):
        model = _qwen("bf16")
        a, b = _qwen_inputs(dt, seed=5), _qwen_other_inputs(dt)
        run = type(model)._run_blocks
        poisoned = []

        def run_and_poison(st, lo, hi, keep_input=False):
            run(model, st, lo, hi, keep_input)
            assert lo == 0 and st.hidden.shape[1] == 512
            st.hidden[:, T_IMG:] = float("nan")
            poisoned.append(hi)

        with fbcache.cache_context(fbcache.create_cache_context()):
            model.forward_cached(*a, residual_diff_threshold=THR)  # stores
            # every later step is a hit (the comparison still runs): the same inputs give ratio 0, others a ratio well above 0
            clean = [model.forward_cached(*x, residual_diff_threshold=1e9).sample for x in (a, b)]
            monkeypatch.setattr(model, "_run_blocks", run_and_poison, raising=False)
            dirty = [model.forward_cached(*x, residual_diff_threshold=1e9).sample for x in (a, b)]
            monkeypatch.undo()
        assert poisoned == [1, 1]
        assert len(decisions) == 4 and all(d[0] for d in decisions)
        print(f"padding rows poisoned: ratios clean {decisions[:2]} poisoned {decisions[2:]}")
        assert decisions[0][1] == 0.0 and decisions[1][1] > 2 * THR
        assert decisions[2:] == decisions[:2], "the padding rows took part in the decision"
        assert all(torch.equal(c, d) for c, d in zip(clean, dirty))


def test_qwen_branches(decisions):
    """A true-CFG step: the conditional call (40 text tokens, branch 0) and the unconditional one (9, branch 1) keep a set of buffers each.
    The stored residuals hold image rows only, so the two branches' buffers have the SAME shape: only the branch index keeps a call from
    being compared with the other call's residual."""
    from nunchaku.caching import fbcache
    from nunchaku_amd import mode

    dt = torch.bfloat16
    with torch.no_grad(), mode.deterministic_mode("strict"):
        model = _qwen("bf16")
        cond, uncond = _qwen_inputs(dt, seed=5, t_txt=40), _qwen_inputs(dt, seed=5, t_txt=9)
        ref = [model(*x).sample for x in (cond, uncond)]
        assert not torch.equal(ref[0], ref[1])
        ctx = fbcache.create_cache_context()
        with fbcache.cache_context(ctx):
            for br, x in enumerate((cond, uncond)):
                assert torch.equal(model.forward_cached(*x, residual_diff_threshold=THR, branch=br).sample, ref[br])
            assert sorted(ctx.buffers) == [FIRST + "_0", FIRST + "_1", REST + "_0", REST + "_1"] and not decisions
            firsts = [ctx.get_buffer(f"{FIRST}_{br}") for br in (0, 1)]
            rests = [ctx.get_buffer(f"{REST}_{br}") for br in (0, 1)]
            assert firsts[0].shape == firsts[1].shape == (1, T_IMG, 3072)
            cross = restated_ratio(firsts[0], firsts[1])
            assert cross > 0.0, "mis-constructed: the two branches' first residuals do not differ"
            # the same step again, then once more in the swapped order: every call meets its own branch's residual -- ratio exactly 0
            for order in ((0, 1), (1, 0)):
                del decisions[:]
                for br in order:
                    out = model.forward_cached(*(cond, uncond)[br], residual_diff_threshold=THR, branch=br).sample
                    assert torch.equal(out, _qwen_restated_hit(model, (cond, uncond)[br], rests[br], 1)), (order, br)
                assert decisions == [(True, 0.0)] * 2, (order, decisions)
            assert all(ctx.get_buffer(f"{FIRST}_{br}") is firsts[br] and ctx.get_buffer(f"{REST}_{br}") is rests[br] for br in (0, 1))
            # (what a mixed-up branch would have compared: a non-zero ratio, with no shape to stop it)
            del decisions[:]
            model.forward_cached(*uncond, residual_diff_threshold=1e-9, branch=0)
            assert decisions[0][1] > 0.0 and abs(decisions[0][1] - cross) <= ratio_bound(cross, dt)


def test_qwen_adapter_on_the_model(decisions):
    """``apply_cache_on_transformer`` on the real model: call k of a context uses branch k % 2; outside a context the plain forward runs"""
    from nunchaku.caching import fbcache
    from nunchaku.caching.diffusers_adapters.qwenimage import apply_cache_on_transformer
    from nunchaku_amd import mode
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    dt = torch.bfloat16
    with torch.no_grad(), mode.deterministic_mode("strict"):
        model = NunchakuQwenImageTransformer2DModel(num_layers=2, num_attention_heads=2, attention_head_dim=128, in_channels=64, out_channels=16,
                                                    joint_attention_dim=128, device="cuda").init_synthetic_(seed=5).eval()
        cond, uncond = _qwen_inputs(dt, seed=5, t_txt=40), _qwen_inputs(dt, seed=5, t_txt=9)
        ref = [model(*x).sample for x in (cond, uncond)]
        apply_cache_on_transformer(model, residual_diff_threshold=THR, cfg_branches=2)
        assert torch.equal(model(*cond).sample, ref[0])  # no context
        ctx = fbcache.create_cache_context()
        with fbcache.cache_context(ctx):
            for _ in range(2):
                for x, r in zip((cond, uncond), ref):
                    out = model(*x)
            assert sorted(ctx.buffers) == [FIRST + "_0", FIRST + "_1", REST + "_0", REST + "_1"]
            assert decisions == [(True, 0.0)] * 2 and torch.isfinite(out.sample.float()).all()


def test_qwen_refusals(monkeypatch):
    from nunchaku.caching import fbcache
    from nunchaku_amd.graph import CapturedStep
    from nunchaku_amd.models.qwenimage import NunchakuQwenImageTransformer2DModel

    dt = torch.bfloat16

    def small(heads, head_dim):
        return NunchakuQwenImageTransformer2DModel(num_layers=2, num_attention_heads=heads, attention_head_dim=head_dim, in_channels=64,
                                                   out_channels=16, joint_attention_dim=128, device="cuda").init_synthetic_(seed=5).eval()

    with torch.no_grad():
        model = small(2, 128)
        x = _qwen_inputs(dt, seed=5)
        launched = []
        prologue = model._prologue
        monkeypatch.setattr(model, "_prologue", lambda *a, **k: (launched.append(1), prologue(*a, **k))[1], raising=False)
        with pytest.raises(RuntimeError, match="cache_context must be set before"):
            model.forward_cached(*x)
        with fbcache.cache_context(fbcache.create_cache_context()):
            two = [torch.cat([x[0], x[0]]), torch.cat([x[1], x[1]]), None, torch.cat([x[3], x[3]]), x[4]]
            with pytest.raises(ValueError, match="batch 1"):
                model.forward_cached(*two)
            cn = [torch.zeros(1, T_IMG, 256, device="cuda", dtype=dt)]
            with pytest.raises(ValueError, match="ControlNet"):
                model.forward_cached(*x, controlnet_block_samples=cn)
            for bad in (0, 2, 3):
                with pytest.raises(ValueError, match="first_blocks"):
                    model.forward_cached(*x, first_blocks=bad)
            with pytest.raises(NotImplementedError, match="fused path"):
                model.forward_cached(*x, attention_kwargs={"scale": 1.0})
            other = small(4, 64)
            monkeypatch.setattr(other, "_prologue", lambda *a, **k: launched.append(1), raising=False)
            with pytest.raises(NotImplementedError, match="fused path"):
                other.forward_cached(*x)
            monkeypatch.setattr(model, "fused_norm", False, raising=False)
            with pytest.raises(NotImplementedError, match="fused path"):
                model.forward_cached(*x)
            monkeypatch.setattr(model, "fused_norm", True, raising=False)
            monkeypatch.setattr(model, "offload", True, raising=False)  # (the flag alone: the refusal comes before the manager is touched)
            with pytest.raises(NotImplementedError, match="offloaded"):
                model.forward_cached(*x)
            monkeypatch.setattr(model, "offload", False, raising=False)
            assert not launched, "a refusal must come before anything is launched"
            with pytest.raises(RuntimeError, match="captured"):
                CapturedStep(lambda *inp: model.forward_cached(*inp).sample, x)
            torch.cuda.synchronize()
            assert torch.isfinite(model.forward_cached(*x).sample.float()).all()  # and the model still runs afterwards


# ---- SANA ----------------------------------------------------------------------------------------------------------------------------
SANA_CFG = dict(num_layers=3, num_attention_heads=36, attention_head_dim=32, num_cross_attention_heads=16, mlp_ratio=2.5)  # SANA-0.6B's block
SANA_DIM, SANA_GRID, SANA_L, SANA_COUNTS = 1152, (16, 16), 300, (300, 37, 120)
_SANA = {}


def _sana():
    """(stack wrapper, stand-in transformer that holds it), built once and left unchanged"""
    from tests.test_gpu_sana_block import _random_state_dict

    from nunchaku_amd.models import SanaModel
    from nunchaku_amd.models.transformer_sana import NunchakuSanaTransformerBlocks

    if not _SANA:
        m = SanaModel(SANA_CFG, pag_layers=[], device="cuda")
        m.load_state_dict(_random_state_dict(m, seed=7), strict=True)
        stack = NunchakuSanaTransformerBlocks(m, torch.bfloat16, "cuda")
        _SANA["stack"] = stack
        _SANA["transformer"] = SimpleNamespace(transformer_blocks=torch.nn.ModuleList([stack]))
    return _SANA["stack"], _SANA["transformer"]


def _sana_inputs(B, seed):
    """-> (hidden [B, 256, 1152], the other arguments of a diffusers SANA block call)"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    T = SANA_GRID[0] * SANA_GRID[1]
    x = torch.randn(B, T, SANA_DIM, device="cuda", generator=g).bfloat16()
    cond = torch.randn(B, SANA_L, SANA_DIM, device="cuda", generator=g).bfloat16()
    ts = (0.5 * torch.randn(B, 6 * SANA_DIM, device="cuda", generator=g)).bfloat16()
    mask = torch.full((B, 1, SANA_L), -10000.0, device="cuda", dtype=torch.bfloat16)
    for i in range(B):
        mask[i, 0, : SANA_COUNTS[i]] = 0
    return x, (None, cond, mask, ts, *SANA_GRID)


def _stack_kw(rest):
    return dict(attention_mask=rest[0], encoder_hidden_states=rest[1], encoder_attention_mask=rest[2], timestep=rest[3], height=rest[4], width=rest[5])


def test_sana_three_steps(decisions, monkeypatch):
    from nunchaku.caching import fbcache
    from nunchaku.caching.utils import SanaCachedTransformerBlocks
    from nunchaku_amd import mode
    from nunchaku_amd.models import sana as sana_mod

    dt = torch.bfloat16
    with torch.no_grad(), mode.deterministic_mode("strict"):
        stack, transformer = _sana()
        cached = SanaCachedTransformerBlocks(transformer=transformer, residual_diff_threshold=THR, verbose=False)
        glue = []
        real = sana_mod.sana_glue
        monkeypatch.setattr(sana_mod, "sana_glue", lambda *a, **k: (glue.append(1), real(*a, **k))[1])
        (xa, rest_a), (xb, rest_b) = _sana_inputs(2, seed=11), _sana_inputs(2, seed=12)
        ref_a, n_full = _launch_counts(lambda: stack(xa, **_stack_kw(rest_a)))
        ref_b = stack(xb, **_stack_kw(rest_b))
        assert len(glue) == 2 * (3 * 3 + 1) and torch.isfinite(ref_a.float()).all() and ref_a.float().abs().max() > 0.01
        # a non-positive threshold: the uncached stack, no context needed
        cached.residual_diff_threshold = 0.0
        assert torch.equal(cached(xa, *rest_a), ref_a)
        cached.residual_diff_threshold = THR
        ctx = fbcache.create_cache_context()
        with fbcache.cache_context(ctx):
            # step 1: a miss that stores -- block 0 alone (4 glue launches), the other two (3 * 2 + 1)
            del glue[:]
            assert torch.equal(cached(xa, *rest_a), ref_a)
            assert len(glue) == 4 + 3 * 2 + 1 and not decisions
            assert sorted(ctx.buffers) == [FIRST, REST]
            first, rest = ctx.get_buffer(FIRST), ctx.get_buffer(REST)
            assert first.shape == rest.shape == xa.shape and first.dtype == rest.dtype == dt and first.is_cuda  # all B * T rows: one problem
            first_bits = first.clone()
            # step 2: identical inputs -- ratio exactly 0, a hit: block 0 and one add
            del glue[:]
            hit_out, n_hit = _launch_counts(lambda: cached(xa, *rest_a))
            assert decisions == [(True, 0.0)] and len(glue) == 4
            after, n_layer = _launch_counts(lambda: stack.forward_layer_at(0, xa, **_stack_kw(rest_a)))
            print(f"sana: launches hit {n_hit} block 0 alone {n_layer} full stack {n_full}")
            assert torch.equal(hit_out, after + rest)
            assert n_hit == n_layer and 0 < n_hit["gemm"] < n_full["gemm"]
            assert all(n_hit[k] <= n_full[k] for k in n_full)
            assert ctx.get_buffer(FIRST) is first and ctx.get_buffer(REST) is rest and torch.equal(first, first_bits)
            # step 3: inputs from another seed -- a miss, equal to the stack, both buffers replaced
            del glue[:], decisions[:]
            out_b = cached(xb, *rest_b)
            new_first = ctx.get_buffer(FIRST)
            assert new_first is not first and ctx.get_buffer(REST) is not rest
            want_ratio = restated_ratio(first, new_first)
            print(f"sana: step 3 ratio: decision {decisions} CPU restatement {want_ratio}")
            assert want_ratio > 2 * THR, f"mis-constructed: the restated ratio {want_ratio} of step 3 is not above 2 x threshold"
            assert len(decisions) == 1 and decisions[0][0] is False
            assert abs(decisions[0][1] - want_ratio) <= ratio_bound(want_ratio, dt)
            assert torch.equal(out_b, ref_b) and len(glue) == 4 + 3 * 2 + 1
            assert torch.equal(new_first, stack.forward_layer_at(0, xb, **_stack_kw(rest_b)) - xb)


def test_sana_batches_and_wrapper_dtype(decisions):
    """B = 1 and B = 2 are cached, B = 3 (what PAG produces) runs the uncached stack and stores nothing; an fp32 stream from the pipeline
    comes back fp32 while the residuals stay 16-bit on the device; the adapter swaps the wrapper in for a forward inside a context."""
    from nunchaku.caching import fbcache
    from nunchaku.caching.diffusers_adapters.sana import apply_cache_on_transformer
    from nunchaku.caching.utils import SanaCachedTransformerBlocks
    from nunchaku_amd import mode

    with torch.no_grad(), mode.deterministic_mode("strict"):
        stack, transformer = _sana()
        cached = SanaCachedTransformerBlocks(transformer=transformer, residual_diff_threshold=THR)
        for B in (1, 2, 3):
            x, rest = _sana_inputs(B, seed=20 + B)
            ref = stack(x, **_stack_kw(rest))
            del decisions[:]
            ctx = fbcache.create_cache_context()
            with fbcache.cache_context(ctx):
                assert torch.equal(cached(x, *rest), ref)
                again = cached(x, *rest)
            if B == 3:
                assert not ctx.buffers and not decisions and torch.equal(again, ref)
            else:
                assert decisions == [(True, 0.0)] and ctx.get_buffer(FIRST).shape == x.shape
                assert torch.equal(again, stack.forward_layer_at(0, x, **_stack_kw(rest)) + ctx.get_buffer(REST))
        x, rest = _sana_inputs(2, seed=30)
        ctx = fbcache.create_cache_context()
        with fbcache.cache_context(ctx):
            out = cached(x.float(), *rest)
        assert out.dtype == torch.float32 and torch.equal(out, stack(x, **_stack_kw(rest)).float())
        assert ctx.get_buffer(FIRST).dtype == torch.bfloat16 and ctx.get_buffer(FIRST).is_cuda
        # the adapter: a stand-in for diffusers' forward, which calls every entry of transformer_blocks once
        model = SimpleNamespace(transformer_blocks=transformer.transformer_blocks)

        def walk(h, *r):
            for blk in model.transformer_blocks:
                h = blk(h, *r)
            return h

        model.forward = walk
        apply_cache_on_transformer(model, residual_diff_threshold=THR)
        ref = stack(x, **_stack_kw(rest))
        del decisions[:]
        assert torch.equal(model.forward(x, *rest), ref) and not decisions  # outside a context: the stack itself
        with fbcache.cache_context(fbcache.create_cache_context()):
            assert torch.equal(model.forward(x, *rest), ref)
            model.forward(x, *rest)
        assert decisions == [(True, 0.0)] and model.transformer_blocks is transformer.transformer_blocks
