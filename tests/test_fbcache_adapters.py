"""First-Block Cache for Qwen-Image and SANA without a GPU: the import surface, the dispatcher, the Qwen-Image adapter (one wrap per class,
a fresh context per pipeline call, the branch of every transformer call, ``cfg_branches`` from the pipeline call's arguments) and the state
machine of ``SanaCachedTransformerBlocks`` on a stand-in stack in torch ops."""

import importlib
import logging

import pytest
import torch

from nunchaku.caching import fbcache

UTILS_NAMES = ("SanaCachedTransformerBlocks", "cache_context", "create_cache_context", "get_current_cache_context", "get_buffer", "set_buffer",
               "are_two_tensors_similar", "get_can_use_cache", "apply_prev_hidden_states_residual")


def test_import_surface():
    utils = importlib.import_module("nunchaku.caching.utils")
    for name in UTILS_NAMES:
        assert callable(getattr(utils, name)), name
    assert utils.cache_context is fbcache.cache_context and utils.get_buffer is fbcache.get_buffer  # one context, whichever path imports it
    for mod in ("nunchaku.caching.diffusers_adapters.sana", "nunchaku.caching.diffusers_adapters.qwenimage",
                "nunchaku_amd.caching.diffusers_adapters.sana", "nunchaku_amd.caching.diffusers_adapters.qwenimage"):
        m = importlib.import_module(mod)
        assert callable(m.apply_cache_on_transformer) and callable(m.apply_cache_on_pipe), mod


# ---- Qwen-Image ----------------------------------------------------------------------------------------------------------------------
class _QwenTransformer(torch.nn.Module):
    """records which forward ran, with which settings, in which context"""

    def __init__(self):
        super().__init__()
        self.calls = []

    def forward(self, hidden_states, encoder_hidden_states=None, **kwargs):
        self.calls.append(("original", None, fbcache.get_current_cache_context()))
        return hidden_states

    def forward_cached(self, hidden_states, encoder_hidden_states=None, *, residual_diff_threshold, first_blocks, branch, verbose, **kwargs):
        assert fbcache.get_current_cache_context() is not None
        self.calls.append(("cached", (residual_diff_threshold, first_blocks, branch, verbose), fbcache.get_current_cache_context()))
        return hidden_states


def _qwen_pipeline_class(name):
    def __init__(self):
        self.transformer = _QwenTransformer()

    def __call__(self, prompt=None, negative_prompt=None, true_cfg_scale=4.0, num_inference_steps=2, negative_prompt_embeds=None, **kwargs):
        """the two calls of a true-CFG step by diffusers' rule; (the stand-in's own restatement: the adapter must arrive at the same count)"""
        x = torch.zeros(1, 4, 8)
        cfg = true_cfg_scale > 1 and (negative_prompt is not None or negative_prompt_embeds is not None)
        for _ in range(num_inference_steps):
            self.transformer(x, x)
            if cfg:
                self.transformer(x, x[:, :2])
        return "image"

    return type(name, (), {"__init__": __init__, "__call__": __call__})


@pytest.mark.parametrize("cls_name", ["QwenImagePipeline", "QwenImageEditPlusPipeline"])
def test_dispatcher_takes_qwen_image_pipelines(cls_name):
    from nunchaku.caching.diffusers_adapters import apply_cache_on_pipe

    cls = _qwen_pipeline_class(cls_name)
    pipe = cls()
    assert apply_cache_on_pipe(pipe, residual_diff_threshold=0.2, first_blocks=8) is pipe and cls._is_cached
    t = pipe.transformer
    assert t._is_cached and (t.residual_diff_threshold, t.first_blocks) == (0.2, 8)
    assert pipe("a cat", num_inference_steps=1) == "image"
    assert [c[0] for c in t.calls] == ["cached"] and t.calls[0][1] == (0.2, 8, 0, False)


def test_qwen_apply_cache_on_transformer():
    from nunchaku.caching.diffusers_adapters.qwenimage import apply_cache_on_transformer

    t = _QwenTransformer()
    original = t.forward
    assert apply_cache_on_transformer(t) is t and t._is_cached and t._original_forward == original
    assert (t.residual_diff_threshold, t.first_blocks, t.cfg_branches) == (0.12, 1, 1)
    cached = t.forward
    assert cached != original
    apply_cache_on_transformer(t, residual_diff_threshold=0.3, first_blocks=2, cfg_branches=2)  # a second call only updates the settings
    assert t.forward == cached and t._original_forward == original
    assert (t.residual_diff_threshold, t.first_blocks, t.cfg_branches) == (0.3, 2, 2)
    x = torch.zeros(1, 4, 8)
    assert t(x, x) is x and t.calls[-1][0] == "original"  # outside a context: the original forward
    with fbcache.cache_context(fbcache.create_cache_context()):
        for _ in range(5):
            t(x, x)
    assert [c[1][2] for c in t.calls[1:]] == [0, 1, 0, 1, 0] and t.calls[1][1] == (0.3, 2, 0, False)
    with fbcache.cache_context(fbcache.create_cache_context()):  # the count belongs to the context: a new one starts at branch 0
        t(x, x)
    assert t.calls[-1][1][2] == 0
    apply_cache_on_transformer(t, cfg_branches=1)
    with fbcache.cache_context(fbcache.create_cache_context()):
        for _ in range(3):
            t(x, x)
    assert [c[1][2] for c in t.calls[-3:]] == [0, 0, 0]
    with pytest.raises(TypeError):
        apply_cache_on_transformer(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError):
        apply_cache_on_transformer(t, cfg_branches=0)


def test_qwen_apply_cache_on_pipe_contexts_and_branches():
    from nunchaku.caching.diffusers_adapters.qwenimage import apply_cache_on_pipe

    cls = _qwen_pipeline_class("QwenImagePipeline")
    pipe = cls()
    assert apply_cache_on_pipe(pipe) is pipe
    wrapped = cls.__call__
    apply_cache_on_pipe(pipe, residual_diff_threshold=0.15)  # the class is wrapped once; the settings follow
    assert cls.__call__ is wrapped and pipe.transformer.residual_diff_threshold == 0.15
    t = pipe.transformer

    def run(*args, **kwargs):
        del t.calls[:]
        assert pipe(*args, **kwargs) == "image" and fbcache.get_current_cache_context() is None
        assert all(c[0] == "cached" for c in t.calls) and len({id(c[2]) for c in t.calls}) == 1
        return [c[1][2] for c in t.calls], t.calls[0][2]

    # true_cfg_scale defaults to 4 in the signature: a negative prompt makes two calls per step, which alternate between two branches
    branches, ctx_a = run("a cat", negative_prompt=" ", num_inference_steps=3)
    assert branches == [0, 1, 0, 1, 0, 1] and t.cfg_branches == 2
    branches, ctx_b = run("a cat", num_inference_steps=3)  # no negative prompt: one call per step, one branch
    assert branches == [0, 0, 0] and t.cfg_branches == 1 and ctx_b is not ctx_a  # a fresh context per pipeline call
    assert run("a cat", " ", 1.0)[0] == [0, 0] and t.cfg_branches == 1  # positional; a scale of 1 switches true CFG off
    assert run("a cat", true_cfg_scale=2.5, negative_prompt_embeds=torch.zeros(1, 2, 8))[0] == [0, 1, 0, 1] and t.cfg_branches == 2
    assert run("a cat", true_cfg_scale=2.5, negative_prompt=None)[0] == [0, 0]
    # a given cfg_branches holds whatever the call's arguments say
    apply_cache_on_pipe(pipe, cfg_branches=2)
    assert run("a cat", num_inference_steps=4)[0] == [0, 1, 0, 1] and t.cfg_branches == 2
    apply_cache_on_pipe(pipe)  # and leaving it out hands the choice back to the call
    assert run("a cat", num_inference_steps=2)[0] == [0, 0]


def test_pipeline_cfg_branches_rule():
    from nunchaku_amd.caching.diffusers_adapters.qwenimage import pipeline_cfg_branches

    def call(self, prompt=None, negative_prompt=None, true_cfg_scale=4.0, negative_prompt_embeds=None):
        pass

    def loose(self, *args, **kwargs):
        pass

    assert pipeline_cfg_branches(call, (None, "p"), {}) == 1
    assert pipeline_cfg_branches(call, (None, "p", "n"), {}) == 2
    assert pipeline_cfg_branches(call, (None, "p", "n", 1.0), {}) == 1
    assert pipeline_cfg_branches(call, (None,), dict(negative_prompt_embeds=torch.zeros(1), true_cfg_scale=1.5)) == 2
    assert pipeline_cfg_branches(loose, (None,), dict(negative_prompt="n", true_cfg_scale=3.0)) == 2
    assert pipeline_cfg_branches(loose, (None,), dict(negative_prompt="n")) == 1  # no scale anywhere: no true CFG


# ---- SANA ----------------------------------------------------------------------------------------------------------------------------
class _Stack:
    """a stand-in for NunchakuSanaTransformerBlocks in torch ops: block i adds (i + 1) * 0.25 * tanh(x); records its calls"""

    layers = 3

    def __init__(self):
        self.calls = []

    @staticmethod
    def _layer(i, x):
        return x + (i + 1) * 0.25 * torch.tanh(x)

    def __call__(self, hidden_states, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None, timestep=None,
                 height=None, width=None, skip_first_layer=False):
        self.calls.append(("forward", bool(skip_first_layer), (height, width)))
        for i in range(1 if skip_first_layer else 0, self.layers):
            hidden_states = self._layer(i, hidden_states)
        return hidden_states

    def forward_layer_at(self, idx, hidden_states, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None,
                         timestep=None, height=None, width=None):
        self.calls.append(("layer", idx, (height, width)))
        return self._layer(idx, hidden_states)


class _SanaTransformer:
    def __init__(self):
        self.transformer_blocks = [_Stack()]

    def forward(self, hidden_states):
        """what diffusers' forward does with the list: every entry once, with the per-block argument list"""
        for block in self.transformer_blocks:
            hidden_states = block(hidden_states, None, hidden_states[:, :2], None, None, 2, 3)
        return hidden_states


def _x(batch, seed):
    return torch.randn(batch, 6, 8, generator=torch.Generator().manual_seed(seed))


def test_sana_cached_blocks_state_machine(caplog):
    from nunchaku.caching.utils import SanaCachedTransformerBlocks

    t = _SanaTransformer()
    stack = t.transformer_blocks[0]
    cached = SanaCachedTransformerBlocks(transformer=t, residual_diff_threshold=0.12, verbose=False)
    assert cached.transformer is t and cached.transformer_blocks[0] is stack
    args = lambda x: (x, None, x[:, :2], None, None, 2, 3)
    a, b = _x(2, 0), _x(2, 1)
    full = lambda x: _Stack()(x)

    # threshold 0 and batch 3 take the uncached path -- no context needed, nothing stored, one notice for the batch through logging
    cached.residual_diff_threshold = 0.0
    assert torch.equal(cached(*args(a)), full(a)) and stack.calls == [("forward", False, (2, 3))]
    cached.residual_diff_threshold = 0.12
    del stack.calls[:]
    with caplog.at_level(logging.INFO, logger="nunchaku_amd.caching.utils"):
        with fbcache.cache_context(fbcache.create_cache_context()) as _:
            ctx = fbcache.get_current_cache_context()
            x3 = _x(3, 2)
            assert torch.equal(cached(*args(x3)), full(x3)) and torch.equal(cached(*args(x3)), full(x3))
            assert stack.calls == [("forward", False, (2, 3))] * 2 and not ctx.buffers
    assert sum("batch 3" in r.getMessage() for r in caplog.records) == 1
    with pytest.raises(AssertionError, match="cache_context must be set before"):
        cached(*args(a))

    del stack.calls[:]
    with fbcache.cache_context(fbcache.create_cache_context()):
        ctx = fbcache.get_current_cache_context()
        # step 1: nothing stored, a miss -- block 0, then the others; equal to the stack
        assert torch.equal(cached(*args(a)), full(a))
        assert stack.calls == [("layer", 0, (2, 3)), ("forward", True, (2, 3))]
        assert sorted(ctx.buffers) == ["first_multi_hidden_states_residual", "multi_hidden_states_residual"]
        after = _Stack._layer(0, a)
        first, rest = ctx.get_buffer("first_multi_hidden_states_residual"), ctx.get_buffer("multi_hidden_states_residual")
        assert first.shape == a.shape and torch.equal(first, after - a) and torch.equal(rest, full(a) - after)  # all B * T rows: one problem
        # step 2: the same input, ratio 0 -- a hit: block 0 only, plus the stored residual; the stored first residual stays
        del stack.calls[:]
        assert torch.equal(cached(*args(a)), after + rest) and stack.calls == [("layer", 0, (2, 3))]
        assert ctx.get_buffer("first_multi_hidden_states_residual") is first
        # step 3: another input -- a miss that replaces both buffers
        ratio = ((first - (_Stack._layer(0, b) - b)).abs().mean() / first.abs().mean()).item()
        assert ratio > 2 * 0.12, f"mis-constructed: ratio {ratio}"
        del stack.calls[:]
        assert torch.equal(cached(*args(b)), full(b)) and stack.calls == [("layer", 0, (2, 3)), ("forward", True, (2, 3))]
        assert ctx.get_buffer("first_multi_hidden_states_residual") is not first
        assert torch.equal(ctx.get_buffer("multi_hidden_states_residual"), full(b) - _Stack._layer(0, b))
        # a slightly moved input is a hit against step 3's residual, not step 1's
        near = b + 1e-3 * _x(2, 3)
        del stack.calls[:]
        out = cached(*args(near))
        assert stack.calls == [("layer", 0, (2, 3))] and torch.equal(out, _Stack._layer(0, near) + ctx.get_buffer("multi_hidden_states_residual"))
        # another batch size: the stored buffers have another shape -- a miss, not an error
        one = _x(1, 4)
        del stack.calls[:]
        assert torch.equal(cached(*args(one)), full(one)) and len(stack.calls) == 2
        assert ctx.get_buffer("first_multi_hidden_states_residual").shape == one.shape


def test_sana_adapter_swaps_the_blocks_inside_a_context_only():
    from nunchaku.caching.diffusers_adapters.sana import apply_cache_on_pipe, apply_cache_on_transformer
    from nunchaku.caching.utils import SanaCachedTransformerBlocks

    t = _SanaTransformer()
    blocks, stack = t.transformer_blocks, t.transformer_blocks[0]
    assert apply_cache_on_transformer(t, residual_diff_threshold=0.2) is t and t._is_cached
    wrapped = t.forward
    apply_cache_on_transformer(t, residual_diff_threshold=0.12)  # once; the threshold follows
    assert t.forward == wrapped and t.transformer_blocks is blocks
    a = _x(2, 0)
    assert torch.equal(t.forward(a), _Stack()(a)) and stack.calls == [("forward", False, (2, 3))]  # outside a context: the original stack
    del stack.calls[:]
    seen = []
    original_layer_at = stack.forward_layer_at
    stack.forward_layer_at = lambda *args, **kw: (seen.append(t.transformer_blocks), original_layer_at(*args, **kw))[1]
    with fbcache.cache_context(fbcache.create_cache_context()):
        assert torch.equal(t.forward(a), _Stack()(a))
        assert [c[0] for c in stack.calls] == ["layer", "forward"]
        assert len(seen[0]) == 1 and isinstance(seen[0][0], SanaCachedTransformerBlocks) and seen[0][0].residual_diff_threshold == 0.12
        assert t.transformer_blocks is blocks  # back in place behind the forward
        del stack.calls[:]
        t.forward(a)
        assert [c[0] for c in stack.calls] == ["layer"]
        stack.forward_layer_at = lambda *args, **kw: (_ for _ in ()).throw(RuntimeError("boom"))
        with pytest.raises(RuntimeError, match="boom"):
            t.forward(a)
        assert t.transformer_blocks is blocks  # and behind a forward that raised

    class SanaPipelineStandIn:
        def __init__(self):
            self.transformer = _SanaTransformer()

        def __call__(self, x, steps):
            for _ in range(steps):
                out = self.transformer.forward(x)
            return out

    pipe = SanaPipelineStandIn()
    assert apply_cache_on_pipe(pipe, residual_diff_threshold=0.12) is pipe and SanaPipelineStandIn._is_cached
    call = SanaPipelineStandIn.__call__
    apply_cache_on_pipe(pipe)
    assert SanaPipelineStandIn.__call__ is call
    calls = pipe.transformer.transformer_blocks[0].calls
    pipe(a, 3)
    assert [c[0] for c in calls] == ["layer", "forward", "layer", "layer"]  # a miss, then two skipped steps
    del calls[:]
    pipe(a, 1)
    assert [c[0] for c in calls] == ["layer", "forward"] and fbcache.get_current_cache_context() is None  # a fresh context per call
