"""First-Block Cache without a GPU: the state machine and the names against a fixture recorded from the reference's own functions
(tools/make_fbcache_golden.py), the adapters on stand-in classes, and the C ABI of svdq_residual_diff (layout, export, validation)."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from nunchaku.caching import fbcache
from nunchaku.caching.diffusers_adapters import apply_cache_on_pipe
from nunchaku.caching.diffusers_adapters.flux_v2 import apply_cache_on_transformer
from nunchaku_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
BUFFERS = ("first_multi_hidden_states_residual", "multi_hidden_states_residual", "multi_encoder_hidden_states_residual",
           "first_single_hidden_states_residual", "single_hidden_states_residual")


def from_bits(a: np.ndarray, dt: torch.dtype) -> torch.Tensor:
    return torch.from_numpy(a.view(np.int16).copy()).view(dt)


def bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# the toy "other blocks" of the recorded trace (tools/make_fbcache_golden.py)
def remaining_multi(hidden_states, encoder_hidden_states):
    uh, ue = hidden_states * 1.25 + 0.5, encoder_hidden_states * 0.75 - 0.25
    return uh, ue, uh - hidden_states, ue - encoder_hidden_states


def remaining_single(hidden_states, encoder_hidden_states):
    uc = hidden_states * 1.5 + 0.125
    return uc, uc - hidden_states


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_similarity_matches_the_reference_fixture(golden_dir, name):
    g, dt = np.load(os.path.join(golden_dir, f"fbcache_{name}.npz")), DTYPES[name]
    thr = float(g["threshold"])
    prev = from_bits(g["sim_prev"], dt)
    answers = []
    for i in range(len(g["amplitudes"])):
        similar, ratio = fbcache.are_two_tensors_similar(prev, from_bits(g[f"sim_cur_{i}"], dt), threshold=thr)
        assert ratio.dtype == dt and np.array_equal(bits(ratio.reshape(1)), g[f"sim_ratio_{i}"]), f"amplitude {g['amplitudes'][i]}"
        assert bool(similar) == bool(g[f"sim_similar_{i}"])
        r = float(ratio)
        assert not (0.5 * thr <= r <= 2 * thr), "the fixture must keep clear of the threshold"
        answers.append(bool(similar))
    assert any(answers) and not all(answers)


@pytest.mark.parametrize("mode", ["multi", "single"])
@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_check_and_apply_cache_reproduces_the_reference_trace(golden_dir, name, mode):
    g, dt = np.load(os.path.join(golden_dir, f"fbcache_{name}.npz")), DTYPES[name]
    thr = float(g["threshold"])
    hits = []
    with fbcache.cache_context(fbcache.create_cache_context()):
        for k in range(int(g["steps"])):
            p = f"trace_{mode}_{k}_"
            first, hidden = from_bits(g[p + "first"], dt), from_bits(g[p + "hidden"], dt)
            enc = from_bits(g[p + "enc"], dt) if mode == "multi" else None
            stored_before = fbcache.get_buffer(f"first_{mode}_hidden_states_residual")
            hit, _ = fbcache.get_can_use_cache(first, threshold=thr, mode=mode)
            assert bool(hit) == bool(g[p + "hit"]), f"step {k}"
            out_h, out_e, out_thr = fbcache.check_and_apply_cache(
                first_residual=first, hidden_states=hidden, encoder_hidden_states=enc, threshold=thr, parallelized=False, mode=mode,
                verbose=False, call_remaining_fn=remaining_multi if mode == "multi" else remaining_single, remaining_kwargs={})
            assert out_thr == thr and np.array_equal(bits(out_h), g[p + "out_hidden"]), f"step {k}"
            if mode == "multi":
                assert np.array_equal(bits(out_e), g[p + "out_enc"]), f"step {k}"
            else:
                assert out_e is None
            for b in BUFFERS:  # the same buffers exist, with the same contents
                have = fbcache.get_buffer(b)
                assert (have is not None) == (p + "buf_" + b in g.files), f"step {k}: {b}"
                if have is not None:
                    assert np.array_equal(bits(have), g[p + "buf_" + b]), f"step {k}: {b}"
            if hit:  # a hit leaves the stored first residual alone: the SAME tensor object
                assert fbcache.get_buffer(f"first_{mode}_hidden_states_residual") is stored_before
            hits.append(bool(hit))
    assert not hits[0] and any(hits) and not all(hits)


def test_context_functions():
    with pytest.raises(AssertionError, match="cache_context must be set before"):
        fbcache.get_buffer("x")
    with pytest.raises(AssertionError, match="cache_context must be set before"):
        fbcache.set_buffer("x", torch.zeros(1))
    outer, inner = fbcache.create_cache_context(), fbcache.create_cache_context()
    assert isinstance(outer, fbcache.CacheContext) and fbcache.get_current_cache_context() is None
    with fbcache.cache_context(outer):
        fbcache.set_buffer("x", torch.ones(1))
        with fbcache.cache_context(inner):
            assert fbcache.get_current_cache_context() is inner and fbcache.get_buffer("x") is None
        assert fbcache.get_current_cache_context() is outer and fbcache.get_buffer("x") is not None
        # no stored residual: a miss, and the reported distance is the threshold
        hit, diff = fbcache.get_can_use_cache(torch.ones(2, 2), threshold=0.25, mode="single")
        assert not bool(hit) and float(diff) == 0.25
        with pytest.raises(ValueError):
            fbcache.get_can_use_cache(torch.ones(2, 2), threshold=0.25, mode="other")
        with pytest.raises(AssertionError, match="single_hidden_states_residual must be set before"):
            fbcache.apply_prev_hidden_states_residual(torch.ones(2, 2), mode="single")
    assert fbcache.get_current_cache_context() is None
    assert outer.get_incremental_name() == "default_0" and outer.get_incremental_name("a") == "a_0" and outer.get_incremental_name("a") == "a_1"
    outer.reset_incremental_name()
    outer.clear_buffers()
    assert outer.get_incremental_name("a") == "a_0" and outer.buffers == {}


# ---- adapters on stand-ins (diffusers is not a dependency) -------------------------------------------------------------------------
def _stand_in_transformer():
    from nunchaku_amd.models.flux import FluxEngineMixin

    class Transformer(torch.nn.Module, FluxEngineMixin):
        """records which forward ran; the engine's cached forward is replaced by a probe"""

        def __init__(self):
            super().__init__()
            self.calls = []

        def forward(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None, img_ids=None, txt_ids=None,
                    guidance=None, joint_attention_kwargs=None, controlnet_block_samples=None, controlnet_single_block_samples=None,
                    return_dict=True, controlnet_blocks_repeat=False):
            self.calls.append("original")
            return hidden_states

        def engine_forward_cached(self, hidden_states, *args, **kwargs):
            assert fbcache.get_current_cache_context() is not None, "cache_context must be set before"
            self.calls.append(("cached", kwargs["use_double_fb_cache"], kwargs["residual_diff_threshold_multi"],
                               kwargs["residual_diff_threshold_single"], fbcache.get_current_cache_context()))
            return hidden_states

    return Transformer()


def test_apply_cache_on_transformer():
    t = _stand_in_transformer()
    original = t.forward
    assert apply_cache_on_transformer(t) is t and t._is_cached and t._original_forward == original
    assert (t.residual_diff_threshold_multi, t.residual_diff_threshold_single, t.use_double_fb_cache, t.verbose) == (0.12, -1.0, False, False)
    cached = t.forward
    assert cached != original
    # a second call only updates the thresholds and the mode
    apply_cache_on_transformer(t, use_double_fb_cache=True, residual_diff_threshold=0.2, residual_diff_threshold_single=0.3)
    assert t.forward == cached and t._original_forward == original
    assert (t.residual_diff_threshold_multi, t.residual_diff_threshold_single, t.use_double_fb_cache) == (0.2, 0.3, True)
    apply_cache_on_transformer(t, residual_diff_threshold=0.2, residual_diff_threshold_multi=0.09)
    assert t.residual_diff_threshold_multi == 0.09
    x = torch.zeros(1, 4, 8)
    with pytest.raises(AssertionError, match="cache_context must be set before"):  # use without an active context
        t(x, x, x, torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3))
    with fbcache.cache_context(fbcache.create_cache_context()):
        out = t(x, x, x, torch.zeros(1), torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), return_dict=False)
        assert isinstance(out, tuple) and out[0] is x
        assert t(x, x, x, torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3)).sample is x
    assert [c[0] for c in t.calls] == ["cached", "cached"] and t.calls[0][1:4] == (False, 0.09, None)
    # a negative multi threshold runs the original forward (no context needed)
    apply_cache_on_transformer(t, residual_diff_threshold=-1.0)
    assert t(x, x, x, torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3)) is x and t.calls[-1] == "original"
    with pytest.raises(TypeError):
        apply_cache_on_transformer(torch.nn.Linear(2, 2))


def test_apply_cache_on_pipe_opens_a_fresh_context_per_call():
    class FluxPipelineStandIn:
        def __init__(self):
            self.transformer = _stand_in_transformer()

        def __call__(self, steps):
            x = torch.zeros(1, 4, 8)
            for _ in range(steps):
                self.transformer(x, x, x, torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3))
            return "image"

    pipe = FluxPipelineStandIn()
    assert apply_cache_on_pipe(pipe, residual_diff_threshold=0.1) is pipe and FluxPipelineStandIn._is_cached
    wrapped = FluxPipelineStandIn.__call__
    apply_cache_on_pipe(pipe, residual_diff_threshold=0.15)  # the class is wrapped once; the thresholds follow
    assert FluxPipelineStandIn.__call__ is wrapped and pipe.transformer.residual_diff_threshold_multi == 0.15
    assert pipe(2) == "image" and pipe(1) == "image"
    ctxs = [c[4] for c in pipe.transformer.calls]
    assert ctxs[0] is ctxs[1] and ctxs[2] is not ctxs[0] and fbcache.get_current_cache_context() is None

    class SanaPipelineStandIn:
        transformer = None

    with pytest.raises(ValueError, match="Unknown pipeline class name"):
        apply_cache_on_pipe(SanaPipelineStandIn())


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
_STRUCTS = {"svdq_residual_diff_args": _lib.ResidualDiffArgs, "svdq_residual_diff_result": _lib.ResidualDiffResult}


def test_residual_diff_struct_layouts_match_header(built_lib, tmp_path):
    """sizeof and every field offset of the ctypes twins against what the C compiler makes of include/svdq_amd.h"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "svdq_amd.h")}"', "int main(void) {"]
    for cname, cls in _STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in _STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls), f"sizeof({cname}): header {got[cname]} != ctypes {C.sizeof(cls)}"
        for fname, _ in cls._fields_:
            assert int(got[f"{cname}.{fname}"]) == getattr(cls, fname).offset, f"offsetof({cname}, {fname})"
    assert C.sizeof(_lib.ResidualDiffResult) == 32


def test_residual_diff_exported_and_abi(built_lib):
    lib = C.CDLL(built_lib)
    assert hasattr(lib, "svdq_residual_diff") and "svdq_residual_diff" in _lib.EXPORTS
    assert _lib.load().svdq_abi_version() == _lib.ABI_VERSION == 24


def test_residual_diff_validation_errors_are_returned_not_aborted(built_lib):
    lib = _lib.load()
    assert lib.svdq_residual_diff(None, None) == 1 and b"NULL" in lib.svdq_last_error()
    a = _lib.ResidualDiffArgs()
    assert lib.svdq_residual_diff(C.byref(a), None) == 1 and b"cur is NULL" in lib.svdq_last_error()
    a.cur, a.base, a.out_res = 4096, 8192, 12288
    a.M, a.C, a.ld = 4, 100, 104
    assert lib.svdq_residual_diff(C.byref(a), None) == 1 and b"multiple of 8" in lib.svdq_last_error()
    a.C, a.ld = 256, 256
    a.base = 8192 + 2
    assert lib.svdq_residual_diff(C.byref(a), None) == 1 and b"16-byte aligned" in lib.svdq_last_error()
    a.base, a.prev = 8192, 16384  # prev without a result record
    assert lib.svdq_residual_diff(C.byref(a), None) == 1 and b"result record" in lib.svdq_last_error()
    a.prev, a.out_res, a.base = None, None, None
    assert lib.svdq_residual_diff(C.byref(a), None) == 1 and b"out_res / prev" in lib.svdq_last_error()
    a.base, a.out_res, a.dtype = 8192, 12288, 7
    assert lib.svdq_residual_diff(C.byref(a), None) == 1 and b"dtype" in lib.svdq_last_error()
    a.dtype, a.cur2, a.M2 = 0, 20480, 4  # the second problem must mirror the first
    assert lib.svdq_residual_diff(C.byref(a), None) == 1 and b"mirror" in lib.svdq_last_error()
    a.cur2, a.C, a.ld = None, 16384 + 512, 16384 + 512
    assert lib.svdq_residual_diff(C.byref(a), None) == 2 and b"ceil(C/512)" in lib.svdq_last_error()


def test_wrappers_refuse_cpu_tensors(built_lib):
    from nunchaku_amd.ops.elementwise import residual_diff

    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        residual_diff(x, x)
