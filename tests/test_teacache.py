"""TeaCache without a GPU: the context manager, the state machine on scripted ratio sequences against a straight-line restatement of the
reference's rule (nunchaku/caching/teacache.py:188-214, 218-256) evaluated with ``numpy.poly1d``, the refusals, and the C ABI of
svdq_modulated_diff (declaration, layout, export, validation)."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from nunchaku.caching.teacache import TeaCache
from nunchaku_amd import _lib
from nunchaku_amd.caching import teacache as tc
from nunchaku_amd.models.flux import FluxEngineMixin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("cnt", "accumulated_rel_l1_distance", "previous_modulated_input", "previous_residual")


class Stub:
    """A transformer as TeaCache sees it: the engine's ``teacache_forward`` hands the state machine a ratio function (here: the scripted
    ratio of the step) and acts on its answer; ``log`` keeps (should_calc, refresh, ratio asked for or None) per step."""

    def __init__(self, ratios=()):
        self.ratios, self.step, self.log, self.fail = list(ratios), 0, [], False

    def forward(self, *args, **kwargs):
        return "original"

    def teacache_forward(self, *args, decide):
        asked = []

        def ratio_fn():
            asked.append(self.ratios[self.step])
            return asked[-1]

        if self.fail:
            raise KeyError("boom")
        should_calc, refresh = decide(ratio_fn)
        if refresh and not should_calc:
            assert self.previous_residual is not None, "a skip needs a stored residual"
        if refresh and should_calc:
            self.previous_residual = ("residual of step", self.step)
        self.log.append((should_calc, refresh, asked[0] if asked else None))
        self.step += 1
        return torch.zeros(1)


def reference_rule(ratios, num_steps, rel_l1_thresh, skip_steps, coefficients):
    """The reference's lines, one after the other -> per step (should_calc, cnt > skip_steps, accumulator after the step, the step whose
    residual is stored after the step or None)."""
    rescale_func = np.poly1d(coefficients)
    cnt, acc, residual, out = 0, 0, None, []
    for step, ratio in enumerate(ratios):
        if cnt == 0 or cnt == num_steps - 1:
            should_calc = True
            acc = 0
        else:
            acc += np.abs(rescale_func(ratio))
            if acc < rel_l1_thresh:
                should_calc = False
            else:
                should_calc = True
                acc = 0
        cnt += 1
        if cnt == num_steps:
            cnt = 0
        if cnt > skip_steps:
            if not should_calc:
                assert residual is not None, "the scripted sequence must not skip before a residual is stored (the reference fails there)"
            else:
                residual = step
        out.append((should_calc, cnt > skip_steps, float(acc), residual))
    return out


def test_import_paths():
    assert TeaCache is tc.TeaCache
    from nunchaku.caching.teacache import make_teacache_forward

    assert make_teacache_forward is tc.make_teacache_forward


@pytest.mark.parametrize("raises", [False, True])
def test_context_installs_and_restores(raises):
    m = Stub([0.0] * 4)
    original = m.forward
    assert "forward" not in vars(m)
    try:
        with TeaCache(m, num_steps=4) as ctx:
            assert isinstance(ctx, TeaCache) and m.forward != original
            assert (m.cnt, m.accumulated_rel_l1_distance, m.previous_modulated_input, m.previous_residual) == (0, 0, None, None)
            x = torch.zeros(1, 4, 8)
            out = m.forward(x, x, x, torch.zeros(1), torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), return_dict=False)
            assert isinstance(out, tuple) and m.cnt == 1 and m.log == [(True, True, None)]
            assert m.forward(x, x, x, torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3)).sample is not None
            with pytest.raises(ValueError, match="joint_attention_kwargs"):  # refused like the other unsupported inputs; empty is fine
                m.forward(x, joint_attention_kwargs={"scale": 0.5})
            assert m.forward(x, joint_attention_kwargs={}, controlnet_blocks_repeat=True).sample is not None and m.cnt == 3
            with pytest.raises(RuntimeError, match="already inside"):
                TeaCache(m).__enter__()
            if raises:
                m.fail = True
                m.forward(x)
    except KeyError:
        assert raises
    else:
        assert not raises
    assert m.forward == original and m.forward() == "original" and "forward" not in vars(m)
    assert not any(hasattr(m, name) for name in STATE)
    # a forward set on the instance comes back as that instance attribute
    m.forward = lambda *a, **k: "own"
    own = m.forward
    with TeaCache(m):
        assert m.forward is not own
    assert m.forward is own


def test_disabled_is_a_no_op():
    m = Stub()
    before = dict(vars(m))
    with TeaCache(m, enabled=False) as ctx:
        assert isinstance(ctx, TeaCache) and vars(m) == before and m.forward() == "original"
    assert vars(m) == before


BF16_RATIOS = [0.0625, 0.03125, 0.25, 0.0078125, 0.125, 0.09375, 0.5, 0.015625, 0.046875, 0.1875, 0.00390625, 0.0234375]
OWN = (2.0, -1.0, 0.125)


@pytest.mark.parametrize("skip_steps", [0, 3])
# (thresholds at which step 3 -- the first outside a window of 3 -- reaches the threshold: the reference cannot skip before a residual is stored)
@pytest.mark.parametrize("name,coefficients,thresh", [("flux", None, 0.6), ("flux", None, 0.2), ("flux-kontext", None, 0.2),
                                                      ("flux", OWN, 0.2)])
def test_state_machine_follows_the_reference_rule(name, coefficients, thresh, skip_steps):
    """Two runs of six steps (``cnt`` wraps into the second run), 16-bit ratios as the record delivers them."""
    num_steps = 6
    coeffs = OWN if coefficients is not None else tc.COEFFICIENTS[name]
    expect = reference_rule(BF16_RATIOS, num_steps, thresh, skip_steps, coeffs)
    m = Stub(BF16_RATIOS)
    x = torch.zeros(1, 4, 8)
    with TeaCache(m, num_steps=num_steps, rel_l1_thresh=thresh, skip_steps=skip_steps, model_name=name, coefficients=coefficients):
        for step, (should_calc, refresh, acc, residual) in enumerate(expect):
            m.forward(x)
            got_calc, got_refresh, asked = m.log[-1]
            forced = step % num_steps in (0, num_steps - 1)
            assert (got_calc, got_refresh) == (should_calc, refresh), f"step {step}"
            assert m.accumulated_rel_l1_distance == acc, f"step {step}: accumulator (float64, numpy.poly1d)"
            assert asked == (None if forced else BF16_RATIOS[step]), "the ratio is read only when the outcome is not forced"
            assert m.cnt == (step + 1) % num_steps
            assert m.previous_residual == (None if residual is None else ("residual of step", residual)), f"step {step}"
            if forced:
                assert should_calc and acc == 0.0
            if should_calc:
                assert acc == 0.0  # the accumulator is reset on a computed step
    calcs = [e[0] for e in expect]
    refreshes = [e[1] for e in expect]
    assert calcs[0] and calcs[5] and calcs[6] and calcs[11]
    if skip_steps == 3:  # steps 0, 1, 2 of each run lie inside the window (cnt after the increment: 1, 2, 3) and step 5 (cnt wrapped to 0)
        assert refreshes == [False, False, False, True, True, False] * 2
        assert all(m.log[i][1] is False for i in (0, 1, 2, 5))
    else:
        assert refreshes == [True, True, True, True, True, False] * 2
    assert not all(calcs), "the sequence must contain skipped steps"


def test_sequences_cover_skips_and_threshold_resets():
    """the scripted cases above are not vacuous: with the published FLUX polynomial at 0.6 there are skips, a computed step caused by the
    accumulator reaching the threshold, and a skip right after such a reset"""
    e = reference_rule(BF16_RATIOS, 6, 0.6, 0, tc.COEFFICIENTS["flux"])
    calcs = [x[0] for x in e]
    assert calcs.count(False) >= 3
    assert any(c and i % 6 not in (0, 5) for i, c in enumerate(calcs)), "a step computed because the accumulator reached the threshold"
    assert tc.rescale(tc.COEFFICIENTS["flux"], 0.125) == abs(np.poly1d(tc.COEFFICIENTS["flux"])(0.125))
    assert tc.rescale(OWN, 0.5) == abs(2.0 * 0.25 - 0.5 + 0.125)


def test_a_skip_without_a_stored_residual_is_computed():
    """skip_steps = 2 and a huge threshold: step 2 is the first outside the window, the rule says "skip", nothing is stored yet (the
    reference fails there adding None) -> computed, the residual stored, the accumulator reset; step 3 then skips."""
    m = Stub([0.0625] * 5)
    with TeaCache(m, num_steps=5, rel_l1_thresh=1e9, skip_steps=2):
        for _ in range(5):
            m.forward(torch.zeros(1, 4, 8))
            if len(m.log) == 3:
                assert m.accumulated_rel_l1_distance == 0.0
    assert [(c, r) for c, r, _ in m.log] == [(True, False), (False, False), (True, True), (False, True), (True, False)]


def test_unknown_model_name_and_bad_coefficients():
    with pytest.raises(ValueError, match="no coefficients for model 'sana'"):
        TeaCache(Stub(), model_name="sana")
    with pytest.raises(ValueError, match="at least one"):
        TeaCache(Stub(), coefficients=[])
    assert TeaCache(Stub(), model_name="sana", coefficients=[1.0, 0.0]).coefficients == (1.0, 0.0)  # the override needs no known name
    assert TeaCache(Stub(), model_name="flux-kontext").coefficients == tc.COEFFICIENTS["flux-kontext"]
    assert len(tc.COEFFICIENTS["flux"]) == len(tc.COEFFICIENTS["flux-kontext"]) == 5


def test_refusals():
    class Engine(FluxEngineMixin):  # the refusals come before anything touches a weight
        blocks, single_blocks = (), ()

        def forward(self, *args):
            return "original"

    x = torch.zeros(1, 4, 8)
    rest = (x, x, torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3))
    e = Engine()
    with pytest.raises(ValueError, match="batch 1"):
        e.teacache_forward(torch.zeros(2, 4, 8), *rest, decide=None)
    with pytest.raises(ValueError, match="ControlNet"):
        e.teacache_forward(x, *rest, controlnet_block_samples=[x], decide=None)
    with pytest.raises(ValueError, match="ControlNet"):
        e.teacache_forward(x, *rest, controlnet_single_block_samples=[x], decide=None)
    with pytest.raises(ValueError, match="at least one joint block"):
        e.teacache_forward(x, *rest, decide=None)
    # First-Block Cache switched on on the same model: refused on entering the context and by the forward itself
    e._is_cached, e.residual_diff_threshold_multi = True, 0.12
    with pytest.raises(RuntimeError, match="First-Block Cache"):
        e.teacache_forward(x, *rest, decide=None)
    with pytest.raises(RuntimeError, match="First-Block Cache"):
        TeaCache(e).__enter__()
    assert not any(hasattr(e, name) for name in STATE) and "forward" not in vars(e)
    e.residual_diff_threshold_multi = -1.0  # applied but switched off: fine
    with TeaCache(e):
        pass
    e._is_cached = False
    e.offload = True
    with pytest.raises(NotImplementedError, match="offloaded"):
        e.teacache_forward(x, *rest, decide=None)
    with pytest.raises(NotImplementedError, match="offloaded"):
        TeaCache(e).__enter__()
    with pytest.raises(TypeError, match="not a FLUX transformer"):
        TeaCache(torch.nn.Linear(2, 2)).__enter__()
    with TeaCache(torch.nn.Linear(2, 2), enabled=False):  # disabled: nothing is looked at
        pass


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_modulated_diff_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    assert re.search(r"^int svdq_modulated_diff\(const svdq_modulated_diff_args \*args, void \*stream\);", text, re.M)
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M)
    assert "WITHOUT a version bump" in text
    assert _lib.ABI_VERSION == 24 and "svdq_modulated_diff" in _lib.EXPORTS


def test_modulated_diff_struct_layout_matches_header(built_lib, tmp_path):
    cname, cls = "svdq_modulated_diff_args", _lib.ModulatedDiffArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "svdq_amd.h")}"', "int main(void) {",
             f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0; }")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"offsetof({cname}, {f})"


def test_modulated_diff_exported_and_validation_errors_are_returned(built_lib):
    lib = _lib.load()
    assert hasattr(C.CDLL(built_lib), "svdq_modulated_diff") and lib.svdq_abi_version() == 24
    assert lib.svdq_modulated_diff(None, None) == 1 and b"NULL" in lib.svdq_last_error()
    a = _lib.ModulatedDiffArgs()
    assert lib.svdq_modulated_diff(C.byref(a), None) == 1 and b"are required" in lib.svdq_last_error()
    a.x, a.stats, a.mod_scale, a.mod_shift = 4096, 8192, 12288, 16384
    a.M, a.C, a.ld = 4, 256, 256
    assert lib.svdq_modulated_diff(C.byref(a), None) == 1 and b"out_mod / prev" in lib.svdq_last_error()
    a.prev = 20480  # prev without a result record
    assert lib.svdq_modulated_diff(C.byref(a), None) == 1 and b"result record" in lib.svdq_last_error()
    a.prev, a.out_mod, a.C, a.ld = None, 24576, 100, 104
    assert lib.svdq_modulated_diff(C.byref(a), None) == 1 and b"multiple of 8" in lib.svdq_last_error()
    a.C, a.ld = 256, 248
    assert lib.svdq_modulated_diff(C.byref(a), None) == 1 and b"ld=248 >= C" in lib.svdq_last_error()
    a.ld, a.M = 256, 0
    assert lib.svdq_modulated_diff(C.byref(a), None) == 1 and b"M=0 > 0" in lib.svdq_last_error()
    a.M, a.mod_shift = 4, 16384 + 2
    assert lib.svdq_modulated_diff(C.byref(a), None) == 1 and b"16-byte aligned" in lib.svdq_last_error()
    a.mod_shift, a.stats = 16384, 8192 + 4
    assert lib.svdq_modulated_diff(C.byref(a), None) == 1 and b"16-byte aligned" in lib.svdq_last_error()
    a.stats, a.dtype = 8192, 7
    assert lib.svdq_modulated_diff(C.byref(a), None) == 1 and b"dtype" in lib.svdq_last_error()
    a.dtype, a.C, a.ld = 0, 16384 + 512, 16384 + 512
    assert lib.svdq_modulated_diff(C.byref(a), None) == 2 and b"ceil(C/512)" in lib.svdq_last_error()  # SVDQ_E_UNSUPPORTED, as its two siblings


def test_wrapper_refuses_cpu_tensors_and_mismatched_shapes(built_lib):
    from nunchaku_amd.ops.elementwise import modulated_diff

    x = torch.zeros(4, 256, dtype=torch.bfloat16)
    st, v = torch.zeros(4, 2), torch.zeros(256, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        modulated_diff(x, st, v, v)
    with pytest.raises(ValueError, match="shapes differ"):
        modulated_diff(x, st, v, v, prev=torch.zeros(5, 256, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="stats must be"):
        modulated_diff(x, torch.zeros(3, 2), v, v)
