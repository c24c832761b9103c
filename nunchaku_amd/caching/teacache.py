"""TeaCache: the context manager and the decision (reference: nunchaku/caching/teacache.py; Liu et al., "Timestep Embedding Tells: It's
Time to Cache for Video Diffusion Model").

Before any transformer block of a denoising step runs, the AdaLayerNormZero-modulated input of the first joint block is compared with the
one of the previous step (relative L1 distance).  A polynomial fitted by the TeaCache authors turns that distance into an estimate of how
much the model's output changed; the estimates are accumulated, and while the sum stays below ``rel_l1_thresh`` the step is skipped: the
summed effect of all blocks at the last computed step (``previous_residual``) is added to the embedded latents instead.  The first and the
last step of a run of ``num_steps`` always compute.  Arguments, state names (``cnt``, ``accumulated_rel_l1_distance``,
``previous_modulated_input``, ``previous_residual``) and the state machine are the reference's; two things are this library's:

* ``coefficients=`` overrides the polynomial (highest power first, as ``numpy.poly1d`` takes them);
* a step that the state machine would skip while no residual is stored yet -- possible with ``skip_steps`` > 0, whose window computes
  without storing one; the reference fails there adding ``None`` -- is computed instead, as a step that reached the threshold.

The engine side is ``FluxEngineMixin.teacache_forward`` (models/flux.py): one ``svdq_modulated_diff`` pass forms the modulated input from
what the step has anyway and compares it in the same pass; the 16-bit quotient is read on the host, which synchronises the stream.
"""

from __future__ import annotations

from types import MethodType
from typing import Callable, Optional, Sequence, Tuple

# rescaling polynomials published by the TeaCache authors (TeaCache4FLUX), highest power first
COEFFICIENTS = {
    "flux": (4.98651651e02, -2.83781631e02, 5.58554382e01, -3.82021401e00, 2.64230861e-01),
    "flux-kontext": (-1.04655119e03, 3.12563399e02, -1.69500694e01, 4.10995971e-01, 3.74537863e-02),
}

STATE = ("cnt", "accumulated_rel_l1_distance", "previous_modulated_input", "previous_residual")


def resolve_coefficients(model_name: str, coefficients: Optional[Sequence[float]] = None) -> Tuple[float, ...]:
    if coefficients is not None:
        coefficients = tuple(float(c) for c in coefficients)
        if not coefficients:
            raise ValueError("TeaCache: coefficients must hold at least one number")
        return coefficients
    if model_name not in COEFFICIENTS:
        raise ValueError(f"TeaCache: no coefficients for model {model_name!r}; known: {sorted(COEFFICIENTS)} (or pass coefficients=)")
    return COEFFICIENTS[model_name]


def rescale(coefficients: Sequence[float], ratio: float) -> float:
    """``abs(numpy.poly1d(coefficients)(ratio))`` in float64: Horner's rule, the order numpy evaluates in."""
    y = 0.0
    for c in coefficients:
        y = y * ratio + c
    return abs(y)


def teacache_decide(model, ratio_fn: Callable[[], float], *, num_steps: int, rel_l1_thresh: float, skip_steps: int,
                    coefficients: Sequence[float]) -> Tuple[bool, bool]:
    """One step of the state machine on ``model``'s ``cnt`` / ``accumulated_rel_l1_distance`` (reference: teacache.py:188-214, 218).
    ``ratio_fn()`` gives ``mean|m - m_prev| / mean|m_prev|`` of this step's modulated input; it is called only when the outcome is not
    forced.  Returns ``(should_calc, refresh)``: ``refresh`` False is a step inside the ``skip_steps`` window -- every block runs whatever
    ``should_calc`` says and ``previous_residual`` is left alone."""
    if model.cnt == 0 or model.cnt == num_steps - 1:
        should_calc = True
        model.accumulated_rel_l1_distance = 0.0
    else:
        model.accumulated_rel_l1_distance += rescale(coefficients, float(ratio_fn()))
        should_calc = not model.accumulated_rel_l1_distance < rel_l1_thresh
        if should_calc:
            model.accumulated_rel_l1_distance = 0.0
    model.cnt += 1
    if model.cnt == num_steps:
        model.cnt = 0
    refresh = model.cnt > skip_steps  # (tested after the increment, as the reference does)
    if refresh and not should_calc and model.previous_residual is None:  # nothing to add yet: compute
        should_calc = True
        model.accumulated_rel_l1_distance = 0.0
    return should_calc, refresh


def make_teacache_forward(num_steps: int = 50, rel_l1_thresh: float = 0.6, skip_steps: int = 0, model_name: str = "flux",
                          coefficients: Optional[Sequence[float]] = None) -> Callable:
    """The forward that replaces ``transformer.forward`` (bind it with ``types.MethodType``): the pipeline's keywords, the engine's
    ``teacache_forward`` underneath.  Batch 1 only, no ControlNet residuals, no ``joint_attention_kwargs``, not under stream capture (each
    raises); ``controlnet_blocks_repeat`` only selects among ControlNet residuals and has nothing to act on."""
    coeffs = resolve_coefficients(model_name, coefficients)

    def teacache_forward(self, hidden_states, encoder_hidden_states=None, pooled_projections=None, timestep=None, img_ids=None,
                         txt_ids=None, guidance=None, joint_attention_kwargs=None, controlnet_block_samples=None,
                         controlnet_single_block_samples=None, return_dict: bool = True, controlnet_blocks_repeat: bool = False):
        if joint_attention_kwargs:
            raise ValueError(f"TeaCache does not support joint_attention_kwargs (got {sorted(joint_attention_kwargs)}): the engine has no "
                             "attention processors to hand them to")
        if txt_ids is not None and txt_ids.ndim == 3:
            txt_ids = txt_ids[0]
        if img_ids is not None and img_ids.ndim == 3:
            img_ids = img_ids[0]
        out = self.teacache_forward(
            hidden_states, encoder_hidden_states, pooled_projections, timestep, img_ids, txt_ids, guidance, controlnet_block_samples,
            controlnet_single_block_samples,
            decide=lambda ratio_fn: teacache_decide(self, ratio_fn, num_steps=num_steps, rel_l1_thresh=rel_l1_thresh,
                                                    skip_steps=skip_steps, coefficients=coeffs))
        from .diffusers_adapters.flux_v2 import _pipeline_signature

        if not _pipeline_signature(self):  # the stand-alone model returns the tensor
            return out
        from ..models.transformer_flux import Transformer2DModelOutput

        return Transformer2DModelOutput(sample=out) if return_dict else (out,)

    return teacache_forward


class TeaCache:
    """``with TeaCache(transformer, num_steps=50, rel_l1_thresh=0.6, skip_steps=0): ...`` -- inside the block ``transformer.forward`` is the
    cached forward and the transformer carries the four state attributes; on exit (also when an exception passes through) the forward is
    put back and the state removed.  ``enabled=False`` changes nothing.  ``transformer``: ``NunchakuFluxTransformer2DModelV2`` or the
    stand-alone ``FluxTransformerAMD`` (anything with the engine's ``teacache_forward``)."""

    def __init__(self, model, num_steps: int = 50, rel_l1_thresh: float = 0.6, skip_steps: int = 0, enabled: bool = True,
                 model_name: str = "flux", coefficients: Optional[Sequence[float]] = None) -> None:
        self.model = model
        self.num_steps = num_steps
        self.rel_l1_thresh = rel_l1_thresh
        self.skip_steps = skip_steps
        self.enabled = enabled
        self.model_name = model_name
        self.coefficients = resolve_coefficients(model_name, coefficients)
        self.previous_model_forward = None

    def __enter__(self) -> "TeaCache":
        if not self.enabled:
            return self
        model = self.model
        if not callable(getattr(model, "teacache_forward", None)):
            raise TypeError(f"TeaCache: {type(model).__name__} is not a FLUX transformer of this library")
        if getattr(model, "_is_cached", False) and getattr(model, "residual_diff_threshold_multi", -1.0) >= 0.0:
            raise RuntimeError("TeaCache and First-Block Cache cannot be active on the same model: both decide which blocks of a step run "
                               "(switch First-Block Cache off: residual_diff_threshold_multi < 0)")
        if getattr(model, "offload", False):
            raise NotImplementedError("TeaCache does not support an offloaded model")
        if getattr(model, "ip_adapter", None) is not None:
            raise NotImplementedError("TeaCache with an IP-Adapter attached is not supported (the reference has no such combination)")
        if any(hasattr(model, name) for name in STATE):
            raise RuntimeError("TeaCache: this model is already inside a TeaCache context")
        # the instance attribute, if there is one, comes back on exit; a forward found on the class is uncovered again by deleting ours
        self._had_own_forward = "forward" in vars(model)
        self.previous_model_forward = model.forward
        model.forward = MethodType(make_teacache_forward(self.num_steps, self.rel_l1_thresh, self.skip_steps, self.model_name,
                                                         self.coefficients), model)
        model.cnt = 0
        model.accumulated_rel_l1_distance = 0.0
        model.previous_modulated_input = None
        model.previous_residual = None
        return self

    def __exit__(self, exc_type, exc_value, traceback) -> None:
        if not self.enabled or self.previous_model_forward is None:
            return
        model = self.model
        if self._had_own_forward:
            model.forward = self.previous_model_forward
        else:
            del model.forward
        self.previous_model_forward = None
        for name in STATE + ("_teacache_scratch",):  # (the last: the decision pass's partial sums and record, kept by the engine)
            if hasattr(model, name):
                delattr(model, name)
