"""Generate tests/golden/fbcache_{bf16,fp16}.npz from the REFERENCE's own First-Block-Cache functions (run in the build container only).

`nunchaku/caching/fbcache.py` of the reference imports only torch, so it is loaded by path.  Two kinds of records, on CPU torch:

(a) `sim_*`: pairs `prev`, `cur = prev + a * noise` of 64 x 256 with a in AMPLITUDES, and what `are_two_tensors_similar(prev, cur,
    threshold=0.12)` answers: the 16-bit ratio (bit pattern) and the decision;
(b) `trace_{multi,single}_*`: `check_and_apply_cache` over STEPS first residuals with a toy `call_remaining_fn` (the same arithmetic
    is restated in tests/test_fbcache.py): hit / miss, the returned tensors and every buffer after each step.

Every recorded ratio must lie outside [0.5, 2] x threshold, so that no decision sits near a rounding boundary: asserted here.
16-bit tensors are stored as their uint16 bit patterns.  The reference does not exist on the GPU box: only the .npz files travel.

    python tools/make_fbcache_golden.py
"""

import importlib.util
import os

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
THRESHOLD = 0.12
# ratios of about a (E|a n| / E|n|).  0.2 would sit inside the excluded band [0.06, 0.24] around the threshold: 0.3 stands for "clearly above"
AMPLITUDES = (0.0, 0.02, 0.05, 0.3, 0.5)
# the trace: ("new", -) a fresh random residual; ("near", a) the LAST "new" residual + a * fresh noise.  A run of "near" steps keeps
# being compared with the last computed step's residual, not with each other.
STEPS = (("new", 0), ("near", 0.02), ("near", 0.05), ("near", 0.5), ("near", 0.02), ("new", 0), ("near", 0.05), ("near", 0.05),
         ("near", 0.3), ("near", 0.0))
TRACE_SHAPE = (1, 8, 64)
BUFFERS = ("first_multi_hidden_states_residual", "multi_hidden_states_residual", "multi_encoder_hidden_states_residual",
           "first_single_hidden_states_residual", "single_hidden_states_residual")


def load_reference_fbcache():
    spec = importlib.util.spec_from_file_location("reference_fbcache", f"{REF}/nunchaku/caching/fbcache.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def remaining_multi(hidden_states, encoder_hidden_states):
    uh, ue = hidden_states * 1.25 + 0.5, encoder_hidden_states * 0.75 - 0.25
    return uh, ue, uh - hidden_states, ue - encoder_hidden_states


def remaining_single(hidden_states, encoder_hidden_states):
    uc = hidden_states * 1.5 + 0.125
    return uc, uc - hidden_states


def check_band(ratio: float, what: str):
    assert not (0.5 * THRESHOLD <= ratio <= 2 * THRESHOLD), f"{what}: ratio {ratio} inside [0.5, 2] x threshold"


def main():
    fb = load_reference_fbcache()
    os.makedirs(OUT, exist_ok=True)
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        g = torch.Generator().manual_seed(1234)
        rec = {"threshold": np.float64(THRESHOLD), "amplitudes": np.array(AMPLITUDES)}
        prev = torch.randn(64, 256, generator=g).to(dt)
        rec["sim_prev"] = bits(prev)
        for i, a in enumerate(AMPLITUDES):
            cur = prev + (a * torch.randn(64, 256, generator=g)).to(dt)
            similar, ratio = fb.are_two_tensors_similar(prev, cur, threshold=THRESHOLD)
            check_band(float(ratio), f"{name} sim {a}")
            rec[f"sim_cur_{i}"], rec[f"sim_ratio_{i}"], rec[f"sim_similar_{i}"] = bits(cur), bits(ratio.reshape(1)), np.bool_(bool(similar))
        for mode, fn in (("multi", remaining_multi), ("single", remaining_single)):
            with fb.cache_context(fb.create_cache_context()):
                anchor = None
                for k, (kind, a) in enumerate(STEPS):
                    rnd = lambda: torch.randn(TRACE_SHAPE, generator=g)
                    if kind == "new":
                        first = anchor = rnd().to(dt)
                    else:
                        first = anchor + (a * rnd()).to(dt)
                    hidden, enc = rnd().to(dt), (rnd().to(dt) if mode == "multi" else None)
                    stored = fb.get_buffer(f"first_{mode}_hidden_states_residual")
                    if stored is not None:
                        check_band(float(fb.are_two_tensors_similar(stored, first, threshold=THRESHOLD)[1]), f"{name} {mode} step {k}")
                    hit, _ = fb.get_can_use_cache(first, threshold=THRESHOLD, mode=mode)
                    out_h, out_e, _ = fb.check_and_apply_cache(
                        first_residual=first, hidden_states=hidden, encoder_hidden_states=enc, threshold=THRESHOLD, parallelized=False,
                        mode=mode, verbose=False, call_remaining_fn=fn, remaining_kwargs={})
                    p = f"trace_{mode}_{k}_"
                    rec[p + "first"], rec[p + "hidden"], rec[p + "hit"], rec[p + "out_hidden"] = bits(first), bits(hidden), np.bool_(bool(hit)), bits(out_h)
                    if enc is not None:
                        rec[p + "enc"], rec[p + "out_enc"] = bits(enc), bits(out_e)
                    for b in BUFFERS:
                        if fb.get_buffer(b) is not None:
                            rec[p + "buf_" + b] = bits(fb.get_buffer(b))
                hits = [bool(rec[f"trace_{mode}_{k}_hit"]) for k in range(len(STEPS))]
                assert any(hits) and not all(hits) and not hits[0], hits
                print(name, mode, "hits:", "".join("H" if h else "." for h in hits))
        rec["steps"] = np.int64(len(STEPS))
        path = os.path.join(OUT, f"fbcache_{name}.npz")
        np.savez_compressed(path, **rec)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
