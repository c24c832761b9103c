"""Test-side glue between the numpy oracle (float32 carriers) and torch GPU tensors."""

import numpy as np
import torch

from oracle import svdq_oracle as O

TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def t16(a: np.ndarray, dtype: str, device="cuda") -> torch.Tensor:
    """exactly-representable float32 carrier -> 16-bit torch tensor"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TORCH_DT[dtype]).to(device)


def f32(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def reference_state_dict(layer: dict, dtype: str) -> dict:
    """Logical oracle layer -> tensors in the REFERENCE checkpoint layout (what load_state_dict sees)."""
    td = TORCH_DT[dtype]
    sd = {
        "qweight": torch.from_numpy(O.pack_qweight_ref(layer["qweight"])),
        "wscales": torch.from_numpy(O.pack_wscales_ref(layer["wscales"])).to(td),
        "smooth_factor": torch.from_numpy(O.pack_vec_ref(layer["smooth"])).to(td),
        "smooth_factor_orig": torch.from_numpy(O.pack_vec_ref(layer["smooth"])).to(td),
        "proj_down": torch.from_numpy(O.pack_lowrank_ref(np.ascontiguousarray(layer["proj_down"].T), down=True)).to(td),
        "proj_up": torch.from_numpy(O.pack_lowrank_ref(layer["proj_up"], down=False)).to(td),
    }
    if layer.get("bias") is not None:
        sd["bias"] = torch.from_numpy(O.pack_vec_ref(layer["bias"])).to(td)
    return sd


def make_module(layer: dict, dtype: str, act_unsigned=False, device="cuda"):
    from nunchaku_amd.models.linear import SVDQW4A4Linear

    N, K = layer["qweight"].shape
    R = layer["proj_up"].shape[1]
    m = SVDQW4A4Linear(K, N, rank=R, bias=layer.get("bias") is not None, act_unsigned=act_unsigned,
                       torch_dtype=TORCH_DT[dtype], device=device)
    m.load_state_dict(reference_state_dict(layer, dtype))
    return m


def assert_close_16(got: np.ndarray, ref: np.ndarray, dtype: str, what: str, max_bad_frac=0.0, ulps=1.0):
    """|got - ref| <= ulps * (one 16-bit ulp relative bound) * |ref| + tiny absolute slack."""
    rel = (2.0 ** -7 if dtype == "bf16" else 2.0 ** -10) * ulps
    atol = rel * 1e-2 * float(np.abs(ref).max() + 1e-30)
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bad = err > rel * np.abs(ref) + atol
    frac = bad.mean()
    assert frac <= max_bad_frac, f"{what}: {bad.sum()} / {bad.size} elements off by more than {ulps} ulp (max err {err.max():.4g})"


def psnr_db(got, ref) -> float:
    """10 log10(max|ref|^2 / mean (got - ref)^2) of two torch tensors"""
    import torch

    got, ref = got.float(), ref.float()
    mse = ((got - ref) ** 2).mean().item()
    return float("inf") if mse == 0 else 10.0 * float(torch.log10(ref.abs().max() ** 2 / mse))


def checked_codes(qx, asc, x: np.ndarray, smooth, dtype: str, max_flips: float = 1e-3, rows=None):
    """The operands a GEMM launch consumed -- the GPU quantiser's codes [M_pad, K] and scales [K/64, M_pad] as numpy -- after checking them against
    the oracle: every code and scale inside the approximation envelope (oracle.quantize_envelope: the reference divides with __fdividef and
    inverts the scale with rcp.approx; this library with v_rcp_f32 -- neither is the IEEE quotient, both must land in the envelope), and at most
    ``max_flips`` of the codes / scales different from the IEEE oracle's (SURVEY.md section 8c's tolerance: +-1 LSB on < 1e-3 of the elements).
    GEMM tests then hold the GEMM to 1 ulp on the operands it really read.  ``rows``: check (and return) only these rows of a large launch; ``x`` is
    then the full input."""
    from nunchaku_amd import layout

    K = x.shape[1]
    codes = layout.unpack_act(qx, K).cpu().numpy()
    scales = f32(layout.unpack_scales(asc, codes.shape[0]))
    if rows is not None:
        x, codes, scales = x[rows], codes[rows], scales[:, rows]
    q_ieee, a_ieee, _ = O.quantize_w4a4_act_fuse_lora(x, smooth, None, dtype, pad_size=1 if rows is not None else O.PAD_M)
    env = O.quantize_envelope(x, smooth, dtype, pad_size=1 if rows is not None else O.PAD_M)
    rep = O.envelope_report(codes, env, q_ieee)
    assert rep["outside"] == 0.0, f"quantiser codes outside the approximation envelope: {rep}"
    assert rep["flips_vs_ieee"] <= max_flips and rep["max_abs_diff_vs_ieee"] <= 1, f"quantiser codes vs the IEEE oracle: {rep}"
    assert np.all(scales >= env["s_lo"]) and np.all(scales <= env["s_hi"]), "quantiser scales outside the approximation envelope"
    assert (scales != a_ieee).mean() <= max_flips, f"{(scales != a_ieee).sum()} scales differ from the IEEE oracle"
    return codes, scales


def retargeted(monkeypatch, symbol: str, launch, edit=None, **fields):
    """``launch()`` with the args struct of the library entry point ``symbol`` changed on its way into the library: ``fields`` are written into it, then
    ``edit(args)`` may change it further (it sees the struct the wrapper built, addresses included).  A batched entry point (``(entries, count, stream)``)
    gets both for each of its ``count`` entries, ``edit(args, i)``.  Everything else about the call is the wrapper's.  Synchronises; -> what ``launch()``
    returned.  (tests/test_gpu_large_extents.py: wide strides; tests/test_gpu_min_alignment.py: the smallest admitted alignments.)"""
    from nunchaku_amd import _lib

    lib = _lib.load()
    real = getattr(lib, symbol)
    batched = len(_lib.EXPORTS[symbol][1]) == 3

    def patched(ref, *rest):
        entries = [ref[i] for i in range(rest[0])] if batched else [ref._obj]
        for i, a in enumerate(entries):
            for k, v in fields.items():
                setattr(a, k, v)
            if edit is not None:
                edit(a, i) if batched else edit(a)
        return real(ref, *rest)

    with monkeypatch.context() as m:
        m.setattr(lib, symbol, patched)
        res = launch()
    torch.cuda.synchronize()
    return res


def served_fragment_images(module: torch.nn.Module):
    """The MFMA-fragment images of low-rank factors (``nunchaku_amd._C._packed_fragments``, ABI 21) that the cache would SERVE for the parameters of
    ``module`` now -- entries whose version is the parameter's current ``_version`` -- each compared with a fresh pack of the parameter's current
    bytes.  Returns ``(images checked, names of the parameters whose served image differs)``.  Bytes a pack does not write (padding) are not compared:
    they are found by packing twice into buffers filled with different bytes.  Synchronises the device."""
    from nunchaku_amd import _C, _lib

    lib = _lib.load()
    torch.cuda.synchronize()
    checked, stale = 0, []
    for name, p in module.named_parameters():
        for (kind, off, shape), (ver, img) in (_C._converted.get(p) or {}).items():
            if not kind.startswith("frag_") or off != p.storage_offset() or shape != tuple(p.shape) or ver != p._version:
                continue
            down = kind == "frag_down"
            N, R = shape  # down: [K, R]-shaped rank-major image of the factor, N = K; up: [N, R]
            fresh = []
            for fill in (0x00, 0xFF):
                out = torch.full((img.numel(),), fill, dtype=torch.uint8, device=p.device)
                fn = lib.svdq_pack_lora_down if down else lib.svdq_pack_lora_up
                _lib.check(fn(p.data_ptr(), out.data_ptr(), N, R, _C._DT[p.dtype], torch.cuda.current_stream().cuda_stream), kind)
                fresh.append(out)
            torch.cuda.synchronize()
            written = fresh[0] == fresh[1]
            checked += 1
            if not torch.equal(img[written], fresh[0][written]):
                stale.append(name)
    return checked, stale


# ---------------------------------------------------------------------------------------------------------------------
# Constructed attention inputs (tests/test_oracle_attention.py on the CPU, tests/test_gpu_attention_edges.py on the GPU): score profiles whose
# exact softmax is known from the inputs alone.  Everything is numpy: [L, H, 128] float32 carriers of 16-bit values.
# ---------------------------------------------------------------------------------------------------------------------
ATT_KB = 64                                               # keys per tile of svdq_attention
ATT_C = (1.0 / np.sqrt(128.0)) * 1.4426950408889634       # ops.attention.q_prescale(128): raw score units -> log2 units
ULP16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}           # half a unit in the last place, relative (the attention tests' "ulp")


def attn_prescaled(q: np.ndarray, dtype: str) -> np.ndarray:
    """The Q a producer hands to geometry 2: q * scale * log2(e), rounded once (tests/test_gpu_attention.py: _as_produced_for)."""
    with np.errstate(invalid="ignore"):
        return O.round16(q.astype(np.float32) * np.float32(ATT_C), dtype)


def attn_real_keys(L: int, valid=None) -> np.ndarray:
    """bool [L]: the real rows of a buffer padded as ``kv_valid`` says ((n,) or (n0, start1, end1); None: all)."""
    real = np.ones(L, dtype=bool)
    if valid is not None:
        real[:] = False
        real[: valid[0]] = True
        if len(valid) == 3:
            real[valid[1]:valid[2]] = True
    return real


def attn_values(L: int, H: int, v_amp: float, seed: int) -> np.ndarray:
    """V[j, h, d] = +-(1 + n / 128) * v_amp, n in 0 .. 127: eight significant bits, exact in bf16 and fp16; sums of them are exact in fp32."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 128, (L, H, 128))
    sign = rng.integers(0, 2, (L, H, 128)) * 2 - 1
    return (sign * (1.0 + n / 128.0) * v_amp).astype(np.float32)


def attn_winners(L: int, H: int, placement: str, segments=None, targets=None, real=None) -> np.ndarray:
    """pi [L, H]: the key each query row selects (-1: a padded row).  With b = l // 32 the row's 32-row block and r = l % 32:
    ``scattered``: tile (r + b) mod ntiles at a varying position -- every block has winners in every tile;
    ``block``: every row of block b in tile b mod ntiles;
    ``segments``: ``segments`` = the records of svdq_attention_schedule; rows of a split task win in the first and the last tile of each of its
    segments (neighbouring rows in different segments), rows of whole tasks as ``scattered``;
    ``targets``: ``targets`` = a list of tiles, ``real`` = bool [L]: real rows cycle through the tiles' real keys."""
    nt = L // ATT_KB
    l = np.arange(L)[:, None]
    h = np.arange(H)[None, :]
    b, r = l // 32, l % 32
    pos = (5 * r + 3 * b + 7 * h + 1) % ATT_KB
    if placement == "scattered":
        return ((r + b) % nt) * ATT_KB + pos + 0 * h
    if placement == "block":
        return (b % nt) * ATT_KB + (5 * l + 7 * h) % ATT_KB
    if placement == "segments":
        pi = ((r + b) % nt) * ATT_KB + pos + 0 * h
        by_task = {}
        for _, task, j0, j1, _, _ in np.asarray(segments).reshape(-1, 6):
            if j0 > 0 or j1 < nt:
                by_task.setdefault(int(task), set()).update((int(j0), int(j1) - 1))
        for task, edge in by_task.items():
            head, qt = divmod(task, L // 256)
            edge = np.array(sorted(edge))
            rows = np.arange(qt * 256, qt * 256 + 256)
            pi[rows, head] = edge[(rows % 32 + rows // 32) % len(edge)] * ATT_KB + pos[rows, head]
        return pi
    if placement == "targets":
        pi = np.full((L, H), -1, dtype=np.int64)
        keys = [np.flatnonzero(real[t * ATT_KB:(t + 1) * ATT_KB]) + t * ATT_KB for t in targets]
        assert all(len(k) for k in keys)
        for row in np.flatnonzero(real):
            for head in range(H):
                k = keys[(row % 32 + row // 32) % len(keys)]
                pi[row, head] = k[((row // len(keys) + head) % 4) * len(k) // 4]  # four spread positions per tile: few enough winners for a decoy each
        return pi
    raise ValueError(placement)


def attn_onehot(L: int, H: int, dtype: str, a: float, v_amp: float, pi: np.ndarray, seed: int, real=None, padded_k="decoy"):
    """K[j] in {+-1}^128, Q[l] = a K[pi(l)], V = attn_values: score(l, pi(l)) = 128 a exactly, every other real key far below.  With ``real``
    (bool [L]) the padded K rows are decoys -- 3 K[w] for winners w, which would beat every real key if they counted -- or NaN
    (``padded_k="nan"``), the padded V rows large and finite, the padded Q rows copies of real ones.  -> q, k, v [L, H, 128] float32, exact in ``dtype``."""
    rng = np.random.default_rng(seed)
    k = (rng.integers(0, 2, (L, H, 128)) * 2 - 1).astype(np.float32)
    v = attn_values(L, H, v_amp, seed + 1)
    real = np.ones(L, dtype=bool) if real is None else real
    pi = np.where(pi < 0, pi[np.flatnonzero(real)[0]][None, :], pi)            # padded query rows: the first real row's winners
    q = np.float32(a) * np.take_along_axis(k, pi[:, :, None], axis=0)
    if not real.all():
        pad = np.flatnonzero(~real)
        for head in range(H):
            w = np.unique(pi[real, head])
            k[pad, head] = 3.0 * k[w[np.arange(len(pad)) % len(w)], head] if padded_k == "decoy" else np.nan
        big = 1000.0 * v_amp if 1000.0 * v_amp < 60000.0 else 49152.0
        v[pad] = np.sign(v[pad]) * np.float32(big)
    for t in (q, v):
        assert np.array_equal(O.round16(t, dtype), t)
    return q, k, v


def attn_twin_pairs(L: int, real=None, targets=None):
    """Key pairs (j1, j2) in different tiles -- half the tile list apart, which on the persistent schedules also means different segments --
    for attn_two_winners.  ``targets``: the tiles to use (default: all), ``real``: bool [L]."""
    real = np.ones(L, dtype=bool) if real is None else real
    tiles = list(range(L // ATT_KB)) if targets is None else list(targets)
    keys = [np.flatnonzero(real[t * ATT_KB:(t + 1) * ATT_KB]) + t * ATT_KB for t in tiles]
    n = len(tiles)
    return [(int(keys[i][len(keys[i]) // 3]), int(keys[(i + max(1, n // 2)) % n][2 * len(keys[(i + max(1, n // 2)) % n]) // 3])) for i in range(n)]


def attn_two_winners(L: int, H: int, dtype: str, a: float, pairs, seed: int, real=None, padded_k="decoy"):
    """As attn_onehot with TWO identical key rows per query row: K[j2] = K[j1] for each pair, row l selects pair (l % 32 + l // 32) mod len(pairs).
    Both probabilities are exp2(0), l = 2 and the exact answer is (V[j1] + V[j2]) / 2.  -> q, k, v, j1 [L], j2 [L]"""
    pairs = np.asarray(pairs)
    rows = np.arange(L)
    sel = pairs[(rows % 32 + rows // 32) % len(pairs)]
    real = np.ones(L, dtype=bool) if real is None else real
    pi = np.where(real[:, None], np.repeat(sel[:, :1], H, axis=1), -1)
    rng = np.random.default_rng(seed)
    k = (rng.integers(0, 2, (L, H, 128)) * 2 - 1).astype(np.float32)
    k[pairs[:, 1]] = k[pairs[:, 0]]
    v = attn_values(L, H, 1.0, seed + 1)
    v[pairs[:, 1]] = np.abs(v[pairs[:, 1]]) * np.sign(v[pairs[:, 0]])          # no cancellation: |V1 + V2| / 2 >= min|V|, as the precondition assumes
    pi = np.where(pi < 0, pi[np.flatnonzero(real)[0]][None, :], pi)
    q = np.float32(a) * np.take_along_axis(k, pi[:, :, None], axis=0)
    if not real.all():
        pad = np.flatnonzero(~real)
        k[pad] = 3.0 * k[pairs[np.arange(len(pad)) % len(pairs), 0]] if padded_k == "decoy" else np.nan
        v[pad] = np.sign(v[pad]) * np.float32(1000.0)
    return q, k, v, sel[:, 0], sel[:, 1]


def attn_scores_log2(q: np.ndarray, k: np.ndarray, c: float) -> np.ndarray:
    """float64 scores [H, L, L] in log2 units (``c``: ATT_C for a raw Q, 1 for a prescaled one)"""
    with np.errstate(invalid="ignore"):
        return np.matmul(np.ascontiguousarray(q.transpose(1, 0, 2), dtype=np.float64), np.ascontiguousarray(k.transpose(1, 2, 0), dtype=np.float64)) * c


def attn_selection_margin(q, k, v, c, dtype, winners, real=None) -> float:
    """The precondition of the exact tests, from the inputs alone in float64: per query row the total weight of the real keys that are NOT its
    winners, relative to a winner's, times max|V| -- as a fraction of 2^-6 * (half a 16-bit ulp of min|V|).  Below 1 the exact answer (the winner's
    value, or the mean of the winners' values) cannot depend on any rounding.  ``winners``: a list of int arrays [L, H] or [L]."""
    L, H = q.shape[:2]
    real = np.ones(L, dtype=bool) if real is None else real
    s = attn_scores_log2(q[real], k[real], c)                                     # [H, rows, keys]
    col = np.cumsum(real) - 1                                                     # key index -> column among the real keys
    other = np.ones(s.shape, dtype=bool)
    win = None
    for w in winners:
        w = np.broadcast_to(w.reshape(L, -1), (L, H))[real].T[:, :, None]        # [H, rows, 1]
        np.put_along_axis(other, col[w], False, axis=2)
        sw = np.take_along_axis(s, col[w], axis=2)
        assert win is None or np.array_equal(sw, win), "the winners of a row must tie exactly"
        win = sw
    with np.errstate(over="ignore"):
        leak = np.where(other, np.exp2(s - win), 0.0).sum(axis=2).max()
    vr = np.abs(v[real].astype(np.float64))
    return float(leak * vr.max() / (2.0 ** -6 * ULP16[dtype] * vr.min()))


def ulp16_of(x: np.ndarray, dtype: str) -> np.ndarray:
    """the spacing of the 16-bit format at |x| (fp16: subnormal spacing below 2^-14)"""
    mant, emin = (7, -126) if dtype == "bf16" else (10, -14)
    e = np.floor(np.log2(np.maximum(np.abs(x.astype(np.float64)), 2.0 ** emin)))
    return 2.0 ** (e - mant)


ATTN_PROFILES = {  # section "controlled growth": the level of key tile t, in log2 units for a query row of slope 1
    "rise-7.5": lambda t, nt: 7.5 * t, "rise-8": lambda t, nt: 8.0 * t, "rise-8.125": lambda t, nt: 8.125 * t, "rise-20": lambda t, nt: 20.0 * t,
    "rise-200": lambda t, nt: 200.0 * t, "fall-3": lambda t, nt: -3.0 * t, "fall-7.5": lambda t, nt: -7.5 * t, "fall-30": lambda t, nt: -30.0 * t,
    "spike-last": lambda t, nt: 40.0 * (t == nt - 1), "spike-second": lambda t, nt: 40.0 * (t == 1),
    "zigzag": lambda t, nt: (0.0, 12.0, -5.0, 30.0, 2.0, 31.0, -40.0, 39.5)[t % 8],
}
ATTN_SLOPES = (-2.0, -1.0, 0.0, 0.25, 0.5, 1.0, 2.0, 4.0)


def attn_rank1(L: int, H: int, dtype: str, profile, seed: int, spike_tile=None):
    """Rank-1 scores: only channel 0 of Q and K is non-zero, Q[l, 0] = a_l drawn from ATTN_SLOPES (one 32-row block mixes rising, falling and flat
    rows), K[j, 0] = b_j = the profile's level of tile j // 64 plus a multiple of 1/8 in [0, 1); V = randn.  All rounded to ``dtype``.  The Q is
    meant to be read in log2 units: softmax scale ln 2, or q_prescaled (it then IS the producer's Q / q_prescale, times q_prescale, rounded once).
    ``profile``: a name of ATTN_PROFILES; ``spike_tile``: aim the profile's "last tile" at this tile instead.  -> q, k, v [L, H, 128] float32"""
    rng = np.random.default_rng(seed)
    nt = L // ATT_KB
    fn = ATTN_PROFILES[profile]
    level = np.array([float(fn(t, nt)) for t in range(nt)])
    if spike_tile is not None:
        level[[spike_tile, nt - 1]] = level[[nt - 1, spike_tile]]
    q = np.zeros((L, H, 128), dtype=np.float32)
    k = np.zeros((L, H, 128), dtype=np.float32)
    q[:, :, 0] = rng.choice(np.array(ATTN_SLOPES, dtype=np.float32), (L, H))
    k[:, :, 0] = np.repeat(level, ATT_KB)[:, None] + rng.integers(0, 8, (L, H)) / 8.0
    v = rng.standard_normal((L, H, 128)).astype(np.float32)
    return O.round16(q, dtype), O.round16(k, dtype), O.round16(v, dtype)


def attn_softmax64(q, k, v, c, real=None):
    """float64 softmax attention of one head over the given 16-bit values, scores q . k * c in log2 units, real keys only.
    -> (sum_j p_j v_j, sum_j p_j |v_j|), both [L, 128]"""
    s = q.astype(np.float64) @ k.astype(np.float64).T * c
    if real is not None:
        s[:, ~real] = -np.inf
    p = np.exp2(s - s.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    v64 = np.where(np.isfinite(v), v, 0.0).astype(np.float64) if real is not None else v.astype(np.float64)
    return p @ v64, p @ np.abs(v64)


# the shape / mode grid of the constructed attention tests: (L, H) on the plain grid, (L, H) on the persistent schedule, (L, kv_valid) masked (H = 3)
ATTN_PLAIN = [(128, 1), (256, 2), (1152, 2)]
ATTN_PERSISTENT = [(256, 3), (1024, 3)]
ATTN_MASKED = [(512, (300, 384, 500)), (768, (700,)), (1024, (37, 256, 1000))]
ATTN_MASKED_H = 3


def attn_schedule(L: int, H: int, cus: int = 256) -> np.ndarray:
    """The records of svdq_attention_schedule [n, 6]: {workgroup, task, first tile, end tile, owner, last contributor} (host only)."""
    import ctypes as C

    from nunchaku_amd import _lib

    lib = _lib.load()
    n = lib.svdq_attention_schedule(L, H, cus, None, 0)
    assert n > 0, (L, H, "runs on the plain grid")
    buf = (C.c_int32 * (6 * n))()
    assert lib.svdq_attention_schedule(L, H, cus, buf, n) == n
    return np.ctypeslib.as_array(buf).reshape(n, 6).copy()


def attn_mask_targets(L: int, H: int, valid):
    """For a masked launch: (main segment [j0, j1) of svdq_attention_plan for a prescaled Q, the tiles a constructed test aims at: the main segment's
    first and last tile, then every "extra" tile -- the tiles outside the main segment that hold a real key, partially padded ones included)."""
    import ctypes as C

    from nunchaku_amd import _lib

    a = _lib.AttentionArgs()
    a.L, a.H, a.head_dim, a.q_prescaled, a.kv_len0 = L, H, 128, 1, valid[0]
    if len(valid) == 3:
        a.kv_start1, a.kv_end1 = valid[1], valid[2]
    plan = (C.c_int32 * 4)()
    assert _lib.load().svdq_attention_plan(C.byref(a), plan) == 0
    assert plan[0] == 2 and plan[1] == 1 and plan[3] - plan[2] >= 2, list(plan)
    real = attn_real_keys(L, valid)
    extra = [t for t in range(L // ATT_KB) if not plan[2] <= t < plan[3] and real[t * ATT_KB:(t + 1) * ATT_KB].any()]
    return (plan[2], plan[3]), [plan[2], plan[3] - 1] + extra


def attn_uniform(L: int, H: int, dtype: str, seed: int, real=None):
    """Q = 0, K = randn (NaN in the padded rows), V = attn_values (+-1000 in the padded rows): every real key has probability exactly 1 / (number
    of real keys).  -> q, k, v [L, H, 128] float32 and round16 of the float64 mean of the real V rows [H, 128]"""
    rng = np.random.default_rng(seed)
    real = np.ones(L, dtype=bool) if real is None else real
    k = O.round16(rng.standard_normal((L, H, 128)).astype(np.float32), dtype)
    v = attn_values(L, H, 1.0, seed + 1)
    k[~real] = np.nan
    v[~real] = np.sign(v[~real]) * np.float32(1000.0)
    return np.zeros((L, H, 128), dtype=np.float32), k, v, O.round16(v[real].astype(np.float64).mean(axis=0), dtype)
