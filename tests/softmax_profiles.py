"""Constructed score profiles for the attention kernels that walk their keys in 64-key chunks with an online softmax (svdq_attention_d64,
svdq_cross_attention): inputs whose exact softmax follows from the inputs alone, a float64 reference, a restatement of the kernels' order of
operations, and the assertions that tests/test_gpu_softmax_profiles.py makes on the GPU and tests/test_softmax_profiles.py makes on the
restatement (and on deliberately broken copies of it).  CPU only, torch, generic in (T, N, H, D, dtype).

Everything works per SAMPLE on [rows, H*D] tensors of 16-bit values: q [T, H*D], k / v [N, H*D], head h in columns h*D .. (h+1)*D.  A
``launch`` is any callable (samples, H, D, scale, dtype) -> list of [T, H*D] 16-bit tensors, samples = a list of (q, k, v) with one T; the GPU
file stacks the samples into the layouts the ops take, the CPU file answers with the restatement.

The construction of values / onehot / two_winners / uniform / rank1 / selection_margin is that of tests/helpers.py (attn_*), which is hard-wired
to [L, H, 128], square problems and svdq_attention's plans."""

import math

import torch

LOG2E = 1.4426950408889634
ULP16 = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # unit roundoff: half a unit in the last place, relative
SUB16 = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -25}        # half the subnormal spacing of a rounded probability
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
CHUNK = 64
BAR = 3.0

# the shapes of the GPU file, as (T, H, D, [N of every sample of the launch])
D64_CASES = [(130, 2, 64, [200, 200]), (96, 3, 64, [520]), (40, 1, 64, [65, 65]), (33, 2, 64, [77]), (64, 1, 64, [128]),
             (130, 2, 64, [130])]  # the last one: T == N, the shape that can also be read from one packed [B, S, 3*H*64] buffer
XATTN_CASES = [(260, 2, 112, [300, 65]), (260, 2, 72, [320, 1]), (40, 1, 128, [128])]
SCALES = (0.03, 0.2, 1.0)


def case_id(case):
    T, H, D, Ns = case
    return f"T{T}-H{H}-D{D}-N" + "_".join(map(str, Ns))


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def spacing16(x, dtype):
    """the spacing of the 16-bit format at |x| (float64 in, float64 out; the subnormal spacing below the smallest normal number)"""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.frexp(x.double().abs().clamp_min(2.0 ** emin))[1] - 1
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - mant)


def round16(x, dtype):
    """float64 -> the nearest value of ``dtype``, rounded ONCE (a cast by way of float32 rounds twice: its result is checked against the neighbour
    on the side of x).  -> a tensor of ``dtype``"""
    x = x.double()
    r = x.float().to(dtype)
    rd = r.double()
    other = rd + torch.sign(x - rd) * spacing16(rd, dtype)
    closer = ((x - other).abs() < (x - rd).abs()) & torch.isfinite(other.float().to(dtype).double())
    return torch.where(closer, other, rd).float().to(dtype)


# ---- builders ---------------------------------------------------------------------------------------------------------------------------
def values(N, H, D, amp, seed):
    """V[j, h*D + d] = +-(1 + n / 128) * amp, n in 0 .. 127: eight significant bits, exact in bf16 and fp16; fp32 sums of them are exact.
    -> float32 [N, H*D]"""
    g = _gen(seed)
    n = torch.randint(0, 128, (N, H * D), generator=g)
    sign = torch.randint(0, 2, (N, H * D), generator=g) * 2 - 1
    return (sign * (1.0 + n / 128.0) * amp).float()


def _signs(N, H, D, seed):
    return (torch.randint(0, 2, (N, H * D), generator=_gen(seed)) * 2 - 1).float()


def _gather_rows(x, idx, H, D):
    """x [N, H*D], idx [T, H] -> [T, H*D]: row idx[t, h] of head h"""
    return torch.gather(x.view(-1, H, D), 0, idx[:, :, None].expand(-1, -1, D)).reshape(idx.shape[0], H * D)


def onehot(T, N, H, D, dtype, a, shift, seed, v_amp=1.0, stride=1):
    """K in {+-1}^D per head, row t of head h selects key (stride t + 7 h + shift) mod N, Q = a K[winner], V = values: the winner's score is
    a * D (times the scale), every other far below.  Walking ``shift`` over range(0, N, T) at stride 1 selects every key position; stride 67
    puts the winners of neighbouring rows of a wave into different chunks.  -> q, k, v, winner [T, H]"""
    k = _signs(N, H, D, seed)
    v = values(N, H, D, v_amp, seed + 1)
    win = (stride * torch.arange(T)[:, None] + 7 * torch.arange(H)[None, :] + shift) % N
    q = a * _gather_rows(k, win, H, D)
    for t in (q, v):
        assert torch.equal(t.to(dtype).float(), t)
    return q.to(dtype), k.to(dtype), v.to(dtype), win


def twin_pairs(N, chunk=CHUNK):
    """Disjoint key pairs (j1, j2) in different chunks: from every chunk to the next one (an odd distance: the other buffer of a double-buffered
    stage) and to the one half the chunk list further, at varying positions; a chunk whose keys are used up (a ragged chunk of one) gives no more."""
    nt = (N + chunk - 1) // chunk
    assert nt >= 2, "two winners in different chunks need more than one chunk"
    used, pairs = set(), []

    def free(c, want):
        lo, hi = c * chunk, min(N, (c + 1) * chunk)
        return next((lo + (want + o) % (hi - lo) for o in range(hi - lo) if lo + (want + o) % (hi - lo) not in used), None)

    for i in range(nt):
        for d in sorted({1, max(1, nt // 2)}):
            c2 = (i + d) % nt
            j1, j2 = free(i, 13 * len(pairs) + 5), free(c2, 29 * len(pairs) + 47)
            if c2 == i or j1 is None or j2 is None:
                continue
            used.update((j1, j2))
            pairs.append((j1, j2))
    assert any((j1 // chunk - j2 // chunk) % 2 == 1 for j1, j2 in pairs)
    return pairs


def two_winners(T, N, H, D, dtype, a, seed):
    """As onehot with TWO identical key rows per query row, in different chunks: K[j2] = K[j1] for every pair of twin_pairs, row t of head h
    selects pair (t + 3 h) mod len(pairs); the twins' V values have equal sign per channel (no cancellation).  Both probabilities are exp2(0),
    l = 2, and the exact answer is round16((V[j1] + V[j2]) / 2).  -> q, k, v, j1 [T, H], j2 [T, H]"""
    pairs = torch.tensor(twin_pairs(N))
    k = _signs(N, H, D, seed)
    k[pairs[:, 1]] = k[pairs[:, 0]]
    v = values(N, H, D, 1.0, seed + 1)
    v[pairs[:, 1]] = v[pairs[:, 1]].abs() * torch.sign(v[pairs[:, 0]])
    sel = pairs[(torch.arange(T)[:, None] + 3 * torch.arange(H)[None, :]) % len(pairs)]   # [T, H, 2]
    q = a * _gather_rows(k, sel[..., 0], H, D)
    return q.to(dtype), k.to(dtype), v.to(dtype), sel[..., 0], sel[..., 1]


def uniform(T, N, H, D, dtype, seed):
    """Q = 0, K = randn, V = values: every key has probability exactly 1 / N.  -> q, k, v and round16 of the float64 mean of the N rows [H*D]"""
    k = torch.randn(N, H * D, generator=_gen(seed)).to(dtype)
    v = values(N, H, D, 1.0, seed + 1)
    return torch.zeros(T, H * D, dtype=dtype), k, v.to(dtype), round16(v.double().mean(dim=0), dtype)


PROFILES = {  # the level of key chunk t of nt, in log2 units for a query row of slope 1 (tests/helpers.py: ATTN_PROFILES)
    "rise-7.5": lambda t, nt: 7.5 * t, "rise-8": lambda t, nt: 8.0 * t, "rise-8.125": lambda t, nt: 8.125 * t, "rise-20": lambda t, nt: 20.0 * t,
    "rise-200": lambda t, nt: 200.0 * t, "fall-3": lambda t, nt: -3.0 * t, "fall-7.5": lambda t, nt: -7.5 * t, "fall-30": lambda t, nt: -30.0 * t,
    "spike-last": lambda t, nt: 40.0 * (t == nt - 1), "spike-second": lambda t, nt: 40.0 * (t == 1),
    "zigzag": lambda t, nt: (0.0, 12.0, -5.0, 30.0, 2.0, 31.0, -40.0, 39.5)[t % 8],
}
SLOPES = (-2.0, -1.0, 0.0, 0.25, 0.5, 1.0, 2.0, 4.0)


def rank1(T, N, H, D, dtype, profile, seed):
    """Rank-1 scores: only channel 0 of every head of Q and K is non-zero, Q[t, 0] drawn from SLOPES (one 32-row wave mixes rising, falling and
    flat rows), K[j, 0] = the profile's level of chunk j // 64 plus m / 8, m in 0 .. 7; V = randn.  All rounded to ``dtype``.  Meant for
    scale = ln 2: the levels are then in log2 units.  -> q, k, v"""
    g = _gen(seed)
    nt = (N + CHUNK - 1) // CHUNK
    level = torch.tensor([float(PROFILES[profile](t, nt)) for t in range(nt)]).repeat_interleave(CHUNK)[:N]
    q = torch.zeros(T, H, D)
    k = torch.zeros(N, H, D)
    q[:, :, 0] = torch.tensor(SLOPES)[torch.randint(0, len(SLOPES), (T, H), generator=g)]
    k[:, :, 0] = level[:, None] + torch.randint(0, 8, (N, H), generator=g) / 8.0
    v = torch.randn(N, H * D, generator=g)
    return q.view(T, H * D).to(dtype), k.view(N, H * D).to(dtype), v.to(dtype)


def two_level_deltas(dtype):
    """the score gaps d = m / 8 (log2 units) whose probability 2^-d moves by 0.3 .. 0.8 of half a spacing when it is rounded to ``dtype``: far
    from representable, and far from a tie"""
    keep = []
    for m in range(1, 33):
        p = torch.tensor(2.0 ** (-m / 8.0), dtype=torch.float64)
        err = (round16(p, dtype).double() - p).abs().item() / (0.5 * spacing16(p, dtype).item())
        if 0.3 <= err <= 0.8:
            keep.append(m / 8.0)
    return keep


def two_level(T, N, H, D, dtype, seed):
    """Rows whose answer depends on the ROUNDED probabilities: one anchor key per chunk scores 0, every other key -d_t (log2 units at scale ln 2;
    d_t cycles through two_level_deltas), V = |values|.  The running maximum is 0 from the first chunk on (alpha = 1), the anchors have
    probability 1 and the others r_t = round16(2^-d_t), so that out = (sum_anchors v + r_t sum_others v) / (A + r_t (N - A)): with r_t, not
    with 2^-d_t -- a row sum over the unrounded probabilities moves every channel by 0.15 .. 0.4 of a 16-bit spacing.
    -> q, k, v, the float64 answer [T, H*D]"""
    deltas = torch.tensor(two_level_deltas(dtype), dtype=torch.float64)
    assert len(deltas) >= 4
    nt = (N + CHUNK - 1) // CHUNK
    anchor = torch.zeros(N, dtype=torch.bool)
    for c in range(nt):
        lo, hi = c * CHUNK, min(N, (c + 1) * CHUNK)
        anchor[lo + (17 * c + 3) % (hi - lo)] = True
    d = deltas[(torch.arange(T)[:, None] + 5 * torch.arange(H)[None, :]) % len(deltas)]       # [T, H]
    q = torch.zeros(T, H, D)
    k = torch.zeros(N, H, D)
    q[:, :, 0] = d.float()
    k[:, :, 0] = torch.where(anchor, 0.0, -1.0)[:, None]
    v = values(N, H, D, 1.0, seed).abs()
    r = round16(torch.exp2(-d), dtype).double()                                               # [T, H]
    va, vo = v[anchor].double().sum(0).view(H, D), v[~anchor].double().sum(0).view(H, D)
    A = int(anchor.sum())
    want = (va[None] + r[:, :, None] * vo[None]) / (A + r * (N - A))[:, :, None]
    assert torch.equal(q.to(dtype).float(), q)
    return q.view(T, H * D).to(dtype), k.view(N, H * D).to(dtype), v.to(dtype), want.reshape(T, H * D)


# ---- references -------------------------------------------------------------------------------------------------------------------------
def _heads(x, H, D, dt):
    return x.to(dt).view(x.shape[0], H, D).transpose(0, 1)                                    # [H, rows, D]


def softmax64(q, k, v, H, D, scale):
    """float64 softmax attention over the given 16-bit values.  -> sum_j p_j v_j, sum_j p_j |v_j| and sum_j |v_j| / l with
    l = sum_j exp(s_j - max s), each [T, H*D] float64"""
    T = q.shape[0]
    s = (_heads(q, H, D, torch.float64) @ _heads(k, H, D, torch.float64).transpose(1, 2)) * float(scale)
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    l = e.sum(dim=-1, keepdim=True)
    vh = _heads(v, H, D, torch.float64)
    flat = lambda x: x.transpose(0, 1).reshape(T, H * D)
    return flat((e / l) @ vh), flat((e / l) @ vh.abs()), flat(vh.abs().sum(dim=1, keepdim=True) / l)


def selection_margin(q, k, v, H, D, scale, dtype, winners):
    """The precondition of the bit-exact tests, in float64 from the inputs alone: per query row the weight of all keys that are NOT its winners,
    relative to a winner's, times max|V| -- as a fraction of 2^-6 * ulp16 * min|V|.  Below 1 the exact answer (the winner's value, or the mean
    of the tied winners' values) cannot depend on any rounding.  ``winners``: a list of [T, H] key indices; they must tie exactly."""
    scale = D ** -0.5 if scale is None else scale
    s = (_heads(q, H, D, torch.float64) @ _heads(k, H, D, torch.float64).transpose(1, 2)) * float(scale)   # [H, T, N]
    other = torch.ones_like(s, dtype=torch.bool)
    win = None
    for w in winners:
        idx = w.t()[:, :, None]
        other.scatter_(2, idx, False)
        sw = s.gather(2, idx)
        assert win is None or torch.equal(sw, win), "the winners of a row must tie exactly"
        win = sw
    leak = torch.where(other, torch.exp(s - win), torch.zeros_like(s)).sum(dim=2).max().item()
    va = v.double().abs()
    return leak * va.max().item() / (2.0 ** -6 * ULP16[dtype] * va.min().item())


MUTANTS = ("alpha-not-on-l", "last-key-dropped", "key-beyond-n-counted", "stale-v-buffer", "v-keys-swapped", "scale-ignored", "sum-unrounded")


def chunked_softmax_ref(q, k, v, H, D, scale=None, dtype=torch.bfloat16, chunk=CHUNK, mutate=None):
    """The kernels' own order of operations in fp32 on the CPU, for any head dimension: ``chunk``-key chunks from the sample's first key, online
    softmax with exp2 and c = float32(scale) * float32(log2 e), the exponent formed as fma(s, c, -(m c)), P rounded to ``dtype`` before it
    meets V, the row sum over the rounded values, the normalisation by o * (1.0f / l) last.  q [T, H*D], k / v [N, H*D] -> [T, H*D] fp32
    (before the final rounding).  What this differs from the kernels in: the order of the fp32 additions inside a matrix product, and exp2's
    last bit.  ``mutate``: one of MUTANTS, a deliberate error (tests/test_softmax_profiles.py: the assertions must catch each)."""
    assert mutate is None or mutate in MUTANTS, mutate
    T, N = q.shape[0], k.shape[0]
    if scale is None or mutate == "scale-ignored":
        scale = D ** -0.5
    c = torch.tensor(float(scale), dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    qh, kh, vh = (_heads(t, H, D, torch.float32) for t in (q, k, v))
    m = torch.full((H, T, 1), float("-inf"))
    l = torch.zeros(H, T, 1)
    o = torch.zeros(H, T, D)
    for ch, n0 in enumerate(range(0, N, chunk)):
        n1 = min(N, n0 + chunk)
        ragged = n1 - n0 < chunk
        vc = vh[:, n0:n1]
        if mutate == "stale-v-buffer" and ch >= 2:          # chunk c's V from chunk c - 2: the same buffer, not yet overwritten
            vc = vh[:, n0 - 2 * chunk:n1 - 2 * chunk]
        if mutate == "v-keys-swapped" and n1 - n0 > 8:      # keys 4 and 8 of a chunk swapped in V only: a wrong transposition order
            vc = vc.clone()
            vc[:, [4, 8]] = vc[:, [8, 4]]
        s = qh @ kh[:, n0:n1].transpose(1, 2)
        if mutate == "last-key-dropped" and ragged:
            s[:, :, -1] = float("-inf")
        if mutate == "key-beyond-n-counted" and ragged:     # the zero image of key N: score 0, V = 0
            s = torch.cat([s, torch.zeros(H, T, 1)], dim=2)
            vc = torch.cat([vc, torch.zeros(H, 1, D)], dim=1)
        m_new = torch.maximum(m, s.amax(dim=-1, keepdim=True))
        alpha = torch.exp2((m - m_new) * c)
        nmc = -(m_new * c)
        e = torch.exp2((s.double() * c.double() + nmc.double()).float())   # (the product of two fp32 values is exact in float64: an fma)
        p = e.to(dtype).float()
        lsum = (e if mutate == "sum-unrounded" else p).sum(dim=-1, keepdim=True)
        l = (l if mutate == "alpha-not-on-l" and ch == 1 else l * alpha) + lsum
        o = o * alpha + p @ vc
        m = m_new
    return (o * (1.0 / l)).transpose(0, 1).reshape(T, H * D)


def restatement_launch(mutate=None):
    """a ``launch`` that answers with chunked_softmax_ref, rounded once to ``dtype``"""
    def launch(samples, H, D, scale, dtype):
        return [chunked_softmax_ref(q, k, v, H, D, scale, dtype, mutate=mutate).to(dtype) for q, k, v in samples]
    return launch


# ---- the assertions (one function per section of the GPU file; each asserts its preconditions on its own inputs before it launches) ----
def _first_wrong(out, want, H, D, b, keys=()):
    bad = (out != want).view(-1, H, D).any(dim=2).nonzero()
    t, h = bad[0].tolist()
    d = int((out.view(-1, H, D)[t, h] != want.view(-1, H, D)[t, h]).nonzero()[0])
    where = ", ".join(f"winner key {int(w[t, h])} = chunk {int(w[t, h]) // CHUNK} position {int(w[t, h]) % CHUNK}" for w in keys)
    return (f"{len(bad)} (row, head) pairs differ; first: sample {b} row {t} (tile {t // 128} wave {t % 128 // 32} lane {t % 32}) head {h} "
            f"channel {d}: out {out.view(-1, H, D)[t, h, d].item()!r}, exact {want.view(-1, H, D)[t, h, d].item()!r}; {where}")


def check_onehot(launch, case, dtype):
    """(a) out == V[winner] bit for bit, at every key position; a = 16, and a = 2048 with v_amp = 2^14; and once with the winners of
    neighbouring rows 67 keys apart: in different chunks"""
    T, H, D, Ns = case
    covered = [torch.zeros(N, dtype=torch.bool) for N in Ns]
    worst = 0.0
    for a, v_amp, stride in ((16.0, 1.0, 1), (2048.0, 2.0 ** 14, 1), (16.0, 1.0, 67)):
        for shift in (range(0, max(Ns), T) if stride == 1 else (11,)):
            built = [onehot(T, N, H, D, dtype, a, shift, 100 * b + N + D, v_amp, stride) for b, N in enumerate(Ns)]
            for b, (q, k, v, win) in enumerate(built):
                margin = selection_margin(q, k, v, H, D, None, dtype, [win]) if Ns[b] > 1 else 0.0
                assert margin < 1.0, f"[onehot] a={a} shift={shift} sample {b}: selection margin {margin:.3g}: the precondition does not hold"
                worst = max(worst, margin)
                covered[b][win.flatten()] = True
            outs = launch([x[:3] for x in built], H, D, None, dtype)
            for b, (out, (q, k, v, win)) in enumerate(zip(outs, built)):
                want = _gather_rows(v, win, H, D)
                assert torch.equal(out, want), f"[onehot] a={a} v_amp={v_amp} shift={shift} stride={stride}: " + _first_wrong(out, want, H, D, b, [win])
    assert all(c.all() for c in covered), "[onehot] the shifts do not select every key position"
    return worst


def check_two_winners(launch, case, dtype):
    """(b) out == round16 of the float64 mean of the two tied rows, bit for bit.  A sample of one chunk has no two chunks: it runs a one-hot row."""
    T, H, D, Ns = case
    built = []
    for b, N in enumerate(Ns):
        if N > CHUNK:
            q, k, v, j1, j2 = two_winners(T, N, H, D, dtype, 16.0, 300 * b + N + D)
            built.append((q, k, v, [j1, j2]))
        else:
            q, k, v, win = onehot(T, N, H, D, dtype, 16.0, 0, 300 * b + N + D)
            built.append((q, k, v, [win]))
        if N > 1:
            margin = selection_margin(q, k, v, H, D, None, dtype, built[-1][3])      # (also asserts that the winners tie exactly)
            assert margin < 1.0, f"[two-winners] sample {b}: selection margin {margin:.3g}: the precondition does not hold"
    outs = launch([x[:3] for x in built], H, D, None, dtype)
    for b, (out, (q, k, v, wins)) in enumerate(zip(outs, built)):
        want = round16(sum(_gather_rows(v, w, H, D).double() for w in wins) / len(wins), dtype)
        assert torch.equal(out, want), "[two-winners] " + _first_wrong(out, want, H, D, b, wins)


def uniform_sensitivity(v, H, D, dtype):
    """for uniform inputs: the smallest, over the keys and heads, of the largest move over a head's channels (in 16-bit spacings of the mean) when
    one key is removed or counted twice"""
    N = v.shape[0]
    v64 = v.double()
    total = v64.sum(dim=0, keepdim=True)
    mean = total / N
    sp = spacing16(mean, dtype)
    worst = float("inf")
    for moved in ((total - v64) / max(N - 1, 1), (total + v64) / (N + 1)):
        move = ((moved - mean).abs() / sp).view(N, H, D).amax(dim=2)
        worst = min(worst, move.min().item())
    return worst


def check_uniform(launch, case, dtype):
    """(c) Q = 0: out is round16 of the float64 mean (N a power of two: bit for bit; otherwise that value or its neighbour, o * (1.0f / l) rounds
    twice), every row of a head equal to every other"""
    T, H, D, Ns = case
    built = [uniform(T, N, H, D, dtype, 500 * b + N + D) for b, N in enumerate(Ns)]
    for b, (q, k, v, want) in enumerate(built):
        if Ns[b] > 1:
            move = uniform_sensitivity(v, H, D, dtype)
            assert move > 2.0, f"[uniform] sample {b}: a lost or doubled key moves the mean by {move:.2f} spacings only"
    outs = launch([x[:3] for x in built], H, D, None, dtype)
    for b, (out, (q, k, v, want)) in enumerate(zip(outs, built)):
        N = Ns[b]
        assert torch.equal(out, out[:1].expand_as(out)), f"[uniform] sample {b}: the rows of a head differ from each other"
        if N & (N - 1) == 0:
            assert torch.equal(out[0], want), f"[uniform] sample {b} N={N}: " + _first_wrong(out, want[None].expand_as(out), H, D, b)
        else:
            err = (out[0].double() - want.double()).abs() / spacing16(want.double(), dtype)
            assert torch.isfinite(out).all() and err.max().item() <= 1.0, \
                f"[uniform] sample {b} N={N}: {err.max().item():.2f} spacings from round16(mean V) at channels {(err > 1).nonzero().flatten()[:4].tolist()}"


def bar_ratio(out, q, k, v, H, D, scale, dtype):
    """|out - ref64| in units of ulp16 * sum_j p_j |v_jd| + sub16 * sum_j |v_jd| / (BAR l), elementwise -> the largest: <= BAR is the bar
    |out - ref64| <= 3.0 * ulp16 * sum_j p_j |v_jd| + sub16 * sum_j |v_jd| / l"""
    ref, condp, condl = softmax64(q, k, v, H, D, scale)
    unit = ULP16[dtype] * condp + SUB16[dtype] * condl / BAR
    err = (out.double() - ref).abs()
    if not torch.isfinite(out).all():
        return float("inf")
    return torch.where(unit > 0, err / unit.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double()).max().item()


def check_growth(launch, case, dtype, profile):
    """(d) rank-1 scores at scale ln 2: elementwise inside the bar against float64.  Sample b of the launch runs the b-th profile after ``profile``.
    -> [(profile, ratio against float64, ratio of |out - restatement| in the same unit)] per sample"""
    T, H, D, Ns = case
    names = list(PROFILES)
    mine = [names[(names.index(profile) + b) % len(names)] for b in range(len(Ns))]
    built = [rank1(T, N, H, D, dtype, name, 700 * b + N + D) for b, (N, name) in enumerate(zip(Ns, mine))]
    scale = math.log(2.0)
    outs = launch(built, H, D, scale, dtype)
    res = []
    for b, (out, (q, k, v)) in enumerate(zip(outs, built)):
        ratio = bar_ratio(out, q, k, v, H, D, scale, dtype)
        _, condp, condl = softmax64(q, k, v, H, D, scale)
        rest = chunked_softmax_ref(q, k, v, H, D, scale, dtype).double()
        against = ((out.double() - rest).abs() / (ULP16[dtype] * condp + SUB16[dtype] * condl / BAR)).max().item()
        res.append((mine[b], ratio, against))
        print(f"growth {case_id(case)} sample {b} {mine[b]} {dtype}: {ratio:.3f} against float64 (bar {BAR}), {against:.3f} against the restatement")
    for name, ratio, _ in res:
        assert ratio <= BAR, f"[growth] {name}: |out - ref64| reaches {ratio:.3f} x (ulp16 sum p|v| + sub16 sum|v| / (3 l)), bar {BAR}"
    return res


def randn_inputs(T, N, H, D, dtype, seed):
    g = _gen(seed)
    return tuple(torch.randn(r, H * D, generator=g).to(dtype) for r in (T, N, N))


def check_scale(launch, case, dtype):
    """(e) randn inputs at scale 0.03 / 0.2 / 1.0 inside the bar of (d) against float64 with THAT scale, and op(2 q, scale / 2) == op(q, scale) bit
    for bit (c = scale * log2(e) halves exactly, the fp32 scores double exactly: identical arithmetic)"""
    T, H, D, Ns = case
    built = [randn_inputs(T, N, H, D, dtype, 900 * b + N + D) for b, N in enumerate(Ns)]
    res = {}
    for scale in SCALES:
        outs = launch(built, H, D, scale, dtype)
        res[scale] = max(bar_ratio(out, q, k, v, H, D, scale, dtype) for out, (q, k, v) in zip(outs, built))
        print(f"scale {scale} {case_id(case)} {dtype}: {res[scale]:.3f} against float64 (bar {BAR})")
    for scale, ratio in res.items():
        assert ratio <= BAR, f"[scale] scale={scale}: |out - ref64| reaches {ratio:.3f} x the unit of the bar {BAR}"
    twice = [((q.float() * 2).to(dtype), k, v) for q, k, v in built]
    assert all(torch.equal(q2.float() / 2, q.float()) for (q2, _, _), (q, _, _) in zip(twice, built)), "[scale] 2 q is not exact"
    for scale in SCALES[:2]:
        one, two = launch(built, H, D, scale, dtype), launch(twice, H, D, scale / 2, dtype)
        for b, (x, y) in enumerate(zip(one, two)):
            assert torch.equal(x, y), f"[scale] op(2 q, {scale} / 2) != op(q, {scale}): " + _first_wrong(y, x, H, D, b)
    return res


def check_rounded_sum(launch, case, dtype):
    """(g) two_level rows: out is round16 of (sum_anchors v + r sum_others v) / (A + r (N - A)) with r the ROUNDED probability -- bit for bit,
    unless the float64 answer lies within (N + 4) * 2^-24 of a rounding boundary (the N fp32 additions, 1 / l, the product and exp2's last bit
    on top of the anchors' exact 1.0), where either side is right.  Samples of one key have nothing to sum and are skipped."""
    T, H, D, Ns = case
    built = [two_level(T, N, H, D, dtype, 1100 * b + N + D) for b, N in enumerate(Ns)]
    outs = launch([x[:3] for x in built], H, D, math.log(2.0), dtype)
    for b, (out, (q, k, v, want)) in enumerate(zip(outs, built)):
        if Ns[b] < 2:
            continue
        tol = (Ns[b] + 4) * 2.0 ** -24 * want.abs()
        lo, hi = round16(want - tol, dtype), round16(want + tol, dtype)
        ok = (out == lo) | (out == hi)
        assert (lo == hi).double().mean().item() > 0.7, "[rounded-sum] too many answers near a rounding boundary: the test has no teeth"
        assert ok.all(), (f"[rounded-sum] sample {b}: {int((~ok).sum())} of {ok.numel()} values are not round16 of the answer over the ROUNDED "
                          f"probabilities; first (row, column) {(~ok).nonzero()[0].tolist()}")
