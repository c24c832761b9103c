"""The workspace contract of include/svdq_amd.h, asserted directly on the process's own cached workspaces (nunchaku_amd._C._workspace: one per device,
stream and kind for every launch of every shape, geometry and epilogue), over the rows of tests/workspace_cases.py:

1. a launch leaves every word of the header -- arrival counters, error word, ticket counters -- at zero;
2. a launch reads no byte behind the header that it did not write itself: its outputs do not change when those bytes are zeros, NaNs or 1e30;
3. a launch does not depend on the launch before it: B after A (other operands, another shape, geometry or epilogue) equals B alone -- the diagonal
   (A, A) on two seeds is the sharp case: the slabs then hold partial tiles of other operands at exactly the addresses B's owners read;
4. the same for launches queued back to back without a host synchronisation, and
5. for a captured graph replayed on fresh operands.

Everything is compared bit for bit (``torch.equal``) but the fp32 sums of atomics, which the header says depend on the order of arrival: those are held to
the bound of the existing test of their path against its oracle, and must be finite -- which the NaN fill makes a sharp check.  No test writes to a
header: a non-zero counter would make an owner spin for its bounded second and raise the error word."""

import pytest
import torch

from tests import workspace_cases as W

pytestmark = pytest.mark.gpu

SEED = 1
PATTERNS = ("zero", "nan", "finite")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from nunchaku_amd import _lib

    _lib.load()


_OPERANDS, _SOLO = {}, {}


def operands(case, dtype, seed):
    """built once per (row, dtype, seed), kept on the device, never modified"""
    key = (case.name, dtype, seed)
    if key not in _OPERANDS:
        _OPERANDS[key] = case.build(seed, dtype)
    return _OPERANDS[key]


def workspace(kind):
    """the current stream's workspace of ``kind``, fetched anew after every launch (a launch may have replaced it by a larger one)"""
    from nunchaku_amd import _C

    return _C._workspace(torch.device("cuda"), kind)


def fill(kinds, pattern):
    for kind in kinds:
        W.poison(workspace(kind).buf, {"gemm": W.GEMM_HEADER_BYTES, "attention": W.ATTENTION_HEADER_BYTES}.get(kind, 0), pattern)


def assert_headers_zero(kinds, what):
    for kind, nbytes in (("gemm", W.GEMM_HEADER_BYTES), ("attention", W.ATTENTION_HEADER_BYTES)):
        if kind in kinds:
            idx = W.first_nonzero_word(workspace(kind).buf, nbytes)
            assert idx is None, f"{what}: word {idx} of the {kind} header is {int(workspace(kind).buf[:nbytes].view(torch.int32)[idx])}, not 0"


def launch(case, o):
    res = case.run(o)
    case.check_plan(case.last_plan())
    return res


def judge(case, o, res, ref, what):
    for name in case.exact:
        same = torch.equal(res[name], ref[name])
        assert same, f"{what}: {name} differs in {int((res[name] != ref[name]).sum())} of {ref[name].numel()} elements"
    if case.bounded:
        case.check_bounded(o, res)


def solo(case, dtype, seed):
    """the row launched alone on a zero-filled tail: the reference of every comparison (once per row, dtype and seed).  The launch before the fill lets a
    launch that asks for a larger workspace get it first, so that the fill and every later launch see the buffer the process keeps."""
    key = (case.name, dtype, seed)
    if key not in _SOLO:
        o = operands(case, dtype, seed)
        launch(case, o)
        fill((case.kind,), "zero")
        res = launch(case, o)
        case.status()
        for name in case.exact:
            assert bool(torch.isfinite(res[name].float()).all()), f"{case.name}: {name} is not finite"
        if case.bounded:
            case.check_bounded(o, res)
        _SOLO[key] = res
    return _SOLO[key]


HEADED = W.of_kind("gemm") + W.of_kind("attention")


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("case", HEADED, ids=repr)
def test_counters_return_to_zero(case, dtype):
    """after the row: all 2048 words of the GEMM header / all 1024 of the attention header are zero, and the status query is clean"""
    o = operands(case, dtype, SEED)
    launch(case, o)
    case.status()
    assert_headers_zero((case.kind,), f"after {case.name} ({dtype})")
    launch(case, o)  # and again, on the header that launch left
    case.status()
    assert_headers_zero((case.kind,), f"after the second {case.name} ({dtype})")


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("case", W.CASES, ids=repr)
def test_a_launch_reads_only_what_it_wrote(case, dtype):
    """the same operands with everything behind the header (scratch-only kinds: the whole buffer) zero, NaN and 1e30: the same outputs"""
    o = operands(case, dtype, SEED)
    ref = solo(case, dtype, SEED)
    for pattern in PATTERNS:
        fill((case.kind,), pattern)
        res = launch(case, o)
        case.status()
        judge(case, o, res, ref, f"{case.name} ({dtype}) on a tail filled with {pattern}")
    assert_headers_zero((case.kind,), f"after {case.name} ({dtype})")


def _pairs():
    return [pytest.param(b, id=b.name) for kind in W.KINDS for b in W.of_kind(kind)]


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("b", _pairs())
def test_launch_order_does_not_matter(b, dtype):
    """every ordered pair (A, B) of one kind: A on seed s, then B on seed s + 1 with the workspace untouched in between -- B equals B alone"""
    ob, ref = operands(b, dtype, SEED + 1), solo(b, dtype, SEED + 1)
    firsts = W.of_kind(b.kind)
    for a in firsts:
        solo(a, dtype, SEED)  # (A's own reference, and its workspace at its final size)
    for a in firsts:
        launch(a, operands(a, dtype, SEED))
        res = launch(b, ob)
        b.status()
        judge(b, ob, res, ref, f"{b.name} after {a.name} ({dtype})")
    assert_headers_zero((b.kind,), f"after the pairs of {b.name} ({dtype})")


_GRAPH_STREAM = []


def _graph_stream():
    """one capture stream for the module: a workspace a graph points at is kept for the life of the process, so both dtypes share the stream's pair"""
    if not _GRAPH_STREAM:
        _GRAPH_STREAM.append(torch.cuda.Stream())
    return _GRAPH_STREAM[0]


def _chain(dtype, seed):
    return [(W.BY_NAME[name], operands(W.BY_NAME[name], dtype, seed)) for name in W.CHAIN]


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_back_to_back_without_a_host_sync(dtype):
    """three stream-K / queue GEMMs of different geometry and two persistent attention launches queued on one stream, nothing in between"""
    chain = _chain(dtype, SEED)
    refs = [solo(case, dtype, SEED) for case, _ in chain]
    fill(("gemm", "attention"), "nan")
    torch.cuda.synchronize()
    got = [launch(case, o) for case, o in chain]  # (no call in here synchronises: the status word is a host read of pinned memory)
    torch.cuda.synchronize()
    for (case, o), res, ref in zip(chain, got, refs):
        judge(case, o, res, ref, f"{case.name} ({dtype}) inside the chain")
    for case, _ in chain:
        case.status()
    assert_headers_zero(("gemm", "attention"), f"after the chain ({dtype})")


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_graph_replay(dtype):
    """the chain captured on a stream of its own (warmed up there first, so that the workspaces the graph points at exist before the capture and are not
    re-created, zero fill included, by every replay): three replays, each on fresh operands and a freshly poisoned tail, equal the eager solo results"""
    from nunchaku_amd import _C

    def clone(t):
        c = t.clone()
        return _C.mark_amd(c) if getattr(t, "_svdq_amd", False) else c

    chain = _chain(dtype, SEED)
    static = [{k: clone(t) for k, t in o.items()} for _, o in chain]
    stream = _graph_stream()
    with torch.cuda.stream(stream):
        for (case, _), o in zip(chain, static):
            launch(case, o)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        outs = [case.run(o) for (case, _), o in zip(chain, static)]
    dev = torch.cuda.current_device()
    spaces = {kind: _C._workspaces[(dev, stream.cuda_stream, kind)] for kind in ("gemm", "attention")}
    assert all(ws.captured for ws in spaces.values())
    for i, pattern in enumerate(("nan", "finite", "zero")):
        seed = SEED + 1 + i
        fresh = _chain(dtype, seed)
        refs = [solo(case, dtype, seed) for case, _ in fresh]
        for o, (_, new) in zip(static, fresh):
            for k, t in new.items():
                o[k].copy_(t)
        W.poison(spaces["gemm"].buf, W.GEMM_HEADER_BYTES, pattern)
        W.poison(spaces["attention"].buf, W.ATTENTION_HEADER_BYTES, pattern)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for (case, o), res, ref in zip(fresh, outs, refs):
            judge(case, o, res, ref, f"{case.name} ({dtype}), replay {i} on a tail filled with {pattern}")
        for kind, nbytes in (("gemm", W.GEMM_HEADER_BYTES), ("attention", W.ATTENTION_HEADER_BYTES)):
            idx = W.first_nonzero_word(spaces[kind].buf, nbytes)
            assert idx is None, f"replay {i}: word {idx} of the {kind} header of the captured workspace is not 0"
    del graph
