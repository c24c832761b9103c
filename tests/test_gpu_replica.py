"""Replica path with REAL repacked models: two processes on cuda:0 (gloo carries the CUDA tensors; RCCL refuses two ranks
on one device), rank 0 initialises and repacks, the broadcast must bring rank 1 to the same kernel-layout model."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from nunchaku_amd import replica
    from nunchaku_amd.models.flux import FluxTransformerAMD

    replica.init_process_group("gloo")
    torch.cuda.set_device(0)
    model = FluxTransformerAMD(num_layers=1, num_single_layers=1, dim=256, heads=2, in_channels=64, joint_attention_dim=128,
                               pooled_projection_dim=64, device="cuda")
    if rank == 0:
        model.init_synthetic_(seed=0)  # repacks: qweight becomes the [out, 3*in/4] FP6 image on this rank only
    nbytes = replica.broadcast_module_(model, src=0)
    model.eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    side, t_txt = 16, 256
    lat = torch.randn(1, side * side, 64, device="cuda", generator=g).bfloat16()
    enc = torch.randn(1, t_txt, 128, device="cuda", generator=g).bfloat16()
    pooled = torch.randn(1, 64, device="cuda", generator=g).bfloat16()
    img_ids = torch.zeros(side * side, 3, device="cuda")
    img_ids[:, 1] = torch.arange(side, device="cuda").repeat_interleave(side)
    img_ids[:, 2] = torch.arange(side, device="cuda").repeat(side)
    from nunchaku_amd import mode

    with torch.no_grad(), mode.deterministic_mode():  # fixed-point low-rank sums: replicas must agree BIT FOR BIT
        y = model(lat, enc, pooled, torch.tensor([0.5], device="cuda"), img_ids, torch.zeros(t_txt, 3, device="cuda"),
                  torch.tensor([3.5], device="cuda")).float()
    torch.cuda.synchronize()
    out.put((rank, nbytes, y.cpu().numpy()))  # by value: a torch tensor travels as a shared-memory handle that dies with this process
    replica.barrier()
    dist.destroy_process_group()


def test_two_replicas_agree_after_the_weight_broadcast(built_lib):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, n0, y0), (_, n1, y1) = res
    y0, y1 = torch.from_numpy(y0), torch.from_numpy(y1)
    assert n0 == n1 > 0 and torch.isfinite(y0).all()
    assert torch.equal(y0, y1), "same weights, same inputs, deterministic mode: the two replicas must agree bit for bit"


def _worker_filled_cache(rank, world, port, out):
    """Rank 128: both ranks own a complete kernel-layout model (other seeds, the same shapes) and run a forward before the broadcast, which
    packs the fragment images of their own low-rank factors (ABI 21); the broadcast then writes the receiver's tensors in place."""
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from nunchaku_amd import _C, mode, replica
    from nunchaku_amd.models.flux import FluxTransformerAMD
    from tests.helpers import served_fragment_images

    replica.init_process_group("gloo")
    torch.cuda.set_device(0)
    model = FluxTransformerAMD(num_layers=1, num_single_layers=1, dim=256, heads=2, in_channels=64, joint_attention_dim=128,
                               pooled_projection_dim=64, rank=128, device="cuda").init_synthetic_(seed=10 + rank).eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    side, t_txt = 16, 256
    lat = torch.randn(1, side * side, 64, device="cuda", generator=g).bfloat16()
    enc = torch.randn(1, t_txt, 128, device="cuda", generator=g).bfloat16()
    pooled = torch.randn(1, 64, device="cuda", generator=g).bfloat16()
    img_ids = torch.zeros(side * side, 3, device="cuda")
    img_ids[:, 1] = torch.arange(side, device="cuda").repeat_interleave(side)
    img_ids[:, 2] = torch.arange(side, device="cuda").repeat(side)

    def fwd():
        return model(lat, enc, pooled, torch.tensor([0.5], device="cuda"), img_ids, torch.zeros(t_txt, 3, device="cuda"),
                     torch.tensor([3.5], device="cuda")).float()

    with torch.no_grad():
        fwd()  # fills the fragment cache from this rank's own weights
    frag = sum(1 for p in model.parameters() for k in (_C._converted.get(p) or {})
               if k[0].startswith("frag_") and (k[1], k[2]) == (p.storage_offset(), tuple(p.shape)))
    ptrs = [p.data_ptr() for p in model.parameters()]
    nbytes = replica.broadcast_module_(model, src=0)
    in_place = ptrs == [p.data_ptr() for p in model.parameters()]
    with torch.no_grad(), mode.deterministic_mode():  # fixed-point low-rank sums: replicas must agree BIT FOR BIT
        y = fwd()
    # the kernels read the images only with fp32 low-rank sums, whose run-to-run noise would hide a stale one in the output: what the cache
    # serves now is compared with a fresh pack of the (broadcast) weights
    served = served_fragment_images(model)
    out.put((rank, nbytes, frag, in_place, served, y.cpu().numpy()))
    replica.barrier()
    dist.destroy_process_group()


def test_two_replicas_agree_after_the_weight_broadcast_with_filled_fragment_cache(built_lib):
    """Rank 128 (the rank of the real Qwen-Image checkpoints): fragment images a receiver packed from its own weights before ``broadcast_module_``
    must not be served after it.  Deterministic mode: the replicas agree bit for bit, and every image either rank serves is a pack of its current
    (broadcast) weights."""
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker_filled_cache, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, n0, f0, _, s0, y0), (_, n1, f1, in_place, s1, y1) = res
    y0, y1 = torch.from_numpy(y0), torch.from_numpy(y1)
    assert n0 == n1 > 0 and f0 == f1 > 0, (n0, n1, f0, f1)
    assert in_place, "same shapes on both ranks: the broadcast writes the receiver's tensors in place"
    assert s0[0] == s1[0] == f0, (s0, s1, f0)  # every image of the model is served and was checked
    assert not s0[1], f"source: stale fragment images of {s0[1]}"
    assert not s1[1], f"receiver: fragment images packed from its weights before the broadcast are still served for {s1[1]}"
    assert torch.isfinite(y0).all()
    assert torch.equal(y0, y1), "same weights, same inputs, deterministic mode: the two replicas must agree bit for bit"
