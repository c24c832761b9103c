"""Layer-wise host offload of transformer blocks over a ring of device slots (SURVEY.md section 8 row f2 / BASELINE config 5).

Public surface of the reference's ``CPUOffloadManager`` (nunchaku/models/utils.py:52-262): constructor arguments,
``set_device``, ``initialize``, ``get_block``, ``step``, ``load_block``, the attributes ``blocks`` / ``buffer_blocks`` /
``memory_stream`` / ``current_block_idx`` / ``forward_counter``.  The mechanism behind it is this package's own:

* **Host side.**  Every offloaded block is ONE flat pinned byte image (all its tensors back to back, 256-byte aligned) and
  its parameters are VIEWS into that image -- the block stays a complete, valid CPU module (``state_dict()``, ``.to()``,
  turning offload off again all work).  SVDQuant layers are converted once: every tensor to the kernel layout except
  ``qweight``, which stays in -- or is converted back to -- the checkpoint's 4-bit nibble form (``svdq_unrepack_qweight``):
  two thirds of the FP6 operand image's bytes on the PCIe link, which bounds an offloaded step (a Qwen-Image block
  computes in ~1.3 ms and weighs 113 MB as nibbles, 170 MB as images).
* **Device side.**  ``num_slots`` (default 2) slots, each ONE flat device buffer with the host image's layout plus the FP6
  images its code tensors are expanded into (``svdq_repack_qweight`` on the memory stream, right behind the copy): a block
  load is a single H2D copy (one SDMA submission; the reference issues one per tensor, ~120).
* **Schedule.**  Offloaded blocks are numbered by a running sequence ``t`` (never reset: it continues from one forward to
  the next); block ``t`` lives in slot ``t % num_slots``.  Two events per slot: ``free`` (recorded on the compute stream
  when the slot's tenant has been computed) and ``filled`` (recorded on the memory stream behind copy + expansion).
  Finishing block ``t`` frees its slot and immediately queues the load of block ``t + num_slots`` into it -- at the end of a
  forward that is already the next forward's first blocks, so a denoise loop never starts cold.  More slots = deeper prefetch.

MI355X: 288 GB of HBM make offload unnecessary for the models of this package (Qwen-Image int4: ~11 GB); it exists for API
parity and for co-locating many models on one GPU, and is off unless ``set_offload(True)`` is called.
"""

from __future__ import annotations

import copy

import torch
from torch import nn

from .. import _lib, layout
from .linear import AWQW4A16Linear, SVDQW4A4Linear

_ALIGN = 256


def copy_params_into(src: nn.Module, dst: nn.Module, non_blocking: bool = True):
    """reference: nunchaku/utils.py:336-366 -- parameters and buffers of ``src`` into the same-structured ``dst``."""
    with torch.no_grad():
        for ps, pd in zip(src.parameters(), dst.parameters()):
            pd.copy_(ps, non_blocking=non_blocking)
        for bs, bd in zip(src.buffers(), dst.buffers()):
            bd.copy_(bs, non_blocking=non_blocking)


def _named_tensors(block: nn.Module):
    """(module name, tensor name, tensor) of every parameter and buffer of ``block``, in a fixed order"""
    out = []
    for mn, m in block.named_modules():
        for pn, p in m.named_parameters(recurse=False):
            out.append((mn, pn, p))
        for bn, b in m.named_buffers(recurse=False):
            out.append((mn, bn, b))
    return out


class _Slot:
    """One device-side home of an offloaded block: a module whose tensors view pieces of ``flat`` (the code tensors: FP6
    images expanded from the nibble pieces), the block index it currently holds, and its two events."""

    def __init__(self, module: nn.Module, flat: torch.Tensor, expand: list, device):
        self.module, self.flat, self.expand = module, flat, expand
        self.tenant = -1
        self.filled = torch.cuda.Event()  # memory stream: copy + expansion of the tenant are done
        self.free = torch.cuda.Event()    # compute stream: the tenant has been computed, the slot may be overwritten
        self.used = False                 # free has been recorded at least once


class CPUOffloadManager:
    def __init__(self, blocks: list[nn.Module], device: str | torch.device = torch.device("cuda"), use_pin_memory: bool = True,
                 on_gpu_modules: list[nn.Module] = [], num_blocks_on_gpu: int | str = 1, empty_cache_freq: int = 0, num_slots: int = 2):
        if num_blocks_on_gpu == "auto":
            # (round 6, VERDICT r5: the reference's default of 1 resident block is sized for a 16-24 GB card; on a 288 GB part every block that fits should stay.)
            # As many blocks as the device's FREE memory holds beside the slots, with a quarter of it left to activations and workspaces
            num_blocks_on_gpu = self.blocks_that_fit(blocks, device, num_slots)
        if not isinstance(num_blocks_on_gpu, int) or num_blocks_on_gpu <= 0:
            raise ValueError("num_blocks_on_gpu must be a positive integer or 'auto'")
        if num_slots < 2:
            raise ValueError("num_slots must be at least 2 (one slot computes while another fills)")
        self.blocks = blocks
        self.use_pin_memory = use_pin_memory
        self.on_gpu_modules = on_gpu_modules
        self.num_blocks_on_gpu = min(num_blocks_on_gpu, len(blocks))
        self.num_slots = num_slots
        self.empty_cache_freq = empty_cache_freq
        self.memory_stream = None
        self.device = None
        self.current_block_idx = 0
        self.forward_counter = 0
        self._images: dict[int, torch.Tensor] = {}   # offloaded block index -> flat pinned byte image
        self._entries: list | None = None            # [(module name, tensor name, offset, nbytes, (N, K) of a nibble tensor or None)]
        self._slots: list[_Slot] = []
        self._seq = 0                                # sequence number of the first offloaded block of the CURRENT forward
        self._queued = 0                             # sequence numbers < _queued have had their load issued
        self.set_device(device)

    @staticmethod
    def blocks_that_fit(blocks: list[nn.Module], device, num_slots: int = 2, reserve: float = 0.25) -> int:
        """num_blocks_on_gpu="auto": how many of ``blocks`` the device's free memory holds resident (FP6 images: 1.5 x the checkpoint's nibble bytes) beside
        ``num_slots`` slots, keeping ``reserve`` of the free memory for activations and workspaces; at least 1, at most all of them (= no offload traffic)."""
        if not blocks:
            return 1
        per = 0
        for t in list(blocks[0].parameters()) + list(blocks[0].buffers()):
            n = t.numel() * t.element_size()
            per += n * 3 // 2 if t.dtype == torch.int8 else n
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            return 1
        free, _total = torch.cuda.mem_get_info(dev)
        room = int(free * (1.0 - reserve)) - num_slots * per
        return max(1, min(len(blocks), room // max(per, 1)))

    # ------------------------------------------------------------------ public views of the internals
    @property
    def buffer_blocks(self) -> list[nn.Module]:
        return [s.module for s in self._slots]

    @property
    def n_offloaded(self) -> int:
        return len(self.blocks) - self.num_blocks_on_gpu

    def host_bytes_per_block(self, block_idx: int | None = None) -> int:
        """Bytes that cross the link for one offloaded block (its flat image: nibble code tensors + every other tensor)."""
        i = self.num_blocks_on_gpu if block_idx is None else block_idx
        return self._images[i].numel() if i in self._images else 0

    def nibble_bytes(self, block_idx: int | None = None) -> int:
        """Bytes of an offloaded block's image that are 4-bit code tensors in checkpoint (nibble) form."""
        return sum(n for _, _, _, n, nib in (self._entries or []) if nib is not None)

    # ------------------------------------------------------------------ placement
    @torch.no_grad()
    def _to_offload_form(self, block: nn.Module):
        """On the GPU: every SVDQuant tensor of ``block`` in the kernel layout, except ``qweight`` in nibble form."""
        for m in block.modules():
            if isinstance(m, AWQW4A16Linear):  # same refusal as below: the LoRA factors are no part of the host image
                if m._lora is not None:
                    import warnings
                    warnings.warn("CPUOffloadManager: the runtime LoRA attached to an offloaded AWQW4A16Linear is removed (set_lora / "
                                  "update_lora_params do not reach offloaded blocks)", RuntimeWarning, stacklevel=3)
                m.reset_lora()
                m._offloaded = True
                continue
            if not isinstance(m, SVDQW4A4Linear):
                continue
            if m._base_lowrank is not None:
                # a runtime LoRA is not part of the host image (its rank changes the shapes of proj_down / proj_up, which the device slots are
                # sized for): it is dropped HERE, loudly; attach LoRAs to resident blocks, or merge them before set_offload(True)
                import warnings
                warnings.warn("CPUOffloadManager: the runtime LoRA attached to an offloaded SVDQW4A4Linear is removed (set_lora / "
                              "update_lora_params do not reach offloaded blocks)", RuntimeWarning, stacklevel=3)
            m.reset_lora()
            m._offloaded = True  # set_lora on this layer raises until restore(): the device slots are sized for the checkpoint's rank
            if "qweight" in m._amd_names:
                m.qweight.data = layout.unrepack_qweight(m.qweight.data)
                m._amd_names.discard("qweight")
                m.qweight._svdq_amd = False
            m.repack_(skip=("qweight",))

    @torch.no_grad()
    def _build_host_image(self, idx: int, device: torch.device):
        block = self.blocks[idx]
        block.to(device)
        self._to_offload_form(block)
        entries, off = [], 0
        tensors = _named_tensors(block)
        mods = dict(block.named_modules())
        for mn, tn, t in tensors:
            m = mods[mn]
            nib = (m.out_features, m.in_features) if isinstance(m, SVDQW4A4Linear) and tn == "qweight" else None
            size = t.numel() * t.element_size()
            entries.append((mn, tn, off, size, nib))
            off = (off + size + _ALIGN - 1) // _ALIGN * _ALIGN
        if self._entries is None:
            self._entries, self._image_bytes = entries, off
        elif entries != self._entries:
            raise RuntimeError(f"offload: block {idx} does not have the tensor layout of the first offloaded block (all "
                               "offloaded blocks must share one structure)")
        flat = torch.empty(off, dtype=torch.uint8, device="cpu")
        if self.use_pin_memory:
            flat = flat.pin_memory()
        for (mn, tn, o, size, _), (_, _, t) in zip(entries, tensors):
            piece = flat[o:o + size]
            piece.copy_(t.data.contiguous().view(-1).view(torch.uint8))
            t.data = piece.view(t.dtype).view(t.shape)  # the block's tensor IS the piece of the pinned image from now on
        self._images[idx] = flat

    @torch.no_grad()
    def _build_slots(self, device: torch.device):
        """``num_slots`` device modules shaped like an offloaded block.  Built from the first offloaded block's host image."""
        first = self.num_blocks_on_gpu
        self._slots = []
        if first >= len(self.blocks):
            return
        template = self.blocks[first]
        for _ in range(self.num_slots):
            module = copy.deepcopy(template)  # CPU copy of the structure (tensors: copies of the host views)
            flat = torch.empty(self._image_bytes, dtype=torch.uint8, device=device)
            mods = dict(module.named_modules())
            expand = []
            for mn, tn, o, size, nib in self._entries:
                m = mods[mn]
                t = getattr(m, tn)
                if nib is not None:
                    N, K = nib
                    dev_t = torch.empty(N, K * 3 // 4, dtype=torch.int8, device=device)
                    expand.append((flat[o:o + size], dev_t, N, K))
                else:
                    dev_t = flat[o:o + size].view(t.dtype).view(t.shape)
                # The slot's tensors ARE the views (not `t.data = view`, which keeps the copy's own version counter): a view shares the
                # version counter of `flat`, so every load's `flat.copy_` bumps `_version` of all of them and nunchaku_amd._C re-packs the
                # fragment images it caches per (storage, version) -- the low-rank factors of a new tenant are never served from the
                # previous tenant's images.  The image an entry replaces was allocated on the compute stream and is read only by kernels
                # queued there; the caching allocator hands its memory out again only to later work of that stream, so freeing it while
                # such a kernel is still queued is safe (the load itself runs on the memory stream and never touches the images).
                if tn in m._parameters:
                    m._parameters[tn] = nn.Parameter(dev_t, requires_grad=t.requires_grad)
                else:
                    m._buffers[tn] = dev_t
            for m in module.modules():
                if isinstance(m, SVDQW4A4Linear):
                    m._set_amd_names(set(m._layout_params()))  # everything in the kernel layout once a load has landed
            self._slots.append(_Slot(module, flat, expand, device))

    def set_device(self, device: torch.device | str, force: bool = False):
        """Resident blocks and the device slots to ``device``; offloaded blocks to their pinned host images (built once: they
        do not depend on the device).  Calling it again with another device (or ``force=True``) rebuilds the slots only."""
        if isinstance(device, str):
            device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("CPUOffloadManager: the compute device must be a GPU")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.device == device and not force:
            return
        if self.memory_stream is not None:
            torch.cuda.synchronize(self.device)  # nothing of the old device's schedule may still be in flight
        self.device = device
        self.memory_stream = torch.cuda.Stream(device=device)
        for module in self.on_gpu_modules:
            module.to(device)
        for i, block in enumerate(self.blocks):
            if i < self.num_blocks_on_gpu:
                block.to(device)
                for m in block.modules():
                    if isinstance(m, SVDQW4A4Linear):
                        m.repack_()
            elif i not in self._images:
                self._build_host_image(i, device)
        torch.cuda.synchronize(device)  # the images are complete before anything reads them
        self._build_slots(device)
        self._seq = self._queued = 0
        self.current_block_idx = 0

    @torch.no_grad()
    def restore(self, device: torch.device | str | None = None):
        """Undo the offload: every block becomes an ordinary module on ``device`` again (its tensors copied out of the pinned
        images; code tensors return to the FP6 image lazily, at their first use).  The manager is unusable afterwards."""
        device = torch.device(device) if device is not None else self.device
        if self.memory_stream is not None:
            torch.cuda.synchronize(self.device)
        for i in sorted(self._images):
            blk = self.blocks[i]
            for _, _, t in _named_tensors(blk):
                t.data = t.data.to(device, copy=True)
            for m in blk.modules():
                if isinstance(m, (SVDQW4A4Linear, AWQW4A16Linear)):
                    m._offloaded = False
        self._images.clear()
        self._slots = []
        self._entries = None

    # ------------------------------------------------------------------ the ring
    def _block_of(self, seq: int) -> int:
        return self.num_blocks_on_gpu + seq % self.n_offloaded

    def load_block(self, block_idx: int, non_blocking: bool = True, slot: int | None = None):
        """Host image of block ``block_idx`` -> device slot (default: the slot the running sequence assigns) on the CURRENT
        stream: one copy of the flat image, then the nibble -> FP6 expansion of its code tensors."""
        if block_idx < self.num_blocks_on_gpu or block_idx >= len(self.blocks):
            return
        if slot is None:
            slot = (self._seq + block_idx - self.num_blocks_on_gpu) % self.num_slots
        s = self._slots[slot]
        s.flat.copy_(self._images[block_idx], non_blocking=non_blocking)
        if s.expand:
            lib = _lib.load()
            st = torch.cuda.current_stream().cuda_stream
            for nib, img, N, K in s.expand:
                _lib.check(lib.svdq_repack_qweight(nib.data_ptr(), img.data_ptr(), N, K, st), "svdq_repack_qweight")
        s.tenant = block_idx

    def _queue_load(self, seq: int):
        """Issue the load of sequence number ``seq`` on the memory stream, behind the event that frees its slot."""
        s = self._slots[seq % self.num_slots]
        with torch.cuda.stream(self.memory_stream):
            if s.used:
                self.memory_stream.wait_event(s.free)
            self.load_block(self._block_of(seq), slot=seq % self.num_slots)
            s.filled.record(self.memory_stream)

    def initialize(self, stream: torch.cuda.Stream | None = None):
        """Start of a forward on ``stream``: make sure the first ``num_slots`` offloaded blocks are on their way (after the
        first forward they already are: the previous forward's last steps queued them)."""
        if self.n_offloaded <= 0:
            return
        if stream is None:
            stream = torch.cuda.current_stream()
        if self.current_block_idx != 0:  # an aborted forward: restart the ring from a clean state
            self.reset()
        while self._queued < self._seq + min(self.num_slots, self.n_offloaded):
            self._queue_load(self._queued)
            self._queued += 1
        if self.num_blocks_on_gpu == 0:
            stream.wait_event(self._slots[self._seq % self.num_slots].filled)

    def reset(self):
        """Drop the ring's state (after an exception in the middle of a forward): the next ``initialize`` reloads."""
        torch.cuda.synchronize(self.device)
        for s in self._slots:
            s.tenant, s.used = -1, False
        self._seq = self._queued = 0
        self.current_block_idx = 0

    def get_block(self, block_idx: int | None = None) -> nn.Module:
        if block_idx is None:
            block_idx = self.current_block_idx
        if block_idx < self.num_blocks_on_gpu:
            return self.blocks[block_idx]
        return self._slots[(self._seq + block_idx - self.num_blocks_on_gpu) % self.num_slots].module

    def step(self, compute_stream: torch.cuda.Stream | None = None):
        """Block ``current_block_idx`` has been queued for compute on ``compute_stream``: free its slot behind it, queue the
        load that reuses the slot, and make the compute stream wait for the block it runs next."""
        if compute_stream is None:
            compute_stream = torch.cuda.current_stream()
        cur, nb = self.current_block_idx, self.num_blocks_on_gpu
        if cur >= nb:
            seq = self._seq + cur - nb
            s = self._slots[seq % self.num_slots]
            s.free.record(compute_stream)
            s.used = True
            if self._queued == seq + self.num_slots:  # the next tenant of exactly this slot (steady state: always)
                self._queue_load(self._queued)
                self._queued += 1
        self.current_block_idx = cur + 1
        if self.current_block_idx < len(self.blocks):
            nxt = self.current_block_idx
            if nxt >= nb:
                compute_stream.wait_event(self._slots[(self._seq + nxt - nb) % self.num_slots].filled)
        else:
            self._seq += self.n_offloaded
            self.current_block_idx = 0
            self.forward_counter += 1
            if self.empty_cache_freq > 0 and self.forward_counter % self.empty_cache_freq == 0:
                torch.cuda.empty_cache()
