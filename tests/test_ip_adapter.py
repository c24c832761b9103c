"""IP-Adapter without a GPU: the loader, the adapters on stand-in classes, the refusals, the K/V cache, the shim import paths and the C
ABI of svdq_ip_attention (declaration, layout, export, validation)."""

import ctypes as C
import os
import re
import subprocess

import pytest
import torch
from torch import nn

from nunchaku_amd import _lib
from nunchaku_amd.models import ip_adapter as ipa
from nunchaku_amd.models.flux import FluxEngineMixin
from tests.ipa_ref import PREFIX, adapter_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def no_hub(monkeypatch):
    """no test may resolve a hub repository id: the branch that would is made to fail loudly"""
    import huggingface_hub

    def refuse(*args, **kwargs):
        raise AssertionError("a test reached huggingface_hub.hf_hub_download")

    monkeypatch.setattr(huggingface_hub, "hf_hub_download", refuse)


class Engine(nn.Module, FluxEngineMixin):
    """A transformer as the adapters see it: joint blocks to count, a width, a dtype and a device"""

    def __init__(self, blocks=3, dim=64):
        super().__init__()
        self.transformer_blocks = nn.ModuleList([nn.Identity() for _ in range(blocks)])
        self.single_transformer_blocks = nn.ModuleList()
        self.proj_out = nn.Linear(dim, 8, dtype=torch.bfloat16)
        self.dim, self.dtype_ = dim, torch.bfloat16

    def forward(self, *args):
        return "original"


# ---- loader -------------------------------------------------------------------------------------------------------------------------
def _check_loaded(ad, sd, blocks, cross_dim, dim):
    assert (len(ad.ip_k_projs), len(ad.ip_v_projs), ad.cross_dim, ad.dim) == (blocks, blocks, cross_dim, dim)
    for i in range(blocks):
        for n, lst in (("k", ad.ip_k_projs), ("v", ad.ip_v_projs)):
            base = f"{PREFIX}{i}.processor.ip_adapter_double_stream_{n}_proj"
            assert isinstance(lst[i], nn.Linear) and lst[i].weight.dtype == torch.bfloat16
            assert torch.equal(lst[i].weight, sd[base + ".weight"]) and torch.equal(lst[i].bias, sd[base + ".bias"])


def test_loader_round_trip_from_a_state_dict_with_inferred_shapes():
    sd = adapter_state_dict(3, 48, 64, seed=1)
    sd["ip_adapter_proj_model.proj.weight"] = torch.zeros(4, 4)  # the file's other content is ignored
    ad = ipa.IPAdapter(0.7).load_ip_adapter_weights_per_layer(sd, device="cpu")
    _check_loaded(ad, sd, 3, 48, 64)
    assert ad.ip_adapter_scale == 0.7


def test_loader_round_trip_from_a_file_and_a_directory(tmp_path):
    from safetensors.torch import save_file

    sd = adapter_state_dict(2, 32, 64, seed=2)
    path = tmp_path / "ip_adapter.safetensors"
    save_file(sd, str(path))
    _check_loaded(ipa.IPAdapter().load_ip_adapter_weights_per_layer(str(path), device="cpu"), sd, 2, 32, 64)
    _check_loaded(ipa.IPAdapter().load_ip_adapter_weights_per_layer(tmp_path, device="cpu"), sd, 2, 32, 64)
    other = tmp_path / "weights.safetensors"
    save_file(sd, str(other))
    _check_loaded(ipa.IPAdapter().load_ip_adapter_weights_per_layer(tmp_path, device="cpu", filename="weights.safetensors"), sd, 2, 32, 64)
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(FileNotFoundError):
        ipa.IPAdapter().load_ip_adapter_weights_per_layer(empty, device="cpu")


def test_loader_errors():
    sd = adapter_state_dict(3, 48, 64)
    with pytest.raises(ValueError, match="3 blocks, the transformer 2 joint blocks"):
        ipa.IPAdapter().load_ip_adapter_weights_per_layer(sd, num_blocks=2, device="cpu")
    with pytest.raises(ValueError, match="projects to 64 channels, the transformer has 128"):
        ipa.IPAdapter().load_ip_adapter_weights_per_layer(sd, dim=128, device="cpu")
    broken = {k: v for k, v in sd.items() if k != f"{PREFIX}1.processor.ip_adapter_double_stream_v_proj.weight"}
    with pytest.raises(KeyError, match="block 1: missing .*1.processor.ip_adapter_double_stream_v_proj.weight"):
        ipa.IPAdapter().load_ip_adapter_weights_per_layer(broken, device="cpu")
    gap = {k: v for k, v in sd.items() if not k.startswith(PREFIX + "1.")}
    with pytest.raises(KeyError, match="not 0 .. 1"):
        ipa.IPAdapter().load_ip_adapter_weights_per_layer(gap, device="cpu")
    with pytest.raises(KeyError, match="not an IP-Adapter file"):
        ipa.IPAdapter().load_ip_adapter_weights_per_layer({"x.weight": torch.zeros(2, 2)}, device="cpu")
    bad = dict(sd)
    bad[f"{PREFIX}2.processor.ip_adapter_double_stream_k_proj.weight"] = torch.zeros(64, 40, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="block 2 k_proj"):
        ipa.IPAdapter().load_ip_adapter_weights_per_layer(bad, device="cpu")


def test_a_string_that_is_no_path_is_a_hub_id_and_only_then(tmp_path):
    with pytest.raises(AssertionError, match="hf_hub_download"):  # (the autouse fixture's stand-in: the branch exists and nothing else takes it)
        ipa.IPAdapter().load_ip_adapter_weights_per_layer("some-org/flux-ip-adapter", device="cpu")


# ---- adapters, refusals, shims ------------------------------------------------------------------------------------------------------
def test_shim_import_paths():
    from nunchaku.models.ip_adapter import utils
    from nunchaku.models.ip_adapter.diffusers_adapters import apply_IPA_on_pipe
    from nunchaku.models.ip_adapter.diffusers_adapters.flux import apply_IPA_on_pipe as flux_pipe, apply_IPA_on_transformer
    from nunchaku.models.ip_adapter.utils import resize_numpy_image_long, undo_all_mods_on_transformer

    assert apply_IPA_on_transformer is ipa.apply_IPA_on_transformer and flux_pipe is ipa.apply_IPA_on_pipe
    assert undo_all_mods_on_transformer is ipa.undo_all_mods_on_transformer and utils.IPAdapter is ipa.IPAdapter
    assert callable(apply_IPA_on_pipe)
    import numpy as np

    small = np.zeros((10, 20, 3), np.uint8)
    assert resize_numpy_image_long(small, 768) is small  # (OpenCV is needed only to shrink)


def test_apply_on_transformer_and_pipe_and_undo():
    from nunchaku.models.ip_adapter.diffusers_adapters import apply_IPA_on_pipe
    from nunchaku.models.ip_adapter.diffusers_adapters.flux import apply_IPA_on_transformer
    from nunchaku.models.ip_adapter.utils import undo_all_mods_on_transformer

    sd = adapter_state_dict(3, 48, 64)
    e = Engine()
    keys = set(e.state_dict())
    forward = e.forward
    assert apply_IPA_on_transformer(e, ip_adapter_scale=0.5, repo_id=sd) is e
    assert e._is_IPA is True and isinstance(e.ip_adapter, ipa.IPAdapter) and e.ip_adapter.ip_adapter_scale == 0.5
    assert e.forward == forward and len(e.transformer_blocks) == 3  # no block swapping: the adapter is state on the engine
    emb = torch.zeros(1, 4, 48)
    e.set_ip_hidden_states(emb, negative_image_embeds=None)
    assert e.ip_adapter.image_embeds is emb
    assert undo_all_mods_on_transformer(e) is e
    assert getattr(e, "ip_adapter", None) is None and not e._is_IPA and not hasattr(e, "set_ip_hidden_states")
    assert set(e.state_dict()) == keys
    undo_all_mods_on_transformer(e)  # twice is fine

    class FluxPipeline:
        transformer = Engine()

    pipe = FluxPipeline()
    assert apply_IPA_on_pipe(pipe, ip_adapter_scale=1.0, repo_id=sd) is pipe and pipe.transformer._is_IPA

    class OtherPipeline:
        transformer = Engine()

    with pytest.raises(ValueError, match="Unknown pipeline class name"):
        apply_IPA_on_pipe(OtherPipeline(), repo_id=sd)
    with pytest.raises(TypeError, match="not a FLUX transformer"):
        apply_IPA_on_transformer(nn.Linear(2, 2), repo_id=sd)
    with pytest.raises(ValueError, match="3 blocks, the transformer 2"):
        apply_IPA_on_transformer(Engine(blocks=2), repo_id=sd)


def test_adapter_without_embeddings_raises_before_anything_runs():
    e = Engine()
    ipa.apply_IPA_on_transformer(e, repo_id=adapter_state_dict(3, 48, 64))
    x = torch.zeros(1, 4, 8)
    with pytest.raises(ValueError, match="no image embeddings"):
        e.engine_forward(x, x, x, torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError, match="no image embeddings"):
        e.engine_forward(x, x, x, torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3), ip_hidden_states=[])
    emb = torch.zeros(2, 48)
    assert e.ip_adapter.resolve([emb]) is emb and e.ip_adapter.resolve(emb) is emb
    e.set_ip_hidden_states(emb)
    other = torch.zeros(3, 48)
    assert e.ip_adapter.resolve(None) is emb and e.ip_adapter.resolve([other]) is other  # the call's embeddings come first


def test_teacache_with_an_adapter_is_refused():
    from nunchaku.caching.teacache import TeaCache

    e = Engine()
    ipa.apply_IPA_on_transformer(e, repo_id=adapter_state_dict(3, 48, 64))
    x = torch.zeros(1, 4, 8)
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        e.teacache_forward(x, x, x, torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3), decide=None)
    with pytest.raises(NotImplementedError, match="IP-Adapter"):
        TeaCache(e).__enter__()
    ipa.undo_all_mods_on_transformer(e)
    with TeaCache(e):
        pass


# ---- K/V cache ----------------------------------------------------------------------------------------------------------------------
def test_kv_is_projected_once_per_embeddings_tensor():
    sd = adapter_state_dict(2, 48, 64, seed=4)
    ad = ipa.IPAdapter().load_ip_adapter_weights_per_layer(sd, device="cpu")
    calls = []
    project = ad._project
    ad._project = lambda x: (calls.append(1), project(x))[1]
    emb = torch.randn(1, 2, 5, 48).bfloat16()
    kv = ad.kv(emb)
    assert len(kv) == 2 and all(k.shape == v.shape == (10, 64) for k, v in kv)  # all leading axes are tokens
    w, b = sd[f"{PREFIX}1.processor.ip_adapter_double_stream_v_proj.weight"], sd[f"{PREFIX}1.processor.ip_adapter_double_stream_v_proj.bias"]
    assert torch.equal(kv[1][1], nn.functional.linear(emb.reshape(10, 48), w, b))
    assert ad.kv(emb) is kv and len(calls) == 1  # the second step: the same object, unmodified
    emb.mul_(2)  # an in-place edit bumps the version: projected again
    kv2 = ad.kv(emb)
    assert len(calls) == 2 and kv2 is not kv and not torch.equal(kv2[0][0], kv[0][0])
    same_values = emb.clone()  # another object, even with equal content: projected again (the key is the object)
    ad.kv(same_values)
    assert len(calls) == 3
    with torch.inference_mode():
        inf = torch.randn(3, 48).bfloat16()
    ad.kv(inf), ad.kv(inf)  # no readable version: never cached
    assert len(calls) == 5
    ad.kv(same_values)  # (and the uncached calls left the entry alone)
    assert len(calls) == 5
    ad.load_ip_adapter_weights_per_layer(sd, device="cpu")  # new weights: the entry is dropped
    ad._project = lambda x: (calls.append(1), project(x))[1]
    ad.kv(same_values)
    assert len(calls) == 6


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_header_declares_ip_attention_and_keeps_the_abi_version():
    text = open(os.path.join(ROOT, "include", "svdq_amd.h")).read()
    assert re.search(r"^typedef struct svdq_ip_attention_args \{", text, re.M)
    assert re.search(r"^int svdq_ip_attention\(const svdq_ip_attention_args \*args, void \*stream\);", text, re.M)
    assert re.search(r"^#define SVDQ_ABI_VERSION 24$", text, re.M)
    assert _lib.ABI_VERSION == 24 and "svdq_ip_attention" in _lib.EXPORTS
    from nunchaku_amd import build

    assert "ip_attention.hip" in build.SOURCES


def test_ip_attention_struct_layout_matches_header(built_lib, tmp_path):
    cname, cls = "svdq_ip_attention_args", _lib.IpAttentionArgs
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


def test_ip_attention_exported_and_validation_errors_are_returned(built_lib):
    """every refusal comes back before a launch (there is no GPU here: a launch would be a HIP error, code 3)"""
    lib = _lib.load()
    assert hasattr(C.CDLL(built_lib), "svdq_ip_attention") and lib.svdq_abi_version() == 24
    call = lambda a: (lib.svdq_ip_attention(C.byref(a), None), lib.svdq_last_error())
    assert lib.svdq_ip_attention(None, None) == 1 and b"NULL" in lib.svdq_last_error()

    def good():
        a = _lib.IpAttentionArgs()
        a.q, a.k, a.v, a.out = 4096, 8192, 12288, 16384
        a.ldq, a.ldk, a.ldv, a.ldo = 768, 256, 256, 256
        a.T, a.H, a.N, a.head_dim, a.dtype, a.scale, a.out_scale = 16, 2, 4, 128, 0, 128 ** -0.5, 1.0
        return a

    for ptr in ("q", "k", "v", "out"):
        a = good()
        setattr(a, ptr, None)
        assert call(a) == (1, b"svdq_ip_attention: q, k, v and out are required")
    for n, code in ((0, 1), (-3, 1), (257, 2), (4096, 2)):
        a = good()
        a.N = n
        rc, msg = call(a)
        assert rc == code and b"N=" in msg, (n, msg)
    for field in ("T", "H"):
        a = good()
        setattr(a, field, 0)
        assert call(a)[0] == 1 and b">= 1" in lib.svdq_last_error()
    for ld in ("ldq", "ldk", "ldv", "ldo"):
        a = good()
        setattr(a, ld, 248)  # smaller than the row of H * 128 = 256 elements
        assert call(a)[0] == 1 and b"at least H * 128 = 256" in lib.svdq_last_error()
        setattr(a, ld, 260)  # rows not 16-byte aligned
        assert call(a)[0] == 1 and b"16-byte aligned" in lib.svdq_last_error()
    for ptr in ("q", "k", "v", "out"):
        a = good()
        setattr(a, ptr, getattr(a, ptr) + 8)
        assert call(a)[0] == 1 and b"16-byte aligned" in lib.svdq_last_error()
    a = good()
    a.dtype = 7
    assert call(a)[0] == 1 and b"dtype" in lib.svdq_last_error()
    a = good()
    a.head_dim = 64
    assert call(a)[0] == 2 and b"head_dim=64" in lib.svdq_last_error()
    for s in (0.0, -1.0, float("inf"), float("nan")):
        a = good()
        a.scale = s
        assert call(a)[0] == 1 and b"scale must be positive" in lib.svdq_last_error()
    a = good()
    a.out_scale = float("nan")
    assert call(a)[0] == 1 and b"out_scale" in lib.svdq_last_error()


def test_wrapper_refuses_cpu_tensors_and_mismatched_shapes(built_lib):
    from nunchaku_amd._C import ops
    from nunchaku_amd.ops.attention import ip_attention

    q, k = torch.zeros(16, 2, 128, dtype=torch.bfloat16), torch.zeros(4, 256, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU tensors"):
        ops.ip_attention(q, k, k, torch.zeros_like(q), 0.1)
    with pytest.raises(ValueError, match="share one 16-bit dtype"):
        ops.ip_attention(q, k.half(), k, torch.zeros_like(q), 0.1)
    with pytest.raises(ValueError, match=r"\[T, H, D\] view"):
        ops.ip_attention(q.view(16, 256), k, k, torch.zeros_like(q), 0.1)
    with pytest.raises(ValueError, match="expected q/out"):
        ops.ip_attention(q, k[:, :128], k[:, :128], torch.zeros_like(q), 0.1)
    with pytest.raises(ValueError, match="expected q "):
        ip_attention(torch.zeros(16, 512, dtype=torch.bfloat16), k, k, heads=2)
