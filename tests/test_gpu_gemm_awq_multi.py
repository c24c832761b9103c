"""``ops.gemm_awq_multi`` (svdq_gemm_awq_multi) on the GPU: CONCAT bit for bit against separate ``gemm_awq`` launches and, where it splits K,
against float64; GATED against ``round16(round16(gelu_new_f64(g)) * u)`` on the two GEMMs' own outputs; the refusals."""
import math

import pytest
import torch

from nunchaku_amd import _lib
from nunchaku_amd.models.text_encoders import W4Linear
from nunchaku_amd.models.text_encoders.tinychat_utils import _pack_codes
from nunchaku_amd.ops import gemm_awq_multi
from tests.test_awq_gemm_host import dequantise
from tests.test_gpu_awq_gemm import DT, assert_close_16, gemm, make_layer

pytestmark = pytest.mark.gpu
K = 512  # four K-steps: no plan can split
MS = [1, 33, 130]


def make_sets(Ns, k, dtype, bias=False):
    g = torch.Generator(device="cuda").manual_seed(sum(Ns))
    return [(*make_layer(N, k, DT[dtype], seed=11 * i + N), torch.randn(N, device="cuda", generator=g).to(DT[dtype]) if bias else None)
            for i, N in enumerate(Ns)]


def rand_x(M, k, dtype, scale=1.0):
    return (torch.randn(M, k, device="cuda", generator=torch.Generator(device="cuda").manual_seed(M)) * scale).to(DT[dtype])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "column-slice"])
@pytest.mark.parametrize("Ns", [(256, 256, 256), (192, 64, 320), (64,)])
@pytest.mark.parametrize("M", MS)
def test_concat_is_bit_equal_to_separate_launches(M, Ns, sliced, bias, dtype):
    sets, x = make_sets(Ns, K, dtype, bias), rand_x(M, K, dtype)
    assert _lib.load().svdq_gemm_awq_multi_workspace_bytes(M, sum(Ns), K, _lib.AWQ_MULTI_CONCAT) == 0
    if sliced:
        buf = torch.full((M, sum(Ns) + 72), float("nan"), dtype=DT[dtype], device="cuda")
        out = gemm_awq_multi(x, sets, "concat", out=buf[:, 8:8 + sum(Ns)])
        assert buf[:, :8].isnan().all() and buf[:, 8 + sum(Ns):].isnan().all()
    else:
        out = gemm_awq_multi(x, sets)
    off = 0
    for qw, sc, zr, b in sets:
        N = qw.shape[0] * 4
        assert torch.equal(out[:, off:off + N], gemm(x, qw, sc, zr, bias=b)), (off, N)
        off += N


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_concat_with_a_k_split_against_float64_and_itself(dtype):
    M, k, Ns = 8, 2048, (256, 256, 256)
    assert _lib.load().svdq_gemm_awq_multi_workspace_bytes(M, sum(Ns), k, _lib.AWQ_MULTI_CONCAT) > 0  # this shape splits
    sets, x = make_sets(Ns, k, dtype, bias=True), rand_x(M, k, dtype)
    out, again = gemm_awq_multi(x, sets), gemm_awq_multi(x, sets)
    assert torch.equal(out, again)
    ref = torch.cat([((x.double() @ dequantise(qw, sc, zr, k).cuda().double().t()).to(DT[dtype]) + b) for qw, sc, zr, b in sets], dim=1)
    assert_close_16(out.float().cpu().numpy(), ref.float().cpu().numpy(), dtype, f"gemm_awq_multi concat {M}x{Ns}x{k}", max_bad_frac=2e-3)


def gelu_new_f64(g):
    """0.5 g (1 + tanh(z)), z = sqrt(2/pi) (g + 0.044715 g^3), as the identical g / (1 + exp(-2z)): in float64 ``1 + tanh(z)`` cancels for
    g below about -6 (30 % off at g = -7) and would not be a reference there"""
    return g / (1.0 + torch.exp(-2.0 * math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)))


def r16(x, dt):
    """float64 -> the 16-bit dtype in ONE rounding, as float64.  torch converts through float32, which rounds twice (0.225402838 lies 6e-9 above
    a float16 midpoint that is a float32: it lands on the midpoint, then on the even neighbour below); so: float32 rounded to odd first."""
    f = x.float()
    bits = f.view(torch.int32) - (f.double().abs() > x.abs()).int()  # towards zero
    f = torch.where(f.double() == x, f, (bits | 1).view(torch.float32))
    return f.to(dt).double()


def check_gated(out, g, u, dtype):
    """bit-equal wherever the activation bound stated in include/svdq_amd.h cannot move the activation's 16-bit rounding, elsewhere within one
    16-bit ulp of the product; returns the share of excused elements.  The bound is taken twice: the float64 reference carries it as well."""
    dt, (mant, emin) = DT[dtype], (7, -126) if dtype == "bf16" else (10, -14)
    g, u, got = g.double().cpu(), u.double().cpu(), out.double().cpu()
    act = gelu_new_f64(g)
    a = -2.0 * math.sqrt(2.0 / math.pi) * (g + 0.044715 * g ** 3)
    bound = 2 * (act.abs() * (8 + 8 * a.clamp(min=1.0)) * 2.0 ** -53 + g.abs() * 2.0 ** -126)
    strict = r16(act - bound, dt) == r16(act + bound, dt)
    want = r16(r16(act, dt) * u, dt)
    ulp = torch.exp2((torch.frexp(want)[1].double() - 1).clamp(min=emin) - mant)
    off = ((got - want).abs() / ulp)[~strict]
    print(f"excused {off.numel()} of {got.numel()}, of them beyond one ulp of the product: {(off > 1).sum().item()} (max {off.max().item() if off.numel() else 0:.1f} ulps)")
    assert torch.equal(got[strict], want[strict])
    assert (off <= 1).all()
    return 1.0 - strict.double().mean().item()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("N", [64, 640])
@pytest.mark.parametrize("M", MS)
def test_gated_gelu_new_against_the_two_gemms(M, N, dtype):
    sets, x = make_sets((N, N), K, dtype, bias=N == 64), rand_x(M, K, dtype, scale=0.5)
    out = gemm_awq_multi(x, sets, "gated_gelu_new")
    assert out.shape == (M, N) and torch.equal(out, gemm_awq_multi(x, sets, "gated_gelu_new"))
    g, u = (gemm(x, qw, sc, zr, bias=b) for qw, sc, zr, b in sets)
    excused = check_gated(out, g, u, dtype)
    print(f"gated {M}x{N} {dtype}: {excused:.4%} of the elements excused from bit equality")
    assert excused < 0.02


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_gated_constructed_rows_give_exact_zeros_and_pass_through(dtype):
    """gate weights 0.5 q - 2 (zero but for column 0), value weights q - 1 (zero but for column 128); x has one entry in each of the two
    columns: g = x[m, 0] * {0, 0.5, -0.5}, u = {1, -1}"""
    N, dt = 64, DT[dtype]
    n = torch.arange(N, device="cuda")
    gate_codes, value_codes = torch.full((N, K), 4, device="cuda"), torch.full((N, K), 1, device="cuda")
    gate_codes[:, 0], value_codes[:, 128] = 4 + (n % 3) - 3 * (n % 3 == 2), 2 * ((n // 3) % 2)
    const = lambda v: torch.full((K // 128, N), v, dtype=dt, device="cuda")
    sets = [(_pack_codes(gate_codes), const(0.5), const(-2.0), None), (_pack_codes(value_codes), const(1.0), const(-1.0), None)]
    x = torch.zeros(2, K, dtype=dt, device="cuda")
    x[:, 128], x[0, 0], x[1, 0] = 1.0, 1.0, 60.0
    out = gemm_awq_multi(x, sets, "gated_gelu_new")
    g, u = (gemm(x, qw, sc, zr) for qw, sc, zr, _ in sets)
    assert set(g[0].tolist()) == {0.0, 0.5, -0.5} and set(g[1].tolist()) == {0.0, 30.0, -30.0} and set(u.flatten().tolist()) == {1.0, -1.0}
    check_gated(out, g, u, dtype)
    assert (out[g <= 0][g[g <= 0] != -0.5] == 0).all()            # g = 0 and g = -30: exact zeros
    assert torch.equal(out[1][g[1] == 30], 30 * u[1][g[1] == 30])  # g = 30: u passes through
    want = r16(gelu_new_f64(torch.tensor(0.5, dtype=torch.float64)), dt).to(dt)
    assert torch.equal(out[0][g[0] == 0.5], want * u[0][g[0] == 0.5])


def test_refusals_come_before_a_launch():
    x = rand_x(4, K, "bf16")
    L = lambda N: (*make_layer(N, K, torch.bfloat16), None)
    with pytest.raises(ValueError, match="two sets of equal N"):
        gemm_awq_multi(x, [L(64), L(128)], "gated_gelu_new")
    with pytest.raises(ValueError, match="multiple of 64"):
        gemm_awq_multi(x, [L(64), L(32)])
    with pytest.raises(NotImplementedError, match="group_size=64"):
        gemm_awq_multi(x, [W4Linear(K, 64, group_size=64, dtype=torch.bfloat16, device="cuda")])
    with pytest.raises(ValueError, match="4 weight sets"):
        gemm_awq_multi(x, [L(64)] * 4)
    with pytest.raises(ValueError, match="mode"):
        gemm_awq_multi(x, [L(64)], "gated_relu")
