"""Self-test of the GEMM error bound of tests/helpers.py on the host: it must ACCEPT an f32-accumulated torch product of the same
operands run through f32 epilogues, and REJECT the references one k term short, at the K values, operand types and epilogues
tests/test_gemm_forms_gpu.py uses.  Nothing here touches the HIP library."""
import pytest
import torch
import torch.nn.functional as F

from helpers import GemmRef, check_gemm, gelu64, gelu_grad64, gelu_operand_err, signed_magnitudes

BF16, F32 = torch.bfloat16, torch.float32
M, N = 192, 136


def products(dtype, K, seed=0):
    x = signed_magnitudes(M, K, seed=seed).to(dtype)
    w = signed_magnitudes(N, K, seed=seed + 1).to(dtype)
    return x, w


@pytest.mark.parametrize('dtype,K', [(BF16, 40), (BF16, 72), (BF16, 96), (BF16, 192), (BF16, 224), (BF16, 256), (BF16, 320), (BF16, 488),
                                     (BF16, 1000), (BF16, 1024), (BF16, 1856), (F32, 112), (F32, 488), (F32, 1000), (F32, 1024)])
def test_bound_accepts_f32_accumulation_and_rejects_a_missing_term(dtype, K):
    x, w = products(dtype, K, seed=K)
    ref = GemmRef(x.double(), w.double())
    acc = x.float() @ w.float().t()                                   # f32 accumulation in torch's order
    g = torch.Generator().manual_seed(K)
    bias, res, pre = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    aux = (torch.randn(M, N, generator=g) * 1.5).to(dtype)
    rs = (torch.rand(M, generator=g) + 0.5)
    low = dtype == BF16
    check_gemm(ref, dtype, {'out': acc.to(dtype)}, 'store', out_bf16=low)
    v = acc + bias
    check_gemm(ref, dtype, {'out': v.to(dtype), 'twin': F.gelu(v).to(dtype)}, 'bias + twin', bias=bias.double(), out_bf16=low, twin=True)
    gp = gelu_grad64(aux.double()).float()
    check_gemm(ref, dtype, {'out': (acc * gp).to(dtype)}, "GELU'", act=2, aux=aux.double(), out_bf16=low)
    check_gemm(ref, dtype, {'out': v * rs[:, None] + res}, 'bias + rowscale + residual', bias=bias.double(), rowscale=rs.double(),
               residual=res.double())
    check_gemm(ref, dtype, {'out': pre + v}, 'add into a pre-filled output', bias=bias.double(), prefill=pre.double())
    check_gemm(ref, dtype, {'out': F.gelu(v).to(dtype)}, 'act = 3', bias=bias.double(), act=3, out_bf16=low)
    half = GemmRef(x.double(), w.double(), alpha=0.5)
    check_gemm(half, dtype, {'out': (acc * 0.5 + bias).to(dtype)}, 'alpha = 0.5', bias=bias.double(), out_bf16=low)


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('K', [64, 72])
@pytest.mark.parametrize('side', ['w_op', 'x_op'])
@pytest.mark.parametrize('drawn', [dict(lo=1.0, hi=1.25, sign=1), dict(lo=0.75, hi=1.0, sign=-1)], ids=['positive', 'negative'])
def test_bound_with_gelu_on_load(dtype, K, side, drawn):
    """the operand GELU is applied to is drawn on one side of zero, as tests/test_gemm_forms_gpu.py draws it (GELU_OPERANDS there
    has the arithmetic): the one-term-short references are then rejected at the same 99 % as everywhere else, the bf16 re-rounding
    term (a bf16 ulp of each of the K transformed values) included"""
    a = signed_magnitudes(M, K, seed=K + 3).to(dtype)                                     # the plain operand
    b = signed_magnitudes(N, K, seed=K + 4, **drawn).to(dtype)                            # the one that goes through GELU
    b64, eb = gelu64(b.double()), gelu_operand_err(b.double(), dtype)
    bt = F.gelu(b.float()).to(dtype).float()                                              # re-rounded to the storage type
    if side == 'w_op':
        ref = GemmRef(a.double(), b64, 1.0, a.double().abs() @ eb.t())
        acc = a.float() @ bt.t()
    else:
        ref = GemmRef(b64, a.double(), 1.0, eb @ a.double().abs().t())
        acc = bt @ a.float().t()
    check_gemm(ref, dtype, {'out': acc}, side)


def test_bound_rejects_what_the_flat_tolerance_accepted():
    """K = 448 with w ~ 0.1 N(0, 1), the last k term missing wherever it is smaller than 2e-2 of the reference's maximum (most of the
    output): max-abs error relative to the maximum lets that through by construction, the derived bound does not"""
    K = 448
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) * 0.1).to(BF16)
    ref = GemmRef(x.double(), w.double())
    term = torch.outer(x.float()[:, -1], w.float()[:, -1])
    small = term.abs() < 1.9e-2 * float(ref.acc.abs().max())
    assert float(small.double().mean()) > 0.75
    right = x.float() @ w.float().t()
    wrong = torch.where(small, right - term, right)
    assert float((wrong.double() - ref.acc).abs().max() / ref.acc.abs().max()) < 2e-2
    check_gemm(ref, BF16, {'out': right}, 'complete', min_rejected=0.0)
    with pytest.raises(AssertionError, match='outside the derived bound'):
        check_gemm(ref, BF16, {'out': wrong}, 'K tail dropped', min_rejected=0.0)
