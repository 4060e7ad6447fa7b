"""fw_gemm at the products the decoder sends it at --embed_dim 32 and 64: the distinct (N, K) of its Linears (fused QKV, proj, LeFF
fc1 / fc2) and of the down- / up-sampling products, at the first stage (C = E, 128 x 128 tokens) and the last (C = 16 E, 8 x 8 tokens) of a
128-pixel image, B = 1, in the three layouts a training step uses:

  fwd    y [M, N] = x [M, K] W[N, K]^T + bias                          ('NT', operand-type output; proj / fc2 also + residual into f32)
  dgrad  dx [M, K] = g [M, N] W[N, K]        through ops.dgrad         ('NN'; fc2 with the GELU' epilogue its backward uses)
  wgrad  dW [N, K] += g [M, N]^T x [M, K]                              ('TN', f32 output, accumulated into a pre-filled buffer)

Each output is held to Product.check's derived bound (tests/helpers.py: (K + 8) 2^-24 |X| |W|^T and the named terms), and the kernel
that ran is asserted against the literal next to the case (fw_gemm_last_kernel) -- for every case, so also for the two forms that
tests/test_gemm_forms_gpu.py does not name: gemm_kernel<float,64,true,true,false,false> and <float,128,true,true,false,false>, the f32
weight gradients.  The first stage is capped at 16 384 + 40 rows: a partial 128-row tile exists.

The missing-term check of Product.check (the bound must tell the output from a reference one k term short at 99 % of the elements)
is asked wherever the reduction is short enough for a term (>= 0.56) to stand clear of the bound: up to RESOLVED_MAX = 1856 terms, the
longest reduction tests/test_gemm_forms_gpu.py asks it at ((K + 8) 2^-24 K E|x w| = 0.21 there, plus 2^-8 |ref| ~ 0.17 for a bf16 output).
Longer reductions -- fc2 and the down-sampling product of the last stage, every weight gradient over 4 096 or 16 424 tokens -- have a bound
that grows with K^2 (1.0 at K = 4096, 16 at K = 16 424): larger than one term by construction of the bound, not of the kernel.  Those
are held to the bound alone (min_rejected = 0).

K = 32 is 64 bytes in bf16, half of the smallest K step: the stream kernel (M >= 32768: the first stage from a batch of 2 on) takes it
in its NCH = 2 class with the second 64-byte chunk zero-filled; test_stream_at_64_and_128_bytes runs that class at K = 32 and 64."""
import pytest
import torch

from test_gemm_forms_gpu import BF16, DEV, F32, Product, Slice, assert_kernel, epilogue_inputs, last_gemm_kernel, ops, padded

pytestmark = pytest.mark.gpu

ROWS0 = 16384 + 40                    # first stage, capped: a partial tile
ROWS4 = 64                            # last stage: one 8 x 8 window
RESOLVED_MAX = 1856                   # longest reduction at which one missing term is asked to show (see above)


def resolving(R):
    return {} if R <= RESOLVED_MAX else dict(min_rejected=0.0)


def shapes(E):
    """[(name, M, N, K)]: the forward products of width E at stages 0 and 4"""
    out = []
    for stage, C, M in ((0, E, ROWS0), (4, 16 * E, ROWS4)):
        out += [(f's{stage}-qkv', M, 3 * C, C), (f's{stage}-proj', M, C, C), (f's{stage}-fc1', M, 4 * C, C), (f's{stage}-fc2', M, C, 4 * C)]
    # dowsample_0: 4 x 4 / 2 convolution as a product over im2col rows (64 x 64 outputs); dowsample_3: 8 x 8 outputs
    out += [('s0-down', 4096, 2 * E, 16 * E), ('s4-down', ROWS4, 16 * E, 128 * E)]
    # upsample_0: 2 x 2 / 2 transposed convolution, 4 C_out columns per input token (64 x 64 inputs); upsample_3: 8 x 8 inputs
    out += [('s0-up', 4096, 4 * E, 4 * E), ('s4-up', ROWS4, 32 * E, 16 * E)]
    return out


# kernel that runs (bf16 fwd, bf16 dgrad, f32 wgrad, bf16 wgrad) per (E, name); literals as FW_KNAME spells them
KERNELS = {
    (32, 's0-qkv', 'fwd'): 'gemm_kernel<bf16,64,false,false,false,false>', (32, 's0-qkv', 'dgrad'): 'gemm_kernel<bf16,64,false,true,false,false>',
    (32, 's0-qkv', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (32, 's0-qkv', 'wgrad bf16'): 'gemm_kernel<bf16,64,true,true,false,false>',
    (32, 's0-proj', 'fwd'): 'gemm_kernel<bf16,64,false,false,false,false>', (32, 's0-proj', 'fwd+res'): 'gemm_kernel<bf16,64,false,false,false,false>',
    (32, 's0-proj', 'dgrad'): 'gemm_kernel<bf16,64,false,true,false,false>', (32, 's0-proj', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>',
    (32, 's0-proj', 'wgrad bf16'): 'gemm_kernel<bf16,64,true,true,false,false>',
    (32, 's0-fc1', 'fwd'): 'gemm_kernel<bf16,64,false,false,false,false>', (32, 's0-fc1', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (32, 's0-fc1', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (32, 's0-fc1', 'wgrad bf16'): 'gemm_kernel<bf16,64,true,true,false,false>',
    (32, 's0-fc2', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (32, 's0-fc2', 'fwd+res'): 'gemm_ring_kernel<bf16,64,2,false>',
    (32, 's0-fc2', 'dgrad'): 'gemm_kernel<bf16,64,false,true,false,false>', (32, 's0-fc2', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>',
    (32, 's0-fc2', 'wgrad bf16'): 'gemm_kernel<bf16,64,true,true,false,false>',
    (32, 's4-qkv', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (32, 's4-qkv', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (32, 's4-qkv', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (32, 's4-qkv', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (32, 's4-proj', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (32, 's4-proj', 'fwd+res'): 'gemm_ring_kernel<bf16,64,2,false>',
    (32, 's4-proj', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>', (32, 's4-proj', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>',
    (32, 's4-proj', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (32, 's4-fc1', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (32, 's4-fc1', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (32, 's4-fc1', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (32, 's4-fc1', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (32, 's4-fc2', 'fwd'): 'gemm_ring_kernel<bf16,64,3,true>', (32, 's4-fc2', 'fwd+res'): 'gemm_ring_kernel<bf16,64,3,false>',
    (32, 's4-fc2', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>', (32, 's4-fc2', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>',
    (32, 's4-fc2', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (32, 's0-down', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (32, 's0-down', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (32, 's0-down', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (32, 's0-down', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (32, 's4-down', 'fwd'): 'gemm_ring_kernel<bf16,64,3,true>', (32, 's4-down', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (32, 's4-down', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (32, 's4-down', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (32, 's0-up', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (32, 's0-up', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (32, 's0-up', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (32, 's0-up', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (32, 's4-up', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (32, 's4-up', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (32, 's4-up', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (32, 's4-up', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (64, 's0-qkv', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's0-qkv', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (64, 's0-qkv', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (64, 's0-qkv', 'wgrad bf16'): 'gemm_kernel<bf16,64,true,true,false,false>',
    (64, 's0-proj', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's0-proj', 'fwd+res'): 'gemm_ring_kernel<bf16,64,2,false>',
    (64, 's0-proj', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>', (64, 's0-proj', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>',
    (64, 's0-proj', 'wgrad bf16'): 'gemm_kernel<bf16,64,true,true,false,false>',
    (64, 's0-fc1', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's0-fc1', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (64, 's0-fc1', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (64, 's0-fc1', 'wgrad bf16'): 'gemm_kernel<bf16,64,true,true,false,false>',
    (64, 's0-fc2', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's0-fc2', 'fwd+res'): 'gemm_ring_kernel<bf16,64,2,false>',
    (64, 's0-fc2', 'dgrad'): 'gemm_tr_ring_kernel<false,64,2,false>', (64, 's0-fc2', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>',
    (64, 's0-fc2', 'wgrad bf16'): 'gemm_kernel<bf16,64,true,true,false,false>',
    (64, 's4-qkv', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's4-qkv', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (64, 's4-qkv', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (64, 's4-qkv', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (64, 's4-proj', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's4-proj', 'fwd+res'): 'gemm_ring_kernel<bf16,64,2,false>',
    (64, 's4-proj', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>', (64, 's4-proj', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>',
    (64, 's4-proj', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (64, 's4-fc1', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's4-fc1', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (64, 's4-fc1', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (64, 's4-fc1', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (64, 's4-fc2', 'fwd'): 'gemm_ring_kernel<bf16,64,3,true>', (64, 's4-fc2', 'fwd+res'): 'gemm_ring_kernel<bf16,64,3,false>',
    (64, 's4-fc2', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>', (64, 's4-fc2', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>',
    (64, 's4-fc2', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (64, 's0-down', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's0-down', 'dgrad'): 'gemm_tr_ring_kernel<false,64,3,true>',
    (64, 's0-down', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (64, 's0-down', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (64, 's4-down', 'fwd'): 'gemm_ring_kernel<bf16,64,3,true>', (64, 's4-down', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (64, 's4-down', 'wgrad f32'): 'gemm_kernel<float,128,true,true,false,false>', (64, 's4-down', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (64, 's0-up', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's0-up', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (64, 's0-up', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (64, 's0-up', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
    (64, 's4-up', 'fwd'): 'gemm_ring_kernel<bf16,64,2,true>', (64, 's4-up', 'dgrad'): 'gemm_kernel<bf16,64,false,true,true,false>',
    (64, 's4-up', 'wgrad f32'): 'gemm_kernel<float,64,true,true,false,false>', (64, 's4-up', 'wgrad bf16'): 'gemm_tr_ring_kernel<true,32,3,false>',
}


def run_case(E, name, M, N, K, ran):
    tag = f'E {E} {name} {M}x{N}x{K}'
    bias, res, aux, rs, rows_per = epilogue_inputs(M, N, BF16, N + K)
    # ---- forward
    p = Product(BF16, 'NT', M, N, K, seed=E + N)
    o = Slice(M, N, BF16)
    p.gemm(out=o.view, bias=bias.to(DEV))
    ran['fwd'] = last_gemm_kernel()
    p.check(f'{tag} fwd', {'out': o.view}, bias=bias.to(DEV, torch.float64), out_bf16=True, **resolving(K))
    o.assert_sentinel(f'{tag} fwd')
    if name.endswith('proj') or name.endswith('fc2'):
        o = Slice(M, N, F32)
        p.gemm(out=o.view, bias=bias.to(DEV), residual=res.to(DEV))
        ran['fwd+res'] = last_gemm_kernel()
        p.check(f'{tag} fwd + residual', {'out': o.view}, bias=bias.to(DEV, torch.float64), residual=res.to(DEV, torch.float64), **resolving(K))
        o.assert_sentinel(f'{tag} fwd + residual')
    del p
    # ---- input gradient: out [M, K] = g [M, N] W [N, K]
    p = Product(BF16, 'NN', M, K, N, seed=E + N + 1)
    o = Slice(M, K, BF16)
    if name.endswith('fc2'):
        _, _, auxk, _, _ = epilogue_inputs(M, K, BF16, K)
        ops().dgrad(p.xd, p.wd, M, K, N, o.view, act=2, aux=padded(auxk.float(), BF16))
        ran['dgrad'] = last_gemm_kernel()
        p.check(f"{tag} dgrad GELU'", {'out': o.view}, act=2, aux=auxk.to(DEV, torch.float64), out_bf16=True, **resolving(N))
    else:
        ops().dgrad(p.xd, p.wd, M, K, N, o.view)
        ran['dgrad'] = last_gemm_kernel()
        p.check(f'{tag} dgrad', {'out': o.view}, out_bf16=True, **resolving(N))
    o.assert_sentinel(f'{tag} dgrad')
    del p
    # ---- weight gradient: dW [N, K] += g [M, N]^T x [M, K], reduction over the M tokens
    pre = torch.randn(N, K, generator=torch.Generator().manual_seed(5))
    for dtype, key in ((F32, 'wgrad f32'), (BF16, 'wgrad bf16')):
        p = Product(dtype, 'TN', N, K, M, seed=E + N + 2)
        o = Slice(N, K, F32, fill=pre.to(DEV))
        p.gemm(out=o.view, accumulate=True)
        ran[key] = last_gemm_kernel()
        p.check(f'{tag} {key}', {'out': o.view}, prefill=pre.to(DEV, torch.float64), **resolving(M))
        o.assert_sentinel(f'{tag} {key}')
        del p


@pytest.mark.parametrize('part', ['s0-linears', 's4-linears', 'sampling'])
@pytest.mark.parametrize('E', [32, 64])
def test_decoder_products(E, part):
    pick = {'s0-linears': lambda n: n.startswith('s0-') and n[3:] in ('qkv', 'proj', 'fc1', 'fc2'),
            's4-linears': lambda n: n.startswith('s4-') and n[3:] in ('qkv', 'proj', 'fc1', 'fc2'),
            'sampling': lambda n: n.endswith('down') or n.endswith('up')}[part]
    names = []
    for name, M, N, K in shapes(E):
        if not pick(name):
            continue
        ran = {}
        run_case(E, name, M, N, K, ran)
        for key, kernel in ran.items():
            print(f"\n    ({E}, '{name}', '{key}'): '{kernel}',", end='')
            names.append(((E, name, key), kernel))
    assert len(names) >= 4 * 4
    wrong = [(k, ran, KERNELS.get(k)) for k, ran in names if KERNELS.get(k) != ran]
    assert not wrong, f'dispatched to another kernel than the case is written for (case, ran, expected): {wrong}'


@pytest.mark.parametrize('K', [32, 64])
def test_stream_at_64_and_128_bytes(K):
    """M = 32768 + 40, N = 3 K (the fused QKV of the first stage): gemm_stream_kernel<bf16, 2, *, *> with half a K step (K = 32: the
    second 64-byte chunk of every X fragment and W panel row is zero-filled) and with exactly one (K = 64)"""
    M, N = 32768 + 40, 3 * K
    bias, res, aux, rs, rows_per = epilogue_inputs(M, N, BF16, K)
    for layout, wt in (('NT', 'false'), ('NN', 'true')):
        p = Product(BF16, layout, M, N, K, seed=K)
        tag = f'stream {layout} K = {K}'
        o = Slice(M, N, BF16)
        p.gemm(out=o.view, bias=bias.to(DEV))
        assert_kernel(f'gemm_stream_kernel<bf16,2,{wt},0>', f'{tag} bias')
        p.check(f'{tag} bias', {'out': o.view}, bias=bias.to(DEV, torch.float64), out_bf16=True)
        o.assert_sentinel(f'{tag} bias')
        o = Slice(M, N, BF16)
        p.gemm(out=o.view, act=2, aux=padded(aux.float(), BF16))
        assert_kernel(f'gemm_stream_kernel<bf16,2,{wt},1>', f"{tag} GELU'")
        p.check(f"{tag} GELU'", {'out': o.view}, act=2, aux=aux.to(DEV, torch.float64), out_bf16=True)
        o.assert_sentinel(f"{tag} GELU'")
        o = Slice(M, N, F32)
        p.gemm(out=o.view, bias=bias.to(DEV), residual=res.to(DEV))
        assert_kernel(f'gemm_stream_kernel<bf16,2,{wt},2>', f'{tag} residual')
        p.check(f'{tag} residual', {'out': o.view}, bias=bias.to(DEV, torch.float64), residual=res.to(DEV, torch.float64))
        o.assert_sentinel(f'{tag} residual')
