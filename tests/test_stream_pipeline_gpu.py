"""gemm_stream_kernel, strip after strip: every wave walks at least four 32-row strips and the last strip of the launch is ragged.

The stream tests of test_gemm_forms_gpu.py and test_ops_gpu.py use M of 33 000 .. 40 000, where each of the launch's waves owns one
strip at most: the code that carries a wave from one strip to the next -- the next strip's X and epilogue operands requested under
the current strip's stores, the counted waits behind them -- never ran in a kernel test.

M: a launch has at most (workgroups resident per CU) x 256 CUs workgroups of 8 waves, split over the column panels, and a strip is
32 rows (STREAM_MTS = 2).  The widest launch is the one of two workgroups per CU and one panel: 512 x 8 waves x 32 rows x 4 strips
= 524 288 rows give every wave four full strips; the instantiations built for one workgroup per CU, and launches of several panels,
have fewer waves and walk more.  40 more rows add one full strip and a ragged one of 8 rows.

Operands, reference and bound are those of test_gemm_forms_gpu.py (helpers.signed_magnitudes, GemmRef, check_gemm: the derived
bound over every element and its one-term-short resolving-power check).  Every case runs into a column slice of a wider,
sentinel-filled buffer with NaN in the operands' row pads, and into a contiguous [M, N] output (ldc == N, the QKV buffer's form).

Which loop a case walks.  The kernel has a straight-line loop of its own (stream_hot_strips) for the full strips of the forms a
training step sends it, and its generic loop for everything else and for the ragged last strip of every launch:
  * hot: k28_n88_bias, k56_n168_bias, k112_n448_bias (staged bf16 store, 2 / 3 / 3+3+1 column blocks), k112_n28_residual,
    k112_n28_rowscale and k28_n28_rowscale (f32 residual with the row scales of proj / fc2: a scale changes every 4096 rows, a wave's
    consecutive strips lie gridDim.x * 256 rows apart, so every strip of a wave reads another scale), k28_n112_dgelu, and
    k88_n56_plain (the W-transposing instantiation of the staged store);
  * generic: k224_n56_rowscale and k224_n56_dgelu (K > 256 bytes with a row-dependent operand: no hot loop is built), k88_n28_plain
    (N % 8 != 0: no staged store).  They walk the same strips through the loop every other form takes."""
import pytest
import torch

from test_gemm_forms_gpu import BF16, DEV, F32, Product, Slice, assert_kernel, padded

pytestmark = pytest.mark.gpu

M = 524288 + 40
ROWS_PER_SCALE = 4096

# (id, layout, K, N, epilogue, kernel).  NT: W stored [N][K] (a Linear's forward); NN: W stored [K][N] (its input gradient).
CASES = [
    ('k28_n88_bias', 'NT', 28, 88, 'bias', 'gemm_stream_kernel<bf16,2,false,0>'),          # partial 16-byte K chunk, second block of 24 columns
    ('k56_n168_bias', 'NT', 56, 168, 'bias', 'gemm_stream_kernel<bf16,2,false,0>'),
    ('k112_n448_bias', 'NT', 112, 448, 'bias', 'gemm_stream_kernel<bf16,4,false,0>'),      # several column panels
    ('k112_n28_residual', 'NT', 112, 28, 'residual', 'gemm_stream_kernel<bf16,4,false,2>'),
    ('k224_n56_rowscale', 'NT', 224, 56, 'rowscale', 'gemm_stream_kernel<bf16,8,false,2>'),
    ('k112_n28_rowscale', 'NT', 112, 28, 'rowscale', 'gemm_stream_kernel<bf16,4,false,2>'),
    ('k28_n28_rowscale', 'NT', 28, 28, 'rowscale', 'gemm_stream_kernel<bf16,2,false,2>'),
    ('k88_n28_plain', 'NN', 88, 28, 'plain', 'gemm_stream_kernel<bf16,4,true,0>'),
    ('k88_n56_plain', 'NN', 88, 56, 'plain', 'gemm_stream_kernel<bf16,4,true,0>'),
    ('k28_n112_dgelu', 'NN', 28, 112, 'dgelu', 'gemm_stream_kernel<bf16,2,true,1>'),
    ('k224_n56_dgelu', 'NN', 224, 56, 'dgelu', 'gemm_stream_kernel<bf16,8,true,1>'),
]


def device_randn(shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV) * scale


@pytest.mark.parametrize('layout,K,N,epilogue,kernel', [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_stream_strip_walk(layout, K, N, epilogue, kernel):
    p = Product(BF16, layout, M, N, K, seed=K + N)
    call, expect = {}, {}
    out_dtype = F32 if epilogue in ('residual', 'rowscale') else BF16
    if epilogue in ('bias', 'residual', 'rowscale'):
        bias = device_randn(N, 1)
        call['bias'], expect['bias'] = bias, bias.double()
    if epilogue in ('residual', 'rowscale'):
        res = device_randn((M, N), 2)
        call['residual'], expect['residual'] = padded(res, F32), res.double()
    if epilogue == 'rowscale':
        g = torch.Generator(device=DEV).manual_seed(3)
        rs = torch.rand((M + ROWS_PER_SCALE - 1) // ROWS_PER_SCALE, generator=g, device=DEV) + 0.5
        call['rowscale'], call['rows_per_scale'] = rs, ROWS_PER_SCALE
        expect['rowscale'] = rs.double().repeat_interleave(ROWS_PER_SCALE)[:M]
    if epilogue == 'dgelu':
        aux = device_randn((M, N), 4, 1.5).to(BF16)                   # beyond +-4 now and then: the polynomial's clamp
        call['act'], call['aux'] = 2, padded(aux, BF16)
        expect['act'], expect['aux'] = 2, aux.double()
    if out_dtype == BF16:
        expect['out_bf16'] = True

    o = Slice(M, N, out_dtype)
    p.gemm(out=o.view, **call)
    assert_kernel(kernel, 'slice of a wider buffer')
    p.check(f'{layout} {K} x {N} {epilogue}, slice of a wider buffer', {'out': o.view}, **expect)
    o.assert_sentinel(f'{layout} {K} x {N} {epilogue}')
    del o

    flat = torch.full((M, N), float('nan'), dtype=out_dtype, device=DEV)
    p.gemm(out=flat, **call)
    assert_kernel(kernel, 'contiguous output')
    p.check(f'{layout} {K} x {N} {epilogue}, contiguous output', {'out': flat}, **expect)
