"""Every kernel form fw_gemm's dispatch can reach, each checked two ways:

1. the NAME of the kernel that ran (fw_gemm_last_kernel, read on the calling thread directly after the call) against a literal
   written next to the case -- a moved threshold fails here, and the message says which kernel ran instead;
2. every output element against a float64 torch product of the same storage-rounded operands, within the bound DERIVED from the
   operation (tests/helpers.py: (K + 8) 2^-24 |alpha| |X| |W|^T, widened only by named terms: bf16 output rounding, the stated
   GELU / GELU' approximation errors).  No constant comes from a run of the kernels.

The bound's resolving power is part of every case: the same kernel output is compared with the reference ONE k TERM SHORT (the last
k, and one in the middle of the last 128-byte K step) and the bound must reject that at >= 99 % of the elements.  Operands are
random-sign values of magnitude [0.75, 1.25) so that a single term (>= 0.56) stands clear of the bound at every K used here.  An
epilogue that is not linear in the sum (v * GELU'(aux), the GELU twin) hides a change of the sum where its own derivative is small;
there the 99 % is asked of the elements whose gain |d out / d sum| is at least 0.5 (the gain comes from the reference), these must
be at least 40 % of the output, and a failure states their share.  The main bound checks every element in every case.

Outputs are column slices of wider buffers pre-filled with a sentinel that must survive; operand row pads hold NaN.
Every M stays below 32768 except in test_stream_forms: the stream kernel's instantiations are among those a training step runs, and
only a product with M >= 32768 can name them (test_ops_gpu.py::test_gemm_stream_tall_skinny covers that kernel's edges)."""
import ctypes

import pytest
import torch

from helpers import GemmRef, check_gemm, gelu64, gelu_operand_err, signed_magnitudes

pytestmark = pytest.mark.gpu

DEV = 'cuda'
F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -77.0                      # exact in bf16
# Operands that go through GELU on load (x_op / w_op = 1), one draw on each side of zero.  In bf16 each of the K re-rounded values
# GELU(w) adds a bf16 ulp of itself times |x| to the bound, 2^-7 E|x| E|GELU(w)| a term with E|x| = 1:
#   w in [1, 1.25):     GELU(w) in [0.84, 1.12],    0.0077 a term, 0.55 at K = 72; every k term is >= 0.75 * 0.84  = 0.63
#   w in (-1, -0.75]:  |GELU(w)| in [0.159, 0.170], 0.0013 a term, 0.10 at K = 72; every k term is >= 0.75 * 0.159 = 0.119
# so a missing term stands clear of the bound in both; the signs of the sum come from the other operand.  (One draw of both signs
# would not do: a term of 0.12 hides under the re-rounding of positive values in the other 63.)
GELU_OPERANDS = {'positive': dict(lo=1.0, hi=1.25, sign=1), 'negative': dict(lo=0.75, hi=1.0, sign=-1)}


def ops():
    from fwair import ops as _ops
    return _ops


def last_gemm_kernel():
    """name of the kernel this thread's last fw_gemm call launched, as FW_KNAME spells it"""
    from fwair.lib import lib
    buf = ctypes.create_string_buffer(128)
    n = lib().fw_gemm_last_kernel(buf, 128)
    assert n >= 0
    return buf.value.decode()


def assert_kernel(expected, what):
    ran = last_gemm_kernel()
    assert ran == expected, f'{what}: dispatched to {ran}, this case is written for {expected}'


def padded(t, dtype, fill=float('nan')):
    """[rows, cols] host tensor -> device view [:, :cols] of a buffer whose rows are 16-byte aligned and end in `fill`"""
    rows, cols = t.shape
    ld = (cols + 7) // 8 * 8 + 8
    buf = torch.full((rows, ld), fill, dtype=dtype, device=DEV)
    buf[:, :cols] = t.to(DEV, dtype)
    return buf[:, :cols]


class Slice:
    """[M, N] output as a column slice of a wider, sentinel-filled buffer (8 columns each side: the slice stays 16-byte aligned)"""

    def __init__(self, M, N, dtype, fill=None):
        self.buf = torch.full((M, N + 16), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[:, 8:8 + N]
        if fill is not None:
            self.view.copy_(fill)

    def assert_sentinel(self, what):
        N = self.view.shape[1]
        left, right = self.buf[:, :8].float(), self.buf[:, 8 + N:].float()
        assert bool((left == SENTINEL).all()) and bool((right == SENTINEL).all()), f'{what}: columns outside the output slice were written'


class Product:
    """operands of one product in the layout a case asks for, on the device, and its float64 reference (torch on the device:
    independent of the library)"""

    def __init__(self, dtype, layout, M, N, K, seed=0, alpha=1.0, w_op=0, x_op=0, gelu_operand='positive'):
        self.dtype, self.M, self.N, self.K = dtype, M, N, K
        # logical X [M, K], W [N, K], rounded to the storage type
        drawn = GELU_OPERANDS[gelu_operand]
        x = signed_magnitudes(M, K, seed=seed, **(drawn if x_op else {})).to(dtype)
        w = signed_magnitudes(N, K, seed=seed + 1, **(drawn if w_op else {})).to(dtype)
        self.x_trans, self.w_trans = layout[0] == 'T', layout[1] == 'N'
        self.xd = padded(x.t() if self.x_trans else x, dtype)
        self.wd = padded(w.t() if self.w_trans else w, dtype)
        x64, w64 = x.to(DEV, torch.float64), w.to(DEV, torch.float64)
        operand_err = None
        if w_op or x_op:                                                 # GELU on load: the reference applies the exact function
            ex = gelu_operand_err(x64, dtype) if x_op else torch.zeros_like(x64)
            ew = gelu_operand_err(w64, dtype) if w_op else torch.zeros_like(w64)
            x64 = gelu64(x64) if x_op else x64
            w64 = gelu64(w64) if w_op else w64
            operand_err = abs(alpha) * (ex @ (w64.abs() + ew).t() + x64.abs() @ ew.t())
        self.ref = GemmRef(x64, w64, alpha, operand_err)

    def gemm(self, **kw):
        return ops().gemm(self.xd, self.wd, self.M, self.N, self.K, x_trans=self.x_trans, w_trans=self.w_trans, **kw)

    def check(self, what, outputs, **kw):
        check_gemm(self.ref, self.dtype, outputs, what, **kw)


def epilogue_inputs(M, N, dtype, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    aux = (torch.randn(M, N, generator=g) * 1.5).to(dtype)                # beyond +-4 now and then: the polynomial's clamp
    rows_per = 100
    rs = torch.rand((M + rows_per - 1) // rows_per, generator=g) + 0.5
    return bias, res, aux, rs, rows_per


def run_five_epilogues(p, k_plain, k_epi, tag):
    """plain store; bias into an output of the operand type (staged mode 0 where eligible); the GELU twin (mode 1); v * GELU'(aux) with
    aux and output in the operand type (mode 2); bias + rowscale + residual into f32 (the direct epilogue)"""
    M, N, dtype = p.M, p.N, p.dtype
    bias, res, aux, rs, rows_per = epilogue_inputs(M, N, dtype, M + N)
    bias_d, res_d, rs_d = bias.to(DEV), res.to(DEV), rs.to(DEV)
    bias64 = bias_d.double()
    low = dtype == BF16

    o = Slice(M, N, dtype)
    p.gemm(out=o.view)
    assert_kernel(k_plain, f'{tag} store')
    p.check(f'{tag} store', {'out': o.view}, out_bf16=low)
    o.assert_sentinel(f'{tag} store')

    o = Slice(M, N, dtype)
    p.gemm(out=o.view, bias=bias_d)
    assert_kernel(k_plain, f'{tag} bias')
    p.check(f'{tag} bias', {'out': o.view}, bias=bias64, out_bf16=low)
    o.assert_sentinel(f'{tag} bias')

    o, t = Slice(M, N, dtype), Slice(M, N, dtype)
    p.gemm(out=o.view, bias=bias_d, out_gelu=t.view)
    assert_kernel(k_epi, f'{tag} GELU twin')
    p.check(f'{tag} GELU twin', {'out': o.view, 'twin': t.view}, bias=bias64, out_bf16=low, twin=True)
    o.assert_sentinel(f'{tag} GELU twin'); t.assert_sentinel(f'{tag} GELU twin (second output)')

    o = Slice(M, N, dtype)
    p.gemm(out=o.view, act=2, aux=padded(aux.float(), dtype))
    assert_kernel(k_epi, f"{tag} GELU'")
    p.check(f"{tag} GELU'", {'out': o.view}, act=2, aux=aux.to(DEV, torch.float64), out_bf16=low)
    o.assert_sentinel(f"{tag} GELU'")

    o = Slice(M, N, F32)
    p.gemm(out=o.view, bias=bias_d, rowscale=rs_d, rows_per_scale=rows_per, residual=res_d)
    assert_kernel(k_epi, f'{tag} bias+rowscale+residual')
    p.check(f'{tag} bias+rowscale+residual', {'out': o.view}, bias=bias64,
            rowscale=rs_d.double().repeat_interleave(rows_per)[:M], residual=res_d.double())
    o.assert_sentinel(f'{tag} bias+rowscale+residual')


# (id, dtype, layout, (M, N, K), kernel of a plain store, kernel of an epilogue with operands of its own).
# layout, first letter: N = X stored [M][K], T = X stored [K][M] (x_trans); second letter: T = W stored [N][K], N = W stored [K][N] (w_trans).
# N % 8 == 0 lets the bf16 epilogue go through LDS (staged); its twin with N % 8 == 4 takes the direct epilogue of the same kernel.
BIG_TILE_CASES = [
    # 3 x 65 = 195 tiles of 256 x 256, ragged both ways; N >= 16384 is what selects the 8-wave kernel
    ('big-nt', BF16, 'NT', (520, 16392, 256), 'gemm_big_kernel<false,true>', 'gemm_big_kernel<false,false>'),
    ('big-nt-n4', BF16, 'NT', (520, 16388, 256), 'gemm_big_kernel<false,true>', 'gemm_big_kernel<false,false>'),
    ('big-nn', BF16, 'NN', (520, 16392, 256), 'gemm_big_kernel<true,true>', 'gemm_big_kernel<true,false>'),
    # 9 x 19 = 171 tiles
    ('wide-nt', BF16, 'NT', (2100, 4616, 320), 'gemm_wide_kernel<false,true>', 'gemm_wide_kernel<false,false>'),
    ('wide-nt-n4', BF16, 'NT', (2100, 4612, 320), 'gemm_wide_kernel<false,true>', 'gemm_wide_kernel<false,false>'),
    ('wide-nn', BF16, 'NN', (2100, 4616, 320), 'gemm_wide_kernel<true,true>', 'gemm_wide_kernel<true,false>'),
    ('wide-nn-n4', BF16, 'NN', (2100, 4612, 320), 'gemm_wide_kernel<true,true>', 'gemm_wide_kernel<true,false>'),
    # 29 K steps of 64: the three-stage ring of the 128 x 64 tile
    ('ring64x3', BF16, 'NT', (300, 200, 1856), 'gemm_ring_kernel<bf16,64,3,true>', 'gemm_ring_kernel<bf16,64,3,false>'),
    ('ring64x3-n4', BF16, 'NT', (300, 204, 1856), 'gemm_ring_kernel<bf16,64,3,true>', 'gemm_ring_kernel<bf16,64,3,false>'),
    # 5 K steps (odd): the two-stage ring of the 128 x 64 tile
    ('ring64x2', BF16, 'NT', (300, 200, 320), 'gemm_ring_kernel<bf16,64,2,true>', 'gemm_ring_kernel<bf16,64,2,false>'),
    # 516 tiles of 128 x 128 but only 130 of 256 x 256
    ('ring128x2', BF16, 'NT', (16400, 392, 320), 'gemm_ring_kernel<bf16,128,2,true>', 'gemm_ring_kernel<bf16,128,2,false>'),
    # K a whole number of 64-byte steps only
    ('ring64b-f32', F32, 'NT', (16400, 392, 112), 'gemm_ring64_kernel<float,128,3,true>', 'gemm_ring64_kernel<float,128,3,false>'),
    ('ring64b-bf16', BF16, 'NT', (6200, 1000, 96), 'gemm_ring64_kernel<bf16,128,3,true>', 'gemm_ring64_kernel<bf16,128,3,false>'),
    # W stored [K][N], read with transposing LDS reads.  26 x 8 = 208 tiles; K < 256 keeps them off the 256 x 256 kernels
    ('tr-208', BF16, 'NN', (3300, 1000, 192), 'gemm_tr_ring_kernel<false,64,3,true>', 'gemm_tr_ring_kernel<false,64,2,false>'),
    ('tr-208-n4', BF16, 'NN', (3300, 1004, 192), 'gemm_tr_ring_kernel<false,64,3,true>', 'gemm_tr_ring_kernel<false,64,2,false>'),
    # 33 x 8 = 264 tiles: more blocks than CUs, a plain store takes the 32-deep form
    ('tr-264', BF16, 'NN', (4200, 1000, 192), 'gemm_tr_ring_kernel<false,32,3,true>', 'gemm_tr_ring_kernel<false,64,2,false>'),
    # K = 224: a multiple of 32 only
    ('tr-k224', BF16, 'NN', (3300, 1000, 224), 'gemm_tr_ring_kernel<false,32,3,true>', 'gemm_tr_ring_kernel<false,32,3,false>'),
    ('tr-k224-n4', BF16, 'NN', (3300, 1004, 224), 'gemm_tr_ring_kernel<false,32,3,true>', 'gemm_tr_ring_kernel<false,32,3,false>'),
    # the register-staged tile kernel: 128 x 128 tiles (392 of them), and the 128 x 64 forms with and without direct staging of X
    ('tile128-nn', BF16, 'NN', (6200, 1000, 72), 'gemm_kernel<bf16,128,false,true,false,false>', 'gemm_kernel<bf16,128,false,true,false,false>'),
    ('tile64-nt', BF16, 'NT', (300, 72, 40), 'gemm_kernel<bf16,64,false,false,false,false>', 'gemm_kernel<bf16,64,false,false,false,false>'),
    ('tile64-nn', BF16, 'NN', (300, 72, 40), 'gemm_kernel<bf16,64,false,true,false,false>', 'gemm_kernel<bf16,64,false,true,false,false>'),
    ('tile64-nn-gx', BF16, 'NN', (300, 72, 128), 'gemm_kernel<bf16,64,false,true,true,false>', 'gemm_kernel<bf16,64,false,true,true,false>'),
]


@pytest.mark.parametrize('cid,dtype,layout,shape,k_plain,k_epi', BIG_TILE_CASES, ids=[c[0] for c in BIG_TILE_CASES])
def test_tile_forms(cid, dtype, layout, shape, k_plain, k_epi):
    M, N, K = shape
    assert M < 32768
    p = Product(dtype, layout, M, N, K, seed=len(cid))
    run_five_epilogues(p, k_plain, k_epi, f'{cid} {layout} {M}x{N}x{K}')


# products with X stored [K][M]: dW = dY^T x and its kin.  A plain store into f32 and / or an add into what the output already holds.
XT_CASES = [
    # x_trans, W k-contiguous: K = 1024 is a whole number of 128-byte steps (W staged directly), K = 1000 is not
    ('xt-k1000-bf16', BF16, 'TT', (168, 56, 1000), ('store', 'add'), 'gemm_kernel<bf16,64,true,false,false,false>'),
    ('xt-k1024-bf16', BF16, 'TT', (168, 56, 1024), ('store', 'add'), 'gemm_kernel<bf16,64,true,false,false,true>'),
    ('xt-k1000-f32', F32, 'TT', (168, 56, 1000), ('store', 'add'), 'gemm_kernel<float,64,true,false,false,false>'),
    ('xt-k1024-f32', F32, 'TT', (168, 56, 1024), ('store', 'add'), 'gemm_kernel<float,64,true,false,false,true>'),
    # both token-major: the register-transposing tile kernel (K not a multiple of 64) and the transposing-read ring
    ('tn-k1000', BF16, 'TN', (168, 56, 1000), ('store', 'add'), 'gemm_kernel<bf16,64,true,true,false,false>'),
    ('tn-ring-store', BF16, 'TN', (168, 56, 1024), ('store',), 'gemm_tr_ring_kernel<true,32,3,true>'),
    ('tn-ring-add', BF16, 'TN', (168, 56, 1024), ('add',), 'gemm_tr_ring_kernel<true,32,3,false>'),
]


@pytest.mark.parametrize('cid,dtype,layout,shape,epilogues,kernel', XT_CASES, ids=[c[0] for c in XT_CASES])
def test_x_trans_forms(cid, dtype, layout, shape, epilogues, kernel):
    M, N, K = shape
    p = Product(dtype, layout, M, N, K, seed=len(cid))
    tag = f'{cid} {M}x{N}x{K}'
    if 'store' in epilogues:
        o = Slice(M, N, F32)
        p.gemm(out=o.view)
        assert_kernel(kernel, f'{tag} store')
        p.check(f'{tag} store', {'out': o.view})
        o.assert_sentinel(f'{tag} store')
    if 'add' in epilogues:
        pre = torch.randn(M, N, generator=torch.Generator().manual_seed(5))
        o = Slice(M, N, F32, fill=pre.to(DEV))
        p.gemm(out=o.view, accumulate=True)
        assert_kernel(kernel, f'{tag} add')
        p.check(f'{tag} add', {'out': o.view}, prefill=pre.to(DEV, torch.float64))
        o.assert_sentinel(f'{tag} add')


@pytest.mark.parametrize('dtype,tn', [(BF16, 'bf16'), (F32, 'float')], ids=['bf16', 'f32'])
def test_argument_values(dtype, tn):
    """w_op = 1, act = 3, alpha != 1 and split-K atomics into a pre-filled buffer on a non-transposed product.  K = 488: 8 steps of 64
    (16 of 32 in f32) with a ragged last one, so four K slices are all non-empty and the last is short."""
    M, N, K = 200, 72, 488
    tile = f'gemm_kernel<{tn},64,false,false,false,false>'
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3)).to(DEV)
    low = dtype == BF16

    # GELU on load: K = 72 (one 128-byte step and a tail) and K = 64 (one whole step: the OTHER operand is then staged directly, the
    # GX / GW forms).  These K keep the re-rounding term of the bf16 bound below a single k term (see GELU_OPERANDS).
    for Kop, kw, name in ((72, dict(w_op=1), tile), (64, dict(w_op=1), f'gemm_kernel<{tn},64,false,false,true,false>'),
                          (64, dict(x_op=1), f'gemm_kernel<{tn},64,false,false,false,true>')):
        for side in GELU_OPERANDS:
            p = Product(dtype, 'NT', M, N, Kop, seed=11 + Kop, gelu_operand=side, **kw)
            o = Slice(M, N, F32)
            p.gemm(out=o.view, **kw)
            assert_kernel(name, f'K = {Kop} {kw} {side}')
            p.check(f'K = {Kop} {kw} {side}', {'out': o.view})
            o.assert_sentinel(f'K = {Kop} {kw} {side}')

    p = Product(dtype, 'NT', M, N, K, seed=13)
    o = Slice(M, N, dtype)
    p.gemm(out=o.view, bias=bias, act=3)
    assert_kernel(tile, 'act = 3')
    p.check('act = 3', {'out': o.view}, bias=bias.double(), act=3, out_bf16=low)
    o.assert_sentinel('act = 3')

    p = Product(dtype, 'NT', M, N, K, seed=14, alpha=0.5)
    o = Slice(M, N, dtype)
    p.gemm(out=o.view, bias=bias, alpha=0.5)
    assert_kernel(tile, 'alpha = 0.5')
    p.check('alpha = 0.5', {'out': o.view}, bias=bias.double(), out_bf16=low)
    o.assert_sentinel('alpha = 0.5')

    p = Product(dtype, 'NT', M, N, K, seed=15)
    pre = torch.randn(M, N, generator=torch.Generator().manual_seed(6))
    o = Slice(M, N, F32, fill=pre.to(DEV))
    p.gemm(out=o.view, bias=bias, accumulate=True, splitk=4)
    assert_kernel(tile, 'split-K atomics')
    p.check('split-K atomics', {'out': o.view}, bias=bias.double(), prefill=pre.to(DEV, torch.float64))
    o.assert_sentinel('split-K atomics')


@pytest.mark.parametrize('dtype,kernel', [(BF16, 'gemm_kernel<bf16,64,false,true,true,false>'), (F32, 'gemm_kernel<float,64,false,true,true,false>')],
                         ids=['bf16', 'f32'])
def test_dgrad_slices_on_the_tile_kernel(dtype, kernel):
    """ops.dgrad with few output tiles: two slices of the reduction, each a partial tile at its own c_zstride offset, on the tile
    kernel that transposes W in registers; folded by the slab reduce and cast into a column slice."""
    M, K, N = 130, 136, 1024                   # out [M, K] = g [M, N] W [N, K]
    p = Product(dtype, 'NN', M, K, N, seed=21)
    o = Slice(M, K, dtype)
    ops().dgrad(p.xd, p.wd, M, K, N, o.view)
    assert_kernel(kernel, 'dgrad')
    p.check('dgrad', {'out': o.view}, out_bf16=dtype == BF16)
    o.assert_sentinel('dgrad')


def test_k_slices_on_the_ring_kernel():
    """Two slices of the reduction on the LDS-DMA ring (the split-K order of the tile walk, 3 x 4 x 2 workgroups: an x extent that is
    no multiple of 8), each a partial tile stored into its own f32 slab at c_zstride.  fw_gemm cuts K = 1856 = 29 steps of 64 into
    slices of ceil(29 / 2) = 15 steps: k < 960 and k >= 960; 15 steps are below the 28 that select the three-stage ring."""
    M, N, K, split = 300, 200, 1856, 2
    kper = 15 * 64
    p = Product(BF16, 'NT', M, N, K, seed=22)
    slabs = torch.full((split, M, N + 16), SENTINEL, dtype=F32, device=DEV)
    p.gemm(out=slabs[0, :, 8:8 + N], splitk=split, c_zstride=M * (N + 16))
    assert_kernel('gemm_ring_kernel<bf16,64,2,true>', 'K slices')
    for z in range(split):
        part = GemmRef(p.ref.x[:, z * kper:(z + 1) * kper], p.ref.w[:, z * kper:(z + 1) * kper])
        check_gemm(part, BF16, {'out': slabs[z, :, 8:8 + N]}, f'K slice {z}')
        outside = torch.cat([slabs[z, :, :8], slabs[z, :, 8 + N:]], 1)
        assert bool((outside == SENTINEL).all()), f'K slice {z}: columns outside the output slice were written'


# gemm_stream_kernel<T, NCH, WT, EXT>: NCH from K (128, 256, 512 bytes), EXT 1 = GELU' input, 2 = f32 residual
@pytest.mark.parametrize('K,nch', [(56, 2), (120, 4), (248, 8)])
def test_stream_forms(K, nch):
    M, N = 32768 + 40, 72
    bias, res, aux, rs, rows_per = epilogue_inputs(M, N, BF16, K)
    for layout, wt in (('NT', 'false'), ('NN', 'true')):
        p = Product(BF16, layout, M, N, K, seed=K)
        tag = f'stream {layout} K = {K}'
        o = Slice(M, N, BF16)
        p.gemm(out=o.view)
        assert_kernel(f'gemm_stream_kernel<bf16,{nch},{wt},0>', f'{tag} store')
        p.check(f'{tag} store', {'out': o.view}, out_bf16=True)
        o.assert_sentinel(f'{tag} store')
        o = Slice(M, N, BF16)
        p.gemm(out=o.view, act=2, aux=padded(aux.float(), BF16))
        assert_kernel(f'gemm_stream_kernel<bf16,{nch},{wt},1>', f"{tag} GELU'")
        p.check(f"{tag} GELU'", {'out': o.view}, act=2, aux=aux.to(DEV, torch.float64), out_bf16=True)
        o.assert_sentinel(f"{tag} GELU'")
        o = Slice(M, N, F32)
        p.gemm(out=o.view, bias=bias.to(DEV), residual=res.to(DEV))
        assert_kernel(f'gemm_stream_kernel<bf16,{nch},{wt},2>', f'{tag} residual')
        p.check(f'{tag} residual', {'out': o.view}, bias=bias.to(DEV, torch.float64), residual=res.to(DEV, torch.float64))
        o.assert_sentinel(f'{tag} residual')
