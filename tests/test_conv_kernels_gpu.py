"""The 15 C-ABI entries of csrc/fw_conv.hip called raw (fwair.lib.call), in both operand types, against the plain f64 statements of
tests/helpers.py (proven on the host in tests/test_conv_bounds_cpu.py).

Conventions, as in tests/test_step_kernels_gpu.py: every output lives in a guarded buffer (SENTINEL before, after and in the pad
columns of a padded row, compared bit for bit); every input with a row stride has cases with ld > C and NaN in the pad columns.
  * cap walks: shapes past the caps of the persistent / grid-stride launches (2048 convolution tiles, 1024 statistics blocks, 65536
    DCN-backward blocks, 262144 elementwise blocks), on values whose f32 partial sums are all exact, so the result does not depend on
    the order of summation and is compared BIT FOR BIT with the f64 reference;
  * edges: random storage-rounded inputs, every element within the counted-rounding bound of the reference.
Each bounded check prints `RATIO <output> <dtype> <worst error / bound>`."""
import pytest
import torch

from helpers import (BN_GRID_CAP, CONV_GRID_CAP, DCN_BORDER_CLASSES, DCN_BWD_GRID_CAP, GUARD, SENTINEL, U32, ConvCase, assert_bits,
                     assert_guarded, assert_within_bound, bn_cl_bwd_ref, bn_cl_fwd_ref, bn_grid, bn_inputs, col2im3_bound, col2im3_ref,
                     conv_chunk, conv_out_size, conv_panel_ref, dcn_bwd_ref, dcn_im2col_ref, dcn_inputs, dgm_bwd_ref, dgm_fwd_ref, dyadic,
                     gap_cl_bwd_ref, gap_cl_ref, guarded, guarded_like, im2col3_ref, lrelu_bwd_ref, lrelu_ref, nchw_to_tokens_ref, padded,
                     rup, signed_magnitudes, storage_rounding, stored, tokens_to_nchw_ref)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
BF, F32 = torch.bfloat16, torch.float32
DTYPES = [F32, BF]
IDS = lambda d: {F32: 'f32', BF: 'bf16'}.get(d, str(d))
ELEM_CAP = 262144 * 256              # threads of the largest grid of the elementwise kernels: n above it takes a second pass


def call(*a):
    from fwair.lib import call as _c
    return _c(*a)


def dt(dtype):
    from fwair.lib import dt as _d
    return _d(dtype)


def dev(t, dtype=None):
    """host tensor (f32 holding storage-rounded values) -> contiguous device tensor of `dtype`; None stays None"""
    return None if t is None else t.to(DEV, dtype or t.dtype).contiguous()


def out2d(rows, ld, dtype, prefill=None):
    """guarded [rows, ld] output -> (buf, view2d); prefill [rows, C] is written to the leading columns"""
    buf, view = guarded(rows * ld, dtype, DEV)
    v2 = view.view(rows, ld)
    if prefill is not None:
        v2[:, :prefill.shape[1]] = prefill.to(DEV, dtype)
    return buf, v2


def check2d(buf, v2, C, value, tol, what, name):
    """the leading C columns of the guarded output against the reference -- bit for bit (tol None: value rounded to the output type)
    or within the bound -- and SENTINEL everywhere else (guards and pad columns), bit for bit"""
    torch.cuda.synchronize()
    got = v2[:, :C].detach().cpu()
    dtype = v2.dtype
    full = torch.full(tuple(v2.shape), SENTINEL, dtype=dtype)
    ratio = 0.0
    if tol is None:
        full[:, :C] = value.to(dtype)
    else:
        assert_within_bound(got, value, tol, what)
        ratio = float(((got.double() - value).abs() / tol.clamp_min(1e-300)).max())
        print(f'RATIO {name} {IDS(dtype) if dtype != torch.float32 else "f32out"} {ratio:.4f}  ({what})')
        full[:, :C] = got
    assert_guarded(buf, full, 0, what + ': buffer around the output')
    return ratio


# ================================================================================================ fw_conv3x3
def run_conv(c):
    B, H, W = c.geo
    Mo = B * c.Ho * c.Wo
    buf, out = out2d(Mo, c.ldo, c.out_dtype)
    x, x2, res = dev(c.x, c.dtype), dev(c.x2, c.dtype), dev(c.res, c.dtype)
    w = dev(c.panel, c.dtype)
    bias = dev(c.bias)
    call('fw_conv3x3', dt(c.dtype), x, c.x.shape[1], x2, c.x2.shape[1] if c.x2 is not None else 0, c.cin, c.cin1, w, bias, out, c.ldo,
         c.out_f32, res, c.res.shape[1] if c.res is not None else 0, c.cout, B, H, W, c.stride, c.taps, c.act, c.slope)
    return buf, out


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('B,H,W,stride', [(8, 130, 120, 1), (12, 125, 353, 2)], ids=['s1_2112_tiles', 's2_2304_tiles'])
def test_conv_cap_walk_exact(B, H, W, stride, dtype):
    """more output tiles than the 2048 workgroups of the capped grid: the persistent loop takes its second trip and re-stages LDS.
    8 x 33 x 8 = 2112 tiles (ragged tile row 130 = 32 * 4 + 2, ragged tile column 120 = 7 * 16 + 8); stride 2: 12 x 16 x 12 = 2304
    (Ho = 63, Wo = 177, both odd inputs).  Exact values: bit for bit, bf16 against RNE of the exact result."""
    c = ConvCase(dtype, B, H, W, stride, conv_chunk(dtype), 16, exact=True, seed=11)
    assert c.tiles() > CONV_GRID_CAP and c.tiles() == {1: 2112, 2: 2304}[stride]
    print(f'WALK conv stride {stride} {IDS(dtype)}: {c.tiles()} tiles on {CONV_GRID_CAP} workgroups')
    v, _ = c.ref()
    assert torch.equal(v.float().double(), v)                              # the exact result IS an f32 value
    buf, out = run_conv(c)
    check2d(buf, out, c.cout, v, None, f'conv cap walk stride {stride} {IDS(dtype)}', 'conv')


def conv_edge(dtype, name):
    part = 96 if dtype == BF else 80
    pad8 = 8 if dtype == BF else 4
    spec = dict(
        s2_19x33=dict(B=2, H=19, W=33, stride=2, cin=64, cout=16, ldx=64 + pad8),
        s2_8x17=dict(B=1, H=8, W=17, stride=2, cin=64, cout=27, ldr=29),
        cin_partial=dict(B=1, H=6, W=20, stride=1, cin=part, cout=16, ldx=part + pad8),
        cout3=dict(B=1, H=5, W=17, stride=1, cin=64, cout=3),
        cout27_f32_ld28=dict(B=1, H=5, W=17, stride=1, cin=64, cout=27, out_f32=True, ldo=28),
        cout27_f32_ld29=dict(B=1, H=5, W=17, stride=1, cin=64, cout=27, out_f32=True, ldo=29, ldr=31),
        cout70=dict(B=1, H=5, W=17, stride=2, cin=64, cout=70, ldo=72),
        cout70_ld75=dict(B=1, H=4, W=16, stride=1, cin=64, cout=70, ldo=75),
        k1_s2=dict(B=2, H=9, W=18, stride=2, cin=64, cout=20, k=1, ldx=64 + 2 * pad8),
        k1_s2_two=dict(B=1, H=7, W=10, stride=2, cin=128, cin1=64, cout=16, k=1, ldx=64 + pad8, ldx2=64 + 3 * pad8, ldr=24),
        two_src=dict(B=1, H=6, W=18, stride=1, cin=128, cin1=64, cout=32, ldx=64 + pad8, ldx2=64 + 2 * pad8, out_f32=True, ldo=32),
        tiny=dict(B=3, H=3, W=5, stride=1, cin=64, cout=16),
        tiny_s2=dict(B=1, H=2, W=3, stride=2, cin=64, cout=16, bias=False, act=0, res=False),
        dgrad=dict(B=1, H=6, W=19, stride=1, cin=64, cout=48, bias=False, act=0, res=False, dgrad=True, ldx=64 + pad8))[name]
    return ConvCase(dtype, seed=12, **spec)


CONV_EDGES = ('s2_19x33', 's2_8x17', 'cin_partial', 'cout3', 'cout27_f32_ld28', 'cout27_f32_ld29', 'cout70', 'cout70_ld75', 'k1_s2',
              'k1_s2_two', 'two_src', 'tiny', 'tiny_s2', 'dgrad')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', CONV_EDGES)
def test_conv_edges_bounded(name, dtype):
    """stride 2 on odd sizes (the last output row / column reads one line outside the image), a partial 64-channel group, ragged
    4-lane cout tails through the scalar stores, f32 output with ldo % 4 != 0, the 1x1 form with stride 2, two sources with different
    row strides, bias + LeakyReLU + residual together (every case but tiny_s2 / dgrad), single partial tiles, the dgrad panel.
    NaN in every pad column of x, x2 and res."""
    c = conv_edge(dtype, name)
    v, tol = c.ref()
    buf, out = run_conv(c)
    check2d(buf, out, c.cout, v, tol, f'conv {name} {IDS(dtype)}', 'conv')


# ================================================================================================ fw_im2col3 / fw_col2im3
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('B,H,W,C,stride', [(2, 7, 9, 16, 1), (2, 7, 9, 16, 2), (1, 6, 5, 40, 2), (3, 1, 1, 8, 2)])
def test_im2col3_col2im3(B, H, W, C, stride, dtype):
    """im2col is a data mover (bit for bit, NaN in the pad columns of x); col2im sums at most 9 taps per pixel in f32 (bounded on
    random values, bit for bit on dyadic ones), writes only the leading C columns of a padded dx, and is im2col's adjoint:
    <im2col x, c> = <x, col2im c> exactly on dyadic values."""
    M, Mo = B * H * W, B * conv_out_size(H, stride) * conv_out_size(W, stride)
    e = 8 if dtype == BF else 4
    x = dyadic(M, C, seed=H * W + C, lo=-8, hi=8, denom=8)
    xd = dev(padded(x, C + e), dtype)
    cbuf, col = out2d(Mo, 9 * C, dtype)
    call('fw_im2col3', dt(dtype), xd, C + e, col, B, H, W, C, stride)
    want = im2col3_ref(x, B, H, W, C, stride)
    check2d(cbuf, col, 9 * C, want, None, f'im2col3 {IDS(dtype)}', 'im2col3')
    rs = storage_rounding(dtype)
    for kind in ('dyadic', 'random'):
        cc = dyadic(Mo, 9 * C, seed=3, lo=-8, hi=8, denom=8) if kind == 'dyadic' else rs(signed_magnitudes(Mo, 9 * C, seed=4))
        dbuf, dx = out2d(M, C + 2 * e, dtype)
        call('fw_col2im3', dt(dtype), dev(cc, dtype), dx, C + 2 * e, B, H, W, C, stride)
        ref, mag = col2im3_ref(cc.double(), B, H, W, C, stride)
        check2d(dbuf, dx, C, ref, None if kind == 'dyadic' else col2im3_bound(ref, mag, dtype), f'col2im3 {kind} {IDS(dtype)}', 'col2im3')
        if kind == 'dyadic' and dtype == F32:
            got = dx[:, :C].double().cpu()
            assert float((want.double() * cc.double()).sum()) == float((x.double() * got).sum())


# ================================================================================================ fw_dcn_im2col / fw_dcn_bwd
def run_dcn(dtype, B, H, W, C, d, dx0, pad):
    M = B * H * W
    xd = dev(padded(d['x'], C + pad), dtype)
    om = dev(d['om'])
    cbuf, col = out2d(M, 9 * C, dtype)
    call('fw_dcn_im2col', dt(dtype), xd, C + pad, om, col, B, H, W, C)
    xbuf, dx = out2d(M, C + 4, F32, prefill=dx0)
    mbuf, dom = out2d(M, 32, F32)
    call('fw_dcn_bwd', dt(dtype), dev(d['dcol'], dtype), xd, C + pad, om, dx, C + 4, dom, B, H, W, C)
    return (cbuf, col), (xbuf, dx), (mbuf, dom)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind,C', [(k, 8) for k in DCN_BORDER_CLASSES] + [('random', 72), ('mixed', 72)])
def test_dcn_border_classes_bounded(kind, C, dtype):
    """one constructed `om` per border class (helpers.dcn_inputs lists them: samples exactly on pixels, in (-1, 0), in (H - 1, H),
    <= -1, >= H, and all of them mixed over the taps), C = 72 (two passes of the 64 lanes, the second ragged), mask logits of scale 30
    in the mixed cases (sigmoid saturates to 0 and 1).  dx accumulates onto a non-zero prefill; dom columns 27..31 and the pad
    columns of dx keep their prefill; NaN in the pad columns of x and in om[:, 27:]."""
    B, H, W = 2, 5, 7
    d = dcn_inputs(dtype, B, H, W, C, kind, seed=21, logit_scale=30.0 if kind == 'mixed' else 1.0)
    dx0 = signed_magnitudes(B * H * W, C, seed=22)
    (cbuf, col), (xbuf, dx), (mbuf, dom) = run_dcn(dtype, B, H, W, C, d, dx0, 8)
    v, tol = dcn_im2col_ref(d['x'], d['om'], B, H, W, C, dtype)
    what = f'dcn {kind} C={C} {IDS(dtype)}'
    check2d(cbuf, col, 9 * C, v, tol, what + ' col', 'dcn_col')
    r = dcn_bwd_ref(d['dcol'], d['x'], d['om'], B, H, W, C, dx0=dx0)
    check2d(xbuf, dx, C, r['dx'], r['tol_dx'], what + ' dx', 'dcn_dx')
    check2d(mbuf, dom, 27, r['dom'], r['tol_dom'], what + ' dom', 'dcn_dom')
    if kind in ('far_before', 'far_after'):
        assert float(v.abs().max()) == 0.0 and torch.equal(r['dx'], dx0.double())


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_dcn_bwd_cap_walk_exact(dtype):
    """B H W = 2 x 121 x 121 = 29282 pixels: 263538 (pixel, tap) pairs on 65536 blocks x 4 waves = 262144, so 1394 waves take a
    second trip.  Offsets from {0, +-1, +-0.5} (bilinear weights 0, 1/4, 1/2, 1), logits 0 (m = 1/2), dyadic x, dcol and dx prefill:
    every product and every partial sum -- the atomics into dx included -- is exact, so all three outputs are compared bit for bit."""
    B, H, W, C = 2, 121, 121, (8 if dtype == BF else 4)
    M = B * H * W
    assert M * 9 > 4 * DCN_BWD_GRID_CAP and (M * 9) % 4 != 0
    print(f'WALK dcn_bwd {IDS(dtype)}: {M * 9} (pixel, tap) waves on {DCN_BWD_GRID_CAP} blocks x 4 waves')
    d = dcn_inputs(dtype, B, H, W, C, 'dyadic', seed=23)
    dx0 = dyadic(M, C, seed=24, lo=-4, hi=4, denom=4)
    (cbuf, col), (xbuf, dx), (mbuf, dom) = run_dcn(dtype, B, H, W, C, d, dx0, 8)
    v, _ = dcn_im2col_ref(d['x'], d['om'], B, H, W, C, dtype)
    r = dcn_bwd_ref(d['dcol'], d['x'], d['om'], B, H, W, C, dx0=dx0)
    for t in (v, r['dx'], r['dom']):
        assert torch.equal(t.float().double(), t)
    check2d(cbuf, col, 9 * C, storage_rounding(dtype)(v), None, f'dcn cap walk col {IDS(dtype)}', 'dcn_col')
    check2d(xbuf, dx, C, r['dx'], None, f'dcn cap walk dx {IDS(dtype)}', 'dcn_dx')
    check2d(mbuf, dom, 27, r['dom'], None, f'dcn cap walk dom {IDS(dtype)}', 'dcn_dom')


# ================================================================================================ fw_bn_cl_fwd / fw_bn_cl_bwd
EPS, MOM = 1e-5, 0.1


def vec(values, dtype=F32):
    """guarded 1-D in/out vector"""
    return guarded_like(values.to(dtype).reshape(-1), DEV)


def check_vec(buf, view, value, tol, what, name):
    torch.cuda.synchronize()
    got = view.detach().cpu()
    ratio = 0.0
    if tol is None:
        assert_guarded(buf, value.reshape(-1).to(view.dtype), 0, what)
    else:
        assert_within_bound(got[None], value.reshape(1, -1), tol.reshape(1, -1), what)
        ratio = float(((got.double() - value.reshape(-1)).abs() / tol.reshape(-1).clamp_min(1e-300)).max())
        print(f'RATIO {name} f32out {ratio:.4f}  ({what})')
        assert_guarded(buf, got, 0, what + ': buffer around the output')
    return ratio


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('C,rows', [(64, 16384 + 83), (256, 4096 + 7), (192, 5 * 1024 + 7), (1024, 1030), (4, 1024 * 256 + 5)])
def test_bn_stats_cap_walk_exact(C, rows, dtype):
    """rows past 1024 blocks x RL row lanes (RL = 256 / (C / 4): 16, 4, 5 with 16 idle threads, 1, 256): the row loops of
    colstats_kernel and bn_bwd_stats_kernel take a second trip.  x = integers / 8, dy = integers / 2, slope 1/2, mean 1/4, rstd 2:
    every partial sum is exact, so `sums` is compared bit for bit after both passes; y, mr, dx then sit within their bounds."""
    grid, RL = bn_grid(rows, C)
    assert grid == BN_GRID_CAP and rows > BN_GRID_CAP * RL
    print(f'WALK bn stats C={C} {IDS(dtype)}: {rows} rows = {-(-rows // RL)} blocks of {RL} row lanes asked, {BN_GRID_CAP} launched')
    d = bn_inputs(dtype, rows, C, seed=31, exact=True)
    x = dev(d['x'], dtype)
    sbuf, sums = vec(torch.zeros(2 * C))
    mbuf, mr = vec(torch.zeros(2 * C))
    rmb, rm = vec(d['rmean']); rvb, rv = vec(d['rvar'])
    ybuf, y = out2d(rows, C, dtype)
    call('fw_bn_cl_fwd', dt(dtype), x, C, dev(d['gamma']), dev(d['beta']), rm, rv, None, sums, mr, None, 0, y, C, rows, C, 1, EPS, MOM, 0.5)
    xs = d['x'].double()
    want = torch.stack([xs.sum(0), (xs * xs).sum(0)])
    assert torch.equal(want.float().double(), want)
    check_vec(sbuf, sums, want.float(), None, f'bn fwd sums C={C} rows={rows} {IDS(dtype)}', 'bn_sums')
    r = bn_cl_fwd_ref(d['x'], d['gamma'], d['beta'], d['rmean'], d['rvar'], None, C, 1, EPS, MOM, 0.5, dtype)
    check_vec(mbuf, mr, torch.cat([r['mean'], r['rstd']]), torch.cat([r['tol_mean'], r['tol_rstd']]), f'bn fwd mr C={C} {IDS(dtype)}', 'bn_mr')
    check2d(ybuf, y, C, r['y'], r['tol_y'], f'bn fwd y C={C} rows={rows} {IDS(dtype)}', 'bn_y')
    # backward statistics with a constructed (mean, rstd) that keeps xh exact
    dy = dyadic(rows, C, seed=32, lo=-2, hi=2, denom=2)
    yv = dyadic(rows, C, seed=33, lo=-8, hi=8, denom=8)
    mean, rstd = torch.full((C,), 0.25), torch.full((C,), 2.0)
    s2buf, sums2 = vec(torch.zeros(2 * C))
    dbuf, dx = out2d(rows, C, dtype)
    call('fw_bn_cl_bwd', dt(dtype), dev(dy, dtype), C, dev(yv, dtype), C, x, C, dev(torch.cat([mean, rstd])), dev(d['gamma']), sums2, dx, C,
         None, 0, rows, C, 1, 0.5)
    b = bn_cl_bwd_ref(dy, yv, d['x'], mean, rstd, d['gamma'], C, 1, 0.5, dtype)
    assert torch.equal(b['sums'].float().double(), b['sums'])
    check_vec(s2buf, sums2, b['sums'].float(), None, f'bn bwd sums C={C} rows={rows} {IDS(dtype)}', 'bn_dsums')
    check2d(dbuf, dx, C, b['dx'], b['tol_dx'], f'bn bwd dx C={C} rows={rows} {IDS(dtype)}', 'bn_dx')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('ratio', [0.0, 1.0, 8.0])
@pytest.mark.parametrize('rows,C', [(333, 192), (50, 8), (1, 16)])
def test_bn_edges_bounded(rows, C, ratio, dtype):
    """train forward twice in a row (running statistics folded twice, nbt counted twice) with a residual and slope 0.1, its backward
    with dres; the no-activation form (slope 1.0: y is not read -- it holds NaN -- no res, no dres, nbt NULL); eval forward and
    backward.  Inputs at |mean| / std = 0, 1, 8: the bound carries 1 + mean^2 / var.  C = 192 leaves 16 idle threads per block;
    rows = 1 has zero variance and the unbiased factor 1.  NaN in the pad columns of x, res, dy, y."""
    e = 8 if dtype == BF else 4
    d = bn_inputs(dtype, rows, C, ratio, seed=41)
    ld = C + e
    x, res, dy = (dev(padded(d[n], ld), dtype) for n in ('x', 'res', 'dy'))
    gamma, beta = dev(d['gamma']), dev(d['beta'])
    rmb, rm = vec(d['rmean']); rvb, rv = vec(d['rvar'])
    nb, nbt = vec(torch.tensor([5]), torch.int64)
    tag = f'rows={rows} C={C} |mean|/std={ratio} {IDS(dtype)}'
    rm_in, rv_in = d['rmean'], d['rvar']
    for step in (1, 2):
        sbuf, sums = vec(torch.zeros(2 * C)); mbuf, mr = vec(torch.zeros(2 * C))
        ybuf, y = out2d(rows, ld + e, dtype)
        call('fw_bn_cl_fwd', dt(dtype), x, ld, gamma, beta, rm, rv, nbt, sums, mr, res, ld, y, ld + e, rows, C, 1, EPS, MOM, 0.1)
        r = bn_cl_fwd_ref(d['x'], d['gamma'], d['beta'], rm_in, rv_in, d['res'], C, 1, EPS, MOM, 0.1, dtype)
        check_vec(mbuf, mr, torch.cat([r['mean'], r['rstd']]), torch.cat([r['tol_mean'], r['tol_rstd']]), f'bn train mr step {step} {tag}',
                  f'bn_mr_ratio{ratio:g}')
        check2d(ybuf, y, C, r['y'], r['tol_y'], f'bn train y step {step} {tag}', f'bn_y_ratio{ratio:g}')
        check_vec(rmb, rm, r['rmean'], r['tol_rmean'], f'bn running mean step {step} {tag}', 'bn_rmean')
        check_vec(rvb, rv, r['rvar'], r['tol_rvar'], f'bn running var step {step} {tag}', f'bn_rvar_ratio{ratio:g}')
        check_vec(nb, nbt, torch.tensor([5 + step]), None, f'bn nbt step {step} {tag}', 'nbt')
        rm_in, rv_in = rm.detach().cpu().clone(), rv.detach().cpu().clone()        # the kernel's own (checked) state feeds the next step
    mrh, yh = mr.detach().cpu(), y[:, :C].detach().float().cpu()
    # train backward, with dres
    sbuf, sums = vec(torch.zeros(2 * C))
    dbuf, dx = out2d(rows, ld, dtype); rbuf, dres = out2d(rows, ld + e, dtype)
    yd = dev(padded(yh, ld), dtype)
    call('fw_bn_cl_bwd', dt(dtype), dy, ld, yd, ld, x, ld, mr, gamma, sums, dx, ld, dres, ld + e, rows, C, 1, 0.1)
    b = bn_cl_bwd_ref(d['dy'], yh, d['x'], mrh[:C], mrh[C:], d['gamma'], C, 1, 0.1, dtype)
    check2d(dbuf, dx, C, b['dx'], b['tol_dx'], f'bn train dx {tag}', 'bn_dx')
    check2d(rbuf, dres, C, b['dres'], b['tol_dres'], f'bn train dres {tag}', 'bn_dres')
    check_vec(sbuf, sums, b['sums'], b['tol_sums'], f'bn train (dbeta, dgamma) {tag}', 'bn_dsums')
    # the no-activation form: slope 1.0, nbt NULL, no res; backward without dres, y = NaN (not read)
    sbuf, sums = vec(torch.zeros(2 * C)); mbuf, mr = vec(torch.zeros(2 * C))
    ybuf, y = out2d(rows, C, dtype)
    call('fw_bn_cl_fwd', dt(dtype), x, ld, gamma, beta, rm, rv, None, sums, mr, None, 0, y, C, rows, C, 1, EPS, MOM, 1.0)
    r = bn_cl_fwd_ref(d['x'], d['gamma'], d['beta'], rm_in, rv_in, None, C, 1, EPS, MOM, 1.0, dtype)
    check2d(ybuf, y, C, r['y'], r['tol_y'], f'bn train y slope 1 {tag}', f'bn_y_ratio{ratio:g}')
    check_vec(nb, nbt, torch.tensor([7]), None, f'bn nbt untouched by a NULL call {tag}', 'nbt')
    mrh = mr.detach().cpu()
    sbuf, sums = vec(torch.zeros(2 * C)); dbuf, dx = out2d(rows, C, dtype)
    ynan = torch.full((rows, C), NAN, dtype=dtype, device=DEV)
    call('fw_bn_cl_bwd', dt(dtype), dy, ld, ynan, C, x, ld, mr, gamma, sums, dx, C, None, 0, rows, C, 1, 1.0)
    b = bn_cl_bwd_ref(d['dy'], None, d['x'], mrh[:C], mrh[C:], d['gamma'], C, 1, 1.0, dtype)
    check2d(dbuf, dx, C, b['dx'], b['tol_dx'], f'bn train dx slope 1 {tag}', 'bn_dx')
    check_vec(sbuf, sums, b['sums'], b['tol_sums'], f'bn (dbeta, dgamma) slope 1 {tag}', 'bn_dsums')
    # eval: the running statistics normalise, nothing is updated
    rm_in, rv_in = rm.detach().cpu().clone(), rv.detach().cpu().clone()
    sbuf, sums = vec(torch.zeros(2 * C)); mbuf, mr = vec(torch.zeros(2 * C))
    ybuf, y = out2d(rows, C, dtype)
    call('fw_bn_cl_fwd', dt(dtype), x, ld, gamma, beta, rm, rv, nbt, sums, mr, res, ld, y, C, rows, C, 0, EPS, MOM, 0.1)
    r = bn_cl_fwd_ref(d['x'], d['gamma'], d['beta'], rm_in, rv_in, d['res'], C, 0, EPS, MOM, 0.1, dtype)
    check2d(ybuf, y, C, r['y'], r['tol_y'], f'bn eval y {tag}', 'bn_y_eval')
    check_vec(mbuf, mr, torch.cat([r['mean'], r['rstd']]), torch.cat([r['tol_mean'], r['tol_rstd']]), f'bn eval mr {tag}', 'bn_mr_eval')
    check_vec(rmb, rm, rm_in, None, f'bn eval leaves running mean {tag}', 'bn_rmean')
    check_vec(rvb, rv, rv_in, None, f'bn eval leaves running var {tag}', 'bn_rvar')
    check_vec(nb, nbt, torch.tensor([7]), None, f'bn eval leaves nbt {tag}', 'nbt')
    check_vec(sbuf, sums, torch.zeros(2 * C), None, f'bn eval leaves sums {tag}', 'bn_sums')
    mrh, yh = mr.detach().cpu(), y.detach().float().cpu()
    sbuf, sums = vec(torch.zeros(2 * C)); dbuf, dx = out2d(rows, C, dtype)
    call('fw_bn_cl_bwd', dt(dtype), dy, ld, dev(yh, dtype), C, x, ld, mr, gamma, sums, dx, C, None, 0, rows, C, 0, 0.1)
    b = bn_cl_bwd_ref(d['dy'], yh, d['x'], mrh[:C], mrh[C:], d['gamma'], C, 0, 0.1, dtype)
    check2d(dbuf, dx, C, b['dx'], b['tol_dx'], f'bn eval dx {tag}', 'bn_dx_eval')
    check_vec(sbuf, sums, b['sums'], b['tol_sums'], f'bn eval (dbeta, dgamma) {tag}', 'bn_dsums')


# ================================================================================================ the elementwise entries
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_lrelu_dgm_gap_layouts(dtype):
    """fw_lrelu_t and its backward (padded rows, NaN pads), fw_dgm_fwd / bwd, fw_gap_cl / bwd, fw_nchw_to_tokens (Cp > Ci zero
    fill) and fw_tokens_to_nchw: bit for bit where the statement is one rounding of an exact value, within the counted roundings
    otherwise."""
    rs = storage_rounding(dtype)
    e = 8 if dtype == BF else 4
    rows, C = 37, 20
    ld = C + e
    slope = 0.1
    x = rs(signed_magnitudes(rows, C, seed=51) * torch.randn(rows, C, generator=torch.Generator().manual_seed(51)))
    dy = rs(signed_magnitudes(rows, C, seed=52))
    ybuf, y = out2d(rows, ld + e, dtype)
    call('fw_lrelu_t', dt(dtype), dev(padded(x, ld), dtype), ld, y, ld + e, rows, C, slope)
    yr = lrelu_ref(x.double(), slope)                                      # one f32 product, one storage rounding
    check2d(ybuf, y, C, yr.float() if dtype == BF else yr, None, f'lrelu_t {IDS(dtype)}', 'lrelu')
    yh = y[:, :C].float().cpu()
    dbuf, dx = out2d(rows, ld, dtype)
    call('fw_lrelu_t_bwd', dt(dtype), dev(padded(dy, ld + e), dtype), ld + e, dev(padded(yh, ld), dtype), ld, dx, ld, rows, C, slope)
    dr = lrelu_bwd_ref(dy.double(), yh.double(), slope)
    check2d(dbuf, dx, C, dr.float() if dtype == BF else dr, None, f'lrelu_t_bwd {IDS(dtype)}', 'lrelu')
    # DGM
    n = 3001
    a, dcn, gam, bet, dout = (rs(signed_magnitudes(1, n, seed=53 + i)) for i in range(5))
    obuf, out = out2d(1, n, dtype)
    call('fw_dgm_fwd', dt(dtype), dev(a, dtype), dev(dcn, dtype), dev(gam, dtype), dev(bet, dtype), out, n, slope)
    v, tol = dgm_fwd_ref(a.double(), dcn.double(), gam.double(), bet.double(), slope)
    check2d(obuf, out, n, v, stored(v, tol, dtype), f'dgm_fwd {IDS(dtype)}', 'dgm')
    oh = out.float().cpu()
    bufs = [out2d(1, n, dtype) for _ in range(3)]
    call('fw_dgm_bwd', dt(dtype), dev(dout, dtype), out, dev(a, dtype), dev(gam, dtype), bufs[0][1], bufs[1][1], bufs[2][1], n, slope)
    b = dgm_bwd_ref(dout.double(), oh.double(), a.double(), gam.double(), slope)
    for (buf, view), name in zip(bufs, ('dx', 'dz', 'dgamma')):
        check2d(buf, view, n, b[name], stored(b[name], b['tol_' + name], dtype), f'dgm_bwd {name} {IDS(dtype)}', 'dgm')
    # global average pool
    B, P, Cg = 3, 50, 300                                                  # C above one block of 256 threads
    xg = rs(signed_magnitudes(B * P, Cg, seed=58))
    gbuf, gap = out2d(B, Cg, F32)
    call('fw_gap_cl', dt(dtype), dev(padded(xg, Cg + e), dtype), Cg + e, gap, B, P, Cg)
    gv, gt = gap_cl_ref(xg.double(), B, P, Cg)
    check2d(gbuf, gap, Cg, gv, gt, f'gap_cl {IDS(dtype)}', 'gap')
    dgap = signed_magnitudes(B, Cg, seed=59)
    dbuf, dxg = out2d(B * P, Cg + e, dtype)
    call('fw_gap_cl_bwd', dt(dtype), dev(dgap), dxg, Cg + e, B, P, Cg)
    gb = gap_cl_bwd_ref(dgap.double(), P)
    check2d(dbuf, dxg, Cg, gb, stored(gb, 2 * U32 * gb.abs(), dtype), f'gap_cl_bwd {IDS(dtype)}', 'gap')
    # layouts
    Bi, Ci, HW, Cp = 2, 3, 35, 16
    img = signed_magnitudes(Bi, Ci, HW, seed=60)
    tbuf, tok = out2d(Bi * HW, Cp + e, dtype)
    call('fw_nchw_to_tokens', dt(dtype), dev(img), tok, Cp + e, Bi, Ci, HW, Cp)
    check2d(tbuf, tok, Cp, nchw_to_tokens_ref(img, Cp), None, f'nchw_to_tokens {IDS(dtype)}', 'layout')
    tk = rs(signed_magnitudes(Bi * HW, Ci, seed=61))
    ibuf, im = out2d(1, Bi * Ci * HW, F32)
    call('fw_tokens_to_nchw', dt(dtype), dev(padded(tk, Cp), dtype), Cp, im, Bi, Ci, HW)
    check2d(ibuf, im, Bi * Ci * HW, tokens_to_nchw_ref(tk, Bi, Ci, HW).reshape(1, -1), None, f'tokens_to_nchw {IDS(dtype)}', 'layout')


def pattern(n, mul, mod, denom, dtype=F32):
    """device values (i * mul % mod - mod // 2) / denom: small dyadic numbers, exact in either type"""
    return ((torch.arange(n, device=DEV, dtype=torch.int32) * mul % mod - mod // 2).float() / denom).to(dtype)


def same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    v = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(v), b.view(v))


def guards_hold(buf, n):
    return bool((torch.cat([buf[:GUARD], buf[GUARD + n:]]).float() == SENTINEL).all())


def rows_out(rows, ld, dtype):
    buf, v = guarded(rows * ld, dtype, DEV)
    return buf, v.view(rows, ld)


def rows_in(rows, ld, C, mul, mod, denom, dtype):
    """[rows, ld] pattern with NaN in the pad columns"""
    t = pattern(rows * ld, mul, mod, denom, dtype).view(rows, ld)
    t[:, C:] = NAN
    return t


SECOND_PASS = ('lrelu_t-f32', 'lrelu_t-bf16', 'lrelu_t_bwd', 'dgm_fwd', 'dgm_bwd', 'gap_cl_bwd', 'nchw_to_tokens', 'tokens_to_nchw')


@pytest.mark.parametrize('entry', SECOND_PASS)
def test_elementwise_second_grid_pass(entry):
    """Every entry launched through the capped grid (262144 blocks of 256 threads) at n = elements above 262144 x 256 with a ragged
    remainder, so that its `i += gstride()` loop takes a second trip and its own row / column arithmetic (i / C, r / P,
    (i / HW) % Ci, ...) runs there: fw_lrelu_t (f32 and bf16) and fw_lrelu_t_bwd on [65729][1021] in padded rows, fw_dgm_fwd / bwd
    on cap + 77 elements, fw_gap_cl_bwd on [1279 x 64][821], fw_nchw_to_tokens on [2 x 2097155][16] from 3 planes,
    fw_tokens_to_nchw on [2][8][4194309].  Values are small dyadic numbers and slope 1/4, so every statement is exact in f32 and is
    evaluated with torch on the device; outputs are compared bit for bit, pad columns and guards included.  (fw_gap_cl launches
    one block per image and has no such loop.)"""
    slope = 0.25
    lrelu = lambda t: torch.where(t > 0, t, t * slope)
    if entry.startswith('lrelu_t'):
        dtype = F32 if entry.endswith('f32') else BF
        rows, C = 65729, 1021
        ld, ldo, n = C + 3, C + 5, rows * C
        x = rows_in(rows, ld, C, 7, 33, 8, dtype)
        buf, y = rows_out(rows, ldo, dtype)
        if entry == 'lrelu_t_bwd':
            dy = rows_in(rows, ldo, C, 11, 17, 8, dtype)
            call('fw_lrelu_t_bwd', dt(dtype), dy, ldo, x, ld, y, ldo, rows, C, slope)           # x plays the forward output: its sign decides
            want = torch.where(x[:, :C].float() < 0, dy[:, :C].float() * slope, dy[:, :C].float()).to(dtype)
        else:
            call('fw_lrelu_t', dt(dtype), x, ld, y, ldo, rows, C, slope)
            want = lrelu(x[:, :C].float()).to(dtype)
        outs = [(buf, y, C, want)]
    elif entry.startswith('dgm'):
        dtype, n = BF, ELEM_CAP + 77
        a, b, g, c = (pattern(n, m, q, 8, dtype) for m, q in ((7, 33), (11, 17), (5, 9), (13, 25)))
        af, bf, gf, cf = (t.float() for t in (a, b, g, c))
        if entry == 'dgm_fwd':
            buf, out = rows_out(1, n, dtype)
            call('fw_dgm_fwd', dt(dtype), a, b, g, c, out, n, slope)
            outs = [(buf, out, n, lrelu(af + bf + af * gf + cf).to(dtype)[None])]
        else:                                                                                      # dout = b, out = c (its sign decides)
            bufs = [rows_out(1, n, dtype) for _ in range(3)]
            call('fw_dgm_bwd', dt(dtype), b, c, a, g, bufs[0][1], bufs[1][1], bufs[2][1], n, slope)
            dz = torch.where(cf < 0, bf * slope, bf)
            outs = [(bufs[0][0], bufs[0][1], n, (dz * (1.0 + gf)).to(dtype)[None]), (bufs[1][0], bufs[1][1], n, dz.to(dtype)[None]),
                    (bufs[2][0], bufs[2][1], n, (dz * af).to(dtype)[None])]
    elif entry == 'gap_cl_bwd':
        dtype, B, P, C = BF, 1279, 64, 821
        rows, ld, n = B * P, C + 3, B * P * C
        dgap = pattern(B * C, 7, 33, 8).view(B, C)
        buf, dx = rows_out(rows, ld, dtype)
        call('fw_gap_cl_bwd', dt(dtype), dgap, dx, ld, B, P, C)
        outs = [(buf, dx, C, (dgap / P).repeat_interleave(P, 0).to(dtype))]                       # P = 2^6: the division is exact
    elif entry == 'nchw_to_tokens':
        dtype, B, Ci, HW, Cp = BF, 2, 3, 2097155, 16
        ld, n = Cp + 8, B * HW * Cp
        img = pattern(B * Ci * HW, 7, 33, 8).view(B, Ci, HW)
        buf, tok = rows_out(B * HW, ld, dtype)
        call('fw_nchw_to_tokens', dt(dtype), img, tok, ld, B, Ci, HW, Cp)
        want = torch.zeros(B * HW, Cp, dtype=dtype, device=DEV)
        want[:, :Ci] = img.permute(0, 2, 1).reshape(B * HW, Ci).to(dtype)
        outs = [(buf, tok, Cp, want)]
    else:
        dtype, B, Ci, HW = BF, 2, 8, 4194309
        ld, n = Ci + 8, B * Ci * HW
        tok = rows_in(B * HW, ld, Ci, 7, 33, 8, dtype)
        buf, img = rows_out(1, n, F32)
        call('fw_tokens_to_nchw', dt(dtype), tok, ld, img, B, Ci, HW)
        outs = [(buf, img, n, tok[:, :Ci].float().view(B, HW, Ci).permute(0, 2, 1).reshape(1, n))]
    torch.cuda.synchronize()
    assert n > ELEM_CAP and n % 256 != 0
    print(f'WALK {entry}: {n} elements on {ELEM_CAP} threads')
    for buf, v2, C, want in outs:
        assert same_bits(v2[:, :C], want), f'{entry}: output differs from the statement'
        assert bool((v2[:, C:].float() == SENTINEL).all()), f'{entry}: pad columns written'
        assert guards_hold(buf, v2.numel()), f'{entry}: guard written'


# ================================================================================================ argument checks
def arg_table(bufs):
    """-> {entry: (ordered good arguments, [(what, {argument: bad value}), ...])}: one violation per CONJUNCT of every FW_CHECK_ARG
    of csrc/fw_conv.hip.  Every bad call differs from a call that succeeds in the named arguments only, and would stay inside the
    (generous) buffers if the check it aims at were missing."""
    x, x2, w, v, ll, out, out2, out3 = bufs
    off = lambda t: t.data_ptr() + 4                                       # a 4-byte-aligned, not 16-byte-aligned address
    nulls = lambda *names: [(f'{n} NULL', {n: None}) for n in names]
    zeros = lambda *names: [(f'{n} = 0', {n: 0}) for n in names]
    two = dict(x2=x2, ldx2=64, cin=128, cin1=64)                           # the two-source form the x2 clauses need
    T = {}
    T['fw_conv3x3'] = (
        dict(dtype=0, x=x, ldx=64, x2=None, ldx2=0, cin=64, cin1=64, w=w, bias=None, out=out, ldo=64, out_f32=0, res=None, ldr=0, cout=16,
             B=1, H=4, W=8, stride=1, taps=0x1ff, act=0, slope=0.0),
        [('dtype', dict(dtype=5))] + nulls('x', 'w', 'out') + zeros('B', 'H', 'W', 'cout') + [
            ('stride 3', dict(stride=3)), ('cin = 0', dict(cin=0, cin1=0)), ('cin % chunk', dict(cin=72, cin1=72)), ('cin1 = 0', dict(cin1=0)),
            ('cin1 > cin', dict(cin1=80, ldx=80)), ('cin1 < cin without x2', dict(cin1=32)),
            ('cin1 % 64 with x2', dict(two, cin1=32)), ('two sources succeed', None, two),
            ('ldx bytes % 16', dict(ldx=66)), ('ldx < cin1', dict(ldx=48)), ('ldx2 bytes % 16', dict(two, ldx2=66)),
            ('ldx2 < cin - cin1', dict(two, ldx2=48)), ('x alignment', dict(x=off(x))), ('w alignment', dict(w=off(w))),
            ('x2 alignment', dict(two, x2=off(x2))), ('taps = 0', dict(taps=0)), ('taps outside the nine bits', dict(taps=0x200)),
            ('ldo < cout', dict(ldo=8)), ('ldr < cout', dict(res=x, ldr=8))])
    col = [('C % e', dict(C=18)), ('stride 3', dict(stride=3))]
    T['fw_im2col3'] = (dict(dtype=0, x=x, ldx=64, col=out, B=1, H=4, W=4, C=16, stride=1), nulls('x', 'col') + col + [('ldx % e', dict(ldx=66))])
    T['fw_col2im3'] = (dict(dtype=0, dcol=x, dx=out, lddx=64, B=1, H=4, W=4, C=16, stride=1), nulls('dcol', 'dx') + col + [('lddx % e', dict(lddx=66))])
    T['fw_dcn_im2col'] = (dict(dtype=0, x=x, ldx=64, om=v, col=out, B=1, H=2, W=2, C=16),
                          nulls('x', 'om', 'col') + [('C % e', dict(C=18)), ('ldx % e', dict(ldx=66)), ('C % e, bf16', dict(dtype=1, C=12))])
    T['fw_dcn_bwd'] = (dict(dtype=0, dcol=x, x=x, ldx=64, om=v, dx=out, lddx=64, dom=out2, B=1, H=2, W=2, C=16),
                       nulls('dcol', 'x', 'om', 'dx', 'dom') + zeros('C'))
    bn = zeros('rows', 'C') + [('C % 4', dict(C=6)), ('C > 1024', dict(C=1028))]
    T['fw_bn_cl_fwd'] = (dict(dtype=0, x=x, ldx=64, gamma=v, beta=v, rmean=out2[0], rvar=out2[1], nbt=ll, sums=out2[2], mr=out3[0], res=None, ldr=0,
                              y=out, ldy=64, rows=8, C=8, training=1, eps=1e-5, momentum=0.1, slope=0.1),
                         nulls('x', 'gamma', 'beta', 'rmean', 'rvar', 'sums', 'mr', 'y') + bn)
    T['fw_bn_cl_bwd'] = (dict(dtype=0, dy=x, ldd=64, y=x, ldy=64, x=x, ldx=64, mr=v, gamma=v, sums=out2[0], dx=out, lddx=64, dres=out3, lddr=64,
                              rows=8, C=8, training=1, slope=0.1), nulls('dy', 'y', 'x', 'mr', 'gamma', 'sums', 'dx') + bn)
    T['fw_lrelu_t'] = (dict(dtype=0, x=x, ldx=64, y=out, ldy=64, rows=8, C=8, slope=0.1), nulls('x', 'y') + zeros('rows', 'C'))
    T['fw_lrelu_t_bwd'] = (dict(dtype=0, dy=x, ldd=64, y=x, ldy=64, dx=out, lddx=64, rows=8, C=8, slope=0.1),
                           nulls('dy', 'y', 'dx') + zeros('rows', 'C'))
    T['fw_dgm_fwd'] = (dict(dtype=0, x=x, dcn=x, gamma=x, beta=x, out=out, n=64, slope=0.1), nulls('x', 'dcn', 'gamma', 'beta', 'out') + zeros('n'))
    T['fw_dgm_bwd'] = (dict(dtype=0, dout=x, out=x, x=x, gamma=x, dx=out, dz=out2, dgamma=out3, n=64, slope=0.1),
                       nulls('dout', 'out', 'x', 'gamma', 'dx', 'dz', 'dgamma') + zeros('n'))
    T['fw_gap_cl'] = (dict(dtype=0, x=x, ldx=64, out=out, B=2, P=4, C=8), nulls('x', 'out') + zeros('B', 'P', 'C'))
    T['fw_gap_cl_bwd'] = (dict(dtype=0, dgap=v, dx=out, lddx=64, B=2, P=4, C=8), nulls('dgap', 'dx') + zeros('B', 'P', 'C'))
    T['fw_nchw_to_tokens'] = (dict(dtype=0, img=v, tok=out, ld=64, B=1, Ci=8, HW=4, Cp=8),
                              nulls('img', 'tok') + zeros('B', 'Ci', 'HW') + [('Cp < Ci', dict(Cp=7)), ('ld < Cp', dict(ld=4))])
    T['fw_tokens_to_nchw'] = (dict(dtype=0, tok=x, ld=64, img=out, B=1, Ci=8, HW=4), nulls('tok', 'img') + zeros('B', 'Ci', 'HW') + [('ld < Ci', dict(ld=7))])
    return T


def test_argument_checks_return_negative_and_write_nothing():
    """One refused call per conjunct of every FW_CHECK_ARG of the 15 entries (null pointers, sizes <= 0, granule and alignment
    rules, the row-stride bounds that keep loads and stores inside the rows, C <= 1024, ...).  First the unviolated call of every
    entry succeeds, so each bad call is refused for the one thing it changes; then the outputs are re-filled, every bad call must
    come back negative (fwair.lib.call raises with 'argument check'), and no guarded output has changed."""
    from fwair.lib import parse_header
    t = lambda *s: torch.zeros(*s, device=DEV)
    houts = [out2d(64, 64, F32) for _ in range(3)]
    ll = torch.zeros(4, dtype=torch.int64, device=DEV)
    T = arg_table((t(64, 128), t(64, 128), t(64, 9 * 128), t(4096), ll) + tuple(o for _, o in houts))
    protos = parse_header()
    assert set(T) <= set(protos) and len(T) == 15
    calls = 0
    for name, (good, cases) in T.items():
        assert len(good) + 1 == len(protos[name]), name                   # the argument names above follow the header's order
        call(name, *good.values())
        for case in cases:
            if case[1] is None:                                            # a second valid form: it must succeed too
                call(name, *dict(good, **case[2]).values())
    torch.cuda.synchronize()
    for buf, _ in houts:
        buf.fill_(SENTINEL)
    ll.zero_()
    for name, (good, cases) in T.items():
        for case in cases:
            if case[1] is None:
                continue
            assert set(case[1]) <= set(good), (name, case[0])
            with pytest.raises(RuntimeError, match='argument check'):
                call(name, *dict(good, **case[1]).values())
            calls += 1
    torch.cuda.synchronize()
    print(f'{calls} refused calls')
    assert calls == 117
    for buf, _ in houts:
        assert_guarded(buf, torch.full((64 * 64,), SENTINEL), 0, 'outputs of refused calls')
    assert int(ll.abs().sum()) == 0


# ================================================================================================ fwair.convnets.panel
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_panel_matches_the_helpers_builder(dtype):
    """fwair.convnets.panel, kinds 'fwd' (3x3 and 1x1) and 'dgrad', against helpers.conv_panel_ref, bit for bit"""
    from fwair import convnets as CV
    from fwair import functional as Fn
    keep = Fn.config.compute_dtype
    Fn.config.compute_dtype = dtype
    try:
        ck = conv_chunk(dtype)
        for Co, Ci, k in ((27, 40, 3), (70, 64, 3), (20, 48, 1)):
            wgt = signed_magnitudes(Co, Ci, k, k, seed=70 + Co)
            p = torch.nn.Parameter(wgt.to(DEV))
            assert_bits(CV.panel(p, 'fwd'), conv_panel_ref(wgt, rup(Ci, ck), 'fwd').to(dtype), f'panel fwd {Co}x{Ci}x{k} {IDS(dtype)}')
            if k == 3:
                assert_bits(CV.panel(p, 'dgrad'), conv_panel_ref(wgt, rup(Co, ck), 'dgrad').to(dtype), f'panel dgrad {Co}x{Ci} {IDS(dtype)}')
    finally:
        Fn.config.compute_dtype = keep
