"""fw_dwconv_fwd / fw_dwconv_bwd (csrc/fw_elem.hip, five kernel templates) called raw (fwair.lib.call), every form the dispatch can
reach, against the f64 statement and the counted-rounding bounds of tests/helpers.py (proven on the host in
tests/test_dwconv_bounds_cpu.py).  helpers.dwconv_plan restates the dispatch; each case asserts the form it is built to reach.

Conventions: operands are rounded to storage and widened to f64 ON THE DEVICE for the reference; input rows are ld = C + 8 wide with
NaN in the pad columns; h2 / g2 / dh1 are guarded views with a row stride of their own (C + 16; ldg == ld1 is a checked contract and
stays); dw / dbias are guarded and pre-filled with multiples of 1/4.  After every call the inputs, their NaN pads, the guards and
the pad columns of the outputs are compared with what they held, and EVERY output element is checked against its bound.  Each check
prints `RATIO <output> <operand dtype> <worst error / bound>`.

  S0  2 x 12 x 24 x 40     strip forward (grid 8, padded from 3), strip + wgrad backward (5 blocks, dead lanes, NSTRIP 2)
  S1  4 x 136 x 120 x 168  pipe NT 1; fused NT 1; with g1: tile<1> + wgrad (NSTRIP 4)
  S2  9 x 920 x 24 x 72    pipe NT 2 (4 walks cross an image border, last walk 1 tile row); fused NT 4 (6 cross, last walk 3, 4 idle
                           padded workgroups); with g1: tile<1> + wgrad (NSTRIP 8)
  S3  66 x 8200 x 8 x 8|4  the walk cap: NT 32 from a raw quotient of 33 (forward) / 66 (backward), 2115 walks, 63 cross, last walk 2
                           rows, 5 idle workgroups; one 16-pixel tile column half beyond W, one channel block with 8 / 4 live channels
  S4  2 x 4100 x 8 x 1024  H % 8 = 4: strip kernels past the 8192-workgroup cap (2 099 200 threads, two grid-stride passes)
  P5  1 x 1280 x 128 x 64  one allocation viewed with ld = 13104 (H W ld < 2^31: pipe / fused at the largest 32-bit offsets) and with
                           ld = 13112 (>= 2^31: dwconv_tile_kernel<T, 0, true>, tile<1> + wgrad<true>)"""
import pytest
import torch

from helpers import (GEMM_MIN_GAIN, GUARD, SENTINEL, assert_within_bound, bound_violations, dwconv_bwd_ref, dwconv_plan, dwconv_ref,
                     dwconv_rows_share, dyadic, gelu64, guarded, guarded_like, signed_magnitudes)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = [F32, BF]
IDS = lambda d: {F32: 'f32', BF: 'bf16'}.get(d, str(d))
S0, S1, S2, S4 = (2, 12, 24, 40), (4, 136, 120, 168), (9, 920, 24, 72), (2, 4100, 8, 1024)
S3 = lambda dtype: (66, 8200, 8, 8 if dtype == BF else 4)
MIN_REJECTED = 0.99


def call(*a):
    from fwair.lib import call as _c
    return _c(*a)


def dt(dtype):
    from fwair.lib import dt as _d
    return _d(dtype)


# ================================================================================================ operands, buffers, checks
def rand_signed(shape, seed, dtype, sign=0, lo=0.75, hi=1.25):
    """signed_magnitudes drawn on the device (the large cases hold up to 67 M elements), rounded to `dtype`"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    mag = lo + (hi - lo) * torch.rand(shape, generator=g, device=DEV)
    s = torch.randint(0, 2, shape, generator=g, device=DEV).float() * 2 - 1 if sign == 0 else sign
    return (mag * s).to(dtype)


def rand_ints(shape, seed, dtype, lo, hi, denom=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randint(lo, hi + 1, shape, generator=g, device=DEV).float() / denom).to(dtype)


def padded_in(vals, pad=8):
    """[M, C] device values -> [M, C + pad] buffer with NaN in the pad columns"""
    buf = torch.full((vals.shape[0], vals.shape[1] + pad), NAN, dtype=vals.dtype, device=DEV)
    buf[:, :vals.shape[1]] = vals
    return buf


def assert_input_kept(buf, vals, what):
    C = vals.shape[1]
    assert torch.equal(buf[:, :C], vals), f'{what}: an input changed'
    assert bool(torch.isnan(buf[:, C:]).all()), f'{what}: the NaN pad of an input changed'


def out2d(M, C, dtype, pad=16, fill=None):
    buf, view = guarded(M * (C + pad), dtype, DEV)
    v2 = view.view(M, C + pad)
    if fill is not None:
        v2[:, :C] = fill
    return buf, v2


def params(C, seed, integer=False, positive=False):
    """w [C, 9], bias [C] (f32 values as f64 on the device), and the guarded, pre-filled dw / dbias"""
    w = signed_magnitudes(C, 9, seed=seed, sign=1 if positive else 0)
    bias = signed_magnitudes(C, seed=seed + 1)
    sg = lambda *sh, n: (torch.randint(0, 2, sh, generator=torch.Generator().manual_seed(seed + n)).float() * 2 - 1) if not integer else 1.0
    dw0 = dyadic(C, 9, seed=seed + 2, lo=1 if integer else 4, hi=8 if integer else 32, denom=1 if integer else 4) * sg(C, 9, n=3)
    db0 = dyadic(C, seed=seed + 4, lo=1 if integer else 4, hi=8 if integer else 32, denom=1 if integer else 4) * sg(C, n=5)
    return dict(w=w.double().to(DEV), bias=bias.double().to(DEV), wt=w.t().contiguous().to(DEV), biasf=bias.to(DEV), dw0=dw0, db0=db0)


def ratio_of(y, value, tol):
    return float(((y.to(value.device, F64) - value).abs() / tol.clamp_min(1e-300)).max())


def check_out(buf, v2, C, value, tol, name, what):
    """the leading C columns within the bound, element by element; guards and pad columns still SENTINEL"""
    torch.cuda.synchronize()
    got = v2[:, :C]
    assert_within_bound(got, value, tol, what + ' ' + name)
    print(f'RATIO {name} {IDS(v2.dtype)} {ratio_of(got, value, tol):.4f}  ({what})')
    assert bool((v2[:, C:] == SENTINEL).all()), f'{what} {name}: a pad column of the output changed'
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), f'{what} {name}: a guard of the output changed'


def check_param(buf, view, value, tol, name, what, exact=False, dtype=None):
    torch.cuda.synchronize()
    got = view.view(value.shape)
    if exact:
        assert torch.equal(got.double(), value), (f'{what} {name}: not the exact sum; largest difference '
                                                  f'{float((got.double() - value).abs().max())!r}')
        print(f'EXACT {name}  ({what})')
    else:
        y, v, t = (x.reshape(value.shape[0], -1) for x in (got, value, tol))
        assert_within_bound(y, v, t, what + ' ' + name)
        print(f'RATIO {name} {IDS(dtype) if dtype else "f32"} {ratio_of(y, v, t):.4f}  ({what})')
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), f'{what} {name}: a guard changed'


def run_fwd(shape, dtype, src, in_gelu, p, what, form, fill=None):
    """src [M, C] device values of `dtype` -> (h2, g2) [M, C] views after the call, checked against the reference"""
    B, H, W, C = shape
    M = B * H * W
    buf = padded_in(src)
    plan = dwconv_plan(B, H, W, C, C + 8, dtype, False)['fwd']
    assert plan['form'] == form, f'{what}: the dispatch takes {plan["form"]}, the case is built for {form}'
    (hb, h2), (gb, g2) = out2d(M, C, dtype, fill=fill), out2d(M, C, dtype, fill=fill)
    call('fw_dwconv_fwd', dt(dtype), buf, C + 8, in_gelu, p['wt'], p['biasf'], h2, g2, C + 16, B, H, W, C)
    torch.cuda.synchronize()
    assert_input_kept(buf, src, what)
    ref = dwconv_ref(src.double(), in_gelu, p['w'], p['bias'], B, H, W, C, dtype)
    check_out(hb, h2, C, *ref['h2'], 'h2', what)
    check_out(gb, g2, C, *ref['g2'], 'g2', what)
    return h2[:, :C], g2[:, :C], ref, plan


def run_bwd(shape, dtype, dh2, g1, h1, p, what, form, exact=()):
    """-> (dh1 view, dw view, dbias view, reference, plan).  exact: the parameter gradients that must equal the f64 sums bit for bit"""
    B, H, W, C = shape
    M = B * H * W
    db_, hb_ = padded_in(dh2), padded_in(h1)
    gb_ = padded_in(g1) if g1 is not None else None
    plan = dwconv_plan(B, H, W, C, C + 8, dtype, g1 is not None)['bwd']
    assert plan['form'] == form, f'{what}: the dispatch takes {plan["form"]}, the case is built for {form}'
    ob, dh1 = out2d(M, C, dtype)
    wb, dw = guarded_like(p['dw0'].reshape(-1), DEV)
    bb, dbias = guarded_like(p['db0'], DEV)
    call('fw_dwconv_bwd', dt(dtype), db_, C + 8, gb_, hb_, C + 8, p['wt'], dh1, C + 16, dw, dbias, B, H, W, C)
    torch.cuda.synchronize()
    assert_input_kept(db_, dh2, what)
    assert_input_kept(hb_, h1, what)
    if g1 is not None:
        assert_input_kept(gb_, g1, what)
    ref = dwconv_bwd_ref(dh2.double(), None if g1 is None else g1.double(), h1.double(), p['w'], B, H, W, C, dtype, ld=C + 8,
                         dw0=p['dw0'].double().to(DEV), db0=p['db0'].double().to(DEV))
    check_out(ob, dh1, C, *ref['dh1'], 'dh1', what)
    check_param(wb, dw, *ref['dw'], 'dw', what, exact='dw' in exact, dtype=dtype)
    check_param(bb, dbias, *ref['dbias'], 'dbias', what, exact='dbias' in exact, dtype=dtype)
    return dh1[:, :C], dw.view(C, 9), dbias, ref, plan


def operands(shape, dtype, seed, sign=0):
    B, H, W, C = shape
    M = B * H * W
    h1 = rand_signed((M, C), seed, dtype, sign)
    g1 = gelu64(h1.double()).to(dtype)                                    # the stored twin
    dh2 = rand_signed((M, C), seed + 1, dtype, sign)
    return h1, g1, dh2


# ================================================================================================ P1: every form
FORMS = {S0: ('strip', 'strip+wgrad', 'strip+wgrad'), S1: ('fwd_pipe', 'fused', 'tile+wgrad'), S2: ('fwd_pipe', 'fused', 'tile+wgrad')}


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', [S0, S1, S2], ids=['S0', 'S1', 'S2'])
def test_forms_forward(shape, dtype):
    """forward with in_gelu 0 (the stored g1) and 1 (GELU while the operand is staged): strip, pipe NT 1, pipe NT 2 across borders"""
    h1, g1, _ = operands(shape, dtype, 11)
    p = params(shape[3], 12)
    for in_gelu in (0, 1):
        _, _, _, plan = run_fwd(shape, dtype, h1 if in_gelu else g1, in_gelu, p, f'fwd {shape} in_gelu {in_gelu}', FORMS[shape][0])
    print(f'FORM fwd {shape} {IDS(dtype)}: {plan}')
    if shape == S0:
        assert plan['grid'] == 8 and plan['threads'] <= 3 * 256
    if shape == S2:
        assert (plan['NT'], plan['crossing'], plan['last_walk']) == (2, 4, 1)


@pytest.mark.parametrize('twin', [False, True], ids=['h1', 'g1'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', [S0, S1, S2], ids=['S0', 'S1', 'S2'])
def test_forms_backward(shape, dtype, twin):
    """backward without g1 (strip + wgrad<GIN>, fused) and with it (strip + wgrad, and -- at tiled sizes -- dwconv_tile_kernel<T, 1>
    with dwconv_wgrad_kernel<T, false>: the path the fused LeFF forward's kept g1 takes)"""
    h1, g1, dh2 = operands(shape, dtype, 13)
    p = params(shape[3], 14)
    *_, plan = run_bwd(shape, dtype, dh2, g1 if twin else None, h1, p, f'bwd {shape} g1 {int(twin)}', FORMS[shape][2 if twin else 1])
    print(f'FORM bwd {shape} {IDS(dtype)} g1 {int(twin)}: {plan}')
    assert plan['NSTRIP'] == {S0: 2, S1: 4, S2: 8}[shape]
    if shape == S0:
        assert plan['wgrad_blocks'] == 5 and plan['dead_lanes']
    if shape == S2 and not twin:
        assert (plan['NT'], plan['crossing'], plan['last_walk'], plan['idle']) == (4, 6, 3, 4)


# ================================================================================================ P2: walks at the cap
def assert_cap(plan, raw):
    assert (plan['NT'], plan['raw'], plan['nchunk'], plan['crossing'], plan['last_walk'], plan['idle']) == (32, raw, 2115, 63, 2, 5), plan


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_cap_walk_forward(dtype):
    shape = S3(dtype)
    h1, _, _ = operands(shape, dtype, 21)
    *_, plan = run_fwd(shape, dtype, h1, 1, params(shape[3], 22), f'fwd cap walk {shape}', 'fwd_pipe')
    assert_cap(plan, 33)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_cap_walk_backward_exact_dbias(dtype):
    """dh2 holds integers in {0, 1, 2, 3}: every partial sum of dbias is a non-negative integer below 2^24 (3 * 4 329 600 pixels), so
    dbias must equal the f64 sum bit for bit in ANY order of the atomics; a tile missed or counted twice moves it by an integer."""
    shape = S3(dtype)
    B, H, W, C = shape
    h1, _, _ = operands(shape, dtype, 23)
    dh2 = rand_ints((B * H * W, C), 24, dtype, 0, 3)
    assert 3 * B * H * W + 8 < 2 ** 24
    *_, plan = run_bwd(shape, dtype, dh2, None, h1, params(C, 25, integer=True), f'bwd cap walk {shape}', 'fused', exact=('dbias',))
    assert_cap(plan, 66)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_cap_walk_backward_probe_rows(dtype):
    """dh2 is zero except on twelve tile rows: the first and last row of the first walk, of a middle walk and of the last (2-row)
    walk, and the rows on either side of three image borders.  sum |terms| is then a few hundred terms per dw element and the bound
    is tight: the reference with any ONE probe row left out is rejected at every element of dw and dbias (h1, dh2 and w are
    positive there, so a row's terms cannot cancel)."""
    shape = S3(dtype)
    B, H, W, C = shape
    nty, NT = H // 8, 32
    nrow = B * nty
    last = (nrow - 1) // NT
    probes = [0, NT - 1, 1000 * NT, 1000 * NT + NT - 1, last * NT, nrow - 1] + [k * nty + d for k in (1, 33, 65) for d in (-1, 0)]
    assert nrow - last * NT == 2 and len(set(probes)) == 12 and all(0 <= s < nrow for s in probes)
    h1 = rand_signed((B * H * W, C), 26, dtype, sign=1)
    dh2 = torch.zeros(B, H, W, C, dtype=dtype, device=DEV)
    full = rand_signed((B, H, W, C), 27, dtype, sign=1)
    for s in probes:
        b, y0 = s // nty, s % nty * 8
        dh2[b, y0:y0 + 8] = full[b, y0:y0 + 8]
    dh2 = dh2.view(B * H * W, C)
    del full
    p = params(C, 28, positive=True)
    _, dw, dbias, ref, plan = run_bwd(shape, dtype, dh2, None, h1, p, f'bwd probe rows {shape}', 'fused')
    assert_cap(plan, 66)
    g = gelu64(h1.double())
    for s in probes:
        b, y0 = s // nty, s % nty * 8
        part = dict(zip(('dw', 'dbias'), dwconv_rows_share(dh2.double(), g, B, H, W, C, b, y0, y0 + 8)))
        for name, y in (('dw', dw), ('dbias', dbias)):
            value, tol = ref[name]                                         # the full reference's bound: no tighter than the short one's
            bad = bound_violations(y.reshape(value.shape), value - part[name], tol)
            assert bool(bad.all()), f'{name}: the reference without tile row {s} (image {b}, rows {y0}..{y0 + 7}) is accepted at {int((~bad).sum())} elements'
    print(f'PROBES {IDS(dtype)}: the reference without any one of {len(probes)} tile rows is rejected at every element of dw and dbias')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_cap_shape_backward_with_g1(dtype):
    """dwconv_tile_kernel<T, 1> over 67 650 tiles (one live half of a tile column, 8 / 4 live channels of 64) and 4229 weight-gradient
    blocks of NSTRIP 16"""
    shape = S3(dtype)
    h1, g1, dh2 = operands(shape, dtype, 29)
    *_, plan = run_bwd(shape, dtype, dh2, g1, h1, params(shape[3], 30), f'bwd cap shape with g1 {shape}', 'tile+wgrad')
    assert (plan['NSTRIP'], plan['wgrad_blocks']) == (16, 4229)


# ================================================================================================ P3: the weight gradient free of rounding
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_exact_weight_gradient(dtype):
    """S2 with g1 = multiples of 1/4 in [-2, 2] and dh2 = integers in {0 .. 3}: every product is a multiple of 1/4 of magnitude <= 6
    and every partial sum of the 198 720 pixels stays below 2^24 quarter-units, so dw and dbias (prefill: multiples of 1/4 as well)
    are exact in f32 in any order: the input-centric weight gradient bit for bit"""
    B, H, W, C = S2
    M = B * H * W
    assert M == 198_720 and M * 6 * 4 + 32 < 2 ** 24
    h1 = rand_signed((M, C), 31, dtype)
    g1, dh2 = rand_ints((M, C), 32, dtype, -8, 8, 4), rand_ints((M, C), 33, dtype, 0, 3)
    run_bwd(S2, dtype, dh2, g1, h1, params(C, 34), 'exact dw S2 with g1', 'tile+wgrad', exact=('dw', 'dbias'))


# ================================================================================================ P4: the strip kernels past their grid cap
def second_pass_rejected(y, value, tol, gain, rows, name):
    """what a kernel without its second grid-stride pass leaves: the guarded output's SENTINEL in the elements of its last threads"""
    without = y.detach().clone()
    without[rows] = SENTINEL
    bad = bound_violations(without, value, tol)[rows]
    sel = torch.ones_like(bad) if gain is None else gain[rows] >= GEMM_MIN_GAIN
    share = float(bad[sel].double().mean())
    print(f'SECOND PASS {name}: an output without it is rejected at {share:.4f} of {int(sel.sum())} elements')
    assert share >= MIN_REJECTED


def test_strip_grid_cap():
    """S4, bf16: 2 099 200 threads on 8192 x 256; the second pass owns the last 2048 threads = the last 8 rows of the last image"""
    dtype = BF
    B, H, W, C = S4
    M = B * H * W
    h1, _, dh2 = operands(S4, dtype, 41)
    p = params(C, 42)
    h2, g2, ref, plan = run_fwd(S4, dtype, h1, 1, p, 'fwd strip cap', 'strip')
    assert (plan['grid'], plan['threads'], plan['passes']) == (8192, 2_099_200, 2)
    rows = slice(M - (plan['threads'] - 8192 * 256) // (C // 4) * W, M)   # one thread: 8 pixels x 4 channels; W = 8: an image row is C / 4 threads
    assert M - rows.start == 64
    second_pass_rejected(h2, *ref['h2'], None, rows, 'h2')
    second_pass_rejected(g2, *ref['g2'], None, rows, 'g2')
    del h2, g2, ref
    dh1, _, _, ref, plan = run_bwd(S4, dtype, dh2, None, h1, p, 'bwd strip cap', 'strip+wgrad')
    assert (plan['grid'], plan['passes'], plan['NSTRIP']) == (8192, 2, 16)
    second_pass_rejected(dh1, *ref['dh1'], None, rows, 'dh1')


# ================================================================================================ P5: the 32-bit offset guard
def test_offset_guard():
    """bf16, 1 x 1280 x 128 x 64 in ONE NaN-filled allocation of 1280 * 128 * 13112 elements (4.3 GB; the backward needs two) viewed
    with ld = 13104 (H W ld = 2 146 959 360 < 2^31: the pipelined forward and the fused backward at the largest 32-bit offsets) and
    with ld = 13112 (2 148 270 080 >= 2^31: dwconv_tile_kernel<T, 0, true>, then dwconv_tile_kernel<T, 1> + dwconv_wgrad_kernel<T,
    true>).  Only the 64 live columns are written and read here; the outputs are compact."""
    dtype = BF
    B, H, W, C = 1, 1280, 128, 64
    M = H * W
    free = torch.cuda.mem_get_info()[0]
    if free < 16 * 2 ** 30:
        print(f'SKIP offset guard: {free / 2 ** 30:.1f} GB free, 16 GB asked')
        pytest.skip(f'{free / 2 ** 30:.1f} GB of device memory free, the case asks for 16 GB')
    h1, _, dh2 = operands((B, H, W, C), dtype, 51)
    p = params(C, 52)
    big = [torch.full((M * 13112,), NAN, dtype=dtype, device=DEV) for _ in range(2)]
    ref_f = dwconv_ref(h1.double(), 1, p['w'], p['bias'], B, H, W, C, dtype)
    for ld, ffwd, fbwd in ((13104, 'fwd_pipe', 'fused'), (13112, 'tile', 'tile+wgrad')):
        assert (H * W * ld < 2 ** 31) == (ld == 13104)
        plan = dwconv_plan(B, H, W, C, ld, dtype, False)
        assert (plan['fwd']['form'], plan['bwd']['form']) == (ffwd, fbwd)
        views = [b.as_strided((M, C), (ld, 1)) for b in big]
        views[0].copy_(h1)
        views[1].copy_(dh2)
        what = f'offset guard ld {ld}'
        (hb, h2), (gb, g2), (ob, dh1) = (out2d(M, C, dtype, pad=0) for _ in range(3))
        wb, dw = guarded_like(p['dw0'].reshape(-1), DEV)
        bb, dbias = guarded_like(p['db0'], DEV)
        call('fw_dwconv_fwd', dt(dtype), big[0], ld, 1, p['wt'], p['biasf'], h2, g2, C, B, H, W, C)
        call('fw_dwconv_bwd', dt(dtype), big[1], ld, None, big[0], ld, p['wt'], dh1, C, dw, dbias, B, H, W, C)
        torch.cuda.synchronize()
        check_out(hb, h2, C, *ref_f['h2'], 'h2', what)
        check_out(gb, g2, C, *ref_f['g2'], 'g2', what)
        ref = dwconv_bwd_ref(dh2.double(), None, h1.double(), p['w'], B, H, W, C, dtype, ld=ld, dw0=p['dw0'].double().to(DEV),
                             db0=p['db0'].double().to(DEV))
        check_out(ob, dh1, C, *ref['dh1'], 'dh1', what)
        check_param(wb, dw, *ref['dw'], 'dw', what, dtype=dtype)
        check_param(bb, dbias, *ref['dbias'], 'dbias', what, dtype=dtype)
        for v, src in zip(views, (h1, dh2)):
            assert torch.equal(v, src), f'{what}: an input changed'
            v.fill_(NAN)                                                   # the next view finds an all-NaN allocation again
        print(f'FORM {what}: forward {ffwd}, backward {fbwd}')
    for b in big:
        assert bool(torch.isnan(b).all()), 'offset guard: an element outside the live columns was written'


# ================================================================================================ P6: contract
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', [S0, S1], ids=['S0', 'S1'])
def test_accumulate_twice_and_plain_stores(shape, dtype):
    """dw / dbias are ACCUMULATED into: two calls give prefill + 2 x the sum, each call within its own bound of what it found;
    h2, g2 and dh1 are plain stores: a call into NaN-filled outputs leaves no NaN"""
    B, H, W, C = shape
    M = B * H * W
    h1, _, dh2 = operands(shape, dtype, 61)
    p = params(C, 62)
    run_fwd(shape, dtype, h1, 1, p, f'fwd into NaN {shape}', FORMS[shape][0], fill=NAN)          # every element is checked against its bound
    db_, hb_ = padded_in(dh2), padded_in(h1)
    ob, dh1 = out2d(M, C, dtype, fill=NAN)
    wb, dw = guarded_like(p['dw0'].reshape(-1), DEV)
    bb, dbias = guarded_like(p['db0'], DEV)
    kw = dict(ld=C + 8)
    first = dwconv_bwd_ref(dh2.double(), None, h1.double(), p['w'], B, H, W, C, dtype, dw0=p['dw0'].double().to(DEV),
                           db0=p['db0'].double().to(DEV), **kw)
    second = dwconv_bwd_ref(dh2.double(), None, h1.double(), p['w'], B, H, W, C, dtype, dw0=first['dw'][0], db0=first['dbias'][0], **kw)
    for _ in range(2):
        call('fw_dwconv_bwd', dt(dtype), db_, C + 8, None, hb_, C + 8, p['wt'], dh1, C + 16, dw, dbias, B, H, W, C)
    what = f'two calls {shape}'
    check_out(ob, dh1, C, *first['dh1'], 'dh1', what)
    plain = dwconv_bwd_ref(dh2.double(), None, h1.double(), p['w'], B, H, W, C, dtype, **kw)
    want = p['dw0'].double().to(DEV) + 2 * plain['dw'][0]
    assert float((second['dw'][0] - want).abs().max()) <= 1e-9 * float(want.abs().max())             # prefill + 2 x, stated directly
    check_param(wb, dw, second['dw'][0], first['dw'][1] + second['dw'][1], 'dw', what, dtype=dtype)
    check_param(bb, dbias, second['dbias'][0], first['dbias'][1] + second['dbias'][1], 'dbias', what, dtype=dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', [S0, S1], ids=['S0', 'S1'])
def test_zero_input_gives_the_bias(shape, dtype):
    """an all-zero h1: GELU(0) = 0 keeps the zero padding, so h2 = bias EXACTLY (rounded to the storage type) at every pixel, borders
    included, and g2 = GELU(bias) within its bound"""
    B, H, W, C = shape
    p = params(C, 63)
    h1 = torch.zeros(B * H * W, C, dtype=dtype, device=DEV)
    h2, _, _, _ = run_fwd(shape, dtype, h1, 1, p, f'zero h1 {shape}', FORMS[shape][0])
    assert torch.equal(h2, p['biasf'].to(dtype).expand(B * H * W, C)), 'h2 of a zero input is not the bias'


# ================================================================================================ P7: refused calls
def test_refused_calls_write_nothing():
    """one call per conjunct of the FW_CHECK_ARG lines of both entries: every null pointer, C % e in both types, each row stride % e,
    W % 8, ldg != ld1, sizes <= 0 and a row stride below C.  The unviolated call succeeds first; every refused call raises the
    library's argument error and leaves the guarded outputs untouched."""
    from fwair.lib import parse_header
    protos = parse_header()
    calls = 0
    for dtype, e in ((BF, 8), (F32, 4)):
        B, H, W, C = 1, 8, 16, 16
        M, ld = B * H * W, 32
        src = torch.zeros(M, ld, dtype=dtype, device=DEV)
        wt, bias = torch.zeros(9, C, device=DEV), torch.zeros(C, device=DEV)
        outs = [guarded(M * ld, dtype, DEV) for _ in range(3)]
        pars = [guarded(C * 9, F32, DEV), guarded(C, F32, DEV)]
        (h2, g2, dh1), (dw, dbias) = (v for _, v in outs), (v for _, v in pars)
        fwd = dict(dtype=dt(dtype), g1=src, ld1=ld, in_gelu=1, w=wt, bias=bias, h2=h2, g2=g2, ld2=ld, B=B, H=H, W=W, C=C)
        bwd = dict(dtype=dt(dtype), dh2=src, ldg=ld, g1=src, h1=src, ld1=ld, w=wt, dh1=dh1, ldo=ld, dw=dw, dbias=dbias, B=B, H=H, W=W, C=C)
        assert len(fwd) + 1 == len(protos['fw_dwconv_fwd']) and len(bwd) + 1 == len(protos['fw_dwconv_bwd'])
        call('fw_dwconv_fwd', *fwd.values())
        call('fw_dwconv_bwd', *bwd.values())
        call('fw_dwconv_bwd', *dict(bwd, g1=None).values())               # g1 may be null
        torch.cuda.synchronize()
        for buf, _ in outs + pars:
            buf.fill_(SENTINEL)
        zeros = lambda *names: [{n: 0} for n in names] + [{n: -1} for n in names]
        bad_f = ([{n: None} for n in ('g1', 'w', 'bias', 'h2', 'g2')] + [dict(C=C - e // 2), dict(ld1=ld + e // 2), dict(ld2=ld + e // 2),
                 dict(W=W + 4), dict(ld1=C - e), dict(ld2=C - e)] + zeros('B', 'H', 'W', 'C'))
        bad_b = ([{n: None} for n in ('dh2', 'h1', 'w', 'dh1', 'dw', 'dbias')] + [dict(C=C - e // 2), dict(ld1=ld + e // 2),
                 dict(ldg=ld + e // 2), dict(ldo=ld + e // 2), dict(W=W + 4), dict(ldg=ld - e), dict(ld1=ld + e), dict(ld1=C - e, ldg=C - e),
                 dict(ldo=C - e)] + zeros('B', 'H', 'W', 'C'))
        for name, good, bads in (('fw_dwconv_fwd', fwd, bad_f), ('fw_dwconv_bwd', bwd, bad_b)):
            for change in bads:
                assert set(change) <= set(good)
                with pytest.raises(RuntimeError, match='argument check'):
                    call(name, *dict(good, **change).values())
                calls += 1
        torch.cuda.synchronize()
        for buf, _ in outs + pars:
            assert bool((buf == SENTINEL).all()), 'a refused call wrote to an output'
    print(f'{calls} refused calls')
    assert calls == 2 * (19 + 23)
