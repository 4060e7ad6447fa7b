"""Host-side proof that the reference, the bounds and the dispatch restatement of the LeFF depthwise 3x3 (tests/helpers.py,
csrc/fw_elem.hip: fw_dwconv_fwd / fw_dwconv_bwd) mean something.

  1. dwconv_plan restates the host dispatch: its constants are read back out of csrc/fw_elem.hip, and the cases of
     tests/test_dwconv_pin_gpu.py reach the forms, walks and caps they are built for;
  2. the f64 statement (nine shifted-slice products) agrees with F.conv2d(F.gelu(.), groups=C) and its autograd to 1e-12;
  3. an honest emulation of the kernels -- operands rounded to storage, f32 fused multiply-adds in two orders, GELU from a port of
     gelu_poly / gelu_grad_poly (coefficients read from csrc/fw_common.h) or from f32 erf, GELU(h1) re-rounded to bf16 (tile and
     pipe forms) or kept in f32 (strip form) -- stays inside every bound;
  4. each wrong kernel of DW_MUTATIONS is rejected at >= 0.99 of the elements it touches.
Which path a mutation is judged on: a mutation of the geometry (halo rows, clamped columns, tap order, dropped blocks, walks) is
judged where the bound carries no GELU approximation term (g1 given / in_gelu = 0), and on dh1 at the elements that pass at least
GEMM_MIN_GAIN of a change of the sum on (|GELU'(h1)| >= 0.5, as check_gemm does); a mutation of GELU itself is judged on the
in-kernel-GELU path with positive weights, h1 and dh2, where the errors of the terms add up instead of cancelling; the exchange of
ky and kx is judged with weights that are antisymmetric under it (w[kx, ky] = -w[ky, kx]), so that no tap equals its transpose.
No GPU is involved: nothing here is measured against a kernel."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers as Hp
from helpers import (DW_MUTATIONS, GEMM_MIN_GAIN, dw_touched, dwconv_bwd_ref, dwconv_plan, dwconv_ref, dwconv_rows_share, dyadic, gelu64,
                     gelu_grad64, signed_magnitudes, storage_rounding)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = [F32, BF]
IDS = lambda d: {F32: 'f32', BF: 'bf16'}.get(d, str(d))
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'frequency-wised_all-in-one_image_restoration_model_amd', 'csrc')
SHAPES = [(3, 24, 40, 72), (2, 12, 24, 40)]
MIN_REJECTED = 0.99


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ================================================================================================ dispatch
def source_constants(text):
    """the dispatch thresholds of fw_dwconv_fwd / fw_dwconv_bwd as csrc/fw_elem.hip states them"""
    one = lambda pat: int(re.search(pat, text).group(1))
    fwd = text[text.index('extern "C" int fw_dwconv_fwd'):text.index('extern "C" int fw_dwconv_bwd')]
    bwd = text[text.index('extern "C" int fw_dwconv_bwd'):text.index('extern "C" int fw_im2col4')]
    ty, tx, cb = (int(v) for v in re.search(r'constexpr int DT_TY = (\d+), DT_TX = (\d+), DT_CB = (\d+);', text).groups())
    vl, sl = (int(v) for v in re.search(r'constexpr int WG_VL = (\d+), WG_SL = (\d+);', text).groups())
    nt_max = {int(v) for part in (fwd, bwd) for v in re.findall(r'NT = NT < 1 \? 1 : \(NT > (\d+) \? (\d+) : NT\);', part)[0]}
    assert len(nt_max) == 1
    assert 'dim3((grid_for(n) + 7) / 8 * 8)' in bwd and '(grid_for(n) + 7) / 8 * 8' in fwd      # the strip grids use grid_for's default cap
    return dict(DW_TILED_MIN=one(r'constexpr long DW_TILED_MIN = (\d+)L;'), DT_TY=ty, DT_TX=tx, DT_CB=cb,
                DW_SX=one(r'constexpr int SX = (\d+);'), WG_VL=vl, WG_SL=sl,
                DW_FWD_WANT=int(re.search(r'constexpr long want = (\d+);', fwd).group(1)),
                DW_BWD_WANT=int(re.search(r'constexpr long want = (\d+);', bwd).group(1)), DW_NT_MAX=nt_max.pop(),
                DW_NSTRIP_MAX=one(r'constexpr int NSTRIP_MAX = (\d+);'), DW_WG_MIN_BLOCKS=one(r'constexpr long wg_min_blocks = (\d+);'),
                DW_STRIP_GRID_CAP=one(r'grid_for\(long n, int cap = (\d+)\)'), DW_TPB=one(r'constexpr int TPB = (\d+);'))


def test_plan_constants_are_the_sources():
    """a threshold edited in fw_elem.hip without dwconv_plan fails here, so no case moves silently onto another kernel"""
    text = source('fw_elem.hip')
    for name, value in source_constants(text).items():
        assert getattr(Hp, name) == value, f'{name}: helpers.py says {getattr(Hp, name)}, csrc/fw_elem.hip says {value}'
    # the shape of the dispatch itself: the conditions dwconv_plan restates, as the source spells them
    for line in ('static bool dw_tiled(int B, int H, int W, int C) { return H % DT_TY == 0 && (long)B * H * W * C >= DW_TILED_MIN; }',
                 'if (dw_tiled(B, H, W, C) && (long)H * W * ld1 < (1L << 31)) {',
                 'if (tiled && !g1 && (long)H * W * ldg < (1L << 31)) {',
                 'while (NSTRIP > 2 && ((nst + (long)NSTRIP * WG_SL - 1) / ((long)NSTRIP * WG_SL)) * nvg < wg_min_blocks) NSTRIP >>= 1;',
                 'long NT = ncol * nrow / want;', 'long nb = ncol * ((nrow + NT - 1) / NT);', 'nb = (nb + 7) / 8 * 8;'):
        assert line in text, f'csrc/fw_elem.hip no longer holds `{line}`: restate dwconv_plan'


def test_plan_of_the_gpu_cases():
    """the properties tests/test_dwconv_pin_gpu.py relies on, computed from the dispatch as it stands"""
    P = lambda B, H, W, C, dtype=BF, g1=False, ld=None: dwconv_plan(B, H, W, C, ld or C + 8, dtype, g1)
    has = lambda d, **kw: all(d[k] == v for k, v in kw.items()) or pytest.fail(f'{d} lacks {kw}')
    for dtype in DTYPES:
        s0 = P(2, 12, 24, 40, dtype)
        has(s0['fwd'], form='strip', grid=8, passes=1) and has(s0['bwd'], form='strip+wgrad', wgrad_blocks=5, dead_lanes=True, NSTRIP=2)
        assert -(-s0['fwd']['threads'] // 256) == 3
        s1 = P(4, 136, 120, 168, dtype)
        has(s1['fwd'], form='fwd_pipe', NT=1) and has(s1['bwd'], form='fused', NT=1, NSTRIP=4)
        has(P(4, 136, 120, 168, dtype, True)['bwd'], form='tile+wgrad', NSTRIP=4)
        s2 = P(9, 920, 24, 72, dtype)
        has(s2['fwd'], form='fwd_pipe', NT=2, crossing=4, last_walk=1)
        has(s2['bwd'], form='fused', NT=4, crossing=6, last_walk=3, idle=4, NSTRIP=8)
        has(P(9, 920, 24, 72, dtype, True)['bwd'], form='tile+wgrad', NSTRIP=8)
    for dtype, C, elems in ((BF, 8, 34_636_800), (F32, 4, 17_318_400)):
        assert 66 * 8200 * 8 * C == elems
        s3 = P(66, 8200, 8, C, dtype)
        has(s3['fwd'], form='fwd_pipe', NT=32, raw=33, nchunk=2115, crossing=63, last_walk=2, idle=5)
        has(s3['bwd'], form='fused', NT=32, raw=66, nchunk=2115, crossing=63, last_walk=2, idle=5, NSTRIP=16)
        has(P(66, 8200, 8, C, dtype, True)['bwd'], form='tile+wgrad', NSTRIP=16, wgrad_blocks=4229)
    s4 = P(2, 4100, 8, 1024)
    has(s4['fwd'], form='strip', grid=8192, threads=2_099_200, passes=2) and has(s4['bwd'], form='strip+wgrad', grid=8192, passes=2, NSTRIP=16)
    # the offset guard: the same allocation viewed with two row strides
    assert 1280 * 128 * 13104 == 2_146_959_360 < 2 ** 31 <= 1280 * 128 * 13112 == 2_148_270_080
    lo, hi = P(1, 1280, 128, 64, ld=13104), P(1, 1280, 128, 64, ld=13112)
    assert (lo['fwd']['form'], lo['bwd']['form']) == ('fwd_pipe', 'fused')
    assert (hi['fwd']['form'], hi['bwd']['form']) == ('tile', 'tile+wgrad')
    # the thresholds from both sides
    assert 64 * 156_248 < Hp.DW_TILED_MIN <= 64 * 156_252
    assert P(1, 8, 8, 156_252)['fwd']['form'] == 'fwd_pipe' and P(1, 8, 8, 156_248)['fwd']['form'] == 'strip'
    assert P(16, 12, 128, 448)['fwd']['form'] == 'strip'                  # H % 8 != 0 never tiles


# ================================================================================================ the reference against torch
def operands(B, H, W, C, dtype, seed, sign=0):
    rs = storage_rounding(dtype)
    M = B * H * W
    s = 100 * seed + C
    h1 = rs(signed_magnitudes(M, C, seed=s + 1, sign=sign))
    dh2 = rs(signed_magnitudes(M, C, seed=s + 2, sign=sign))
    w = signed_magnitudes(C, 9, seed=s + 3, sign=sign)
    bias = signed_magnitudes(C, seed=s + 4)
    g1 = rs(gelu64(h1.double()).float())                                  # the stored twin of GELU(h1)
    sg = lambda *sh, n: torch.randint(0, 2, sh, generator=torch.Generator().manual_seed(s + n)).float() * 2 - 1
    dw0 = dyadic(C, 9, seed=s + 5, lo=4, hi=32, denom=4) * sg(C, 9, n=6)  # |prefill| in [1, 8], multiples of 1/4
    db0 = dyadic(C, seed=s + 7, lo=4, hi=32, denom=4) * sg(C, n=8)
    return {k: v.double() for k, v in dict(h1=h1, dh2=dh2, w=w, bias=bias, g1=g1, dw0=dw0, db0=db0).items()}


@pytest.mark.parametrize('twin', [False, True], ids=['h1', 'g1'])
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_reference_is_conv2d_and_its_autograd(shape, twin):
    B, H, W, C = shape
    o = operands(B, H, W, C, F32, 1)
    h1 = o['h1'].clone().requires_grad_(True)
    w, bias = o['w'].clone().requires_grad_(True), o['bias'].clone().requires_grad_(True)
    img = lambda t: t.view(B, H, W, C).permute(0, 3, 1, 2)
    ref = F.conv2d(img(F.gelu(h1)), w.view(C, 1, 3, 3), bias, padding=1, groups=C).permute(0, 2, 3, 1).reshape(B * H * W, C)
    ref.backward(o['dh2'])
    src = gelu64(o['h1']) if twin else o['h1']                            # the exact activation: the statement, not its stored rounding
    f = dwconv_ref(src, not twin, o['w'], o['bias'], B, H, W, C, F32)
    b = dwconv_bwd_ref(o['dh2'], src if twin else None, o['h1'], o['w'], B, H, W, C, F32, dw0=o['dw0'], db0=o['db0'])
    worst = 0.0
    for got, want in ((f['h2'][0], ref.detach()), (f['g2'][0], F.gelu(ref.detach())), (b['dh1'][0], h1.grad),
                      (b['dw'][0], w.grad + o['dw0']), (b['dbias'][0], bias.grad + o['db0'])):
        worst = max(worst, float(((got - want).abs() / want.abs().clamp_min(1.0)).max()))
    print(f'reference vs torch f64 {shape} twin {twin}: worst relative difference {worst:.2e}')
    assert worst < 1e-12


@pytest.mark.parametrize('rows', [(0, 0, 8), (1, 8, 16), (2, 16, 24)], ids=str)
def test_rows_share_is_the_dropped_part(rows):
    """dwconv_rows_share (what one tile row adds to dw / dbias) == the reference minus the reference with that row dropped: at the
    top of an image, in its middle and at its bottom"""
    B, H, W, C = SHAPES[0]
    o = operands(B, H, W, C, F32, 4)
    full = dwconv_bwd_ref(o['dh2'], None, o['h1'], o['w'], B, H, W, C, F32)
    short = dwconv_bwd_ref(o['dh2'], None, o['h1'], o['w'], B, H, W, C, F32, drop=rows)
    dw, db = dwconv_rows_share(o['dh2'], gelu64(o['h1']), B, H, W, C, *rows)
    assert float((full['dw'][0] - short['dw'][0] - dw).abs().max()) < 1e-10 and float(dw.abs().min()) > 0
    assert float((full['dbias'][0] - short['dbias'][0] - db).abs().max()) < 1e-10


# ================================================================================================ the honest emulation
def poly_coefficients(name):
    body = re.search(r'FW_DEV float ' + name + r'\(float x\) \{(.*?)\n\}', source('fw_common.h'), re.S).group(1)
    c = [float(np.float32(float(v))) for v in re.findall(r'(-?\d\.\d+e[-+]\d+)f', body)]
    assert len(c) == 8, (name, c)
    return c


def fma(a, b, c):
    """one f32 fused multiply-add: the product of two f32 values is exact in f64"""
    return (a.double() * (b.double() if torch.is_tensor(b) else b) + (c.double() if torch.is_tensor(c) else c)).float()


def gelu_kernel(x, dtype, grad=False):
    """gelu_t / gelu_grad_t of csrc/fw_common.h on an f32 tensor"""
    if dtype == BF:
        c = poly_coefficients('gelu_grad_poly' if grad else 'gelu_poly')
        xc = x.clamp(-4.0, 4.0)
        u = xc * xc
        p = torch.full_like(x, c[0])
        for ck in c[1:]:
            p = fma(p, u, ck)
        return fma(xc, p, 0.5) if grad else x * fma(xc, p, 0.5)
    half, r = np.float32(0.5), np.float32(0.70710678118654752440)
    cdf = half * (1 + torch.erf(x * r))
    return cdf + x * (np.float32(0.39894228040143267794) * torch.exp(-half * x * x)) if grad else half * x * (1 + torch.erf(x * r))


def shifted(t4, dy, dx):
    out = torch.zeros_like(t4)
    H, W = t4.shape[1:3]
    ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    out[:, ya:yb, xa:xb] = t4[:, ya + dy:yb + dy, xa + dx:xb + dx]
    return out


def emulate_fwd(o, B, H, W, C, dtype, in_gelu, reverse, reround):
    rs = storage_rounding(dtype)
    x = (o['h1'] if in_gelu else o['g1']).float().view(B, H, W, C)
    if in_gelu:
        x = gelu_kernel(x, dtype)
        if reround:
            x = rs(x)                                                      # tile / pipe forms: GELU(h1) goes to LDS in the operand type
    acc = o['bias'].float().expand(B, H, W, C).clone()
    taps = [(ky, kx) for ky in range(3) for kx in range(3)]
    for ky, kx in (reversed(taps) if reverse else taps):
        acc = fma(shifted(x, ky - 1, kx - 1), o['w'][:, ky * 3 + kx].float(), acc)
    f = lambda t: rs(t).double().reshape(B * H * W, C)
    return f(acc), f(gelu_kernel(acc, dtype))


def emulate_bwd(o, B, H, W, C, dtype, twin, reverse):
    rs = storage_rounding(dtype)
    d, h = o['dh2'].float().view(B, H, W, C), o['h1'].float().view(B, H, W, C)
    acc = torch.zeros_like(d)
    taps = [(ky, kx) for ky in range(3) for kx in range(3)]
    for ky, kx in (reversed(taps) if reverse else taps):
        acc = fma(shifted(d, 1 - ky, 1 - kx), o['w'][:, ky * 3 + kx].float(), acc)
    dh1 = rs(acc * gelu_kernel(h, dtype, grad=True)).double().reshape(B * H * W, C)
    g = o['g1'].float().view(B, H, W, C) if twin else gelu_kernel(h, dtype)           # kept in f32 by both weight-gradient forms

    def total(t):                                                          # f32 sums in two orders, then onto the prefill
        if not reverse:
            return t.sum((0, 1, 2))
        s = torch.zeros(C)
        for row in t.sum(2).reshape(B * H, C).flip(0):
            s = s + row
        return s
    dw = torch.stack([total(g * shifted(d, 1 - ky, 1 - kx)) for ky, kx in taps], 1) + o['dw0'].float()
    return dh1, dw.double(), (total(d) + o['db0'].float()).double()


def ratio(y, value, tol, what):
    r = float(((y - value).abs() / tol.clamp_min(1e-300)).max())
    print(f'EMULATION {what}: worst error / bound {r:.3f}')
    assert r <= 1.0, f'{what}: the honest emulation leaves the bound (worst ratio {r:.3f})'
    return r


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_emulation_inside_bounds(shape, dtype):
    B, H, W, C = shape
    o = operands(B, H, W, C, dtype, 2)
    for in_gelu in (0, 1):
        ref = dwconv_ref(o['h1'] if in_gelu else o['g1'], in_gelu, o['w'], o['bias'], B, H, W, C, dtype)
        for reverse in (False, True):
            for reround in ((False, True) if in_gelu and dtype == BF else (False,)):
                h2, g2 = emulate_fwd(o, B, H, W, C, dtype, in_gelu, reverse, reround)
                tag = f'{IDS(dtype)} {shape} in_gelu {in_gelu} order {int(reverse)} reround {int(reround)}'
                ratio(h2, *ref['h2'], f'h2 {tag}')
                ratio(g2, *ref['g2'], f'g2 {tag}')
    for twin in (False, True):
        ref = dwconv_bwd_ref(o['dh2'], o['g1'] if twin else None, o['h1'], o['w'], B, H, W, C, dtype, dw0=o['dw0'], db0=o['db0'])
        for reverse in (False, True):
            dh1, dw, db = emulate_bwd(o, B, H, W, C, dtype, twin, reverse)
            tag = f'{IDS(dtype)} {shape} g1 {int(twin)} order {int(reverse)}'
            ratio(dh1, *ref['dh1'], f'dh1 {tag}')
            ratio(dw, *ref['dw'], f'dw {tag}')
            ratio(db, *ref['dbias'], f'dbias {tag}')


# ================================================================================================ mutations
GEOMETRY = ('halo_top_neighbour', 'halo_bottom_neighbour', 'col_left_clamped', 'col_right_clamped', 'kykx_swapped', 'cblock_dropped',
            'half_tile_dropped')
# mutation -> the outputs it is judged on
JUDGED = {m: ('h2', 'g2', 'dh1') for m in GEOMETRY}
for m in ('halo_top_neighbour', 'halo_bottom_neighbour', 'col_left_clamped', 'col_right_clamped'):
    JUDGED[m] += ('dw',)
for m in ('cblock_dropped', 'half_tile_dropped'):
    JUDGED[m] += ('dw', 'dbias')
JUDGED.update(taps_not_flipped=('dh1',), beyond_w_counted=('dw', 'dbias'), gelu_missing=('h2', 'g2', 'dw'), gelu_twice=('h2', 'g2', 'dw'),
              gelu_grad_at_gelu=('dh1',), dw_tap_reversed=('dw',), prefill_overwritten=('dw', 'dbias'), tile_row_dropped=('dw', 'dbias'))
GELU_MUTATIONS = ('gelu_missing', 'gelu_twice', 'gelu_grad_at_gelu')


def touched_params(mutation, C, W):
    """-> (dw mask [C, 9], dbias mask [C]): the weight-gradient elements a mutation changes"""
    mw, mb = torch.ones(C, 9, dtype=torch.bool), torch.ones(C, dtype=torch.bool)
    if mutation == 'cblock_dropped':
        mw[:C // 64 * 64] = False
        mb[:C // 64 * 64] = False
    elif mutation in ('halo_top_neighbour', 'halo_bottom_neighbour'):      # dh2 one row above / below the input pixel: ky = 2 / ky = 0
        mw[:] = False
        ky = 2 if mutation == 'halo_top_neighbour' else 0
        mw[:, 3 * ky:3 * ky + 3] = True
    elif mutation in ('col_left_clamped', 'col_right_clamped', 'beyond_w_counted'):
        kx = 2 if mutation != 'col_right_clamped' else 0                   # dh2 left of the input pixel: kx = 2
        mw[:] = False
        mw[:, kx::3] = True
    elif mutation == 'dw_tap_reversed':
        mw[:, 4] = False
    return mw, mb


def test_every_mutation_is_judged():
    assert set(JUDGED) == set(DW_MUTATIONS)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=str)
@pytest.mark.parametrize('mutation', DW_MUTATIONS)
def test_mutation_rejected(mutation, shape, dtype):
    B, H, W, C = shape
    assert W % 16 == 8 and C % 64 and B > 1                               # both shapes carry every feature a mutation breaks
    rs = storage_rounding(dtype)
    gelu_path = mutation in GELU_MUTATIONS
    o = operands(B, H, W, C, dtype, 3, sign=1 if gelu_path else 0)
    if mutation == 'kykx_swapped':                                         # every tap differs from its transpose by 2 |w|
        for ky in range(3):
            for kx in range(ky):
                o['w'][:, kx * 3 + ky] = -o['w'][:, ky * 3 + kx]
    src, in_gelu, g1 = (o['h1'], 1, None) if gelu_path else (o['g1'], 0, o['g1'])
    drop = (B - 1, 8, 16) if mutation == 'tile_row_dropped' else None     # one tile row of the last image
    good = dict(dwconv_ref(src, in_gelu, o['w'], o['bias'], B, H, W, C, dtype),
                **dwconv_bwd_ref(o['dh2'], g1, o['h1'], o['w'], B, H, W, C, dtype, dw0=o['dw0'], db0=o['db0']))
    bad = dict(dwconv_ref(src, in_gelu, o['w'], o['bias'], B, H, W, C, dtype, mutation=mutation),
               **dwconv_bwd_ref(o['dh2'], g1, o['h1'], o['w'], B, H, W, C, dtype, dw0=o['dw0'], db0=o['db0'], mutation=mutation, drop=drop))
    mw, mb = touched_params(mutation, C, W)
    gain = gelu_grad64(o['h1']).abs() >= GEMM_MIN_GAIN
    for name in JUDGED[mutation]:
        value, tol = good[name]
        y = bad[name][0]
        if name in ('h2', 'g2', 'dh1'):
            y, sel = rs(y), dw_touched(mutation, B, H, W, C)
            if name == 'dh1':
                sel = sel & gain
            if name == 'g2':                                               # the twin shows a change of h2 scaled by GELU'(h2)
                sel = sel & (gelu_grad64(good['h2'][0]).abs() >= GEMM_MIN_GAIN)
        else:
            sel = mw if name == 'dw' else mb
        n = int(sel.sum())
        assert n > 0, f'{mutation} touches no element of {name}'
        share = float((~((y - value).abs() <= tol))[sel].double().mean())
        print(f'MUTATION {mutation} {name} {IDS(dtype)} {shape}: rejected at {share:.4f} of {n} touched elements')
        assert share >= MIN_REJECTED, f'{mutation}: {name} rejected at {share:.4f} of its {n} touched elements only (asked: {MIN_REJECTED})'
