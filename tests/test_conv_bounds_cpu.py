"""Host-side proof that the references and bounds of the convolutional plug-ins (tests/helpers.py, csrc/fw_conv.hip) mean something.

  1. the f64 statements agree with torch's own operators (conv2d and its input gradient, unfold, batch_norm and autograd, the
     oracle's differentiable DCNv2 sampler);
  2. an honest emulation of every kernel -- f32 arithmetic, the operand type's rounding where the kernel stores -- stays inside
     every bound, the one-pass BatchNorm variance included at |mean| / std = 0, 1, 8, 64;
  3. each wrong kernel of CONV_MUTATIONS / BN_MUTATIONS / DCN_MUTATIONS puts at least one element outside the bound in every case it
     is parametrised over.  A mutation runs on the cases that HAVE the feature it breaks (a `cin1` split needs two sources, a bias
     order needs a bias and an activation); where a case has the feature and the mutation still provably cannot show, it is listed
     in EXEMPT with its reason -- at most one case per mutation.
No GPU is involved: nothing here is measured against a kernel."""
import pytest
import torch
import torch.nn.functional as F

import convnets_oracle as CO
from helpers import (BN_MUTATIONS, CONV_MUTATIONS, DCN_BORDER_CLASSES, DCN_MUTATIONS, ConvCase, bn_cl_bwd_ref, bn_cl_fwd_ref,
                     bn_inputs, col2im3_bound, col2im3_ref, dcn_bwd_ref, dcn_im2col_ref, dcn_inputs, f32c, im2col3_ref,
                     outside_share, storage_rounding)

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = [F32, BF]
IDS = lambda d: {F32: 'f32', BF: 'bf16'}.get(d, str(d))


def inside(y, value, tol, what):
    share = outside_share(y, value, tol)
    ratio = float(((y.double() - value).abs() / tol.clamp_min(1e-300)).max())
    print(f'{what}: worst error / bound {ratio:.3f}')
    assert share == 0.0, f'{what}: {share:.4f} of the honest emulation lies outside the bound (worst ratio {ratio:.3f})'
    return ratio


def rejected(y, value, tol, what):
    share = outside_share(y, value, tol)
    print(f'{what}: rejected at {share:.4f} of the elements')
    assert share > 0.0, f'{what}: the bound does not tell the mutation from the reference at any element'


# ================================================================================================ convolution
def conv_case(name, dtype, **kw):
    """the host cases: every one has bias, LeakyReLU and a residual; pad columns hold FINITE values here (a kernel that reads them
    must be caught by the values, not by a NaN)"""
    part = 96 if dtype == BF else 80
    spec = dict(k3s1=dict(B=2, H=5, W=18, stride=1, cin=64, cout=27),
                k3s2_two=dict(B=1, H=7, W=19, stride=2, cin=128, cin1=64, cout=16, ldx=136, ldx2=72),
                k1s2_two=dict(B=1, H=6, W=9, stride=2, cin=192, cin1=64, cout=70, k=1, ldx=128, ldx2=128),
                k3_partial=dict(B=1, H=3, W=5, stride=1, cin=part, cout=3))[name]
    return ConvCase(dtype, pad=0.875, seed=3, **spec, **kw)


CONV_CASES = ('k3s1', 'k3s2_two', 'k1s2_two', 'k3_partial')
TWO_SOURCE, STRIDE2 = ('k3s2_two', 'k1s2_two'), ('k3s2_two', 'k1s2_two')
# a mutation -> the cases that have the feature it breaks
CONV_MUTATION_CASES = dict(halo_shift=CONV_CASES, border_clamped=CONV_CASES, bias_after_act=CONV_CASES, res_before_act=CONV_CASES,
                           cin1_off_group=TWO_SOURCE, stride2_at_2o=STRIDE2, taps_not_flipped=('dgrad32', 'dgrad64'))
EXEMPT = {('border_clamped', 'k1s2_two'): 'a 1x1 convolution computes the centre tap only, which never leaves the image'}


def test_exemptions_are_capped():
    assert set(CONV_MUTATION_CASES) == set(CONV_MUTATIONS)
    for m in CONV_MUTATIONS + BN_MUTATIONS + DCN_MUTATIONS:
        assert sum(1 for (mm, _) in EXEMPT if mm == m) <= 1
    for (m, c), reason in EXEMPT.items():
        assert c in CONV_MUTATION_CASES[m] and reason


@pytest.mark.parametrize('stride,k,H,W', [(1, 3, 5, 7), (2, 3, 7, 9), (2, 3, 6, 8), (2, 1, 5, 6), (1, 1, 4, 5)])
def test_conv_reference_is_conv2d(stride, k, H, W):
    """conv3x3_ref through the helper's own panel == torch conv2d (padding k // 2) -> + bias -> LeakyReLU -> + residual, in f64"""
    c = ConvCase(F32, 2, H, W, stride, 32, 5, k=k, cin1=None, seed=1)
    v, _ = c.ref()
    B = 2
    x = c.x[:, :32].double().reshape(B, H, W, 32).permute(0, 3, 1, 2)
    y = F.leaky_relu(F.conv2d(x, c.weight.double(), c.bias.double(), stride, k // 2), f32c(c.slope))        # the slope the ABI receives is an f32
    y = y.permute(0, 2, 3, 1).reshape(-1, 5) + c.res[:, :5].double()
    assert float((v - y).abs().max()) < 1e-12
    assert c.panel.shape == (16, 9 * 32) and float(c.panel[5:].abs().max()) == 0.0           # zero rows above cout


def test_dgrad_panel_is_the_input_gradient():
    """the flipped, transposed panel turns fw_conv3x3 into the input gradient of a stride-1 convolution; unflipped it does not"""
    Co, Ci, B, H, W = 32, 48, 1, 5, 6
    c = ConvCase(F32, B, H, W, 1, Co, Ci, bias=False, act=0, res=False, dgrad=True, seed=2)
    x = torch.zeros(B, Ci, H, W, dtype=F64, requires_grad=True)
    dy = c.x[:, :Co].double().reshape(B, H, W, Co).permute(0, 3, 1, 2)
    F.conv2d(x, c.weight.double(), None, 1, 1).backward(dy)
    want = x.grad.permute(0, 2, 3, 1).reshape(-1, Ci)
    v, tol = c.ref()
    assert float((v - want).abs().max()) < 1e-11
    assert outside_share(want, v, tol) == 0.0


@pytest.mark.parametrize('stride,H,W', [(1, 5, 7), (2, 7, 9), (2, 6, 5)])
def test_im2col_is_unfold_and_col2im_its_adjoint(stride, H, W):
    B, C = 2, 8
    x = torch.randn(B * H * W, C + 4, generator=torch.Generator().manual_seed(H * W), dtype=F64)
    col = im2col3_ref(x, B, H, W, C, stride)
    unf = F.unfold(x[:, :C].reshape(B, H, W, C).permute(0, 3, 1, 2), 3, padding=1, stride=stride)          # [B, C * 9, L]
    want = unf.reshape(B, C, 9, -1).permute(0, 3, 2, 1).reshape(col.shape[0], 9 * C)
    assert torch.equal(col, want)
    cc = torch.randn(col.shape, generator=torch.Generator().manual_seed(1), dtype=F64)
    dx, _ = col2im3_ref(cc, B, H, W, C, stride)
    assert abs(float((col * cc).sum() - (x[:, :C] * dx).sum())) < 1e-9


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('name', CONV_CASES)
def test_conv_emulation_inside_bound(name, dtype):
    c = conv_case(name, dtype)
    v, tol = c.ref()
    y, _ = c.ref(ft=F32)
    inside(y, v, tol, f'conv {name} {IDS(dtype)}')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('mutation,name', [(m, n) for m in CONV_MUTATIONS for n in CONV_MUTATION_CASES[m] if (m, n) not in EXEMPT])
def test_conv_mutation_rejected(mutation, name, dtype):
    if mutation == 'taps_not_flipped':
        ch = int(name[5:])
        kw = dict(dtype=dtype, B=1, H=4, W=17, stride=1, cin=ch, cout=ch + 8, bias=False, act=0, res=False, dgrad=True, seed=4)
        good, bad = ConvCase(**kw), ConvCase(flip=False, **kw)
        (v, tol), (y, _) = good.ref(), bad.ref(ft=F32)
    else:
        c = conv_case(name, dtype)
        (v, tol), (y, _) = c.ref(), c.ref(ft=F32, mutation=mutation)
    rejected(y, v, tol, f'conv {name} {IDS(dtype)} {mutation}')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_col2im_emulation_inside_bound(dtype):
    B, H, W, C, S = 2, 7, 9, 8, 2
    rs = storage_rounding(dtype)
    Mo = B * 4 * 5
    dcol = rs(torch.randn(Mo, 9 * C, generator=torch.Generator().manual_seed(5)))
    dx, mag = col2im3_ref(dcol.double(), B, H, W, C, S)
    y, _ = col2im3_ref(dcol, B, H, W, C, S)
    inside(rs(y), dx, col2im3_bound(dx, mag, dtype), f'col2im {IDS(dtype)}')


# ================================================================================================ BatchNorm
BN_CASES = [(37, 8, 0.0), (130, 192, 1.0), (64, 64, 8.0)]
EPS, MOM = 1e-5, 0.1


def bn_fwd(dtype, rows, C, ratio, ft=F64, mutation=None, training=1, slope=0.1, res=True):
    d = bn_inputs(dtype, rows, C, ratio, seed=6)
    return d, bn_cl_fwd_ref(d['x'], d['gamma'], d['beta'], d['rmean'], d['rvar'], d['res'] if res else None, C, training, EPS, MOM,
                            slope, dtype, ft, mutation)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_bn_reference_is_batch_norm(dtype):
    rows, C = 37, 8
    d, r = bn_fwd(dtype, rows, C, 1.0)
    x = d['x'].double().requires_grad_(True)
    rm, rv = d['rmean'].double().clone(), d['rvar'].double().clone()
    res = d['res'].double().requires_grad_(True)
    y = F.leaky_relu(F.batch_norm(x, rm, rv, d['gamma'].double(), d['beta'].double(), True, f32c(MOM), f32c(EPS)) + res, f32c(0.1))   # the f32 values the ABI receives
    assert float((y.detach() - r['y']).abs().max()) < 1e-12
    assert float((rm - r['rmean']).abs().max()) < 1e-14 and float((rv - r['rvar']).abs().max()) < 1e-14       # unbiased running variance
    y.backward(d['dy'].double())
    b = bn_cl_bwd_ref(d['dy'], y.detach(), d['x'], r['mean'], r['rstd'], d['gamma'], C, 1, 0.1, dtype)
    assert float((b['dx'] - x.grad).abs().max()) < 1e-9 and float((b['dres'] - res.grad).abs().max()) < 1e-14
    # eval: running statistics, nothing updated
    _, e = bn_fwd(dtype, rows, C, 1.0, training=0, slope=1.0, res=False)
    ye = F.batch_norm(d['x'].double(), d['rmean'].double(), d['rvar'].double(), d['gamma'].double(), d['beta'].double(), False, f32c(MOM), f32c(EPS))
    assert float((ye - e['y']).abs().max()) < 1e-12 and torch.equal(e['rvar'], d['rvar'].double())


BN_RATIOS = {}


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('ratio', [0.0, 1.0, 8.0, 64.0])
@pytest.mark.parametrize('rows,C', [(37, 8), (1200, 64), (1, 16)])
def test_bn_one_pass_emulation_inside_bound(rows, C, ratio, dtype):
    """the one-pass variance in f32 against the two-pass f64 reference: the bound holds BECAUSE it carries 1 + mean^2 / var"""
    d, r = bn_fwd(dtype, rows, C, ratio)
    _, e = bn_fwd(dtype, rows, C, ratio, ft=F32)
    for n in ('mean', 'rstd', 'rmean', 'rvar', 'y'):
        inside(e[n], r[n], r['tol_' + n], f'bn fwd rows={rows} C={C} |mean|/std={ratio} {IDS(dtype)} {n}')
    if rows > 1:
        cond = float(r['cond'].median())
        assert 0.5 * (1 + ratio ** 2) < cond < 2 * (1 + ratio ** 2) + 1, cond
    b = bn_cl_bwd_ref(d['dy'], e['y'], d['x'], e['mean'], e['rstd'], d['gamma'], C, 1, 0.1, dtype)
    bb = bn_cl_bwd_ref(d['dy'], e['y'], d['x'], e['mean'], e['rstd'], d['gamma'], C, 1, 0.1, dtype, ft=F32)
    for n in ('dx', 'dres', 'sums'):
        inside(bb[n], b[n], b['tol_' + n], f'bn bwd rows={rows} C={C} {IDS(dtype)} {n}')


def test_bn_bound_without_conditioning_would_fail():
    """the same emulation against a bound WITHOUT the conditioning factor (cond = 1) fails at |mean| / std = 64: the factor is needed"""
    rows, C = 1200, 64
    d, r = bn_fwd(F32, rows, C, 64.0)
    _, e = bn_fwd(F32, rows, C, 64.0, ft=F32)
    err = (e['rstd'].double() - r['rstd']).abs()
    flat = r['tol_rstd'] / r['cond']
    print(f'rstd error / unconditioned bound: {float((err / flat).max()):.2f}; / conditioned bound: {float((err / r["tol_rstd"]).max()):.4f}')
    assert bool((err <= r['tol_rstd']).all())
    assert float((err / flat).max()) > 1.0


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows,C,ratio', BN_CASES)
@pytest.mark.parametrize('mutation', BN_MUTATIONS)
def test_bn_mutation_rejected(mutation, rows, C, ratio, dtype):
    d, r = bn_fwd(dtype, rows, C, ratio)
    what = f'bn rows={rows} C={C} {IDS(dtype)} {mutation}'
    if mutation == 'dres_before_slope':
        b = bn_cl_bwd_ref(d['dy'], r['y'], d['x'], r['mean'], r['rstd'], d['gamma'], C, 1, 0.1, dtype)
        bad = bn_cl_bwd_ref(d['dy'], r['y'], d['x'], r['mean'], r['rstd'], d['gamma'], C, 1, 0.1, dtype, ft=F32, mutation=mutation)
        return rejected(bad['dres'], b['dres'], b['tol_dres'], what)
    _, e = bn_fwd(dtype, rows, C, ratio, ft=F32, mutation=mutation)
    n = 'rvar' if mutation == 'biased_running_var' else 'rstd'
    rejected(e[n], r[n], r['tol_' + n], what)


# ================================================================================================ DCNv2
DCN_CASES = [(1, 5, 7, 8), (2, 4, 6, 72)]


def test_dcn_reference_is_the_oracles_sampler():
    """dcn_im2col_ref / dcn_bwd_ref against the oracle's differentiable bilinear sampler and autograd (offsets on a 1/64 grid, so the
    f32 sample point the reference takes is the f64 one)"""
    B, H, W, C = 2, 4, 5, 8
    d = dcn_inputs(F32, B, H, W, C, seed=7)
    om = d['om']
    om[:, :18] = (om[:, :18] * 64).round() / 64
    M = B * H * W
    x = d['x'].double().reshape(B, H, W, C).permute(0, 3, 1, 2).requires_grad_(True)
    o = om[:, :27].double().reshape(B, H, W, 27).permute(0, 3, 1, 2).requires_grad_(True)
    gy, gx = torch.arange(H, dtype=F64).view(1, H, 1), torch.arange(W, dtype=F64).view(1, 1, W)
    cols = [CO.bilinear_sample(x, gy + (k // 3 - 1) + o[:, 2 * k], gx + (k % 3 - 1) + o[:, 2 * k + 1]) * torch.sigmoid(o[:, 18 + k:19 + k])
            for k in range(9)]
    col = torch.stack(cols, 1).permute(0, 3, 4, 1, 2).reshape(M, 9 * C)
    v, _ = dcn_im2col_ref(d['x'], om, B, H, W, C, F32)
    assert float((v - col).abs().max()) < 1e-12
    col.backward(d['dcol'].double())
    r = dcn_bwd_ref(d['dcol'], d['x'], om, B, H, W, C)
    assert float((r['dx'] - x.grad.permute(0, 2, 3, 1).reshape(M, C)).abs().max()) < 1e-10
    assert float((r['dom'] - o.grad.permute(0, 2, 3, 1).reshape(M, 27)).abs().max()) < 1e-10


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind', ('random',) + DCN_BORDER_CLASSES)
def test_dcn_emulation_inside_bound(kind, dtype):
    B, H, W, C = 2, 4, 6, 8
    d = dcn_inputs(dtype, B, H, W, C, kind, seed=8, logit_scale=30.0 if kind == 'mixed' else 1.0)
    v, tol = dcn_im2col_ref(d['x'], d['om'], B, H, W, C, dtype)
    y, _ = dcn_im2col_ref(d['x'], d['om'], B, H, W, C, dtype, ft=F32)
    inside(y, v, tol + 1e-300, f'dcn im2col {kind} {IDS(dtype)}')
    if kind in ('far_before', 'far_after'):
        assert float(v.abs().max()) == 0.0
    r = dcn_bwd_ref(d['dcol'], d['x'], d['om'], B, H, W, C)
    e = dcn_bwd_ref(d['dcol'], d['x'], d['om'], B, H, W, C, ft=F32)
    inside(e['dx'], r['dx'], r['tol_dx'] + 1e-300, f'dcn dx {kind} {IDS(dtype)}')
    inside(e['dom'], r['dom'], r['tol_dom'] + 1e-300, f'dcn dom {kind} {IDS(dtype)}')


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('B,H,W,C', DCN_CASES)
@pytest.mark.parametrize('mutation', DCN_MUTATIONS)
def test_dcn_mutation_rejected(mutation, B, H, W, C, dtype):
    d = dcn_inputs(dtype, B, H, W, C, seed=9)
    what = f'dcn {B}x{H}x{W}x{C} {IDS(dtype)} {mutation}'
    r = dcn_bwd_ref(d['dcol'], d['x'], d['om'], B, H, W, C)
    e = dcn_bwd_ref(d['dcol'], d['x'], d['om'], B, H, W, C, ft=F32, mutation=mutation)
    if mutation == 'mask_no_sigmoid_grad':
        return rejected(e['dom'][:, 18:], r['dom'][:, 18:], r['tol_dom'][:, 18:], what)
    v, tol = dcn_im2col_ref(d['x'], d['om'], B, H, W, C, dtype)
    y, _ = dcn_im2col_ref(d['x'], d['om'], B, H, W, C, dtype, ft=F32, mutation=mutation)
    rejected(y, v, tol, what + ' col')
    rejected(e['dx'], r['dx'], r['tol_dx'], what + ' dx')
    rejected(e['dom'][:, :18], r['dom'][:, :18], r['tol_dom'][:, :18], what + ' dom')


# ================================================================================================ what BatchNorm sees in the model
def test_resnet_encoder_bn_inputs_are_well_conditioned():
    """DESIGN.md section 2 quotes the |mean| / std of the nine maps BatchNorm normalises in `model_resnet_encoder` (train mode,
    the oracle on the golden's input and the seeded weights): per-channel medians between 0.01 and 0.43, maximum 1.84 at
    E.0.shortcut.1, i.e. a conditioning factor 1 + mean^2 / var of at most 4.4 for the one-pass variance.  Recomputed here."""
    import airnet_oracle as O
    from helpers import load, schema
    prefix = 'E.E.encoder_q.'
    st = {k[len(prefix):]: v for k, v in O.fill_state_seeded(schema('resnet_dgrn')).items() if k.startswith(prefix)}
    upd = {}
    with torch.no_grad():
        CO.resnet_encoder(st, '', load('model_resnet_encoder')['x'], True, upd)
    ratio = {k: m.abs() / v.sqrt() for k, (m, v) in upd.items()}
    assert len(ratio) == 9
    medians = [float(r.median()) for r in ratio.values()]
    worst = max(ratio, key=lambda k: float(ratio[k].max()))
    top = float(ratio[worst].max())
    print(f'|mean|/std: medians {min(medians):.3f} .. {max(medians):.3f}, maximum {top:.3f} at {worst}')
    assert 0.005 < min(medians) and max(medians) < 0.5
    assert worst == 'E.0.shortcut.1.' and 1.7 < top < 2.0 and 1 + top ** 2 < 5.0
