"""fw_layernorm_bwd_slab: LayerNorm backward that takes dy straight from the unfolded slab of a split-K input-gradient GEMM, and the
autograd hand-over that feeds it (ops.dgrad(lazy=True) -> functional.LnResFn / LayerNormFn backward).

  * dx and twin must be, bit for bit, those of the three launches it replaces: fw_slab_reduce -> fw_cast_rows -> fw_layernorm_bwd2;
  * dgamma / dbeta (block partials folded by fw_slab_reduce) are held to an f64 evaluation on the host of the SAME operands -- the dy
    the chain produced, x, and the mean / rstd the kernel reads -- within the rounding chain of the sum:
        term   dy * xhat, xhat = (x - mean) * rstd : two roundings for xhat, one for the product (none more if it is fused)
        sum    `rows` terms in ANY order (lane registers, the ordered LDS fold, the fold of the block partials, the add into the
               zeroed dgamma): at most rows additions on the path of a term
    so |got - ref| <= (rows + 4) u sum_r |dy xhat|  (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), u = 2^-24,
    and (rows + 1) u sum_r |dy| for dbeta, whose terms are exact.  Nothing in it is fitted to a run;
  * the fold is ordered: the same call twice gives the same dgamma / dbeta bits."""
import functools

import pytest
import torch

from test_model_layouts_gpu import DEV, DTYPES, call, dt, ln_blocks, ops
from test_ops_gpu import close, rnd

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
RPS = 64                                   # tw_rows_per_scale


def step_rows(C):
    """rows one workgroup of ln_bwd_kernel takes per step: (threads / G) lane groups x U rows (ln_bwd_dispatch of csrc/fw_norm.hip)"""
    G = 8 if C <= 32 else 16 if C <= 64 else 32 if C <= 128 else 64
    U = 4 if C <= 256 else 2 if C <= 512 else 1
    return (512 if C > 128 else 256) // G * U


def grid_cap(C):
    return 256 if C > 512 else 512 if C > 128 else 1024


def case_rows(C, kind):
    """'ragged': three full steps and one row (the last workgroup's only step is ragged); 'wrap': more row groups than the grid cap, so
    the persistent walk takes a second, ragged, pass (2 100 rows at C = 896)."""
    return 3 * step_rows(C) + 1 if kind == 'ragged' else grid_cap(C) * step_rows(C) + 6 * step_rows(C) + 4


@functools.lru_cache(maxsize=2)
def problem(rows, C):
    x, g = rnd(rows, C) * 2 + 0.3, 1 + 0.1 * rnd(C, seed=1)
    xd, gd = x.to(DEV), g.to(DEV)
    _, mean, rstd = ops().layernorm_fwd(xd, gd, torch.zeros(C, device=DEV), torch.float32)
    dres = rnd(rows, C, seed=4).to(DEV)
    scale = (0.5 + torch.arange((rows + RPS - 1) // RPS, dtype=torch.float32) % 3).to(DEV)
    return xd, gd, mean, rstd, dres, scale


@functools.lru_cache(maxsize=2)
def slab_of(rows, C, nz):
    """[nz, S] with S > rows * C the way ops.dgrad pads it -- and then some: NaN behind every slice, which no one may read"""
    S = (rows * C + 3) // 4 * 4 + 64
    slab = torch.full((nz, S), float('nan'), device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5 + nz)
    slab[:, :rows * C] = torch.randn(nz, rows * C, device=DEV, generator=gen) * 0.5       # on the device: up to 59 M values
    return slab, S


def run_chain(dtype, slab, nz, S, p, rows, C, dres, twin, scale):
    xd, gd, mean, rstd = p
    tmp = torch.empty(rows, C, device=DEV)
    dy = torch.empty(rows, C, dtype=dtype, device=DEV)
    call('fw_slab_reduce', slab, nz, rows * C, S, tmp, 0, None, 0, 0)
    call('fw_cast_rows', dt(dtype), tmp, C, dy, C, rows, C, None, 1)
    dx = torch.empty(rows, C, device=DEV)
    partial = torch.empty((ln_blocks(rows, C), 2 * C), device=DEV)
    call('fw_layernorm_bwd2', dt(dtype), dy, C, xd, C, gd, mean, rstd, dres, C if dres is not None else 0, dx, C, None, None, partial,
         rows, C, twin, C if twin is not None else 0, scale, RPS)
    return dy, dx


def run_slab(dtype, slab, nz, S, p, rows, C, dres, twin, scale, fold=1):
    """-> dx, dgamma, dbeta (the block partials folded into zeros by fw_slab_reduce(accumulate = fold)), partial"""
    xd, gd, mean, rstd = p
    dx = torch.empty(rows, C, device=DEV)
    partial = torch.full((ln_blocks(rows, C), 2 * C), float('nan'), device=DEV)
    call('fw_layernorm_bwd_slab', dt(dtype), None, 0, slab, nz, S, xd, C, gd, mean, rstd, dres, C if dres is not None else 0, dx, C,
         None, None, partial, rows, C, twin, C if twin is not None else 0, scale, RPS)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    call('fw_slab_reduce', partial, partial.shape[0], C, 2 * C, dg, fold, db, C, C)
    return dx, dg, db, partial


def check_against_f64(dy, p, rows, dx, dres, dg, db, what):
    """dx by the limit tests/test_model_layouts_gpu.py holds fw_layernorm_bwd2 to (1e-4 of the largest element); dgamma, dbeta by the
    bound of this file's docstring"""
    xd, gd, mean, rstd = p
    d = dy.double().cpu()
    xh = (xd.double().cpu() - mean.double().cpu()[:, None]) * rstd.double().cpu()[:, None]
    t = d * xh
    g = d * gd.double().cpu()
    ref = rstd.double().cpu()[:, None] * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    close(dx, ref + (dres.double().cpu() if dres is not None else 0), 1e-4, f'{what} dx')
    for name, got, ref, mag, n in (('dgamma', dg, t.sum(0), t.abs().sum(0), rows + 4), ('dbeta', db, d.sum(0), d.abs().sum(0), rows + 1)):
        err = (got.double().cpu() - ref).abs()
        bound = n * U32 * mag
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f'{what} {name}: max |err| {float(err.max()):.3e}, worst err / bound {worst:.3f}')
        assert torch.isfinite(got).all() and bool((err <= bound).all()), f'{what} {name}: error is {worst:.2f} x its bound'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('nz', [2, 3, 4, 16])
@pytest.mark.parametrize('kind', ['ragged', 'wrap'])
@pytest.mark.parametrize('C', [28, 224, 448, 896])
def test_slab_entry_equals_fold_cast_ln(dtype, nz, kind, C):
    rows = case_rows(C, kind)
    if kind == 'wrap':
        assert rows > ln_blocks(rows, C) * step_rows(C), 'the walk must wrap: the grid cap moved'
    else:
        assert ln_blocks(rows, C) == 4, 'three full steps and a ragged fourth: the step moved'
    xd, gd, mean, rstd, dres_, scale_ = problem(rows, C)
    p = (xd, gd, mean, rstd)
    slab, S = slab_of(rows, C, nz)
    for with_dres in (False, True):
        for with_twin in (False, True):
            what = f'C={C} rows={rows} nz={nz} dres={with_dres} twin={with_twin}'
            dres = dres_ if with_dres else None
            tw_a = torch.full((rows, C), 7.0, dtype=dtype, device=DEV) if with_twin else None
            tw_b = torch.full((rows, C), 7.0, dtype=dtype, device=DEV) if with_twin else None
            scale = scale_ if with_twin else None
            dy, dx_a = run_chain(dtype, slab, nz, S, p, rows, C, dres, tw_a, scale)
            dx_b, dg, db, _ = run_slab(dtype, slab, nz, S, p, rows, C, dres, tw_b, scale)
            assert torch.isfinite(dx_b).all(), what
            assert torch.equal(dx_a.view(torch.int32), dx_b.view(torch.int32)), f'{what}: dx differs from the three-launch chain'
            if with_twin:
                it = torch.int32 if dtype == torch.float32 else torch.int16
                assert torch.equal(tw_a.view(it), tw_b.view(it)), f'{what}: twin differs from the three-launch chain'
            if with_dres == with_twin:
                check_against_f64(dy, p, rows, dx_b, dres, dg, db, what)


@pytest.mark.parametrize('dtype', DTYPES)
def test_ordered_fold_repeats_its_bits(dtype):
    C, nz = 896, 3
    rows = case_rows(C, 'wrap')
    xd, gd, mean, rstd, dres, _ = problem(rows, C)
    slab, S = slab_of(rows, C, nz)
    # accumulate = 2: the fold of the block partials that keeps one z range per address (no atomics), so that what is compared is the kernel
    _, dg1, db1, p1 = run_slab(dtype, slab, nz, S, (xd, gd, mean, rstd), rows, C, dres, None, None, fold=2)
    _, dg2, db2, p2 = run_slab(dtype, slab, nz, S, (xd, gd, mean, rstd), rows, C, dres, None, None, fold=2)
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)), 'block partials differ between two identical calls'
    assert torch.equal(dg1.view(torch.int32), dg2.view(torch.int32)) and torch.equal(db1.view(torch.int32), db2.view(torch.int32))
    assert float(dg1.abs().max()) > 0 and float(db1.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ autograd: LayerNorm -> Linear(448 -> 1792)
B, HW, C_, N_ = 2, 16 * 16, 448, 1792


def _ln_linear(dtype, lazy, heads, monkeypatch):
    """LnResFn -> `heads` Linears on its output, backward from fixed cotangents on the outputs and on the residual stream.
    -> (dx of the stream, dgamma, dbeta, [(lazy asked, lazy taken) per ops.dgrad call], [sum_r |dy xhat|, sum_r |dy|] per column in
    f64 -- None when the LayerNorm backward got its dy as a slab)"""
    from fwair import functional as Fn
    monkeypatch.setattr(Fn.config, 'compute_dtype', dtype)
    monkeypatch.setattr(Fn.config, 'lazy_dgrad', lazy)
    went, mags = [], []
    real_dgrad, real_ln = ops().dgrad, ops().layernorm_bwd

    def spy_dgrad(*a, **k):
        r = real_dgrad(*a, **k)
        went.append((bool(k.get('lazy')), bool(r)))
        return r

    def spy_ln(dy, x, gamma, mean, rstd, *a, **k):
        if getattr(dy, '_fw_slab', None) is None:
            d = dy.double().cpu()
            xh = (x.double().cpu() - mean.double().cpu()[:, None]) * rstd.double().cpu()[:, None]
            mags.extend([(d * xh).abs().sum(0), d.abs().sum(0)])
        return real_ln(dy, x, gamma, mean, rstd, *a, **k)
    monkeypatch.setattr(ops(), 'dgrad', spy_dgrad)
    monkeypatch.setattr(ops(), 'layernorm_bwd', spy_ln)
    rows = B * HW
    x = (rnd(rows, C_) * 2 + 0.3).to(DEV).requires_grad_(True)
    gamma = (1 + 0.1 * rnd(C_, seed=1)).to(DEV).requires_grad_(True)
    beta = (0.1 * rnd(C_, seed=2)).to(DEV).requires_grad_(True)
    ws = [(rnd(N_, C_, seed=10 + i) * 0.05).to(DEV).requires_grad_(True) for i in range(heads)]
    res, xn = Fn.LnResFn.apply(x, gamma, beta)
    ys = [Fn.linear(xn, w) for w in ws]
    cot = [rnd(rows, N_, seed=20 + i).to(DEV, dtype) for i in range(heads)]
    torch.autograd.backward(ys + [res], cot + [rnd(rows, C_, seed=30).to(DEV)])
    torch.cuda.synchronize()
    monkeypatch.setattr(ops(), 'dgrad', real_dgrad)
    monkeypatch.setattr(ops(), 'layernorm_bwd', real_ln)
    return x.grad, gamma.grad, beta.grad, went, mags or None


def _same_sums(a, b, mag, what):
    """two f32 evaluations, in different orders, of column sums of the same B * HW terms: each is within (rows + 4) u sum |terms| of
    the exact sum (this file's docstring), so they are within twice that of each other"""
    err = (a - b).abs().double().cpu()
    bound = 2 * (B * HW + 4) * U32 * mag
    print(f'{what}: max |difference| {float(err.max()):.3e}, worst difference / bound {float((err / bound).max()):.3f}')
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize('dtype', DTYPES)
def test_autograd_single_consumer_goes_lazy(dtype, monkeypatch):
    dx0, dg0, db0, went0, mags = _ln_linear(dtype, False, 1, monkeypatch)
    dx1, dg1, db1, went1, none = _ln_linear(dtype, True, 1, monkeypatch)
    # ops.dgrad splits this product (16 output tiles, 1792 reduction rows); switched on, it left the result to the slab
    assert went0 == [(False, False)] and went1 == [(True, True)] and none is None, (went0, went1)
    assert torch.isfinite(dx1).all()
    assert torch.equal(dx0.view(torch.int32), dx1.view(torch.int32)), 'dx differs from the unfused path'
    _same_sums(dg0, dg1, mags[0], 'dgamma')
    _same_sums(db0, db1, mags[1], 'dbeta')


@pytest.mark.parametrize('dtype', DTYPES)
def test_autograd_two_consumers_stay_eager(dtype, monkeypatch):
    dx0, dg0, db0, went0, mags = _ln_linear(dtype, False, 2, monkeypatch)
    dx1, dg1, db1, went1, mags1 = _ln_linear(dtype, True, 2, monkeypatch)
    assert went1 == [(False, False)] * 2 and went0 == went1 and mags1 is not None, (went0, went1)      # nobody asked for the lazy mode
    assert torch.equal(dx0.view(torch.int32), dx1.view(torch.int32))
    _same_sums(dg0, dg1, mags[0], 'dgamma')
    _same_sums(db0, db1, mags[1], 'dbeta')
