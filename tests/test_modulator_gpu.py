"""The decoder's learnable window modulator (--learnable_modulator, decoder_Uformer.py:536-539,687-691) on the GPU.
Kernels (csrc/fw_norm.hip): fw_layernorm_mod_fwd differentially against fw_layernorm_fwd -- a kernel the existing tests pin -- with a
derived element bound, fw_modulator_bwd against the f64 sum over windows with Higham's any-order summation bound.  Then the modulated
LayerNorm Function against f64 autograd, the model against goldens of the reference built with the flag
(tests/golden/make_golden_modulator.py), and a graph-captured training step."""
import pytest
import torch
import torch.nn.functional as F

import airnet_oracle as O
from helpers import (GUARD, SENTINEL, U32, assert_bits, assert_within_bound, close, guarded, load, make_opt, rejected_share, rnd,
                     signed_magnitudes, synth_batch)
from modulator_cases import (B, GEOS, MIN_REJECTED, SHIFTS, WIDTHS, fwd_bound, reseed_tables, schema_modulator, unit_table, window_add,
                             window_pos, wrong_positions)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.float32, torch.bfloat16]
NAN = float('nan')
GRAD_GEOS = [(H, W, C) for H, W in GEOS for C in WIDTHS] + [(64, 64, 112)]        # 64 x 64: more than one slice, the fold runs
_plain, _state = {}, []


def call(*a):
    from fwair.lib import call as _c
    return _c(*a)


def dt(dtype):
    from fwair.lib import dt as _dt
    return _dt(dtype)


def slices(rows, C):
    from fwair.lib import lib
    return lib().fw_modulator_bwd_blocks(rows, C)


def plain(H, W, C):
    """x, gamma, beta and the PLAIN kernel's own f32 output, mean and rstd on them: computed once per shape, never modified"""
    key = (H, W, C)
    if key not in _plain:
        rows = B * H * W
        x = (rnd(f'mod.x.{H}x{W}x{C}', (rows, C)) * 2 + 0.3).to(DEV)
        g, b = (1 + 0.1 * rnd(f'mod.g{C}', (C,))).to(DEV), (0.1 * rnd(f'mod.b{C}', (C,))).to(DEV)
        y0 = torch.empty(rows, C, device=DEV)
        mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
        call('fw_layernorm_fwd', dt(torch.float32), x, C, g, b, y0, C, mean, rstd, rows, C, 1e-5)
        _plain[key] = (x, g, b, y0.cpu().double(), mean, rstd, unit_table(f'mod.table{C}', C))
    return _plain[key]


def check_forward(y, y0, table, H, W, s, dtype, what):
    p = window_pos(B, H, W, s)
    value, tol = y0 + table.double()[p], fwd_bound(y0, table.double()[p], dtype)
    y = y.float().cpu()
    assert torch.equal(value, window_add(y0, table.double(), B, H, W, s)), 'index formula vs the restated window add'
    assert_within_bound(y, value, tol, what)
    for name, pw in wrong_positions(B, H, W, s).items():          # the same output must NOT fit a wrong kernel's expectation
        differs = pw != p                                            # 7/8 of the rows (all for the shift): test_modulator_cpu.py
        m = table.double()[pw]
        share, _ = rejected_share(y[differs], (y0 + m)[differs], fwd_bound(y0, m, dtype)[differs])
        assert share >= MIN_REJECTED, f'{what}: fits the `{name}` expectation at {1 - share:.4f} of the elements where it differs'


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('C', WIDTHS)
@pytest.mark.parametrize('s', SHIFTS)
@pytest.mark.parametrize('H,W', GEOS)
def test_layernorm_mod_fwd(H, W, s, C, dtype):
    """y = T(y0 + mod[p]) with y0 the plain kernel's f32 output on the same x: |y - (y0 + mod[p])| <= 2 * 2^-24 (|y0| + |mod[p]|)
    (+ 2^-8 |y0 + mod[p]| in bf16); mean and rstd bit-equal to the plain kernel's."""
    x, g, b, y0, mean0, rstd0, table = plain(H, W, C)
    rows = B * H * W
    y = torch.empty(rows, C, dtype=dtype, device=DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    call('fw_layernorm_mod_fwd', dt(dtype), x, C, g, b, table.to(DEV), y, C, mean, rstd, rows, C, H, W, s, 1e-5)
    assert_bits(mean, mean0, 'mean')
    assert_bits(rstd, rstd0, 'rstd')
    check_forward(y, y0, table, H, W, s, dtype, f'mod fwd {H}x{W} s={s} C={C}')


@pytest.mark.parametrize('dtype', DTYPES)
def test_layernorm_mod_fwd_padded_rows(dtype):
    """ldx, ldy > C, the way functional.act_empty hands rows out: NaN in the pad columns of x, 7.0 in those of y must survive"""
    H, W, s, C, ld = 16, 24, 4, 112, 120
    x, g, b, y0, mean0, rstd0, table = plain(H, W, C)
    rows = B * H * W
    xb = torch.full((rows, ld), NAN, device=DEV)
    xb[:, :C] = x
    yb = torch.full((rows, ld), 7.0, dtype=dtype, device=DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    call('fw_layernorm_mod_fwd', dt(dtype), xb, ld, g, b, table.to(DEV), yb, ld, mean, rstd, rows, C, H, W, s, 1e-5)
    assert bool((yb[:, C:].float() == 7.0).all()), 'forward wrote into the pad columns of y'
    assert_bits(mean, mean0, 'mean')
    assert_bits(rstd, rstd0, 'rstd')
    check_forward(yb[:, :C], y0, table, H, W, s, dtype, 'mod fwd, padded rows')


def last_window_rows(H, W, s):
    """rows of the last window (of the rolled image) of the last image: one row for every p"""
    r = torch.arange(B * H * W)
    b, yy, xx = r // (H * W), (r // W) % H, r % W
    return (b == B - 1) & ((yy - s) % H >= H - 8) & ((xx - s) % W >= W - 8)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('s', SHIFTS)
@pytest.mark.parametrize('H,W,C', GRAD_GEOS)
def test_modulator_bwd(H, W, C, s, dtype):
    """dmod[p] = prefill + sum over the n = rows / 64 rows with p(r) = p of dy[r], within (n + 1) 2^-24 (sum |dy| + |prefill|)
    (any order of summation, tests/helpers.py); the bound tells a missing window; two calls agree bit for bit; partials + fold
    (dmod == NULL) give the immediate form."""
    rows = B * H * W
    n, nz = rows // 64, slices(rows, C)
    if (H, W) == (64, 64):
        assert nz > 1, 'this case is here for the fold across slices'
    dy = signed_magnitudes(rows, C, seed=H + s).to(dtype)
    assert float(dy.float().abs().min()) >= 0.75
    prefill = torch.linspace(0.5, 1.5, 64 * C).view(64, C)
    p = window_pos(B, H, W, s)
    dy64 = dy.double()
    total = torch.zeros(64, C, dtype=torch.float64).index_add_(0, p, dy64)
    mag = torch.zeros(64, C, dtype=torch.float64).index_add_(0, p, dy64.abs()) + prefill.double()
    tol = (n + 1) * U32 * mag
    assert float(tol.max()) < 1e-2
    dyd = dy.to(DEV)
    outs = []
    for _ in range(2):
        dbuf, dmod = guarded(64 * C, torch.float32, DEV)
        dmod.copy_(prefill.reshape(-1))
        pbuf, partial = guarded(nz * 64 * C, torch.float32, DEV)
        call('fw_modulator_bwd', dt(dtype), dyd, C, dmod, partial, rows, C, H, W, s)
        for buf in (dbuf, pbuf):
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all()), 'wrote outside its buffers'
        outs.append(dmod.view(64, C).cpu())
    assert_bits(outs[0], outs[1], 'two identical calls')
    assert_within_bound(outs[0], prefill.double() + total, tol, f'dmod {H}x{W} s={s} C={C}')
    lw = last_window_rows(H, W, s)
    assert int(lw.sum()) == 64 and sorted(p[lw].tolist()) == list(range(64))
    short = torch.zeros(64, C, dtype=torch.float64).index_add_(0, p[~lw], dy64[~lw])
    share, _ = rejected_share(outs[0], prefill.double() + short, tol)
    assert share >= MIN_REJECTED, f'the bound tells a missing window at {share:.4f} of the elements only'
    # deferred form: slices by plain stores, folded by the caller
    partial = torch.empty(nz, 64 * C, device=DEV)
    call('fw_modulator_bwd', dt(dtype), dyd, C, None, partial, rows, C, H, W, s)
    d2 = prefill.clone().to(DEV)
    call('fw_slab_reduce', partial, nz, 64 * C, 64 * C, d2, 1, None, 0, 0)
    close(d2, outs[0], 1e-6, 'partials folded by fw_slab_reduce vs the immediate form')


@pytest.mark.parametrize('dtype', DTYPES)
def test_modulator_bwd_padded_rows(dtype):
    """dy as rows of a wider buffer with NaN in the pad columns (bf16: rows that are 8-byte but not 16-byte aligned as well)"""
    H, W, s, C = 16, 24, 4, 28
    rows = B * H * W
    for ld in (32, 36):
        dy = signed_magnitudes(rows, C, seed=ld).to(dtype)
        buf = torch.full((rows, ld), NAN, dtype=dtype, device=DEV)
        buf[:, :C] = dy.to(DEV)
        p = window_pos(B, H, W, s)
        total = torch.zeros(64, C, dtype=torch.float64).index_add_(0, p, dy.double())
        mag = torch.zeros(64, C, dtype=torch.float64).index_add_(0, p, dy.double().abs())
        dmod = torch.zeros(64, C, device=DEV)
        partial = torch.empty(slices(rows, C), 64 * C, device=DEV)
        call('fw_modulator_bwd', dt(dtype), buf, ld, dmod, partial, rows, C, H, W, s)
        assert_within_bound(dmod.cpu(), total, (rows // 64 + 1) * U32 * mag, f'dmod, ld = {ld}')


@pytest.mark.parametrize('dtype', DTYPES)
def test_modulated_layernorm_function(dtype):
    """LnResModFn against f64 torch autograd of layer_norm(x) * gamma + beta + table[p], (B, H, W, C, s) = (2, 16, 24, 112, 4):
    y, dx with a residual gradient, dgamma, dbeta, dmod at the limits of test_layernorm_bwd_many_passes (1e-4, rel-to-max).  The
    gradient the Function receives is of the compute type, so the reference is given that rounded dy; a bf16 y is one rounding of
    the format (2^-8 |y|) away from the value on top of the same 1e-4."""
    from fwair import functional as Fn
    H, W, s, C = 16, 24, 4, 112
    rows = B * H * W
    x = rnd('modfn.x', (rows, C)) * 2 + 0.3
    g, b, table = 1 + 0.1 * rnd('modfn.g', (C,)), 0.1 * rnd('modfn.b', (C,)), unit_table('modfn.table', C)
    dy, dres = rnd('modfn.dy', (rows, C)).to(dtype), rnd('modfn.dres', (rows, C))
    p = window_pos(B, H, W, s)
    ref = [t.double().requires_grad_(True) for t in (x, g, b, table)]
    y_ref = F.layer_norm(ref[0], (C,), ref[1], ref[2]) + ref[3][p]
    y_ref.backward(dy.double())
    keep = Fn.config.compute_dtype
    try:
        Fn.config.compute_dtype = dtype
        leaf = [t.to(DEV).requires_grad_(True) for t in (x, g, b, table)]
        xo, y = Fn.LnResModFn.apply(leaf[0], leaf[1], leaf[2], leaf[3], (H, W, s))
        torch.autograd.backward((xo, y), (dres.to(DEV), dy.to(DEV)))
    finally:
        Fn.config.compute_dtype = keep
    assert y.dtype == dtype
    if dtype == torch.float32:
        close(y, y_ref, 1e-4, 'y')
    else:
        yr = y_ref.detach()
        assert_within_bound(y.float().cpu(), yr, 2.0 ** -8 * yr.abs() + 1e-4 * float(yr.abs().max()), 'y (bf16)')
    close(leaf[0].grad, ref[0].grad + dres.double(), 1e-4, 'dx')
    close(leaf[1].grad, ref[1].grad, 1e-4, 'dgamma')
    close(leaf[2].grad, ref[2].grad, 1e-4, 'dbeta')
    close(leaf[3].grad, ref[3].grad, 1e-4, 'dmod')


# ---------------------------------------------------------------------------------------------------------------- model
def state():
    """seeded weights with the tables at unit variance, built once for the module and never modified"""
    if not _state:
        st = O.fill_state_seeded(schema_modulator())
        assert len(reseed_tables(st)) == 20
        _state.append(st)
    return _state[0]


def make(st, dtype, **kw):
    from net.model import AirNet
    from fwair import functional as Fn
    opt = make_opt('all3', batch_size=1, compute_dtype=dtype, learnable_modulator=True, **kw)
    net = AirNet(opt)
    sd = net.state_dict()
    for key in sd:
        if st.get(key) is not None and sd[key].is_floating_point():
            sd[key] = st[key]
    net.load_state_dict(sd)
    Fn.set_droppath_override(lambda name, n, rate, device: None)      # DropPath off (the golden was made that way)
    return net.to(DEV), opt


def test_model_fp32_and_bf16_against_reference_golden():
    g = load('model_all3_modulator')
    clean, q, k = synth_batch(1, 128, 'modulator.')
    st = state()
    net, opt = make(st, 'fp32')
    net.eval()
    with torch.no_grad():
        out = net(x_query=q.to(DEV), x_key=q.to(DEV))
    close(out, g['restored_eval'], 1e-4, 'restored_eval vs reference golden')
    net.train()
    restored, logits, labels = net(x_query=q.to(DEV), x_key=k.to(DEV))
    close(restored, g['restored_train'], 1e-4, 'restored_train')
    close(torch.stack(logits), g['logits'], 2e-4, 'logits')
    CE = torch.nn.CrossEntropyLoss()
    contrast = sum(CE(logits[i], labels[i]) for i in range(opt.L)) / opt.L
    loss = torch.nn.L1Loss()(restored, clean.to(DEV)) + opt.contrast_loss_weight * contrast
    close(loss, g['loss'], 1e-4, 'loss')
    loss.backward()
    names = [str(n) for n in g['grad_names']]
    assert sum(n.endswith('.modulator.weight') for n in names) == 20
    params = dict(net.named_parameters())
    norms = torch.tensor([params[n].grad.norm().item() for n in names])
    floor = float(g['grad_norms'].max()) * 1e-5                        # the gradient-norm rule of the 256 / 384 tests
    rel = ((norms - g['grad_norms']).abs() / g['grad_norms'].clamp_min(floor))
    worst = int(rel.argmax())
    print(f'modulator fp32: worst grad-norm deviation {float(rel.max()):.3e} at {names[worst]}')
    assert rel.max() < 5e-3, f'grad norm of {names[worst]}: {norms[worst]:.6e} vs {g["grad_norms"][worst]:.6e}'
    gmax = float(g['grad_norms'].max())
    tables = 0
    for key, val in g.items():
        if key.startswith('g.'):
            is_table = key.endswith('.modulator.weight')
            tables += is_table
            close(params[key[2:]].grad, val, 5e-3 if is_table or float(val.norm()) > 1e-6 * gmax else 5e-2, key)
    assert tables == 3
    close(net.E.E.queue, g['queue_after'], 1e-4, 'queue')
    del net, params
    net, opt = make(st, 'bf16')
    net.eval()
    with torch.no_grad():
        out = net(x_query=q.to(DEV), x_key=q.to(DEV))
    assert abs(O.psnr(out.float().cpu(), clean) - float(g['psnr_eval'])) < 0.01


def test_debug_before_spectrum_excludes_the_table():
    """debug_mode: the "before" spectrum of a block is taken from norm1's output WITHOUT the table (decoder_Uformer.py:668-673 precede
    :687).  decoderlayer_3's first block is the first that holds a table, so nothing in front of its norm1 depends on any table: its
    "before" spectrum is the same with the tables at unit variance and zeroed (1e-6), its "after" spectrum is not."""
    _, q, _ = synth_batch(1, 128, 'modulator.')
    st = state()
    zeroed = {k: (torch.zeros_like(v) if k.endswith('.modulator.weight') else v) for k, v in st.items()}
    spectra = []
    for weights in (st, zeroed):
        net, _ = make(weights, 'fp32', debug_mode=True)
        net.eval()
        with torch.no_grad():
            out, visual = net(x_query=q.to(DEV), x_key=q.to(DEV))
        assert len(visual) == 10                        # one list per layer, in forward order: decoderlayer_3 is the seventh
        spectra.append(visual[6][0])
        del net
    (before, after, _), (before0, after0, _) = spectra
    close(before, before0, 1e-6, '"before" spectrum with and without the tables')
    moved = float((after - after0).abs().max() / after0.abs().max())
    assert moved > 1e-3, f'the "after" spectrum moved by {moved:.3e} only: is the table in the attention input at all?'


def test_graph_step_bf16_trains_the_tables():
    """One graph-captured TrainEngine step at 128x128, B = 1, bf16, replayed three times: finite losses, the first step equal to an
    eager engine's to 1e-4 of the loss; every table has moved (Adam reached it) and its gradient is a view of the flat gradient
    buffer that the engine's zeroing clears; state_dict -> new net -> load_state_dict reproduces the eval output bit for bit."""
    from fwair import engine as E
    from fwair import functional as Fn
    clean, q, k = (t.to(DEV) for t in synth_batch(1, 128, 'modulator.'))
    st = state()
    first = {}
    try:
        for graph in (True, False):
            Fn.config.direct_grads = False
            net, opt = make(st, 'bf16')
            net.train()
            eng = E.TrainEngine(net, lr=2e-4, contrast_loss_weight=0.6, use_graph=graph)
            losses = torch.stack([eng.step(q, k, clean).clone() for _ in range(3 if graph else 1)])
            torch.cuda.synchronize()
            assert bool(torch.isfinite(losses).all()), losses
            first[graph] = losses[0].cpu()
            if graph:
                tables = {n: p for n, p in net.named_parameters() if n.endswith('.modulator.weight')}
                assert len(tables) == 20
                lo, hi = eng.flat_g.data_ptr(), eng.flat_g.data_ptr() + eng.flat_g.numel() * 4
                for n, p in tables.items():
                    assert not torch.equal(p.detach().cpu(), st[n]), f'{n} never moved'
                    assert lo <= p.grad.data_ptr() < hi and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
                eng.flat_g.zero_()
                assert all(float(p.grad.abs().max()) == 0 for p in tables.values())
                net.eval()
                with torch.no_grad():
                    out = net(x_query=q, x_key=q)
                net2, _ = make(st, 'bf16')
                net2.load_state_dict(net.state_dict())
                net2.eval()
                with torch.no_grad():
                    out2 = net2(x_query=q, x_key=q)
                assert_bits(out2, out, 'eval output after the state_dict round trip')
                del net2, tables
            del eng, net
    finally:
        Fn.config.direct_grads = False
    print('modulator bf16 engine step (loss, l1, contrast): graph', first[True].tolist(), 'eager', first[False].tolist())
    close(first[True][:2], first[False][:2], 1e-4, 'first step, graph vs eager: loss, l1')
    assert abs(float(first[True][2]) - float(first[False][2])) < 1e-4 * float(first[False][0]), 'contrast, on the scale of the loss'
