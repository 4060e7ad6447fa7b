"""The SSIM loss term on the device (--ssim_loss_weight): fw_ssim11_loss against the reference-run fixture
tests/golden/unit_ssim11.npz (utils/pytorch_ssim/__init__.py:19-43, f64), its store contract, the autograd wrapper, the term inside
TrainEngine's three step forms against the CPU oracle, and the driver's log field.

Tolerances of the kernel test.  U = 2^-24 (f32 unit roundoff), ulp = 2^-23.
  gradient: 8 x the deviation of the reference's own f32 run from its f64 run on that case (recorded in the fixture) -- the kernel's
            separable 11 + 11-term sums are ordered differently from conv2d's 121-term ones and the second convolution passes the error
            through once more -- with a floor of 4 ulp of max|grad|; all times |gscale|.
  value:    8 x the recorded deviation, with a floor from the kernel's summation: a thread adds at most 7 values of S, a wave folds in
            6 steps, the workgroup's 4 waves in 3, one division by N, i.e. 17 roundings each relative to a partial sum of a total <= 1,
            and G workgroups add their parts with one float atomic each, half an ulp of a sum < 1 per addition: (17 + G / 2) U."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import airnet_oracle as O
import ssim_cases as SC
from helpers import GUARD, SENTINEL, assert_bits, close, guarded, load, make_opt, schema, synth_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd')
NAMES = [c[0] for c in SC.CASES]


@pytest.fixture(scope='module')
def golden():
    return load('unit_ssim11')


def _case(name):
    _, shape, seed, kind = next(c for c in SC.CASES if c[0] == name)
    a, b = SC.inputs(shape, seed, kind)
    return shape, a.to(DEV), b.to(DEV)


def launch(a, b, gscale=1.0, accumulate=0, prefill=None, want_da=True, k=0):
    """-> (value [1] host, da host or None, guarded buffers intact).  k: extra offset of da (elements) behind its 16-byte aligned guard."""
    from fwair.lib import call
    n, C, H, W = a.shape
    lbuf, loss = guarded(1, torch.float32, DEV)
    loss.zero_()
    dbuf = da = None
    if want_da:
        dbuf, da = guarded(a.numel(), torch.float32, DEV, k)
        if prefill is not None:
            da.copy_(prefill.reshape(-1))
    call('fw_ssim11_loss', a, b, da, n, C, H, W, float(gscale), accumulate, loss)
    torch.cuda.synchronize()
    for buf, lead, inner in ((lbuf, GUARD, 1), (dbuf, GUARD + k, a.numel())):
        if buf is not None:
            h = buf.cpu()
            edge = torch.cat([h[:lead], h[lead + inner:]])
            assert_bits(edge, torch.full_like(edge, SENTINEL), 'guard words around ' + ('loss' if inner == 1 else 'da'))
    return loss.cpu().clone(), (da.cpu().clone().view(a.shape) if want_da else None)


def value_floor(shape):
    return (17 + SC.workgroups(shape) / 2) * U


@pytest.mark.parametrize('name', NAMES)
def test_kernel_matches_the_reference_fixture(golden, name):
    shape, a, b = _case(name)
    gscale = -0.5                                          # a power of two: the expected gradient scales exactly
    v, da = launch(a, b, gscale)
    want_v, want_g = float(golden[name + '.value']), golden[name + '.grad'] * gscale
    gmax = float(want_g.abs().max())
    tol_g = max(8 * float(golden[name + '.f32_grad_dev']) * abs(gscale), 4 * 2 * U * gmax)
    tol_v = max(8 * float(golden[name + '.f32_value_dev']), value_floor(shape))
    err = (da.double() - want_g).abs()
    worst = int(err.argmax())
    n_, c_, y_, x_ = (int(i) for i in np.unravel_index(worst, shape))
    H, W = shape[2:]
    ev, eg = abs(float(v.double()) - want_v), float(err.max())
    print(f'{name} {shape}: value err {ev:.2e} = {ev / max(float(golden[name + ".f32_value_dev"]), 1e-300):.2f} x reference f32 deviation '
          f'(tol {tol_v:.2e}); gradient err {eg:.2e} = {eg / (float(golden[name + ".f32_grad_dev"]) * abs(gscale)):.2f} x reference f32 deviation, '
          f'{eg / (2 * U * gmax):.2f} ulp of max|grad| (tol {tol_g:.2e}); worst element (n {n_}, c {c_}, y {y_}, x {x_}): '
          f'{min(y_, H - 1 - y_, x_, W - 1 - x_)} from the border, {min(y_ % SC.TILE, x_ % SC.TILE)} behind a tile line')
    assert torch.isfinite(da).all()
    assert ev <= tol_v, f'{name}: SSIM {float(v):.9f} vs {want_v:.9f}'
    assert eg <= tol_g, f'{name}: gradient off by {eg:.3e} > {tol_g:.3e}'


@pytest.mark.parametrize('name', ['seams_partial_tile', 'seams_both_odd'])        # 16-byte stores / element-wise stores
def test_store_contract(name):
    shape, a, b = _case(name)
    v, da = launch(a, b, 0.7)
    v2, da2 = launch(a, b, 0.7)
    assert_bits(da2, da, 'two calls')                                             # one writer per element, no atomics
    pre = torch.randn(shape, generator=torch.Generator().manual_seed(5)) * float(da.abs().max())
    _, acc = launch(a, b, 0.7, accumulate=1, prefill=pre.to(DEV))
    assert_bits(acc, pre + da, 'accumulate = prefilled + fresh')
    v3, _ = launch(a, b, 0.7, want_da=False)
    # the workgroups' parts are the same bits; the order of their atomic additions is not: half an ulp of a sum < 1 per addition and run
    assert abs(float(v3) - float(v)) <= SC.workgroups(shape) * U
    _, da4 = launch(a, b, 0.7, k=1)                                               # da 4 bytes off the 16-byte grid: element-wise stores
    assert_bits(da4, da, 'unaligned da')
    _, da5 = launch(a, b, 0.0)
    assert float(da5.abs().max()) == 0.0


def test_single_workgroup_value_is_reproducible():
    a, b = SC.inputs((1, 1, 24, 24), 3, 'noise')
    v, _ = launch(a.to(DEV), b.to(DEV))
    v2, _ = launch(a.to(DEV), b.to(DEV), want_da=False)
    assert_bits(v2, v, 'value with and without da')


def test_identical_images():
    """a == b: the maps of a and of b are the same bits, so A1 == B1 and A2 == B2 exactly (2 (m m) and m m + m m round alike), S == 1 in
    every pixel and a workgroup's part is count / N.  With 12 workgroups the value is within 4 ulp of 1: U for the parts' roundings (they
    sum to 1), and the additions' half ulps -- at most 2^-25 each while the sum is in [0.5, 1), 2^-26 in [0.25, 0.5), ... -- stay below 3 U.
    Gradient: all three G terms cancel, G_ab = -2 G_aa = 2 / B2 and G_mu = 0 in exact arithmetic.  What is left are roundings: G_mu's
    three quotients, four roundings each on magnitudes <= K = 2 max|a| (1 / min B1 + 1 / min B2): 12 U K; G_ab against -2 G_aa three
    roundings, their two 22-term convolutions 24 roundings each, on magnitudes <= 1 / min B2, times 2 a and b: 51 U K; the last sums: below
    64 U K |gscale| / N in all."""
    shape, _, b = _case('planes_nonsquare')
    assert SC.workgroups(shape) == 12
    gscale = -0.2
    v, da = launch(b, b, gscale)
    assert abs(float(v) - 1.0) <= 4 * 2 * U, float(v)
    b64 = b.double().cpu()
    ma, _, eaa, _, _ = SC.maps(b64, b64)
    B1, B2 = 2 * ma * ma + SC.C1, 2 * (eaa - ma * ma) + SC.C2
    K = 2 * float(b64.abs().max()) * (1 / float(B1.min()) + 1 / float(B2.min()))
    bound = 64 * U * K * abs(gscale) / b.numel()
    print(f'a == b: SSIM - 1 = {float(v) - 1.0:.2e}; max|da| {float(da.abs().max()):.2e}, bound {bound:.2e} (K = {K:.1f})')
    assert float(da.abs().max()) <= bound


def test_autograd_function_and_value_entry():
    from fwair.losses import SSIMLossFn, ssim11
    shape, a, b = _case('odd_unaligned')
    _, da = launch(a, b, -0.3)
    x = a.clone().requires_grad_(True)
    s = SSIMLossFn.apply(x, b, -0.3)
    g, = torch.autograd.grad(s.sum(), x)
    assert s.shape == (1,) and s.dtype == torch.float32
    assert_bits(g.cpu(), da, 'SSIMLossFn gradient = the kernel\'s da')
    x3 = a[0].clone().requires_grad_(True)                                        # [C, H, W]
    g3, = torch.autograd.grad(SSIMLossFn.apply(x3, b[0], 1.0).sum(), x3)
    assert g3.shape == x3.shape and bool(torch.isfinite(g3).all())
    # u8 images: divided by 255, then the f32 path
    gen = torch.Generator().manual_seed(9)
    u1 = torch.randint(0, 256, (3, 40, 56), generator=gen, dtype=torch.uint8)
    u2 = (u1.int() + torch.randint(-20, 21, u1.shape, generator=gen)).clamp(0, 255).to(torch.uint8)
    vu = ssim11(u1.to(DEV), u2.to(DEV))
    vf = ssim11(u1.to(DEV).float() / 255.0, u2.to(DEV).float() / 255.0)
    assert vu.dim() == 0 and vu.dtype == torch.float32
    assert abs(float(vu) - float(vf)) <= SC.workgroups((1,) + tuple(u1.shape)) * U     # same parts, the atomics' order only
    want = float(SC.ssim((u1.double() / 255.0)[None], (u2.double() / 255.0)[None]))
    assert abs(float(vu) - want) < 1e-5
    with pytest.raises(RuntimeError):
        ssim11(torch.zeros(1, 4, 4, device=DEV), torch.zeros(1, 4, 4, device=DEV))     # under 8 pixels: the entry's argument check


# ---------------------------------------------------------------------------------------------------------------
# the term inside the training step
# ---------------------------------------------------------------------------------------------------------------
WS = 0.2
PROBE = ('R.R.output_proj.proj.0.weight', 'R.R.encoderlayer_0.blocks.1.attn.qkv.to_q.weight',
         'E.E.encoder_q.uformer.conv.blocks.1.attn_inter.proj.weight')              # the three gradients smoke() probes


def _state():
    st = O.fill_state_seeded(schema('all3'))
    st['E.E.queue'] = st['E.E.queue'][:, :, :3].contiguous()                       # K = 3 * batch_size
    return st


def build_net():
    from net.model import AirNet
    from fwair import functional as Fn
    Fn.config.direct_grads = False
    opt = make_opt('all3', batch_size=1)
    net = AirNet(opt)
    st = _state()
    sd = net.state_dict()
    for k in sd:
        if st.get(k) is not None and sd[k].is_floating_point():
            sd[k] = st[k]
    net.load_state_dict(sd)
    Fn.set_droppath_override(lambda name, n, rate, device: None)
    return net.to(DEV).train()


def engine_step(**kw):
    """One step of a fresh engine on the shared batch -> (loss vector, eng.ssim, flat gradient, probed gradients), host copies."""
    from fwair import engine as E
    from fwair import functional as Fn
    net = build_net()
    try:
        eng = E.TrainEngine(net, lr=2e-4, contrast_loss_weight=0.6, **kw)
        clean, q, k = synth_batch(1, 128, 'ssim.')
        out = eng.step(q.to(DEV), k.to(DEV), clean.to(DEV))
        torch.cuda.synchronize()
        params = dict(net.named_parameters())
        return dict(out=out.detach().cpu().clone(), ssim=None if eng.ssim is None else eng.ssim.cpu().clone(), flat_g=eng.flat_g.cpu().clone(),
                    grads={n: params[n].grad.detach().cpu().clone() for n in PROBE}, split=eng._gsplit is not None)
    finally:
        Fn.config.direct_grads = False


@pytest.fixture(scope='module')
def oracle_step():
    """The CPU oracle's step on the same weights and batch with the objective training_loss + 0.2 (1 - SSIM): computed once."""
    st = _state()
    opt = make_opt('all3', batch_size=1)
    for n in PROBE:
        st[n] = st[n].clone().requires_grad_(True)
    clean, q, k = synth_batch(1, 128, 'ssim.')
    restored, logits, labels = O.airnet_forward(st, opt, q, k, True)
    loss, l1, contrast = O.training_loss(opt, restored, logits, labels, clean)
    s = SC.ssim(restored, clean)
    total = loss + WS * (1 - s)
    total.backward()
    return dict(total=total.detach(), l1=l1.detach(), contrast=contrast.detach(), ssim=s.detach(), grads={n: st[n].grad.clone() for n in PROBE})


_RUNS = {}


def engine_run(graph):
    if graph not in _RUNS:
        _RUNS[graph] = engine_step(use_graph=graph, ssim_loss_weight=WS)
    return _RUNS[graph]


@pytest.mark.parametrize('graph', [False, True])
def test_engine_step_with_the_term_matches_the_oracle(oracle_step, graph):
    r = engine_run(graph)
    assert r['out'].shape == (3,)
    e = close(r['out'][0], oracle_step['total'], 1e-4, 'total with the SSIM term')
    close(r['out'][1], oracle_step['l1'], 1e-4, 'l1 entry')
    assert abs(float(r['out'][2]) - float(oracle_step['contrast'])) < 1e-4 * float(oracle_step['total']), 'contrast entry'
    es = close(r['ssim'][0], oracle_step['ssim'], 1e-4, 'eng.ssim')
    worst = max(close(r['grads'][n], oracle_step['grads'][n], 2e-3, 'grad ' + n) for n in PROBE)
    assert float(oracle_step['ssim']) < 0.99                                       # the term is not idle on this batch
    print(f'engine(graph={graph}) with {WS} (1 - SSIM): total err {e:.2e}, SSIM {float(r["ssim"]):.6f} err {es:.2e}, worst probed gradient err {worst:.2e}')


def test_engine_two_stage_backward_with_the_term():
    """split_backward=True (the data-parallel replay scheme on one GPU) against the single-graph step: the tolerances of
    test_model_gpu.py::test_engine_two_stage_backward_matches_single_pass."""
    one = engine_run(True)
    two = engine_step(use_graph=True, ssim_loss_weight=WS, split_backward=True)
    assert two['split'] and not one['split']
    close(two['out'], one['out'], 1e-5, 'losses (total, l1, contrast)')
    close(two['ssim'], one['ssim'], 1e-5, 'eng.ssim')
    close(two['flat_g'], one['flat_g'], 2e-4, 'flat gradient')


class LaunchLog:
    """Stands in for the loaded library: every C-ABI call is noted as (entry, its non-pointer arguments) and passed on."""

    def __init__(self, real, protos):
        self._real, self._protos, self.calls = real, protos, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        sig = self._protos.get(name)
        if sig is None:
            return fn

        def noted(*args):
            self.calls.append((name,) + tuple(a for a, (_, isptr) in zip(args, sig) if not isptr))
            return fn(*args)
        return noted


def test_weight_zero_is_the_engine_without_the_argument(monkeypatch):
    """Weight 0 must be the engine as it was.  What is deterministic is compared exactly: the two engines make the same C-ABI calls with
    the same sizes and scalars in the same order (warm-up steps, capture and replay), none of them fw_ssim11_loss, and hold no SSIM buffer.
    The step's numbers cannot be compared bit for bit: measured on an MI355X, two engines built WITHOUT the argument on the same batch
    already differ from each other -- loss vector in the last bit of two entries (7.5e-9), flat_g in 11.6 to 11.7 million of its 273 million
    elements by at most 3.0e-8, eager and captured alike, since the step's kernels fold with float atomics (l1_loss_kernel's 48 workgroups
    among them) whose order is not fixed; weight 0.0 against no argument showed the same figures (11.6 million elements, 3.0e-8).  So the
    numbers are held to the tolerances the suite uses for one step computed twice in another launch order
    (test_model_gpu.py::test_engine_two_stage_backward_matches_single_pass)."""
    from fwair import engine as E
    from fwair import lib as L

    def no_launch(*a, **k):
        raise AssertionError('fw_ssim11_loss launched with weight 0')

    monkeypatch.setattr(E, 'ssim11_launch', no_launch)
    L.lib()
    real, logs = L._lib, {}
    for key, kw in (('zero', dict(ssim_loss_weight=0.0)), ('none', {})):
        logs[key] = LaunchLog(real, L._protos)
        monkeypatch.setattr(L, '_lib', logs[key])
        try:
            logs[key + '.run'] = engine_step(use_graph=True, **kw)         # warm-up steps, the capture and one replay
        finally:
            monkeypatch.setattr(L, '_lib', real)
    zero, none = logs['zero.run'], logs['none.run']
    # the same launches with the same sizes and scalars, in the same order: nothing new inside or outside the captured graphs
    assert len(logs['zero'].calls) > 100 and logs['zero'].calls == logs['none'].calls
    assert not any(c[0] == 'fw_ssim11_loss' for c in logs['zero'].calls)
    assert zero['ssim'] is None and none['ssim'] is None
    close(zero['out'], none['out'], 1e-5, 'loss vector')
    close(zero['flat_g'], none['flat_g'], 2e-4, 'flat gradient')


def run_driver(out, *extra):
    cmd = [sys.executable, os.path.join(PKG, 'train_ddp.py'), '--de_type', 'denoising_25', '--degradation_embedding_method', 'all_3_bands',
           '--contrast_loss_weight', '0.6', '--compute_dtype', 'bf16', '--per_gpu_batch', '1', '--synthetic_steps', '2', '--epochs', '1',
           '--epochs_encoder', '0', '--no_eval', '--output_path', out, *extra]
    r = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return open(out + 'train.log').read().splitlines()


def test_driver_logs_the_term(tmp_path):
    out = str(tmp_path) + '/'
    log = run_driver(out + 'a/', '--ssim_loss_weight', '0.2')
    m = re.fullmatch(r'Epoch \(0\)  Loss: l1_loss:(\d+\.\d{4}) contrast_loss:(\d+\.\d{4}) ssim_loss:(\d+\.\d{4})', log[0])
    assert m and 0 < float(m.group(3)) < 1, log[0]
    log = run_driver(out + 'b/')
    assert re.fullmatch(r'Epoch \(0\)  Loss: l1_loss:\d+\.\d{4} contrast_loss:\d+\.\d{4}', log[0]), log[0]
