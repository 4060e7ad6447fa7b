"""The headline model (Uformer encoder + Uformer decoder, all_3_bands, L = 3, frequency MSA) at 384x384 and 512x512 on the GPU,
against goldens produced by the REAL reference's classes with img_size=384 / 512 (tests/golden/make_golden_uformer_sizes.py).
The encoder's pre-processing there is a 384- / 512-point band decomposition on the tiled f32-MFMA passes (csrc/fw_dft.hip).
Limits: those of tests/test_model_gpu.py::test_256_resolution_fp32_and_bf16, on the sub-grid the goldens store."""
import pytest
import torch

import airnet_oracle as O
from helpers import close, load, make_opt, schema, synth_batch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_state = []


def state():
    """seeded weights, built once for the module and never modified (`make` copies them into a fresh net)"""
    if not _state:
        st = O.fill_state_seeded(schema('all3'))
        st['E.E.queue'] = torch.nn.functional.normalize(O.seeded_tensor('E.E.queue', (3, 256, 3)) / 0.02, dim=1)   # K = 3 * batch_size
        _state.append(st)
    return _state[0]


def make(st, size, dtype):
    from net.model import AirNet
    from fwair import functional as Fn
    opt = make_opt('all3', batch_size=1, patch_size=size, compute_dtype=dtype)
    net = AirNet(opt)
    sd = net.state_dict()
    for key in sd:
        if st.get(key) is not None and sd[key].is_floating_point():
            sd[key] = st[key]
    net.load_state_dict(sd)
    Fn.set_droppath_override(lambda name, n, rate, device: None)      # DropPath off (goldens were made that way)
    return net.to(DEV), opt


def test_384_resolution_fp32_and_bf16():
    g = load('model384_all3')
    clean, q, k = synth_batch(1, 384, 'model384.')
    st = state()
    net, opt = make(st, 384, 'fp32')
    assert net.E.E.encoder_q.preprocess_decompose.h == 384
    net.eval()
    with torch.no_grad():
        out = net(x_query=q.to(DEV), x_key=q.to(DEV))
    close(out[:, :, ::3, ::3], g['restored_eval'], 1e-4, 'restored_eval (384) vs reference golden')
    assert abs(O.psnr(out.cpu(), clean) - float(g['psnr_eval'])) < 0.01
    net.train()
    restored, logits, labels = net(x_query=q.to(DEV), x_key=k.to(DEV))
    close(restored[:, :, ::3, ::3], g['restored_train'], 1e-4, 'restored_train (384)')
    close(torch.stack(logits), g['logits'], 2e-4, 'logits (384)')
    CE = torch.nn.CrossEntropyLoss()
    contrast = sum(CE(logits[i], labels[i]) for i in range(opt.L)) / opt.L
    loss = torch.nn.L1Loss()(restored, clean.to(DEV)) + opt.contrast_loss_weight * contrast
    close(loss, g['loss'], 1e-4, 'loss (384)')
    loss.backward()
    names = [str(n) for n in g['grad_names']]
    params = dict(net.named_parameters())
    norms = torch.tensor([params[n].grad.norm().item() for n in names])
    # the gradient-norm rule of the 256 test, with its floor of 1e-5 x the largest norm (the lambda-head gradients hang off one
    # scalar per (block, band, head) that sums cancelling terms over every window)
    floor = float(g['grad_norms'].max()) * 1e-5
    rel = ((norms - g['grad_norms']).abs() / g['grad_norms'].clamp_min(floor))
    worst = int(rel.argmax())
    print(f'384 fp32: worst grad-norm deviation {float(rel.max()):.3e} at {names[worst]}')
    assert rel.max() < 5e-3, f'grad norm of {names[worst]}: {norms[worst]:.6e} vs {g["grad_norms"][worst]:.6e}'
    gmax = float(g['grad_norms'].max())
    for key, val in g.items():
        if key.startswith('g.'):
            close(params[key[2:]].grad, val, 5e-3 if float(val.norm()) > 1e-6 * gmax else 5e-2, key)
    close(net.E.E.queue, g['queue_after'], 1e-4, 'queue (384)')
    del net, params
    net, opt = make(st, 384, 'bf16')
    net.eval()
    with torch.no_grad():
        out = net(x_query=q.to(DEV), x_key=q.to(DEV))
    assert abs(O.psnr(out.float().cpu(), clean) - float(g['psnr_eval'])) < 0.01


def test_384_graph_step_bf16_matches_eager():
    """One graph-captured TrainEngine step at 384x384, B = 1, bf16, replayed three times: finite losses, and the first step equal
    to an eager engine's on the same batch and seeds.  tests/test_engine_parity_gpu.py holds a graph step and an eager step to the
    same reference at 1e-4 of the loss; the two are held to each other at that figure here."""
    from fwair import engine as E
    from fwair import functional as Fn
    clean, q, k = (t.to(DEV) for t in synth_batch(1, 384, 'model384.'))
    st = state()
    first = {}
    try:
        for graph in (True, False):
            Fn.config.direct_grads = False
            net, opt = make(st, 384, 'bf16')
            net.train()
            eng = E.TrainEngine(net, lr=2e-4, contrast_loss_weight=0.6, use_graph=graph)
            losses = torch.stack([eng.step(q, k, clean).clone() for _ in range(3 if graph else 1)])
            torch.cuda.synchronize()
            assert bool(torch.isfinite(losses).all()), losses
            first[graph] = losses[0].cpu()
            del eng, net
    finally:
        Fn.config.direct_grads = False
    print('384 bf16 engine step (loss, l1, contrast): graph', first[True].tolist(), 'eager', first[False].tolist())
    close(first[True][:2], first[False][:2], 1e-4, 'first step, graph vs eager: loss, l1')
    assert abs(float(first[True][2]) - float(first[False][2])) < 1e-4 * float(first[False][0]), 'contrast, on the scale of the loss'


def test_512_eval_fp32():
    g = load('model512_all3')
    clean, q, k = synth_batch(1, 512, 'model512.')
    net, opt = make(state(), 512, 'fp32')
    assert net.E.E.encoder_q.preprocess_decompose.h == 512
    net.eval()
    with torch.no_grad():
        out = net(x_query=q.to(DEV), x_key=q.to(DEV))
    close(out[:, :, ::4, ::4], g['restored_eval'], 1e-4, 'restored_eval (512) vs reference golden')
    assert abs(O.psnr(out.cpu(), clean) - float(g['psnr_eval'])) < 0.01
