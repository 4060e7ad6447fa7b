"""The model at the decoder widths --embed_dim 32 and 64 (head_dim of every decoder attention = embed_dim; csrc/fw_attn.hip
attn2_* <T, 32 / 64, lfs 2>) against goldens of the reference built at those widths (tests/golden/make_golden_widths.py), at the
limits of test_modulator_gpu.py::test_model_fp32_and_bf16_against_reference_golden; at width 32 a graph-captured engine step, the
checkpoint round trip through net.model.options_from_checkpoint, and the refusal of a width the kernels do not take."""
import types

import pytest
import torch

import airnet_oracle as O
from helpers import assert_bits, close, load, make_opt, synth_batch
from widths_cases import schema_width

pytestmark = pytest.mark.gpu
DEV = 'cuda'
_state = {}


def state(E):
    """seeded weights of the width, built once for the module and never modified"""
    if E not in _state:
        _state[E] = O.fill_state_seeded(schema_width(E))
    return _state[E]


def make(E, dtype, st=None, **kw):
    from net.model import AirNet
    from fwair import functional as Fn
    opt = make_opt('all3', batch_size=1, compute_dtype=dtype, embed_dim=E, **kw)
    net = AirNet(opt)
    st = state(E) if st is None else st
    sd = net.state_dict()
    for key in sd:
        if st.get(key) is not None and sd[key].is_floating_point():
            sd[key] = st[key]
    net.load_state_dict(sd)
    Fn.set_droppath_override(lambda name, n, rate, device: None)      # DropPath off (the golden was made that way)
    return net.to(DEV), opt


@pytest.mark.parametrize('E', [32, 64])
def test_model_fp32_and_bf16_against_reference_golden(E):
    g = load(f'model_all3_w{E}')
    clean, q, k = synth_batch(1, 128, f'w{E}.')
    net, opt = make(E, 'fp32')
    assert net.R.R.embed_dim == E and net.R.R.bottleneck_0.blocks[0].attn.dim == 16 * E
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
    params = dict(net.named_parameters())
    norms = torch.tensor([params[n].grad.norm().item() for n in names])
    floor = float(g['grad_norms'].max()) * 1e-5                        # the gradient-norm rule of the 256 / 384 tests
    rel = ((norms - g['grad_norms']).abs() / g['grad_norms'].clamp_min(floor))
    worst = int(rel.argmax())
    print(f'width {E} fp32: worst grad-norm deviation {float(rel.max()):.3e} at {names[worst]}')
    assert rel.max() < 5e-3, f'grad norm of {names[worst]}: {norms[worst]:.6e} vs {g["grad_norms"][worst]:.6e}'
    gmax = float(g['grad_norms'].max())
    stored = 0
    for key, val in g.items():
        if key.startswith('g.'):
            stored += 1
            close(params[key[2:]].grad, val, 5e-3 if float(val.norm()) > 1e-6 * gmax else 5e-2, key)
    assert stored == 4
    close(net.E.E.queue, g['queue_after'], 1e-4, 'queue')
    del net, params
    net, opt = make(E, 'bf16')
    net.eval()
    with torch.no_grad():
        out = net(x_query=q.to(DEV), x_key=q.to(DEV))
    psnr = O.psnr(out.float().cpu(), clean)
    print(f'width {E} bf16: eval PSNR {psnr:.4f} dB, reference {float(g["psnr_eval"]):.4f} dB')
    assert abs(psnr - float(g['psnr_eval'])) < 0.01


def test_graph_step_bf16_and_checkpoint_round_trip_at_32():
    """One graph-captured TrainEngine step at width 32, 128x128, B = 1, bf16, replayed three times: finite losses, the first step
    equal to an eager engine's to 1e-4 of the loss.  Then state_dict -> options_from_checkpoint on options that say 56 -> a new net of
    width 32 -> load_state_dict reproduces the eval output bit for bit."""
    from fwair import engine as Eng
    from fwair import functional as Fn
    from net.model import AirNet, options_from_checkpoint
    clean, q, k = (t.to(DEV) for t in synth_batch(1, 128, 'w32.'))
    first = {}
    try:
        for graph in (True, False):
            Fn.config.direct_grads = False
            net, opt = make(32, 'bf16')
            net.train()
            eng = Eng.TrainEngine(net, lr=2e-4, contrast_loss_weight=0.6, use_graph=graph)
            losses = torch.stack([eng.step(q, k, clean).clone() for _ in range(3 if graph else 1)])
            torch.cuda.synchronize()
            assert bool(torch.isfinite(losses).all()), losses
            first[graph] = losses[0].cpu()
            if graph:
                net.eval()
                with torch.no_grad():
                    out = net(x_query=q, x_key=q)
                sd = {n: v.detach().clone() for n, v in net.state_dict().items()}
                opt2 = options_from_checkpoint(make_opt('all3', batch_size=5, compute_dtype='bf16'), sd)
                assert opt2.embed_dim == 32 and opt2.batch_size == 1 and opt2.learnable_modulator is False
                net2 = AirNet(opt2)
                assert net2.R.R.embed_dim == 32
                net2.load_state_dict(sd)
                net2 = net2.to(DEV).eval()
                with torch.no_grad():
                    out2 = net2(x_query=q, x_key=q)
                assert_bits(out2, out, 'eval output after the state_dict round trip')
                del net2
            del eng, net
    finally:
        Fn.config.direct_grads = False
    print('width 32 bf16 engine step (loss, l1, contrast): graph', first[True].tolist(), 'eager', first[False].tolist())
    close(first[True][:2], first[False][:2], 1e-4, 'first step, graph vs eager: loss, l1')
    assert abs(float(first[True][2]) - float(first[False][2])) < 1e-4 * float(first[False][0]), 'contrast, on the scale of the loss'


def test_unsupported_width_is_refused_at_construction():
    from net.model import AirNet
    with pytest.raises(NotImplementedError, match='32, 56, 64'):
        AirNet(make_opt('all3', batch_size=1, embed_dim=48))
