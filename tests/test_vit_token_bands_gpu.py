"""GPU parity of `--vit_band_grid tokens` at N = 256 tokens (256x256 inputs): the ViT's band re-weighting with masks sized by the
attention map.  '<n>_bands' runs the multi-pass 256x256 DFT filter (csrc/fw_gattn.hip bands_*_kernel, fw_gattn_bands_fwd/bwd), 'DC'
the affine form (gattn_dc_*).  References: the f64 FFT statement of encoder_ViT.py:85-92 with N x N masks
(convnets_oracle.attn_band_masks(type, 256)) and the CPU oracle with the same masks.  Tolerances are those of
tests/test_vit256_gpu.py for the same quantities (rel-to-max, helpers.close)."""
import pytest
import torch

import airnet_oracle as O
import convnets_oracle as C
import dropout_hash as DH
from helpers import close, synth_batch
from test_vit256_gpu import oracle_step, seeded_vit, set_dtype

pytestmark = pytest.mark.gpu
DEV = 'cuda'
N = 256


def ref_attention(qkv, B, heads, drop=None, lamb=None, ftype=None):
    """encoder_ViT.py:76-96 in f64 on the CPU with N x N band masks: -> (out [B*N, heads*64], softmax map)."""
    x = qkv.double().reshape(B, N, 3, heads, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    attn = ((q @ k.transpose(-1, -2)) * 64 ** -0.5).softmax(-1)
    soft = attn
    if lamb is not None:
        masks = C.attn_band_masks(ftype, N).double()
        spec = torch.fft.fft2(attn)
        bands = torch.stack([torch.fft.ifft2(spec * m).real for m in masks], 0)
        attn = attn + (bands * lamb.double()[:, :, :, None, None]).sum(0)
    if drop is not None:
        seed, site, p = drop
        attn = attn * torch.from_numpy(DH.keep_mask(seed, site, tuple(attn.shape), p)).double() / (1.0 - p)
    return (attn @ v).transpose(1, 2).reshape(B * N, heads * 64), soft


def operands(dtype, tag, B, heads):
    g = torch.Generator().manual_seed(N + tag)
    qkv0 = (torch.randn(B * N, 3 * heads * 64, generator=g) * 0.8).to(dtype)
    dout0 = (torch.randn(B * N, heads * 64, generator=g) * 0.5).to(dtype)
    return g, qkv0, dout0


def tables(ftype):
    """What Transformer.run hands to the kernel: nothing for 'DC' (affine form), the 256x256 tables for <n>_bands."""
    from fwair import vit as V
    return None if ftype == 'DC' else V._spectral_tables('bands', int(ftype.split('_')[0]), torch.device(DEV), n=N)


def run_kernel(qkv0, dout0, lamb0, B, heads, p, site, ftype='DC'):
    from fwair import vit as V
    qk = qkv0.to(DEV).requires_grad_(True)
    lk = torch.nn.Parameter(lamb0.to(DEV)) if lamb0 is not None else None
    out = V.GlobalAttnFn.apply(qk, lk, (B, N, heads, p, site, tables(ftype) if lamb0 is not None else None))
    out.backward(dout0.to(DEV))
    return out, qk.grad, (lk.grad if lk is not None else None)


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('p,ftype,batchwise', [(0.0, '3_bands', False), (0.1, '3_bands', False), (0.0, '5_bands', False), (0.1, 'DC', False),
                                               (0.0, 'DC', True), (0.1, 'DC', True), (0.1, '3_bands', True)])
def test_kernel_vs_f64_fft_statement(dt, p, ftype, batchwise):
    from fwair import functional as Fn
    dtype = set_dtype(dt)
    B, heads, seed, site = 3, 2, 777, 41
    nb = 2 if ftype == 'DC' else int(ftype.split('_')[0])
    Fn.set_dropout_seed(seed, DEV, frozen=True)
    try:
        g, qkv0, dout0 = operands(dtype, int(p * 100) + 7 * batchwise + nb, B, heads)
        lamb0 = torch.randn(nb, B if batchwise else 1, heads, generator=g) * 0.5
        qr = qkv0.float().clone().requires_grad_(True)
        lr = lamb0.clone().requires_grad_(True)
        ref, _ = ref_attention(qr, B, heads, (seed, site, p) if p > 0 else None, lr, ftype)
        (ref * dout0.double()).sum().backward()
        out, dqkv, dlamb = run_kernel(qkv0, dout0, lamb0, B, heads, p, site, ftype)
        t1, t2, t3 = (2e-5, 1e-4, 2e-4) if dt == 'fp32' else (1.5e-2, 3e-2, 3e-2)
        err = lambda a, b: float((a.detach().double().cpu() - b.detach().double()).abs().max() / b.detach().double().abs().max())
        print(f'{ftype} p={p} {dt}: out {err(out, ref):.3e} dqkv {err(dqkv, qr.grad):.3e} dlamb {err(dlamb, lr.grad):.3e}')
        close(out.float(), ref, t1, 'out')
        close(dqkv.float(), qr.grad, t2, 'dqkv')
        close(dlamb, lr.grad, t3, 'dlamb')
    finally:
        Fn.set_dropout_seed(1, DEV, frozen=False)


@pytest.mark.parametrize('ftype', ['3_bands', 'DC'])
def test_invariants_without_an_fft_reference(ftype):
    """fp32, Dropout off: lamb = 0 is the plain N = 256 kernel; all bands equal to c scale the output by 1 + c (the bands sum to
    the map); 'DC' is the affine form (1 + lamb1) A + (lamb0 - lamb1) / N evaluated in f64."""
    dtype = set_dtype('fp32')
    B, heads = 3, 2
    nb = 2 if ftype == 'DC' else 3
    g, qkv0, dout0 = operands(dtype, 3, B, heads)
    base, dbase, _ = run_kernel(qkv0, dout0, None, B, heads, 0.0, 0)
    out, dqkv, _ = run_kernel(qkv0, dout0, torch.zeros(nb, 1, heads), B, heads, 0.0, 0, ftype)
    close(out, base, 2e-5, 'lamb = 0: out')
    close(dqkv, dbase, 1e-4, 'lamb = 0: dqkv')
    c = 0.375
    out, dqkv, _ = run_kernel(qkv0, dout0, torch.full((nb, 1, heads), c), B, heads, 0.0, 0, ftype)
    close(out, (1 + c) * base, 2e-5, 'equal bands: out')
    close(dqkv, (1 + c) * dbase, 1e-4, 'equal bands: dqkv')
    if ftype == 'DC':
        lamb0 = torch.randn(2, B, heads, generator=g) * 0.5
        _, soft = ref_attention(qkv0, B, heads)
        l0, l1 = (lamb0[i].double()[:, :, None, None] for i in range(2))
        v = qkv0.double().reshape(B, N, 3, heads, 64)[:, :, 2].transpose(1, 2)
        affine = (((1 + l1) * soft + (l0 - l1) / N) @ v).transpose(1, 2).reshape(B * N, heads * 64)
        out, _, _ = run_kernel(qkv0, dout0, lamb0, B, heads, 0.0, 0)
        close(out, affine, 2e-5, 'affine form')


@pytest.mark.parametrize('dt', ['fp32', 'bf16'])
@pytest.mark.parametrize('ftype,nb', [('3_bands', 3), ('DC', 2)])
def test_vit256_train_step_vs_oracle(dt, ftype, nb, monkeypatch):
    """ViT(256) + Uformer(256) with lamb on the N x N grid, one training step against the oracle (its masks re-sized to 256x256)."""
    from fwair import functional as Fn
    original = C.attn_band_masks
    monkeypatch.setattr(C, 'attn_band_masks', lambda t, n=64: original(t, N))
    seed = 4242
    net, opt, st = seeded_vit('vit256_uformer', dt, lamb_shape=(nb, 1, 12), patch_size=256, batch_size=1, frequency_decompose_type=ftype,
                              vit_band_grid='tokens')
    clean, q_, k_ = synth_batch(1, 256, 'vit256bands.')
    restored, logits, loss, names = oracle_step(st, opt, q_, k_, clean, seed)
    assert any(n.endswith('.fn.lamb') for n in names)
    net.train()
    Fn.set_dropout_seed(seed, DEV, frozen=True)
    try:
        r2, lg2, lb2 = net(x_query=q_.to(DEV), x_key=k_.to(DEV))
        loss2 = torch.nn.L1Loss()(r2, clean.to(DEV)) + 0.6 * torch.nn.CrossEntropyLoss()(lg2[0], lb2[0])
        loss2.backward()
    finally:
        Fn.set_dropout_seed(1, DEV, frozen=False)
    if dt == 'fp32':
        close(r2, restored, 1e-4, 'restored (train)')
        close(torch.stack(lg2), torch.stack(logits), 2e-4, 'logits')
        close(loss2, loss, 1e-4, 'loss')
    else:
        assert abs(O.psnr(r2.float().cpu(), clean) - O.psnr(restored.detach(), clean)) < 0.01
        close(loss2, loss, 2e-2, 'loss')
    params = dict(net.named_parameters())
    gn = torch.tensor([float(st[n].grad.norm()) for n in names], dtype=torch.float64)
    mine = torch.tensor([float(params[n].grad.norm()) for n in names], dtype=torch.float64)
    rel = (mine - gn).abs() / gn.clamp_min(float(gn.max()) * 1e-6)
    print(f'ViT(256) {ftype} tokens {dt}: grad-norm deviation max {rel.max():.2e} ({names[int(rel.argmax())]}) median {rel.median():.2e}')
    assert rel.median() < (1e-4 if dt == 'fp32' else 5e-2) and rel.max() < (5e-3 if dt == 'fp32' else 1.0)
    if dt == 'fp32':
        for i in (0, 11):
            n = f'E.E.encoder_q.transformer.layers.{i}.0.fn.lamb'
            print(n, close(params[n].grad, st[n].grad, 2e-3, n))


def test_engine_trains_lamb_at_256():
    """ViT(256) + 3_bands + tokens, bf16, whole-step graph: finite losses, every lamb of the query encoder moves, the key encoder's follows by EMA."""
    from fwair import engine as E
    from fwair import functional as Fn
    net, opt, st = seeded_vit('vit256_uformer', 'bf16', lamb_shape=(3, 1, 12), patch_size=256, batch_size=2, frequency_decompose_type='3_bands',
                              vit_band_grid='tokens')
    net.train()
    lq = [l[0].fn.lamb for l in net.E.E.encoder_q.transformer.layers]
    lk = [l[0].fn.lamb for l in net.E.E.encoder_k.transformer.layers]
    before = [p.detach().clone() for p in lq]
    eng = E.TrainEngine(net, lr=1e-4, contrast_loss_weight=0.6, use_graph=True)
    clean, q_, k_ = (t.to(DEV) for t in synth_batch(2, 256, 'vit256bandsgraph.'))
    losses = [eng.step(q_, k_, clean).clone() for _ in range(3)]
    torch.cuda.synchronize()
    Fn.config.direct_grads = False
    assert torch.isfinite(torch.stack(losses)).all()
    m = float(net.E.E.m)
    for i, (a, b, k) in enumerate(zip(before, lq, lk)):
        assert not torch.equal(a, b.detach()), f'layer {i}: lamb did not move'
        assert not torch.equal(a, k.detach()), f'layer {i}: the key encoder lamb did not follow'
        # k <- m k + (1 - m) q three times from k = q = a: |k - a| <= (1 - m^3) max_j |q_j - a|, and one Adam step moves an
        # element by at most lr (1 - beta1) / sqrt(1 - beta2) = 3.17 lr
        dk = (k.detach() - a).abs().max().item()
        assert dk <= (1 - m ** 3) * 3 * 3.17 * 1e-4 * 1.01, f'layer {i}: |dk| {dk:.3e}'


def test_head_dim_grid_at_256_still_raises():
    for ftype, nb in (('3_bands', 3), ('DC', 2)):
        net, opt, _ = seeded_vit('vit256_uformer', 'fp32', lamb_shape=(nb, 1, 12), patch_size=256, vit_band_grid='head_dim',
                                 frequency_decompose_type=ftype)
        net.eval()
        with pytest.raises(NotImplementedError), torch.no_grad():
            net.E.E.encoder_q(torch.zeros(1, 3, 256, 256, device=DEV))
