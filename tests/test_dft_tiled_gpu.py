"""The tiled f32-MFMA 2-D DFT passes (csrc/fw_dft.hip: fw_dft2t_fwd / fw_dft2t_bands / fw_dft2t_decompose) for square maps whose
side is a multiple of 64 in [192, 512], and FrequencyDecompose on top of them.

Limit: 2e-5 relative to the reference's maximum, the bound of tests/test_ops_gpu.py::test_dft_band_decomposition.  The same f32
cos / sin matmul chain emulated on a CPU against the f64 FFT (seeded normal inputs, N = 192 / 256 / 384 / 512) is at most 6.9e-7
away in the spectrum and 9.2e-7 in the band images, so the limit leaves a 20x margin at every size used here.
Every output buffer is pre-filled with NaN: a tile no workgroup wrote fails `close`."""
import pytest
import torch

import airnet_oracle as O
from helpers import close, load, rnd as seeded
from fwair.lib import call

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KINDS = (('frequency_decompose_1', 0.5), ('frequency_decompose', 1 / 3.))
NIMG = 3
_cache = {}


def nan(*shape):
    return torch.full(shape, float('nan'), device=DEV)


def panels(N):
    from net.utils.frequency_decompose import _dft_panels
    return _dft_panels(N, torch.device(DEV))


def case(N):
    """-> x [5, N, N] (host), its f64 spectrum, and per kind: shifted masks, un-shifted device masks, f64 band images of x[:NIMG]"""
    if N not in _cache:
        from fwair import lfs
        g = torch.Generator().manual_seed(1000 + N)
        x = torch.randn(5, N, N, generator=g)
        kinds = {}
        for kind, size in KINDS:
            masks = torch.stack(lfs.band_masks_shifted(kind, size, N, N)).float()
            assert bool((masks.sum(0) == 1).all())                              # the masks partition the spectrum
            mu = torch.fft.ifftshift(masks, dim=(-2, -1)).contiguous()
            ref = O.frequency_decompose(x[:NIMG].double().view(1, NIMG, N, N), kind, size, N, N, True)[:, 0]
            kinds[kind] = (masks, mu.to(DEV), ref)
        _cache[N] = (x, torch.fft.fft2(x.double()), kinds)
    return _cache[N]


def spectrum(xd, N):
    n = xd.shape[0]
    fr, fi = nan(n, N, N), nan(n, N, N)
    call('fw_dft2t_fwd', xd, panels(N), nan(2 * n * N * N), fr, fi, n, N)
    return fr, fi


@pytest.mark.parametrize('nimg', [1, 3, 5])
@pytest.mark.parametrize('N', [192, 320, 384, 512])
def test_spectrum(N, nimg):
    x, F2, _ = case(N)
    fr, fi = spectrum(x[:nimg].to(DEV), N)
    close(fr, F2[:nimg].real, 2e-5, 'spectrum re')
    close(fi, F2[:nimg].imag, 2e-5, 'spectrum im')


@pytest.mark.parametrize('kind,size', KINDS)
@pytest.mark.parametrize('N', [192, 320, 384, 512])
def test_band_images(N, kind, size):
    x, _, kinds = case(N)
    masks, mu, ref = kinds[kind]
    nb, n = mu.shape[0], NIMG
    xd = x[:n].to(DEV)
    fr, fi = spectrum(xd, N)
    out = nan(nb, n, N, N)
    call('fw_dft2t_bands', fr, fi, mu, panels(N), nan(2 * nb * n * N * N), out, n, N, nb, 0)
    close(out, ref, 2e-5, f'{kind} real bands')
    close(out.sum(0), x[:n], 2e-5, f'{kind} bands sum to x')
    outp = nan(nb, n, N, N)
    call('fw_dft2t_bands', fr, fi, mu, panels(N), nan(2 * (nb - 1) * n * N * N), outp, n, N, nb - 1, 0)
    call('fw_band_residual', xd, outp, n, N, nb)
    close(outp, ref, 2e-5, f'{kind} real bands, last by subtraction')
    dc = sum(1 << b for b in range(nb) if float(masks[b].sum()) == 1.0 and float(mu[b, 0, 0]) == 1.0)
    assert dc == (1 if kind == 'frequency_decompose_1' else 0)
    for bits in (dc, 0):
        outm = nan(nb, n, N, N)
        call('fw_dft2t_decompose', xd, mu, panels(N), nan((2 + 2 * nb) * n * N * N), outm, n, N, nb, bits)
        close(outm, ref, 2e-5, f'{kind} whole decomposition (dc_bits {bits})')
        close(outm.sum(0), x[:n], 2e-5, f'{kind} whole decomposition sums to x (dc_bits {bits})')


@pytest.mark.parametrize('kind,size', KINDS)
@pytest.mark.parametrize('N', [192, 384])
def test_masked_spectra_and_magnitudes(N, kind, size):
    x, F2, kinds = case(N)
    masks, mu, _ = kinds[kind]
    nb, n = mu.shape[0], NIMG
    fr, fi = spectrum(x[:n].to(DEV), N)
    out1 = nan(nb, n, N, N, 2)
    call('fw_dft2t_bands', fr, fi, mu, None, None, out1, n, N, nb, 1)
    ref1 = O.frequency_decompose(x[:n].double().view(1, n, N, N), kind, size, N, N, False)[:, 0]
    close(out1, ref1, 2e-5, f'{kind} masked spectrum (re, im)')
    out2 = nan(nb, n, N, N)
    call('fw_dft2t_bands', fr, fi, mu, None, None, out2, n, N, nb, 2)
    ref2 = (torch.fft.fftshift(F2[:n], dim=(-2, -1)).unsqueeze(0) * masks.double().unsqueeze(1)).abs()
    close(out2, ref2, 2e-5, f'{kind} magnitudes, fftshift-ed')


def test_256_against_the_scalar_kernels():
    """N = 256 is accepted by both families: every output of the tiled entries against the existing kernels on the same input."""
    N, n = 256, NIMG
    x, _, kinds = case(N)
    xd = x[:n].to(DEV)
    fr0, fi0 = nan(n, N, N), nan(n, N, N)
    call('fw_dft2_fwd', xd, fr0, fi0, n, N)
    fr, fi = spectrum(xd, N)
    close(fr, fr0, 2e-5, 'spectrum re'); close(fi, fi0, 2e-5, 'spectrum im')
    for kind, size in KINDS:
        masks, mu, _ = kinds[kind]
        nb = mu.shape[0]
        for mode in (0, 1, 2):
            shape = (nb, n, N, N, 2) if mode == 1 else (nb, n, N, N)
            old, new = nan(*shape), nan(*shape)
            call('fw_dft2_bands', fr0, fi0, mu, old, n, N, nb, mode)
            call('fw_dft2t_bands', fr0, fi0, mu, panels(N), nan(2 * nb * n * N * N), new, n, N, nb, mode)
            close(new, old, 2e-5, f'{kind} mode {mode}')
        old = nan(nb, n, N, N)
        call('fw_dft2_bands', fr0, fi0, mu, old, n, N, nb - 1, 0)
        call('fw_band_residual', xd, old, n, N, nb)
        dc = 1 if kind == 'frequency_decompose_1' else 0
        new = nan(nb, n, N, N)
        call('fw_dft2t_decompose', xd, mu, panels(N), nan((2 + 2 * nb) * n * N * N), new, n, N, nb, dc)
        close(new, old, 2e-5, f'{kind} whole decomposition')


@pytest.mark.parametrize('fixture', ['unit_freq_decompose_384', 'unit_freq_decompose_384_spectra'])
def test_module_384_against_reference_golden(fixture):
    from net.utils.frequency_decompose import FrequencyDecompose
    g = load(fixture)
    n = 384
    x = seeded(f'fd{n}', (1, 2, n, n)).to(DEV)
    for tag, ref in g.items():
        kind, size, inv = tag.split('|')
        inv = {'True': True, 'False': False}.get(inv, inv)
        out = FrequencyDecompose(kind, float(size), n, n, inverse=inv)(x)
        close(out[:, :, :, ::4, ::4], ref, 2e-5, tag)


@pytest.mark.parametrize('inverse', [True, False])
@pytest.mark.parametrize('kind,size', [('frequency_decompose', 1 / 3.), ('frequency_decompose_1', 0.5)])
def test_frequency_decompose_backward_192(kind, size, inverse):
    """test_ops_gpu.py::test_frequency_decompose_backward at a side only the tiled passes take: forward and input gradient against
    torch autograd through the f64 oracle."""
    from net.utils.frequency_decompose import FrequencyDecompose
    N = 192
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, N, N, generator=g)
    xo = x.clone().double().requires_grad_(True)
    ref = O.frequency_decompose(xo, kind, size, N, N, inverse)
    wgt = torch.randn(*ref.shape, generator=g).double()
    (ref * wgt).sum().backward()
    xd = x.to(DEV).requires_grad_(True)
    out = FrequencyDecompose(kind, size, N, N, inverse=inverse)(xd)
    close(out, ref, 2e-5, 'forward')
    (out * wgt.to(DEV).float()).sum().backward()
    close(xd.grad, xo.grad, 5e-5, 'input gradient')


@pytest.mark.parametrize('N', [576, 200])
def test_other_sides_are_argument_errors(N):
    """the library's argument error (a negative source line), and nothing is launched: the outputs keep their NaN fill"""
    n, nb = 1, 2
    x = torch.zeros(n, N, N, device=DEV)
    mu = torch.ones(nb, N, N, device=DEV)
    pn = torch.zeros(3, N, N, device=DEV)
    fr, fi, out, work = nan(n, N, N), nan(n, N, N), nan(nb, n, N, N, 2), nan((2 + 2 * nb) * n * N * N)
    for name, args in (('fw_dft2t_fwd', (x, pn, work, fr, fi, n, N)),
                       ('fw_dft2t_bands', (x, x, mu, pn, work, out, n, N, nb, 0)),
                       ('fw_dft2t_bands', (x, x, mu, pn, work, out, n, N, nb, 1)),
                       ('fw_dft2t_decompose', (x, mu, pn, work, out, n, N, nb, 0))):
        with pytest.raises(RuntimeError, match='argument check'):
            call(name, *args)
    torch.cuda.synchronize()
    for t in (fr, fi, out, work):
        assert bool(torch.isnan(t).all())
