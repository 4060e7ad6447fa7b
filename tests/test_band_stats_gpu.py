"""fw_band_stats (csrc/fw_spec.hip) and what stands on it: fwair/spectrum.py and restore.py --band_report.

Limit.  Every comparison is PER BAND and relative to that band's own reference value (an empty band must be exactly 0), never to the
largest band.  The limit is not guessed: band_stats_cases.emulate_f32 runs the kernel's chain on the host for these tests' own inputs
-- f32 panels, f32 products accumulated four terms at a time in order as the MFMA chain does, f32 magnitudes, one f32 partial per 64 x 64
tile and band, the fold in double -- and `limit(group)` is 20 times its largest per-band deviation from the f64 FFT within the group,
the margin tests/test_dft_tiled_gpu.py gives its own emulation.  The groups: 'golden' (the ten fixture cases, three images each) and
each large size with both ring kinds and both powers.  Measured: golden 9.6e-8 .. 4.7e-7 (worst: 50 x 36 with ten rings), (320, 480)
5.7e-7, (321, 481) 4.4e-7, (1024, 8) 1.8e-5 -- so the limits are 9.3e-6, 1.1e-5, 8.7e-6 and 3.5e-4; the kernel itself was at most 6.4e-7 at
(320, 480), 6.0e-7 at (321, 481) and 8.2e-6 at (1024, 8).  The inputs have a mean of 128 grey levels, as the fixture asks (no ring sum near
zero); the bins next to DC are then what is left of a sum of H W terms of that size, and at 1024 x 8 the 'plot' rings (half the width =
4 bins) consist of little else, hence that size's figure.  The figures are recomputed where the tests run (the host's arithmetic
decides their last digit); a floor of 20 * 2^-24 keeps the limit from ever asking for more than f32 can give.

Every buffer handed to the library -- maps, ring, panels, work, out -- is a slice of a larger allocation with sentinel zones on both
sides that must come back untouched; work and out are pre-filled with NaN, and out must come back finite."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import airnet_oracle as O
import band_stats_cases as BC
from helpers import load, make_opt, schema
from fwair.lib import call

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd')
ZONE = 64                                     # sentinel elements on either side (a multiple of 16 bytes for every type used)
BIG = [(320, 480), (321, 481), (1024, 8)]
BIG_N, BIG_NB = 2, 5
_cache = {}


def sentinel(dtype):
    return 0x5A if dtype == torch.uint8 else 7.0


class Guarded:
    """values (host tensor) inside a larger device allocation: ZONE + shift sentinel elements before, ZONE after"""

    def __init__(self, values, shift=0):
        v = values.contiguous().reshape(-1)
        self.buf = torch.full((ZONE + shift + v.numel() + ZONE,), sentinel(v.dtype), dtype=v.dtype, device=DEV)
        self.lo = ZONE + shift
        self.view = self.buf[self.lo:self.lo + v.numel()]
        self.view.copy_(v)
        self.shape = values.shape

    def check(self, what):
        s = torch.full((1,), sentinel(self.buf.dtype), dtype=self.buf.dtype, device=DEV)
        assert bool((self.buf[:self.lo] == s).all()) and bool((self.buf[self.lo + self.view.numel():] == s).all()), f'{what}: a sentinel zone was written'


def run_stats(kind, src, clean, ring_shifted, nb, power, shift=0):
    """src / clean: host tensors [n, h, w]; every buffer guarded, work and out NaN.  -> out [n, nb] (host, f64), all checks done"""
    from fwair import spectrum as S
    n, h, w = src.shape
    ring = torch.from_numpy(np.ascontiguousarray(np.fft.ifftshift(ring_shifted)))
    g = dict(src=Guarded(src, shift), ring=Guarded(ring, shift), ph=Guarded(torch.from_numpy(S.panels_host(h))),
             pw=Guarded(torch.from_numpy(S.panels_host(w))),
             work=Guarded(torch.full((S.work_floats(n, h, w, nb),), float('nan'))),
             out=Guarded(torch.full((n * nb,), float('nan'), dtype=torch.float64)))
    if clean is not None:
        g['clean'] = Guarded(clean, shift)
    keep = {k: v.view.clone() for k, v in g.items() if k not in ('work', 'out')}
    call('fw_band_stats', kind, g['src'].view, g['clean'].view if clean is not None else None, g['ring'].view, g['ph'].view, g['pw'].view,
         g['work'].view, g['out'].view, n, h, w, nb, power)
    torch.cuda.synchronize()
    for k, v in g.items():
        v.check(k)
    for k, v in keep.items():
        assert torch.equal(g[k].view, v), f'{k}: an input was changed'
    out = g['out'].view.cpu().view(n, nb)
    assert bool(torch.isfinite(out).all()), 'out is not finite'
    return out.numpy()


def big_case(h, w):
    """-> x f64 numpy [BIG_N][h][w], {ring kind: shifted ring}, {(ring kind, power): f64 reference}"""
    from fwair import spectrum as S
    if (h, w) not in _cache:
        x = BC.images(h, w, BIG_N, 'big')
        rings = {k: S.ring_index(k, 1.0 / BIG_NB, h, w) for k in ('plot', 'bands')}
        _cache[(h, w)] = (x, rings, {(k, p): BC.band_sums(x, rings[k], BIG_NB, p) for k in rings for p in (0, 1)})
    return _cache[(h, w)]


def limit(group):
    """20 x the largest per-band relative deviation of the f32 emulation from f64 over the inputs of `group`: 'golden', or (h, w) of BIG
    (module docstring)"""
    from fwair import spectrum as S
    if ('limit', group) not in _cache:
        worst = {}
        if group == 'golden':
            for h, w, size in BC.CASES:
                ring, nb = S.ring_index('plot', size, h, w), int(1 / size)
                x = BC.images(h, w)
                worst[(h, w)] = BC.rel_err(BC.emulate_f32(x, ring, nb, 0), BC.band_sums(x, ring, nb, 0))
        else:
            x, rings, ref = big_case(*group)
            worst = {kp: BC.rel_err(BC.emulate_f32(x, rings[kp[0]], BIG_NB, kp[1]), ref[kp]) for kp in ref}
        _cache[('limit', group)] = 20 * max(max(worst.values()), 2.0 ** -24)
        print(f'f32 emulation against f64, largest per-band relative deviation ({group}):', {k: f'{v:.2e}' for k, v in worst.items()},
              f'-> limit {_cache[("limit", group)]:.3e}')
    return _cache[('limit', group)]


@pytest.mark.parametrize('src_kind', [0, 1])
@pytest.mark.parametrize('nimg', [1, 3])
@pytest.mark.parametrize('h,w,size', BC.CASES)
def test_against_the_reference_golden(h, w, size, nimg, src_kind):
    """the reference's own get_frequency_distribution (norm=False and, divided here, norm=True); f32 maps start 4 bytes and u8 maps and
    the ring 1 byte off a 16-byte boundary, so that W % 4 == 0 also meets the element-wise loader"""
    from fwair import spectrum as S
    g = load('unit_band_stats')
    nb = int(1 / size)
    x = torch.from_numpy(BC.images(h, w)[:nimg])
    src = x.float() if src_kind == 0 else x.to(torch.uint8)
    assert torch.equal(src.double(), x)
    ring = S.ring_index('plot', size, h, w)
    ref = g[BC.key(h, w, size, False)].numpy()[:nimg]
    lim = limit('golden')
    for shift in (0, 1):
        out = run_stats(src_kind, src, None, ring, nb, 0, shift)
        err = BC.rel_err(out, ref)
        errn = BC.rel_err(out / out.sum(1, keepdims=True), g[BC.key(h, w, size, True)].numpy()[:nimg])
        print(f'{h}x{w} size {size:.3f} nimg {nimg} kind {src_kind} shift {shift}: raw {err:.2e} norm {errn:.2e} (limit {lim:.2e})')
        assert err <= lim and errn <= 2 * lim


@pytest.mark.parametrize('power', [0, 1])
@pytest.mark.parametrize('rings', ['plot', 'bands'])
@pytest.mark.parametrize('h,w', BIG)
def test_against_f64_fft(h, w, rings, power):
    x, ring, ref = big_case(h, w)
    out = run_stats(0, torch.from_numpy(x).float(), None, ring[rings], BIG_NB, power)
    err = BC.rel_err(out, ref[(rings, power)])
    print(f'{h}x{w} {rings} power {power}: {err:.2e} (limit {limit((h, w)):.2e})')
    assert err <= limit((h, w))


@pytest.mark.parametrize('h,w', [(33, 47), (40, 24), (65, 130)])
def test_a_ring_without_symmetry(h, w):
    """The kernel computes the columns v <= W / 2 and credits each bin's value to its mirror bin's band too: a random table (no
    radial or point symmetry; 255 and a value >= nbands both mean `no band`) shows a mirror looked up at the wrong place.  Odd W,
    even W (the column 2 v = W is its own mirror) and two tiles per axis."""
    nb = 4
    g = torch.Generator().manual_seed(h * 7 + w)
    ring = torch.randint(0, 6, (h, w), generator=g).to(torch.uint8)
    ring[ring == 4] = 255
    ring[ring == 5] = 40
    ring = ring.numpy()                                              # taken as fftshift-ed, like every table here
    x = BC.images(h, w, 2, 'asym')
    for power in (0, 1):
        out = run_stats(0, torch.from_numpy(x).float(), None, ring, nb, power)
        err = BC.rel_err(out, BC.band_sums(x, ring, nb, power))
        print(f'{h}x{w} random ring power {power}: {err:.2e} (limit {limit("golden"):.2e})')
        assert err <= limit('golden')


def error_maps(h, w, n, tag):
    """restored f32 in [-0.1, 1.1] (the clamp bites), clean u8 -> host tensors [n, h, w] and the f64 error map"""
    g = torch.Generator().manual_seed(h * 1031 + w)
    r = (torch.rand(n, h, w, generator=g) * 1.2 - 0.1).float()
    c = torch.randint(0, 256, (n, h, w), generator=g).to(torch.uint8)
    return r, c, (r.double().clamp(0, 1) - c.double() / 255.0).numpy()


@pytest.mark.parametrize('h,w', [(33, 47), (321, 481)])
def test_parseval(h, w):
    """kind 'bands', power 1: sum_b out / (H W) = sum x^2 in double -- for a plain f32 map and for the error map of source kind 2"""
    from fwair import spectrum as S
    nb = 3
    lim = limit((h, w) if (h, w) in BIG else 'golden')
    ring = S.ring_index('bands', 1.0 / nb, h, w)
    x = BC.images(h, w, 2, 'parseval')
    out = run_stats(0, torch.from_numpy(x).float(), None, ring, nb, 1)
    r, c, e = error_maps(h, w, 2, 'parseval')
    out2 = run_stats(2, r, c, ring, nb, 1)
    for o, m, what in ((out, x, 'f32 map'), (out2, e, 'error map')):
        got, want = o.sum(1) / (h * w), (m * m).sum((1, 2))
        err = float((np.abs(got - want) / want).max())
        print(f'{h}x{w} {what}: Parseval {err:.2e} (limit {lim:.2e})')
        assert err <= lim
    assert BC.rel_err(out2, BC.band_sums(e, ring, nb, 1)) <= lim


def test_bit_reproducible():
    from fwair import spectrum as S
    h, w, nb = 100, 130, 5
    x = torch.from_numpy(BC.images(h, w, 3, 'repro')).float().to(DEV)
    ring, _ = S.ring_table('plot', 0.2, h, w, DEV)
    for power in (0, 1):
        a, b = S.band_stats(x, ring, nb, power), S.band_stats(x, ring, nb, power)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize('bad', ['H7', 'W1025', 'nbands33', 'null'])
def test_argument_errors(bad):
    """the library's argument error (a negative source line), and nothing is launched: work and out keep their NaN fill"""
    from fwair import spectrum as S
    h, w, nb, n = {'H7': (7, 16), 'W1025': (16, 1025)}.get(bad, (16, 16)) + ((33 if bad == 'nbands33' else 2), 1)
    x = torch.zeros(n, h, w, device=DEV)
    ring = torch.zeros(h, w, dtype=torch.uint8, device=DEV)
    ph, pw = torch.zeros(3, S.padded(h), S.padded(h), device=DEV), torch.zeros(3, S.padded(w), S.padded(w), device=DEV)
    work = torch.full((S.work_floats(n, h, w, nb),), float('nan'), device=DEV)
    out = torch.full((n, nb), float('nan'), dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match='argument check'):
        call('fw_band_stats', 0, x, None, None if bad == 'null' else ring, ph, pw, work, out, n, h, w, nb, 0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(work).all()) and bool(torch.isnan(out).all())


def test_distribution_and_report_on_mixed_sizes():
    """frequency_distribution on a batch and on a single map, band_report on a list of sizes (24, 40), (40, 24), (24, 40): each against
    the per-image f64 computation; images of equal size share a launch and still land in their own rows"""
    from fwair import spectrum as S
    sizes, nb = [(24, 40), (40, 24), (24, 40)], 4
    x = BC.images(24, 40, 3, 'dist')
    ring = S.ring_index('plot', 0.2, 24, 40)
    ref = BC.band_sums(x, ring, 5, 0)
    xd = torch.from_numpy(x).float().to(DEV)
    d = S.frequency_distribution(xd, size=0.2, norm=False)
    assert d.shape == (3, 5) and d.dtype == torch.float64 and d.is_cuda
    assert BC.rel_err(d.cpu().numpy(), ref) <= limit('golden')
    dn = S.frequency_distribution(xd[1].to(torch.uint8), size=0.2)
    assert dn.shape == (1, 5) and BC.rel_err(dn.cpu().numpy(), (ref / ref.sum(1, keepdims=True))[1:2]) <= 2 * limit('golden')
    gray = S.rgb2gray(torch.from_numpy(x).permute(1, 2, 0).to(DEV))
    assert gray.shape == (24, 40) and BC.rel_err(gray.cpu().numpy(), np.clip(0.2989 * x[0] + 0.5870 * x[1] + 0.1140 * x[2], 0, 255)) < 1e-6
    clean, rest, want = [], [], []
    for i, (h, w) in enumerate(sizes):
        r, c, e = error_maps(h + i, w, 3, 'report')
        r, c, e = r[:, :h], c[:, :h], e[:, :h]
        rest.append(r.contiguous().to(DEV)); clean.append(c.contiguous().to(DEV))
        want.append(BC.band_sums(e, S.ring_index('bands', 1.0 / nb, h, w), nb, 1).sum(0) / (h * w))
    E = S.band_report(clean, rest, nb)
    assert E.shape == (3, nb) and E.dtype == torch.float64
    assert BC.rel_err(E.cpu().numpy(), np.stack(want)) <= limit('golden')
    assert not np.allclose(want[0], want[2], rtol=1e-3), 'the two images of one size differ, so a swapped row would show'


# ---- end to end: restore.py --band_report on a small folder tree (the images of tests/test_folder_train_gpu.py, one per set)
def _image(rs, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.stack([127 + 90 * np.sin(xx / (7 + c) + yy / (11 + 2 * c)) + rs.randn(h, w) * 12 for c in range(3)], -1)
    return np.clip(img, 0, 255).astype(np.uint8)


def _save(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _run(script, *args):
    env = dict(os.environ, PYTHONPATH=PKG)
    r = subprocess.run([sys.executable, os.path.join(PKG, script), *args], cwd=PKG, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_restore_band_report_end_to_end(tmp_path):
    from net.model import AirNet
    rs = np.random.RandomState(5)
    root = str(tmp_path / 'data')
    _save(f'{root}/denoising_bsd68_test/GT/test0.png', _image(rs, 144, 160))
    g = _image(rs, 128, 150)
    _save(f'{root}/deraining_test/GT/rain-0.png', g)
    rain = g.astype(np.float32)
    rain[rs.rand(*g.shape[:2]) < 0.03] += 120
    _save(f'{root}/deraining_test/Input/rain-0_x.png', np.clip(rain, 0, 255).astype(np.uint8))
    net = AirNet(make_opt('all3'))
    st = O.fill_state_seeded(schema('all3'))
    sd = net.state_dict()
    for k in sd:
        if st.get(k) is not None and sd[k].is_floating_point():
            sd[k] = st[k]
    tasks = ('denoising_bsd68_25', 'deraining')
    outs = {}
    for flag in (True, False):
        out = str(tmp_path / ('with' if flag else 'without')) + '/'
        os.makedirs(out + 'ckpt')
        torch.save(sd, out + 'ckpt/epoch_1.pth')
        _run('restore.py', '--data_root', root, '--epochs', '1', '--degradation_embedding_method', 'all_3_bands', '--test_de_type', *tasks,
             '--output_path', out, '--no_graph', *(['--band_report', '3'] if flag else []))
        outs[flag] = out
    res = open(outs[True] + 'epoch_1_results.log', 'rb').read()
    assert res == open(outs[False] + 'epoch_1_results.log', 'rb').read(), 'the results log depends on --band_report'
    assert not os.path.exists(outs[False] + 'epoch_1_bands.log')
    lines = open(outs[True] + 'epoch_1_bands.log').read().splitlines()
    print('\n'.join(lines))
    assert len(lines) == len(tasks) * 3 + len(tasks)
    for t, (task, rline) in enumerate(zip(tasks, res.decode().splitlines())):
        psnr = re.fullmatch(re.escape(task) + r': +PSNR/SSIM: (-?\d+\.\d{2})/(-?\d\.\d{4})', rline).group(1)
        shares = []
        for b in range(3):
            m = re.fullmatch(re.escape(task) + r': +band %d \[(\d\.\d{4}), (\d\.\d{4})[)\]] error share: (\d\.\d{4}) PSNR: (-?\d+\.\d{2})' % b, lines[4 * t + b])
            assert m, lines[4 * t + b]
            assert abs(float(m.group(1)) - b / 3) < 1e-4 and abs(float(m.group(2)) - (b + 1) / 3) < 1e-4
            shares.append(float(m.group(3)))
            assert float(m.group(4)) >= float(psnr)                      # a band holds at most the whole error
        assert abs(sum(shares) - 1) < 2e-4
        m = re.fullmatch(re.escape(task) + r': +all 3 bands PSNR: (-?\d+\.\d{2})', lines[4 * t + 3])
        assert m and m.group(1) == psnr, (lines[4 * t + 3], rline)
    # no ground truth: the ring distribution of every input and its restoration
    dst = str(tmp_path / 'restored')
    _run('restore.py', '--ckpt', outs[True] + 'ckpt/epoch_1.pth', '--input', root + '/deraining_test/Input', '--output', dst,
         '--degradation_embedding_method', 'all_3_bands', '--no_graph', '--band_report', '4')
    blines = open(dst + '/bands.log').read().splitlines()
    assert len(blines) == 2 and blines[0].startswith('rain-0_x.png input: ') and blines[1].startswith('rain-0_x.png restored: ')
    for ln in blines:
        v = [float(s) for s in ln.split(': ')[1].split()]
        assert len(v) == 4 and abs(sum(v) - 1) < 1e-5 and min(v) > 0
