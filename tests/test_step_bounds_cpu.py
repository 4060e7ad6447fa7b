"""The derived bounds of tests/test_step_kernels_gpu.py, proven on the host: an f32 restatement of each kernel's expression stays
inside its bound, and the wrong kernels the bound exists to catch fall outside it.  No GPU, no library."""
import numpy as np
import pytest
import torch

from helpers import (ADAM_SPECIAL, U32, adam_case, adam_f32, adam_reference, ema_reference, l1_chain_length, l1_loss_bound,
                     outside_share)

B1, B2, EPS = 0.9, 0.999, 1e-8
MUTATIONS = ['eps_in_sqrt', 'bc2_no_sqrt', 'b2_for_m', 'lr_no_bc1']


def hyper_after(ticks, lr=1e-3):
    """hyper = {lr, b1^t, b2^t, t} as adam_tick_kernel advances it: f32 products"""
    h = np.array([lr, 1.0, 1.0, 0.0], dtype=np.float32)
    for _ in range(ticks):
        h[1] *= np.float32(B1); h[2] *= np.float32(B2); h[3] += np.float32(1)
    return h


def reference(p, g, m, v, h):
    d = lambda a: torch.from_numpy(a).double()
    return adam_reference(d(p), d(g), d(m), d(v), h, B1, B2, EPS)


@pytest.mark.parametrize('scale', [1e-6, 1.0])
@pytest.mark.parametrize('ticks', [1, 3, 1000])
def test_adam_f32_restatement_is_inside_the_bound(scale, ticks):
    p, g, m, v = adam_case(10007, seed=ticks, scale=scale)
    h = hyper_after(ticks)
    ref = reference(p, g, m, v, h)
    p1, m1, v1 = adam_f32(p, g, m, v, h, B1, B2, EPS)
    assert np.isfinite(p1).all() and np.isfinite(m1).all() and np.isfinite(v1).all()
    for name, y in (('m', m1), ('v', v1), ('p', p1)):
        assert outside_share(torch.from_numpy(y), ref[name], ref['tol_' + name]) == 0.0, name
    # the bound is a few roundings wide, not a tolerance: the final rounding of p plus 1e-5 of the update
    upd = (torch.from_numpy(p).double() - ref['p']).abs()
    assert bool((ref['tol_p'] <= 2 * U32 * ref['p'].abs() + 1e-5 * upd + 1e-30).all())


@pytest.mark.parametrize('mutation', MUTATIONS)
def test_adam_bound_rejects_the_wrong_kernels(mutation):
    n = 10007
    p, g, m, v = adam_case(n, seed=3, scale=1e-6)
    assert ADAM_SPECIAL / n < 0.01                              # the edge elements (g = 0, m = v = 0: no update to get wrong) are not counted on
    h = hyper_after(3)
    ref = reference(p, g, m, v, h)
    p1, _, _ = adam_f32(p, g, m, v, h, B1, B2, EPS, mutation=mutation)
    share = outside_share(torch.from_numpy(p1), ref['p'], ref['tol_p'])
    assert share >= 0.99, f'{mutation}: the bound rejects only {share:.4f} of the elements'


def test_adam_underflowing_gradient_gives_a_finite_tiny_update():
    p, g, m, v = adam_case(ADAM_SPECIAL, seed=5)
    h = hyper_after(1)
    ref = reference(p, g, m, v, h)
    tiny = np.abs(g) == np.float32(1e-20)
    assert tiny.sum() >= 4 and (np.float32(g[tiny]) * np.float32(g[tiny]) < np.float32(2.0 ** -126)).all()
    zero_state = tiny & (m == 0) & (v == 0)
    assert zero_state.any()
    upd = (torch.from_numpy(p).double() - ref['p']).abs()
    assert torch.isfinite(ref['p']).all() and float(upd[torch.from_numpy(zero_state)].max()) < 1e-12
    assert float(ref['tol_p'].max()) < 4 * U32                  # |p| < 1: the bound stays at the final rounding of p there


def test_ema_restatement_and_a_stale_or_swapped_momentum():
    gen = torch.Generator().manual_seed(11)
    pk = torch.randn(10007, generator=gen).numpy()
    pq = torch.randn(10007, generator=gen).numpy()
    mom = np.float32(0.999)
    x, tol = ema_reference(torch.from_numpy(pk).double(), torch.from_numpy(pq).double(), 0.999)
    y = pk * mom + pq * (np.float32(1) - mom)
    assert y.dtype == np.float32 and outside_share(torch.from_numpy(y), x, tol) == 0.0
    swapped = pq * mom + pk * (np.float32(1) - mom)
    assert outside_share(torch.from_numpy(swapped), x, tol) >= 0.99
    no_update = pk                                               # pk left as it was: off by (1 - mom) |pq - pk| ~ 1e-3
    assert outside_share(torch.from_numpy(no_update), x, tol) >= 0.99


def test_l1_chain_and_bound():
    n = 8192 * 256 + 257
    assert l1_chain_length(n) == 1 + 9 + 6 + 1 + 4096           # 262144 threads: 9 elements for the first 257 of them
    assert l1_chain_length(100) == 1 + 1 + 6 + 1 + 4
    gen = torch.Generator().manual_seed(12)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    loss, tol = l1_loss_bound(a.double(), b.double())
    # an f32 evaluation in the kernel's order: threads, then waves, then the running sum of the atomics
    threads = 1024 * 256
    d = (a - b).abs()
    d = torch.cat([d, torch.zeros(-n % threads)]).view(-1, threads)
    part = torch.zeros(threads)
    for row in d:
        part = part + row
    waves = part.view(-1, 64)
    for s in (32, 16, 8, 4, 2, 1):
        waves = waves[:, :s] + waves[:, s:2 * s]
    acc = np.float32(0)
    for w in (waves[:, 0] / np.float32(n)).numpy():
        acc = np.float32(acc + w)
    assert abs(float(acc) - loss) <= tol
    assert tol / loss < 3e-4                                     # one missing element of 2M is NOT what this bound sees; the exact case is
