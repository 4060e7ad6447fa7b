"""The small kernels every training step ends in (csrc/fw_elem.hip): slab folds, Adam / EMA with their shadows, casts, copies,
permutes, LeakyReLU, fill and the two losses, each against a plain f64 (or bit-exact) host statement of the same operation.

Conventions: every output lives in a buffer larger than what the kernel may write, SENTINEL (7.0) before and after, compared bit for
bit afterwards; every operand pad the kernel must not consume holds NaN; data movers and single roundings are bit-exact, arithmetic
is bounded per element by the operation counts in tests/helpers.py (proven on the host in tests/test_step_bounds_cpu.py)."""
import numpy as np
import pytest
import torch

from helpers import (ADAM_SPECIAL, GUARD, SENTINEL, U32, adam_case, adam_reference, assert_bits, assert_bound_1d, assert_guarded,
                     close, ema_reference, guarded, guarded_like, l1_loss_bound)

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
B1, B2, EPS = 0.9, 0.999, 1e-8
CAP = 8192 * 256                     # threads of the largest grid of the grid-stride kernels: n above it takes a second pass
BF, F32 = torch.bfloat16, torch.float32


def call(*a):
    from fwair.lib import call as _c
    return _c(*a)


def OPS():
    from fwair import ops
    return ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


def sixteenths(*shape, seed):
    """small integers times 2^-4: sums of a few hundred of them are exact in f32, in any order"""
    return torch.randint(-8, 9, shape, generator=gen(seed)).float() / 16


def rup(x, m):
    return (x + m - 1) // m * m


# ================================================================================================ 1. slab folds
NZS = [1, 7, 8, 9, 13, 64, 65, 130]
NS = [4, 250, 252, 256, 260, 1028]


class Slab:
    """One fold: slab [nz][zstride] of sixteenths with NaN in every column outside [0, n) and [off2, off2 + n2); guarded
    destinations pre-filled with sixteenths; want = the f64 sum, which f32 holds exactly."""

    def __init__(self, nz, n, seed, off2=None, n2=0, pad=0, k=0, k2=0):
        self.nz, self.n, self.off2, self.n2, self.k, self.k2 = nz, n, off2, n2, k, k2
        self.end = n if off2 is None else off2 + n2
        assert off2 is None or (off2 >= n and n2 > 0)
        self.zstride = rup(self.end, 4) + pad
        vals = sixteenths(nz, self.zstride, seed=seed)
        host = torch.full((nz, self.zstride), NAN)
        host[:, :n] = vals[:, :n]
        if off2 is not None:
            host[:, off2:off2 + n2] = vals[:, off2:off2 + n2]
        self.slab = host.to(DEV)
        assert self.slab.data_ptr() % 16 == 0 and self.zstride % 4 == 0 and self.slab.numel() == nz * self.zstride
        self.sum = vals[:, :n].double().sum(0)
        self.dst0 = sixteenths(n, seed=seed + 1)
        self.dbuf, self.dst = guarded_like(self.dst0, DEV, k)
        self.dst2 = self.d2buf = None
        if off2 is not None:
            self.sum2 = vals[:, off2:off2 + n2].double().sum(0)
            self.dst20 = sixteenths(n2, seed=seed + 2)
            self.d2buf, self.dst2 = guarded_like(self.dst20, DEV, k2)

    def reset(self, value=None):
        self.dst.copy_(self.dst0 if value is None else torch.full_like(self.dst0, value))
        if self.dst2 is not None:
            self.dst2.copy_(self.dst20 if value is None else torch.full_like(self.dst20, value))

    def row(self, force_atomics=False):
        """the table entry and its block count, by the contract of include/fwair.h"""
        nchunks = ((self.end + 3) // 4 + 63) // 64
        zper = min(self.nz, 64)
        splits = (self.nz + zper - 1) // zper
        upw = max(1, 32 // zper)
        blocks = (nchunks * splits + 4 * upw - 1) // (4 * upw)
        unaligned = self.dst.data_ptr() % 16 != 0 or (self.dst2 is not None and self.dst2.data_ptr() % 16 != 0)
        atomics = int(splits > 1 or unaligned or force_atomics)
        return ([self.slab.data_ptr(), self.dst.data_ptr(), self.dst2.data_ptr() if self.dst2 is not None else 0, self.n, self.zstride,
                 self.off2 or 0, self.n2, self.nz, zper, nchunks, upw, atomics], blocks)

    def check(self, what, accumulate=True):
        base = self.dst0.double() if accumulate else torch.zeros(self.n, dtype=torch.float64)
        assert_guarded(self.dbuf, (base + self.sum).float(), self.k, f'{what}: dst of nz={self.nz} n={self.n} off2={self.off2} n2={self.n2}')
        if self.dst2 is not None:
            base2 = self.dst20.double() if accumulate else torch.zeros(self.n2, dtype=torch.float64)
            assert_guarded(self.d2buf, (base2 + self.sum2).float(), self.k2, f'{what}: dst2 of nz={self.nz} n={self.n} off2={self.off2} n2={self.n2}')


def fold_multi(slabs, force_atomics=False):
    rows, offs = [], [0]
    for s in slabs:
        r, blocks = s.row(force_atomics)
        rows.append(r)
        offs.append(offs[-1] + blocks)
    tab = torch.tensor(rows, dtype=torch.int64).to(DEV)
    prefix = torch.tensor(offs, dtype=torch.int64).to(DEV)
    call('fw_slab_reduce_multi', tab, prefix, len(slabs), offs[-1])
    torch.cuda.synchronize()
    return rows, offs


def edge_slabs():
    """every nz x n edge without a second segment, then the second segment at off2 in {256, 258} x n2 in {3, 4, 56} behind n in
    {4, 250, 252, 256} (NaN between n and off2), nz cycling through the same edges"""
    out, seed = [], 100
    for nz in NZS:
        for n in NS:
            out.append(Slab(nz, n, seed, pad=(0, 4, 8)[len(out) % 3]))
            seed += 3
    i = 0
    for n in (4, 250, 252, 256):
        for off2 in (256, 258):
            for n2 in (3, 4, 56):
                out.append(Slab(NZS[i % len(NZS)], n, seed, off2=off2, n2=n2, pad=(0, 4)[i % 2]))
                seed += 3
                i += 1
    return out


def test_slab_multi_edges_plain_and_atomic():
    """nz at the edges of the unroll by 8 and above zper (atomics), every upw, the straddling word at n = 250, the dst2 vector path
    (off2 = 256) and element path (off2 = 258, n2 = 3), all as entries of ONE launch; then the same data with atomics forced."""
    slabs = edge_slabs()
    rows, _ = fold_multi(slabs)
    assert {r[10] for r in rows} == {32, 4, 3, 2, 1} and {r[11] for r in rows} == {0, 1}       # upw values; both paths in one launch
    for s, r in zip(slabs, rows):
        assert r[11] == int(s.nz > 64)
        s.check('plain where the contract allows')
    first = [(s.dbuf.clone(), None if s.d2buf is None else s.d2buf.clone()) for s in slabs]
    for s in slabs:
        s.reset()
    rows, _ = fold_multi(slabs, force_atomics=True)
    assert all(r[11] == 1 for r in rows)
    for s, (d, d2) in zip(slabs, first):
        s.check('atomics forced')
        assert_bits(s.dbuf, d, 'atomics 0 / 1 on the same data')
        if d2 is not None:
            assert_bits(s.d2buf, d2, 'atomics 0 / 1 on the same data (dst2)')


COUNT_SPECS = [(130, 1028), (1, 4), (65, 1028), (7, 250), (130, 260), (13, 256), (64, 1028), (9, 252), (130, 1028), (8, 4), (65, 260)]


@pytest.mark.parametrize('num', [1, 2, 5, 37])
def test_slab_multi_entry_search(num):
    """1, 2, 5 and 37 entries: one-block entries between many-block ones, so a wrong search over `prefix` folds a neighbour's slab
    (or nothing) into an entry -- every destination and its guards would show it."""
    slabs = []
    for i in range(num):
        nz, n = COUNT_SPECS[i % len(COUNT_SPECS)]
        kw = dict(off2=256, n2=56) if (i % 7 == 3 and n <= 256) else {}
        slabs.append(Slab(nz, n, 500 + 3 * i, **kw))
    rows, offs = fold_multi(slabs)
    blocks = [b - a for a, b in zip(offs, offs[1:])]
    assert blocks[0] >= 4
    if num >= 5:
        assert any(blocks[i] == 1 and blocks[i - 1] > 1 and blocks[i + 1] > 1 for i in range(1, num - 1)), blocks
    for s in slabs:
        s.check(f'{num} entries, blocks {blocks}')


def test_slab_multi_unaligned_destinations_with_atomics():
    """destinations at base pointers that are no multiple of 16 (the contract then asks for atomics = 1)"""
    slabs = [Slab(7, 250, 700, k=1), Slab(9, 252, 703, off2=256, n2=56, k2=3), Slab(65, 260, 706, k=2), Slab(8, 256, 709, off2=258, n2=4, k=1, k2=1)]
    rows, _ = fold_multi(slabs)
    assert all(r[11] == 1 for r in rows)
    for s in slabs:
        s.check('unaligned')


def single_grid_y(nz, end, accumulate):
    """gridDim.y of fw_slab_reduce's launch (its host code: z is split only when accumulating, >= 8 slab rows per block)"""
    if not accumulate:
        return 1
    gx = ((end + 3) // 4 + 63) // 64
    splits = max(1, min(1024 // gx, nz // 8))
    zper = (nz + splits - 1) // splits
    return (nz + zper - 1) // zper


@pytest.mark.parametrize('accumulate', [0, 1])
def test_slab_reduce_single(accumulate):
    """fw_slab_reduce at the same nz and n edges; nz >= 16 with accumulate = 1 splits z over gridDim.y (atomics); accumulate = 0
    must overwrite whatever dst held (NaN here)."""
    slabs = edge_slabs()
    ys = set()
    for s in slabs:
        if not accumulate:
            s.reset(NAN)
        ys.add(single_grid_y(s.nz, s.end, accumulate))
        call('fw_slab_reduce', s.slab, s.nz, s.n, s.zstride, s.dst, accumulate, s.dst2, s.off2 or 0, s.n2)
    torch.cuda.synchronize()
    assert ys == ({1, 8, 15} if accumulate else {1}), ys                 # nz = 64 / 65 -> 8 z ranges, 130 -> 15
    for s in slabs:
        s.check(f'single launch, accumulate={accumulate}', accumulate=bool(accumulate))


@pytest.fixture
def slab_queue(monkeypatch):
    ops = OPS()
    for name in ('_host_ring', '_host_reserved'):
        monkeypatch.setattr(ops, name, list(getattr(ops, name)))
    monkeypatch.setattr(ops, '_host_next', list(ops._host_next))
    try:
        yield ops
    finally:
        torch.cuda.synchronize()
        ops._pending.clear(); ops._pending_w.clear()


@pytest.fixture
def fold_tables(monkeypatch):
    """every fw_slab_reduce_multi launch of ops, its table copied to the host: rows [num, 12]"""
    ops = OPS()
    seen, orig = [], ops.call

    def spy(name, *args):
        if name == 'fw_slab_reduce_multi':
            seen.append(args[0].cpu()[:args[2] * 12].view(args[2], 12).clone())
        return orig(name, *args)

    monkeypatch.setattr(ops, 'call', spy)
    return seen


def deferred_fold(ops, items):
    """queue the folds inside one backward pass (ops.slab_reduce(defer=True)); its end-of-pass callback launches them"""
    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t * 1.0

        @staticmethod
        def backward(ctx, d):
            for s, dst, dst2 in items:
                ops.slab_reduce(s.slab, s.nz, s.n, s.zstride, dst, dst2, s.off2 or 0, s.n2, defer=True)
            assert len(ops._pending) == len(items), 'the folds were not deferred'
            return d

    t = torch.ones(1, device=DEV, requires_grad=True)
    Fn.apply(t).sum().backward()
    torch.cuda.synchronize()
    assert not ops._pending


def atomics_words(fold_tables, num):
    assert len(fold_tables) == 1 and fold_tables[0].shape == (num, 12), 'one fold launch per backward pass'
    return fold_tables[0][:, 11].tolist()


def test_flush_two_slabs_into_one_destination(slab_queue, fold_tables):
    a, b = Slab(7, 250, 800), Slab(13, 250, 803)
    deferred_fold(slab_queue, [(a, a.dst, None), (b, a.dst, None)])
    assert atomics_words(fold_tables, 2) == [1, 1], 'two entries share a destination: both must add with atomics'
    assert_guarded(a.dbuf, (a.dst0.double() + a.sum + b.sum).float(), 0, 'two slabs, one dst')


def test_flush_unaligned_dst(slab_queue, fold_tables):
    s, aligned = Slab(9, 252, 810, k=1), Slab(9, 252, 813)
    assert s.dst.data_ptr() % 16 == 4 and aligned.dst.data_ptr() % 16 == 0
    deferred_fold(slab_queue, [(s, s.dst, None), (aligned, aligned.dst, None)])
    assert atomics_words(fold_tables, 2) == [1, 0], 'the plain 16-byte path is for aligned, unshared, unsplit entries only'
    aligned.check('the aligned sole writer next to it')
    s.check('dst view at a pointer not divisible by 16')


def test_flush_unaligned_dst2(slab_queue, fold_tables):
    s = Slab(8, 256, 820, off2=256, n2=56, k2=3)
    assert s.dst.data_ptr() % 16 == 0 and s.dst2.data_ptr() % 16 == 12
    deferred_fold(slab_queue, [(s, s.dst, s.dst2)])
    assert atomics_words(fold_tables, 1) == [1]
    s.check('dst2 view at a pointer not divisible by 16')


# ================================================================================================ 2. Adam, tick, EMA, shadows
def ticked_hyper(ticks, lr=1e-3):
    """-> (device hyper after `ticks` fw_adam_tick calls, the f32 products computed on the host)"""
    hyper = torch.tensor([lr, 1.0, 1.0, 0.0], device=DEV)
    want = np.array([lr, 1.0, 1.0, 0.0], dtype=np.float32)
    for _ in range(ticks):
        call('fw_adam_tick', hyper, B1, B2)
        want[1] *= np.float32(B1); want[2] *= np.float32(B2); want[3] += np.float32(1)
    return hyper, torch.from_numpy(want)


SHADOWS = {'bf16': (1, BF), 'f32': (0, F32), 'none': (0, None)}


class AdamState:
    """guarded p, g, m, v (and shadow) at base offset k"""

    def __init__(self, n, k, shadow, seed, scale):
        self.n, self.k = n, k
        self.shadow_code, self.shadow_dtype = SHADOWS[shadow]
        host = self.host = adam_case(n, seed, scale)
        self.bufs, self.views = {}, {}
        for name, arr in zip('pgmv', host):
            self.bufs[name], self.views[name] = guarded_like(torch.from_numpy(arr), DEV, k)
        self.g_host = torch.from_numpy(host[1])
        self.shbuf = self.sh = None
        if self.shadow_dtype is not None:
            self.shbuf, self.sh = guarded(n, self.shadow_dtype, DEV, k)

    def step(self, hyper, lo=0, hi=None, what=''):
        """one fw_adam on elements [lo, hi) against the f64 reference fed with the device's own state"""
        hi = self.n if hi is None else hi
        v = {name: t[lo:hi] for name, t in self.views.items()}
        before = {name: v[name].cpu().double() for name in 'pgmv'}
        h = hyper.cpu()
        call('fw_adam', self.shadow_code, v['p'], v['g'], v['m'], v['v'], None if self.sh is None else self.sh[lo:hi], hi - lo, hyper,
             B1, B2, EPS)
        torch.cuda.synchronize()
        assert_bits(hyper, h, f'{what}: fw_adam must not write hyper')
        ref = adam_reference(before['p'], before['g'], before['m'], before['v'], h, B1, B2, EPS)
        for name in 'mvp':
            assert_bound_1d(v[name], ref[name], ref['tol_' + name], f'{what}: {name}')
        return ref

    def check_layout(self, what, lo=0, hi=None):
        """sentinels of all five buffers; g untouched; the shadow = the stored p (rounded to nearest even for bf16) on [lo, hi)"""
        hi = self.n if hi is None else hi
        for name in 'pmv':
            assert_guarded(self.bufs[name], self.views[name], self.k, f'{what}: guards of {name}')
        assert_guarded(self.bufs['g'], self.g_host, self.k, f'{what}: g')
        if self.sh is not None:
            want = torch.full((self.n,), SENTINEL, dtype=self.shadow_dtype)
            want[lo:hi] = self.views['p'][lo:hi].to(self.shadow_dtype).cpu()
            assert_guarded(self.shbuf, want, self.k, f'{what}: shadow')


@pytest.mark.parametrize('shadow', ['bf16', 'f32', 'none'])
@pytest.mark.parametrize('n', [1, 63, 257, 10007])
@pytest.mark.parametrize('k', [0, 1, 2, 3, 5])
def test_adam_one_step(k, n, shadow):
    # scale 1e-6 is where the bound tells the wrong kernels apart (tests/test_step_bounds_cpu.py): sqrt(v) of the order of eps
    run_adam_one_step(k, n, shadow, 1e-6)


def test_adam_one_step_unit_scale():
    """gradients and moments of order 1, where eps is 1e-8 of the denominator: the same bound, the ordinary operating point"""
    run_adam_one_step(3, 10007, 'bf16', 1.0)


def run_adam_one_step(k, n, shadow, scale):
    hyper, _ = ticked_hyper(3)
    st = AdamState(n, k, shadow, seed=k, scale=scale)
    what = f'adam n={n} base offset {k} shadow {shadow} scale {scale}'
    ref = st.step(hyper, what=what)
    st.check_layout(what)
    # the edge elements: a zero or underflowing gradient on a zero state gives an update far below an ulp of p: p stays, bit for bit
    p0, g0, m0, v0 = (torch.from_numpy(a) for a in st.host)
    still = (m0 == 0) & (v0 == 0) & (g0.abs() <= 1e-20)
    assert n < 6 or int(still.sum()) >= 2
    assert_bits(st.views['p'].cpu()[still], p0[still], f'{what}: p at g in {{0, 1e-20}}, m = v = 0')
    assert float((p0.double() - ref['p']).abs()[still].max() if bool(still.any()) else 0.0) < 1e-12


def test_adam_second_grid_pass():
    n = CAP + 257
    hyper, _ = ticked_hyper(2)
    st = AdamState(n, 1, 'bf16', seed=7, scale=1e-6)
    st.step(hyper, what='adam second grid pass')
    st.check_layout('adam second grid pass')


def test_adam_shadow_follows_every_step():
    """3 steps; after step 2 the shadow is the p of step 2, not of step 1 -- and the two differ, so a shadow written before the
    update cannot pass"""
    n = 10007
    hyper = torch.tensor([1e-2, 1.0, 1.0, 0.0], device=DEV)
    st = AdamState(n, 3, 'bf16', seed=9, scale=1.0)
    for step in range(3):
        g = torch.from_numpy(adam_case(n, 20 + step, 1.0)[1])
        st.views['g'].copy_(g); st.g_host = g
        old = st.views['p'].to(BF).cpu()
        call('fw_adam_tick', hyper, B1, B2)
        st.step(hyper, what=f'adam step {step + 1} of 3')
        st.check_layout(f'adam step {step + 1} of 3')
        changed = int((old.view(torch.int16) != st.views['p'].to(BF).cpu().view(torch.int16)).sum())
        assert changed > n // 10, f'step {step + 1}: the bf16 image of p moved at {changed} elements only: a stale shadow would not show'


def test_adam_tick_and_two_segments():
    """3 ticks against f32 products; then two hyper vectors ticked independently drive two disjoint segments of one flat buffer"""
    hyper, want = ticked_hyper(3)
    assert_bits(hyper, want, 'hyper after 3 ticks')
    hyper_rest, want_rest = ticked_hyper(1, lr=2e-3)
    assert_bits(hyper_rest, want_rest, 'hyper_rest after 1 tick')
    n, ne = 4099, 1001
    st = AdamState(n, 0, 'bf16', seed=11, scale=1e-6)
    st.step(hyper, 0, ne, what='segment [0, ne)')
    st.check_layout('after the first segment', 0, ne)                   # nothing of [ne, n) written yet, the shadow there included
    tail0 = {name: st.views[name][ne:].clone() for name in 'pmv'}
    st2 = st.step(hyper_rest, ne, n, what='segment [ne, n)')
    st.check_layout('after both segments')
    assert float((tail0['p'].cpu().double() - st2['p']).abs().max()) > 1e-4      # the tail did move, by its own hyper
    assert_bits(hyper, want, 'hyper'); assert_bits(hyper_rest, want_rest, 'hyper_rest')


def run_ema(n, k, shadow, seed, what):
    code, sdt = SHADOWS[shadow]
    g = gen(seed)
    pk0, pq0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    kbuf, pk = guarded_like(pk0, DEV, k)
    qbuf, pq = guarded_like(pq0, DEV, k)
    shbuf, sh = guarded(n, sdt, DEV, k) if sdt is not None else (None, None)
    call('fw_ema', code, pk, pq, sh, n, 0.999)
    torch.cuda.synchronize()
    x, tol = ema_reference(pk0.double(), pq0.double(), 0.999)
    assert_bound_1d(pk, x, tol, f'{what}: pk')
    assert_guarded(kbuf, pk, k, f'{what}: guards of pk')
    assert_guarded(qbuf, pq0, k, f'{what}: pq')
    if sh is not None:
        assert_guarded(shbuf, pk.to(sdt), k, f'{what}: shadow')


@pytest.mark.parametrize('shadow', ['bf16', 'f32', 'none'])
@pytest.mark.parametrize('n', [1, 63, 257, 10007])
@pytest.mark.parametrize('k', [0, 1, 2, 3, 5])
def test_ema(k, n, shadow):
    run_ema(n, k, shadow, 30 + k, f'ema n={n} base offset {k} shadow {shadow}')


@pytest.mark.parametrize('shadow', ['bf16', 'f32'])
def test_ema_second_grid_pass(shadow):
    run_ema(CAP + 257, 1, shadow, 40, f'ema second grid pass, shadow {shadow}')


# ================================================================================================ 3. casts, copies, permutes, LeakyReLU, fill
def normal_values(n, seed):
    """finite normal f32 values whose first elements are the rounding edges: exact ties of the bf16 grid and both zeros"""
    x = torch.randn(n, generator=gen(seed)) * 3
    edge = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, 2.0 ** -100, -3.0e38])
    x[:min(n, edge.numel())] = edge[:n]
    return x


def test_bf16_ties_round_to_even_on_the_host():
    """the host conversion the bit-exact tests compare with is round-to-nearest-even, stated without torch's own rounding"""
    x = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0])
    assert_bits(x.to(BF), torch.tensor([0x3f80, 0x3f82, 0xbf80 - 65536, 0xbf82 - 65536, 0, 0x8000 - 65536], dtype=torch.int16).view(BF), 'RNE')


@pytest.mark.parametrize('dtype', [BF, F32])
@pytest.mark.parametrize('n,k', [(1, 0), (1001, 1), (1001, 3), (CAP + 257, 1)])
def test_cast_flat(dtype, n, k):
    x = normal_values(n, 50 + k)
    sbuf, src = guarded_like(x, DEV, k)
    dbuf, dst = guarded(n, dtype, DEV, k)
    call('fw_cast_flat', 1 if dtype == BF else 0, src, dst, n)
    torch.cuda.synchronize()
    assert_guarded(dbuf, x.to(dtype), k, f'cast_flat n={n} k={k}')
    assert_guarded(sbuf, x, k, 'cast_flat source')


def padded_rows(vals, ld, pad_value, dtype=None):
    """-> (buf, 2-D view [rows, cols] with row stride ld) on the device: vals inside, pad_value in the pad columns and the guards"""
    rows, cols = vals.shape
    dtype = dtype or vals.dtype
    buf = torch.full((GUARD + rows * ld + GUARD,), pad_value, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(vals.to(dtype))
    return buf, view


def want_rows(vals, ld, dtype):
    rows, cols = vals.shape
    want = torch.full((GUARD + rows * ld + GUARD,), SENTINEL, dtype=dtype)
    want[GUARD:GUARD + rows * ld].view(rows, ld)[:, :cols] = vals.to(dtype)
    return want


@pytest.mark.parametrize('dtype', [BF, F32])
@pytest.mark.parametrize('rps', [0, 1, 3, 37])
def test_cast_rows(dtype, rps):
    rows, cols, lds, ldd = 37, 20, 28, 24
    x = normal_values(rows * cols, 60).view(rows, cols).clone()
    x[x.abs() > 1e30] = 1.0                                             # the scale below must not overflow
    _, src = padded_rows(x, lds, NAN)
    dbuf, dst = padded_rows(torch.full((rows, cols), SENTINEL), ldd, SENTINEL, dtype)
    scale = None
    want = x
    if rps:
        scale = torch.rand((rows + rps - 1) // rps, generator=gen(61)) + 0.5
        want = x * scale.repeat_interleave(rps)[:rows, None]            # one f32 rounding, then the cast's
    call('fw_cast_rows', 1 if dtype == BF else 0, src, lds, dst, ldd, rows, cols, None if scale is None else scale.to(DEV), max(rps, 1))
    torch.cuda.synchronize()
    assert_bits(dbuf, want_rows(want, ldd, dtype), f'cast_rows rows_per_scale={rps}')


def test_cast_rows_second_grid_pass():
    rows, cols, lds, ldd = 65540, 128, 132, 136
    assert rows * cols // 4 > CAP
    x = torch.randn(rows, cols, generator=gen(62))
    scale = torch.rand((rows + 2) // 3, generator=gen(63)) + 0.5
    _, src = padded_rows(x, lds, NAN)
    dbuf, dst = padded_rows(torch.full((rows, cols), SENTINEL), ldd, SENTINEL, BF)
    call('fw_cast_rows', 1, src, lds, dst, ldd, rows, cols, scale.to(DEV), 3)
    torch.cuda.synchronize()
    assert_bits(dbuf, want_rows(x * scale.repeat_interleave(3)[:rows, None], ldd, BF), 'cast_rows above the grid cap')


@pytest.mark.parametrize('accumulate', [0, 1])
def test_copy_rows(accumulate):
    rows, cols, lds, ldd = 37, 20, 28, 24
    x, d0 = normal_values(rows * cols, 64).view(rows, cols), torch.randn(rows, cols, generator=gen(65))
    _, src = padded_rows(x, lds, NAN)
    dbuf, dst = padded_rows(d0, ldd, SENTINEL)
    call('fw_copy_rows', src, lds, dst, ldd, rows, cols, accumulate)
    torch.cuda.synchronize()
    assert_bits(dbuf, want_rows(x + d0 if accumulate else x, ldd, F32), f'copy_rows accumulate={accumulate}')


@pytest.mark.parametrize('dtype', [BF, F32])
def test_add_rows(dtype):
    rows, cols, lds, ldd = 37, 20, 28, 24
    x, d0 = torch.randn(rows, cols, generator=gen(66)).to(dtype), torch.randn(rows, cols, generator=gen(67)).to(dtype)
    _, src = padded_rows(x, lds, NAN)
    dbuf, dst = padded_rows(d0, ldd, SENTINEL)
    call('fw_add_rows', 1 if dtype == BF else 0, src, lds, dst, ldd, rows, cols)
    torch.cuda.synchronize()
    assert_bits(dbuf, want_rows((d0.float() + x.float()).to(dtype), ldd, dtype), f'add_rows {dtype}')   # RNE of the f32 sum


def permuted(src, dims, strides, base):
    """host statement of out[a*s0 + b*s1 + c*s2] = src[a][b][c] into a copy of `base` (1-D)"""
    a, b, c = torch.meshgrid(*(torch.arange(d) for d in dims), indexing='ij')
    idx = (a * strides[0] + b * strides[1] + c * strides[2]).reshape(-1)
    assert idx.unique().numel() == idx.numel() and int(idx.min()) >= 0 and int(idx.max()) < base.numel()
    out = base.clone()
    out[idx] = src.reshape(-1).to(base.dtype)
    return out, idx


PERMUTES = {'taps': ((112, 1, 9), (1, 0, 112)),                   # depthwise (C, 1, 9) -> tap-major (9, C)
            'k4s2': ((112, 56, 16), (16 * 56, 1, 56)),            # Downsample weight (2C, C, 4x4) -> [Cout][(ky, kx, ci)]
            'k4s2_grad': ((112, 16, 56), (16 * 56, 1, 16)),       # ... and its gradient back
            'gaps': ((5, 7, 3), (50, 6, 2))}                      # a strided destination: the words in between stay as they were


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('pair', [(F32, F32), (F32, BF), (BF, F32)])
@pytest.mark.parametrize('shape', list(PERMUTES))
def test_permute3(shape, pair, accumulate):
    dims, strides = PERMUTES[shape]
    tin, tout = pair
    n = dims[0] * dims[1] * dims[2]
    span = 1 + sum((d - 1) * s for d, s in zip(dims, strides))
    x = normal_values(n, 70).to(tin)
    base = torch.randn(span, generator=gen(71)).to(tout) if accumulate else torch.full((span,), SENTINEL, dtype=tout)
    _, src = guarded_like(x, DEV)
    dbuf, dst = guarded_like(base, DEV)
    call('fw_permute3', int(tin == BF), int(tout == BF), src, dst, *dims, *strides, accumulate)
    torch.cuda.synchronize()
    want, idx = permuted(x.float(), dims, strides, base.float())
    if accumulate:
        want[idx] = x.float().reshape(-1) + base.float()[idx]             # one f32 sum, then the output's rounding
    assert_guarded(dbuf, want.to(tout), 0, f'permute3 {shape} {tin}->{tout} accumulate={accumulate}')


def test_permute3_rejects_bf16_to_bf16():
    x = torch.zeros(64, dtype=BF, device=DEV)
    dbuf, dst = guarded(64, BF, DEV)
    with pytest.raises(RuntimeError, match='fw_permute3'):
        call('fw_permute3', 1, 1, x, dst, 4, 4, 4, 16, 4, 1, 0)
    torch.cuda.synchronize()
    assert_guarded(dbuf, torch.full((64,), SENTINEL, dtype=BF), 0, 'a rejected call writes nothing')


MULTI_SPECS = [((1, 1, 1), (0, 0, 1)), ((3, 11, 31), (1, 3 * 31, 3)), ((8, 8, 16), (16, 128, 1)), ((5, 5, 41), (41, 5 * 41, 1)),
               ((4099, 1, 1), (2, 0, 0)), ((112, 1, 9), (1, 0, 112)), ((2, 16, 33), (33, 66, 1)),
               ((112, 56, 16), (16 * 56, 1, 56))]                    # the k4s2 weight: 100352 elements, 98 blocks


@pytest.mark.parametrize('num', [1, 2, 37])
def test_permute3_multi(num):
    """entries of 1, 1023, 1024, 1025 and 4099 elements (the last with a strided destination), f32 and bf16 outputs mixed: every
    destination, its gaps and its guards bit-equal to fw_permute3 on the same entry and to the host statement"""
    # a 5-block entry first, the one-element entry behind it; then the 98-block entry between small ones: a block stride other than
    # 1024 elements still covers an entry of a few blocks (the blocks overlap), from 43 blocks on it leaves the tail unwritten
    order = [4, 0, 7, 1, 3, 2, 5, 6]
    rows, offs, ents = [], [0], []
    for i in range(num):
        dims, strides = MULTI_SPECS[order[i % len(order)]]
        tout = BF if (i + i // 8) % 2 else F32
        n = dims[0] * dims[1] * dims[2]
        span = 1 + sum((d - 1) * s for d, s in zip(dims, strides))
        x = normal_values(n, 80 + i)
        src = x.to(DEV)
        dbuf, dst = guarded(span, tout, DEV)
        rbuf, rdst = guarded(span, tout, DEV)
        rows.append([src.data_ptr(), dst.data_ptr(), *dims, *strides, int(tout == BF), 0])
        offs.append(offs[-1] + (n + 1023) // 1024)
        ents.append((x, src, dims, strides, tout, span, dbuf, rbuf, rdst))
    assert {e[2][0] * e[2][1] * e[2][2] for e in ents} >= ({4099} if num == 1 else {4099, 1})
    if num == 37:
        assert {e[2][0] * e[2][1] * e[2][2] for e in ents} >= {1, 1023, 1024, 1025, 4099, 100352} and {e[4] for e in ents} == {BF, F32}
        assert {e[4] for e in ents if e[2] == (112, 56, 16)} == {BF, F32}
    tab = torch.tensor(rows, dtype=torch.int64).to(DEV)
    prefix = torch.tensor(offs, dtype=torch.int64).to(DEV)
    call('fw_permute3_multi', tab, prefix, num, offs[-1])
    for x, src, dims, strides, tout, span, dbuf, rbuf, rdst in ents:
        call('fw_permute3', 0, int(tout == BF), src, rdst, *dims, *strides, 0)
    torch.cuda.synchronize()
    for i, (x, src, dims, strides, tout, span, dbuf, rbuf, rdst) in enumerate(ents):
        want, _ = permuted(x.to(tout), dims, strides, torch.full((span,), SENTINEL, dtype=tout))
        assert_guarded(rbuf, want, 0, f'fw_permute3 on entry {i} {dims}')
        assert_bits(dbuf, rbuf, f'entry {i} of {num} {dims} -> {tout}: fw_permute3_multi vs fw_permute3')


@pytest.mark.parametrize('dtype', [BF, F32])
@pytest.mark.parametrize('n,k', [(1, 0), (1001, 1), (CAP + 257, 3)])
def test_lrelu(dtype, n, k):
    slope = torch.tensor(0.1, dtype=F32)
    x = normal_values(n, 90)
    if n > 8:
        x[6] = 1.5
    dy = torch.randn(n, generator=gen(91)).to(dtype)
    xbuf, xs = guarded_like(x, DEV, k)
    ybuf, y = guarded(n, dtype, DEV, k)
    gbuf, dyd = guarded_like(dy, DEV, k)
    dxbuf, dx = guarded(n, F32, DEV, k)
    code = 1 if dtype == BF else 0
    call('fw_lrelu_fwd', code, xs, y, n, 0.1)
    call('fw_lrelu_bwd', code, dyd, xs, dx, n, 0.1)
    torch.cuda.synchronize()
    assert_guarded(ybuf, torch.where(x > 0, x, x * slope).to(dtype), k, f'lrelu_fwd {dtype} n={n}')      # -0.0 * slope = -0.0
    assert_guarded(dxbuf, dy.float() * torch.where(x > 0, torch.ones(()), slope), k, f'lrelu_bwd {dtype} n={n}')   # slope at x <= 0
    assert_guarded(xbuf, x, k, 'lrelu x'); assert_guarded(gbuf, dy, k, 'lrelu dy')


@pytest.mark.parametrize('n,k', [(1, 0), (1001, 1), (1001, 3), (CAP + 257, 1)])
def test_fill(n, k):
    buf, view = guarded(n, F32, DEV, k)
    call('fw_fill', view, n, -3.25)
    torch.cuda.synchronize()
    assert_guarded(buf, torch.full((n,), -3.25), k, f'fill n={n} k={k}')


# ================================================================================================ 4. losses
def l1_run(a, b, gscale, with_da=True):
    n = a.numel()
    lbuf, loss = guarded_like(torch.zeros(1), DEV)
    dabuf, da = guarded(n, F32, DEV) if with_da else (None, None)
    call('fw_l1_loss', a, b, da, n, gscale, loss)
    torch.cuda.synchronize()
    assert_guarded(lbuf, loss, 0, 'guards of the loss')
    return loss.cpu(), dabuf, da


def check_l1_grad(dabuf, da, a, b, gscale):
    n = a.numel()
    d = (a.cpu().double() - b.cpu().double())
    ref = torch.sign(d) * (float(np.float32(gscale)) / n)
    assert_bound_1d(da, ref, 2 * U32 * ref.abs(), 'l1 da: sign * (gscale / n) to 1 ulp')
    assert bool((da.cpu()[d == 0] == 0).all()), 'a == b must give exactly 0'
    assert_guarded(dabuf, da, 0, 'guards of da')


def test_l1_loss_exact():
    """a - b in {-1, -0.5, 0, 0.5, 1} at n = 2^22: every partial sum and s / n are exact, so the loss has ONE right value"""
    n = 1 << 22
    g = gen(95)
    d = torch.randint(-2, 3, (n,), generator=g).float() / 2
    b = torch.randint(-4, 5, (n,), generator=g).float() / 2
    a = b + d
    assert bool(((a.double() - b.double()) == d.double()).all()) and bool((d == 0).any())
    ad, bd = a.to(DEV), b.to(DEV)
    want = torch.tensor([float(d.double().abs().sum()) / n], dtype=torch.float64)
    loss, dabuf, da = l1_run(ad, bd, 0.7)
    assert_bits(loss, want.float(), 'l1 loss'); assert float(loss) == float(want)
    check_l1_grad(dabuf, da, ad, bd, 0.7)
    loss_none, _, _ = l1_run(ad, bd, 0.7, with_da=False)
    assert_bits(loss_none, loss, 'l1 loss with da = NULL')
    i = int((d == 0.5).nonzero()[-1])                                   # the last such element: in the tail of the grid-stride loop
    ad[i] += 0.5
    loss2, _, _ = l1_run(ad, bd, 0.7, with_da=False)
    assert float(loss2) - float(loss) == 0.5 / n, f'one element moved by 0.5: the loss moved by {float(loss2) - float(loss)!r}, not {0.5 / n!r}'


def test_l1_loss_ragged():
    n = CAP + 257
    g = gen(96)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    b[:1000] = a[:1000]
    ad, bd = a.to(DEV), b.to(DEV)
    want, tol = l1_loss_bound(a.double(), b.double())
    loss, dabuf, da = l1_run(ad, bd, 0.6)
    print(f'l1 ragged: loss {float(loss)!r}, reference {want!r}, |difference| {abs(float(loss) - want):.3e}, bound {tol:.3e}')
    assert abs(float(loss) - want) <= tol
    check_l1_grad(dabuf, da, ad, bd, 0.6)


@pytest.mark.parametrize('N', [1, 49, 64, 65, 4097])
@pytest.mark.parametrize('R', [1, 6, 300])
def test_ce0_loss(R, N):
    gscale = 0.6
    x = torch.randn(R, N, generator=gen(97 + R + N)) * 3
    if N >= 3:
        x[R - 1, 1], x[R - 1, 2] = 80.0, -80.0                          # finite only because the row maximum is subtracted
    if N >= 65 and R >= 2:
        x[0, 0], x[0, N - 1] = -80.0, 80.0                              # the label column at the bottom, the maximum in the tail
    xd = x.to(DEV)
    lbuf, loss = guarded_like(torch.zeros(1), DEV)
    dbuf, dl = guarded(R * N, F32, DEV)
    call('fw_ce0_loss', xd, dl, R, N, gscale, loss)
    torch.cuda.synchronize()
    x64 = x.double()
    lse = torch.logsumexp(x64, dim=1)
    want_loss = (lse - x64[:, 0]).mean().reshape(1)
    want_dl = torch.exp(x64 - lse[:, None])
    want_dl[:, 0] -= 1
    want_dl *= float(np.float32(gscale)) / R
    got = dl.cpu().view(R, N)
    assert_guarded(lbuf, loss, 0, 'guards of the loss'); assert_guarded(dbuf, dl, 0, 'guards of dlogits')
    if N == 1:
        assert float(loss) == 0.0 and bool((got == 0).all()), 'one class: loss and gradient are exactly 0'
    else:
        close(loss, want_loss, 1e-5, f'ce0 loss R={R} N={N}')
        close(got, want_dl, 1e-5, f'ce0 dlogits R={R} N={N}')
    rowsum = got.double().sum(1).abs().max().item()
    bound = N * 2.0 ** -23 * gscale / R
    print(f'ce0 R={R} N={N}: max |row sum of dlogits| {rowsum:.3e}, bound {bound:.3e}')
    assert rowsum <= bound, f'ce0 R={R} N={N}: a row of dlogits sums to {rowsum:.3e} > {bound:.3e}'
    loss.zero_()
    call('fw_ce0_loss', xd, None, R, N, gscale, loss)
    torch.cuda.synchronize()
    if N == 1:
        assert float(loss) == 0.0
    else:
        close(loss, want_loss, 1e-5, 'ce0 loss with dlogits = NULL')
