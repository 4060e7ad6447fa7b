"""Grouped weight gradients (fwair/ops.py: wgrad(defer=True), _flush_wgrads, _launch_group; csrc/fw_gemm.hip:
gemm_wgrad_group_kernel / gemm_wgrad_group_big_kernel) against a float64 reference built from the same bf16-rounded operands:
dW = dW0 + dY^T x, db = db0 + sum dY.  Every product runs through a small autograd.Function whose backward queues it, as the
model's Linear backward does, so the end-of-pass callback launches it.

Besides the shapes, these tests pin the host-side contract of the launch: which tiles STORE instead of add (only the sole writer
of a range marked zero by ops.mark_zeroed), which add with atomics (products of one pass whose gradients overlap), that the work
table covers every (problem, tile, slice) exactly once, and that a table overflow, a captured pass and a failed pass leave the
gradients right.  Tolerance: rel-to-max 2e-3 (f32 accumulation of exact bf16 products; a lost contribution is ~10 % or more)."""
import pytest
import torch

from helpers import close
from test_ops_gpu import rnd

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 2e-3
SENTINEL = -1234.5625                                       # exactly representable: must come back bit-identical


def OPS():
    from fwair import ops
    return ops


class Prod:
    """One dW = dY^T x product: bf16 operands on the host (the reference) and on the device, rows optionally padded (ld > cols)."""

    def __init__(self, n, k, m, seed, gpad=0, xpad=0):
        self.n, self.k, self.m = n, k, m
        self.g = (rnd(m, n, seed=seed) * 0.3).to(torch.bfloat16)
        self.x = (rnd(m, k, seed=seed + 7919) * 0.3).to(torch.bfloat16)
        self.gd, self.xd = _dev(self.g, gpad), _dev(self.x, xpad)

    def dw(self):
        return self.g.double().t() @ self.x.double()

    def db(self):
        return self.g.double().sum(0)

    def renew(self, seed):
        """New operand values in the same device buffers (a captured pass re-reads them at every replay)."""
        self.g = (rnd(self.m, self.n, seed=seed) * 0.3).to(torch.bfloat16)
        self.x = (rnd(self.m, self.k, seed=seed + 7919) * 0.3).to(torch.bfloat16)
        self.gd.copy_(self.g.to(DEV)); self.xd.copy_(self.x.to(DEV))


def _dev(t, pad):
    """Device copy whose rows are 16-byte aligned (ld a multiple of 8), `pad` extra elements wide."""
    ld = (t.shape[1] + 7) // 8 * 8 + pad
    buf = torch.full((t.shape[0], ld), 3.0, dtype=t.dtype, device=DEV)       # garbage in the pad: must not be read
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


def backward_pass(items, raise_after=False):
    """One backward pass whose backward hands every (product, dw, db) to ops.wgrad(defer=True) in order."""
    ops = OPS()

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t * 1.0

        @staticmethod
        def backward(ctx, d):
            for p, dw, db in items:
                ops.wgrad(p.gd, p.xd, p.n, p.k, p.m, dw, db, defer=True)
            if raise_after:
                raise ValueError('backward failed after queueing its products')
            return d

    t = torch.ones(1, device=DEV, requires_grad=True)
    Fn.apply(t).sum().backward()


@pytest.fixture
def engine_mode(monkeypatch):
    """Engine-like global state (direct_grads on, as TrainEngine leaves it), restored afterwards together with the queues, the zeroed
    marks and the pinned table ring."""
    from fwair import functional as Fn
    ops = OPS()
    monkeypatch.setattr(Fn.config, 'direct_grads', True)
    for name in ('_host_ring', '_host_reserved'):
        monkeypatch.setattr(ops, name, list(getattr(ops, name)))
    monkeypatch.setattr(ops, '_host_next', list(ops._host_next))
    ops.clear_marks()
    try:
        yield ops
    finally:
        torch.cuda.synchronize()
        ops.clear_marks()
        ops._pending.clear(); ops._pending_w.clear()


@pytest.fixture
def fires(monkeypatch):
    """Every grouped launch, its table copied to the host: (rows [nprob, 16], items [total, 4], nprob, total, tile)."""
    ops = OPS()
    seen, orig = [], ops._group_fire

    def fire(table, probs, nprob, total, tile):
        host = table.cpu()
        seen.append((host[:nprob * 16].view(nprob, 16).clone(), host[nprob * 16:].view(torch.int32).view(total, 4).clone(),
                     nprob, total, tile))
        orig(table, probs, nprob, total, tile)

    monkeypatch.setattr(ops, '_group_fire', fire)
    return seen


def zeroed(n, k, ops, mark=True):
    buf = torch.zeros(n, k, device=DEV)
    if mark:
        ops.mark_zeroed(buf)
    return buf


def modes(fires):
    """Epilogue of every unsliced product of the recorded launches, in table order: 'store', 'rmw' or 'atomic'."""
    out = []
    for rows, _, _, _, _ in fires:
        for r in rows.tolist():
            if r[10] == 1:
                out.append('store' if (r[12] == 1 and r[14] == 0) else {1: 'rmw', 2: 'atomic'}[r[14]])
    return out


def check_schedule(fires, chunk):
    """Every (problem, m tile, n tile, slice) of every launch's products appears exactly once; the rest is (-1, ...) padding;
    the item count is a multiple of the 8 XCDs; a product's slices cover its tokens in whole 32-token steps."""
    for rows, items, nprob, total, tile in fires:
        assert total % 8 == 0 and items.shape[0] == total
        want = set()
        for pi, r in enumerate(rows.tolist()):
            n, k, m, kper, sk = r[6], r[7], r[8], r[9], r[10]
            assert kper % 32 == 0 and sk == max(1, -(-m // kper)) and (sk - 1) * kper < m <= sk * kper
            assert sk == 1 or kper <= chunk, 'a slice longer than FW_WGRAD_CHUNK'
            want |= {(pi, bx, by, z) for bx in range(-(-n // tile)) for by in range(-(-k // tile)) for z in range(sk)}
        real = [tuple(it) for it in items.tolist() if it[0] != -1]
        pad = [tuple(it) for it in items.tolist() if it[0] == -1]
        assert all(p == (-1, 0, 0, 0) for p in pad)
        assert len(real) == len(set(real)), 'a work item appears twice'
        assert set(real) == want, f'work items missing {sorted(want - set(real))[:4]} / extra {sorted(set(real) - want)[:4]}'


def check(p_list, dw, dw0, what):
    ref = (dw0.double() if dw0 is not None else torch.zeros(dw.shape, dtype=torch.float64))
    for p in p_list:
        ref = ref + p.dw()
    close(dw, ref, TOL, what)


# ---------------------------------------------------------------------------------------------------------- 1. shape matrix
SHAPES = [
    (220, 300, 1024),      # min side below _GROUP_BIG_MIN: 128 x 128 tiles, ragged against 128 and 256
    (300, 220, 1024),
    (224, 388, 2048),      # exactly _GROUP_BIG_MIN: 256 x 256 tiles, both sides ragged
    (388, 228, 2048),
    (228, 228, 512),
    (8, 4, 32),            # the smallest groupable problem
    (96, 136, 4096),       # exactly _GROUP_CHUNK tokens: one slice
    (96, 136, 4096 + 32),  # two slices (2080 + 2048 tokens)
    (260, 228, 4096 + 32),
    (132, 72, 3 * 4096 - 32),  # three slices, the last one 32 tokens short
]


@pytest.mark.parametrize('form', ['add', 'store'])
@pytest.mark.parametrize('with_db', [True, False])
@pytest.mark.parametrize('n,k,m', SHAPES)
def test_shape_matrix(engine_mode, fires, n, k, m, with_db, form):
    ops = engine_mode
    assert ops._GROUP_CHUNK == 4096 and ops._GROUP_BIG_MIN == 224
    p = Prod(n, k, m, seed=n + 3 * k + m, gpad=8 if m % 64 == 0 else 0, xpad=16 if m % 64 == 0 else 0)
    if form == 'store':
        dw0 = torch.zeros(n, k)
        dw = zeroed(n, k, ops)
    else:
        dw0 = rnd(n, k, seed=5)
        dw = dw0.to(DEV)
    db0 = rnd(n, seed=6) if with_db else None
    db = db0.to(DEV) if with_db else None
    backward_pass([(p, dw, db)])
    torch.cuda.synchronize()
    assert not ops._pending_w and not ops._pending
    check([p], dw, dw0, f'dW {n}x{k} over {m} tokens ({form})')
    if with_db:
        close(db, db0.double() + p.db(), TOL, 'db')
    assert len(fires) == 1 and fires[0][4] == (256 if min(n, k) >= 224 else 128)
    if m <= ops._GROUP_CHUNK:
        assert modes(fires) == (['store'] if form == 'store' else ['rmw'])
    check_schedule(fires, ops._GROUP_CHUNK)


@pytest.mark.parametrize('form', ['add', 'store'])
@pytest.mark.parametrize('n,k,m', [(200, 120, 1024), (260, 228, 2048), (8, 4, 64)])
def test_strided_dw_inside_a_larger_buffer(engine_mode, fires, n, k, m, form):
    """dW a strided view (row stride > k) inside a bigger f32 buffer, db inside another: the pad columns and the rows before and after
    hold a sentinel that must come back bit-identical, whether the tiles store (sole writer of a marked range) or add."""
    ops = engine_mode
    ld, before, after = k + 12, 3, 2
    p = Prod(n, k, m, seed=11 + n)
    buf = torch.zeros(before + n + after, ld, device=DEV)
    bbuf = torch.zeros(n + 8, device=DEV)
    if form == 'store':
        ops.mark_zeroed(buf); ops.mark_zeroed(bbuf)
    # sentinels written behind the marks' back: the plain store must not touch them (they are not part of dW)
    buf.fill_(SENTINEL)
    bbuf.fill_(SENTINEL)
    dw = buf[before:before + n, :k]
    db = bbuf[4:4 + n]
    dw0 = torch.zeros(n, k) if form == 'store' else rnd(n, k, seed=12)
    dw.copy_(dw0.to(DEV)); db.zero_()
    assert dw.stride(0) == ld and dw.data_ptr() % 16 == 0
    backward_pass([(p, dw, db)])
    torch.cuda.synchronize()
    assert modes(fires) == (['store'] if form == 'store' else ['rmw'])
    check([p], dw, dw0, f'strided dW ({form})')
    close(db, p.db(), TOL, 'db')
    host = buf.cpu()
    mask = torch.ones_like(host, dtype=torch.bool)
    mask[before:before + n, :k] = False
    assert (host[mask] == SENTINEL).all(), 'the launch wrote outside dW (pad columns or neighbouring rows)'
    bh = bbuf.cpu()
    assert (bh[:4] == SENTINEL).all() and (bh[4 + n:] == SENTINEL).all(), 'the bias gradient spilled'


# ---------------------------------------------------------------------------------------------------------- 2. schedule coverage
def _mixed():
    """Small and big tile forms, ragged, sliced (with a short last slice) and whole, with and without db."""
    return [Prod(200, 72, 8192 + 64, seed=1), Prod(96, 136, 1024, seed=2), Prod(300, 260, 4096 + 32, seed=3),
            Prod(448, 232, 2048, seed=4), Prod(56, 224, 3 * 4096 - 32, seed=5), Prod(136, 96, 512, seed=6)]


@pytest.mark.parametrize('unit_bx,chunk', [(1, None), (2, None), (3, None), (1, 1024), (3, 1024)])
def test_schedule_covers_every_tile_once(engine_mode, fires, monkeypatch, unit_bx, chunk):
    ops = engine_mode
    monkeypatch.setattr(ops, '_GROUP_UNIT_BX', unit_bx)
    if chunk is not None:
        monkeypatch.setattr(ops, '_GROUP_CHUNK', chunk)
    prods = _mixed()
    dws = [rnd(p.n, p.k, seed=20 + i) for i, p in enumerate(prods)]
    dev = [(p, w.to(DEV), torch.zeros(p.n, device=DEV) if i % 2 == 0 else None) for i, (p, w) in enumerate(zip(prods, dws))]
    backward_pass(dev)
    torch.cuda.synchronize()
    assert not ops._pending_w and not ops._pending
    assert sorted(f[4] for f in fires) == [128, 256]
    check_schedule(fires, ops._GROUP_CHUNK)
    for (p, dw, db), w0 in zip(dev, dws):
        check([p], dw, w0, f'dW {p.n}x{p.k} over {p.m} tokens, unit {unit_bx}, chunk {ops._GROUP_CHUNK}')
        if db is not None:
            close(db, p.db(), TOL, 'db')


# ---------------------------------------------------------------------------------------------------------- 3. table overflow
def test_table_overflow_splits_the_launch(engine_mode, fires, monkeypatch):
    """A host table too small for one pass: each tile form's launch is cut into halves (recursively), sliced products on both sides
    of every cut; a slab queued by the pass before the flush must survive the bookkeeping of the cut."""
    ops = engine_mode
    monkeypatch.setattr(ops, '_HOST_WORDS', 120)                 # also bounds the slab fold's table (7 slabs here: 92 words)
    monkeypatch.setattr(ops, '_host_ring', [])
    monkeypatch.setattr(ops, '_host_next', [0])
    monkeypatch.setattr(ops, '_host_reserved', [])
    C = 4096
    prods = [Prod(200, 200, 2 * C + 64, seed=31), Prod(200, 200, 1024, seed=32), Prod(136, 72, 2 * C + 64, seed=33),
             Prod(200, 200, 2 * C + 64, seed=34), Prod(72, 136, 512, seed=35), Prod(136, 200, 2 * C + 64, seed=36),
             Prod(260, 260, 2 * C + 64, seed=37), Prod(264, 228, 1024, seed=38), Prod(260, 232, 2 * C + 64, seed=39),
             Prod(260, 260, 1024, seed=40), Prod(232, 264, 2048, seed=41)]
    dws = [rnd(p.n, p.k, seed=40 + i) for i, p in enumerate(prods)]
    dev = [(p, w.to(DEV), torch.zeros(p.n, device=DEV)) for p, w in zip(prods, dws)]
    slab = rnd(3, 64, seed=50).to(DEV)
    dst = torch.zeros(64, device=DEV)

    class Early(torch.autograd.Function):                        # a slab fold of the pass, queued before the launches queue theirs
        @staticmethod
        def forward(ctx, t):
            return t * 1.0

        @staticmethod
        def backward(ctx, d):
            ops.slab_reduce(slab, 3, 64, 64, dst, defer=True)
            return d

    class Late(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t * 1.0

        @staticmethod
        def backward(ctx, d):
            for p, dw, db in dev:
                ops.wgrad(p.gd, p.xd, p.n, p.k, p.m, dw, db, defer=True)
            return d

    t = torch.ones(1, device=DEV, requires_grad=True)
    Late.apply(Early.apply(t)).sum().backward()                  # backward: Late's products queue after Early's slab
    torch.cuda.synchronize()
    assert not ops._pending and not ops._pending_w
    assert sum(f[4] == 128 for f in fires) >= 2 and sum(f[4] == 256 for f in fires) >= 2, 'the table did not overflow'
    for rows, _, nprob, total, _ in fires:
        assert nprob * 16 + total * 2 <= 120
    check_schedule(fires, ops._GROUP_CHUNK)
    assert sorted(r[6] * 100000 + r[7] * 10 + (r[10] > 1) for f in fires for r in f[0].tolist()) == \
        sorted(p.n * 100000 + p.k * 10 + (p.m > C) for p in prods), 'every product in exactly one launch'
    for (p, dw, db), w0 in zip(dev, dws):
        check([p], dw, w0, f'dW {p.n}x{p.k} over {p.m} tokens after a table overflow')
        close(db, p.db(), TOL, 'db')
    close(dst, slab.cpu().double().sum(0), 1e-5, 'the foreign slab fold')


# ---------------------------------------------------------------------------------------------------------- 4. freshness, shared writers
def test_sole_writer_of_a_zeroed_buffer_stores(engine_mode, fires):
    ops = engine_mode
    p = Prod(224, 448, 2048, seed=60)
    dw = zeroed(224, 448, ops)
    backward_pass([(p, dw, None)])
    torch.cuda.synchronize()
    assert modes(fires) == ['store']
    check([p], dw, None, 'sole writer, zeroed')


def test_direct_grads_alone_never_permits_a_store(engine_mode, fires):
    """The buffer holds data and nobody marked it zero: the product adds, even with direct_grads on."""
    ops = engine_mode
    p = Prod(224, 448, 2048, seed=61)
    dw0 = rnd(224, 448, seed=62)
    dw = dw0.to(DEV)
    backward_pass([(p, dw, None)])
    torch.cuda.synchronize()
    assert modes(fires) == ['rmw']
    check([p], dw, dw0, 'sole writer, unmarked buffer with data')


@pytest.mark.parametrize('n,k', [(136, 96), (256, 288)])
@pytest.mark.parametrize('writers', [2, 8])
def test_shared_writers_add_atomically(engine_mode, fires, writers, n, k):
    """Several products of identical shape and token count into ONE marked-zero dW: same tile class, same launch, same tiles spread
    over the XCDs -- they must add with atomics, and every contribution must arrive."""
    ops = engine_mode
    prods = [Prod(n, k, 2048, seed=70 + i) for i in range(writers)]
    dw = zeroed(n, k, ops)
    db = torch.zeros(n, device=DEV)
    backward_pass([(p, dw, db) for p in prods])
    torch.cuda.synchronize()
    assert modes(fires) == ['atomic'] * writers
    check(prods, dw, None, f'{writers} writers into one dW')
    close(db, sum(p.db() for p in prods), TOL, 'db of all writers')


@pytest.mark.parametrize('order', ['groupable_first', 'immediate_first'])
@pytest.mark.parametrize('imm_m', [4096 + 16, 1008])
def test_groupable_and_immediate_writer(engine_mode, fires, order, imm_m):
    """A non-groupable product (m % 32 != 0: ops.wgrad runs it at once) adds into the same marked-zero dW as a queued one.  4112 tokens:
    split-K slab whose fold is deferred to the end of the pass; 1008 tokens: one GEMM that adds into dW before the grouped launch."""
    ops = engine_mode
    q = Prod(136, 232, 2048, seed=80)
    imm = Prod(136, 232, imm_m, seed=81)
    assert not ops._groupable(imm.gd, imm.xd, imm.n, imm.k, imm.m, torch.zeros(136, 232, device=DEV), None)
    dw = zeroed(136, 232, ops)
    items = [(q, dw, None), (imm, dw, None)]
    backward_pass(items if order == 'groupable_first' else items[::-1])
    torch.cuda.synchronize()
    assert modes(fires) == ['rmw']
    check([q, imm], dw, None, f'queued + immediate writer of {imm_m} tokens ({order})')


def test_sliced_and_unsliced_writer(engine_mode, fires):
    ops = engine_mode
    a = Prod(200, 136, 3 * 4096 + 64, seed=90)
    b = Prod(200, 136, 1024, seed=91)
    dw = zeroed(200, 136, ops)
    db = torch.zeros(200, device=DEV)
    backward_pass([(a, dw, db), (b, dw, db)])
    torch.cuda.synchronize()
    assert modes(fires) == ['rmw']
    check([a, b], dw, None, 'sliced + unsliced writer')
    close(db, a.db() + b.db(), TOL, 'db')


@pytest.mark.parametrize('C,K', [(64, 128), (96, 256)])
def test_fused_qkv_overlap(engine_mode, fires, C, K):
    """One product into the fused [3C, K] gradient, another into its [2C, K] tail view: different data_ptr()s, overlapping bytes.
    (C = 96, K = 256: the two land in different tile classes, hence different launches.)"""
    ops = engine_mode
    gw = zeroed(3 * C, K, ops)
    a = Prod(3 * C, K, 1024, seed=100)
    b = Prod(2 * C, K, 1024, seed=101)
    backward_pass([(a, gw, None), (b, gw[C:], None)])
    torch.cuda.synchronize()
    assert modes(fires) == ['atomic', 'atomic']
    ref = a.dw()
    ref[C:] += b.dw()
    close(gw, ref, TOL, 'fused QKV gradient')


def test_second_pass_adds(engine_mode, fires):
    """Two backward passes into the same buffers with no zeroing in between (gradient accumulation): twice one pass."""
    ops = engine_mode
    prods = [Prod(224, 448, 2048, seed=110), Prod(136, 96, 1024, seed=111), Prod(200, 72, 8192 + 64, seed=112)]
    flat = torch.zeros(sum(p.n * p.k + p.n for p in prods), device=DEV)
    ops.mark_zeroed(flat)
    items, o = [], 0
    for p in prods:
        dw = flat[o:o + p.n * p.k].view(p.n, p.k); o += p.n * p.k
        items.append((p, dw, flat[o:o + p.n])); o += p.n
    backward_pass(items)
    backward_pass(items)
    torch.cuda.synchronize()
    assert modes(fires) == ['store', 'store', 'rmw', 'rmw']
    for p, dw, db in items:
        close(dw, 2 * p.dw(), TOL, f'dW {p.n}x{p.k} after two passes')
        close(db, 2 * p.db(), TOL, 'db after two passes')


def test_untouched_marks_survive_a_pass(engine_mode, fires):
    """A pass writes part of a marked buffer; the next pass (the encoder stage of the engine's two-stage backward) still stores into
    the part nobody wrote, and adds into the part that was written."""
    ops = engine_mode
    a, b = Prod(136, 96, 1024, seed=120), Prod(224, 232, 1024, seed=121)
    flat = torch.zeros(a.n * a.k + b.n * b.k, device=DEV)
    ops.mark_zeroed(flat)
    dwa, dwb = flat[:a.n * a.k].view(a.n, a.k), flat[a.n * a.k:].view(b.n, b.k)
    backward_pass([(a, dwa, None)])
    backward_pass([(b, dwb, None), (a, dwa, None)])
    torch.cuda.synchronize()
    assert modes(fires) == ['store', 'store', 'rmw']
    close(dwa, 2 * a.dw(), TOL, 'dW written in both passes')
    close(dwb, b.dw(), TOL, 'dW of the second pass')


# ---------------------------------------------------------------------------------------------------------- 5. captured pass
def test_captured_pass_replays(engine_mode):
    """As TrainEngine.capture: eager warm-up on a side stream, reserve_capture_tables, capture zeroing + mark + backward, then replay
    with new operand values copied into the static inputs; sole writers, a shared pair and a sliced product."""
    ops = engine_mode
    prods = [Prod(224, 448, 2048, seed=130), Prod(136, 96, 1024, seed=131), Prod(136, 96, 1024, seed=132),
             Prod(200, 72, 8192 + 64, seed=133)]
    flat = torch.zeros(224 * 448 + 224 + 136 * 96 + 200 * 72 + 200, device=DEV)
    views = [flat[:224 * 448].view(224, 448), flat[224 * 448:224 * 448 + 224]]
    o = 224 * 448 + 224
    shared = flat[o:o + 136 * 96].view(136, 96); o += 136 * 96
    last = flat[o:o + 200 * 72].view(200, 72); o += 200 * 72
    items = [(prods[0], views[0], views[1]), (prods[1], shared, None), (prods[2], shared, None), (prods[3], last, flat[o:o + 200])]

    def one_pass():
        flat.zero_()
        ops.mark_zeroed(flat)
        backward_pass(items)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        one_pass()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ops.reserve_capture_tables()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_pass()
    for rep in range(2):
        for i, p in enumerate(prods):
            p.renew(1000 * (rep + 1) + i)
        graph.replay()
        torch.cuda.synchronize()
        close(views[0], prods[0].dw(), TOL, f'replay {rep}: sole writer')
        close(views[1], prods[0].db(), TOL, f'replay {rep}: db')
        close(shared, prods[1].dw() + prods[2].dw(), TOL, f'replay {rep}: shared pair')
        close(last, prods[3].dw(), TOL, f'replay {rep}: sliced product')
        close(flat[o:o + 200], prods[3].db(), TOL, f'replay {rep}: sliced db')


# ---------------------------------------------------------------------------------------------------------- 6. failed pass
@pytest.mark.parametrize('where', ['backward', 'launch'])
def test_failed_pass_leaves_nothing_behind(engine_mode, fires, monkeypatch, where):
    """A pass that queues products and then dies -- in a backward function, or in the grouped launch itself -- must not change the
    result of the next clean pass."""
    ops = engine_mode
    a, b = Prod(224, 232, 2048, seed=140), Prod(136, 96, 8192 + 64, seed=141)
    dwa, dwb = zeroed(224, 232, ops), zeroed(136, 96, ops)
    items = [(a, dwa, None), (b, dwb, None)]
    if where == 'backward':
        with pytest.raises((ValueError, RuntimeError)):
            backward_pass(items, raise_after=True)
    else:
        orig = ops._group_fire

        def boom(*args):
            raise RuntimeError('launch failed')

        monkeypatch.setattr(ops, '_group_fire', boom)
        with pytest.raises(RuntimeError):
            backward_pass(items)
        monkeypatch.setattr(ops, '_group_fire', orig)
        assert not ops._pending and not ops._pending_w and not ops._zeroed
    torch.cuda.synchronize()
    dwa.zero_(); dwb.zero_()
    ops.mark_zeroed(dwa); ops.mark_zeroed(dwb)
    fires.clear()
    backward_pass(items)
    torch.cuda.synchronize()
    assert not ops._pending and not ops._pending_w
    check([a], dwa, None, f'clean pass after a failed one ({where})')
    check([b], dwb, None, f'sliced product, clean pass after a failed one ({where})')


# ---------------------------------------------------------------------------------------------------------- 7. the engine stores plainly
def test_engine_step_stores_every_unsliced_product(fires):
    """One eager TrainEngine step of the small bf16 model: every unsliced weight gradient of the step is the sole writer of a
    zeroed range and STORES its tiles (a fix that demoted them all to read-modify-write would cost 1 GB of reads per step)."""
    from fwair import engine as E
    from fwair import functional as Fn
    from helpers import synth_batch
    from test_engine_parity_gpu import build
    net, _, _ = build('bf16')
    try:
        eng = E.TrainEngine(net, lr=2e-4, contrast_loss_weight=0.6, use_graph=False)
        clean, q, k = synth_batch(2, 128, 'model.')
        out = eng.step_eager(q.to(DEV), k.to(DEV), clean.to(DEV))
        torch.cuda.synchronize()
        assert torch.isfinite(out).all()
        m = modes(fires)
        print(f'engine step: {len(m)} unsliced weight gradients in {len(fires)} grouped launches')
        assert m and set(m) == {'store'}, f'{m.count("rmw")} read-modify-write, {m.count("atomic")} atomic of {len(m)}'
        assert torch.isfinite(eng.flat_g).all()
    finally:
        Fn.config.direct_grads = False
        OPS().clear_marks()
