"""Host bookkeeping of the zeroed-range marks that decide whether a grouped weight gradient may STORE its tiles (fwair/ops.py:
mark_zeroed, _note_write, _is_zero, _clusters).  Pure address arithmetic on CPU tensors: no GPU, no kernel."""
import pytest
import torch

from fwair import ops


@pytest.fixture(autouse=True)
def _clean_marks():
    ops.clear_marks()
    yield
    ops.clear_marks()


def test_span_covers_strided_rows():
    buf = torch.zeros(10, 20)
    v = buf[2:5, 4:12]
    lo, hi = ops._span(v)
    assert lo == v.data_ptr() and hi == lo + 4 * (2 * 20 + 8)
    assert ops._span(buf[3:3]) == (buf[3:3].data_ptr(),) * 2


def test_clusters_see_overlap_not_adjacency():
    union, shared = ops._clusters([(0, 10), (10, 20), (30, 40), (35, 36), (50, 60), (5, 7)])
    assert union == [[0, 10], [10, 20], [30, 40], [50, 60]]
    assert shared == [True, False, True, True, False, True]


def test_marks_follow_writes():
    flat = torch.zeros(1000)
    a, b, c = flat[:100].view(10, 10), flat[100:400].view(10, 30), flat[100:400].view(10, 30)[:, 4:20]
    ops.mark_zeroed(flat)
    assert ops._is_zero(ops._span(a)) and ops._is_zero(ops._span(b)) and ops._is_zero(ops._span(c))
    ops._note_write(c)                                         # a write into part of b: b is no longer zero, a still is
    assert not ops._is_zero(ops._span(b)) and ops._is_zero(ops._span(a))
    assert ops._is_zero(ops._span(flat[400:]))
    ops._unmark([ops._span(a)])
    assert not ops._is_zero(ops._span(a)) and ops._is_zero(ops._span(flat[450:460]))
    ops.mark_zeroed(flat[:400])                                # re-zeroed: whole again (in two marked pieces)
    assert ops._is_zero(ops._span(a)) and ops._is_zero(ops._span(b)) and ops._is_zero(ops._span(flat[400:]))


def test_marks_hold_their_buffers():
    """A marked range must not be handed to another tensor while it is marked (its bytes would not be zero)."""
    t = torch.zeros(64)
    ops.mark_zeroed(t)
    assert any(b.data_ptr() == t.data_ptr() for b in ops._zeroed_bufs.values())
    ops.clear_marks()
    assert not ops._zeroed and not ops._zeroed_bufs
