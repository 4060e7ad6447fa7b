"""fwair.lib.graph_capture: every HIP-graph capture of the package runs with Python's cyclic garbage collected beforehand and the
collector off until the capture ends; where a capture is preceded by warm-up steps the region opens before them, because the
set of live parameters must not change between the two (functional.refresh_shadows).  A collection inside a capture (torch.cuda.graph does not collect on entry any more) destroys
whatever dead cycle is around -- an earlier engine with its graphs and pools -- under the capture, which has aborted the process."""
import gc
import weakref

import pytest
import torch


class Node:
    pass


def cycle():
    a, b = Node(), Node()
    a.other, b.other = b, a
    return weakref.ref(a)


def test_gc_quiet_collects_first_and_restores():
    from fwair.lib import gc_quiet
    assert gc.isenabled()
    dead = cycle()
    with gc_quiet():
        assert dead() is None and not gc.isenabled()
        inner = cycle()
        [Node() for _ in range(5000)]                       # far past the generation-0 threshold: nothing collects
        assert inner() is not None
        with gc_quiet():                                    # nested: neither collects nor re-enables
            assert inner() is not None and not gc.isenabled()
        assert not gc.isenabled()
    assert gc.isenabled()
    gc.disable()
    try:
        with gc_quiet():
            pass
        assert not gc.isenabled()                           # an outer choice is kept
    finally:
        gc.enable()
    with pytest.raises(ValueError):
        with gc_quiet():
            raise ValueError
    assert gc.isenabled()


def test_every_capture_of_the_package_goes_through_the_guard():
    import os
    import fwair
    root = os.path.dirname(os.path.abspath(fwair.__file__))
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith('.py') and f != 'lib.py':
                src = open(os.path.join(dirpath, f)).read()
                assert 'torch.cuda.graph(' not in src and 'capture_begin' not in src, f


@pytest.mark.gpu
def test_graph_capture_runs_with_the_collector_off():
    from fwair.lib import graph_capture
    x = torch.zeros(64, device='cuda')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x.add_(1.0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    dead = cycle()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        assert dead() is None and not gc.isenabled()
        x.add_(1.0)
    assert gc.isenabled()
    g.replay(); g.replay()
    torch.cuda.synchronize()
    assert float(x.sum()) == 64 * 3.0
