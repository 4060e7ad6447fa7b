"""ctypes binding of libfwair_hip.so.  Prototypes are parsed from include/fwair.h (the single source of
truth for the C ABI), so the header, the library and this loader cannot drift apart silently."""
import contextlib
import ctypes
import gc
import os
import re

import torch

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, 'libfwair_hip.so')
# the header ships inside the package (build.sh copies include/fwair.h next to this file); a source checkout that has not been
# built yet falls back to the repository's include/ directory
HEADER_PATH = next((p for p in (os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fwair.h'),
                                os.path.join(os.path.dirname(_PKG), 'include', 'fwair.h')) if os.path.exists(p)),
                   os.path.join(os.path.dirname(_PKG), 'include', 'fwair.h'))

F32, BF16 = 0, 1
_CT = {'int': ctypes.c_int, 'long': ctypes.c_long, 'float': ctypes.c_float}


def parse_header(path=HEADER_PATH):
    """-> {name: [(ctype, is_pointer), ...]} for every `int fw_*(...)` declaration."""
    txt = open(path).read()
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    protos = {}
    for m in re.finditer(r'\bint\s+(fw_\w+)\s*\(([^)]*)\)\s*;', txt):
        name, args = m.group(1), m.group(2).strip()
        sig = []
        if args and args != 'void':
            for a in args.split(','):
                a = a.strip()
                if '*' in a:
                    sig.append((ctypes.c_void_p, True))
                else:
                    t = a.rsplit(' ', 1)[0].replace('const', '').strip()
                    sig.append((_CT[t], False))
        protos[name] = sig
    return protos


_lib = None
_protos = None


def lib():
    global _lib, _protos
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'fwair: HIP library not built: {LIB_PATH} (run build.sh / __graft_entry__.build()); '
                               'there is no CPU fallback')
        _protos = parse_header()
        L = ctypes.CDLL(LIB_PATH)
        for name, sig in _protos.items():
            fn = getattr(L, name)          # AttributeError if a declared symbol is not exported
            fn.restype = ctypes.c_int
            fn.argtypes = [t for t, _ in sig]
        _lib = L
    return _lib


def protos():
    lib()
    return _protos


def dt(dtype):
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise TypeError(f'fwair: unsupported dtype {dtype}')


def _ptr(x):
    if x is None:
        return None
    if torch.is_tensor(x):
        if not x.is_cuda:
            raise RuntimeError('fwair: tensor is not on a HIP device (the product path has no CPU implementation)')
        return x.data_ptr()
    return int(x)


def call(name, *args):
    """Call a C-ABI entry on torch's current HIP stream (appended as the last argument)."""
    L = lib()
    sig = _protos[name]
    if len(args) + 1 != len(sig):
        raise TypeError(f'{name}: expected {len(sig) - 1} arguments, got {len(args)}')
    conv = []
    for a, (t, isptr) in zip(args, sig):
        conv.append(_ptr(a) if isptr else a)
    conv.append(torch.cuda.current_stream().cuda_stream)
    rc = getattr(L, name)(*conv)
    if rc != 0:
        raise RuntimeError(f'fwair: {name} failed with code {rc} '
                           f'({"argument check at source line " + str(-rc) if rc < 0 else "hipError"})')


_quiet_depth = 0


@contextlib.contextmanager
def gc_quiet():
    """Collect Python's cyclic garbage now and keep the collector off until the block ends (its earlier state is restored).
    Re-entrant: a nested region neither collects nor re-enables -- between a capture's warm-up steps and the capture itself the set
    of live parameters must not change (functional.refresh_shadows builds its device table from it during the warm-up).
    For the ONE thread that drives captures: the depth is a plain module global, so a region opened from a second thread while one is
    open would neither collect nor restore; the engines capture from the thread that steps them, and nothing else opens one."""
    global _quiet_depth
    if _quiet_depth:
        yield
        return
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    _quiet_depth = 1
    try:
        yield
    finally:
        _quiet_depth = 0
        if was_on:
            gc.enable()


@contextlib.contextmanager
def graph_capture(graph, **kw):
    """torch.cuda.graph(graph, **kw) with Python's cyclic garbage collector out of the way.  torch.cuda.graph no longer collects on
    entry (torch.compiler.config.force_cudagraph_gc is off by default), so a collection that falls INSIDE the capture -- on this
    thread or on autograd's -- runs the destructors of whatever dead cycle is around: an engine of an earlier run with its graphs,
    private pools, streams and parameters (whose weak references edit functional's shadow tables).  A capture has aborted the
    process with the collector running on autograd's thread inside it; that it was the release of such objects under the capture is
    inferred from that traceback, not demonstrated.  Callers that warm up first open gc_quiet() around
    the warm-up AND the capture, so that the collection happens before both."""
    with gc_quiet():
        with torch.cuda.graph(graph, **kw):
            yield
