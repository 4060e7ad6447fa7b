"""Golden vectors of the reference's get_frequency_distribution (utils/visualization_utils.py:158-184) -- runs ONLY where the reference
checkout exists.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_band_stats.py

  unit_band_stats.npz   for every (h, w, size) of tests/band_stats_cases.py:CASES and its NIMG seeded images: the function's output
                        with norm=False ('<h>x<w>|<size>|raw', [NIMG][int(1 / size)]) and norm=True ('...|norm').
                        The images are NOT stored: a test rebuilds them from the seed name (band_stats_cases.images).

visualization_utils imports torchvision and imageio at module level, which are not installed; neither is used by the function, so
both names are registered as empty modules before the import (as oracle/refshim.py does for timm).
A fixture is data (expected outputs); no reference source text is stored."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'),
          os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)
sys.dont_write_bytecode = True

import band_stats_cases as BC  # noqa: E402
from refshim import REFERENCE_ROOT  # noqa: E402


def reference_function():
    for name in ('torchvision', 'imageio'):
        sys.modules.setdefault(name, types.ModuleType(name))
    os.environ.setdefault('MPLBACKEND', 'Agg')
    spec = importlib.util.spec_from_file_location('ref_visualization_utils', os.path.join(REFERENCE_ROOT, 'utils', 'visualization_utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.get_frequency_distribution


def main():
    f = reference_function()
    out = {}
    for h, w, size in BC.CASES:
        x = BC.images(h, w)
        for norm in (False, True):
            out[BC.key(h, w, size, norm)] = np.stack([np.asarray(f(x[i], size=size, norm=norm), dtype=np.float64) for i in range(BC.NIMG)])
        print(BC.key(h, w, size, False), out[BC.key(h, w, size, False)][0])
    np.savez(os.path.join(HERE, 'unit_band_stats.npz'), **out)


if __name__ == '__main__':
    main()
