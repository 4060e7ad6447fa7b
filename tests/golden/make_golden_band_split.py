"""Golden vectors of the reference's FrequencyDecompose (net/utils/frequency_decompose.py:5-125) on maps that are not square powers of
two -- runs ONLY where the reference checkout exists, like make_golden.py, whose helpers it imports unchanged.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_band_split.py

  unit_band_split.npz   for every (h, w) of tests/band_split_cases.py:GOLDEN_SIZES, every (kind, size) of GOLDEN_KINDS and inverse =
                        True / False / 'visual': the module's output on golden_input(h, w) = rnd('bandsplit.<h>x<w>', (1, 2, h, w)),
                        key '<h>x<w>|<kind>|<size>|<inverse>', [nb, 1, 2, h, w] (inverse=False: [..., 2], re and im).  The two largest
                        sizes are stored at every STRIDE-th pixel / bin of the two map axes.
                        The inputs are NOT stored: a test rebuilds them from the seed name.

A fixture is data (expected outputs); no reference source text is stored."""
import os
import sys

import torch

import make_golden as MG
from make_golden import FrequencyDecompose, save

sys.path.insert(0, os.path.join(MG.ROOT, 'tests'))
import band_split_cases as SC  # noqa: E402


def main():
    out = {}
    for h, w in SC.GOLDEN_SIZES:
        x = SC.golden_input(h, w)
        s = SC.STRIDE.get((h, w), 1)
        for kind, size in SC.GOLDEN_KINDS:
            for inv in SC.GOLDEN_INVERSE:
                with torch.no_grad():
                    y = FrequencyDecompose(kind, size, h, w, inverse=inv)(x)
                if torch.is_complex(y):
                    y = torch.view_as_real(y)
                out[SC.key(h, w, kind, size, inv)] = y[:, :, :, ::s, ::s].float()
    save('unit_band_split', **out)


if __name__ == '__main__':
    main()
