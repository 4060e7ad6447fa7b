"""The bytes of fw_band_stats, fw_band_split and fw_dft2t_fwd / _bands / _decompose are pinned: SHA-256 of every output of the cases in
tests/spec_bits_cases.py against tests/golden/spec_bits.json, which tests/golden/make_spec_bits.py wrote on the MI355X at the commit
the fixture names.  Equality, never a tolerance: dft_pass_kernel of csrc/fw_dft.hip and the contracting kernels of csrc/fw_spec.hip
stand on one chunk type (csrc/fw_common.h, DftChunk) whose order of MFMAs per accumulator is a contract; a digest that
differs means an operation changed place -- the MFMA order, where a band's weight multiplies the fragment, the `s +=` of the band
reduction, where the scale is applied.  Group gattn_bands pins out and dqkv of the attention-map band filter (fw_gattn_bands_fwd /
bwd through vit.GlobalAttnFn) at N = 256 and, with lamb = 0, at N = 576 (spec_bits_cases.gattn_bands).  The digests hold for one compiler: under another `hipcc --version` the tests skip and say so
(a hipcc that cannot be run at all is an error)."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'spec_bits.json')


@pytest.fixture(scope='module')
def pinned():
    import spec_bits_cases as PC
    with open(FIXTURE) as f:
        fx = json.load(f)
    have = PC.toolchain()
    if have != fx['hipcc']:
        pytest.skip(f'spec_bits.json was written under another compiler: {fx["hipcc"]!r}, here {have!r}')
    return fx['digests']


@pytest.mark.parametrize('group', ['band_stats', 'band_split', 'dft2t', 'gattn_bands'])
def test_output_bytes(pinned, group):
    import spec_bits_cases as PC
    got, want = PC.digests(group), pinned[group]
    assert sorted(got) == sorted(want), 'the cases of spec_bits_cases.py are not those of the fixture'
    differ = [k for k in sorted(want) if got[k] != want[k]]
    assert not differ, f'{group}: {len(differ)} of {len(want)} outputs changed their bytes: {differ[:12]}'
