"""SHA-256 digests of the project's OWN outputs (no reference data): what fw_band_stats, fw_band_split and the fw_dft2t_* entries
write for the cases of tests/spec_bits_cases.py.  Run on the MI355X with the library built from the commit whose bits are to be
kept -- before a refactor of csrc/fw_spec.hip, csrc/fw_dft.hip or the shared chunk in csrc/fw_common.h, at its parent commit:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_spec_bits.py <commit hash> [out.json]

  spec_bits.json   {"commit": the hash given, "hipcc": `hipcc --version` (tests/test_spec_bits_gpu.py skips under another compiler),
                    "device": torch.cuda.get_device_name(0) -- the ROCm build of torch calls the MI355X "AMD Radeon Graphics",
                    "digests": {group: {case: sha256 of the output bytes}}}"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'frequency-wised_all-in-one_image_restoration_model_amd'), os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import torch  # noqa: E402

import spec_bits_cases as PC  # noqa: E402


def main():
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, 'spec_bits.json')
    res = dict(commit=sys.argv[1], hipcc=PC.toolchain(), device=torch.cuda.get_device_name(0),
               digests={g: PC.digests(g) for g in PC.GROUPS})
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{out}: ' + ', '.join(f'{g} {len(d)}' for g, d in res['digests'].items()))


if __name__ == '__main__':
    main()
