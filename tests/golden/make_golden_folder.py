"""Golden fixture of the folder data path -- runs only where the reference checkout exists (its root in FW_REFERENCE, default
/root/reference), like make_golden.py.

unit_crop_img.npz: seeded HWC uint8 arrays of sizes (37, 50), (128, 129), (321, 481) and what the reference's
utils/image_utils.py `crop_img` returns for them with base=16 (every call in utils/dataset_utils.py) and base=64 (its default).
A fixture is data (inputs / expected outputs); no reference source text is stored.  tests/test_folder_data_cpu.py needs only the fixture.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('FW_REFERENCE', '/root/reference')
SIZES = [(37, 50), (128, 129), (321, 481)]


def main():
    spec = importlib.util.spec_from_file_location('ref_image_utils', os.path.join(REF, 'utils', 'image_utils.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                                  # numpy, torch and PIL only
    rs = np.random.RandomState(20240)
    out = {}
    for k, (h, w) in enumerate(SIZES):
        # a seeded column term + a seeded row term that changes every 8 rows: any shift of the crop window changes the array, and
        # the file compresses (fully random bytes would exceed the size limit of a committed fixture)
        rows = np.repeat(rs.randint(0, 256, size=((h + 7) // 8, 1, 3)), 8, axis=0)[:h]
        img = ((rows + rs.randint(0, 256, size=(1, w, 3))) % 256).astype(np.uint8)
        out[f'in{k}'] = img
        out[f'base16_{k}'] = np.ascontiguousarray(mod.crop_img(img, base=16))
        out[f'base64_{k}'] = np.ascontiguousarray(mod.crop_img(img, base=64))
    np.savez_compressed(os.path.join(HERE, 'unit_crop_img.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
