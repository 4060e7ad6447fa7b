"""What tests/test_widths_cpu.py and tests/test_model_widths_gpu.py share: the state-dict schemas of the reference built at the
decoder widths 32 and 64 (tests/golden/schema_widths.json, written by tests/golden/make_golden_widths.py: one shape per key, the keys
and dtypes being those of schema.json's `all3`, which the generator asserts)."""
import json
import os

from helpers import GOLDEN, schema

WIDTHS = (32, 64)
_schemas = {}


def schema_width(E):
    """[(key, shape, dtype)] of the reference AirNet with embed_dim = E (all_3_bands, L = 3, freq, batch_size 1)"""
    if not _schemas:
        with open(os.path.join(GOLDEN, 'schema_widths.json')) as f:
            stored = json.load(f)
        assert stored.pop('keys') == 'schema.json:all3'
        base = schema('all3')
        for width, shapes in stored.items():
            assert len(shapes) == len(base)
            _schemas[int(width)] = [(k, s, d) for (k, _, d), s in zip(base, shapes)]
    return _schemas[E]
