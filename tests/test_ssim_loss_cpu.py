"""Host side of the SSIM loss term (--ssim_loss_weight; fw_ssim11_loss): the torch-CPU restatement of tests/ssim_cases.py and the
closed-form gradient the kernel implements against the reference-run fixture tests/golden/unit_ssim11.npz
(tests/golden/make_ssim_golden.py; utils/pytorch_ssim/__init__.py:19-43), the option and the engine's signature."""
import inspect
import sys

import pytest
import torch

import ssim_cases as SC
from helpers import load

NAMES = [c[0] for c in SC.CASES]


@pytest.fixture(scope='module')
def golden():
    return load('unit_ssim11')


def _case(name):
    return next(c for c in SC.CASES if c[0] == name)


def _rel(got, want):
    return float((got - want).abs().max()) / float(want.abs().max())


@pytest.mark.parametrize('name', NAMES)
def test_fixture_records_the_case(golden, name):
    _, shape, seed, _ = _case(name)
    assert tuple(int(v) for v in golden[name + '.shape']) == shape and int(golden[name + '.seed']) == seed
    assert golden[name + '.grad'].shape == shape and golden[name + '.grad'].dtype == torch.float64
    assert float(golden[name + '.f32_grad_dev']) > 0 and float(golden[name + '.f32_value_dev']) >= 0


@pytest.mark.parametrize('name', NAMES)
def test_restatement_equals_the_reference_in_f64(golden, name):
    _, shape, seed, kind = _case(name)
    a, b = SC.inputs(shape, seed, kind)
    a = a.double().requires_grad_(True)
    v = SC.ssim(a, b.double())
    g, = torch.autograd.grad(v, a)
    assert abs(float(v.detach()) - float(golden[name + '.value'])) <= 1e-12 * abs(float(golden[name + '.value']))
    assert _rel(g, golden[name + '.grad']) <= 1e-12


@pytest.mark.parametrize('name', NAMES)
def test_closed_form_gradient_equals_the_reference_in_f64(golden, name):
    _, shape, seed, kind = _case(name)
    a, b = SC.inputs(shape, seed, kind)
    g = SC.closed_form_grad(a.double(), b.double())
    assert _rel(g, golden[name + '.grad']) <= 1e-12


def test_taps_are_the_kernels_constants():
    """fw_loss.hip carries the taps as f32 literals: the same eleven bit patterns."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'frequency-wised_all-in-one_image_restoration_model_amd',
                            'csrc', 'fw_loss.hip')).read()
    body = re.search(r'constexpr float g\[11\] = \{(.*?)\};', src, re.S).group(1)
    lits = [float.fromhex(t.strip().rstrip('f')) for t in body.split(',')]
    assert lits == [float(v) for v in SC.taps()]


def test_option_ssim_loss_weight(monkeypatch):
    monkeypatch.setattr(sys, 'argv', ['x', '--degradation_embedding_method', 'all_3_bands'])
    sys.modules.pop('option', None)
    try:
        import option
        p = option.build_parser()
        assert p.parse_args([]).ssim_loss_weight == 0.0
        assert p.parse_args(['--ssim_loss_weight', '0.2']).ssim_loss_weight == 0.2
        with pytest.raises(SystemExit):
            p.parse_args(['--ssim_loss_weight', 'much'])
    finally:
        sys.modules.pop('option', None)


def test_engine_signature_accepts_the_weight():
    from fwair import engine as E
    p = inspect.signature(E.TrainEngine.__init__).parameters
    assert 'ssim_loss_weight' in p and p['ssim_loss_weight'].default == 0.0
    assert list(inspect.signature(E.train_loss).parameters)[:5] == ['restored', 'clean', 'logits', 'w', 'gscale']
