"""The decoder's learnable window modulator (--learnable_modulator, decoder_Uformer.py:536-539,687-691) on the host: the state_dict
schema with and without the flag, the fixture's separation, the index formula of include/fwair.h against a torch restatement of the
reference's window add, and the power of the wrong expectations tests/test_modulator_gpu.py holds the kernel's output against."""
import types

import pytest
import torch

from helpers import load, make_opt, rnd, schema
from modulator_cases import (B, GEOS, INDEX_CASES, MIN_REJECTED, SHIFTS, WIDTHS, fwd_bound, schema_modulator, unit_table, window_add,
                             window_pos, wrong_positions)

MODEL_LIMIT = 1e-4                 # restored_eval / restored_train / loss of the GPU model test


def _schema_of(net):
    return [(k, list(v.shape), str(v.dtype).replace('torch.', '')) for k, v in net.state_dict().items()]


def test_schema_with_the_flag_matches_reference():
    from net.model import AirNet
    net = AirNet(make_opt('all3', batch_size=1, learnable_modulator=True))
    ref = [(k, list(s), d) for k, s, d in schema_modulator()]
    assert _schema_of(net) == ref
    tables = [(k, s) for k, s, _ in ref if k.endswith('.modulator.weight')]
    assert len(tables) == 20 and all(k.startswith('R.R.decoderlayer_') for k, _ in tables)
    assert sorted({s[1] for _, s in tables}) == [112, 224, 448, 896] and all(s[0] == 64 for _, s in tables)
    # nn.Embedding's own initialisation stays (N(0, 1)): _init_weights touches Linear and LayerNorm only
    w = net.R.R.decoderlayer_0.blocks[0].modulator.weight
    assert 0.9 < float(w.detach().std()) < 1.1 and w.requires_grad
    assert net.R.R.encoderlayer_0.blocks[0].modulator is None and net.R.R.bottleneck_0.blocks[0].modulator is None


def test_schema_without_the_flag_is_unchanged():
    from net.model import AirNet
    net = AirNet(make_opt('all3'))
    assert _schema_of(net) == [(k, list(s), d) for k, s, d in schema('all3')]
    assert all(blk.modulator is None for blk in net.R.R.all_blocks())


def test_checkpoint_keys_set_the_flag():
    from net.model import options_from_checkpoint
    sd = {k: torch.empty(s) for k, s, _ in schema_modulator() if k.endswith('.modulator.weight') or k == 'E.E.queue'}
    opt = options_from_checkpoint(types.SimpleNamespace(batch_size=7, learnable_modulator=False), sd)
    assert opt.learnable_modulator is True and opt.batch_size == 1
    opt = options_from_checkpoint(types.SimpleNamespace(batch_size=7, learnable_modulator=True), {'R.R.x.norm1.weight': torch.empty(1)})
    assert opt.learnable_modulator is False and opt.batch_size == 7


def test_fixture_tells_an_omitted_table():
    """the golden's eval output moves by at least 100 x the model test's limit when every table is zeroed"""
    g = load('model_all3_modulator')
    sep = float((g['restored_eval'] - g['restored_eval_zero_mod']).abs().max() / g['restored_eval'].abs().max())
    print(f'max|restored_eval - restored_eval_zero_mod| / max|restored_eval| = {sep:.3e}')
    assert sep >= 100 * MODEL_LIMIT
    names = [str(n) for n in g['grad_names']]
    mod = [i for i, n in enumerate(names) if n.endswith('.modulator.weight')]
    assert len(mod) == 20
    floor = 1e-5 * float(g['grad_norms'].max())
    assert float(g['grad_norms'][mod].min()) > floor, 'a modulator gradient norm below the floor of the gradient-norm rule'


@pytest.mark.parametrize('H,W,s', INDEX_CASES)
def test_window_add_restatement_agrees_with_the_index_formula(H, W, s):
    C = 28
    y = rnd(f'modcpu.y{H}x{W}', (B * H * W, C))
    table = unit_table('modcpu.table', C)
    assert torch.equal(window_add(y, table, B, H, W, s), y + table[window_pos(B, H, W, s)])


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('C', WIDTHS)
def test_wrong_expectations_fall_outside_the_bound(C, dtype):
    """The right expectation y0 + mod[p] against the three wrong ones (s = 0 where s = 4, H and W exchanged, the table transposed in
    its 8x8 index), with the bound the GPU test uses.  A wrong position can coincide with the right one: exchanging H and W leaves
    xx mod 8 alone (8 | H, 8 | W) and matches yy mod 8 on one row in eight, a transposed index is its own on the diagonal -- at
    exactly 1/8 of the rows both, where the wrong expectation IS the right one and no bound can reject it.  Asked: the positions
    differ at 7/8 of the rows (all of them for the shift), and there the bound rejects at >= 99 % of the elements."""
    for H, W in GEOS:
        y0 = rnd(f'modcpu.y0.{H}x{W}x{C}', (B * H * W, C)).double()
        table = unit_table(f'modcpu.table{C}', C).double()
        for s in SHIFTS:
            p = window_pos(B, H, W, s)
            right = y0 + table[p]
            for name, pw in wrong_positions(B, H, W, s).items():
                differs = pw != p
                assert float(differs.double().mean()) == (1.0 if name == 'shift0' else 0.875), name
                wrong = y0 + table[pw]
                assert torch.equal(wrong[~differs], right[~differs])
                bad = ~((right - wrong).abs() <= fwd_bound(y0, table[pw], dtype))
                share = float(bad[differs].double().mean())
                assert share >= MIN_REJECTED, f'{name} at {H}x{W}, s = {s}: rejected at {share:.4f} of the elements'
