"""Host side of the decoder widths (--embed_dim 32 / 56 / 64): what a checkpoint tells about its width, the module tree against the
reference's own state-dict schema at 32 and 64, and the refusal of any other width.  Construction needs no GPU."""
import types

import pytest
import torch

from helpers import make_opt
from widths_cases import WIDTHS, schema_width


def test_options_from_checkpoint_reads_the_width():
    from net.model import options_from_checkpoint
    sd = {'R.R.input_proj.proj.0.weight': torch.empty(32, 3, 3, 3), 'E.E.queue': torch.empty(3, 256, 12)}
    opt = options_from_checkpoint(types.SimpleNamespace(batch_size=7, learnable_modulator=True, embed_dim=56), sd)
    assert opt.embed_dim == 32 and isinstance(opt.embed_dim, int) and opt.batch_size == 4 and opt.learnable_modulator is False
    sd['R.R.input_proj.proj.0.weight'] = torch.empty(64, 3, 3, 3)
    assert options_from_checkpoint(opt, sd).embed_dim == 64
    # a state_dict without a Uformer decoder (another decoder_type) leaves the option alone
    opt = options_from_checkpoint(types.SimpleNamespace(batch_size=7, learnable_modulator=False, embed_dim=56), {'R.R.x.weight': torch.empty(1)})
    assert opt.embed_dim == 56


@pytest.mark.parametrize('E', WIDTHS)
def test_module_tree_has_the_reference_schema(E):
    from net.model import AirNet
    net = AirNet(make_opt('all3', batch_size=1, embed_dim=E))
    got = [(k, tuple(v.shape), str(v.dtype).replace('torch.', '')) for k, v in net.state_dict().items()]
    want = [(k, tuple(s), d) for k, s, d in schema_width(E)]
    assert [k for k, _, _ in got] == [k for k, _, _ in want], 'keys, in order'
    assert got == want
    assert dict((k, s) for k, s, _ in got)['R.R.input_proj.proj.0.weight'] == (E, 3, 3, 3)
    # the encoder keeps its own width: the LFS heads read the 28 * 16 = 448-wide representation
    assert dict((k, s) for k, s, _ in got)['E.E.encoder_q.uformer.input_proj.proj.0.weight'][0] == 28
    assert dict((k, s) for k, s, _ in got)['R.R.bottleneck_0.blocks.0.attn.mlp_head.1.0.weight'] == (448,)


@pytest.mark.parametrize('E', [16, 28, 48, 128])
def test_other_widths_are_refused_at_construction(E):
    from fwair.modules import DECODER_WIDTHS, UformerDecoder
    assert DECODER_WIDTHS == (32, 56, 64)
    with pytest.raises(NotImplementedError, match='32, 56, 64'):
        UformerDecoder(make_opt('all3', batch_size=1, embed_dim=E))
