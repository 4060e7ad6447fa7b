"""Host protocol of the lazy split-K input gradient (fwair/functional.py: _ln_publish / _ln_consume / _ln_may_be_lazy / _ln_take), on
the CPU and without the HIP library: two stand-in autograd Functions use the real helpers the way LayerNormFn / LnResFn and
LinearFn / QKVFn do, under the real autograd engine.

  * a LayerNorm output counts the producers that take it as a differentiable input, at forward time;
  * the one consumer counted may leave its input gradient unwritten and attach the slab; the attribute arrives at the LayerNorm;
  * two counted consumers: nobody goes lazy;
  * a consumer the cell cannot see (any other op on the LayerNorm output) makes autograd SUM the gradients: the attribute is lost,
    and the LayerNorm backward raises instead of reading the unwritten buffer;
  * config.lazy_dgrad = False switches the whole thing off."""
import pytest
import torch

from fwair import functional as Fn

NAN = float('nan')


class Norm(torch.autograd.Function):
    """y = 2 x; stands in for the LayerNorm functions"""

    @staticmethod
    def forward(ctx, x):
        y = x * 2
        Fn._ln_publish(ctx, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = Fn._ln_take(ctx, dy)
        slab = getattr(dy, '_fw_slab', None)
        Norm.saw_slab.append(slab is not None)
        return 2 * (slab[0].sum(0) if slab is not None else dy)


class Producer(torch.autograd.Function):
    """y = 3 x; stands in for LinearFn / QKVFn: its input gradient is the sum of a two-slice slab"""

    @staticmethod
    def forward(ctx, x):
        Fn._ln_consume(ctx, x)
        return x * 3

    @staticmethod
    def backward(ctx, dy):
        slab = torch.stack([dy * 1, dy * 2])
        if Fn._ln_may_be_lazy(ctx):
            d = torch.full_like(dy, NAN)                  # "unwritten"
            d._fw_slab = (slab, 2, dy.numel())
            ctx.ln_cell[1] = True
            return d
        return slab.sum(0)


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    monkeypatch.setattr(Fn.config, 'lazy_dgrad', True)
    Norm.saw_slab = []


def leaf():
    return torch.arange(8, dtype=torch.float32).reshape(2, 4).requires_grad_(True)


def test_forward_publishes_a_cell_and_counts_differentiable_consumers():
    x = leaf()
    y = Norm.apply(x)
    assert y._fw_ln == [0, False]
    Producer.apply(y)
    assert y._fw_ln == [1, False]
    Producer.apply(y)
    assert y._fw_ln == [2, False]
    Producer.apply(y.detach())
    assert y._fw_ln == [2, False], 'a consumer that needs no input gradient was counted'
    z = Norm.apply(leaf().detach())
    Producer.apply(z)
    assert z._fw_ln == [0, False], 'the consumer of a LayerNorm output that needs no gradient was counted'


def test_single_consumer_goes_lazy_and_the_slab_arrives():
    x = leaf()
    y = Norm.apply(x)
    Producer.apply(y).sum().backward()
    assert Norm.saw_slab == [True] and y._fw_ln == [1, False]
    assert torch.equal(x.grad, torch.full((2, 4), 6.0))
    x.grad = None
    Fn.config.lazy_dgrad = False
    Producer.apply(Norm.apply(x)).sum().backward()
    assert Norm.saw_slab == [True, False]
    assert torch.equal(x.grad, torch.full((2, 4), 6.0))


def test_second_backward_through_a_kept_graph():
    x = leaf()
    out = Producer.apply(Norm.apply(x)).sum()
    out.backward(retain_graph=True)
    out.backward()
    assert Norm.saw_slab == [True, True]
    assert torch.equal(x.grad, torch.full((2, 4), 12.0))


def test_two_consumers_stay_eager():
    x = leaf()
    y = Norm.apply(x)
    (Producer.apply(y).sum() + Producer.apply(y).sum()).backward()
    assert Norm.saw_slab == [False]
    assert torch.equal(x.grad, torch.full((2, 4), 12.0))


def test_unseen_consumer_raises_instead_of_reading_the_unwritten_buffer():
    x = leaf()
    y = Norm.apply(x)
    loss = Producer.apply(y).sum() + (y * 5).sum()        # autograd sums the two gradients of y: the attribute cannot arrive
    with pytest.raises(RuntimeError, match='split-K slab'):
        loss.backward()
    assert Norm.saw_slab == []


def test_layernorm_without_a_lazy_producer_takes_any_gradient():
    x = leaf()
    y = Norm.apply(x)
    (y * 5).sum().backward()
    assert Norm.saw_slab == [False]
    assert torch.equal(x.grad, torch.full((2, 4), 10.0))
