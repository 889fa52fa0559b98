"""The record that carries a gradient panel's row maxima from SplineFn.backward to the data gradient of the layer in front of it
(train_ops._attach_rowmax / _rowmax_for): it may hit only on the very tensor the spline backward wrote, unmodified since.  CPU tensors,
no GPU and no library needed."""
import torch

from flowcompare_amd import train_ops as T


def _panel(rows_pad=512, cols=64, rows=300):
    """A gradient panel as SplineFn.backward makes it (pad rows zeroed in place before the kernel call) with its record."""
    dparams = torch.empty(rows_pad, cols)
    dparams[rows:].zero_()
    dparams[:rows] = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows))
    rowmax = dparams.abs().amax(1)
    T._attach_rowmax(dparams, rowmax)
    return dparams, rowmax


def test_lookup_hits_on_direct_hand_over():
    dparams, rowmax = _panel()
    assert T._rowmax_for(dparams) is rowmax
    assert T._rowmax_for(dparams.contiguous()) is rowmax          # what the consumers call first: contiguous() of a contiguous tensor is the tensor


def test_lookup_misses_after_an_in_place_edit():
    dparams, _ = _panel()
    dparams.mul_(3.0)
    assert T._rowmax_for(dparams) is None
    dparams, _ = _panel()
    dparams[5, 7] = 1e6                                           # a write through a view counts too
    assert T._rowmax_for(dparams) is None


def test_lookup_misses_on_a_copy_another_shape_and_a_tensor_without_a_record():
    dparams, rowmax = _panel()
    assert T._rowmax_for(dparams.clone()) is None
    assert T._rowmax_for(dparams * 1.0) is None
    assert T._rowmax_for(dparams[:256]) is None                   # a view is another tensor object
    assert T._rowmax_for(torch.zeros(512, 64)) is None
    other = torch.zeros(256, 64)
    T._attach_rowmax(other, rowmax)                               # maxima of 512 rows beside a panel of 256
    assert T._rowmax_for(other) is None
    half = torch.zeros(512, 64, dtype=torch.float64)
    T._attach_rowmax(half, rowmax)
    assert T._rowmax_for(half) is None
    assert T._rowmax_for(dparams) is rowmax                       # none of this touched the original


class _Producer(torch.autograd.Function):
    """Stands in for SplineFn: its backward returns a fresh panel with a record."""

    @staticmethod
    def forward(ctx, p):
        return p.sum(1)

    @staticmethod
    def backward(ctx, g):
        dparams = g[:, None].expand(5, 8).contiguous()
        T._attach_rowmax(dparams, dparams.abs().amax(1))
        return dparams


class _Consumer(torch.autograd.Function):
    """Stands in for MlpFn: its backward looks the record up on the gradient it receives."""
    seen = []

    @staticmethod
    def forward(ctx, x):
        return x.repeat(1, 2)

    @staticmethod
    def backward(ctx, dy):
        _Consumer.seen.append(T._rowmax_for(dy.contiguous()))
        return dy[:, :4] + dy[:, 4:]


def _through_autograd(hook=None, second_user=False):
    _Consumer.seen.clear()
    x = torch.randn(5, 4, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    p = _Consumer.apply(x)
    if hook is not None:
        p.register_hook(hook)
    loss = _Producer.apply(p).sum()
    if second_user:
        loss = loss + (p * p).sum()
    loss.backward()
    (hit,) = _Consumer.seen
    return hit


def test_record_survives_autograd_only_on_the_untouched_gradient():
    """The record rides on the tensor object through torch's autograd engine: a gradient handed over directly arrives with it, one edited
    in place by a hook arrives with a newer version, one replaced by a hook or accumulated from two users arrives without a valid record."""
    assert _through_autograd() is not None
    assert _through_autograd(hook=lambda g: g.mul_(3.0)) is None
    assert _through_autograd(hook=lambda g: g * 3.0) is None
    assert _through_autograd(second_user=True) is None
