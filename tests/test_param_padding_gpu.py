"""GPU: the padding of the flat parameter layout neither changes a result nor
is changed ("padding is finite and inert").

param_layout rounds every leaf up to 64 floats, so the flat `online`,
`target`, `mu`, `nu` and gradient tensors hold floats that belong to no leaf,
between the leaves and after the last.  Two kernels read some of them on
purpose: c51_head_kernel's dz1 window and qr_dz1_kernel's 16-byte loads run
past the end of a W2 row, past the last row into the fc2 bias leaf and the
padding behind it, and multiply what they read by zero.  The optimizer
(opt_real, csrc/optim.hpp) and the update kernel skip padding on purpose.
Nothing else asserted that the padding stays out of every result, or that it
is left alone.

Each configuration below runs twice from the same state, once with every
padding float zero and once with every padding float of online, target, mu, nu
and of the gradient buffers holding a large finite sentinel (1e30: its square
overflows float32, so a norm or a moment that took it in would show).  Three
carried steps; before each step a gradient call into a buffer whose padding
holds the fill; after the steps, where the learner has an optimizer handle,
one dqz_optimizer_apply from that gradient buffer.  Then

  * every output, gradient leaf, grad_norm, step count and real parameter /
    moment of the two runs is bit-equal;
  * every padding float of online, target, mu and nu still holds its fill,
    bit for bit;
  * the padding of the gradient buffer still holds its fill: Learner.grad
    writes the leaves only and leaves the rest of `out` as the caller gave it
    (zeros in the buffer it allocates itself).

A finite-sentinel test: a NaN is never placed anywhere.  A padding float that
c51_head_kernel or qr_dz1_kernel reads and multiplies by zero is allowed by
the contract, and a NaN there would poison dz1 by design (NaN x 0 = NaN); the
contract is "finite", and create / set_params / the optimizer keep it so.

  scalar ('double', 5, 3)   clip + Adam; the fused centered RMSProp
  C51 (5, 3, 7)             clip + Adam (the head has no fused RMSProp)
  QR (4, 20, 201)           clip + Adam; A N = 4020: the last K group of
                            qr_dz1_kernel reads 12 floats past each W2 row
                            (past the last row: the fc2 bias leaf's first 12)
  C51 (2, 1, 2)             clip + Adam; the one action is the last: row 511's
                            dz1 window runs 12 floats past W2, over the
                            two-float bias leaf into 10 floats of padding
  QR (2, 1, 1)              clip + Adam; A N = 1: row 511's 16-byte loads run 15
                            floats past W2, over the one-float bias leaf into
                            14 floats of padding
The last two are the shapes at which the sentinel itself is read and multiplied
by zero; at the others the reads past a row end in the bias leaf.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 1.0e30
CONFIGS = ['scalar-clip_adam', 'scalar-fused_rmsprop', 'c51-clip_adam', 'qr-clip_adam', 'c51_small-clip_adam',
           'qr_small-clip_adam']


def _make(config, device):
  """(learner, store, device slots) of one configuration, from fixed seeds."""
  head, optimizer = config.split('-')
  if head == 'scalar':
    from tests import test_optimizers_gpu as og
    lrn, st, _, _, _ = og._setup('double', og._adam(clip=0.05) if optimizer == 'clip_adam' else None, 3,  # pylint: disable=protected-access
                                 batch=5, num_actions=3)
    slots = np.random.default_rng(5).integers(0, 256, size=5).astype(np.int32)
  else:
    if head.startswith('c51'):
      from tests import test_c51_gpu as hg
      case = hg._case(*((5, 3, 7) if head == 'c51' else (2, 1, 2)))  # pylint: disable=protected-access
    else:
      from tests import test_qr_gpu as hg
      case = hg._case(*((4, 20, 201) if head == 'qr' else (2, 1, 1)), hg.KAPPA)  # pylint: disable=protected-access
    lrn, st = hg._device(case, device, clip=0.05)  # pylint: disable=protected-access
    slots = case['slots']
  return lrn, st, torch.from_numpy(slots).to(device)


def _bits(t):
  return t.detach().cpu().numpy().reshape(-1).view(np.int32).copy()


def _run(config, device, fill):
  from dqn_mgsc_zoo_amd import _native
  lrn, st, slots = _make(config, device)
  offs, sizes, total = lrn.network.layout()
  real = np.zeros(total, bool)
  for o, s in zip(offs, sizes):
    real[o:o + s] = True
  assert (~real).sum() >= 32 and not real[offs[9] + sizes[9]:].any()
  pad = torch.from_numpy(~real).to(device)
  fill_bits = np.float32(fill).view(np.int32)
  state = dict(online=lrn.online, target=lrn.target, mu=lrn.mu, nu=lrn.nu)
  for t in state.values():
    assert not _bits(t)[~real].any()  # set_params and the constructor leave the padding zero
    t[pad] = fill
  record = []
  g = None
  for _ in range(3):
    g = torch.zeros_like(lrn.online)
    g[pad] = fill
    lrn.grad(st, slots, out=g)
    gb = _bits(g)
    assert (gb[~real] == fill_bits).all(), 'the gradient call wrote into the padding of its output'
    record.append(gb[real])
    lrn.step(st, slots)
    record += [_bits(x) for x in lrn.fetch_outputs()]
    if lrn._opt_h is not None:  # pylint: disable=protected-access
      record.append(_bits(lrn.grad_norm()))
    assert lrn.sync_status() == 0
  if lrn._opt_h is not None:  # pylint: disable=protected-access
    _native.check(_native.lib().dqz_optimizer_apply(
        lrn._opt_h, _native.ptr(lrn.online), _native.ptr(g), _native.ptr(lrn.mu),  # pylint: disable=protected-access
        _native.ptr(lrn.nu), _native.ptr(lrn.count), _native.stream_handle()))
    record.append(_bits(lrn.grad_norm()))
    assert (_bits(g)[~real] == fill_bits).all()
  torch.cuda.synchronize()
  record.append(_bits(lrn.count))
  for name, t in state.items():
    b = _bits(t)
    assert (b[~real] == fill_bits).all(), 'padding of %s changed' % name
    assert np.isfinite(b.view(np.float32)).all(), name
    record.append(b[real])
  return record


@pytest.mark.parametrize('config', CONFIGS)
def test_padding_neither_changes_a_result_nor_is_changed(device, config):
  zero = _run(config, device, 0.0)
  sentinel = _run(config, device, SENTINEL)
  assert len(zero) == len(sentinel)
  for i, (x, y) in enumerate(zip(zero, sentinel)):
    assert np.array_equal(x, y), (config, i, int((x != y).sum()))
  # the steps did something: the parameters moved, and the gradient is not all zeros
  lrn, _, _ = _make(config, device)
  offs, sizes, _ = lrn.network.layout()
  start = np.concatenate([_bits(lrn.online)[o:o + s] for o, s in zip(offs, sizes)])
  assert not np.array_equal(start, zero[-4]) and zero[0].any()
