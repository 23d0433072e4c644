"""The backward launch's tail: conv2 dW's 16-byte dy2 loads and the chain
grid's order of the dW ranges.

In the chain grid conv2 dW (csrc/bwd.hpp conv2_bwd_dw_split<true>) reads its
sample's dy2 with 12 16-byte loads per lane and a 4 x 4 transpose inside each
quad of lanes in place of 42 four-byte loads, and its blocks are dispatched
ahead of the conv3-dW blocks; the block-range grid keeps the four-byte loads
and its order.  Neither changes a bit of any result, so at the smallest
shapes at which these bodies branch

  ('dqn', 2)   the smallest chain grid
  ('dqn', 5)   a partial group of 8
  ('dqn', 9)   a second group of 8 (one per XCD), padded and invalid samples
  ('per', 8)   with the fused priority write-back: the WB instantiation

(6 actions throughout) the tests hold

  * conv2's weight and bias gradients of a gradient call to the product of
    the device's own y1 and dy2 (Learner.fetch_activations), at the two bars
    of tests/layer_checks.py: every lane's 21 positions, the clamped tail
    positions 81..83 and both output-channel halves enter these sums;
  * the chain grid and the block-range grid (Learner.debug_backward: the
    transposed 16-byte loads against the four-byte ones) to the same bits in
    every output, parameter and moment after three carried steps, and two
    runs of one grid to the same bits (for 'per': with the
    write-back in the launch, the tree and the running maximum too, and the
    parameters equal those of the same steps without the write-back);
  * every hand-off word (Learner.debug_sync_words) to zero after eager steps,
    after a replayed graph of three steps and after profile mode, on both
    grids, with sync_status() 0.
"""

import types

import numpy as np
import pytest
import torch

from oracle import learner_ref
from tests import helpers
from tests import layer_checks as lc

pytestmark = pytest.mark.gpu

SHAPES = [('dqn', 2), ('dqn', 5), ('dqn', 9), ('per', 8)]
ACTIONS, CAPACITY, NUM_FRAMES, ALPHA = 6, 96, 260, 0.6


def _learner(algo, batch, seed, chain):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import networks
  net = (networks.dqn_atari_network(ACTIONS) if algo == 'dqn' else
         networks.double_dqn_atari_network(ACTIONS))
  online = net.init(seed)
  lrn = learner_lib.Learner(net, batch, algo=algo)
  lrn.set_params(online, helpers.perturbed_tree(online, seed + 1))
  assert lrn.debug_backward(chain) == chain
  return lrn


def _words_zero(lrn, what):
  words = lrn.debug_sync_words()
  assert words.size > 0 and words.dtype == np.int32
  bad = np.flatnonzero(words)
  assert bad.size == 0, '%s: non-zero hand-off ints at %s = %s' % (
      what, bad[:8].tolist(), words[bad[:8]].tolist())


@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: '%s-%d' % s)
def setup(request, device):
  """The shape's store, three batches of slots, the PER weights and a fresh
  sum tree per learner."""
  from dqn_mgsc_zoo_amd import replay as replay_lib
  from dqn_mgsc_zoo_amd import store as store_lib
  algo, batch = request.param
  frames, fidx, action, reward, discount = helpers.random_store_contents(
      CAPACITY, NUM_FRAMES, ACTIONS, 91 + batch)
  st = store_lib.FrameStore(CAPACITY, NUM_FRAMES)
  for name, arr in (('frames', frames), ('fidx', fidx), ('action', action),
                    ('reward', reward), ('discount', discount)):
    getattr(st, name).copy_(torch.from_numpy(arr))
  rng = np.random.default_rng(92 + batch)
  slots = [torch.from_numpy(rng.integers(0, CAPACITY, size=batch).astype(np.int32)).to(device)
           for _ in range(3)]
  weights, host = None, None
  if algo == 'per':
    slots[1][3] = slots[1][6]  # a repeated draw
    weights = torch.from_numpy(rng.uniform(0.2, 1.0, size=batch).astype(np.float32)).to(device)
    host = replay_lib.SumTree()
    host.set_all(rng.random(CAPACITY))

  def write_back():
    """(tree, max_seen, per-step keyword arguments) of one learner."""
    if host is None:
      return None, None, [{}, {}, {}]
    tree = torch.from_numpy(host.storage.copy()).to(device)
    seen = torch.tensor([0.5], dtype=torch.float64, device=device)
    return tree, seen, [dict(write_back=(tree, host.capacity, s, ALPHA, seen)) for s in slots]

  return types.SimpleNamespace(algo=algo, batch=batch, store=st, slots=slots, weights=weights,
                               write_back=write_back)


@pytest.mark.parametrize('chain', [1, 0], ids=['chain', 'ranges'])
def test_conv2_dw_from_the_devices_own_y1_and_dy2(setup, chain):
  lrn = _learner(setup.algo, setup.batch, 93, chain)
  grad = lrn.grad(setup.store, setup.slots[0], setup.weights)
  act = {k: v.cpu().numpy() for k, v in lrn.fetch_activations(0, backward=True).items()}
  assert lrn.sync_status() == 0
  g = lrn.network.unflatten(grad.cpu().numpy())[learner_ref.CONV_NAMES[1]]
  dy2 = act['dy2'].reshape(-1, act['dy2'].shape[-1])
  assert float(np.abs(dy2).max()) > 0.0 and bool(np.isfinite(dy2).all())
  # the last position of every sample (80: the only one of 80..83 that exists)
  assert float(np.abs(act['dy2'][:, 8, 8, :]).max()) > 0.0
  lc.report([
      ('conv2 dW', lc.product_check(g['w'].reshape(-1, g['w'].shape[-1]),
                                    lc.conv_cols(act['y1'], 1).T, dy2)),
      ('conv2 db', lc.product_check(g['b'], np.ones((1, dy2.shape[0])), dy2)),
  ])


def _state(lrn):
  torch.cuda.synchronize()
  assert lrn.sync_status() == 0
  out = {k: getattr(lrn, k).clone() for k in ('online', 'target', 'mu', 'nu')}
  q, td, loss = lrn.fetch_outputs()
  torch.cuda.synchronize()
  out.update(q_tm1=q.clone(), td=td.clone(), loss=loss.clone())
  return out


def test_grids_and_repeats_agree_bit_for_bit(setup):
  """Three carried steps, twice on each grid."""
  runs = []
  for chain in (1, 1, 0, 0):
    lrn = _learner(setup.algo, setup.batch, 95, chain)
    tree, seen, kw = setup.write_back()
    for s, k in zip(setup.slots, kw):
      lrn.step(setup.store, s, setup.weights, **k)
    state = _state(lrn)
    if tree is not None:
      state.update(tree=tree, max_seen=seen)
    _words_zero(lrn, 'three steps, chain = %d' % chain)
    runs.append(state)
  assert bool(torch.isfinite(runs[0]['online']).all())
  assert not torch.equal(runs[0]['online'], runs[0]['target'])
  for i, other in enumerate(runs[1:]):
    for k, v in runs[0].items():
      assert torch.equal(v, other[k]), (i + 1, k)
  if setup.algo == 'per':  # the same steps without the write-back in the launch
    lrn = _learner(setup.algo, setup.batch, 95, 1)
    for s in setup.slots:
      lrn.step(setup.store, s, setup.weights)
    plain = _state(lrn)
    for k, v in plain.items():
      assert torch.equal(v, runs[0][k]), ('no write-back', k)


@pytest.mark.parametrize('chain', [1, 0], ids=['chain', 'ranges'])
def test_hand_off_words_are_zero_after_every_kind_of_launch(setup, chain):
  lrn = _learner(setup.algo, setup.batch, 97, chain)
  _, _, kw = setup.write_back()
  _words_zero(lrn, 'a new learner')
  for s, k in zip(setup.slots, kw):
    lrn.step(setup.store, s, setup.weights, **k)
  _words_zero(lrn, 'three eager steps')
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for s, k in zip(setup.slots, kw):
      lrn.step(setup.store, s, setup.weights, **k)
  g.replay()
  g.replay()
  _words_zero(lrn, 'a graph of three steps replayed twice')
  lrn.profile(setup.store, setup.slots[0], setup.weights, iters=3)
  _words_zero(lrn, 'profile mode')
  assert lrn.sync_status() == 0
  assert bool(torch.isfinite(lrn.online).all())
