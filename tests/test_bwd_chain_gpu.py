"""The backward launch's two grids compute the same bits.

bwd_bc_kernel runs the dX chain (conv3 dX -> conv2 dX -> conv1 dW) either as
three block ranges of one grid or, for batches of at most 64 samples, in
resident chain workgroups that carry one job through all three stages
(Learner.debug_backward, dqz_learner_debug_backward).  Job bodies,
accumulation orders and the hand-off protocol are the same, so two learners
from the same seed, one forced to each grid, must agree bit for bit
(torch.equal, no tolerance) and leave the health word at 0.
"""

import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

CAPACITY, NUM_FRAMES = 2048, 1024  # a synthetic store of a few thousand slots


def _learner(algo, batch, seed):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import networks
  net = (networks.dqn_atari_network(6) if algo == 'dqn' else
         networks.double_dqn_atari_network(6))
  online = net.init(seed)
  lrn = learner_lib.Learner(net, batch, algo=algo)
  lrn.set_params(online, helpers.perturbed_tree(online, seed + 1))
  return lrn


@pytest.fixture(scope='module')
def store(device):
  from dqn_mgsc_zoo_amd import store as store_lib
  frames, fidx, action, reward, discount = helpers.random_store_contents(
      CAPACITY, NUM_FRAMES, 6, 73)
  st = store_lib.FrameStore(CAPACITY, NUM_FRAMES)
  st.frames.copy_(torch.from_numpy(frames))
  st.fidx.copy_(torch.from_numpy(fidx))
  st.action.copy_(torch.from_numpy(action))
  st.reward.copy_(torch.from_numpy(reward))
  st.discount.copy_(torch.from_numpy(discount))
  return st


def _slots(rng, batch, device):
  return torch.from_numpy(
      rng.integers(0, CAPACITY, size=batch).astype(np.int32)).to(device)


def _assert_same(a, b):
  torch.cuda.synchronize()
  assert a.sync_status() == 0 and b.sync_status() == 0
  for which in ('online', 'mu', 'nu'):
    assert torch.equal(getattr(a, which), getattr(b, which)), which
  qa, tda, la = (t.clone() for t in a.fetch_outputs())
  qb, tdb, lb = b.fetch_outputs()
  torch.cuda.synchronize()
  assert torch.equal(tda, tdb), 'td'
  assert torch.equal(qa, qb), 'q_tm1'
  assert torch.equal(la, lb), 'loss'


@pytest.mark.parametrize('algo,batch', [
    ('dqn', 1),      # one sample, one 8-block group
    ('dqn', 9),      # B8 = 16: a group with seven padded samples, whose blocks exit
    ('dqn', 32),     # the step's own shape
    ('dqn', 33),     # padded sample count
    ('dqn', 64),     # the largest chained batch
    ('double', 32),  # Z = 3
])
def test_chain_equals_block_ranges(device, store, algo, batch):
  """Three carried steps on each grid: parameters, moments and outputs equal."""
  ranges, chain = _learner(algo, batch, 61), _learner(algo, batch, 61)
  assert ranges.debug_backward(0) == 0
  assert chain.debug_backward(1) == 1
  rng = np.random.default_rng(62)
  for _ in range(3):
    s = _slots(rng, batch, device)
    ranges.step(store, s)
    chain.step(store, s)
  _assert_same(ranges, chain)
  # the default: the chain for 2 <= B <= 64
  assert chain.debug_backward(-1) == (1 if batch > 1 else 0)


def test_chain_with_fused_per_write_back(device, store):
  """The WB grid (8 leading workgroups in front of the chain blocks): the sum
  tree and the running max agree too."""
  from dqn_mgsc_zoo_amd import replay as replay_lib
  batch, alpha = 32, 0.6
  ranges, chain = _learner('per', batch, 63), _learner('per', batch, 63)
  assert ranges.debug_backward(0) == 0
  assert chain.debug_backward(1) == 1
  rng = np.random.default_rng(64)
  host = replay_lib.SumTree()
  host.set_all(rng.random(CAPACITY))
  ta = torch.from_numpy(host.storage.copy()).to(device)
  tb = ta.clone()
  ma = torch.tensor([0.5], dtype=torch.float64, device=device)
  mb = ma.clone()
  w = torch.rand((batch,), device=device) + 0.5
  for _ in range(3):
    s = _slots(rng, batch, device)
    s[3] = s[17]  # a repeated draw
    ranges.step(store, s, w, write_back=(ta, host.capacity, s, alpha, ma))
    chain.step(store, s, w, write_back=(tb, host.capacity, s, alpha, mb))
  _assert_same(ranges, chain)
  assert torch.equal(ta, tb) and torch.equal(ma, mb)


def test_chain_under_graph_replay_and_profile(device, store):
  """A graph of three chained steps replayed twice equals six eager steps on
  the block ranges from the same state, and after profile mode's back-to-back
  launches the hand-off words are still clean (they reset themselves)."""
  batch = 32
  ranges, chain = _learner('dqn', batch, 65), _learner('dqn', batch, 65)
  assert ranges.debug_backward(0) == 0
  assert chain.debug_backward(1) == 1
  rng = np.random.default_rng(66)
  s = _slots(rng, batch, device)
  side = torch.cuda.Stream(device)
  side.wait_stream(torch.cuda.current_stream(device))
  with torch.cuda.stream(side):
    chain.step(store, s)  # the first launches happen outside the capture
  torch.cuda.current_stream(device).wait_stream(side)
  ranges.step(store, s)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(3):
      chain.step(store, s)
  for _ in range(2):
    g.replay()
  for _ in range(6):
    ranges.step(store, s)
  _assert_same(ranges, chain)
  chain.profile(store, s, iters=5)
  torch.cuda.synchronize()
  assert chain.sync_status() == 0


def test_large_batch_keeps_the_block_ranges(device, store):
  """B = 72 > 64: the chain is not legal, `active` says so, and the step still
  matches the learner forced to the block ranges."""
  batch = 72
  ranges, asked = _learner('dqn', batch, 67), _learner('dqn', batch, 67)
  assert ranges.debug_backward(0) == 0
  assert asked.debug_backward(1) == 0
  assert asked.debug_backward(-1) == 0
  assert asked.debug_backward(1) == 0
  rng = np.random.default_rng(68)
  for _ in range(3):
    s = _slots(rng, batch, device)
    ranges.step(store, s)
    asked.step(store, s)
  _assert_same(ranges, asked)
