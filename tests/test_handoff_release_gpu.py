"""The in-launch hand-offs acknowledge off the critical path and still reset.

A consumer block of a hand-off (csrc/common.hpp Handoff) polls the sample's
arrival word, and later in its body counts itself on the acknowledgement word
(release_issue); the last consumer of the sample resets both words
(release_finish).  Every launch therefore has to leave every word at zero:
graph replays and profile mode's repeated launches start from what the launch
before left.  dqz_learner_debug_sync_words (Learner.debug_sync_words) reads
the words back, the error word included, and the tests here require all of
them to be zero after eager steps, graph replays and profile mode, on both
backward grids, for batches that take the block ranges (1), the smallest
chain (2), padded samples beside valid ones (9) and the step's own shape
(32); and the outputs of eager steps to equal those of a graph replay bit for
bit.  The give-up path of a wait has its own test (test_learner_gpu.py's stall
hook).
"""

import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

CAPACITY, NUM_FRAMES = 2048, 1024


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
def host_store():
  return helpers.random_store_contents(CAPACITY, NUM_FRAMES, 6, 81)


@pytest.fixture(scope='module')
def store(device, host_store):
  from dqn_mgsc_zoo_amd import store as store_lib
  frames, fidx, action, reward, discount = host_store
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


def _assert_words_zero(lrn, what):
  words = lrn.debug_sync_words()
  assert words.size > 0 and words.dtype == np.int32
  bad = np.flatnonzero(words)
  assert bad.size == 0, '%s: non-zero hand-off ints at %s = %s' % (
      what, bad[:8].tolist(), words[bad[:8]].tolist())


@pytest.mark.parametrize('algo,batch', [
    ('dqn', 1),       # the block ranges
    ('dqn', 2),       # the smallest chain batch
    ('dqn', 9),       # padded to 16: invalid jobs beside valid ones
    ('dqn', 32),      # the step's own shape
    ('double', 1),    # Z = 3
    ('double', 2),
    ('double', 9),
    ('double', 32),
    ('per', 9),       # with the fused write-back (8 leading workgroups)
])
def test_words_are_zero_after_every_kind_of_launch(device, store, algo, batch):
  """One step, three eager steps, a graph of three steps replayed twice and
  profile mode's three launches each leave every hand-off int, the error
  word included, at zero."""
  lrn = _learner(algo, batch, 83)
  rng = np.random.default_rng(84)
  s = [_slots(rng, batch, device) for _ in range(3)]
  w, kw = None, [{}, {}, {}]
  if algo == 'per':
    from dqn_mgsc_zoo_amd import replay as replay_lib
    host = replay_lib.SumTree()
    host.set_all(rng.random(CAPACITY))
    tree = torch.from_numpy(host.storage.copy()).to(device)
    seen = torch.tensor([0.5], dtype=torch.float64, device=device)
    w = torch.rand((batch,), device=device) + 0.5
    kw = [dict(write_back=(tree, host.capacity, x, 0.6, seen)) for x in s]
  _assert_words_zero(lrn, 'a new learner')
  lrn.step(store, s[0], w, **kw[0])
  _assert_words_zero(lrn, 'one step')
  for i in range(3):
    lrn.step(store, s[i], w, **kw[i])
  _assert_words_zero(lrn, 'three eager steps')
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for i in range(3):
      lrn.step(store, s[i], w, **kw[i])
  g.replay()
  g.replay()
  _assert_words_zero(lrn, 'a graph of three steps replayed twice')
  lrn.profile(store, s[0], w, iters=3)
  _assert_words_zero(lrn, 'profile mode')
  assert lrn.sync_status() == 0
  assert bool(torch.isfinite(lrn.online).all())


@pytest.mark.parametrize('chain', [0, 1])
@pytest.mark.parametrize('batch', [2, 9])
def test_eager_steps_equal_one_graph_replay(device, store, batch, chain):
  """The same three steps from the same state, eager and as one graph replay,
  on either backward grid: outputs, parameters and moments equal bit for bit."""
  eager, graph = _learner('dqn', batch, 85), _learner('dqn', batch, 85)
  assert eager.debug_backward(chain) == chain
  assert graph.debug_backward(chain) == chain
  rng = np.random.default_rng(86)
  s = [_slots(rng, batch, device) for _ in range(3)]
  for x in s:
    eager.step(store, x)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for x in s:
      graph.step(store, x)
  g.replay()
  torch.cuda.synchronize()
  _assert_words_zero(eager, 'eager')
  _assert_words_zero(graph, 'graph')
  assert eager.sync_status() == 0 and graph.sync_status() == 0
  for which in ('online', 'target', 'mu', 'nu'):
    assert torch.equal(getattr(eager, which), getattr(graph, which)), which
  qa, tda, la = (t.clone() for t in eager.fetch_outputs())
  qb, tdb, lb = graph.fetch_outputs()
  torch.cuda.synchronize()
  assert torch.equal(qa, qb), 'q_tm1'
  assert torch.equal(tda, tdb), 'td'
  assert torch.equal(la, lb), 'loss'
  assert bool(torch.isfinite(qa).all()) and bool(torch.isfinite(la).all())


@pytest.mark.parametrize('n', [1, 2])
def test_actor_forward_repeats_and_resets(device, host_store, n):
  """The forward launch with 8 conv2 / conv3 jobs per sample (the actor's):
  a second call returns the first call's bits, and the words are zero."""
  lrn = _learner('dqn', 2, 87)
  frames, fidx = host_store[0], host_store[1]
  states = torch.from_numpy(
      helpers.stacks_from(frames, fidx, [5, 11][:n], 0)).to(device)
  q1 = lrn.q_values(states).clone()
  _assert_words_zero(lrn, 'first forward')
  q2 = lrn.q_values(states)
  torch.cuda.synchronize()
  _assert_words_zero(lrn, 'second forward')
  assert q1.shape == (n, 6) and bool(torch.isfinite(q1).all())
  assert float(q1.abs().max()) > 0.0
  assert torch.equal(q1, q2)
