"""GPU: the nonsense-transition MGSC agent and its two device entry points.

* dqz_logits_census against tests/nonsense_ref.py: min / max / count / probe
  sums and nums exact, mass within 1e-9 relative of numpy float64 (the term
  arguments are exact in float64; n 2^-53 ~ 1.2e-10 bounds the order
  difference of a non-negative sum at 2^20 terms), a repeated call
  bit-identical.  Capacity 8,269 = 2 * 4,096 + 77: three chunks, the last one
  ragged, windows wrapped and not.
* dqz_store_jumble against gather_stacks and a host composition: stacks byte
  for byte, scalars, flag, nothing else touched.
* replay_circular_nonsense.MGSCFiFoTransitionReplay reproduces the reference
  replay's log (tests/golden/nonsense_golden.json) add for add, with host
  items and with frame transitions in HBM.
* the agent through parts.run_loop, and a checkpoint round trip.
"""

import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import fake_env
from tests import nonsense_ref

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), 'golden',
                                     'nonsense_golden.json')))
LR, DECAY, EPS, BOUND = 2.5e-4, 0.95, 0.01 / 32**2, 1.0 / 32
CAP = 8269


# ---------------------------------------------------------------------------
# census


class _Buffer:
  """A dqz_logit_buffer handle with its logits and flags tensors."""

  def __init__(self, capacity, device):
    from dqn_mgsc_zoo_amd import _native
    self.n = _native
    self.h = ctypes.c_void_p()
    _native.check(_native.lib().dqz_logit_buffer_create(capacity, 4, ctypes.byref(self.h)))
    self.logits = torch.full((capacity,), -np.inf, dtype=torch.float32, device=device)
    self.flags = torch.zeros((capacity,), dtype=torch.uint8, device=device)

  def close(self):
    self.n.lib().dqz_logit_buffer_destroy(self.h)

  def load(self, logits, flags):
    self.logits.copy_(torch.from_numpy(logits))
    self.flags.copy_(torch.from_numpy(flags))

  def raw(self, left_head, size, acc):
    n = self.n
    return n.lib().dqz_logits_census(self.h, n.ptr(self.logits), n.ptr(self.flags), left_head, size,
                                     n.ptr(acc.tensor), n.stream_handle())

  def census(self, left_head, size, acc):
    self.n.check(self.raw(left_head, size, acc))


@pytest.fixture(scope='module')
def buf(device):
  b = _Buffer(CAP, device)
  yield b
  b.close()


def _acc(device):
  from dqn_mgsc_zoo_amd import replay_circular_nonsense as rcn
  return rcn.Census(device)


def _inputs(capacity, left_head, size, seed, flag_at=(), empty_class=False):
  """Logits 3 N(0,1) with a few at +-80 in the window; dead slots -inf, some
  of them flagged; flags random (or none), then `flag_at` = ((window position, flag), ...)."""
  rng = np.random.default_rng(seed)
  logits = (3 * rng.standard_normal(capacity)).astype(np.float32)
  flags = np.zeros(capacity, np.uint8) if empty_class else (rng.random(capacity) < 0.2).astype(np.uint8)
  live = (left_head + np.arange(size)) % capacity
  if size >= 8:
    logits[live[rng.choice(size, 4, replace=False)]] = np.float32([80, -80, 79.5, -80])
  for p, value in dict(flag_at).items():
    if p < size:
      flags[live[p]] = value
  dead = np.ones(capacity, bool)
  dead[live] = False
  logits[dead] = -np.inf
  flags[dead] = rng.integers(0, 2, int(dead.sum()))  # junk outside the window
  return logits, flags


def _check(got, want, mass_rtol=1e-9):
  assert got['calls'] == want['calls']
  for cls in nonsense_ref.CLASSES:
    g, w = got[cls], want[cls]
    assert np.float32(g['max']) == w['max'] and np.float32(g['min']) == w['min'], cls
    assert g['count'] == w['count'], cls
    for p in nonsense_ref.PROBES:
      assert g[p]['num'] == w[p]['num'], (cls, p)
      assert g[p]['sum'] == w[p]['sum'], (cls, p)  # float64, same adds in the same order
    print('%s mass device %.17g numpy %.17g' % (cls, g['mass'], w['mass']))
    np.testing.assert_allclose(g['mass'], w['mass'], rtol=mass_rtol, atol=0)


# window positions on both sides of the chunk boundaries, both classes on each side
BOUNDARIES = ((4094, 0), (4095, 1), (4096, 0), (4097, 1), (8190, 1), (8191, 0), (8192, 1), (8193, 0))


@pytest.mark.parametrize('left_head,size', [(8000, 5000), (100, 5000), (17, CAP), (0, CAP), (8268, 8200),
                                            (8000, 0), (8268, 1), (8268, 2), (8267, 4), (8266, 5), (3, 5)])
def test_census_one_call(device, buf, left_head, size):
  logits, flags = _inputs(CAP, left_head, size, seed=size + left_head, flag_at=BOUNDARIES)
  buf.load(logits, flags)
  acc = _acc(device)
  buf.census(left_head, size, acc)
  want = nonsense_ref.census(nonsense_ref.new_state(), logits, flags, left_head, size)
  _check(acc.as_dict(), want)
  if size == 1:  # only `exit` counts
    nums = {p: sum(want[c][p]['num'] for c in nonsense_ref.CLASSES) for p in nonsense_ref.PROBES}
    assert nums == {'entry': 0, '1st_quarter': 0, '2nd_quarter': 0, '3rd_quarter': 0, 'exit': 1}
  # equal inputs, equal bits
  again = _acc(device)
  buf.census(left_head, size, again)
  assert torch.equal(acc.tensor, again.tensor)


def test_census_class_without_a_member(device, buf):
  logits, flags = _inputs(CAP, 8000, 5000, seed=5, empty_class=True)
  buf.load(logits, flags)
  acc = _acc(device)
  buf.census(8000, 5000, acc)
  got = acc.as_dict()
  _check(got, nonsense_ref.census(nonsense_ref.new_state(), logits, flags, 8000, 5000))
  none = got['nonsense']
  assert none['min'] == np.inf and none['max'] == -np.inf and none['mass'] == 0 and none['count'] == 0
  assert got['real']['mass'] == 1.0 and got['real']['count'] == 5000


def test_census_running_fields_over_twenty_calls(device, buf):
  acc, want = _acc(device), nonsense_ref.new_state()
  rng = np.random.default_rng(9)
  for call in range(20):
    size = int(rng.integers(0, CAP + 1)) if call % 5 else (0, 1, 4, CAP)[call // 5]
    left_head = int(rng.integers(0, CAP))
    logits, flags = _inputs(CAP, left_head, size, seed=100 + call, empty_class=call == 7)
    buf.load(logits, flags)
    buf.census(left_head, size, acc)
    nonsense_ref.census(want, logits, flags, left_head, size)
  _check(acc.as_dict(), want)
  assert want['calls'] == 20


def test_census_at_a_million_slots(device):
  n = 1 << 20
  b = _Buffer(n, device)
  try:
    left_head, size = n - 12345, n - 7
    logits, flags = _inputs(n, left_head, size, seed=1, flag_at=BOUNDARIES)
    b.load(logits, flags)
    acc, again = _acc(device), _acc(device)
    b.census(left_head, size, acc)
    b.census(left_head, size, again)
    _check(acc.as_dict(), nonsense_ref.census(nonsense_ref.new_state(), logits, flags, left_head, size))
    assert torch.equal(acc.tensor, again.tensor)
  finally:
    b.close()


def test_census_refuses_bad_ranges(device, buf):
  acc = _acc(device)
  before = acc.tensor.clone()
  lib = buf.n.lib()
  assert buf.raw(CAP, 1, acc) == -1 and b'left_head' in lib.dqz_last_error()
  assert buf.raw(-1, 1, acc) == -1
  assert buf.raw(0, CAP + 1, acc) == -1 and b'size' in lib.dqz_last_error()
  assert buf.raw(0, -1, acc) == -1
  torch.cuda.synchronize()
  assert torch.equal(before, acc.tensor)


# ---------------------------------------------------------------------------
# jumble


def _filled_store(device, capacity=6, num_frames=40, seed=0):
  from dqn_mgsc_zoo_amd import store as store_lib
  rng = np.random.default_rng(seed)
  st = store_lib.FrameStore(capacity, num_frames, device=device)
  host = {
      'frames': rng.integers(0, 256, (num_frames, 84 * 84), dtype=np.uint8),
      # slot s uses rows 5 s .. 5 s + 4 (s_t shifted by one), inside rows 5 .. 34
      'fidx': np.stack([5 + 5 * s + np.array([0, 1, 2, 3, 1, 2, 3, 4]) for s in range(capacity)]).astype(np.int32),
      'action': rng.integers(0, 6, capacity).astype(np.int32),
      'reward': rng.standard_normal(capacity).astype(np.float32),
      'discount': rng.random(capacity).astype(np.float32),
  }
  host['fidx'][1, 2:4] = -1  # an episode start: trailing zero padding in s_tm1
  host['fidx'][1, 7] = -1
  host['fidx'][4, 4:8] = [20, -1, -1, -1]
  for k, v in host.items():
    getattr(st, k).copy_(torch.from_numpy(v))
  return st, host


def _host_stack(host, slot, which):
  out = np.zeros((84, 84, 4), np.uint8)
  for c in range(4):
    row = host['fidx'][slot, 4 * which + c]
    if row >= 0:
      out[..., c] = host['frames'][row].reshape(84, 84)
  return out


# fresh rows that wrap around the end of the 40-row pool
ROWS = [37, 38, 39, 0, 1, 2, 3, 4]


@pytest.mark.parametrize('slot,sources', [
    (5, (0, 3, 2, 4, 1)),   # s_t from a slot with padding, s_tm1 full
    (5, (1, 0, 0, 0, 4)),   # padding in both sources
    (0, (2, 2, 2, 2, 2)),   # all five the same slot (a replay of one item)
    (3, (3, 2, 0, 1, 4)),   # destination = the s_tm1 source (full ring)
    (4, (4, 4, 1, 1, 4)),   # destination = both stack sources
])
def test_jumble_against_host_composition(device, slot, sources):
  st, host = _filled_store(device)
  s0, sa, sr, sd, s1 = sources
  want_tm1, want_t = _host_stack(host, s0, 0), _host_stack(host, s1, 1)
  src_rows = list(host['fidx'][s0, :4]) + list(host['fidx'][s1, 4:])
  st.jumble(slot, s0, sa, sr, sd, s1, ROWS)
  sl = torch.tensor([slot], dtype=torch.int32, device=device)
  np.testing.assert_array_equal(st.gather_stacks(sl, 0).cpu().numpy()[0], want_tm1)
  np.testing.assert_array_equal(st.gather_stacks(sl, 1).cpu().numpy()[0], want_t)
  fidx = st.fidx.cpu().numpy()
  assert fidx[slot].tolist() == [ROWS[c] if src_rows[c] >= 0 else -1 for c in range(8)]
  assert int(st.action[slot]) == host['action'][sa]
  assert float(st.reward[slot]) == host['reward'][sr]
  assert float(st.discount[slot]) == host['discount'][sd]
  flags = st.flags.cpu().numpy()
  assert flags[slot] == 1 and flags.sum() == 1
  # nothing else moved: other slots, and every pool row but the copies
  others = [s for s in range(st.capacity) if s != slot]
  np.testing.assert_array_equal(fidx[others], host['fidx'][others])
  for name in ('action', 'reward', 'discount'):
    np.testing.assert_array_equal(getattr(st, name).cpu().numpy()[others], host[name][others])
  frames = st.frames.cpu().numpy()
  written = [ROWS[c] for c in range(8) if src_rows[c] >= 0]
  untouched = [r for r in range(st.num_frames) if r not in written]
  np.testing.assert_array_equal(frames[untouched], host['frames'][untouched])
  for c in range(8):
    if src_rows[c] >= 0:
      np.testing.assert_array_equal(frames[ROWS[c]], host['frames'][src_rows[c]])


# ---------------------------------------------------------------------------
# replay against the reference's log


def _scalar_item(rcn, i):
  return rcn.Transition(s_tm1=i, a_tm1=i % 4, r_t=0.5 * i, discount_t=0.99 - 0.01 * (i % 3), s_t=i + 1)


def _frame_of(v):
  """The stack standing for the golden's scalar state v: four distinct
  planes, the last one zero padding for every third v."""
  s = np.zeros((84, 84, 4), np.uint8)
  for c in range(4):
    s[..., c] = (7 * v + c) % 255 + 1
  if v % 3 == 0:
    s[..., 3] = 0
  s[v % 84, c, :3] += 1  # not constant planes
  return s


def _logits_match(got, want, exact):
  """As tests/test_samplers_gpu.py: the running log-sum-exp sums in another
  order (1e-6); exact mode gives the reference's float32 bits."""
  if exact:
    np.testing.assert_array_equal(np.asarray(got, np.float32), np.asarray(want, np.float32))
  else:
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize('frames,exact', [(False, False), (False, True), (True, False)])
def test_replay_reproduces_the_reference_log(device, frames, exact):
  from dqn_mgsc_zoo_amd import replay_circular_nonsense as rcn
  g = GOLDEN
  r = rcn.MGSCFiFoTransitionReplay(g['capacity'], rcn.Transition(None, None, None, None, None),
                                   np.random.default_rng(g['seed']), exact_sampling=exact)
  cache = {}
  for i, want in enumerate(g['steps']):
    jumbled = r._t % g['ratio'] == 0 and r._t > 0  # pylint: disable=protected-access
    assert jumbled == want['jumbled']
    if jumbled:
      size = r.size
      r.add_jumbled(0, size - 1, size // 4, size // 3, size // 2)
    else:
      item = _scalar_item(rcn, i)
      if frames:
        s_tm1 = cache.pop(i, None)
        s_tm1 = _frame_of(i) if s_tm1 is None else s_tm1
        cache[i + 1] = s_t = _frame_of(i + 1)  # the accumulator hands s_t back as the next s_tm1
        item = item._replace(s_tm1=s_tm1, s_t=s_t)
      r.add(item)
    if want['update'] is not None:
      r.update_priorities(np.asarray(want['update'][0]), np.asarray(want['update'][1], np.float32))
    assert r.size == want['size'] and r.left_head == want['left_head']
    assert r.is_nonsense.tolist() == want['is_nonsense']
    assert r.get_state()['storage']['is_nonsense'].tolist() == want['is_nonsense']
    got = r.stack_transitions(np.arange(r.size))
    items = np.array(want['items'])
    if frames:
      store = r.frame_store
      flags = (store.flags.cpu().numpy() if store.has_flags else np.zeros(g['capacity'], np.uint8))
      assert flags.astype(bool).tolist() == want['is_nonsense']
      np.testing.assert_array_equal(got.s_tm1.cpu().numpy(), np.stack([_frame_of(int(v)) for v in items[:, 0]]))
      np.testing.assert_array_equal(got.s_t.cpu().numpy(), np.stack([_frame_of(int(v)) for v in items[:, 4]]))
      fields = [got.a_tm1.cpu().numpy(), got.r_t.cpu().numpy(), got.discount_t.cpu().numpy()]
      np.testing.assert_array_equal(fields[1], items[:, 2].astype(np.float32))
      np.testing.assert_array_equal(fields[2], items[:, 3].astype(np.float32))
    else:
      np.testing.assert_array_equal(got.s_tm1, items[:, 0])
      np.testing.assert_array_equal(got.s_t, items[:, 4])
      fields = [got.a_tm1, got.r_t, got.discount_t]
      np.testing.assert_array_equal(fields[1], items[:, 2])
      np.testing.assert_array_equal(fields[2], items[:, 3])
    np.testing.assert_array_equal(fields[0], items[:, 1])
    live = (r.left_head + np.arange(r.size)) % g['capacity']
    _logits_match(r.device_logits.logits.cpu().numpy()[live], want['logits'], exact)
  assert r.check_valid()[0]


def test_small_pool_is_refused_not_overwritten(device):
  """Every second add jumbled needs 4.5 rows per add: 2 C + 64 rows run out
  and the allocator says so before anything is written."""
  from dqn_mgsc_zoo_amd import replay_circular_nonsense as rcn
  r = rcn.MGSCFiFoTransitionReplay(40, rcn.Transition(None, None, None, None, None), np.random.default_rng(0))
  with pytest.raises(RuntimeError, match='too small'):
    for i in range(200):
      if i % 2 == 0 and i > 0:
        t, size = r._t, r.size  # pylint: disable=protected-access
        try:
          r.add_jumbled(0, size - 1, size // 4, size // 3, size // 2)
        except RuntimeError:
          assert r._t == t and r.size == size  # pylint: disable=protected-access
          raise
      else:
        r.add(_scalar_item(rcn, i)._replace(s_tm1=_frame_of(i), s_t=_frame_of(i + 1)))


# ---------------------------------------------------------------------------
# agent


def _make(ratio, num_frames=None, seed=0, capacity=192):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import networks
  from dqn_mgsc_zoo_amd import parts
  from dqn_mgsc_zoo_amd import replay_circular_nonsense as rcn
  from dqn_mgsc_zoo_amd.dqn_mgsc_batched_nonsense_transitions import agent as agent_lib
  replay = rcn.MGSCFiFoTransitionReplay(
      capacity, rcn.Transition(None, None, None, None, None), np.random.default_rng(seed),
      num_frames=num_frames)
  agent = agent_lib.MGSCDqn(
      preprocessor=fake_env.FrameStacker(),
      sample_network_input=np.zeros((84, 84, 4), np.uint8),
      network=networks.dqn_atari_network(6),
      optimizer=learner_lib.rmsprop(LR, DECAY, EPS, centered=True),
      transition_accumulator=rcn.TransitionAccumulator(),
      replay=replay, batch_size=32,
      exploration_epsilon=parts.LinearSchedule(
          begin_t=40, decay_steps=200, begin_value=1.0, end_value=0.1),
      min_replay_capacity_fraction=0.25, learn_period=4,
      target_network_update_period=40, grad_error_bound=BOUND,
      rng_key=np.array([0, seed], np.uint32),
      meta_optimizer=learner_lib.adam(2.5e-4), meta_batch_size=16,
      nonsense_transition_ratio=ratio)
  return agent, replay


class _Shadow:
  """Host copies of what the replay should hold, by slot: real items as
  added, jumbled ones composed here from the copies."""

  def __init__(self, replay):
    from dqn_mgsc_zoo_amd import replay_circular_nonsense as rcn
    self.T = rcn.Transition
    self.replay = replay
    self.items, self.nonsense, self.jumbled_at = {}, {}, []
    self._add, self._jumble = replay.add, replay.add_jumbled
    replay.add, replay.add_jumbled = self.add, self.add_jumbled

  def add(self, item, nonsense=False):
    slot = self.replay._ring._right_head  # pylint: disable=protected-access
    self._add(item, nonsense)
    self.items[slot] = self.T(np.array(item.s_tm1), int(item.a_tm1), np.float32(item.r_t),
                              np.float32(item.discount_t), np.array(item.s_t))
    self.nonsense[slot] = False

  def add_jumbled(self, *relative):
    r = self.replay
    size = r.size
    assert relative == (0, size - 1, size // 4, size // 3, size // 2)
    src = [self.items[int(s)] for s in r._slots(list(relative))]  # pylint: disable=protected-access
    slot = r._ring._right_head  # pylint: disable=protected-access
    self.jumbled_at.append(r._t)  # pylint: disable=protected-access
    self._jumble(*relative)
    self.items[slot] = self.T(src[0].s_tm1, src[1].a_tm1, src[2].r_t, src[3].discount_t, src[4].s_t)
    self.nonsense[slot] = True


def _run(agent, num_steps, seed=1, episode_len=23):
  from dqn_mgsc_zoo_amd import parts
  env = fake_env.FakeAtari(episode_len=episode_len, seed=seed)
  loop = parts.run_loop(agent, env, max_steps_per_episode=0)
  for _ in range(num_steps):
    next(loop)


@pytest.mark.parametrize('ratio,num_frames', [(5, 640), (50, None)])
def test_agent_run_loop(device, ratio, num_frames):
  agent, replay = _make(ratio, num_frames)
  shadow = _Shadow(replay)
  ref = nonsense_ref.new_state()
  census = replay.census

  def spy(acc):  # the numpy walk over the device's own logits, then the device's
    store = replay.frame_store
    flags = store.flags.cpu().numpy() if store is not None else replay.is_nonsense
    nonsense_ref.census(ref, replay.device_logits.logits.cpu().numpy(), flags, replay.left_head, replay.size)
    census(acc)

  replay.census = spy
  p0 = agent.learner.online.clone()
  _run(agent, 300)
  assert agent.check_learner_health() == 0
  assert replay.size == replay.capacity and replay._t > replay.capacity  # pylint: disable=protected-access
  assert not torch.equal(p0, agent.learner.online) and torch.isfinite(agent.learner.online).all()
  assert agent.meta_learner.get_state()[0].count > 0
  # the schedule: add number t is jumbled iff t is a positive multiple of ratio
  t = replay._t  # pylint: disable=protected-access
  assert shadow.jumbled_at == list(range(ratio, t, ratio))
  live_t = range(t - replay.size, t)
  scheduled = sum(1 for k in live_t if k % ratio == 0)
  assert scheduled > 0
  want_flags = np.zeros(replay.capacity, bool)
  for k in live_t:
    want_flags[k % replay.capacity] = k % ratio == 0
  assert replay.is_nonsense.tolist() == want_flags.tolist()
  assert replay.frame_store.flags.cpu().numpy().astype(bool).tolist() == want_flags.tolist()
  # every stored transition, jumbled or real, bit for bit
  slots = replay._slots(np.arange(replay.size))  # pylint: disable=protected-access
  got = replay.stack_transitions(np.arange(replay.size))
  got = [x.cpu().numpy() for x in got]
  for k, slot in enumerate(slots):
    want = shadow.items[int(slot)]
    assert shadow.nonsense[int(slot)] == want_flags[slot]
    np.testing.assert_array_equal(got[0][k], want.s_tm1, err_msg=str(slot))
    np.testing.assert_array_equal(got[4][k], want.s_t, err_msg=str(slot))
    assert got[1][k] == want.a_tm1 and got[2][k] == want.r_t and got[3][k] == want.discount_t
  # the statistics: the numpy walk stepped on the same logits
  rows = agent.logit_value_stats()
  want_rows = nonsense_ref.stats_rows(ref)
  assert [r[0] for r in rows] == [r[0] for r in want_rows] and len(rows) == 17
  assert all(isinstance(r[2], str) and r[2] % r[1] for r in rows)
  for (name, value, _), (_, want) in zip(rows, want_rows):
    if name.endswith('_mass'):
      np.testing.assert_allclose(value, want, rtol=1e-9, atol=0, err_msg=name)
    else:
      assert value == want, name
  assert dict((r[0], r[1]) for r in rows)['nonsense_count'] == scheduled
  assert ref['calls'] == agent.census.read().calls > 0
  state = agent.get_state()
  lvt = state['logits_vs_time']
  assert set(lvt) == {'nonsense', 'real'}
  assert set(lvt['real']) == {'max', 'min', 'entry', '1st_quarter', '2nd_quarter', '3rd_quarter', 'exit'}
  assert set(lvt['real']['exit']) == {'sum', 'num'} and lvt['real']['exit']['num'] > 0


def _timesteps(n, seed, episode_len):
  env = fake_env.FakeAtari(episode_len=episode_len, seed=seed)
  steps = [env.reset()]
  for t in range(n - 1):
    steps.append(env.step(t % 6) if not steps[-1].last() else env.reset())
  return steps


def _drive(agent, steps):
  actions = []
  for ts in steps:
    if ts.first():
      agent.reset()
    actions.append(agent.step(ts))
  return actions


def test_checkpoint_round_trip_continues_bit_identically(device, tmp_path):
  """The shape of tests/test_checkpoint_gpu.py: save through
  parts.Checkpoint after the ring has wrapped, restore into a fresh agent
  with another seed, drive both with the same 60 frames."""
  from dqn_mgsc_zoo_amd import parts
  a1, r1 = _make(5, 640, seed=4)
  _drive(a1, _timesteps(230, 5, 19))
  assert r1.size == r1.capacity and r1.is_nonsense.any()
  ck = parts.Checkpoint(str(tmp_path / 'run.chkpt'))
  ck.state.train_agent = a1
  ck.save()
  a2, r2 = _make(5, 640, seed=99)
  ck2 = parts.Checkpoint(str(tmp_path / 'run.chkpt'))
  ck2.state.train_agent = a2
  assert ck2.can_be_restored()
  ck2.restore()
  assert a2.learner.online.data_ptr() != a1.learner.online.data_ptr()
  assert torch.equal(a1.census.tensor, a2.census.tensor)
  assert torch.equal(r1.frame_store.flags, r2.frame_store.flags)
  assert r1.is_nonsense.tolist() == r2.is_nonsense.tolist()

  more = _timesteps(60, 6, 17)
  assert _drive(a1, more) == _drive(a2, more)
  for which in ('online', 'target', 'mu', 'nu'):
    assert torch.equal(getattr(a1.learner, which), getattr(a2.learner, which)), which
  assert torch.equal(r1.device_logits.logits, r2.device_logits.logits)
  m1, m2 = a1.meta_learner.get_state()[0], a2.meta_learner.get_state()[0]
  assert m1.count == m2.count and m1.count > 0
  np.testing.assert_array_equal(m1.mu, m2.mu)
  np.testing.assert_array_equal(m1.nu, m2.nu)
  assert torch.equal(a1.census.tensor, a2.census.tensor)
  assert a1.logit_value_stats() == a2.logit_value_stats()
  assert torch.equal(r1.frame_store.flags, r2.frame_store.flags)
  assert r1.is_nonsense.tolist() == r2.is_nonsense.tolist() and r1.is_nonsense.any()
  live = np.arange(r1.size)
  for x, y in zip(r1.stack_transitions(live), r2.stack_transitions(live)):
    assert torch.equal(x, y)
  assert a1.check_learner_health() == 0 and a2.check_learner_health() == 0
