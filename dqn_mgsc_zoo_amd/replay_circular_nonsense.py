"""`dqn_zoo/replay_circular_nonsense.py`: the MGSC FIFO replay that also
remembers which of its items are nonsense transitions.

The reference differs from `replay_circular.py` in one place: its
`CircularBuffer` keeps `_is_nonsense`, a bool per absolute slot written by
every add (replay_circular_nonsense.py:97-110), and
`MGSCFiFoTransitionReplay.add(item, nonsense=False)` passes it through
(:1086-1097).  The agent composes each nonsense item from five stored ones
(dqn_mgsc_batched_nonsense_transitions/agent.py:277-286) and walks the
whole buffer after every timestep (:290-310).  Here:

* `add_jumbled` composes the item where it is stored: on device for frame
  transitions (FrameStore.jumble, one launch, no host copy of the stacks),
  on the host for host-stored items;
* the flags live twice: a host mirror `is_nonsense` (the reference's list)
  and, for frame transitions, the store's device `flags`, which the census
  kernel reads.  A reused slot's device flag is cleared only when the mirror
  says it was set, so an ordinary add costs no extra launch;
* `census(acc)` is the agent's walk as one device reduction
  (dqz_logits_census) into a `Census` accumulator; nothing synchronises
  until somebody reads it.
"""

import ctypes
from typing import Any, Mapping

import numpy as np

from dqn_mgsc_zoo_amd import replay as replay_lib
from dqn_mgsc_zoo_amd import replay_circular
from dqn_mgsc_zoo_amd.replay_circular import *  # pylint: disable=wildcard-import,unused-wildcard-import
from dqn_mgsc_zoo_amd.replay_circular import _torch

CLASSES = ('real', 'nonsense')  # dqz_census.cls[0], cls[1]


class Census:
  """A dqz_census in device memory: the running statistics of the learned
  logits by class.  `read()` copies it to the host (synchronises)."""

  def __init__(self, device='cuda'):
    from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
    self._native = _native
    torch = _torch()
    self._dev = torch.zeros((ctypes.sizeof(_native.DqzCensus),), dtype=torch.uint8,
                            device=torch.device(device))
    self.write(self.initial())

  def initial(self):
    c = self._native.DqzCensus()
    for k in range(2):
      c.cls[k].max_seen = -np.inf
      c.cls[k].min_seen = np.inf
    return c

  @property
  def tensor(self):
    return self._dev

  def read(self):
    raw = self._dev.cpu().numpy().tobytes()
    return self._native.DqzCensus.from_buffer_copy(raw)

  def write(self, c) -> None:
    host = np.frombuffer(bytes(c), np.uint8).copy()
    self._dev.copy_(_torch().from_numpy(host))

  def as_dict(self) -> Mapping[str, Any]:
    """The reference's `_logits_vs_time` (agent.py:81-122) plus, per class,
    this call's `count` and `mass`, and `calls`."""
    c = self.read()
    out = {}
    for k, name in enumerate(CLASSES):
      cls = c.cls[k]
      d = {'max': float(cls.max_seen), 'min': float(cls.min_seen)}
      for p, probe in enumerate(self._native.CENSUS_PROBES):
        d[probe] = {'sum': float(cls.probe_sum[p]), 'num': int(cls.probe_num[p])}
      d['count'] = int(cls.count)
      d['mass'] = float(cls.mass)
      out[name] = d
    out['calls'] = int(c.calls)
    return out

  def load_dict(self, state: Mapping[str, Any]) -> None:
    c = self.initial()
    for k, name in enumerate(CLASSES):
      d, cls = state[name], c.cls[k]
      cls.max_seen, cls.min_seen = d['max'], d['min']
      for p, probe in enumerate(self._native.CENSUS_PROBES):
        cls.probe_sum[p] = d[probe]['sum']
        cls.probe_num[p] = d[probe]['num']
      cls.count = d.get('count', 0)
      cls.mass = d.get('mass', 0.0)
    c.calls = state.get('calls', 0)
    self.write(c)


class _SlotStorage(replay_circular._SlotStorage):  # pylint: disable=protected-access
  """Item storage with a chosen frame-pool size and device-side composition."""

  def __init__(self, capacity, mode, device, num_frames=None):
    super().__init__(capacity, mode, device)
    self._num_frames = num_frames

  def _make(self, use_device):
    if use_device:
      return replay_lib._DeviceStorage(  # pylint: disable=protected-access
          self._capacity, self._mode, self._num_frames, self._device)
    return super()._make(False)

  def reserve(self, slot, oldest_live_slot):
    """Eight fresh pool rows owned by `slot` (FrameAllocator.reserve)."""
    nf = self._backend.store.num_frames
    return [p % nf for p in self._backend.allocator.reserve(slot, 8, oldest_live_slot)]

  def host_item(self, slot):
    return self._backend.get(slot)


class MGSCFiFoTransitionReplay(replay_circular.MGSCFiFoTransitionReplay):
  """The MGSC FIFO replay with nonsense flags (:1064-1162)."""

  def __init__(self, capacity: int, structure, random_state: np.random.Generator,
               encoder=None, decoder=None, device='cuda', exact_sampling=False,
               num_frames=None):
    """num_frames: frame-pool rows.  A jumbled add takes eight fresh rows, so
    the default 2 * capacity + 64 holds a stream in which at most every
    eighth add is jumbled; give more for a smaller ratio (the allocator
    raises when the pool is too small)."""
    super().__init__(capacity, structure, random_state, encoder, decoder, device,
                     exact_sampling)
    self._items = _SlotStorage(capacity, 'ring', device, num_frames)
    self._is_nonsense = np.zeros((capacity,), np.bool_)

  @property
  def is_nonsense(self) -> np.ndarray:
    """Host mirror of the flags, by absolute slot (the reference's
    `_storage._is_nonsense`)."""
    return self._is_nonsense

  @property
  def left_head(self) -> int:
    return self._ring._left_head  # pylint: disable=protected-access

  def add(self, item, nonsense: bool = False) -> None:
    """Adds a host item; `nonsense` only labels it (:1086-1097)."""
    slot = self._ring._right_head  # pylint: disable=protected-access
    super().add(item)
    nonsense = bool(nonsense)
    store = self.frame_store
    if store is not None and self._is_nonsense[slot] != nonsense:
      store.set_flag(slot, nonsense)
    self._is_nonsense[slot] = nonsense

  def add_jumbled(self, s_tm1_from: int, a_tm1_from: int, r_t_from: int,
                  discount_t_from: int, s_t_from: int) -> None:
    """Adds the transition whose five fields are those of five stored items,
    given by relative index into the ring as it is before this add pops
    anything (agent.py:277-286), flagged nonsense."""
    relative = [int(i) for i in (s_tm1_from, a_tm1_from, r_t_from, discount_t_from, s_t_from)]
    size = self._ring.size
    if size == 0:
      raise BufferError('Buffer is empty: nothing to compose a transition from.')
    if min(relative) < 0 or max(relative) >= size:
      raise KeyError('Buffer is not large enough to index at positions %s. '
                     'Must be in [0,%d).' % (relative, size))
    sources = [int(s) for s in self._slots(relative)]
    slot = self._ring._right_head  # pylint: disable=protected-access
    on_device = self._items.on_device
    if on_device:
      # the oldest live item is a source (on a full ring it is also the slot
      # written), so the rows are claimed while it still protects its frames;
      # reserve() then makes `slot` the owner of the fresh rows
      rows = self._items.reserve(slot, self._ring[0])
    else:
      parts = [self._items.host_item(s) for s in sources]
      item = parts[0]._replace(a_tm1=parts[1].a_tm1, r_t=parts[2].r_t,
                               discount_t=parts[3].discount_t, s_t=parts[4].s_t)
    if self._ring.is_full():
      self._distribution.popleft(return_value=False)
      popped = self._ring.popleft()
      if not on_device:
        self._items.drop(popped)
    self._distribution.add()
    if on_device:
      self.frame_store.jumble(slot, *sources, rows)
    else:
      self._items.put(slot, item)
    self._ring.add(slot)
    self._is_nonsense[slot] = True
    self._t += 1

  def census(self, acc: Census) -> None:
    """One pass of the agent's walk over the live logits (agent.py:290-310)
    into `acc`, on device; no host synchronisation."""
    from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
    dl = self.device_logits
    store = self.frame_store
    if store is not None:
      flags = store.flags
    else:  # host-stored items: the mirror is the only copy
      flags = _torch().from_numpy(self._is_nonsense.view(np.uint8).copy()).to(dl.device)
    _native.check(_native.lib().dqz_logits_census(
        dl.handle, _native.ptr(dl.logits), _native.ptr(flags), int(self.left_head),
        int(self._ring.size), _native.ptr(acc.tensor), _native.stream_handle()))

  def get_state(self) -> Mapping[str, Any]:
    state = dict(super().get_state())
    state['storage'] = dict(state['storage'], is_nonsense=self._is_nonsense.copy())
    return state

  def set_state(self, state: Mapping[str, Any]) -> None:
    super().set_state(state)
    flags = state['storage'].get('is_nonsense')
    self._is_nonsense = (np.zeros((self._capacity,), np.bool_) if flags is None
                         else np.array(flags, np.bool_))
