"""CPU: the host pieces of the nonsense-transition agent.

* tests/nonsense_ref.py: the vectorised census equals the literal
  slot-by-slot loop at sizes 0-9 (every collision of the five probes), with
  wrapped windows, dead slots holding junk and an empty class.
* store.FrameAllocator.reserve against a stub store: fresh rows, the
  overwrite check against the pre-pop oldest transition, `_recent` and the
  s_t hand-back untouched.
* dqz_store_jumble / dqz_logits_census refuse bad arguments before any HIP
  call (the census's range checks need a logit buffer: test_nonsense_gpu.py).
"""

import ctypes
import types

import numpy as np
import pytest

from tests import nonsense_ref


def _same(a, b):
  assert a['calls'] == b['calls']
  for cls in nonsense_ref.CLASSES:
    for key in ('max', 'min', 'count'):
      assert a[cls][key] == b[cls][key], (cls, key)
    np.testing.assert_allclose(a[cls]['mass'], b[cls]['mass'], rtol=1e-14, atol=0)
    for p in nonsense_ref.PROBES:
      assert a[cls][p] == b[cls][p], (cls, p)


@pytest.mark.parametrize('size', range(10))
def test_vectorised_census_equals_the_literal_walk(size):
  rng = np.random.default_rng(size)
  capacity = 11
  a, b = nonsense_ref.new_state(), nonsense_ref.new_state()
  for call in range(6):
    left = int(rng.integers(0, capacity))
    logits = (3 * rng.standard_normal(capacity)).astype(np.float32)
    flags = rng.integers(0, 2, capacity).astype(np.uint8)
    if call == 2:
      flags[:] = 0  # no nonsense item at all
    live = (left + np.arange(size)) % capacity
    dead = np.setdiff1d(np.arange(capacity), live)
    logits[dead] = -np.inf
    flags[dead] = 1  # junk outside the window is not looked at
    nonsense_ref.census(a, logits, flags, left, size)
    nonsense_ref.census_loop(b, logits, flags, left, size)
    _same(a, b)
  assert a['calls'] == 6


def test_probe_precedence():
  p = nonsense_ref.probe_positions
  assert p(0) == {}
  assert p(1) == {'exit': 0}
  assert p(2) == {'exit': 0, '2nd_quarter': 1}
  assert p(3) == {'exit': 0, '2nd_quarter': 1, 'entry': 2}
  assert p(4) == {'exit': 0, '3rd_quarter': 1, '2nd_quarter': 2, '1st_quarter': 3}
  assert p(5) == {'exit': 0, '3rd_quarter': 1, '2nd_quarter': 2, '1st_quarter': 3, 'entry': 4}
  assert p(8) == {'exit': 0, '3rd_quarter': 2, '2nd_quarter': 4, '1st_quarter': 6, 'entry': 7}


def _allocator(num_frames):
  from dqn_mgsc_zoo_amd import store as store_lib
  return store_lib.FrameAllocator(types.SimpleNamespace(num_frames=num_frames), 'ring')


def _stack(values):
  s = np.zeros((84, 84, 4), np.uint8)
  for c, v in enumerate(values):
    s[..., c] = v
  return s


def test_reserve_hands_out_fresh_rows_and_leaves_the_window_alone():
  alloc = _allocator(32)
  a, b = _stack([1, 2, 3, 4]), _stack([2, 3, 4, 5])
  fidx, new = alloc.allocate(0, a, b, None)
  assert fidx == [0, 1, 2, 3, 1, 2, 3, 4] and [r for r, _ in new] == [0, 1, 2, 3, 4]
  recent, prev = list(alloc._recent), alloc._prev  # pylint: disable=protected-access
  rows = alloc.reserve(1, 8, 0)
  assert rows == list(range(5, 13))
  assert alloc._min_ref[1] == 5 and alloc._min_ref[0] == 0  # pylint: disable=protected-access
  assert list(alloc._recent) == recent and alloc._prev is prev  # pylint: disable=protected-access
  # the next real transition still shares the frames placed before the reserve
  fidx, new = alloc.allocate(2, b, _stack([3, 4, 5, 6]), 0)
  assert fidx == [1, 2, 3, 4, 2, 3, 4, 13] and [r for r, _ in new] == [13]
  with pytest.raises(ValueError, match='frame ring'):
    from dqn_mgsc_zoo_amd import store as store_lib
    store_lib.FrameAllocator(types.SimpleNamespace(num_frames=32), 'slot').reserve(0, 8)


def test_reserve_refuses_rows_of_the_pre_pop_oldest():
  alloc = _allocator(12)
  alloc.allocate(0, _stack([1, 2, 3, 4]), _stack([2, 3, 4, 5]), None)  # rows 0..4
  alloc.allocate(1, _stack([2, 3, 4, 5]), _stack([3, 4, 5, 6]), 0)     # row 5
  assert alloc._pos == 6  # pylint: disable=protected-access
  # 8 rows from position 6 wrap onto rows 0 and 1, which slot 0 still needs
  with pytest.raises(RuntimeError, match='too small'):
    alloc.reserve(0, 8, 0)
  assert alloc._pos == 6 and alloc._min_ref[0] == 0  # pylint: disable=protected-access
  # with the post-pop oldest (slot 1, rows 1..5) the check would have passed
  # row 0 and stopped one row later: the protected slot matters
  with pytest.raises(RuntimeError, match='overwriting frame 1 '):
    alloc.reserve(0, 8, 1)
  # once slot 0 is gone and slot 1 is the oldest, 6 rows (6..11) fit
  alloc.forget(0)
  assert alloc.reserve(2, 6, 1) == [6, 7, 8, 9, 10, 11]
  assert alloc._min_ref[2] == 6  # pylint: disable=protected-access


@pytest.fixture(scope='module')
def lib():
  from dqn_mgsc_zoo_amd import _native
  return _native.lib()


def test_jumble_validation_without_a_gpu(lib):
  from dqn_mgsc_zoo_amd import _native
  store = _native.DqzStore(1, 1, 1, 1, 1, 10, 40)  # non-null, never dereferenced
  def call(**kw):
    j = _native.DqzJumble()
    j.slot, j.src_s_tm1, j.src_action, j.src_reward, j.src_discount, j.src_s_t = 3, 3, 9, 0, 1, 2
    for i in range(8):
      j.frame_rows[i] = 30 + i
    for k, v in kw.items():
      if k == 'rows':
        for i, r in v.items():
          j.frame_rows[i] = r
      else:
        setattr(j, k, v)
    return lib.dqz_store_jumble(ctypes.byref(store), ctypes.byref(j), None)
  assert call(slot=10) == -1 and b'out of range' in lib.dqz_last_error()
  assert call(slot=-1) == -1
  for field in ('src_s_tm1', 'src_action', 'src_reward', 'src_discount', 'src_s_t'):
    assert call(**{field: 10}) == -1, field
    assert call(**{field: -1}) == -1, field
  assert call(rows={7: 40}) == -1 and b'frame_rows[7]' in lib.dqz_last_error()
  assert call(rows={0: -1}) == -1
  assert call(rows={5: 31}) == -1 and b'repeats' in lib.dqz_last_error()
  assert lib.dqz_store_jumble(ctypes.byref(store), None, None) == -1
  assert lib.dqz_store_jumble(None, None, None) == -1


def test_census_validation_without_a_gpu(lib):
  """Without a device no logit buffer exists, so the refusals that can be
  seen here are the null ones; the range checks against a real buffer are in
  test_nonsense_gpu.py."""
  one = ctypes.c_void_p(1)
  assert lib.dqz_logits_census(None, one, one, 0, 0, one, None) == -1
  assert b'null' in lib.dqz_last_error()
  assert lib.dqz_logits_census(None, None, None, -1, -1, None, None) == -1
