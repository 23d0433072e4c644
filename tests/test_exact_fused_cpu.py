"""CPU: dqz_learner_step_logits_exact and Learner.step_logits(exact=True)
refuse bad arguments before any device call."""

import ctypes

import pytest


@pytest.fixture(scope='module')
def lib():
  import os  # pylint: disable=g-import-not-at-top
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  if not os.path.exists(_native.LIB_PATH):
    import __graft_entry__  # pylint: disable=g-import-not-at-top
    __graft_entry__._compile_lib()  # pylint: disable=protected-access
  return _native.lib()


def test_entry_is_declared_exported_and_bound(lib):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  assert 'dqz_learner_step_logits_exact' in _native.SIGNATURES
  assert (_native.SIGNATURES['dqz_learner_step_logits_exact'] ==
          _native.SIGNATURES['dqz_learner_step_logits'])
  assert lib.dqz_learner_step_logits_exact.argtypes is not None


def test_null_arguments_are_invalid(lib):
  """Null learner / buffer / logits / slots_out, and neither or both of
  counter_dev and uniforms: DQZ_ERR_INVALID with a message, no HIP call (the
  handles are never dereferenced: each call fails on its null first)."""
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  params, store = _native.DqzParams(), _native.DqzStore()
  word = ctypes.c_int64(0)
  p = ctypes.cast(ctypes.pointer(word), ctypes.c_void_p)  # any non-null address

  def call(learner=p, buf=p, logits=p, counter=p, uniforms=None, slots=p):
    return lib.dqz_learner_step_logits_exact(learner, ctypes.byref(params), ctypes.byref(store), buf,
                                             logits, 7, counter, uniforms, slots, None)

  for kw in (dict(learner=None), dict(buf=None), dict(logits=None), dict(slots=None)):
    assert call(**kw) == -1, kw
    assert b'null argument' in lib.dqz_last_error(), kw
    with pytest.raises(_native.NativeLibraryError, match='null argument'):
      _native.check(call(**kw))
  for kw in (dict(counter=None, uniforms=None), dict(counter=p, uniforms=p)):
    assert call(**kw) == -1, kw
    assert b'exactly one of counter_dev and uniforms' in lib.dqz_last_error(), kw


def test_step_logits_exact_wants_one_of_counter_and_uniforms():
  """Learner.step_logits raises before it touches the library."""
  import torch  # pylint: disable=g-import-not-at-top
  from dqn_mgsc_zoo_amd import learner as learner_lib  # pylint: disable=g-import-not-at-top
  lrn = object.__new__(learner_lib.Learner)  # no device: only the argument checks run
  lrn.batch_size = 4
  slots = torch.zeros((4,), dtype=torch.int32)
  u = torch.zeros((4,), dtype=torch.float64)
  c = torch.zeros((1,), dtype=torch.int64)
  with pytest.raises(ValueError, match='exactly one'):
    lrn.step_logits(None, None, slots, exact=True)
  with pytest.raises(ValueError, match='exactly one'):
    lrn.step_logits(None, None, slots, counter=c, uniforms=u, exact=True)
  with pytest.raises(ValueError, match='int32'):
    lrn.step_logits(None, None, slots.to(torch.int64), uniforms=u, exact=True)
