"""CPU: the learner-step entries, dqz_learner_create and dqz_per_sample refuse
bad arguments before any device call and before any handle is dereferenced.

One table: each row is a call, the status it returns and a fragment of
dqz_last_error().  The handles are fake non-null addresses, so a row passes
only if the call fails on the named argument first."""

import ctypes

import pytest

INVALID = -1  # DQZ_ERR_INVALID


@pytest.fixture(scope='module')
def lib():
  import os  # pylint: disable=g-import-not-at-top
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  if not os.path.exists(_native.LIB_PATH):
    import __graft_entry__  # pylint: disable=g-import-not-at-top
    __graft_entry__._compile_lib()  # pylint: disable=protected-access
  return _native.lib()


_WORD = ctypes.c_int64(0)
P = ctypes.cast(ctypes.pointer(_WORD), ctypes.c_void_p)  # any non-null address
_PHASES = (ctypes.c_float * 16)()


def _draw(**kw):
  """A dqz_per_draw whose every pointer is set and whose numbers pass, then kw."""
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  d = _native.DqzPerDraw()
  for name, ctype in d._fields_:  # pylint: disable=protected-access
    if ctype is ctypes.c_void_p and name not in ('injected_uniform', 'injected_u', 'index_to_slot'):
      setattr(d, name, P.value)
  d.cap, d.live_base, d.size, d.capacity = 64, 0, 10, 64
  d.uniform_sample_probability, d.importance_sampling_exponent, d.alpha = 0.5, 0.5, 0.6
  for k, v in kw.items():
    setattr(d, k, v)
  return d


def _per_sample(**kw):
  """dqz_per_sample's arguments, all acceptable, then kw."""
  a = dict(tree=P, cap=64, live_base=0, size=10, capacity=64, n=4, usp=0.5, beta=0.5, normalize=1, seed=7,
           counter_dev=P, injected_uniform=None, injected_u=None, index_to_slot=None, out_indices=P, out_slots=P,
           out_weights=P, out_probs=P, stream=None)
  a.update(kw)
  return tuple(a.values())


def _rows():
  """(id, entry, arguments after (learner, params, store) or all of them, fragment)."""
  step = lambda learner, *rest: (learner, 'PARAMS', 'STORE') + rest
  rows = [
      ('step-null-learner', 'dqz_learner_step', step(None, P, None, None), 'null argument'),
      ('grad-null-learner', 'dqz_learner_grad', step(None, P, None, P, None), 'null argument'),
      ('grad-null-out', 'dqz_learner_grad', step(P, P, None, None, None), 'null grad_out'),
      ('profile-null-phases', 'dqz_learner_profile', step(None, P, None, 1, None, None), 'phase_ms must be non-null'),
      ('profile-no-iters', 'dqz_learner_profile', step(None, P, None, 0, _PHASES, None), 'iters >= 1'),
      # dqz_learner_step_per(L, P, S, slots, is_weights, tree, cap, indices, alpha, max_seen, stream)
      ('per-null-learner', 'dqz_learner_step_per', step(None, P, P, P, 64, P, 0.6, P, None), 'null argument'),
      ('per-null-tree', 'dqz_learner_step_per', step(P, P, P, None, 64, P, 0.6, P, None), 'null argument'),
      ('per-null-indices', 'dqz_learner_step_per', step(P, P, P, P, 64, None, 0.6, P, None), 'null argument'),
      ('per-null-max-seen', 'dqz_learner_step_per', step(P, P, P, P, 64, P, 0.6, None, None), 'null argument'),
      # dqz_learner_step_uniform(L, P, S, base, size, capacity, seed, counter, slots_out, stream); a null
      # learner, so L->cfg is never read
      ('uniform-null-counter', 'dqz_learner_step_uniform', step(None, 0, 10, 64, 7, None, P, None), 'null argument'),
      ('uniform-null-slots', 'dqz_learner_step_uniform', step(None, 0, 10, 64, 7, P, None, None), 'null argument'),
      ('uniform-empty', 'dqz_learner_step_uniform', step(None, 0, 0, 64, 7, P, P, None),
       'cannot sample from an empty replay (size=0)'),
      ('uniform-capacity', 'dqz_learner_step_uniform', step(None, 0, 10, 9, 7, P, P, None), 'bad replay geometry'),
      ('uniform-base', 'dqz_learner_step_uniform', step(None, -1, 10, 64, 7, P, P, None), 'bad replay geometry'),
      ('uniform-null-learner', 'dqz_learner_step_uniform', step(None, 0, 10, 64, 7, P, P, None), 'null argument'),
      # dqz_learner_step_logits(L, P, S, buf, logits, seed, counter, uniforms, slots_out, stream)
      ('logits-null-learner', 'dqz_learner_step_logits', step(None, P, P, 7, P, None, P, None), 'null argument'),
      ('logits-null-buffer', 'dqz_learner_step_logits', step(P, None, P, 7, P, None, P, None), 'null argument'),
      ('logits-null-logits', 'dqz_learner_step_logits', step(P, P, None, 7, P, None, P, None), 'null argument'),
      ('logits-null-slots', 'dqz_learner_step_logits', step(P, P, P, 7, P, None, None, None), 'null argument'),
      ('logits-no-uniform-source', 'dqz_learner_step_logits', step(P, P, P, 7, None, None, P, None), 'null argument'),
      # dqz_learner_step_per_draw(L, P, S, draw, stream)
      ('per-draw-null-learner', 'dqz_learner_step_per_draw', step(None, _draw(), None), 'null argument'),
      ('per-draw-null-draw', 'dqz_learner_step_per_draw', step(P, None, None), 'null argument'),
      ('per-draw-null-tree', 'dqz_learner_step_per_draw', step(P, _draw(tree=None), None), 'null argument'),
      ('per-draw-null-indices', 'dqz_learner_step_per_draw', step(P, _draw(out_indices=None), None), 'null argument'),
      ('per-draw-null-slots', 'dqz_learner_step_per_draw', step(P, _draw(out_slots=None), None), 'null argument'),
      ('per-draw-null-probs', 'dqz_learner_step_per_draw', step(P, _draw(out_probs=None), None), 'null argument'),
      ('per-draw-null-max-seen', 'dqz_learner_step_per_draw', step(P, _draw(max_seen_dev=None), None), 'null argument'),
      # dqz_learner_step_opt(L, P, S, slots, is_weights, optimizer, count, stream)
      ('opt-null-learner', 'dqz_learner_step_opt', step(None, P, None, P, P, None), 'null argument'),
      ('opt-null-optimizer', 'dqz_learner_step_opt', step(P, P, None, None, P, None), 'null argument'),
      ('opt-null-state', 'dqz_learner_step_opt', step(P, P, None, P, P, None), 'null optimizer state'),
      # dqz_learner_step_opt_uniform(L, P, S, base, size, capacity, seed, counter, slots_out, optimizer, count, stream)
      ('opt-uniform-null-learner', 'dqz_learner_step_opt_uniform', step(None, 0, 10, 64, 7, P, P, P, P, None),
       'null argument'),
      ('opt-uniform-null-optimizer', 'dqz_learner_step_opt_uniform', step(P, 0, 10, 64, 7, P, P, None, P, None),
       'null argument'),
      ('opt-uniform-null-state', 'dqz_learner_step_opt_uniform', step(P, 0, 10, 64, 7, P, P, P, P, None),
       'null optimizer state'),
      # dqz_learner_step_opt_per_draw(L, P, S, draw, optimizer, count, stream)
      ('opt-per-draw-null-learner', 'dqz_learner_step_opt_per_draw', step(None, _draw(), P, P, None), 'null argument'),
      ('opt-per-draw-null-optimizer', 'dqz_learner_step_opt_per_draw', step(P, _draw(), None, P, None),
       'null argument'),
      ('opt-per-draw-null-state', 'dqz_learner_step_opt_per_draw', step(P, None, P, P, None), 'null optimizer state'),
  ]
  sample = [
      ('null-tree', dict(tree=None), 'null argument'),
      ('null-slots', dict(out_slots=None), 'null argument'),
      ('null-weights', dict(out_weights=None), 'null argument'),
      ('no-counter', dict(counter_dev=None), 'Philox draws need counter_dev'),
      ('injected-u-alone', dict(injected_u=P), 'injected_uniform and injected_u go together'),
      ('injected-uniform-alone', dict(injected_uniform=P), 'injected_uniform and injected_u go together'),
      ('cap-below-capacity', dict(cap=32), 'cap must be a power of two >= capacity'),
      ('cap-not-a-power', dict(cap=96), 'cap must be a power of two >= capacity'),
      ('empty', dict(size=0), 'No IDs to sample.'),
      ('n-zero', dict(n=0), 'n must be in [1, 1024]'),
      ('n-large', dict(n=1025), 'n must be in [1, 1024]'),
      ('beta-high', dict(beta=1.5), 'Require 0 <= exponent <= 1.'),
      ('beta-nan', dict(beta=float('nan')), 'Require 0 <= exponent <= 1.'),
      ('usp-negative', dict(usp=-0.1), 'Require 0 <= uniform_sample_probability <= 1.'),
  ]
  rows += [('per-sample-' + name, 'dqz_per_sample', _per_sample(**kw), frag) for name, kw, frag in sample]
  # dqz_learner_create(config, out): the first value past each limit (batch 1 .. 256, 1 .. 32 actions), refused
  # before the first HIP call
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  handle = ctypes.c_void_p()
  create = lambda batch, a: (ctypes.byref(_native.DqzLearnerConfig(batch, a, 0, 2.5e-4, 0.95, 1e-5, 1.0 / 32)),
                             ctypes.byref(handle))
  rows += [('create-batch-zero', 'dqz_learner_create', create(0, 6), 'batch must be in [1, 256]'),
           ('create-batch-257', 'dqz_learner_create', create(257, 6), 'batch must be in [1, 256]'),
           ('create-no-actions', 'dqz_learner_create', create(256, 0), 'num_actions must be in [1, 32]'),
           ('create-33-actions', 'dqz_learner_create', create(1, 33), 'num_actions must be in [1, 32]')]
  return rows


_ROWS = _rows()


@pytest.mark.parametrize('entry,args,fragment', [r[1:] for r in _ROWS], ids=[r[0] for r in _ROWS])
def test_refused_before_any_device_call(lib, entry, args, fragment):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  params, store = _native.DqzParams(), _native.DqzStore()  # every pointer null
  named = {'PARAMS': ctypes.byref(params), 'STORE': ctypes.byref(store)}
  args = [named.get(a, a) if isinstance(a, str) else a for a in args]
  args = [ctypes.byref(a) if isinstance(a, _native.DqzPerDraw) else a for a in args]
  assert getattr(lib, entry)(*args) == INVALID
  assert fragment.encode() in lib.dqz_last_error()
