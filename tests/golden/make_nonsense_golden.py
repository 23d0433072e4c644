"""Generates tests/golden/nonsense_golden.json from the REFERENCE's
`dqn_zoo/replay_circular_nonsense.py`.

Runs only where the reference checkout exists (never on the GPU box: the JSON
output is committed).  The module imports jax, snappy, dm_env and
dqn_zoo.parts at top level but does not use them on the numpy code paths
exercised here, so those names are stubbed in sys.modules, as
make_golden.py does.  Nothing from the reference is copied: this script only
records inputs and the reference's outputs.

One MGSCFiFoTransitionReplay of capacity 7 receives 30 adds (more than four
wraps).  Every add whose count `_t` is a positive multiple of 5 is a jumbled
transition, composed and added the way the reference's agent does it
(dqn_mgsc_batched_nonsense_transitions/agent.py:277-286); `update_priorities`
calls are interleaved so the logits differ.  After each add the state is
recorded: size, left head, the `_is_nonsense` list, the live items' fields
in FIFO order and the live logits.
"""

import importlib
import json
import os
import sys
import types

import numpy as np

REF = '/root/reference'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                   'nonsense_golden.json')
CAPACITY, N_ADD, RATIO, SEED = 7, 30, 5, 21


def _load_reference():
  jax = types.ModuleType('jax')
  jnp = types.ModuleType('jax.numpy')
  jnp.ndarray = np.ndarray
  jax.numpy = jnp
  sys.modules.setdefault('jax', jax)
  sys.modules.setdefault('jax.numpy', jnp)
  sys.modules.setdefault('snappy', types.ModuleType('snappy'))
  dm = types.ModuleType('dm_env')
  dm.TimeStep = object
  dm.StepType = object
  sys.modules.setdefault('dm_env', dm)
  pkg = types.ModuleType('dqn_zoo')
  pkg.__path__ = [os.path.join(REF, 'dqn_zoo')]
  sys.modules['dqn_zoo'] = pkg
  parts = types.ModuleType('dqn_zoo.parts')
  parts.Action = int
  sys.modules['dqn_zoo.parts'] = parts
  pkg.parts = parts
  return importlib.import_module('dqn_zoo.replay_circular_nonsense')


def item(rcn, i):
  """The i-th real transition of the stream (tests rebuild it from i)."""
  return rcn.Transition(s_tm1=i, a_tm1=i % 4, r_t=0.5 * i, discount_t=0.99 - 0.01 * (i % 3), s_t=i + 1)


def update(i, size):
  """The update_priorities call made after add i (None: no call)."""
  if i % 3 != 2 or size < 2:
    return None
  indices = [0, size - 1] if i % 2 else [size // 2, 0]
  return indices, [0.25 * (i % 5) - 0.5, 1.0 - 0.125 * i]


def main():
  rcn = _load_reference()
  r = rcn.MGSCFiFoTransitionReplay(CAPACITY, rcn.Transition(None, None, None, None, None),
                                   np.random.default_rng(SEED))
  steps = []
  for i in range(N_ADD):
    jumbled = r._t % RATIO == 0 and r._t > 0
    if jumbled:
      st = r._storage
      r.add(item(rcn, i)._replace(
          s_tm1=st[0].s_tm1, a_tm1=st[st.size - 1].a_tm1, r_t=st[st.size // 4].r_t,
          discount_t=st[st.size // 3].discount_t, s_t=st[st.size // 2].s_t), nonsense=True)
    else:
      r.add(item(rcn, i))
    up = update(i, r.size)
    if up is not None:
      r.update_priorities(np.asarray(up[0]), np.asarray(up[1], np.float32))
    st = r._storage
    live = [st[k] for k in range(st.size)]
    steps.append({
        'jumbled': bool(jumbled), 'update': up, 'size': int(st.size), 'left_head': int(st._left_head),
        'is_nonsense': [bool(x) for x in st._is_nonsense],
        'items': [[int(x.s_tm1), int(x.a_tm1), float(x.r_t), float(x.discount_t), int(x.s_t)] for x in live],
        'logits': [float(r._distribution[k]) for k in range(st.size)],
    })
  golden = {
      'generator': 'tests/golden/make_nonsense_golden.py (reference replay_circular_nonsense.py, '
                   'numpy %s)' % np.__version__,
      'capacity': CAPACITY, 'n_add': N_ADD, 'ratio': RATIO, 'seed': SEED, 'steps': steps,
  }
  with open(OUT, 'w') as f:
    json.dump(golden, f, indent=1)
  print('wrote', OUT)


if __name__ == '__main__':
  main()
