"""The nonsense agent's walk over its replay, restated in numpy.

`dqn_zoo/dqn_mgsc_batched_nonsense_transitions/agent.py:290-310` cannot be
recorded (the module needs jax / haiku), so tests compare the device census
(dqz_logits_census) with this restatement:

* `census(state, logits, flags, left_head, size)`: one pass, vectorised;
* `census_loop(...)`: the same pass as a literal slot-by-slot loop with the
  reference's if / elif order, kept to cross-check the vectorised form.

Both follow the device's documented deviation from the reference: probe sums
are float64, one add per call.  `count` and `mass` (the class's share of
softmax(live logits), float64) describe the last call only.  Logits are
float32, flags non-zero for a nonsense slot, both by absolute slot; only
the window (left_head + i) mod capacity, i < size, is looked at.
"""

import numpy as np

CLASSES = ('real', 'nonsense')
PROBES = ('entry', '1st_quarter', '2nd_quarter', '3rd_quarter', 'exit')


def new_state():
  state = {'calls': 0}
  for cls in CLASSES:
    state[cls] = {'max': np.float32(-np.inf), 'min': np.float32(np.inf), 'count': 0, 'mass': 0.0}
    for p in PROBES:
      state[cls][p] = {'sum': 0.0, 'num': 0}
  return state


def probe_positions(size):
  """{probe: relative index} of the probes that count in a window of `size`
  items: a position shared by several probes goes to the first of exit,
  3rd_quarter, 2nd_quarter, 1st_quarter, entry."""
  out, seen = {}, set()
  for probe, pos in (('exit', 0), ('3rd_quarter', size // 4), ('2nd_quarter', size // 2),
                     ('1st_quarter', 3 * (size // 4)), ('entry', size - 1)):
    if size > 0 and pos not in seen:
      out[probe] = pos
      seen.add(pos)
  return out


def _window(logits, flags, left_head, size):
  logits = np.asarray(logits, np.float32)
  idx = (left_head + np.arange(size)) % logits.shape[0]
  return logits[idx], np.asarray(flags)[idx] != 0


def _terms(x):
  """exp((double)x - (double)max x) per live logit, 0 for -inf."""
  x64 = x.astype(np.float64)
  m = x64.max() if x64.size else 0.0
  with np.errstate(invalid='ignore'):
    return np.where(np.isneginf(x64), 0.0, np.exp(x64 - m))


def census(state, logits, flags, left_head, size):
  x, nonsense = _window(logits, flags, left_head, size)
  t = _terms(x)
  total = t.sum()
  for k, cls in enumerate(CLASSES):
    mine = nonsense == bool(k)
    s = state[cls]
    if mine.any():
      s['max'] = np.float32(max(s['max'], x[mine].max()))
      s['min'] = np.float32(min(s['min'], x[mine].min()))
    s['count'] = int(mine.sum())
    s['mass'] = float(t[mine].sum() / total) if total > 0 else 0.0
  for probe, pos in probe_positions(size).items():
    s = state[CLASSES[int(nonsense[pos])]][probe]
    s['sum'] += float(x[pos])
    s['num'] += 1
  state['calls'] += 1
  return state


def census_loop(state, logits, flags, left_head, size):
  logits = np.asarray(logits, np.float32)
  capacity = logits.shape[0]
  live = [float(logits[(left_head + i) % capacity]) for i in range(size)]
  m = max(live) if live else 0.0
  part = {cls: 0.0 for cls in CLASSES}
  for cls in CLASSES:
    state[cls]['count'] = 0
  for idx in range(size):
    slot = (left_head + idx) % capacity
    cls = 'nonsense' if flags[slot] else 'real'
    value = logits[slot]
    s = state[cls]
    s['max'] = max(value, s['max'])
    s['min'] = min(value, s['min'])
    s['count'] += 1
    part[cls] += 0.0 if value == -np.inf else float(np.exp(np.float64(value) - np.float64(m)))
    if idx == 0:
      probe = 'exit'
    elif idx == size // 4:
      probe = '3rd_quarter'
    elif idx == size // 2:
      probe = '2nd_quarter'
    elif idx == 3 * (size // 4):
      probe = '1st_quarter'
    elif idx == size - 1:
      probe = 'entry'
    else:
      continue
    s[probe]['sum'] += float(value)
    s[probe]['num'] += 1
  total = part['real'] + part['nonsense']
  for cls in CLASSES:
    state[cls]['mass'] = part[cls] / total if total > 0 else 0.0
  state['calls'] += 1
  return state


def stats_rows(state):
  """logit_value_stats() of the agent, from a state of this module."""
  rows = [('%s_%s' % (cls, m), float(state[cls][m])) for cls in ('nonsense', 'real') for m in ('max', 'min')]
  for cls in ('nonsense', 'real'):
    for probe in PROBES:
      p = state[cls][probe]
      rows.append(('%s_%s_avg' % (cls, probe), p['sum'] / p['num'] if p['num'] else 0))
  rows.append(('nonsense_count', state['nonsense']['count']))
  rows.append(('nonsense_mass', state['nonsense']['mass']))
  rows.append(('real_mass', state['real']['mass']))
  return rows
