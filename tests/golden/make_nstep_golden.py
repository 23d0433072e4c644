"""Generates tests/golden/nstep_golden.json from the REFERENCE's
NStepTransitionAccumulator (dqn_zoo/replay.py).

Runs only where the reference checkout exists (the JSON output is committed).
The reference module imports jax, snappy, dm_env and dqn_zoo.parts at top
level but uses none of them on the path exercised here, so those names are
stubbed in sys.modules (make_golden.py's manner).  Nothing from the reference
is copied: this script records a stream of timesteps and what the reference's
class yields for each.

A stream is a list of [step_type, reward, discount, observation, action] with
step_type 0 / 1 / 2 = FIRST / MID / LAST and observations small integers (the
accumulator hands them through untouched); `yields` holds, per timestep, the
transitions [s_tm1, a_tm1, r_t, discount_t, s_t] the reference yields.  Floats
are float64 and survive JSON exactly (repr round-trips).
"""

import importlib
import json
import os
import sys
import types

import numpy as np

REF = '/root/reference'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                   'nstep_golden.json')
FIRST, MID, LAST = 0, 1, 2


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
  return importlib.import_module('dqn_zoo.replay')


class _TimeStep:
  """What the accumulator reads of a dm_env.TimeStep."""

  def __init__(self, step_type, reward, discount, observation):
    self.step_type, self.reward, self.discount = step_type, reward, discount
    self.observation = observation

  def first(self):
    return self.step_type == FIRST

  def last(self):
    return self.step_type == LAST

  def __str__(self):
    return 'TimeStep(%d)' % self.step_type


def episode_stream(lengths, seed, cut_after=None):
  """Timesteps of episodes of `lengths` transitions each (T = length).  With
  cut_after = k the first episode stops after k MID steps without a LAST: the
  next FIRST arrives mid-stream."""
  rs = np.random.RandomState(seed)
  stream, obs = [], 0
  for e, length in enumerate(lengths):
    stream.append([FIRST, None, None, obs, int(rs.randint(6))])
    obs += 1
    for t in range(1, length + 1):
      last = t == length
      if e == 0 and cut_after is not None and t > cut_after:
        break
      reward = float(rs.choice([-1.0, 0.0, 1.0, 0.37]))
      # an environment discount of 1 (0 at the end) times the agent's 0.99, and now and then a mid-episode 0.5
      discount = 0.0 if last else (0.5 * 0.99 if rs.rand() < 0.2 else 0.99)
      stream.append([LAST if last else MID, reward, discount, obs, int(rs.randint(6))])
      obs += 1
  return stream


def run(replay, n, stream):
  acc = replay.NStepTransitionAccumulator(n)
  yields = []
  for step_type, reward, discount, obs, action in stream:
    out = acc.step(_TimeStep(step_type, reward, discount, obs), action)
    yields.append([[t.s_tm1, t.a_tm1, float(t.r_t), float(t.discount_t), t.s_t] for t in (out or ())])
  return yields


def main():
  replay = _load_reference()
  cases = []
  for n in (1, 3, 5):
    # episodes shorter than, equal to and longer than n, then a one-transition episode
    lengths = sorted({max(n - 1, 1), n, n + 1, 2 * n + 3}) + [1]
    for name, stream in (
        ('episodes', episode_stream(lengths, seed=10 + n)),
        ('first_mid_stream', episode_stream([2 * n + 2, n + 2], seed=20 + n, cut_after=n + 1))):
      cases.append({'name': name, 'n': n, 'stream': stream, 'yields': run(replay, n, stream)})
  # a stream that does not start with FIRST raises ValueError
  acc = replay.NStepTransitionAccumulator(3)
  try:
    list(acc.step(_TimeStep(MID, 0.0, 0.99, 0), 0))
    raised = False
  except ValueError as e:
    raised = True
    message = str(e)
  assert raised
  doc = {'numpy': np.__version__, 'cases': cases,
         'non_first_start': {'error': 'ValueError', 'message': message}}
  with open(OUT, 'w') as f:
    json.dump(doc, f, indent=1)
  print('wrote %s: %d cases, %d transitions' % (
      OUT, len(cases), sum(len(y) for c in cases for y in c['yields'])))


if __name__ == '__main__':
  main()
