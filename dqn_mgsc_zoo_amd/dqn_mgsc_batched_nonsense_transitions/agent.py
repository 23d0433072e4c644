"""MGSC DQN agent with nonsense transitions
(drop-in for dqn_zoo/dqn_mgsc_batched_nonsense_transitions/agent.py).

The experiment that shows what the learned logits are for: every
`nonsense_transition_ratio`-th replay add is replaced by a transition jumbled
together from five stored ones (agent.py:277-286), and after the adds of
every processed timestep the agent walks the whole replay (agent.py:290-310)
to track, for nonsense and real items apart, the extremes of the logits and
their value at five ages between entry and exit of the FIFO.

Against dqn_mgsc_batched/agent.py the reference file differs in that walk,
the jumbled adds, `logit_value_stats()`, one more state entry, and the
missing `jax.lax.stop_gradient` on theta'' (:191 of the batched agent), so
the meta-gradient is the second-order one, as in the reservoir agent.

Here the jumbled item is composed on device (FrameStore.jumble) and the walk
is one device census per timestep (dqz_logits_census) into a struct that
stays in HBM; `logit_value_stats()`, `get_state()` and `set_state()` are its
only readers and the only places that synchronise for it.

Deviations from the reference, both on purpose:
* the probe sums accumulate in float64 (one add per call), the reference in
  float32 (`0 + np.float32` stays float32), which stops resolving single
  logits after some 10^7 adds;
* the `*_avg` rows are sum / num (0 when num == 0); the reference's
  `safe_div` returns the tuple (a, b).
"""

from typing import Any, List, Mapping, Tuple

from dqn_mgsc_zoo_amd import replay_circular_nonsense as replay_lib
from dqn_mgsc_zoo_amd.dqn_mgsc_batched import agent as batched

_PROBES = ('entry', '1st_quarter', '2nd_quarter', '3rd_quarter', 'exit')


def jumble_sources(size: int) -> Tuple[int, int, int, int, int]:
  """Relative indices of the items a jumbled transition takes s_tm1, a_tm1,
  r_t, discount_t and s_t from, in a replay of `size` items (agent.py:279-285)."""
  return 0, size - 1, size // 4, size // 3, size // 2


class MGSCDqn(batched.MGSCDqn):
  """MGSC DQN whose replay receives a nonsense transition every
  `nonsense_transition_ratio` adds; second-order meta-gradient."""

  _SECOND_ORDER = True

  def __init__(self, *args, nonsense_transition_ratio: int, **kwargs):
    super().__init__(*args, **kwargs)
    if nonsense_transition_ratio < 1:
      raise ValueError('nonsense_transition_ratio must be positive.')
    self._nonsense_transition_ratio = int(nonsense_transition_ratio)
    self._census = replay_lib.Census(self._learner.device)

  def step(self, timestep):
    """agent.py:251-321."""
    self._frame_t += 1
    timestep = self._preprocessor(timestep)
    transitions = []
    if timestep is None:
      if self._action is None:
        raise RuntimeError('Cannot repeat if action has never been selected.')
      action = self._action
    else:
      action = self._action = self._act(timestep)
      transitions = list(self._transition_accumulator.step(timestep, action))
      self._last_transitions = self._last_transitions + transitions
    if (self._frame_t % self._learn_period == 0 and self._replay.size >= max(
        self._meta_batch_size, self._min_replay_capacity)):
      if self._last_transitions:
        self._meta_prioritization_learn(self._last_transitions[-1])
        self._last_transitions.clear()
      else:
        print('Skipping a META LEARNING train step because the '
              '_last_transitions buffer was empty on frame %d...' %
              self._frame_t)
    if timestep is not None:
      replay = self._replay
      for transition in transitions:
        t = replay._t  # pylint: disable=protected-access
        if t % self._nonsense_transition_ratio == 0 and t > 0:
          replay.add_jumbled(*jumble_sources(replay.size))  # replaces `transition`
        else:
          replay.add(transition)
      replay.census(self._census)
    if self._replay.size < self._min_replay_capacity:
      return action
    if self._frame_t % self._learn_period == 0:
      self._learn()
      self._after_learn()
    if self._frame_t % self._target_network_update_period == 0:
      self._learner.sync_target()
      self.check_learner_health()
    return action

  def logit_value_stats(self) -> List[Tuple[str, Any, str]]:
    """The reference's 14 rows (agent.py:323-339), then the nonsense count
    and the two classes' shares of the sampling probability at the last
    census.  Synchronises."""
    c = self._census.as_dict()
    rows = [('%s_%s' % (cls, m), c[cls][m], '%.3f')
            for cls in ('nonsense', 'real') for m in ('max', 'min')]
    for cls in ('nonsense', 'real'):
      for probe in _PROBES:
        p = c[cls][probe]
        rows.append(('%s_%s_avg' % (cls, probe), p['sum'] / p['num'] if p['num'] else 0, '%.3f'))
    rows.append(('nonsense_count', c['nonsense']['count'], '%d'))
    rows.append(('nonsense_mass', c['nonsense']['mass'], '%.3f'))
    rows.append(('real_mass', c['real']['mass'], '%.3f'))
    return rows

  @property
  def census(self) -> replay_lib.Census:
    return self._census

  def get_state(self) -> Mapping[str, Any]:
    state = dict(super().get_state())
    c = self._census.as_dict()
    # the reference's nested dict (agent.py:81-122); the last call's counts and
    # masses travel beside it so a restored struct has the saver's bits
    state['logits_census'] = {'calls': c.pop('calls'),
                              **{cls: {'count': c[cls].pop('count'), 'mass': c[cls].pop('mass')}
                                 for cls in ('nonsense', 'real')}}
    state['logits_vs_time'] = c
    return state

  def set_state(self, state: Mapping[str, Any]) -> None:
    super().set_state(state)
    extra = state.get('logits_census', {})
    c = {cls: dict(state['logits_vs_time'][cls], **extra.get(cls, {})) for cls in ('nonsense', 'real')}
    c['calls'] = extra.get('calls', 0)
    self._census.load_dict(c)
