"""What the prioritized C51 and QR-DQN agents share: Rainbow's learning rule
(dqn_zoo/rainbow/agent.py:85-150,179-206) around a wide-head learner created
with `prioritized=True`.

New items enter the replay at the running `max_seen_priority`; a learn samples
by priority, weights the loss with the replay's importance weights and writes
clip(|loss_b|, 0, 100) back as the sampled items' priorities.  With frame
transitions the sum tree lives in HBM and a learn is three device calls with
no host synchronisation: the sample (dqz_per_sample), the weighted step, and
dqz_per_write_back on the head's inner learner, whose TD buffer the head filled
with the priorities.  `max_seen_priority` is then a device scalar, read back
only when asked for.  Host-stored items keep the reference's host path.
"""

import numpy as np
import torch


class PrioritizedWideMixin:
  """In front of an agent_base.DeviceDqnAgent whose learner is a wide one with
  prioritized=True and whose replay is a PrioritizedTransitionReplay."""

  def _init_priorities(self):
    dev = self._learner.device
    b = self._batch_size
    self._max_seen_priority = 1.0
    self._max_seen_dev = torch.ones((1,), dtype=torch.float64, device=dev)
    self._w = torch.zeros((b,), dtype=torch.float32, device=dev)
    self._sample_out = (torch.zeros((b,), dtype=torch.int32, device=dev),
                        torch.zeros((b,), dtype=torch.int32, device=dev),
                        self._w)

  def _add(self, transition) -> None:
    if self._replay.stores_on_device(transition):
      self._replay.add(transition, priority=self._max_seen_dev)
    else:
      self._replay.add(transition, priority=self._max_seen_priority)

  def _step_extra(self):
    """What this agent's learner step takes behind the weights, made ready
    between the sample and the step (Rainbow: its noise)."""
    return ()

  def _learn(self) -> None:
    if self._replay.on_device:
      indices, slots, weights = self._replay.sample_device(
          self._batch_size, out=self._sample_out)
      self._learner.step(self._store(), slots, weights, *self._step_extra())
      self._replay.write_back(self._learner, indices, self._max_seen_dev)
      return
    ids, slots, weights = self._replay.sample_slots(self._batch_size)
    self._w.copy_(torch.from_numpy(np.asarray(weights, np.float32)))
    self._learner.step(self._store(), slots, self._w, *self._step_extra())
    priorities = self._learner.fetch_outputs()[-1].cpu().numpy().astype(np.float64)
    self._max_seen_priority = max(self._max_seen_priority, float(priorities.max()))
    self._replay.update_priorities(ids, priorities)

  @property
  def importance_sampling_exponent(self) -> float:
    return self._replay.importance_sampling_exponent

  @property
  def max_seen_priority(self) -> float:
    if self._replay.on_device:
      return float(self._max_seen_dev.item())
    return self._max_seen_priority

  def get_state(self):
    state = dict(super().get_state())
    state['max_seen_priority'] = self.max_seen_priority
    return state

  def set_state(self, state) -> None:
    super().set_state(state)
    self._max_seen_priority = float(state['max_seen_priority'])
    self._max_seen_dev.fill_(self._max_seen_priority)
