"""Rainbow agent class (drop-in for dqn_zoo/rainbow/agent.py:40-250).

rlax.categorical_double_q_learning weighted by the replay's importance weights,
clip(|loss_b|, 0, 100) written back as the priority, on
`networks.rainbow_atari_network` (noisy, dueling).  The learning rule and the
replay plumbing are prioritized_wide's; what this file adds is the noise.

There is no epsilon: an actor call applies the network once under fresh noise
and takes the argmax (rainbow/agent.py:121-131), and a learn draws three noise
vectors, one per application (online(s_tm1), target(s_t), online(s_t)).  All
noise comes from one Philox stream, the agent's seed, at a device counter that
`dqz_rainbow_noise` advances; `get_state` carries the counter, so a restored
agent continues the same stream.  (JAX's threefry keys are not reproducible
here; the distribution is the reference's.)
"""

from typing import Any

import torch

from dqn_mgsc_zoo_amd import learner as learner_lib
from dqn_mgsc_zoo_amd import networks as networks_lib
from dqn_mgsc_zoo_amd import parts
from dqn_mgsc_zoo_amd import prioritized_wide
from dqn_mgsc_zoo_amd.c51 import agent as c51_agent


class Rainbow(prioritized_wide.PrioritizedWideMixin, c51_agent.C51):
  """Rainbow agent."""

  _ALGO = 'rainbow'

  def __init__(self, preprocessor, sample_network_input,
               network: networks_lib.RainbowNetworkSpec, support, optimizer,
               transition_accumulator: Any, replay, batch_size: int,
               min_replay_capacity_fraction: float, learn_period: int,
               target_network_update_period: int, rng_key, device='cuda'):
    super().__init__(preprocessor, sample_network_input, network, support,
                     optimizer, transition_accumulator, replay, batch_size,
                     lambda t: 0.0, min_replay_capacity_fraction, learn_period,
                     target_network_update_period, rng_key, device=device)
    self._init_priorities()
    lrn = self._learner
    self._noise_counter = torch.zeros((1,), dtype=torch.int64, device=lrn.device)
    self._act_noise = torch.zeros((1, lrn.noise_len), dtype=torch.float32, device=lrn.device)
    self._learn_noise = torch.zeros((3, lrn.noise_len), dtype=torch.float32, device=lrn.device)

  def _new_learner(self, network, batch_size, optimizer, grad_error_bound,
                   device):
    del grad_error_bound  # categorical_double_q_learning has no clip_gradient
    return learner_lib.RainbowLearner(network, batch_size, optimizer=optimizer,
                                      device=device)

  def _act(self, timestep) -> parts.Action:
    """select_action (rainbow/agent.py:121-131): one application under fresh
    noise, the argmax, v_t = max_a q as statistics['state_value']."""
    lrn = self._learner
    lrn.make_noise(self._act_seed, self._noise_counter, 1, out=self._act_noise)
    a, v = lrn.act(timestep.observation, self._act_noise)
    self._act_count += 1
    self._statistics['state_value'] = v
    return parts.Action(a)

  def _step_extra(self):
    """A learn's three noise vectors, drawn behind the sample."""
    return (self._learner.make_noise(self._act_seed, self._noise_counter, 3,
                                     out=self._learn_noise),)

  @property
  def noise_counter(self) -> int:
    """Floats of noise drawn so far (reads the device counter)."""
    return int(self._noise_counter.item())

  def get_state(self):
    state = dict(super().get_state())
    state['noise_counter'] = self.noise_counter
    return state

  def set_state(self, state) -> None:
    super().set_state(state)
    self._noise_counter.fill_(int(state['noise_counter']))
