"""Prioritized double-Q C51 agent: the learning rule of
dqn_zoo/rainbow/agent.py:85-150 (rlax.categorical_double_q_learning, the loss
weighted by the replay's importance weights, clip(|loss_b|, 0, 100) written
back as the priority) on `networks.c51_atari_network`.

What Rainbow has beyond this is its network (noisy, dueling), which is
`rainbow/agent.py`'s: this agent's network has no noisy layers, so acting stays
eps-greedy and the constructor is the C51 agent's, with `double_q` (on by
default; off gives plain prioritized C51).  The replay is a PrioritizedTransitionReplay and the
transitions usually come from replay.NStepTransitionAccumulator.
"""

from dqn_mgsc_zoo_amd import learner as learner_lib
from dqn_mgsc_zoo_amd import prioritized_wide
from dqn_mgsc_zoo_amd.c51 import agent as c51_agent


class PrioritizedC51(prioritized_wide.PrioritizedWideMixin, c51_agent.C51):
  """Prioritized (double-Q) C51 agent."""

  _ALGO = 'prioritized_c51'

  def __init__(self, *args, double_q=True, **kwargs):
    self._double_q = bool(double_q)
    super().__init__(*args, **kwargs)
    self._init_priorities()

  def _new_learner(self, network, batch_size, optimizer, grad_error_bound,
                   device):
    del grad_error_bound  # categorical_double_q_learning has no clip_gradient
    return learner_lib.C51Learner(network, batch_size, optimizer=optimizer,
                                  device=device, double_q=self._double_q,
                                  prioritized=True)
