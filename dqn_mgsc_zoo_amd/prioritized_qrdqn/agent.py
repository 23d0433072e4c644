"""Prioritized double-Q QR-DQN agent: Rainbow's learning rule
(dqn_zoo/rainbow/agent.py:85-150) with rlax.quantile_q_learning in place of
the categorical loss, its selector the online network at s_t, on
`networks.qr_atari_network`.

The reference has no prioritized QR-DQN: the priority, clip(|loss_b|, 0, 100)
of the quantile loss, is this project's definition (Rainbow's rule on another
loss).  The constructor is the QR-DQN agent's with `double_q` (on by default);
acting stays eps-greedy.  The replay is a PrioritizedTransitionReplay and the
transitions usually come from replay.NStepTransitionAccumulator.
"""

from dqn_mgsc_zoo_amd import learner as learner_lib
from dqn_mgsc_zoo_amd import prioritized_wide
from dqn_mgsc_zoo_amd.qrdqn import agent as qr_agent


class PrioritizedQrDqn(prioritized_wide.PrioritizedWideMixin, qr_agent.QrDqn):
  """Prioritized (double-Q) QR-DQN agent."""

  _ALGO = 'prioritized_qrdqn'

  def __init__(self, *args, double_q=True, **kwargs):
    self._double_q = bool(double_q)
    super().__init__(*args, **kwargs)
    self._init_priorities()

  def _new_learner(self, network, batch_size, optimizer, grad_error_bound,
                   device):
    del grad_error_bound  # quantile_q_learning has no clip_gradient
    return learner_lib.QrLearner(network, batch_size,
                                 huber_param=self._huber_param,
                                 optimizer=optimizer, device=device,
                                 double_q=self._double_q, prioritized=True)
