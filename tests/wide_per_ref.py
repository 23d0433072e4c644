"""numpy float64 restatement of Rainbow's learning rule
(rainbow/agent.py:85-150,198) on the C51 and the QR-DQN networks, on top of
tests/c51_ref.py and tests/qr_ref.py: test infrastructure only.

  selector   a*_b = argmax_a q_values of learner_ref.forward(online, s_t)
             (first maximum): rlax.categorical_double_q_learning's q_t_selector,
             and quantile_q_learning's dist_q_t_selector = online(s_t).  It
             enters both losses through c51_ref / qr_ref's `select=`; nothing
             else in either loss changes and no gradient flows through it.
  weights    loss = mean_b(w_b loss_b) (`jnp.mean(losses * weights)` with the
             unweighted losses returned as the aux), so the dense cotangent at
             the network's output is w_b times the unweighted one, and the
             gradient tree learner_ref.backward of that.
  priority   clip(|loss_b|, 0, 100) of the unweighted loss (rainbow/agent.py:
             198).  The reference has no prioritized QR-DQN; the same rule on
             the quantile loss is this project's definition.

`head` is ('c51', support) or ('qr', tau, kappa).
"""

import numpy as np

from oracle import learner_ref
from tests import c51_ref
from tests import optim_ref
from tests import qr_ref

MAX_PRIORITY = 100.0


def head_shape(head, num_actions):
  """The [.., .] shape of one sample's outputs: (A, N) categorical, (N, A)
  quantile-major."""
  n = len(head[1])
  return (num_actions, n) if head[0] == 'c51' else (n, num_actions)


def q_values(head, out):
  """[B, A] q_values of outputs [B, *head_shape]."""
  return c51_ref.q_values(out, head[1]) if head[0] == 'c51' else qr_ref.q_values(out)


def selector(head, out_selector):
  """a* [B] = argmax_a q_values of the selector's outputs (first maximum)."""
  return np.argmax(q_values(head, out_selector), axis=1)


def head_loss(head, out_tm1, a_tm1, r_t, discount_t, out_target_t, select=None, weights=None):
  """c51_ref.categorical_loss / qr_ref.quantile_loss with `select`, plus
  `dense` (the unweighted dense cotangent, [B, *head_shape]), `wdense` (w_b
  times it), `wdtaken` (w_b times dl / dtheta), `wloss` = mean(w loss_b) and
  `priorities`."""
  if head[0] == 'c51':
    res = c51_ref.categorical_loss(out_tm1, a_tm1, r_t, discount_t, out_target_t, head[1], select)
    res['dense'], res['dtaken'], res['taken'] = res['dlogits'], res['dl'], res['logits_a']
  else:
    res = qr_ref.quantile_loss(out_tm1, a_tm1, r_t, discount_t, out_target_t, head[1], head[2], select)
    res['dense'], res['dtaken'], res['taken'] = res['dout'], res['dtheta'], res['theta']
  b = res['loss_b'].shape[0]
  w = np.ones(b) if weights is None else np.asarray(weights, np.float64)
  res['wdense'] = w.reshape((b,) + (1,) * (res['dense'].ndim - 1)) * res['dense']
  res['wdtaken'] = w[:, None] * res['dtaken']
  res['wloss'] = float(np.mean(w * res['loss_b']))
  res['priorities'] = np.clip(np.abs(res['loss_b']), 0.0, MAX_PRIORITY)
  return res


def learner_grads(head, online, target, batch, num_actions, weights=None, double_q=True, masks=None,
                  select=None):
  """Forward of the copies, the loss and the gradient tree.  batch = (s_tm1,
  a_tm1, r_t, discount_t, s_t).  double_q: the selector is the online network
  at s_t (else the target's own greedy action).  select pins a* to another
  implementation's choice; `selector` is always this reference's own.  masks:
  the ReLU decisions of the online(s_tm1) pass.  Adds to head_loss's dict:
  `out` [3, B, *head_shape] (online(s_tm1), target(s_t), online(s_t)), `q` [3,
  B, A], `selector`, `target_greedy`, `grads`, `masks`, `h1`."""
  s_tm1, a_tm1, r_t, discount_t, s_t = batch
  shape = head_shape(head, num_actions)
  out, cache = learner_ref.forward(online, s_tm1, masks=masks)
  out_t, _ = learner_ref.forward(target, s_t)
  out_s, _ = learner_ref.forward(online, s_t)
  b = out.shape[0]
  outs = np.stack([o.reshape((b,) + shape) for o in (out, out_t, out_s)])
  q = np.stack([q_values(head, o) for o in outs])
  sel, target_greedy = selector(head, outs[2]), selector(head, outs[1])
  if select is None:
    select = sel if double_q else target_greedy
  res = head_loss(head, outs[0], a_tm1, r_t, discount_t, outs[1], select, weights)
  res.update(out=outs, q=q, selector=sel, target_greedy=target_greedy,
             grads=learner_ref.backward(online, cache, res['wdense'].reshape(b, -1)),
             masks=cache['masks'], h1=cache['h1'])
  return res


def learner_step(head, online, target, m, v, count, batch, num_actions, lr, b1, b2, eps, clip=None,
                 weights=None, double_q=True, masks=None, select=None):
  """One `update` with chain(clip_by_global_norm(clip), adam) from the state
  (online, target, m, v, count).  Adds params / mu / nu / count / grad_norm."""
  res = learner_grads(head, online, target, batch, num_actions, weights, double_q, masks, select)
  grads = res['grads']
  res['grad_norm'] = optim_ref.global_norm(grads)
  if clip is not None:
    grads, _ = optim_ref.clip_by_global_norm(grads, clip)
  res['params'], res['mu'], res['nu'], res['count'] = optim_ref.adam(
      online, grads, m, v, count, lr, b1, b2, eps)
  return res
