"""numpy float64 restatement of the QR-DQN learner step (qrdqn/agent.py:36-39,
88-120) on top of oracle.learner_ref's forward / backward: test infrastructure
only.

  network   networks.qr_atari_network (networks.py:295-313): the NatureQNetwork
            whose last layer is N * A wide, quantile-major: q_dist[b, i, a] =
            out[b, i A + a], q_values[b, a] = mean_i q_dist[b, i, a].
  loss      rlax 0.1.2 quantile_q_learning per sample with dist_q_t_selector =
            dist_q_t (no double-Q), batch mean: a* = argmax_a mean_j x_t[j, a]
            (first maximum), theta_i = x_o[i, a_b], t_j = r + d x_t[j, a*],
            delta_ij = t_j - theta_i, w_ij = |tau_i - 1[delta_ij < 0]|,
            H_k(x) = 0.5 min(|x|, k)^2 + k (|x| - min(|x|, k)), loss_b = sum_i
            (1/N) sum_j w_ij H_k(delta_ij), with t and the indicator under
            stop_gradient.  kappa > 0 only.
  gradient  d loss / d q_dist[b, i, a_b] = -(1 / (N B)) sum_j w_ij
            clip(delta_ij, -k, k), zero for every other action; through
            learner_ref.backward as the dense cotangent at the network's output.

rlax is not installed, so parity with its float32 arithmetic is unpinned;
tests/test_qr_cpu.py pins `quantile_loss` against a plain triple loop and the
gradient against torch autograd.
"""

import numpy as np

from oracle import learner_ref
from tests import optim_ref


def make_quantiles(num_quantiles):
  """qrdqn/run_atari.py:137: (arange(N) + 0.5) / N as float32."""
  return ((np.arange(num_quantiles, dtype=np.float32) + 0.5) / float(num_quantiles)).astype(np.float32)


def q_values(q_dist):
  """[..., N, A] quantile values -> [..., A] q_values."""
  return np.asarray(q_dist, np.float64).mean(axis=-2)


def huber(x, kappa):
  ax = np.abs(x)
  m = np.minimum(ax, kappa)
  return 0.5 * m * m + kappa * (ax - m)


def quantile_loss(out_tm1, a_tm1, r_t, discount_t, out_target_t, tau, kappa, select=None):
  """The batch's loss from q_dist [B, N, A] of online(s_tm1) and target(s_t).

  select (int [B]): the target's greedy actions, in place of the argmax (a
  near-tie pinned to another implementation's choice).
  Returns dict(q_tm1 [B, A], q_target_t [B, A], a_star [B], theta [B, N], t
  [B, N], delta [B, N, N] (i, j), g [B, N, N] = w clip(delta), loss_b [B], loss,
  dtheta [B, N], dout [B, N, A])."""
  if not kappa > 0:
    raise NotImplementedError('huber_param = 0 is not built')
  xo = np.asarray(out_tm1, np.float64)
  xt = np.asarray(out_target_t, np.float64)
  tau = np.asarray(tau, np.float64)
  b, n, _ = xo.shape
  idx = np.arange(b)
  a_tm1 = np.asarray(a_tm1, np.int64)
  q_t = q_values(xt)
  a_star = np.argmax(q_t, axis=1) if select is None else np.asarray(select, np.int64)
  r = np.asarray(r_t, np.float64)
  d = np.asarray(discount_t, np.float64)
  theta = xo[idx, :, a_tm1]  # [B, N]
  t = r[:, None] + d[:, None] * xt[idx, :, a_star]  # [B, N]
  delta = t[:, None, :] - theta[:, :, None]  # [B, i, j]
  w = np.abs(tau[None, :, None] - (delta < 0))
  loss_b = np.sum(np.mean(w * huber(delta, kappa), axis=2), axis=1)
  g = w * np.clip(delta, -kappa, kappa)
  dtheta = -g.sum(axis=2) / (n * b)
  dout = np.zeros_like(xo)
  dout[idx, :, a_tm1] = dtheta
  return dict(q_tm1=q_values(xo), q_target_t=q_t, a_star=a_star, theta=theta, t=t, delta=delta, g=g,
              loss_b=loss_b, loss=float(np.mean(loss_b)), dtheta=dtheta, dout=dout)


def learner_grads(online, target, s_tm1, a_tm1, r_t, discount_t, s_t, tau, kappa, num_actions, masks=None,
                  select=None):
  """Forward of both copies, the loss and the gradient tree.  masks: the ReLU
  decisions of the online(s_tm1) pass (learner_ref.forward).  Adds `grads`,
  `masks`, `h1` (online, post-ReLU), `out_tm1` and `out_target_t` [B, N, A] to
  quantile_loss's dict."""
  n = len(tau)
  out, cache = learner_ref.forward(online, s_tm1, masks=masks)
  out_t, _ = learner_ref.forward(target, s_t)
  b = out.shape[0]
  res = quantile_loss(out.reshape(b, n, num_actions), a_tm1, r_t, discount_t, out_t.reshape(b, n, num_actions),
                      tau, kappa, select)
  res['grads'] = learner_ref.backward(online, cache, res['dout'].reshape(b, -1))
  res['masks'] = cache['masks']
  res['h1'] = cache['h1']
  res['out_tm1'] = out.reshape(b, n, num_actions)
  res['out_target_t'] = out_t.reshape(b, n, num_actions)
  return res


def learner_step(online, target, m, v, count, batch, tau, kappa, num_actions, lr, b1, b2, eps, clip=None,
                 masks=None, select=None):
  """One `update` with chain(clip_by_global_norm(clip), adam) (clip None: adam
  alone) from the state (online, target, m, v, count); batch = (s_tm1, a_tm1,
  r_t, discount_t, s_t).  Adds params / mu / nu / count / grad_norm."""
  s_tm1, a_tm1, r_t, discount_t, s_t = batch
  res = learner_grads(online, target, s_tm1, a_tm1, r_t, discount_t, s_t, tau, kappa, num_actions, masks, select)
  grads = res['grads']
  res['grad_norm'] = optim_ref.global_norm(grads)
  if clip is not None:
    grads, _ = optim_ref.clip_by_global_norm(grads, clip)
  res['params'], res['mu'], res['nu'], res['count'] = optim_ref.adam(
      online, grads, m, v, count, lr, b1, b2, eps)
  return res
