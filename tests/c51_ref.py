"""numpy float64 restatement of the C51 learner step (c51/agent.py:36-39,
87-117) on top of oracle.learner_ref's forward / backward: test
infrastructure only.

  network   networks.c51_atari_network (networks.py:316-335): the NatureQNetwork
            whose last layer is A * N wide; q_logits[b, a, j] = out[b, a N + j],
            q_values[b, a] = sum_j softmax_j(q_logits[b, a, :]) z_j.
  loss      rlax 0.1.2 categorical_q_learning per sample, batch mean:
            P = softmax(target logits at s_t), a* = argmax_a sum_j P[a, j] z_j
            (first maximum), p = P[a*], y_i = clip(r + d z_i, z_0, z_{N-1}),
            m = categorical_l2_project(y, p, z), loss_b = -sum_k m_k
            log_softmax(l)_k with l the online logits of the taken action and m
            under stop_gradient.
  gradient  d loss / d q_logits[b, a_b, k] = (softmax(l)_k - m_k) / B, zero for
            every other action; through learner_ref.backward as the dense
            cotangent at the network's output.

rlax is not installed, so parity with its float32 arithmetic is unpinned;
tests/test_c51_cpu.py pins `project` against the C51 paper's two-neighbour loop
and the gradient against torch autograd.
"""

import numpy as np

from oracle import learner_ref
from tests import optim_ref


def make_support(vmax, num_atoms):
  """c51/run_atari.py:134: linspace(-vmax, vmax, N) as float32."""
  return np.linspace(-vmax, vmax, num_atoms).astype(np.float32)


def softmax(x):
  x = np.asarray(x, np.float64)
  e = np.exp(x - x.max(axis=-1, keepdims=True))
  return e / e.sum(axis=-1, keepdims=True)


def log_softmax(x):
  x = np.asarray(x, np.float64)
  s = x - x.max(axis=-1, keepdims=True)
  return s - np.log(np.exp(s).sum(axis=-1, keepdims=True))


def q_values(q_logits, support):
  """[..., A, N] logits -> [..., A] q_values."""
  return softmax(q_logits) @ np.asarray(support, np.float64)


def project(z_p, probs, z_q):
  """rlax.categorical_l2_project of one distribution (z_p, probs) onto z_q."""
  z_p, probs, z_q = (np.asarray(x, np.float64) for x in (z_p, probs, z_q))
  d_pos = np.roll(z_q, -1) - z_q
  d_neg = z_q - np.roll(z_q, 1)
  z_p = np.clip(z_p, z_q[0], z_q[-1])[None, :]
  with np.errstate(divide='ignore'):
    d_pos = np.where(d_pos > 0, 1.0 / d_pos, 0.0)[:, None]
    d_neg = np.where(d_neg > 0, 1.0 / d_neg, 0.0)[:, None]
  delta_qp = z_p - z_q[:, None]
  d_sign = (delta_qp >= 0.0).astype(np.float64)
  delta_hat = d_sign * delta_qp * d_pos - (1.0 - d_sign) * delta_qp * d_neg
  return np.sum(np.clip(1.0 - delta_hat, 0.0, 1.0) * probs[None, :], axis=-1)


def categorical_loss(logits_tm1, a_tm1, r_t, discount_t, logits_target_t, support,
                     select=None):
  """The batch's loss from q_logits [B, A, N] of online(s_tm1) and target(s_t).

  select (int [B]): the target's greedy actions, in place of the argmax (a
  near-tie pinned to another implementation's choice).
  Returns dict(q_tm1 [B, A], q_target_t [B, A], a_star [B], m [B, N], logits_a
  [B, N], loss_b [B], loss, dl [B, N], dlogits [B, A, N])."""
  lo = np.asarray(logits_tm1, np.float64)
  lt = np.asarray(logits_target_t, np.float64)
  z = np.asarray(support, np.float64)
  b = lo.shape[0]
  idx = np.arange(b)
  a_tm1 = np.asarray(a_tm1, np.int64)
  q_t = q_values(lt, z)
  a_star = np.argmax(q_t, axis=1) if select is None else np.asarray(select, np.int64)
  p = softmax(lt)[idx, a_star]
  r = np.asarray(r_t, np.float64)
  d = np.asarray(discount_t, np.float64)
  m = np.stack([project(r[i] + d[i] * z, p[i], z) for i in range(b)])
  la = lo[idx, a_tm1]
  loss_b = -np.sum(m * log_softmax(la), axis=-1)
  dl = (softmax(la) - m) / b
  dlogits = np.zeros_like(lo)
  dlogits[idx, a_tm1] = dl
  return dict(q_tm1=q_values(lo, z), q_target_t=q_t, a_star=a_star, m=m, logits_a=la,
              loss_b=loss_b, loss=float(np.mean(loss_b)), dl=dl, dlogits=dlogits)


def learner_grads(online, target, s_tm1, a_tm1, r_t, discount_t, s_t, support,
                  num_actions, masks=None, select=None):
  """Forward of both copies, the loss and the gradient tree.  masks: the ReLU
  decisions of the online(s_tm1) pass (learner_ref.forward).  Adds `grads`,
  `masks`, `h1` (online, post-ReLU) and `logits_target_t` to categorical_loss's
  dict."""
  n = len(support)
  out, cache = learner_ref.forward(online, s_tm1, masks=masks)
  out_t, _ = learner_ref.forward(target, s_t)
  b = out.shape[0]
  res = categorical_loss(out.reshape(b, num_actions, n), a_tm1, r_t, discount_t,
                         out_t.reshape(b, num_actions, n), support, select)
  res['grads'] = learner_ref.backward(online, cache, res['dlogits'].reshape(b, -1))
  res['masks'] = cache['masks']
  res['h1'] = cache['h1']
  res['logits_target_t'] = out_t.reshape(b, num_actions, n)
  return res


def learner_step(online, target, m, v, count, batch, support, num_actions, lr, b1,
                 b2, eps, clip=None, masks=None, select=None):
  """One `update` with chain(clip_by_global_norm(clip), adam) (clip None: adam
  alone) from the state (online, target, m, v, count); batch = (s_tm1, a_tm1,
  r_t, discount_t, s_t).  Adds params / mu / nu / count / grad_norm."""
  s_tm1, a_tm1, r_t, discount_t, s_t = batch
  res = learner_grads(online, target, s_tm1, a_tm1, r_t, discount_t, s_t, support,
                      num_actions, masks, select)
  grads = res['grads']
  res['grad_norm'] = optim_ref.global_norm(grads)
  if clip is not None:
    grads, _ = optim_ref.clip_by_global_norm(grads, clip)
  res['params'], res['mu'], res['nu'], res['count'] = optim_ref.adam(
      online, grads, m, v, count, lr, b1, b2, eps)
  return res
