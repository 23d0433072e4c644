"""numpy float64 restatement of the Rainbow learner step (rainbow/agent.py,
networks.py:137-178, 224-261): test infrastructure only.

The network is computed through *effective weights*: a noisy layer with noise
(e_in, e_out) is the plain linear layer

  W = Wmu + Wsig * (e_in (x) e_out),   b = bmu + bsig * e_out,

which is another formulation than the device's (noise on the activations: x Wmu
+ bmu + ((e_in x) Wsig + bsig) e_out), so agreement is not by construction.
The gradient of an effective layer chains back as dWmu = dW, dWsig = dW *
(e_in (x) e_out), dbmu = db, dbsig = db * e_out.

The torso's forward and backward are oracle.learner_ref's: both hidden layers
ride through it as one 1024-wide `linear` (advantage | value) behind an
identity `linear_1`, so its ReLU-mask pinning covers them.  The loss, weights
and priorities are tests/wide_per_ref.head_loss on the categorical head
(tests/c51_ref.categorical_loss with `select`), the optimizer tests/optim_ref.

rlax and haiku are not installed: parity with their float32 arithmetic is
unpinned; tests/test_rainbow_cpu.py pins the gradient against torch autograd
written in the reference's own order.
"""

import collections

import numpy as np

from oracle import learner_ref
from tests import optim_ref
from tests import wide_per_ref

HID = 512
FLAT = 3136
TORSO = ('sequential/conv2_d', 'sequential/conv2_d_1', 'sequential/conv2_d_2')
_REF_HEAD = 'sequential/sequential_1'
# (mu module, sigma module, mu has a bias), in the noise vector's order
LAYERS = collections.OrderedDict(
    a1=('mu', 'sigma', True), a2=('mu_1', 'sigma_1', False),
    v1=('mu_2', 'sigma_2', True), v2=('mu_3', 'sigma_3', False))


def noise_len(num_actions, num_atoms):
  return 2 * FLAT + 4 * HID + num_actions * num_atoms + num_atoms


def split_noise(vec, num_actions, num_atoms):
  """One application's vector -> {layer: (e_in, e_out)} in the draw order
  A1_in | A1_out | A2_in | A2_out | V1_in | V1_out | V2_in | V2_out."""
  vec = np.asarray(vec, np.float64).reshape(-1)
  an = num_actions * num_atoms
  assert vec.size == noise_len(num_actions, num_atoms)
  sizes = dict(a1=(FLAT, HID), a2=(HID, an), v1=(FLAT, HID), v2=(HID, num_atoms))
  out, o = {}, 0
  for name in LAYERS:
    i, j = sizes[name]
    out[name] = (vec[o:o + i], vec[o + i:o + i + j])
    o += i + j
  return out


def make_noise(rng, applications, num_actions, num_atoms):
  """sign(t) sqrt|t| of a standard normal truncated to [-2, 2] (by rejection),
  float32 [applications, noise_len]."""
  n = applications * noise_len(num_actions, num_atoms)
  t = rng.standard_normal(2 * n + 64)
  t = t[np.abs(t) <= 2.0][:n]
  return (np.sign(t) * np.sqrt(np.abs(t))).astype(np.float32).reshape(applications, -1)


def effective(params, noise):
  """{layer: (W, b)} float64 of one application."""
  out = {}
  for name, (mu, sig, mu_bias) in LAYERS.items():
    e_in, e_out = noise[name]
    w = (np.asarray(params[mu]['w'], np.float64) +
         np.asarray(params[sig]['w'], np.float64) * np.outer(e_in, e_out))
    b = np.asarray(params[sig]['b'], np.float64) * e_out
    if mu_bias:
      b = b + np.asarray(params[mu]['b'], np.float64)
    out[name] = (w, b)
  return out


def _proxy(params, eff):
  """The learner_ref parameter tree that carries both hidden layers."""
  proxy = {ref: params[own] for ref, own in zip(learner_ref.CONV_NAMES, TORSO)}
  proxy[_REF_HEAD + '/linear'] = {
      'w': np.concatenate([eff['a1'][0], eff['v1'][0]], axis=1),
      'b': np.concatenate([eff['a1'][1], eff['v1'][1]])}
  proxy[_REF_HEAD + '/linear_1'] = {'w': np.eye(2 * HID), 'b': np.zeros(2 * HID)}
  return proxy


def dueling(adv, val):
  """adv [B, A, N], val [B, N] -> q_logits [B, A, N]."""
  return val[:, None, :] + adv - adv.mean(axis=1, keepdims=True)


def network(params, s, noise_vec, num_actions, num_atoms, masks=None):
  """One application.  masks: None or (conv1, conv2, conv3, h_adv, h_val) ReLU
  decisions.  Returns dict(q_logits [B, A, N], adv, val, h_adv, h_val, masks
  (five), cache, eff, noise, proxy)."""
  noise = split_noise(noise_vec, num_actions, num_atoms)
  eff = effective(params, noise)
  proxy = _proxy(params, eff)
  if masks is not None:
    masks = tuple(masks[:3]) + (np.concatenate(
        [np.asarray(masks[3], bool).reshape(-1, HID), np.asarray(masks[4], bool).reshape(-1, HID)], axis=1),)
  h, cache = learner_ref.forward(proxy, s, masks=masks)
  h_adv, h_val = h[:, :HID], h[:, HID:]
  b = h.shape[0]
  adv = (h_adv @ eff['a2'][0] + eff['a2'][1]).reshape(b, num_actions, num_atoms)
  val = h_val @ eff['v2'][0] + eff['v2'][1]
  m = cache['masks']
  return dict(q_logits=dueling(adv, val), adv=adv, val=val, h_adv=h_adv, h_val=h_val,
              masks=tuple(m[:3]) + (m[3][:, :HID], m[3][:, HID:]), cache=cache, eff=eff,
              noise=noise, proxy=proxy)


def backward(params, fwd, dq_logits):
  """Gradient tree (the spec's leaf names) of sum(dq_logits * q_logits)."""
  b, a, n = dq_logits.shape
  eff, noise = fwd['eff'], fwd['noise']
  dval = dq_logits.sum(axis=1)
  dadv = (dq_logits - dq_logits.mean(axis=1, keepdims=True)).reshape(b, a * n)
  d_eff = {'a2': (fwd['h_adv'].T @ dadv, dadv.sum(axis=0)),
           'v2': (fwd['h_val'].T @ dval, dval.sum(axis=0))}
  dh = np.concatenate([dadv @ eff['a2'][0].T, dval @ eff['v2'][0].T], axis=1)
  g = learner_ref.backward(fwd['proxy'], fwd['cache'], dh)
  gw, gb = g[_REF_HEAD + '/linear']['w'], g[_REF_HEAD + '/linear']['b']
  d_eff['a1'] = (gw[:, :HID], gb[:HID])
  d_eff['v1'] = (gw[:, HID:], gb[HID:])
  grads = {own: g[ref] for ref, own in zip(learner_ref.CONV_NAMES, TORSO)}
  for name, (mu, sig, mu_bias) in LAYERS.items():
    e_in, e_out = noise[name]
    dw, db = d_eff[name]
    grads[mu] = {'w': dw}
    if mu_bias:
      grads[mu]['b'] = db
    grads[sig] = {'w': dw * np.outer(e_in, e_out), 'b': db * e_out}
  return grads


def learner_grads(online, target, batch, noise3, support, num_actions, weights,
                  masks=None, select=None):
  """The three applications (online(s_tm1), target(s_t), online(s_t), each
  with its own row of noise3), the double-Q weighted categorical loss and the
  gradient tree.  masks: application 0's five ReLU decisions; select pins a*.
  wide_per_ref.head_loss's dict plus `out` [3, B, A, N], `q` [3, B, A],
  `selector`, `grads`, `fwd` (application 0's network dict)."""
  s_tm1, a_tm1, r_t, discount_t, s_t = batch
  n = len(support)
  head = ('c51', support)
  f0 = network(online, s_tm1, noise3[0], num_actions, n, masks)
  f1 = network(target, s_t, noise3[1], num_actions, n)
  f2 = network(online, s_t, noise3[2], num_actions, n)
  outs = np.stack([f['q_logits'] for f in (f0, f1, f2)])
  q = np.stack([wide_per_ref.q_values(head, o) for o in outs])
  sel = wide_per_ref.selector(head, outs[2])
  res = wide_per_ref.head_loss(head, outs[0], a_tm1, r_t, discount_t, outs[1],
                               sel if select is None else select, weights)
  res.update(out=outs, q=q, selector=sel, fwd=f0,
             grads=backward(online, f0, res['wdense']))
  return res


def learner_step(online, target, m, v, count, batch, noise3, support, num_actions,
                 lr, b1, b2, eps, clip=None, weights=None, masks=None, select=None):
  """One update with chain(clip_by_global_norm(clip), adam)."""
  res = learner_grads(online, target, batch, noise3, support, num_actions, weights,
                      masks, select)
  grads = res['grads']
  res['grad_norm'] = optim_ref.global_norm(grads)
  if clip is not None:
    grads, _ = optim_ref.clip_by_global_norm(grads, clip)
  res['params'], res['mu'], res['nu'], res['count'] = optim_ref.adam(
      online, grads, m, v, count, lr, b1, b2, eps)
  return res
