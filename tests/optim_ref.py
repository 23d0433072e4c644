"""numpy float64 restatement of the optax 0.1.2 transforms the device applies
to a finished gradient (requirements_cc.txt pins optax 0.1.2;
c51/run_atari.py:210-216 builds `chain(clip_by_global_norm(10.0), adam(lr,
eps=0.01/32))`):

  clip_by_global_norm(c)  g if |g| < c else (g / |g|) * c     (clipping.py)
  scale_by_adam           m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
                          count += 1; m / (1 - b1^count) /
                          (sqrt(v / (1 - b2^count) + eps_root) + eps)
  scale_by_rms            nu = d nu + (1 - d) g^2; g / sqrt(nu + eps)
  scale(-lr), apply_updates

Every function takes one array or a Haiku tree {module: {name: array}} (any
nesting of dicts) and returns the same shape, in float64 with no intermediate
rounding.  optax itself is not installed, so parity with optax's float32
arithmetic is unpinned; tests/test_optimizers_cpu.py pins `adam` against
torch.optim.Adam in float64.
"""

import numpy as np


def _leaves(x):
  if isinstance(x, dict):
    for k in x:
      yield from _leaves(x[k])
  else:
    yield np.asarray(x, np.float64)


def _map(f, *xs):
  if isinstance(xs[0], dict):
    return {k: _map(f, *(x[k] for x in xs)) for k in xs[0]}
  return f(*(np.asarray(x, np.float64) for x in xs))


def _unzip(tree, n):
  """A tree of n-tuples -> n trees."""
  if isinstance(tree, dict):
    parts = {k: _unzip(v, n) for k, v in tree.items()}
    return tuple({k: p[i] for k, p in parts.items()} for i in range(n))
  return tree


def global_norm(g):
  """optax.global_norm: sqrt of the sum of squares over every leaf."""
  return float(np.sqrt(sum(float(np.sum(x * x)) for x in _leaves(g))))


def clip_by_global_norm(g, max_norm):
  """(clipped gradient, the norm before clipping)."""
  norm = global_norm(g)
  if norm < max_norm:
    return _map(lambda x: x.copy(), g), norm
  return _map(lambda x: (x / norm) * max_norm, g), norm


def adam(theta, g, m, v, count, lr, b1=0.9, b2=0.999, eps=1e-8):
  """optax.adam (eps_root = 0): (theta, m, v, count) after one step."""
  count = int(count) + 1
  bc1, bc2 = 1.0 - b1**count, 1.0 - b2**count

  def leaf(th, gg, mm, vv):
    mm = b1 * mm + (1.0 - b1) * gg
    vv = b2 * vv + (1.0 - b2) * gg * gg
    return th - lr * (mm / bc1) / (np.sqrt(vv / bc2) + eps), mm, vv

  th, m, v = _unzip(_map(leaf, theta, g, m, v), 3)
  return th, m, v, count


def adam_update(g, m, v, count, lr, b1=0.9, b2=0.999, eps=1e-8):
  """The step u (theta' = theta - u) that `adam` applies, for error bounds."""
  zero = _map(np.zeros_like, g)
  th, _, _, _ = adam(zero, g, m, v, count, lr, b1, b2, eps)
  return _map(lambda x: -x, th)


def rmsprop(theta, g, nu, lr, decay=0.9, eps=1e-8):
  """optax.rmsprop(centered=False): (theta, nu) after one step."""

  def leaf(th, gg, nn):
    nn = decay * nn + (1.0 - decay) * gg * gg
    return th - lr * gg / np.sqrt(nn + eps), nn

  return _unzip(_map(leaf, theta, g, nu), 2)


def rmsprop_update(g, nu, lr, decay=0.9, eps=1e-8):
  zero = _map(np.zeros_like, g)
  th, _ = rmsprop(zero, g, nu, lr, decay, eps)
  return _map(lambda x: -x, th)
