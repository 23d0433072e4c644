"""GPU: the Rainbow learner step, noise kernel and actor (csrc/rainbow.hpp,
dqz_rainbow_*) against tests/rainbow_ref.py (float64, effective weights: another
formulation than the device's noise-on-activations one).

Store: tests/test_c51_gpu.py's.  Shapes (B, A, N): B in {2, 17, 33} (one
partial 16-row tile, two tiles, two 32-row fc1 groups), (A, N) in {(1, 2) no
advantage, (3, 51) the usual case, (18, 51) a wide head, (16, 64) A N = 1024};
(33, 16, 64) appears together.  The sigma leaves are scaled up from their
initial constant by random factors in [2, 6], so that a noise term that is
wrong or transposed moves every compared quantity far past its bar.

Stage checks, from the device's own inputs (u = 2^-24; a K-term f32 sum of
products in any order is within (K + c) u sum|term| of the exact one, c
counting the roundings that form a term):
  h_adv, h_val  from the device's y3: K = 3136 + 2 (bias, e_out), both parts
  adv, val      from the device's h: atol 1e-5, the bar tests/test_c51_gpu.py
                holds the same product to
  q_logits      from the device's adv / val: an A-term mean and two adds
  dz_adv/val    from the device's dl and ReLU decisions: K = A N (or N)
  fc leaves     from the device's h, dz and dl: K = B terms
End to end, ReLU masks of the torso and of both hidden layers and a* pinned
from the device: tests/test_c51_gpu.py's bars (logits 1e-4, q_values 1e-4 zmax,
loss and grad_norm rtol 1e-4, params atol 2e-6 after clip + Adam).

The sigma leaves' gradients have no bar elsewhere in the project.  Measured on
an MI355X against the float64 reference at the four shapes (SIGMA_MEASURED
below: worst absolute error, and worst error relative to the leaf's largest
|gradient|):
  (2, 1, 2)     abs 1.400e-08   rel 5.888e-07
  (17, 3, 51)   abs 1.450e-08   rel 7.914e-07
  (17, 18, 51)  abs 1.410e-08   rel 1.500e-06
  (33, 16, 64)  abs 6.757e-09   rel 6.045e-07
The bar is 4 x the worst of each column (5.8e-8 and 6.0e-6), which a wrong
term (errors of order 1 relative) misses by orders of magnitude and f32
summation order does not reach.
"""

import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import c51_ref
from tests import fake_env
from tests import helpers
from tests import rainbow_ref
from tests.test_c51_gpu import _store_contents
from tests.test_trajectory_gpu import _batch

pytestmark = pytest.mark.gpu

LR, ADAM_EPS, B1, B2, CLIP = 6.25e-5, 0.005 / 32, 0.9, 0.999, 10.0  # rainbow/run_atari.py
VMAX = 10.0
U = 2.0**-24
SHAPES = {(2, 1, 2): 0, (17, 3, 51): 1, (17, 18, 51): 2, (33, 16, 64): 3}
SHAPE_IDS = ['%dx%dx%d' % s for s in SHAPES]
SIGMA_LEAVES = [(m, k) for m in ('sigma', 'sigma_1', 'sigma_2', 'sigma_3') for k in ('w', 'b')]
# worst over the four shapes, MI355X: (absolute error, error / max|gradient| of the leaf)
SIGMA_MEASURED = (1.45e-8, 1.5e-6)
SIGMA_BAR = tuple(None if x is None else 4.0 * x for x in SIGMA_MEASURED)


def _f32(x):
  return float(np.float32(x))


def _np(t):
  return t.detach().cpu().numpy()


def _bits(t):
  return _np(t).view(np.int32).copy()


def _optimizer(clip=CLIP):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  opt = learner_lib.adam(LR, B1, B2, ADAM_EPS)
  return opt if clip is None else learner_lib.chain(learner_lib.clip_by_global_norm(clip), opt)


def _params(net, seed):
  rng = np.random.default_rng(seed + 100)
  tree = net.init(seed)
  for mod in tree:
    if mod.startswith('sigma'):
      for k in tree[mod]:
        tree[mod][k] = (tree[mod][k] * rng.uniform(2.0, 6.0, size=tree[mod][k].shape)).astype(np.float32)
  return tree


@functools.lru_cache(maxsize=None)
def _case(b, a, n):
  """Host side of one shape, computed once and never modified."""
  from dqn_mgsc_zoo_amd import networks
  seed = SHAPES.get((b, a, n), 4)
  support = c51_ref.make_support(VMAX, n)
  net = networks.rainbow_atari_network(a, support, 0.1)
  online = _params(net, seed)
  target = helpers.perturbed_tree(online, seed + 1)
  host = _store_contents(a, seed)
  rng = np.random.default_rng(seed + 5)
  slots = rng.integers(0, 256, size=b).astype(np.int32)
  weights = rng.uniform(0.25, 1.0, size=b).astype(np.float32)
  noise = rainbow_ref.make_noise(rng, 3, a, n)
  return dict(net=net, support=support, online=online, target=target, host=host, slots=slots,
              weights=weights, noise=noise, shape=(b, a, n))


def _device(case, device, clip=CLIP, optimizer=None):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import store as store_lib
  lrn = learner_lib.RainbowLearner(case['net'], case['shape'][0], optimizer=optimizer or _optimizer(clip),
                                   device=device)
  lrn.set_params(case['online'], case['target'])
  st = store_lib.FrameStore(256, 640)
  for name, arr in case['host'].items():
    getattr(st, name).copy_(torch.from_numpy(arr))
  return lrn, st


def _args(case, device, noise=None):
  return (torch.from_numpy(case['slots']).to(device), torch.from_numpy(case['weights']).to(device),
          torch.from_numpy(case['noise'] if noise is None else noise).to(device))


def _within(got, want, bound, what):
  err = np.abs(np.asarray(got, np.float64) - want)
  bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
  worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
  print('%s: err / bound at most %.3f (err %.3e, bound %.3e)' % (
      what, err.flat[worst] / max(bound.flat[worst], 1e-300), err.flat[worst], bound.flat[worst]))
  assert (err <= bound).all(), (what, worst, err.flat[worst], bound.flat[worst])


def _masks(lrn):
  """Application 0's five ReLU decisions, from the device."""
  act = lrn.fetch_activations(0)
  h_val = lrn.fetch_noisy()[1]
  return [_np(act[k]) > 0 for k in ('y1', 'y2', 'y3', 'h1')] + [_np(h_val) > 0]


def _f64(tree, mod, name):
  return np.asarray(tree[mod][name], np.float64)


@pytest.mark.parametrize('shape', list(SHAPES), ids=SHAPE_IDS)
def test_stages_from_the_devices_own_inputs(device, shape):
  b, a, n = shape
  an = a * n
  case = _case(*shape)
  lrn, st = _device(case, device)
  slots, weights, noise = _args(case, device)
  g = lrn.grad(st, slots, weights, noise)
  logits, dl = [_np(x) for x in lrn.fetch_head()]
  h_adv, h_val, adv, val, dz_adv, dz_val = [_np(x).astype(np.float64) for x in lrn.fetch_noisy()]
  act0 = lrn.fetch_activations(0, backward=True)
  y3 = _np(act0['y3']).astype(np.float64).reshape(b, -1)
  assert lrn.sync_status() == 0
  np.testing.assert_array_equal(h_adv, _np(act0['h1']))
  np.testing.assert_array_equal(dz_adv, _np(act0['dz1']))
  p, e = case['online'], rainbow_ref.split_noise(case['noise'][0], a, n)

  def noisy(x, layer, bound_terms):
    mu, sig, mu_bias = rainbow_ref.LAYERS[layer]
    e_in, e_out = e[layer]
    bmu = _f64(p, mu, 'b') if mu_bias else 0.0
    out = x @ _f64(p, mu, 'w') + bmu + ((x * e_in) @ _f64(p, sig, 'w') + _f64(p, sig, 'b')) * e_out
    mag = (np.abs(x) @ np.abs(_f64(p, mu, 'w')) + np.abs(bmu) +
           (np.abs(x * e_in) @ np.abs(_f64(p, sig, 'w')) + np.abs(_f64(p, sig, 'b'))) * np.abs(e_out))
    return out, (bound_terms + 4) * U * mag

  for layer, got in (('a1', h_adv), ('v1', h_val)):
    want, bound = noisy(y3, layer, 3136)
    _within(got, np.maximum(want, 0.0), bound, 'h of ' + layer)
  want, _ = noisy(h_adv, 'a2', 512)
  np.testing.assert_allclose(adv.reshape(b, an), want, atol=1e-5, err_msg='adv')
  want, _ = noisy(h_val, 'v2', 512)
  np.testing.assert_allclose(val, want, atol=1e-5, err_msg='val')
  mag = np.abs(val)[:, None, :] + np.abs(adv) + np.abs(adv).mean(axis=1, keepdims=True)
  _within(logits[0], rainbow_ref.dueling(adv, val), (a + 4) * U * mag, 'q_logits')
  # the dueling combine's known answers on the device's own numbers
  _within((logits[0] - val[:, None, :]).mean(axis=1), 0.0, (a + 4) * U * mag.max(axis=1), 'mean_a(q - val)')
  if a == 1:
    np.testing.assert_array_equal(logits[0][:, 0], val.astype(np.float32))
  # backward from dl
  acts = case['host']['action'][case['slots']]
  dl64 = dl.astype(np.float64)
  onehot = (acts[:, None] == np.arange(a)[None, :]).astype(np.float64)
  dadv = ((onehot - 1.0 / a)[:, :, None] * dl64[:, None, :]).reshape(b, an)
  dval = dl64

  def noisy_t(gr, layer, x_mask):
    mu, sig, _ = rainbow_ref.LAYERS[layer]
    e_in, e_out = e[layer]
    out = gr @ _f64(p, mu, 'w').T + e_in * ((gr * e_out) @ _f64(p, sig, 'w').T)
    mag = np.abs(gr) @ np.abs(_f64(p, mu, 'w')).T + np.abs(e_in) * (np.abs(gr * e_out) @ np.abs(_f64(p, sig, 'w')).T)
    return out * x_mask, (gr.shape[1] + 6) * U * mag + 1e-45

  want, bound = noisy_t(dadv, 'a2', h_adv > 0)
  _within(dz_adv, want, bound, 'dz_adv')
  want, bound = noisy_t(dval, 'v2', h_val > 0)
  _within(dz_val, want, bound, 'dz_val')
  # every fc leaf from the device's own x and g: K = B terms
  got = case['net'].unflatten(_np(g))
  xs = dict(a1=y3, v1=y3, a2=h_adv, v2=h_val)
  gs = dict(a1=dz_adv, v1=dz_val, a2=dadv, v2=dval)
  for layer, (mu, sig, mu_bias) in rainbow_ref.LAYERS.items():
    e_in, e_out = e[layer]
    x, gr = xs[layer], gs[layer]
    leaves = [(mu, 'w', x.T @ gr, np.abs(x).T @ np.abs(gr)),
              (sig, 'w', (x * e_in).T @ (gr * e_out), np.abs(x * e_in).T @ np.abs(gr * e_out)),
              (sig, 'b', (gr * e_out).sum(0), np.abs(gr * e_out).sum(0))]
    if mu_bias:
      leaves.append((mu, 'b', gr.sum(0), np.abs(gr).sum(0)))
    for mod, name, want, mag in leaves:
      _within(got[mod][name], want, (b + 6) * U * mag + 1e-45, 'd %s/%s' % (mod, name))
  # every element of every leaf is written: a second call into a poisoned buffer gives the same bytes
  g2 = torch.full_like(g, float('nan'))
  lrn.grad(st, slots, weights, noise, out=g2)
  offs, sizes, _ = case['net'].layout()
  for o, s in zip(offs, sizes):
    assert torch.equal(g[o:o + s].view(torch.int32), g2[o:o + s].view(torch.int32))


def _reference_step(case, state, count, slots, weights, noise, masks, a_star):
  hp = [_f32(x) for x in (LR, B1, B2, ADAM_EPS)]
  return rainbow_ref.learner_step(state[0], state[1], state[2], state[3], count, _batch(case['host'], slots),
                                  noise, case['support'], case['shape'][1], *hp, clip=_f32(CLIP),
                                  weights=weights, masks=masks, select=a_star)


def _check_a_star(a_star, ref):
  """The device's a* is the reference's own wherever the selector's best two
  q_values are 1e-3 apart; closer ones are a rounding matter and stay pinned."""
  q = np.sort(ref['q'][2], axis=1)
  clear = (q[:, -1] - q[:, -2] >= 1e-3) if q.shape[1] > 1 else np.ones(len(q), bool)
  np.testing.assert_array_equal(a_star[clear], ref['selector'][clear])


def _check_step(lrn, ref, what):
  logits_a, qv, loss_b, loss, a_star, prio = [_np(x) for x in lrn.fetch_outputs()]
  logits = _np(lrn.fetch_head()[0])
  zmax = float(np.abs(lrn.network.support).max())
  _check_a_star(a_star, ref)
  np.testing.assert_allclose(logits, ref['out'], atol=1e-4, err_msg=what)
  np.testing.assert_allclose(logits_a, ref['taken'], atol=1e-4, err_msg=what)
  np.testing.assert_allclose(qv, ref['q'], atol=1e-4 * zmax, err_msg=what)
  np.testing.assert_allclose(loss[0], ref['wloss'], rtol=1e-4, err_msg=what)
  # |d loss_b| <= 2 max|d logit|: the logits' bar carried to the per-sample loss and the priority
  np.testing.assert_allclose(loss_b, ref['loss_b'], rtol=0, atol=2e-4, err_msg=what)
  np.testing.assert_allclose(prio, ref['priorities'], rtol=0, atol=2e-4, err_msg=what)
  np.testing.assert_allclose(float(lrn.grad_norm().item()), ref['grad_norm'], rtol=1e-4, err_msg=what)
  assert int(lrn.count.item()) == ref['count']
  got = lrn.params_tree('online')
  for m in ref['params']:
    for k in ref['params'][m]:
      np.testing.assert_allclose(got[m][k], ref['params'][m][k], atol=2e-6, err_msg='%s %s/%s' % (what, m, k))


def _sigma_errors(got, want):
  """(worst absolute error, worst error / max|gradient|) over the sigma leaves."""
  worst_abs = worst_rel = 0.0
  for m, k in SIGMA_LEAVES:
    err = float(np.abs(got[m][k].astype(np.float64) - want[m][k]).max())
    scale = float(np.abs(want[m][k]).max())
    print('  d %s/%s: err %.3e, max|g| %.3e, err / max|g| %.3e' % (m, k, err, scale, err / max(scale, 1e-300)))
    worst_abs, worst_rel = max(worst_abs, err), max(worst_rel, err / max(scale, 1e-300))
  return worst_abs, worst_rel


@pytest.mark.parametrize('shape', list(SHAPES), ids=SHAPE_IDS)
def test_one_step_matches_the_oracle(device, shape):
  case = _case(*shape)
  lrn, st = _device(case, device)
  slots, weights, noise = _args(case, device)
  g = case['net'].unflatten(_np(lrn.grad(st, slots, weights, noise)))
  lrn.step(st, slots, weights, noise)
  a_star = _np(lrn.fetch_outputs()[4])
  zeros = {m: {k: np.zeros_like(v, np.float64) for k, v in d.items()} for m, d in case['online'].items()}
  ref = _reference_step(case, [case['online'], case['target'], zeros, zeros], 0, case['slots'],
                        case['weights'], case['noise'], _masks(lrn), a_star)
  _check_step(lrn, ref, 'x'.join(map(str, shape)))
  got_t = lrn.params_tree('target')
  for m in case['target']:
    for k in case['target'][m]:
      np.testing.assert_array_equal(got_t[m][k], case['target'][m][k])
  assert lrn.sync_status() == 0
  worst_abs, worst_rel = _sigma_errors(g, ref['grads'])
  print('SIGMA %s abs %.3e rel %.3e' % ('x'.join(map(str, shape)), worst_abs, worst_rel))
  assert SIGMA_BAR[0] is not None, 'the sigma leaves\' bar has not been measured'
  assert worst_abs <= SIGMA_BAR[0] and worst_rel <= SIGMA_BAR[1]


def test_ten_carried_steps(device):
  """Every step the oracle starts from the device's own state, with the
  device's masks and a*, under fresh device-drawn noise; a target sync after
  step 5, bit-equal."""
  case = _case(4, 3, 7)
  lrn, st = _device(case, device)
  rng = np.random.default_rng(21)
  counter = torch.zeros((1,), dtype=torch.int64, device=device)
  seen = []
  for step in range(10):
    slots = rng.integers(0, 256, size=4).astype(np.int32)
    weights = rng.uniform(0.25, 1.0, size=4).astype(np.float32)
    noise = lrn.make_noise(77, counter)
    torch.cuda.synchronize()
    state = [lrn.params_tree(w) for w in ('online', 'target', 'mu', 'nu')]
    count = int(lrn.count.item())
    lrn.step(st, torch.from_numpy(slots).to(device), torch.from_numpy(weights).to(device), noise)
    a_star = _np(lrn.fetch_outputs()[4])
    ref = _reference_step(case, state, count, slots, weights, _np(noise), _masks(lrn), a_star)
    _check_step(lrn, ref, 'step %d' % step)
    seen.append(_bits(noise))
    if step == 5:
      lrn.sync_target()
      torch.cuda.synchronize()
      assert torch.equal(lrn.online.view(torch.int32), lrn.target.view(torch.int32))
  assert int(lrn.count.item()) == 10 and lrn.sync_status() == 0
  assert int(counter.item()) == 10 * 3 * lrn.noise_len
  assert all(not np.array_equal(seen[0], s) for s in seen[1:])


def test_zero_noise_is_the_mu_only_dueling_network(device):
  shape = (17, 3, 51)
  b, a, n = shape
  case = _case(*shape)
  lrn, st = _device(case, device)
  zero = np.zeros_like(case['noise'])
  slots, weights, noise = _args(case, device, zero)
  g = case['net'].unflatten(_np(lrn.grad(st, slots, weights, noise)))
  for m, k in SIGMA_LEAVES:  # e_in = e_out = 0: exactly zero, weights and biases
    assert np.all(g[m][k] == 0.0), (m, k)
  lrn.step(st, slots, weights, noise)
  a_star = _np(lrn.fetch_outputs()[4])
  # the oracle's mu-only dueling network: every sigma leaf 0, so its own noise (not zero) has nothing to act on
  mu_only = lambda tree: {m: ({k: np.zeros_like(v) for k, v in d.items()} if m.startswith('sigma') else d)
                          for m, d in tree.items()}
  other = rainbow_ref.make_noise(np.random.default_rng(0), 3, a, n)
  s_tm1, _, _, _, s_t = _batch(case['host'], case['slots'])
  fwd = [rainbow_ref.network(mu_only(tree), s, other[i], a, n)['q_logits']
         for i, (tree, s) in enumerate(((case['online'], s_tm1), (case['target'], s_t), (case['online'], s_t)))]
  np.testing.assert_allclose(_np(lrn.fetch_head()[0]), np.stack(fwd), atol=1e-4, err_msg='mu-only logits')
  # and the whole step: the oracle under zero noise (its effective weights are then mu's, bit for bit:
  # tests/test_rainbow_cpu.py), whose sigma gradients are zero as well
  zeros = {m: {k: np.zeros_like(v, np.float64) for k, v in d.items()} for m, d in case['online'].items()}
  ref = _reference_step(case, [case['online'], case['target'], zeros, zeros], 0, case['slots'], case['weights'],
                        zero, _masks(lrn), a_star)
  for m, k in SIGMA_LEAVES:
    assert not np.any(ref['grads'][m][k])
  _check_step(lrn, ref, 'zero noise')


def test_noise_kernel(device):
  from dqn_mgsc_zoo_amd import _native
  lib = _native.lib()
  n, seed = 3 * (8320 + 3 * 51 + 51), 12345
  counter = torch.full((1,), 5, dtype=torch.int64, device=device)
  u = torch.empty((n,), dtype=torch.float64, device=device)
  _native.check(lib.dqz_uniform_philox(seed, _native.ptr(counter), n, _native.ptr(u), _native.stream_handle()))
  outs = []
  for _ in range(2):
    counter.fill_(5)
    f = torch.empty((n,), dtype=torch.float32, device=device)
    _native.check(lib.dqz_rainbow_noise(seed, _native.ptr(counter), n, _native.ptr(f), _native.stream_handle()))
    outs.append(f)
  torch.cuda.synchronize()
  assert int(counter.item()) == 5 + n
  assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
  f = outs[0].double().cpu()
  hi = torch.erf(torch.tensor(2.0, dtype=torch.float64).sqrt())
  lo = -hi
  t = np.sqrt(2.0) * torch.special.erfinv(lo + u.cpu() * (hi - lo))
  got = torch.sign(f) * f * f
  assert float((got - t).abs().max()) <= 1e-5
  assert float(got.abs().max()) <= 2.0 + 1e-6 and float(f.abs().max()) <= np.sqrt(2.0) + 1e-6
  # a truncated standard normal: mean 0, variance 1 - 4 phi(2) / (2 Phi(2) - 1) = 0.774
  assert abs(float(t.mean())) < 0.02 and abs(float(t.var()) - 0.7737) < 0.02
  other = torch.empty((n,), dtype=torch.float32, device=device)
  _native.check(lib.dqz_rainbow_noise(seed, _native.ptr(counter), n, _native.ptr(other), _native.stream_handle()))
  assert not torch.equal(other, outs[0])
  for bad in (0, 65537):
    assert lib.dqz_rainbow_noise(seed, _native.ptr(counter), bad, _native.ptr(other), None) == -1


def _snapshot(lrn):
  return [t.clone() for t in (lrn.online, lrn.mu, lrn.nu, lrn.count)]


def _restore(lrn, snap):
  for t, s in zip((lrn.online, lrn.mu, lrn.nu, lrn.count), snap):
    t.copy_(s)


def _all_bits(lrn):
  out = [_bits(t) for t in (lrn.online, lrn.mu, lrn.nu, lrn.count, lrn.target)]
  out += [_bits(t) for t in lrn.fetch_outputs()]
  out += [_bits(t) for t in lrn.fetch_head()]
  out += [_bits(t) for t in lrn.fetch_noisy()]
  out.append(_bits(lrn.grad_norm()))
  return out


def test_a_step_is_bit_reproducible(device):
  case = _case(17, 3, 51)
  lrn, st = _device(case, device)
  args = _args(case, device)
  lrn.step(st, *args)  # carried moments under the repeated step
  snap = _snapshot(lrn)
  runs = []
  for _ in range(2):
    _restore(lrn, snap)
    lrn.step(st, *args)
    torch.cuda.synchronize()
    runs.append(_all_bits(lrn))
  for x, y in zip(*runs):
    assert np.array_equal(x, y)
  assert not np.array_equal(runs[0][0], _bits(snap[0]))


def test_a_step_is_its_gradient_then_apply(device):
  case = _case(4, 3, 7)
  lrn, st = _device(case, device, clip=0.05)
  args = _args(case, device)
  for step in range(2):  # the second from carried moments
    snap = _snapshot(lrn)
    lrn.step(st, *args)
    after = _snapshot(lrn)
    gn = lrn.grad_norm().clone()
    _restore(lrn, snap)
    lrn.apply(lrn.grad(st, *args))
    torch.cuda.synchronize()
    for x, y in zip(after, _snapshot(lrn)):
      assert torch.equal(x, y), step
    assert torch.equal(gn, lrn.grad_norm())
    torch.cuda.synchronize()
    assert not torch.equal(snap[0], after[0])
    assert float(gn.item()) > 0.05 and int(lrn.count.item()) == step + 1
    assert lrn.sync_status() == 0


def test_three_captured_steps_equal_three_eager_steps(device):
  case = _case(17, 3, 51)
  lrn, st = _device(case, device)
  args = _args(case, device)
  snap = _snapshot(lrn)
  for _ in range(3):
    lrn.step(st, *args)
  torch.cuda.synchronize()
  eager = _all_bits(lrn)
  side = torch.cuda.Stream(device)
  side.wait_stream(torch.cuda.current_stream(device))
  with torch.cuda.stream(side):  # warm-up off the default stream, as capture requires
    lrn.step(st, *args)
  torch.cuda.current_stream(device).wait_stream(side)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(3):
      lrn.step(st, *args)
  torch.cuda.synchronize()
  _restore(lrn, snap)
  g.replay()
  torch.cuda.synchronize()
  for x, y in zip(eager, _all_bits(lrn)):
    assert np.array_equal(x, y)
  assert int(lrn.count.item()) == 3


def test_padding_is_inert_and_kept(device):
  """tests/test_param_padding_gpu.py's contract on the twenty-leaf layout: with
  1e30 in every padding float of the parameters, the moments and the gradient
  buffer, two carried steps and the gradient are bit-equal to the zero-padding
  run's, and the padding holds its fill afterwards."""
  case = _case(4, 3, 7)
  offs, sizes, total = case['net'].layout()
  pad = torch.ones((total,), dtype=torch.bool)
  for o, s in zip(offs, sizes):
    pad[o:o + s] = False
  assert int(pad.sum()) > 0
  runs = []
  for fill in (0.0, 1e30):
    lrn, st = _device(case, device)
    args = _args(case, device)
    padd = pad.to(device)
    state = (lrn.online, lrn.target, lrn.mu, lrn.nu)
    for t in state:
      t[padd] = fill
    g = torch.full((total,), fill, dtype=torch.float32, device=device)
    lrn.grad(st, *args, out=g)
    for _ in range(2):
      lrn.step(st, *args)
    torch.cuda.synchronize()
    for t in state + (g,):
      assert bool((t[padd] == fill).all())
    runs.append([_bits(t[~padd]) for t in state + (g,)] + [_bits(lrn.grad_norm())] +
                [_bits(t) for t in lrn.fetch_outputs()])
    assert lrn.sync_status() == 0
  for x, y in zip(*runs):
    assert np.array_equal(x, y)


def test_other_learners_unchanged_beside_a_rainbow_learner(device):
  """A DQN step and a plain C51 step leave the same bytes with and without a
  Rainbow learner alive (and having stepped) beside them."""
  from tests import test_c51_gpu
  from tests.test_learner_gpu import _setup

  def dqn_step():
    _, lrn, st, _, _, _, _, _ = _setup('dqn', 8, seed=3)
    slots = torch.from_numpy(np.random.default_rng(5).integers(0, 256, 8).astype(np.int32)).to(device)
    lrn.step(st, slots)
    torch.cuda.synchronize()
    return [_bits(t) for t in (lrn.online, lrn.mu, lrn.nu) + tuple(lrn.fetch_outputs())]

  def c51_step():
    c = test_c51_gpu._case(5, 3, 7)  # pylint: disable=protected-access
    lrn, st = test_c51_gpu._device(c, device)  # pylint: disable=protected-access
    lrn.step(st, torch.from_numpy(c['slots']).to(device))
    torch.cuda.synchronize()
    return [_bits(t) for t in (lrn.online, lrn.mu, lrn.nu, lrn.count) + tuple(lrn.fetch_outputs())]

  before = dqn_step() + c51_step()
  case = _case(4, 3, 7)
  rb, st = _device(case, device)
  slots, weights, noise = _args(case, device)
  rb.step(st, slots, weights, noise)
  rb.q_values_slots(st, slots, 0, noise[0])
  torch.cuda.synchronize()
  for x, y in zip(before, dqn_step() + c51_step()):
    assert np.array_equal(x, y)
  assert rb.sync_status() == 0


def test_actor(device):
  shape = (17, 3, 51)
  b, a, n = shape
  case = _case(*shape)
  lrn, st = _device(case, device)
  host, slots = case['host'], case['slots']
  s_t = helpers.stacks_from(host['frames'], host['fidx'], slots, 1)
  noise = torch.from_numpy(case['noise']).to(device)
  zmax = float(np.abs(case['support']).max())
  ref = rainbow_ref.network(case['online'], s_t, case['noise'][2], a, n)
  q_ref = c51_ref.q_values(ref['q_logits'], case['support'])
  q_direct = lrn.q_values(torch.from_numpy(s_t).to(device), noise[2])
  q_slots = lrn.q_values_slots(st, torch.from_numpy(slots).to(device), 1, noise[2])
  np.testing.assert_allclose(_np(q_direct), q_ref, atol=1e-4 * zmax)
  assert torch.equal(q_direct, q_slots)
  q1 = lrn.q_values(torch.from_numpy(s_t[2:3]).to(device), noise[2])  # n below the batch (fc1's few-row kernel)
  np.testing.assert_allclose(_np(q1), q_ref[2:3], atol=1e-4 * zmax)
  q_other = lrn.q_values(torch.from_numpy(s_t).to(device), noise[0])
  assert not torch.equal(q_other, q_direct)  # other noise, other q
  for i in range(3):  # no epsilon: the argmax of q_values under the same noise, v_t = max_a q
    q_host = _np(lrn.q_values(torch.from_numpy(s_t[i:i + 1]).to(device), noise[2]))[0]
    action, value = lrn.act(s_t[i], noise[2])
    assert action == int(np.argmax(q_host))
    assert value == float(q_host.max())
    np.testing.assert_allclose(q_host, q_ref[i], atol=1e-4 * zmax)


def _small(device):
  """B = 5, A = 3, N = 7: (learner, store, (slots, weights, noise [3, len]),
  the batch's s_t stacks [B,84,84,4], another three noise vectors)."""
  case = _case(5, 3, 7)
  lrn, st = _device(case, device)
  host = case['host']
  s_t = helpers.stacks_from(host['frames'], host['fidx'], case['slots'], 1)
  other = rainbow_ref.make_noise(np.random.default_rng(11), 3, 3, 7)
  assert not np.array_equal(other, case['noise'])
  return lrn, st, _args(case, device), s_t, torch.from_numpy(other).to(device)


def test_profile_names_the_noisy_networks_launches(device):
  """profile() reports the noisy network's launches under their own names, in
  place of the C51 and QR-DQN ones, and changes no state."""
  from dqn_mgsc_zoo_amd import learner as learner_lib
  lrn, st, (slots, weights, noise), _, _ = _small(device)
  state = (lrn.online, lrn.target, lrn.mu, lrn.nu, lrn.count)
  before = [_bits(t) for t in state]
  ms = lrn.profile(st, slots, weights, noise, iters=2)
  torch.cuda.synchronize()
  print(sorted(ms))
  own = {'rb_noisy_forward', 'c51_head', 'rb_dhidden', 'rb_fc1_dx', 'rb_fc_grad'}
  assert own == set(learner_lib.RainbowLearner._PROFILE_SLOTS.values())  # pylint: disable=protected-access
  assert own <= set(ms)
  replaced = set()
  for other in (learner_lib.C51Learner, learner_lib.QrLearner):
    replaced |= set(other._PROFILE_SLOTS.values()) - own  # pylint: disable=protected-access
  assert len(replaced) == 6 and not replaced & set(ms)
  assert set(ms) == own | {
      'conv1_fwd', 'fc1_fwd', 'conv3_dx+conv2_dx+fc1_dw+conv3_dw+conv2_dw+conv1_dw', 'update'}
  for t, b in zip(state, before):
    assert np.array_equal(_bits(t), b)
  assert lrn.sync_status() == 0


def test_noise_belongs_to_the_call(device):
  """No call leaves its noise behind for a later one: a gradient under one
  noise has the same bits before and after forwards and an actor call under
  others, and a forward the same bits before and after a gradient."""
  lrn, st, (slots, weights, noise_a), s_t, other = _small(device)
  states = torch.from_numpy(s_t).to(device)
  grad_a = _bits(lrn.grad(st, slots, weights, noise_a))
  q_b = _bits(lrn.q_values(states, other[0]))
  lrn.q_values_slots(st, slots, 1, other[1])
  lrn.act(s_t[0], other[2])
  assert np.array_equal(_bits(lrn.grad(st, slots, weights, noise_a)), grad_a)
  assert np.array_equal(_bits(lrn.q_values(states, other[0])), q_b)
  # the noise is read: other vectors, other bits
  assert not np.array_equal(_bits(lrn.grad(st, slots, weights, other)), grad_a)
  assert not np.array_equal(_bits(lrn.q_values(states, other[1])), q_b)
  assert lrn.sync_status() == 0


def test_q_values_in_chunks(device):
  """q_values of 2B - 1 states under one noise vector is the calls on [0, B)
  and [B, 2B - 1) side by side, bit for bit."""
  lrn, _, _, s_t, other = _small(device)
  b = s_t.shape[0]
  states = torch.from_numpy(np.concatenate([s_t, s_t[::-1][:b - 1]])).to(device)
  assert states.shape[0] == 2 * b - 1
  whole = lrn.q_values(states, other[0])
  parts = torch.cat([lrn.q_values(states[:b], other[0]), lrn.q_values(states[b:], other[0])])
  assert whole.shape == (2 * b - 1, 3)
  assert np.array_equal(_bits(whole), _bits(parts))
  assert not np.array_equal(_bits(whole[:b - 1]), _bits(whole[b:]))  # other states behind the first chunk


def test_refusals_and_limits(device):
  from dqn_mgsc_zoo_amd import _native
  from dqn_mgsc_zoo_amd import learner as learner_lib
  lib = _native.lib()
  req = _native.C51_REQ
  w = req['weights']
  expect = {
      w | req['per_draw']: b'the rainbow head takes no prioritized draw',
      w | req['uniform_draw']: b'the rainbow head takes no in-launch batch draw',
      w | req['logit_draw']: b'the rainbow head takes no in-launch batch draw',
      w | req['exact_draw']: b'the rainbow head takes no in-launch batch draw',
      w | req['meta_p']: b'the rainbow head has no MGSC meta mode',
      w | req['meta_epi']: b'the rainbow head has no MGSC meta mode',
      w | req['meta_softmax']: b'the rainbow head has no MGSC meta mode',
      w | req['unit']: b'the rainbow head has no unit-cotangent pass',
      w | req['write_back']:
          b'the rainbow head writes its priorities back through dqz_per_write_back (no fused write-back)',
      w | req['fused_rmsprop']: b'the rainbow head runs in gradient mode only (no fused centered RMSProp)',
      0: b'a weighted rainbow step needs is_weights',
  }
  for request, message in expect.items():
    assert lib.dqz_rainbow_debug_check(8, request) == -1
    assert lib.dqz_last_error() == message, (request, lib.dqz_last_error())
  assert lib.dqz_rainbow_debug_check(8, w) == 0
  assert lib.dqz_rainbow_debug_check(1, w) == -1
  assert lib.dqz_last_error() == b'the rainbow head needs batch >= 2'
  h = ctypes.c_void_p()
  past = [(8, 6, 65, b'num_atoms must be in [2, 64]'), (8, 6, 1, b'num_atoms must be in [2, 64]'),
          (8, 25, 41, b'num_actions * num_atoms must be <= 1024'),
          (8, 33, 31, b'num_actions must be in [1, 32]'), (8, 0, 31, b'num_actions must be in [1, 32]'),
          (1, 6, 51, b'batch must be in [2, 256]'), (257, 6, 51, b'batch must be in [2, 256]')]
  for batch, a, n, message in past:
    cfg = _native.DqzLearnerConfig(batch, a, _native.ALGO_DQN, LR, 0.0, ADAM_EPS, 0.0)
    sup = torch.from_numpy(c51_ref.make_support(VMAX, max(n, 2))).to(device)
    assert lib.dqz_rainbow_create(ctypes.byref(cfg), n, _native.ptr(sup), None, ctypes.byref(h)) == -1
    assert lib.dqz_last_error() == message, (batch, a, n, lib.dqz_last_error())
  for batch, a, n in ((256, 1, 2), (2, 32, 32), (2, 16, 64)):  # the last value inside each limit
    cfg = _native.DqzLearnerConfig(batch, a, _native.ALGO_DQN, LR, 0.0, ADAM_EPS, 0.0)
    sup = torch.from_numpy(c51_ref.make_support(VMAX, n)).to(device)
    assert lib.dqz_rainbow_create(ctypes.byref(cfg), n, _native.ptr(sup), None, ctypes.byref(h)) == 0
    assert lib.dqz_rainbow_destroy(h) == 0
  cfg = _native.DqzLearnerConfig(8, 6, _native.ALGO_DQN, LR, 0.0, ADAM_EPS, 0.0)
  sup = torch.from_numpy(c51_ref.make_support(VMAX, 51)).to(device)
  plain = _native.DqzWideOptions(1, 0)
  assert lib.dqz_rainbow_create(ctypes.byref(cfg), 51, _native.ptr(sup), ctypes.byref(plain), ctypes.byref(h)) == -1
  assert lib.dqz_last_error().startswith(b'the rainbow step is always double-Q and weighted')
  bad = torch.tensor([0.0, 1.0, 0.5], device=device)
  assert lib.dqz_rainbow_create(ctypes.byref(cfg), 3, _native.ptr(bad), None, ctypes.byref(h)) == -1
  assert lib.dqz_last_error() == b'support must be finite and strictly increasing (atom 2)'
  # the Python surface: no fused draws, no centered RMSProp, noise and weights required
  case = _case(4, 3, 7)
  with pytest.raises(NotImplementedError, match='centered'):
    learner_lib.RainbowLearner(case['net'], 4, optimizer=learner_lib.rmsprop(1e-4, centered=True), device=device)
  with pytest.raises(ValueError, match='rainbow_atari_network'):
    learner_lib.RainbowLearner(_c51_net(), 4, device=device)
  lrn, st = _device(case, device)
  slots, weights, noise = _args(case, device)
  with pytest.raises(ValueError, match='importance weights'):
    lrn.step(st, slots, None, noise)
  with pytest.raises(ValueError, match='noise'):
    lrn.step(st, slots, weights, noise[:2])
  for call in (lrn.step, lrn.grad, lrn.profile):  # weights are refused before noise, noise by every entry
    with pytest.raises(ValueError, match='importance weights'):
      call(st, slots, None, noise[:2])
    with pytest.raises(ValueError, match='noise'):
      call(st, slots, weights, noise[:2])
  with pytest.raises(NotImplementedError, match='takes its batch as slots'):
    lrn.step_uniform()
  # an optimizer of another layout is refused before anything runs
  c51_opt = ctypes.c_void_p()
  ocfg = _native.DqzOptimizerConfig(_native.OPT_ADAM, LR, B1, B2, 0.0, ADAM_EPS, 0.0, 3, 0)
  _native.check(lib.dqz_c51_optimizer_create(ctypes.byref(ocfg), 7, ctypes.byref(c51_opt)))
  rc = lib.dqz_rainbow_step(lrn._wide, ctypes.byref(lrn._params_c), st.c_ref(), _native.ptr(slots),  # pylint: disable=protected-access
                            _native.ptr(weights), _native.ptr(noise), c51_opt, _native.ptr(lrn.count), None)
  assert rc == -1 and lib.dqz_last_error() == b'the optimizer was created for another parameter layout'
  lib.dqz_optimizer_destroy(c51_opt)


def _c51_net():
  from dqn_mgsc_zoo_amd import networks
  return networks.c51_atari_network(3, c51_ref.make_support(VMAX, 7))


# -- the agent -------------------------------------------------------------------

def _agent(seed, capacity=256):
  from dqn_mgsc_zoo_amd import networks
  from dqn_mgsc_zoo_amd import replay as replay_lib
  from dqn_mgsc_zoo_amd.rainbow import agent as agent_lib
  replay = replay_lib.PrioritizedTransitionReplay(
      capacity, replay_lib.Transition(None, None, None, None, None), priority_exponent=0.5,
      importance_sampling_exponent=lambda t: 0.4, uniform_sample_probability=1e-3, normalize_weights=True,
      random_state=np.random.RandomState(seed))
  support = c51_ref.make_support(VMAX, 51)
  agent = agent_lib.Rainbow(
      preprocessor=fake_env.FrameStacker(), sample_network_input=np.zeros((84, 84, 4), np.uint8),
      network=networks.rainbow_atari_network(6, support, 0.1), support=support, optimizer=_optimizer(),
      transition_accumulator=replay_lib.NStepTransitionAccumulator(3), replay=replay, batch_size=10,
      min_replay_capacity_fraction=0.15, learn_period=2, target_network_update_period=4,
      rng_key=np.array([0, seed], np.uint32))
  return agent, replay


def _run(agent, num_steps, seed=1, episode_len=11):
  from dqn_mgsc_zoo_amd import parts
  env = fake_env.FakeAtari(episode_len=episode_len, seed=seed)
  loop = parts.run_loop(agent, env, max_steps_per_episode=0)
  for _ in range(num_steps):
    next(loop)


def test_agent_learns_and_syncs_the_target(device):
  agent, replay = _agent(0)
  lrn = agent.learner
  p0 = lrn.online.clone()
  synced = []
  sync_target = lrn.sync_target

  def spy(*args, **kwargs):
    sync_target(*args, **kwargs)
    synced.append(agent._frame_t)  # pylint: disable=protected-access

  lrn.sync_target = spy
  _run(agent, 110)
  learns = int(lrn.count.item())
  assert replay.on_device and replay.size >= 90 and learns >= 20
  assert not torch.equal(p0, lrn.online) and torch.isfinite(lrn.online).all()
  assert len(synced) >= 10 and all(t % 4 == 0 for t in synced)
  assert not torch.equal(p0, lrn.target)
  assert agent.check_learner_health() == 0
  assert np.isfinite(agent.statistics['state_value'])
  assert agent.exploration_epsilon == 0.0
  # one application per action selected, three per learn, all from the one counter
  acts = agent._act_count  # pylint: disable=protected-access
  assert agent.noise_counter == (acts + 3 * learns) * lrn.noise_len
  assert set(agent.get_state()) == {'rng_key', 'frame_t', 'opt_state', 'online_params', 'target_params', 'replay',
                                    'max_seen_priority', 'noise_counter'}
  assert agent.max_seen_priority >= 1.0
  ok, msg = replay.check_valid()
  assert ok, msg


def test_agent_state_round_trip(device):
  a1, r1 = _agent(4)
  _run(a1, 80, seed=5)
  state = copy.deepcopy(a1.get_state())
  assert state['noise_counter'] == a1.noise_counter > 0
  a2, r2 = _agent(99)
  a2.set_state(state)
  r2._random_state.set_state(r1._random_state.get_state())  # pylint: disable=protected-access
  assert a2.noise_counter == a1.noise_counter and a2.max_seen_priority == a1.max_seen_priority
  env = fake_env.FakeAtari(episode_len=9, seed=6)
  steps = [env.reset()]
  for t in range(24):
    steps.append(env.step(t % 6) if not steps[-1].last() else env.reset())
  before = int(a1.learner.count.item())
  for ts in steps:
    if ts.first():
      a1.reset()
      a2.reset()
    assert a1.step(ts) == a2.step(ts)  # the next actions, under the same noise
  for which in ('online', 'target', 'mu', 'nu', 'count'):
    assert torch.equal(getattr(a1.learner, which), getattr(a2.learner, which))  # and the next learns
  assert int(a1.learner.count.item()) > before
  assert a1.noise_counter == a2.noise_counter > state['noise_counter']
  # a restored agent with another counter acts under other noise
  a3, _ = _agent(99)
  a3.set_state(dict(state, noise_counter=state['noise_counter'] + 1))
  at = torch.full((1,), state['noise_counter'], dtype=torch.int64, device=device)
  seed = a3._act_seed  # pylint: disable=protected-access
  assert seed == a1._act_seed  # pylint: disable=protected-access
  assert not torch.equal(a3.learner.make_noise(seed, a3._noise_counter, 1),  # pylint: disable=protected-access
                         a3.learner.make_noise(seed, at, 1))
  # checkpoint kinds follow prioritized_c51: a DQN agent's centered-RMSProp state is refused by name
  from dqn_mgsc_zoo_amd import optim_state
  zeros = a1.learner.params_tree('mu')
  with pytest.raises(ValueError, match='centered-RMSProp state'):
    a2.set_state(dict(state, opt_state=optim_state.rmsprop_state(zeros, zeros)))
