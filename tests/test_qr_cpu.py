"""CPU: the QR-DQN restatement (tests/qr_ref.py) against independent
implementations, and the quantile entries' refusals that run before any device
call.

  loss        against a plain triple loop over (b, i, j) written from the
              formulas of include/dqz.h, within 1e-12.
  gradient    the loss and d loss / d out against torch autograd in float64 on
              the head alone (h1 -> out -> loss; the indicator and the target
              under .detach()), then the whole network's gradient at B = 2,
              A = 3, N = 5.
  known       N = 1 with tau = 0.5; d = 0; theta = t sorted.
"""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import learner_ref
from tests import helpers
from tests import qr_ref

INVALID = -1  # DQZ_ERR_INVALID


def _huber(x, k):
  ax = abs(x)
  m = min(ax, k)
  return 0.5 * m * m + k * (ax - m)


def _loop_loss(xo, a_tm1, r, d, xt, tau, kappa):
  """loss_b [B] and d loss / d theta [B, N] by a plain loop."""
  b, n, _ = xo.shape
  loss_b = np.zeros(b)
  dtheta = np.zeros((b, n))
  for s in range(b):
    means = [sum(xt[s, j, a] for j in range(n)) / n for a in range(xt.shape[2])]
    a_star = int(np.argmax(means))
    for i in range(n):
      theta = xo[s, i, a_tm1[s]]
      row = 0.0
      for j in range(n):
        delta = r[s] + d[s] * xt[s, j, a_star] - theta
        w = abs(tau[i] - (1.0 if delta < 0 else 0.0))
        row += w * _huber(delta, kappa)
        dtheta[s, i] -= w * min(max(delta, -kappa), kappa) / (n * b)
      loss_b[s] += row / n
  return loss_b, dtheta


def _random_head(b, a, n, seed, scale=1.0):
  rng = np.random.default_rng(seed)
  xo = scale * rng.standard_normal((b, n, a))
  xt = scale * rng.standard_normal((b, n, a))
  a_tm1 = rng.integers(0, a, b)
  r = rng.choice([-1.0, 0.0, 1.0], b)
  d = 0.99 * (rng.random(b) > 0.3)
  return xo, xt, a_tm1, r, d


@pytest.mark.parametrize('b,a,n,kappa', [(3, 2, 4, 1.0), (4, 3, 7, 0.25), (2, 6, 33, 1.0), (2, 2, 1, 1.0)])
def test_quantile_loss_matches_a_plain_loop(b, a, n, kappa):
  xo, xt, a_tm1, r, d = _random_head(b, a, n, seed=b + 10 * n, scale=2.0)
  tau = qr_ref.make_quantiles(n).astype(np.float64)
  res = qr_ref.quantile_loss(xo, a_tm1, r, d, xt, tau, kappa)
  loss_b, dtheta = _loop_loss(xo, a_tm1, r, d, xt, tau, kappa)
  assert np.abs(res['loss_b'] - loss_b).max() <= 1e-12
  assert np.abs(res['dtheta'] - dtheta).max() <= 1e-12
  assert abs(res['loss'] - loss_b.mean()) <= 1e-12
  # both sides of |delta| = kappa and of delta = 0 occur, so every branch of the loop ran
  if n > 1:
    assert (np.abs(res['delta']) > kappa).any() and (np.abs(res['delta']) < kappa).any()
    assert (res['delta'] < 0).any() and (res['delta'] > 0).any()
  # the dense cotangent is dtheta at the taken action and zero elsewhere
  idx = np.arange(b)
  assert np.array_equal(res['dout'][idx, :, a_tm1], res['dtheta'])
  assert np.count_nonzero(res['dout']) <= b * n


def _torch_loss(out_tm1, a_tm1, r, d, out_t, tau, kappa):
  """mean_b of rlax's quantile_regression_loss in torch float64; the target and
  the indicator are detached."""
  b, n, _ = out_tm1.shape
  idx = torch.arange(b)
  with torch.no_grad():
    a_star = out_t.mean(dim=1).argmax(dim=1)
  theta = out_tm1[idx, :, torch.as_tensor(a_tm1, dtype=torch.long)]
  t = (torch.as_tensor(r)[:, None] + torch.as_tensor(d)[:, None] * out_t[idx, :, a_star]).detach()
  delta = t[:, None, :] - theta[:, :, None]
  w = torch.abs(torch.as_tensor(tau)[None, :, None] - (delta < 0).to(torch.float64).detach())
  ad = delta.abs()
  m = torch.clamp(ad, max=kappa)
  return (w * (0.5 * m * m + kappa * (ad - m))).mean(dim=2).sum(dim=1).mean()


@pytest.mark.parametrize('b,a,n,kappa', [(4, 3, 5, 1.0), (8, 6, 201, 1.0), (4, 3, 9, 0.05)])
def test_loss_and_dout_match_autograd_on_the_head(b, a, n, kappa):
  rng = np.random.default_rng(b + n)
  tau = qr_ref.make_quantiles(n).astype(np.float64)
  h1 = np.maximum(rng.standard_normal((b, 512)), 0.0)
  w = rng.uniform(-1, 1, (512, n * a)) / np.sqrt(512)
  bias = rng.uniform(-1, 1, n * a) / np.sqrt(512)
  out_t = rng.standard_normal((b, n, a))
  a_tm1 = rng.integers(0, a, b)
  r = rng.choice([-1.0, 0.0, 1.0], b)
  d = 0.99 * (rng.random(b) > 0.3)
  res = qr_ref.quantile_loss((h1 @ w + bias).reshape(b, n, a), a_tm1, r, d, out_t, tau, kappa)
  th1, tw, tb = (torch.tensor(x, requires_grad=True) for x in (h1, w, bias))
  out = (th1 @ tw + tb).reshape(b, n, a)
  out.retain_grad()
  tt = torch.tensor(out_t, requires_grad=True)
  loss = _torch_loss(out, a_tm1, r, d, tt, tau, kappa)
  loss.backward()
  assert tt.grad is None or not tt.grad.abs().max() > 0  # nothing flows into the target copy
  assert abs(loss.item() - res['loss']) <= 1e-12 * max(1.0, abs(res['loss']))
  np.testing.assert_allclose(res['dout'], out.grad.numpy(), atol=1e-14)
  dense = res['dout'].reshape(b, -1)
  np.testing.assert_allclose(h1.T @ dense, tw.grad.numpy(), atol=1e-13)
  np.testing.assert_allclose(dense.sum(0), tb.grad.numpy(), atol=1e-13)
  np.testing.assert_allclose(dense @ w.T, th1.grad.numpy(), atol=1e-13)


def test_whole_network_gradient_matches_autograd():
  from dqn_mgsc_zoo_amd import networks
  b, a, n = 2, 3, 5
  tau = qr_ref.make_quantiles(n)
  net = networks.qr_atari_network(a, tau)
  online = net.init(1)
  target = helpers.perturbed_tree(online, 2)
  rng = np.random.default_rng(3)
  s_tm1 = rng.integers(0, 256, (b, 84, 84, 4), dtype=np.uint8)
  s_t = rng.integers(0, 256, (b, 84, 84, 4), dtype=np.uint8)
  a_tm1, r, d = np.array([2, 0]), np.array([1.0, -1.0]), np.array([0.99, 0.0])
  kappa = 1.0
  res = qr_ref.learner_grads(online, target, s_tm1, a_tm1, r, d, s_t, tau, kappa, a)

  names = list(learner_ref.CONV_NAMES)
  head = 'sequential/sequential_1'
  tp = {m: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in leaves.items()}
        for m, leaves in online.items()}

  def apply(params, s):
    x = torch.as_tensor(s.astype(np.float64) / 255.0).permute(0, 3, 1, 2)
    for name, stride in zip(names, (4, 2, 1)):
      x = F.relu(F.conv2d(x, params[name]['w'].permute(3, 2, 0, 1), params[name]['b'], stride=stride))
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)  # Haiku's (h, w, c) flatten
    h = F.relu(x @ params[head + '/linear']['w'] + params[head + '/linear']['b'])
    return (h @ params[head + '/linear_1']['w'] + params[head + '/linear_1']['b']).reshape(-1, n, a)

  with torch.no_grad():
    tt = {m: {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in leaves.items()}
          for m, leaves in target.items()}
    out_t = apply(tt, s_t)
  np.testing.assert_allclose(res['out_target_t'], out_t.numpy(), atol=1e-12)
  loss = _torch_loss(apply(tp, s_tm1), a_tm1, r, d, out_t, tau.astype(np.float64), kappa)
  loss.backward()
  assert abs(loss.item() - res['loss']) <= 1e-12
  for m in online:
    for k in online[m]:
      got, want = res['grads'][m][k], tp[m][k].grad.numpy()
      assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (m, k)
  assert np.abs(res['grads'][head + '/linear_1']['w']).max() > 0


def test_known_answers():
  kappa = 1.0
  # N = 1, tau = 0.5: loss_b = 0.5 H_k(t - theta), on both sides of kappa
  for theta, x_t, r, d in ((0.3, 0.7, 1.0, 0.99), (2.0, -1.0, -1.0, 0.5), (0.0, 0.25, 0.0, 1.0)):
    res = qr_ref.quantile_loss(np.array([[[theta, 9.0]]]), [0], [r], [d], np.array([[[x_t, -9.0]]]), [0.5], kappa)
    assert res['a_star'][0] == 0
    assert abs(res['loss_b'][0] - 0.5 * _huber(r + d * x_t - theta, kappa)) <= 1e-15
  # d = 0: every t_j = r, whatever the target holds
  xo, xt, a_tm1, r, _ = _random_head(3, 2, 6, seed=4)
  tau = qr_ref.make_quantiles(6).astype(np.float64)
  res = qr_ref.quantile_loss(xo, a_tm1, r, np.zeros(3), xt, tau, kappa)
  assert np.array_equal(res['t'], np.broadcast_to(np.asarray(r)[:, None], (3, 6)))
  other = qr_ref.quantile_loss(xo, a_tm1, r, np.zeros(3), 5.0 * xt[:, ::-1], tau, kappa)
  assert np.array_equal(res['loss_b'], other['loss_b']) and np.array_equal(res['dtheta'], other['dtheta'])
  # theta equal to t elementwise and sorted: the diagonal terms vanish, and the loss is the off-diagonal sum
  n = 5
  tau = qr_ref.make_quantiles(n).astype(np.float64)
  t = np.array([-0.8, -0.1, 0.0, 0.4, 2.5])
  xo = np.zeros((1, n, 2))
  xo[0, :, 1] = t
  xt = np.zeros((1, n, 2))
  xt[0, :, 0] = t  # a* = 0: mean 0.4 against 0
  xt[0, :, 1] = -1.0
  res = qr_ref.quantile_loss(xo, [1], [0.0], [1.0], xt, tau, kappa)
  assert res['a_star'][0] == 0 and np.array_equal(res['theta'][0], t) and np.array_equal(res['t'][0], t)
  assert not np.diagonal(res['delta'][0]).any() and not np.diagonal(res['g'][0]).any()
  want = sum((tau[i] if t[j] > t[i] else 1 - tau[i]) * _huber(t[j] - t[i], kappa)
             for i in range(n) for j in range(n) if i != j) / n
  assert abs(res['loss_b'][0] - want) <= 1e-15
  with pytest.raises(NotImplementedError, match='huber_param = 0'):
    qr_ref.quantile_loss(xo, [1], [0.0], [1.0], xt, tau, 0.0)


# -- refusals before any device call -------------------------------------------

@pytest.fixture(scope='module')
def lib():
  import os  # pylint: disable=g-import-not-at-top
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  if not os.path.exists(_native.LIB_PATH):
    import __graft_entry__  # pylint: disable=g-import-not-at-top
    __graft_entry__._compile_lib()  # pylint: disable=protected-access
  return _native.lib()


_WORD = ctypes.c_int64(0)
P = ctypes.cast(ctypes.pointer(_WORD), ctypes.c_void_p)  # any non-null address


def _cfg(batch=8, num_actions=6, algo=0):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  return _native.DqzLearnerConfig(batch, num_actions, algo, 5e-5, 0.0, 1e-4, 0.0)


def _ocfg(num_actions=6, shared=0, kind=0):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  return _native.DqzOptimizerConfig(kind, 5e-5, 0.9, 0.999, 0.9, 1e-4, 10.0, num_actions, shared)


def _refusals():
  h = ctypes.c_void_p()
  out = ctypes.byref(h)
  i64 = (ctypes.c_int64 * 10)()
  tot = ctypes.byref(ctypes.c_int64())
  create = lambda cfg, n, tau=P, k=1.0: ('dqz_qr_create', (ctypes.byref(cfg), n, tau, k, out))
  opt = lambda cfg, n: ('dqz_qr_optimizer_create', (ctypes.byref(cfg), n, out))
  layout = lambda a, n, o=i64: ('dqz_qr_param_layout', (a, n, o, i64, tot))
  huber = 'huber_param must be finite and > 0 (huber_param = 0, rlax\'s plain |delta| branch, is not built)'
  return [
      ('layout-no-quantiles', layout(6, 0), 'num_quantiles must be in [1, 256]'),
      ('layout-too-many-quantiles', layout(6, 257), 'num_quantiles must be in [1, 256]'),
      ('layout-too-wide', layout(17, 241), 'num_actions * num_quantiles must be <= 4096'),  # A N = 4097
      ('layout-no-actions', layout(0, 201), 'num_actions must be in [1, 32]'),
      ('layout-null-out', layout(6, 201, None), 'null output pointer'),
      ('create-null-config', ('dqz_qr_create', (None, 201, P, 1.0, out)), 'null argument'),
      ('create-null-quantiles', create(_cfg(), 201, None), 'null argument'),
      ('create-null-out', ('dqz_qr_create', (ctypes.byref(_cfg()), 201, P, 1.0, None)), 'null argument'),
      ('create-no-quantiles', create(_cfg(), 0), 'num_quantiles must be in [1, 256]'),
      ('create-too-many-quantiles', create(_cfg(), 257), 'num_quantiles must be in [1, 256]'),
      ('create-too-wide', create(_cfg(num_actions=17), 241), 'num_actions * num_quantiles must be <= 4096'),
      ('create-batch-one', create(_cfg(batch=1), 201), 'batch must be in [2, 256]'),
      # the first value past each limit (N = 257, A N = 4097 and batch 1 are above)
      ('create-33-actions', create(_cfg(num_actions=33), 124), 'num_actions must be in [1, 32]'),
      ('create-batch-257', create(_cfg(batch=257), 201), 'batch must be in [2, 256]'),
      ('create-double-q', create(_cfg(algo=1), 201), 'the quantile head runs on a DQN learner'),
      ('create-huber-zero', create(_cfg(), 201, P, 0.0), huber),
      ('create-huber-negative', create(_cfg(), 201, P, -1.0), huber),
      ('create-huber-nan', create(_cfg(), 201, P, float('nan')), huber),
      ('optimizer-null-config', ('dqz_qr_optimizer_create', (None, 201, out)), 'null argument'),
      ('optimizer-no-quantiles', opt(_ocfg(), 0), 'num_quantiles must be in [1, 256]'),
      ('optimizer-too-wide', opt(_ocfg(num_actions=17), 241), 'num_actions * num_quantiles must be <= 4096'),
      ('optimizer-shared-bias', opt(_ocfg(shared=1), 201), 'the quantile head has no shared bias'),
      ('optimizer-kind', opt(_ocfg(kind=2), 201), 'optimizer kind must be DQZ_OPT_ADAM or DQZ_OPT_RMSPROP'),
      ('step-null-handle', ('dqz_qr_step', (None, 'PARAMS', 'STORE', P, P, P, None)), 'null argument'),
      ('grad-null-handle', ('dqz_qr_grad', (None, 'PARAMS', 'STORE', P, P, None)), 'null argument'),
      ('profile-null-handle', ('dqz_qr_profile', (None, 'PARAMS', 'STORE', P, P, 1, None, None)), 'null argument'),
      ('outputs-null-handle', ('dqz_qr_outputs', (None, P, P, P, P, P, None)), 'null argument'),
      ('debug-null-handle', ('dqz_qr_debug', (None, P, P, None)), 'null argument'),
      ('forward-null-handle', ('dqz_qr_forward', (None, P, P, 1, P, None)), 'null argument'),
      ('forward-slots-null-handle', ('dqz_qr_forward_slots', (None, P, 'STORE', P, 1, 0, P, None)),
       'null argument'),
      ('act-null-handle', ('dqz_qr_act', (None, P, P, 1, 0.1, 0, 0, P, None)), 'null argument'),
      ('learner-null-handle', ('dqz_qr_learner', (None, out)), 'null argument'),
  ]


_REFUSALS = _refusals()


@pytest.mark.parametrize('call,fragment', [r[1:] for r in _REFUSALS], ids=[r[0] for r in _REFUSALS])
def test_refused_before_any_device_call(lib, call, fragment):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  params, store = _native.DqzParams(), _native.DqzStore()  # every pointer null
  named = {'PARAMS': ctypes.byref(params), 'STORE': ctypes.byref(store)}
  entry, args = call
  args = [named.get(x, x) if isinstance(x, str) else x for x in args]
  assert getattr(lib, entry)(*args) == INVALID
  assert fragment.encode() in lib.dqz_last_error(), lib.dqz_last_error()


def test_the_widest_shapes_have_a_layout(lib):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  for a, n in ((18, 201), (16, 256), (1, 1), (32, 128)):
    offs, sizes, total = _native.qr_param_layout(a, n)
    assert sizes[8:] == [512 * a * n, a * n] and total >= offs[9] + a * n


_STEP_REFUSALS = [
    ('weights', 8, 'the quantile head takes no importance weights'),
    ('per_draw', 8, 'the quantile head takes no prioritized draw'),
    ('uniform_draw', 8, 'the quantile head takes no in-launch batch draw'),
    ('logit_draw', 8, 'the quantile head takes no in-launch batch draw'),
    ('exact_draw', 8, 'the quantile head takes no in-launch batch draw'),
    ('meta_p', 8, 'the quantile head takes no MGSC meta mode'),
    ('meta_epi', 8, 'the quantile head takes no MGSC meta mode'),
    ('meta_softmax', 8, 'the quantile head takes no MGSC meta mode'),
    ('unit', 8, 'the quantile head takes no unit-cotangent pass'),
    ('write_back', 8, 'the quantile head takes no PER priority write-back'),
    ('fused_rmsprop', 8, 'the quantile head takes no fused centered RMSProp (it runs in gradient mode only)'),
    (None, 1, 'the quantile head needs batch >= 2'),
]


@pytest.mark.parametrize('mode,batch,message', _STEP_REFUSALS, ids=[r[0] or 'batch-one' for r in _STEP_REFUSALS])
def test_check_step_refuses_what_the_quantile_head_does_not_take(lib, mode, batch, message):
  """check_step on host structures alone (dqz_qr_debug_check): each mode has
  its own message, and the plain quantile request passes."""
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  assert set(_native.C51_REQ) == {r[0] for r in _STEP_REFUSALS if r[0]}  # every request bit is tried
  assert lib.dqz_qr_debug_check(8, 0) == 0
  assert lib.dqz_qr_debug_check(batch, _native.C51_REQ[mode] if mode else 0) == INVALID
  assert lib.dqz_last_error() == message.encode()


class _Replay:
  capacity = 1000


def _agent(optimizer=None, huber_param=1.0, quantiles=None, n=201):
  from dqn_mgsc_zoo_amd import networks
  from dqn_mgsc_zoo_amd.qrdqn import agent as agent_lib
  tau = qr_ref.make_quantiles(n)
  return agent_lib.QrDqn(
      preprocessor=None, sample_network_input=np.zeros((84, 84, 4), np.uint8),
      network=networks.qr_atari_network(6, tau), quantiles=tau if quantiles is None else quantiles,
      optimizer=optimizer, transition_accumulator=None, replay=_Replay(), batch_size=8,
      exploration_epsilon=lambda t: 0.1, min_replay_capacity_fraction=0.05, learn_period=2,
      target_network_update_period=4, huber_param=huber_param, rng_key=np.array([0, 1], np.uint32), device='cpu')


def test_centered_rmsprop_and_huber_zero_are_refused_by_name(lib):
  """Before any device allocation: the constructors' first checks."""
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import networks
  net = networks.qr_atari_network(6, qr_ref.make_quantiles(201))
  centered = learner_lib.rmsprop(5e-5, 0.95, 1e-5, centered=True)
  with pytest.raises(NotImplementedError, match='centered'):
    learner_lib.QrLearner(net, 8, optimizer=centered, device='cpu')
  with pytest.raises(NotImplementedError, match='centered'):
    _agent(optimizer=centered)
  with pytest.raises(NotImplementedError, match=r'huber_param = 0 .* is not built'):
    learner_lib.QrLearner(net, 8, huber_param=0, device='cpu')
  with pytest.raises(NotImplementedError, match=r'huber_param = 0 .* is not built'):
    _agent(huber_param=0.0)
  with pytest.raises(ValueError, match='huber_param must be finite and > 0'):
    learner_lib.QrLearner(net, 8, huber_param=-1.0, device='cpu')
  with pytest.raises(ValueError, match='qr_atari_network'):
    learner_lib.QrLearner(networks.dqn_atari_network(6), 8, device='cpu')
  with pytest.raises(ValueError, match='quantiles differ from the network'):
    _agent(quantiles=qr_ref.make_quantiles(200))
  shifted = qr_ref.make_quantiles(201).copy()
  shifted[3] = np.nextafter(shifted[3], np.float32(1))
  with pytest.raises(ValueError, match='quantiles differ from the network'):
    _agent(quantiles=shifted)


def test_network_spec_surface(lib):
  from dqn_mgsc_zoo_amd import networks
  tau = qr_ref.make_quantiles(201)
  assert tau.dtype == np.float32 and tau[0] == np.float32(0.5 / 201) and tau[-1] < 1
  net = networks.qr_atari_network(6, tau)
  assert net.num_quantiles == 201 and net.num_actions == 6 and np.array_equal(net.quantiles, tau)
  assert net.quantiles.dtype == np.float32 and not net.shared_bias
  assert net.leaf_paths() == networks.dqn_atari_network(6).leaf_paths()
  assert net.leaf_shapes()[8:] == [(512, 1206), (1206,)]
  offs, sizes, total = net.layout()
  o6, s6, _ = networks.dqn_atari_network(6).layout()
  assert offs[:9] == o6[:9] and sizes[:8] == s6[:8] and sizes[8:] == [512 * 1206, 1206]
  assert total % 64 == 0 and total >= offs[9] + 1206
  tree = net.init(0)
  back = net.unflatten(net.flatten(tree))
  for m in tree:
    for k in tree[m]:
      assert np.array_equal(tree[m][k], back[m][k])
  assert networks.QRNetworkOutputs._fields == ('q_values', 'q_dist')
  for bad in ([0.0, 0.5], [0.5, 1.0], [0.5, float('nan')]):
    with pytest.raises(ValueError, match=r'strictly inside \(0, 1\)'):
      networks.qr_atari_network(6, bad)
  with pytest.raises(ValueError, match='num_quantiles < 1'):
    networks.qr_atari_network(6, [])



# -- the input conditions of the GPU tests' corner shapes, without a GPU ---------

def _corner_ids():
  from tests import test_qr_gpu as gpu  # pylint: disable=g-import-not-at-top
  return gpu.CORNERS


@pytest.mark.parametrize('shape', _corner_ids(), ids=lambda s: '%dx%dx%d-kappa%g' % s)
def test_corner_shapes_meet_their_input_conditions(lib, shape):
  """tests/test_qr_gpu.py's _check_conditions on each corner shape's pinned
  seed, in float64 on the CPU: every condition but the ones WAIVED names for
  that shape, and each waiver is one the shape makes impossible (or, for the
  kink-free draw, one its tests do not need)."""
  from tests import test_qr_gpu as gpu  # pylint: disable=g-import-not-at-top
  b, a, n, kappa = shape
  case = gpu._case(*shape)  # pylint: disable=protected-access
  gpu._check_conditions(case)  # pylint: disable=protected-access
  waived = gpu.WAIVED.get(shape, set())
  for what in ('absent action', 'best action not 0', 'margin'):
    assert (what in waived) == (a == 1), what
  assert ('both signs' in waived) == (n == 1)
  assert ('kink-free draw' in waived) == (shape in gpu.STAGE_ONLY)
  assert waived <= {'absent action', 'best action not 0', 'margin', 'both signs', 'kink-free draw'}
  assert len(case['slots']) == b and case['slots'][0] == gpu.SPECIAL and kappa == gpu.KAPPA
  if shape not in gpu.STAGE_ONLY:  # the end-to-end step's batch is kink-free
    s = helpers.stacks_from(case['host']['frames'], case['host']['fidx'], case['slots'], 0)
    assert learner_ref.relu_margin(case['online'], s) >= 1e-6
  assert a * n <= 4096 and 1 <= n <= 256 and 1 <= a <= 32 and 2 <= b <= 256
