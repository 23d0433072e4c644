"""CPU: the C51 restatement (tests/c51_ref.py) against independent
implementations, and the categorical entries' refusals that run before any
device call.

  projection  against the C51 paper's Algorithm 1 (each y_i's mass split
              between its floor and ceil atom) on an equally spaced float64
              support, N in {5, 7, 51}: mass sum 1 and agreement within 1e-12.
  loss        and d loss / d logits against torch autograd in float64 on the
              head alone (h1 -> logits -> loss), then the whole network's
              gradient at B = 2, A = 3, N = 5.
"""

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import learner_ref
from tests import c51_ref
from tests import helpers

INVALID = -1  # DQZ_ERR_INVALID


def _paper_projection(r, d, probs, vmin, vmax, n):
  """Algorithm 1 of Bellemare et al. 2017 for one transition."""
  dz = (vmax - vmin) / (n - 1)
  z = vmin + dz * np.arange(n)
  m = np.zeros(n)
  for j in range(n):
    tz = min(max(r + d * z[j], vmin), vmax)
    b = (tz - vmin) / dz
    lo, up = int(np.floor(b)), int(np.ceil(b))
    if lo == up:  # on an atom: the two weights of the paper's loop are both 0
      m[lo] += probs[j]
    else:
      m[lo] += probs[j] * (up - b)
      m[up] += probs[j] * (b - lo)
  return m


@pytest.mark.parametrize('n', [5, 7, 51])
def test_projection_matches_the_paper_loop(n):
  vmax = 10.0
  z = np.linspace(-vmax, vmax, n)
  dz = 2 * vmax / (n - 1)
  rng = np.random.default_rng(n)
  cases = [
      ('d=0, r between atoms', 0.37 * dz, 0.0),
      ('d=0, r on an atom', float(z[n // 2 + 1]), 0.0),
      ('d=0, r on the last atom', vmax, 0.0),
      ('beyond the upper end', 1.0 + vmax, 0.99),
      ('beyond both ends', 0.0, 3.0),
      ('beyond the lower end', -3.0 * vmax, 0.5),
      ('plain', 1.0, 0.99),
      ('plain negative', -1.0, 0.99),
      ('terminal reward 1', 1.0, 0.0),
  ]
  for what, r, d in cases:
    for trial in range(3):
      p = rng.random(n) ** 3 + 1e-9
      p /= p.sum()
      m = c51_ref.project(r + d * z, p, z)
      want = _paper_projection(r, d, p, -vmax, vmax, n)
      assert abs(m.sum() - 1.0) <= 1e-12, (what, trial, m.sum())
      assert np.abs(m - want).max() <= 1e-12, (what, trial, np.abs(m - want).max())
      assert (m >= 0).all()
  # every y_i on or beyond the last atom: all of the mass lands there
  m = c51_ref.project(vmax + 1.0 + 0.99 * np.abs(z), np.full(n, 1.0 / n), z)
  assert m[-1] == pytest.approx(1.0, abs=1e-12) and np.abs(m[:-1]).max() == 0.0


def test_projection_takes_an_unequal_support():
  """No equal spacing is assumed: mass is conserved and the mean is kept for
  targets inside the support (the projection is linear interpolation)."""
  z = np.array([-3.0, -1.0, -0.5, 0.25, 4.0])
  rng = np.random.default_rng(0)
  p = rng.random(5)
  p /= p.sum()
  y = 0.3 + 0.5 * z  # inside [-3, 4]
  m = c51_ref.project(y, p, z)
  assert abs(m.sum() - 1.0) <= 1e-12
  assert abs(m @ z - p @ y) <= 1e-12


def _torch_loss(logits_tm1, a_tm1, m):
  """mean_b -sum_k m[b, k] log_softmax(logits_tm1[b, a_b])[k], torch float64."""
  idx = torch.arange(logits_tm1.shape[0])
  la = logits_tm1[idx, torch.as_tensor(a_tm1, dtype=torch.long)]
  return -(torch.as_tensor(m) * F.log_softmax(la, dim=-1)).sum(-1).mean()


@pytest.mark.parametrize('b,a,n', [(4, 3, 5), (8, 6, 51)])
def test_loss_and_dlogits_match_autograd_on_the_head(b, a, n):
  rng = np.random.default_rng(b + n)
  z = np.linspace(-10.0, 10.0, n)
  h1 = np.maximum(rng.standard_normal((b, 512)), 0.0)
  w = rng.uniform(-1, 1, (512, a * n)) / np.sqrt(512)
  bias = rng.uniform(-1, 1, a * n) / np.sqrt(512)
  logits_t = rng.standard_normal((b, a, n))
  a_tm1 = rng.integers(0, a, b)
  r = rng.choice([-1.0, 0.0, 1.0], b)
  d = 0.99 * (rng.random(b) > 0.3)
  res = c51_ref.categorical_loss((h1 @ w + bias).reshape(b, a, n), a_tm1, r, d, logits_t, z)
  # the target side, independently: torch softmax, argmax, the paper's projection
  pt = F.softmax(torch.as_tensor(logits_t), dim=-1)
  a_star = (pt @ torch.as_tensor(z)).argmax(dim=1).numpy()
  assert np.array_equal(a_star, res['a_star'])
  m = np.stack([_paper_projection(r[i], d[i], pt[i, a_star[i]].numpy(), -10.0, 10.0, n) for i in range(b)])
  np.testing.assert_allclose(res['m'], m, atol=1e-12)
  th1, tw, tb = (torch.tensor(x, requires_grad=True) for x in (h1, w, bias))
  logits = (th1 @ tw + tb).reshape(b, a, n)
  logits.retain_grad()
  loss = _torch_loss(logits, a_tm1, m)
  loss.backward()
  assert abs(loss.item() - res['loss']) <= 1e-12 * max(1.0, abs(res['loss']))
  np.testing.assert_allclose(res['dlogits'], logits.grad.numpy(), atol=1e-14)
  dense = res['dlogits'].reshape(b, -1)
  np.testing.assert_allclose(h1.T @ dense, tw.grad.numpy(), atol=1e-13)
  np.testing.assert_allclose(dense.sum(0), tb.grad.numpy(), atol=1e-13)
  np.testing.assert_allclose(dense @ w.T, th1.grad.numpy(), atol=1e-13)
  np.testing.assert_allclose(res['dl'].sum(-1), 0.0, atol=1e-15)  # sum m = sum softmax = 1


def test_whole_network_gradient_matches_autograd():
  from dqn_mgsc_zoo_amd import networks
  b, a, n = 2, 3, 5
  z = c51_ref.make_support(10.0, n)
  net = networks.c51_atari_network(a, z)
  online = net.init(1)
  target = helpers.perturbed_tree(online, 2)
  rng = np.random.default_rng(3)
  s_tm1 = rng.integers(0, 256, (b, 84, 84, 4), dtype=np.uint8)
  s_t = rng.integers(0, 256, (b, 84, 84, 4), dtype=np.uint8)
  a_tm1, r, d = np.array([2, 0]), np.array([1.0, -1.0]), np.array([0.99, 0.0])
  res = c51_ref.learner_grads(online, target, s_tm1, a_tm1, r, d, s_t, z, a)

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
    return (h @ params[head + '/linear_1']['w'] + params[head + '/linear_1']['b']).reshape(-1, a, n)

  with torch.no_grad():
    tt = {m: {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in leaves.items()}
          for m, leaves in target.items()}
    logits_t = apply(tt, s_t)
  np.testing.assert_allclose(res['logits_target_t'], logits_t.numpy(), atol=1e-12)
  loss = _torch_loss(apply(tp, s_tm1), a_tm1, res['m'])
  loss.backward()
  assert abs(loss.item() - res['loss']) <= 1e-12
  for m in online:
    for k in online[m]:
      got, want = res['grads'][m][k], tp[m][k].grad.numpy()
      assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (m, k)
  assert np.abs(res['grads'][head + '/linear_1']['w']).max() > 0


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
  return _native.DqzLearnerConfig(batch, num_actions, algo, 2.5e-4, 0.0, 1e-4, 0.0)


def _ocfg(num_actions=6, shared=0, kind=0):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  return _native.DqzOptimizerConfig(kind, 2.5e-4, 0.9, 0.999, 0.9, 1e-4, 10.0, num_actions, shared)


def _refusals():
  h = ctypes.c_void_p()
  out = ctypes.byref(h)
  i64 = (ctypes.c_int64 * 10)()
  tot = ctypes.byref(ctypes.c_int64())
  create = lambda cfg, n, sup=P: ('dqz_c51_create', (ctypes.byref(cfg), n, sup, out))
  opt = lambda cfg, n: ('dqz_c51_optimizer_create', (ctypes.byref(cfg), n, out))
  layout = lambda a, n, o=i64: ('dqz_c51_param_layout', (a, n, o, i64, tot))
  return [
      ('create-null-config', ('dqz_c51_create', (None, 51, P, out)), 'null argument'),
      ('create-null-support', create(_cfg(), 51, None), 'null argument'),
      ('create-null-out', ('dqz_c51_create', (ctypes.byref(_cfg()), 51, P, None)), 'null argument'),
      ('create-one-atom', create(_cfg(), 1), 'num_atoms must be in [2, 64]'),
      ('create-too-many-atoms', create(_cfg(), 65), 'num_atoms must be in [2, 64]'),
      ('create-too-wide', create(_cfg(num_actions=18), 57), 'num_actions * num_atoms must be <= 1024'),
      ('create-no-actions', create(_cfg(num_actions=0), 51), 'num_actions must be in [1, 32]'),
      ('create-batch-one', create(_cfg(batch=1), 51), 'batch must be in [2, 256]'),
      # the first value past each limit (N = 65 and batch 1 are above)
      ('create-a-n-1025', create(_cfg(num_actions=25), 41), 'num_actions * num_atoms must be <= 1024'),
      ('create-33-actions', create(_cfg(num_actions=33), 31), 'num_actions must be in [1, 32]'),
      ('create-batch-257', create(_cfg(batch=257), 51), 'batch must be in [2, 256]'),
      ('create-double-q', create(_cfg(algo=1), 51), 'the categorical head runs on a DQN learner'),
      ('layout-one-atom', layout(6, 1), 'num_atoms must be in [2, 64]'),
      ('layout-too-wide', layout(32, 33), 'num_actions * num_atoms must be <= 1024'),
      ('layout-null-out', layout(6, 51, None), 'null output pointer'),
      ('optimizer-null-config', ('dqz_c51_optimizer_create', (None, 51, out)), 'null argument'),
      ('optimizer-one-atom', opt(_ocfg(), 1), 'num_atoms must be in [2, 64]'),
      ('optimizer-too-wide', opt(_ocfg(num_actions=21), 51), 'num_actions * num_atoms must be <= 1024'),
      ('optimizer-shared-bias', opt(_ocfg(shared=1), 51), 'the categorical head has no shared bias'),
      ('optimizer-kind', opt(_ocfg(kind=2), 51), 'optimizer kind must be DQZ_OPT_ADAM or DQZ_OPT_RMSPROP'),
      ('step-null-handle', ('dqz_c51_step', (None, 'PARAMS', 'STORE', P, P, P, None)), 'null argument'),
      ('step-null-optimizer', ('dqz_c51_step', (P, 'PARAMS', 'STORE', P, None, P, None)), 'null argument'),
      ('step-null-state', ('dqz_c51_step', (P, 'PARAMS', 'STORE', P, P, P, None)), 'null optimizer state'),
      ('grad-null-handle', ('dqz_c51_grad', (None, 'PARAMS', 'STORE', P, P, None)), 'null argument'),
      ('grad-null-out', ('dqz_c51_grad', (P, 'PARAMS', 'STORE', P, None, None)), 'null grad_out'),
      ('outputs-null-handle', ('dqz_c51_outputs', (None, P, P, P, P, P, None)), 'null argument'),
      ('forward-null-handle', ('dqz_c51_forward', (None, P, P, 1, P, None)), 'null argument'),
      ('forward-null-states', ('dqz_c51_forward', (P, P, None, 1, P, None)), 'null argument'),
      ('forward-slots-null-slots', ('dqz_c51_forward_slots', (P, P, 'STORE', None, 1, 0, P, None)),
       'null argument'),
      ('act-null-out', ('dqz_c51_act', (P, P, P, 1, 0.1, 0, 0, None, None)), 'null argument'),
      ('learner-null-handle', ('dqz_c51_learner', (None, out)), 'null argument'),
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


_STEP_REFUSALS = [
    ('weights', 8, 'the categorical head takes no importance weights'),
    ('per_draw', 8, 'the categorical head takes no prioritized draw'),
    ('uniform_draw', 8, 'the categorical head takes no in-launch batch draw'),
    ('logit_draw', 8, 'the categorical head takes no in-launch batch draw'),
    ('exact_draw', 8, 'the categorical head takes no in-launch batch draw'),
    ('meta_p', 8, 'the categorical head has no MGSC meta mode'),
    ('meta_epi', 8, 'the categorical head has no MGSC meta mode'),
    ('meta_softmax', 8, 'the categorical head has no MGSC meta mode'),
    ('unit', 8, 'the categorical head has no unit-cotangent pass'),
    ('write_back', 8, 'the categorical head has no TD error to write back as a priority'),
    ('fused_rmsprop', 8, 'the categorical head runs in gradient mode only (no fused centered RMSProp)'),
    (None, 1, 'the categorical head needs batch >= 2'),
]


@pytest.mark.parametrize('mode,batch,message', _STEP_REFUSALS, ids=[r[0] or 'batch-one' for r in _STEP_REFUSALS])
def test_check_step_refuses_what_the_categorical_head_does_not_take(lib, mode, batch, message):
  """check_step on host structures alone (dqz_c51_debug_check): each mode has
  its own message, and the plain categorical request passes."""
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  assert lib.dqz_c51_debug_check(8, 0) == 0
  assert lib.dqz_c51_debug_check(batch, _native.C51_REQ[mode] if mode else 0) == INVALID
  assert lib.dqz_last_error() == message.encode()


def test_centered_rmsprop_is_refused_by_name(lib):
  """Before any device allocation: the constructor's first check."""
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import networks
  net = networks.c51_atari_network(6, c51_ref.make_support(10.0, 51))
  with pytest.raises(NotImplementedError, match='centered'):
    learner_lib.C51Learner(net, 8, optimizer=learner_lib.rmsprop(2.5e-4, 0.95, 1e-5, centered=True),
                           device='cpu')
  with pytest.raises(ValueError, match='c51_atari_network'):
    learner_lib.C51Learner(networks.dqn_atari_network(6), 8, device='cpu')


def test_network_spec_surface(lib):
  from dqn_mgsc_zoo_amd import networks
  z = c51_ref.make_support(10.0, 51)
  net = networks.c51_atari_network(6, z)
  assert net.num_atoms == 51 and net.num_actions == 6 and np.array_equal(net.support, z)
  assert net.leaf_paths() == networks.dqn_atari_network(6).leaf_paths()
  assert net.leaf_shapes()[8:] == [(512, 306), (306,)]
  offs, sizes, total = net.layout()
  o6, s6, _ = networks.dqn_atari_network(6).layout()
  assert offs[:9] == o6[:9] and sizes[:8] == s6[:8] and sizes[8:] == [512 * 306, 306]
  assert total % 64 == 0 and total >= offs[9] + 306
  tree = net.init(0)
  back = net.unflatten(net.flatten(tree))
  for m in tree:
    for k in tree[m]:
      assert np.array_equal(tree[m][k], back[m][k])
  with pytest.raises(ValueError, match='strictly increasing'):
    networks.c51_atari_network(6, [0.0, 1.0, 1.0])
  with pytest.raises(ValueError, match='num_atoms < 2'):
    networks.c51_atari_network(6, [0.0])


# -- the input conditions of the GPU tests' corner shapes, without a GPU ---------

def _corner_ids():
  from tests import test_c51_gpu as gpu  # pylint: disable=g-import-not-at-top
  return gpu.CORNERS


@pytest.mark.parametrize('shape', _corner_ids(), ids=lambda s: '%dx%dx%d' % s)
def test_corner_shapes_meet_their_input_conditions(lib, shape):
  """tests/test_c51_gpu.py's _check_conditions on each corner shape's pinned
  seed, in float64 on the CPU: every condition but the ones WAIVED names for
  that shape, and each waiver is one the shape makes impossible (or, for the
  kink-free draw, one its tests do not need)."""
  from tests import test_c51_gpu as gpu  # pylint: disable=g-import-not-at-top
  b, a, n = shape
  case = gpu._case(*shape)  # pylint: disable=protected-access
  gpu._check_conditions(case)  # pylint: disable=protected-access
  waived = gpu.WAIVED.get(shape, set())
  assert ('absent action' in waived) == (a == 1) and ('margin' in waived) == (a == 1)
  assert ('kink-free draw' in waived) == (shape in gpu.STAGE_ONLY)
  assert waived <= {'absent action', 'margin', 'kink-free draw'}
  assert len(case['slots']) == b and case['slots'][0] == gpu.SPECIAL
  if shape not in gpu.STAGE_ONLY:  # the end-to-end step's batch is kink-free
    s = helpers.stacks_from(case['host']['frames'], case['host']['fidx'], case['slots'], 0)
    assert learner_ref.relu_margin(case['online'], s) >= 1e-6
  assert a * n <= 1024 and 2 <= n <= 64 and 1 <= a <= 32 and 2 <= b <= 256
