"""GPU: Adam, plain RMSProp and clip_by_global_norm on the learner's finished
gradient (csrc/optim.hpp, dqz_optimizer_* and dqz_learner_step_opt*).

Shapes: B = 8, capacity 256, 640 frames (tests/test_learner_gpu.py's store).
The reference is tests/optim_ref.py (float64) on the device's own float32
inputs, with the hyper-parameters rounded to float32 as the C ABI carries them.

Bounds of the injected-gradient test, per element, u the float64 update:
  |theta_dev - theta_ref| <= 2^-23 |theta| + 2^-20 |u|   (<= 8 roundings)
  |m_dev - m_ref| <= 2^-22 max(|b m|, |(1 - b) g|) + 2^-150, likewise v, nu.
The 2^-150 is half the smallest float32 subnormal: with the +-1e-30 gradients
the test injects, (1 - b2) g^2 = 1e-63 has no float32 representation at all,
so the stored moment is its nearest float32 (0), not a relative-error result.

End-to-end bars are the project's: q / td atol 1e-4, loss rtol 1e-4, params
atol 2e-6, moments rtol 1e-3 (atol 2e-9 for m = 0.1 g and 1e-12 for v: the
1e-9 / 1e-12 of tests/test_learner_gpu.py on mu = 0.05 g, scaled by the
coefficient of g).
"""

import copy
import ctypes

import numpy as np
import pytest
import torch

from oracle import learner_ref
from tests import fake_env
from tests import helpers
from tests import optim_ref
from tests.test_trajectory_gpu import _batch
from tests.test_trajectory_gpu import _state

pytestmark = pytest.mark.gpu

LR, ADAM_EPS = 2.5e-4, 0.01 / 32  # c51/run_atari.py:80-81
B1, B2 = 0.9, 0.999
BATCH = 8


def _f32(x):
  return float(np.float32(x))


def _setup(algo, optimizer, seed, batch=BATCH, num_actions=6):
  """tests/test_learner_gpu.py's _setup with an optimizer."""
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import networks
  from dqn_mgsc_zoo_amd import store as store_lib
  net = (networks.dqn_atari_network(num_actions) if algo == 'dqn' else
         networks.double_dqn_atari_network(num_actions))
  online = net.init(seed)
  target = helpers.perturbed_tree(online, seed + 1)
  lrn = learner_lib.Learner(net, batch, algo=algo, optimizer=optimizer)
  lrn.set_params(online, target)
  frames, fidx, action, reward, discount = helpers.random_store_contents(
      256, 640, num_actions, seed + 3)
  st = store_lib.FrameStore(256, 640)
  for name, arr in (('frames', frames), ('fidx', fidx), ('action', action),
                    ('reward', reward), ('discount', discount)):
    getattr(st, name).copy_(torch.from_numpy(arr))
  host = dict(frames=frames, fidx=fidx, action=action, reward=reward, discount=discount)
  return lrn, st, host, online, target


def _adam(eps=ADAM_EPS, clip=None):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  opt = learner_lib.adam(LR, B1, B2, eps)
  return opt if clip is None else learner_lib.chain(learner_lib.clip_by_global_norm(clip), opt)


class _Handle:
  """A dqz_optimizer of its own, for the stand-alone apply."""

  def __init__(self, kind, num_actions, shared, lr=LR, b1=B1, b2=B2, decay=0.95, eps=1e-8, clip=0.0, wide=None):
    """wide: ('c51' | 'qr', N) for a handle over a wide head's layout (dqz_c51_optimizer_create /
    dqz_qr_optimizer_create: fc2 is [512, A N] + [A N])."""
    from dqn_mgsc_zoo_amd import _native
    self.n = _native
    cfg = _native.DqzOptimizerConfig(kind, lr, b1, b2, decay, eps, clip, num_actions, int(shared))
    self.h = ctypes.c_void_p()
    if wide is None:
      _native.check(_native.lib().dqz_optimizer_create(ctypes.byref(cfg), ctypes.byref(self.h)))
    else:
      create = getattr(_native.lib(), 'dqz_%s_optimizer_create' % wide[0])
      _native.check(create(ctypes.byref(cfg), int(wide[1]), ctypes.byref(self.h)))

  def apply(self, th, g, m, v, count):
    n = self.n
    n.check(n.lib().dqz_optimizer_apply(self.h, n.ptr(th), n.ptr(g), n.ptr(m), n.ptr(v), n.ptr(count),
                                        n.stream_handle()))

  def norm(self):
    out = torch.zeros((1,), dtype=torch.float32, device='cuda')
    self.n.check(self.n.lib().dqz_optimizer_outputs(self.h, self.n.ptr(out), self.n.stream_handle()))
    return out

  def close(self):
    if self.h.value:
      self.n.lib().dqz_optimizer_destroy(self.h)
      self.h = ctypes.c_void_p()


def _real_mask(num_actions, shared, wide=None):
  from dqn_mgsc_zoo_amd import _native
  if wide is None:
    offs, sizes, total = _native.param_layout(num_actions, shared)
  else:
    offs, sizes, total = getattr(_native, wide[0] + '_param_layout')(num_actions, wide[1])
  real = np.zeros(total, bool)
  for o, s in zip(offs, sizes):
    real[o:o + s] = True
  return real


def _injected_grad(rng, real):
  """Random magnitudes over six decades with exact zeros, +-1e-30 and 1e4
  entries; the padding holds a value the apply must ignore."""
  n = real.size
  g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
  r = rng.random(n)
  g[r < 0.10] = 0.0
  g[(r >= 0.10) & (r < 0.13)] = 1e-30
  g[(r >= 0.13) & (r < 0.16)] = -1e-30
  g[(r >= 0.16) & (r < 0.17)] = 1e4
  g[~real] = 7.0
  return g


def _start_state(rng, real):
  n = real.size
  th = (0.05 * rng.standard_normal(n)).astype(np.float32)
  m = (1e-3 * rng.standard_normal(n)).astype(np.float32)
  v = (m.astype(np.float64) ** 2 + 1e-6 * rng.random(n)).astype(np.float32)
  fresh = rng.random(n) < 0.3  # a third of the elements start from zero moments
  m[fresh] = 0.0
  v[fresh] = 0.0
  for a in (th, m, v):
    a[~real] = 0.0
  return th, m, v


def _check_theta(got, want, prev, what):
  """|theta_dev - theta_ref| <= 2^-23 |theta| + 2^-20 |u|."""
  u = np.abs(prev.astype(np.float64) - want)
  err = np.abs(got.astype(np.float64) - want)
  bound = 2.0**-23 * np.abs(prev.astype(np.float64)) + 2.0**-20 * u
  worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
  print('%s: theta err / bound at most %.3f (err %.3e, u %.3e)' % (
      what, err[worst] / max(bound[worst], 1e-300), err[worst], u[worst]))
  assert (err <= bound).all(), (what, worst, err[worst], bound[worst])


def _check_moment(got, want, prev, g, b, power, what):
  """Within 2^-22 of the larger summand of b prev + (1 - b) g^power (+ 2^-150)."""
  larger = np.maximum(np.abs(b * prev.astype(np.float64)), np.abs((1.0 - b) * g.astype(np.float64) ** power))
  err = np.abs(got.astype(np.float64) - want)
  bound = 2.0**-22 * larger + 2.0**-150
  worst = int(np.argmax(err / bound))
  print('%s: err / bound at most %.3f (err %.3e)' % (what, err[worst] / bound[worst], err[worst]))
  assert (err <= bound).all(), (what, worst, err[worst], bound[worst])


def _bits(t):
  return t.detach().cpu().numpy().view(np.int32)


# The ends of the layout: 1 and 32 actions (dqz_optimizer_create's limits; with a shared bias the last leaf
# is one float whatever A is), and through the wide heads' creates A N = 2 (the smallest fc2 either takes),
# 1024 (the categorical head's limit) and 4096 (the quantile head's).
WIDE_LAYOUTS = [('c51', 1, 2), ('qr', 2, 1), ('c51', 16, 64), ('qr', 16, 256)]


@pytest.mark.parametrize('wide', WIDE_LAYOUTS, ids=lambda w: '%s-%dx%d' % w)
@pytest.mark.parametrize('kind,eps', [('adam', ADAM_EPS), ('rmsprop', 1e-8)])
def test_apply_from_injected_gradients_on_wide_layouts(device, kind, eps, wide):
  """test_apply_from_injected_gradients on the layouts of dqz_c51_param_layout /
  dqz_qr_param_layout, against tests/optim_ref.py at the same bars."""
  head, a, n = wide
  test_apply_from_injected_gradients(device, kind, eps, a, False, wide=(head, n))


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('num_actions', [1, 3, 6, 18, 32])
@pytest.mark.parametrize('kind,eps', [('adam', 1e-8), ('adam', ADAM_EPS), ('rmsprop', 1e-8)])
def test_apply_from_injected_gradients(device, kind, eps, num_actions, shared, wide=None):
  from dqn_mgsc_zoo_amd import _native
  real = _real_mask(num_actions, shared, wide)
  assert real.size % 64 == 0 and not real.all()  # every layout here has padding for the apply to skip
  rng = np.random.default_rng(100 + num_actions + int(shared) + (0 if wide is None else wide[1]))
  th0, m0, v0 = _start_state(rng, real)
  th, m, v = (torch.from_numpy(a).to(device) for a in (th0, m0, v0))
  count = torch.zeros((1,), dtype=torch.int32, device=device)
  is_adam = kind == 'adam'
  lr, b1, b2, decay, e = _f32(LR), _f32(B1), _f32(B2), _f32(0.95), _f32(eps)
  h = _Handle(_native.OPT_ADAM if is_adam else _native.OPT_RMSPROP, num_actions, shared, eps=eps, wide=wide)
  try:
    for step in range(3):
      g_np = _injected_grad(rng, real)
      prev = [a.cpu().numpy() for a in (th, m, v)]
      h.apply(th, torch.from_numpy(g_np).to(device), m, v, count)
      torch.cuda.synchronize()
      got = [a.cpu().numpy() for a in (th, m, v)]
      what = '%s eps %g A %d shared %d step %d' % (kind, eps, num_actions, shared, step)
      if is_adam:
        t_ref, m_ref, v_ref, _ = optim_ref.adam(prev[0], g_np, prev[1], prev[2], step, lr, b1, b2, e)
        _check_moment(got[1][real], m_ref[real], prev[1][real], g_np[real], b1, 1, what + ' m')
        _check_moment(got[2][real], v_ref[real], prev[2][real], g_np[real], b2, 2, what + ' v')
      else:
        t_ref, v_ref = optim_ref.rmsprop(prev[0], g_np, prev[2], lr, decay, e)
        _check_moment(got[2][real], v_ref[real], prev[2][real], g_np[real], decay, 2, what + ' nu')
        assert np.array_equal(got[1].view(np.int32), prev[1].view(np.int32))  # mu is not RMSProp's
      _check_theta(got[0][real], t_ref[real], prev[0][real], what)
      assert np.isfinite(got[0]).all()
      for a in got:  # padding stays bit-zero
        assert not a.view(np.int32)[~real].any()
    assert int(count.item()) == (3 if is_adam else 0)
  finally:
    h.close()


@pytest.mark.parametrize('seed,want', [(3, 0.110), (11, 0.145)])
def test_global_norm_and_clip(device, seed, want):
  from dqn_mgsc_zoo_amd import _native
  lrn, st, host, online, _ = _setup('dqn', _adam(clip=10.0), seed)
  slots = helpers.kink_free_slots(online, host, st.capacity, BATCH, np.random.default_rng(5))
  slots_d = torch.from_numpy(slots).to(device)
  g = lrn.grad(st, slots_d)
  real = _real_mask(6, False)
  g_np = g.cpu().numpy()
  norm64 = float(np.sqrt(np.sum(g_np[real].astype(np.float64) ** 2)))
  print('seed %d: gradient norm %.6f' % (seed, norm64))
  assert abs(norm64 - want) < 5e-4  # the oracle's, computed on the CPU
  th0, m0, v0 = lrn.online.clone(), lrn.mu.clone(), lrn.nu.clone()
  # the step's own norm (clip inactive at 10) and its update = unclipped Adam's
  lrn.step(st, slots_d)
  gn = lrn.grad_norm().clone()
  torch.cuda.synchronize()
  assert abs(float(gn.item()) - norm64) <= 2.0**-22 * norm64
  plain = _Handle(_native.OPT_ADAM, 6, False, eps=ADAM_EPS)
  loose = _Handle(_native.OPT_ADAM, 6, False, eps=ADAM_EPS, clip=10.0)
  tight = _Handle(_native.OPT_ADAM, 6, False, eps=ADAM_EPS, clip=0.05)
  try:
    # garbage in the caller's padding does not reach the norm
    g_dirty = g.clone()
    g_dirty[torch.from_numpy(~real).to(device)] = 3.0
    outs = {}
    for name, h in (('plain', plain), ('loose', loose), ('tight', tight)):
      runs = []
      for _ in range(3):  # repeats: the same bits every time
        th, m, v = th0.clone(), m0.clone(), v0.clone()
        count = torch.zeros((1,), dtype=torch.int32, device=device)
        h.apply(th, g_dirty, m, v, count)
        runs.append((_bits(th), _bits(m), _bits(v), _bits(h.norm()), int(count.item())))
      for r in runs[1:]:
        for x, y in zip(runs[0], r):
          assert np.array_equal(x, y), name
      outs[name] = runs[0]
      assert runs[0][4] == 1
      assert np.array_equal(runs[0][3], _bits(gn)), name  # the step's norm, bit for bit
    for k in range(3):  # inactive clip: exactly the unclipped update, which is the step's
      assert np.array_equal(outs['plain'][k], outs['loose'][k])
    assert np.array_equal(outs['loose'][0], _bits(lrn.online))
    assert np.array_equal(outs['loose'][1], _bits(lrn.mu))
    assert np.array_equal(outs['loose'][2], _bits(lrn.nu))
    assert not np.array_equal(outs['tight'][0], outs['plain'][0])
    # active at 0.05: the reference's clipped gradient through Adam
    lr, b1, b2, e = _f32(LR), _f32(B1), _f32(B2), _f32(ADAM_EPS)
    g_c, n_ref = optim_ref.clip_by_global_norm(np.where(real, g_np, 0.0), _f32(0.05))
    assert abs(n_ref - norm64) < 1e-12 and abs(optim_ref.global_norm(g_c) - _f32(0.05)) < 1e-12
    prev = [a.cpu().numpy() for a in (th0, m0, v0)]
    t_ref, m_ref, v_ref, _ = optim_ref.adam(prev[0], g_c, prev[1], prev[2], 0, lr, b1, b2, e)
    got = [a.view(np.float32) for a in outs['tight'][:3]]
    _check_theta(got[0][real], t_ref[real], prev[0][real], 'clipped')
    _check_moment(got[1][real], m_ref[real], prev[1][real], g_c[real], b1, 1, 'clipped m')
    _check_moment(got[2][real], v_ref[real], prev[2][real], g_c[real], b2, 2, 'clipped v')
  finally:
    for h in (plain, loose, tight):
      h.close()


def test_global_norm_and_clip_on_a_wide_layout(device):
  """test_global_norm_and_clip's checks on the quantile head's widest layout
  (A N = 4096: an fc2 of 2 M weights, whose bias leaf fills its 64-float
  blocks exactly), from an injected gradient: the norm is the float64 norm
  of the real elements whatever the padding holds, an inactive clip changes
  no bit, an active one is the reference's clipped gradient through Adam."""
  from dqn_mgsc_zoo_amd import _native
  a, wide = 16, ('qr', 256)
  real = _real_mask(a, False, wide)
  rng = np.random.default_rng(7)
  th0, m0, v0 = _start_state(rng, real)
  g_np = (rng.standard_normal(real.size) * 10.0 ** rng.uniform(-6, -2, real.size)).astype(np.float32)
  g_np[~real] = 0.0
  norm64 = float(np.sqrt(np.sum(g_np[real].astype(np.float64) ** 2)))
  tight_clip = 0.5 * norm64
  assert norm64 < 10.0
  g_dirty = g_np.copy()
  g_dirty[~real] = 3.0  # garbage in the caller's padding does not reach the norm
  kw = dict(eps=ADAM_EPS, wide=wide)
  handles = dict(plain=_Handle(_native.OPT_ADAM, a, False, **kw), loose=_Handle(_native.OPT_ADAM, a, False, clip=10.0, **kw),
                 tight=_Handle(_native.OPT_ADAM, a, False, clip=tight_clip, **kw))
  try:
    outs = {}
    for name, h in handles.items():
      for g_host in (g_np, g_dirty):
        th, m, v = (torch.from_numpy(x).to(device) for x in (th0, m0, v0))
        count = torch.zeros((1,), dtype=torch.int32, device=device)
        h.apply(th, torch.from_numpy(g_host).to(device), m, v, count)
        run = (_bits(th), _bits(m), _bits(v), _bits(h.norm()), int(count.item()))
        if name in outs:  # dirty padding: the same bits
          for x, y in zip(outs[name], run):
            assert np.array_equal(x, y), name
        outs[name] = run
      gn = float(outs[name][3].view(np.float32)[0])
      assert abs(gn - norm64) <= 2.0**-22 * norm64, (name, gn, norm64)
      for arr in outs[name][:3]:  # the padding of theta, m and v stays bit-zero
        assert not arr[~real].any()
    for k in range(3):
      assert np.array_equal(outs['plain'][k], outs['loose'][k])
    assert not np.array_equal(outs['tight'][0], outs['plain'][0])
    lr, b1, b2, e = _f32(LR), _f32(B1), _f32(B2), _f32(ADAM_EPS)
    g_c, n_ref = optim_ref.clip_by_global_norm(g_np, _f32(tight_clip))
    assert abs(n_ref - norm64) < 1e-12
    t_ref, m_ref, v_ref, _ = optim_ref.adam(th0, g_c, m0, v0, 0, lr, b1, b2, e)
    got = [x.view(np.float32) for x in outs['tight'][:3]]
    _check_theta(got[0][real], t_ref[real], th0[real], 'wide clipped')
    _check_moment(got[1][real], m_ref[real], m0[real], g_c[real], b1, 1, 'wide clipped m')
    _check_moment(got[2][real], v_ref[real], v0[real], g_c[real], b2, 2, 'wide clipped v')
  finally:
    for h in handles.values():
      h.close()


def _compare_tree(got, want, atol, rtol=0.0, what=''):
  for m in want:
    for n in want[m]:
      np.testing.assert_allclose(got[m][n], want[m][n], atol=atol, rtol=rtol,
                                 err_msg='%s %s/%s' % (what, m, n))


def _check_step(lrn, ref, prev, count, clip, outputs, what):
  """Device outputs and state after one step against learner_ref's forward /
  backward / td_loss (ref) followed by optim_ref from the state `prev`."""
  q, td, loss = outputs
  np.testing.assert_allclose(q, ref['q_tm1'], atol=1e-4)
  np.testing.assert_allclose(td, ref['td'], atol=1e-4)
  np.testing.assert_allclose(loss[0], ref['loss'], rtol=1e-4, atol=1e-7)
  grads = ref['grads']
  if clip is not None:
    grads, norm = optim_ref.clip_by_global_norm(grads, clip)
    np.testing.assert_allclose(float(lrn.grad_norm().item()), norm, rtol=1e-4)
  p, mu, nu = prev
  t_ref, m_ref, v_ref, c_ref = optim_ref.adam(p, grads, mu, nu, count, LR, B1, B2, ADAM_EPS)
  assert int(lrn.count.item()) == c_ref
  _compare_tree(lrn.params_tree('online'), t_ref, 2e-6, what=what + ' params')
  _compare_tree(lrn.params_tree('mu'), m_ref, 2e-9, 1e-3, what=what + ' m')
  _compare_tree(lrn.params_tree('nu'), v_ref, 1e-12, 1e-3, what=what + ' v')


@pytest.mark.parametrize('algo', ['dqn', 'double', 'per'])
def test_one_adam_step_matches_oracle(device, algo):
  lrn, st, host, online, target = _setup(algo, _adam(), seed=3)
  rng = np.random.default_rng(5)
  slots = helpers.kink_free_slots(online, host, st.capacity, BATCH, rng)
  weights = None
  if algo == 'per':
    weights = rng.uniform(0.2, 1.0, size=BATCH).astype(np.float32)
    weights /= weights.max()
  zeros = learner_ref.zeros_like_tree(online)
  ref = learner_ref.learner_step(online, target, zeros, zeros, *_batch(host, slots), algo=algo,
                                 weights=weights)
  w_d = None if weights is None else torch.from_numpy(weights).to(device)
  lrn.step(st, torch.from_numpy(slots).to(device), w_d)
  outputs = [x.cpu().numpy() for x in lrn.fetch_outputs()]
  _check_step(lrn, ref, (online, zeros, zeros), 0, None, outputs, algo)
  _compare_tree(lrn.params_tree('target'), target, 0.0, what='target')
  assert lrn.sync_status() == 0


def _snapshot(lrn):
  return [t.clone() for t in (lrn.online, lrn.mu, lrn.nu, lrn.count)]


def _restore(lrn, snap):
  for t, s in zip((lrn.online, lrn.mu, lrn.nu, lrn.count), snap):
    t.copy_(s)


def _raw_apply(lrn, g):
  from dqn_mgsc_zoo_amd import _native
  _native.check(_native.lib().dqz_optimizer_apply(
      lrn._opt_h, _native.ptr(lrn.online), _native.ptr(g), _native.ptr(lrn.mu),  # pylint: disable=protected-access
      _native.ptr(lrn.nu), _native.ptr(lrn.count), _native.stream_handle()))


@pytest.mark.parametrize('optimizer', ['clip_adam', 'rmsprop'])
def test_step_opt_is_grad_then_apply_and_uniform_is_sample_then_step(device, optimizer):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  opt = _adam(clip=0.12) if optimizer == 'clip_adam' else learner_lib.rmsprop(LR, 0.95, 1e-6)
  lrn, st, _, _, _ = _setup('dqn', opt, seed=41)
  rng = np.random.default_rng(42)
  for step in range(2):  # the second from carried moments
    slots = torch.from_numpy(rng.integers(0, st.capacity, BATCH).astype(np.int32)).to(device)
    snap = _snapshot(lrn)
    lrn.step(st, slots)
    after = _snapshot(lrn)
    gn = lrn.grad_norm().clone()
    _restore(lrn, snap)
    g = lrn.grad(st, slots)  # kept: an unclipped handle norms it on demand
    _raw_apply(lrn, g)
    torch.cuda.synchronize()
    for x, y in zip(after, _snapshot(lrn)):
      assert torch.equal(x, y), step
    assert torch.equal(gn, lrn.grad_norm())
    torch.cuda.synchronize()
    assert int(lrn.count.item()) == (step + 1 if optimizer == 'clip_adam' else 0)
  # the fused uniform draw
  ca = torch.full((1,), 5, dtype=torch.int64, device=device)
  cb = ca.clone()
  sa = torch.zeros((BATCH,), dtype=torch.int32, device=device)
  sb = sa.clone()
  snap = _snapshot(lrn)
  lrn.step_uniform(st, 17, 200, st.capacity, 9, ca, sa)
  after = _snapshot(lrn)
  _restore(lrn, snap)
  learner_lib.sample_uniform(17, 200, st.capacity, BATCH, 9, cb, sb)
  lrn.step(st, sb)
  torch.cuda.synchronize()
  assert torch.equal(sa, sb) and int(ca.item()) == int(cb.item()) == 6
  for x, y in zip(after, _snapshot(lrn)):
    assert torch.equal(x, y)
  assert lrn.sync_status() == 0


def test_step_opt_per_draw_draws_and_writes_back_as_the_rmsprop_path(device):
  """The fused PER draw, IS weights and priority write-back do not depend on
  the optimizer: from equal parameters the Adam step leaves the slots, the
  weights, the probabilities, the sum tree, max_seen and the Philox counter of
  the centered-RMSProp step; its update is grad-then-apply on those draws."""
  from dqn_mgsc_zoo_amd import _native
  from dqn_mgsc_zoo_amd import replay as replay_lib
  alpha, usp, beta = 0.6, 0.05, 0.4
  a, st, _, _, _ = _setup('per', None, seed=61)
  b, _, _, _, _ = _setup('per', _adam(clip=0.12), seed=61)
  rng = np.random.default_rng(62)
  host = replay_lib.SumTree()
  prios = rng.random(st.capacity) ** 2
  prios[::17] = 0.0
  host.set_all(prios)
  cap = host.capacity
  out = {}
  for name in 'ab':
    i32 = lambda: torch.zeros((BATCH,), dtype=torch.int32, device=device)
    o = dict(tree=torch.from_numpy(host.storage.copy()).to(device),
             max=torch.tensor([1.0], dtype=torch.float64, device=device),
             counter=torch.zeros((1,), dtype=torch.int64, device=device), idx=i32(), slots=i32(),
             probs=torch.zeros((BATCH,), dtype=torch.float64, device=device),
             w=torch.zeros((BATCH,), dtype=torch.float32, device=device))
    o['draw'] = _native.DqzPerDraw(
        o['tree'].data_ptr(), cap, 0, st.capacity, st.capacity, usp, beta, 1, 7, o['counter'].data_ptr(),
        None, None, None, alpha, o['max'].data_ptr(), o['idx'].data_ptr(), o['slots'].data_ptr(),
        o['probs'].data_ptr(), o['w'].data_ptr())
    out[name] = o
  snap = _snapshot(b)
  a.step_per_draw(st, out['a']['draw'])
  b.step_per_draw(st, out['b']['draw'])
  torch.cuda.synchronize()
  for k in ('tree', 'max', 'counter', 'idx', 'slots', 'probs', 'w'):
    assert torch.equal(out['a'][k], out['b'][k]), k
  qa, tda, la = [x.clone() for x in a.fetch_outputs()]
  qb, tdb, lb = b.fetch_outputs()
  assert torch.equal(qa, qb) and torch.equal(tda, tdb) and torch.equal(la, lb)
  assert not torch.equal(out['a']['tree'], torch.from_numpy(host.storage).to(device))
  after = _snapshot(b)
  assert not torch.equal(after[0], snap[0]) and int(b.count.item()) == 1
  _restore(b, snap)
  _raw_apply(b, b.grad(st, out['b']['slots'], out['b']['w']))
  torch.cuda.synchronize()
  for x, y in zip(after, _snapshot(b)):
    assert torch.equal(x, y)
  assert a.sync_status() == 0 and b.sync_status() == 0


def test_graph_of_five_steps_replayed_twice_equals_ten_eager(device):
  a, st, _, _, _ = _setup('dqn', _adam(clip=0.12), seed=71)
  b, _, _, _, _ = _setup('dqn', _adam(clip=0.12), seed=71)
  ca = torch.zeros((1,), dtype=torch.int64, device=device)
  cb = ca.clone()
  sa = torch.zeros((BATCH,), dtype=torch.int32, device=device)
  sb = sa.clone()
  step = lambda lrn, c, s: lrn.step_uniform(st, 0, st.capacity, st.capacity, 13, c, s)
  side = torch.cuda.Stream(device)  # every kernel has run once before the capture
  side.wait_stream(torch.cuda.current_stream(device))
  with torch.cuda.stream(side):
    step(b, cb, sb)
  torch.cuda.current_stream(device).wait_stream(side)
  step(a, ca, sa)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):  # one stream, a linear chain of launches
    for _ in range(5):
      step(b, cb, sb)
  g.replay()
  g.replay()
  for _ in range(10):
    step(a, ca, sa)
  torch.cuda.synchronize()
  assert int(a.count.item()) == int(b.count.item()) == 11
  assert int(ca.item()) == int(cb.item()) == 11 and torch.equal(sa, sb)
  for which in ('online', 'mu', 'nu'):
    assert torch.equal(getattr(a, which), getattr(b, which)), which
  assert torch.equal(a.grad_norm(), b.grad_norm())
  assert torch.isfinite(a.online).all() and not torch.equal(a.online, a.target)
  assert a.sync_status() == 0 and b.sync_status() == 0


def test_twenty_carried_steps_clip_adam_with_target_sync(device):
  """Twenty steps of chain(clip_by_global_norm, adam) from carried state with
  a target sync after the tenth; every step against the oracle stepped from
  the device's own state, ReLU masks and argmax (tests/test_trajectory_gpu.py)."""
  clip = 0.15
  lrn, st, host, _, _ = _setup('double', _adam(clip=clip), seed=310)
  rng = np.random.default_rng(311)
  active = 0
  for step in range(20):
    p, t, mu, nu = _state(lrn)
    count = int(lrn.count.item())
    slots = rng.integers(0, st.capacity, size=BATCH).astype(np.int32)
    lrn.step(st, torch.from_numpy(slots).to(device))
    outputs = [x.cpu().numpy() for x in lrn.fetch_outputs()]
    masks = [lrn.fetch_activations(0)[k].cpu().numpy() > 0 for k in ('y1', 'y2', 'y3', 'h1')]
    select = np.argmax(lrn.fetch_activations(2)['q'].cpu().numpy(), axis=1)
    zeros = learner_ref.zeros_like_tree(p)
    ref = learner_ref.learner_step(p, t, zeros, zeros, *_batch(host, slots), algo='double',
                                   masks=masks, select=select)
    active += optim_ref.global_norm(ref['grads']) >= clip
    _check_step(lrn, ref, (p, mu, nu), count, clip, outputs, 'step %d' % step)
    t1 = lrn.params_tree('target')
    for m in t:
      for n in t[m]:
        np.testing.assert_array_equal(t1[m][n], t[m][n])
    if step == 9:
      lrn.sync_target()
      p1, t1, _, _ = _state(lrn)
      for m in p1:
        for n in p1[m]:
          np.testing.assert_array_equal(t1[m][n], p1[m][n])
  print('clip active on %d of 20 steps' % active)
  assert int(lrn.count.item()) == 20 and lrn.sync_status() == 0


def test_unsupported_calls_say_so(device):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  lrn, st, _, _, _ = _setup('dqn', _adam(), seed=5)
  slots = torch.zeros((BATCH,), dtype=torch.int32, device=device)
  with pytest.raises(NotImplementedError, match='centered-RMSProp'):
    lrn.profile(st, slots)
  with pytest.raises(NotImplementedError, match='centered-RMSProp'):
    lrn.step_logits(st, None, slots, counter=slots)
  with pytest.raises(ValueError, match='differentiates through'):
    learner_lib.MetaLearner(lrn, 4)
  fused, _, _, _, _ = _setup('dqn', None, seed=5)
  with pytest.raises(NotImplementedError):
    fused.grad_norm()
  # an unclipped optimizer still reports the norm of its last step's gradient
  slots = torch.arange(BATCH, dtype=torch.int32, device=device)
  norm64 = float(lrn.grad(st, slots).double().norm().item())
  lrn.step(st, slots)
  assert abs(float(lrn.grad_norm().item()) - norm64) <= 2.0**-22 * norm64


def _make_agent(cls_name, optimizer, seed):
  from dqn_mgsc_zoo_amd import networks
  from dqn_mgsc_zoo_amd import parts
  from dqn_mgsc_zoo_amd import replay as replay_lib
  kw = dict(
      preprocessor=fake_env.FrameStacker(),
      sample_network_input=np.zeros((84, 84, 4), np.uint8),
      network=networks.dqn_atari_network(6), optimizer=optimizer, batch_size=BATCH,
      exploration_epsilon=parts.LinearSchedule(begin_t=40, decay_steps=200, begin_value=1.0, end_value=0.1),
      min_replay_capacity_fraction=0.25, learn_period=4, target_network_update_period=40,
      grad_error_bound=1.0 / 32, rng_key=np.array([0, seed], np.uint32))
  if cls_name == 'mgsc':
    from dqn_mgsc_zoo_amd import learner as learner_lib
    from dqn_mgsc_zoo_amd import replay_circular as rc
    from dqn_mgsc_zoo_amd.dqn_mgsc_batched import agent as agent_lib
    replay = rc.MGSCFiFoTransitionReplay(160, rc.Transition(None, None, None, None, None),
                                         np.random.default_rng(seed))
    return agent_lib.MGSCDqn(transition_accumulator=rc.TransitionAccumulator(), replay=replay,
                             meta_optimizer=learner_lib.adam(2.5e-4), meta_batch_size=8, **kw), replay
  from dqn_mgsc_zoo_amd.dqn import agent as agent_lib
  replay = replay_lib.TransitionReplay(160, replay_lib.Transition(None, None, None, None, None),
                                       np.random.RandomState(seed))
  return agent_lib.Dqn(transition_accumulator=replay_lib.TransitionAccumulator(), replay=replay, **kw), replay


def test_dqn_agent_with_clipped_adam_checkpoints_and_continues(device):
  from dqn_mgsc_zoo_amd import parts
  a1, r1 = _make_agent('dqn', _adam(clip=10.0), seed=4)
  env = fake_env.FakeAtari(episode_len=23, seed=5)
  loop = parts.run_loop(a1, env, max_steps_per_episode=0)
  p0 = a1.learner.online.clone()
  for _ in range(90):
    next(loop)
  assert not torch.equal(p0, a1.learner.online) and torch.isfinite(a1.learner.online).all()
  state = copy.deepcopy(a1.get_state())
  clip_state, inner = state['opt_state']
  assert clip_state == () and type(clip_state).__name__ == 'EmptyState'
  adam_state, scale_state = inner
  assert type(adam_state).__name__ == 'ScaleByAdamState' and scale_state == ()
  assert adam_state.count.dtype == np.int32 and int(adam_state.count) == int(a1.learner.count.item()) > 0
  online = state['online_params']
  for tree in (adam_state.mu, adam_state.nu):
    assert list(tree) == list(online)
    for m in online:
      for n in online[m]:
        assert tree[m][n].shape == online[m][n].shape and tree[m][n].dtype == np.float32
  assert 0.0 < float(a1.learner.grad_norm().item()) < 10.0
  a2, r2 = _make_agent('dqn', _adam(clip=10.0), seed=99)
  a2.set_state(state)
  r2._random_state.set_state(r1._random_state.get_state())  # pylint: disable=protected-access
  env = fake_env.FakeAtari(episode_len=17, seed=6)
  steps = [env.reset()]
  for t in range(60):
    steps.append(env.step(t % 6) if not steps[-1].last() else env.reset())
  for ts in steps:
    if ts.first():
      a1.reset()
      a2.reset()
    assert a1.step(ts) == a2.step(ts)
  for which in ('online', 'target', 'mu', 'nu', 'count'):
    assert torch.equal(getattr(a1.learner, which), getattr(a2.learner, which)), which
  assert int(a1.learner.count.item()) > int(adam_state.count)
  # a centered-RMSProp checkpoint is not an Adam one
  a3, _ = _make_agent('dqn', None, seed=4)
  with pytest.raises((ValueError, AttributeError, TypeError)):
    a2.set_state(dict(state, opt_state=a3.get_state()['opt_state']))


def test_mgsc_agent_refuses_adam(device):
  with pytest.raises(ValueError, match='centered-RMSProp'):
    _make_agent('mgsc', _adam(), seed=0)
  from dqn_mgsc_zoo_amd import learner as learner_lib
  with pytest.raises(ValueError, match='centered-RMSProp'):
    _make_agent('mgsc', learner_lib.rmsprop(LR, 0.95, 1e-5), seed=0)
