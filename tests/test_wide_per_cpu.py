"""CPU: Rainbow's learning rule on the C51 and QR-DQN heads, without a GPU.

  reference   tests/wide_per_ref.py against torch autograd in float64, written
              independently here (torch softmax / log_softmax / where, the
              selector's argmax in torch): loss = mean(w loss_b) and its
              gradient on the head alone and through the whole network, both
              heads, weights that include an exact 0 and an exact 1; the
              priorities clip(|loss_b|, 0, 100).
  known answer  two actions whose selector and target disagree: the loss is
              the hand-computed one for the selector's action, and differs from
              the target-greedy one.
  accumulator replay.NStepTransitionAccumulator against what the reference's
              own class yielded for the same streams
              (tests/golden/nstep_golden.json, written by make_nstep_golden.py):
              n = 1, 3, 5; episodes shorter than, equal to and longer than n; a
              FIRST arriving mid-stream; ValueError on a non-FIRST start.
              Rewards and discounts are compared as float64 bits.
  refusals    what check_step says of a head created with options
              (dqz_*_debug_check_opt), the null checks of the new entries, and
              the old dqz_*_debug_check still refusing weights.
"""

import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import learner_ref
from tests import c51_ref
from tests import helpers
from tests import qr_ref
from tests import wide_per_ref

INVALID = -1  # DQZ_ERR_INVALID
HEADS = ['c51', 'qr']


def _head(kind, n):
  if kind == 'c51':  # float64 and equally spaced, for _torch_loss_b's two-neighbour projection
    return ('c51', np.linspace(-10.0, 10.0, n))
  return ('qr', qr_ref.make_quantiles(n), 1.0)


def _torch_loss_b(head, out_tm1, a_tm1, r, d, out_target, a_star):
  """Per-sample loss in torch float64; out_* are [B, *head_shape] tensors, the
  target side under no_grad."""
  b = out_tm1.shape[0]
  idx = torch.arange(b)
  a_tm1 = torch.as_tensor(a_tm1, dtype=torch.long)
  a_star = torch.as_tensor(a_star, dtype=torch.long)
  r, d = torch.as_tensor(r, dtype=torch.float64), torch.as_tensor(d, dtype=torch.float64)
  if head[0] == 'c51':
    z = torch.as_tensor(np.asarray(head[1], np.float64))
    with torch.no_grad():
      p = F.softmax(out_target, dim=-1)[idx, a_star]  # [B, N]
      y = torch.clamp(r[:, None] + d[:, None] * z[None, :], z[0], z[-1])  # [B, N]
      dz = z[1] - z[0]  # make_support is equally spaced: the two-neighbour projection
      w = torch.clamp(1.0 - (y[:, None, :] - z[None, :, None]).abs() / dz, 0.0, 1.0)  # [B, k, i]
      m = (w * p[:, None, :]).sum(-1)
    return -(m * F.log_softmax(out_tm1[idx, a_tm1], dim=-1)).sum(-1)
  tau, kappa = torch.as_tensor(np.asarray(head[1], np.float64)), head[2]
  theta = out_tm1[idx, :, a_tm1]  # [B, N]
  with torch.no_grad():
    t = r[:, None] + d[:, None] * out_target[idx, :, a_star]
  delta = t[:, None, :] - theta[:, :, None]
  ad = delta.abs()
  hub = torch.where(ad <= kappa, 0.5 * delta * delta, kappa * (ad - 0.5 * kappa))
  w = (tau[None, :, None] - (delta.detach() < 0).double()).abs()
  return (w * hub).mean(2).sum(1)


def _torch_selector(head, out_s):
  if head[0] == 'c51':
    q = F.softmax(out_s, dim=-1) @ torch.as_tensor(np.asarray(head[1], np.float64))
  else:
    q = out_s.mean(dim=1)
  return q.argmax(dim=1).numpy()


WEIGHTS = {4: [0.0, 1.0, 0.37, 0.81], 8: [0.9, 0.0, 1.0, 0.05, 0.33, 0.6, 0.125, 0.77]}


@pytest.mark.parametrize('kind', HEADS)
@pytest.mark.parametrize('b,a,n', [(4, 3, 5), (8, 6, 51)])
def test_weighted_double_q_loss_matches_autograd_on_the_head(kind, b, a, n):
  head = _head(kind, n)
  shape = wide_per_ref.head_shape(head, a)
  rng = np.random.default_rng(b + n)
  h1 = np.maximum(rng.standard_normal((b, 512)), 0.0)
  w2 = rng.uniform(-1, 1, (512, a * n)) / np.sqrt(512)
  bias = rng.uniform(-1, 1, a * n) / np.sqrt(512)
  out_t = rng.standard_normal((b,) + shape)
  out_s = rng.standard_normal((b,) + shape)
  a_tm1 = rng.integers(0, a, b)
  r = rng.choice([-1.0, 0.0, 1.0], b)
  d = 0.99 * (rng.random(b) > 0.3)
  w = np.array(WEIGHTS[b])
  assert (w == 0).any() and (w == 1).any()
  sel = wide_per_ref.selector(head, out_s)
  assert np.array_equal(sel, _torch_selector(head, torch.as_tensor(out_s)))
  assert (sel != wide_per_ref.selector(head, out_t)).any()
  res = wide_per_ref.head_loss(head, (h1 @ w2 + bias).reshape((b,) + shape), a_tm1, r, d, out_t, sel, w)
  th1, tw, tb = (torch.tensor(x, requires_grad=True) for x in (h1, w2, bias))
  out = (th1 @ tw + tb).reshape((b,) + shape)
  out.retain_grad()
  loss_b = _torch_loss_b(head, out, a_tm1, r, d, torch.as_tensor(out_t), sel)
  loss = (torch.as_tensor(w) * loss_b).mean()
  loss.backward()
  np.testing.assert_allclose(res['loss_b'], loss_b.detach().numpy(), rtol=1e-12, atol=1e-13)
  assert abs(loss.item() - res['wloss']) <= 1e-12 * max(1.0, abs(res['wloss']))
  np.testing.assert_allclose(res['wdense'], out.grad.numpy(), atol=1e-14)
  dense = res['wdense'].reshape(b, -1)
  np.testing.assert_allclose(h1.T @ dense, tw.grad.numpy(), atol=1e-13)
  np.testing.assert_allclose(dense.sum(0), tb.grad.numpy(), atol=1e-13)
  np.testing.assert_allclose(dense @ w2.T, th1.grad.numpy(), atol=1e-13)
  zero = int(np.flatnonzero(w == 0)[0])
  assert not res['wdense'][zero].any() and res['dense'][zero].any()
  one = int(np.flatnonzero(w == 1)[0])
  assert np.array_equal(res['wdense'][one], res['dense'][one])
  np.testing.assert_array_equal(res['priorities'], np.minimum(np.abs(res['loss_b']), 100.0))
  # the unweighted loss of the reference this one is built on is untouched by the weights
  plain = wide_per_ref.head_loss(head, (h1 @ w2 + bias).reshape((b,) + shape), a_tm1, r, d, out_t, sel)
  assert np.array_equal(plain['loss_b'], res['loss_b']) and plain['wloss'] == plain['loss']


@pytest.mark.parametrize('kind', HEADS)
def test_whole_network_gradient_matches_autograd(kind):
  from dqn_mgsc_zoo_amd import networks
  b, a, n = 3, 3, 5
  head = _head(kind, n)
  shape = wide_per_ref.head_shape(head, a)
  net = (networks.c51_atari_network(a, c51_ref.make_support(10.0, n)) if kind == 'c51'
         else networks.qr_atari_network(a, head[1]))
  online = net.init(1)
  target = helpers.perturbed_tree(online, 2)
  rng = np.random.default_rng(3)
  s_tm1 = rng.integers(0, 256, (b, 84, 84, 4), dtype=np.uint8)
  s_t = rng.integers(0, 256, (b, 84, 84, 4), dtype=np.uint8)
  a_tm1, r, d = np.array([2, 0, 1]), np.array([1.0, -1.0, 0.0]), np.array([0.99, 0.0, 0.99])
  w = np.array([0.4, 0.0, 1.0])
  res = wide_per_ref.learner_grads(head, online, target, (s_tm1, a_tm1, r, d, s_t), a, weights=w)

  names = list(learner_ref.CONV_NAMES)
  hd = 'sequential/sequential_1'
  tp = {m: {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in leaves.items()}
        for m, leaves in online.items()}

  def apply(params, s):
    x = torch.as_tensor(s.astype(np.float64) / 255.0).permute(0, 3, 1, 2)
    for name, stride in zip(names, (4, 2, 1)):
      x = F.relu(F.conv2d(x, params[name]['w'].permute(3, 2, 0, 1), params[name]['b'], stride=stride))
    x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)  # Haiku's (h, w, c) flatten
    h = F.relu(x @ params[hd + '/linear']['w'] + params[hd + '/linear']['b'])
    return (h @ params[hd + '/linear_1']['w'] + params[hd + '/linear_1']['b']).reshape((-1,) + shape)

  with torch.no_grad():
    tt = {m: {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in leaves.items()}
          for m, leaves in target.items()}
    out_t = apply(tt, s_t)
    out_s = apply(tp, s_t)  # the selector: online parameters at s_t, no gradient
  np.testing.assert_allclose(res['out'][1], out_t.numpy(), atol=1e-12)
  np.testing.assert_allclose(res['out'][2], out_s.numpy(), atol=1e-12)
  sel = _torch_selector(head, out_s)
  assert np.array_equal(sel, res['selector'])
  loss_b = _torch_loss_b(head, apply(tp, s_tm1), a_tm1, r, d, out_t, sel)
  loss = (torch.as_tensor(w) * loss_b).mean()
  loss.backward()
  np.testing.assert_allclose(res['loss_b'], loss_b.detach().numpy(), rtol=1e-12)
  assert abs(loss.item() - res['wloss']) <= 1e-12
  for m in online:
    for k in online[m]:
      got, want = res['grads'][m][k], tp[m][k].grad.numpy()
      assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (m, k)
  assert np.abs(res['grads'][hd + '/linear_1']['w']).max() > 0


def test_known_answer_where_selector_and_target_disagree():
  ln = np.log
  # categorical: support {0, 1}, r = 0, d = 1, so m = p[a*]; the taken action's softmax is (1/4, 3/4)
  head = ('c51', np.array([0.0, 1.0], np.float32))
  out_t = np.array([[[0.0, 0.0], [ln(0.25), ln(0.75)]]])  # q = (1/2, 3/4): the target's greedy action is 1
  out_s = np.array([[[0.0, 2.0], [0.0, 0.0]]])  # the selector prefers action 0
  out_o = np.array([[[ln(0.25), ln(0.75)], [0.0, 0.0]]])
  sel = wide_per_ref.selector(head, out_s)
  assert sel.tolist() == [0] and wide_per_ref.selector(head, out_t).tolist() == [1]
  double = wide_per_ref.head_loss(head, out_o, [0], [0.0], [1.0], out_t, sel, [0.5])
  plain = wide_per_ref.head_loss(head, out_o, [0], [0.0], [1.0], out_t, None, [0.5])
  want_double = -(0.5 * ln(0.25) + 0.5 * ln(0.75))  # m = (1/2, 1/2)
  want_plain = -(0.25 * ln(0.25) + 0.75 * ln(0.75))  # m = (1/4, 3/4)
  assert double['loss_b'][0] == pytest.approx(want_double, abs=1e-15)
  assert plain['loss_b'][0] == pytest.approx(want_plain, abs=1e-15)
  assert double['wloss'] == pytest.approx(0.5 * want_double, abs=1e-15)
  assert abs(want_double - want_plain) > 0.1
  # quantile: one quantile tau = 1/2, kappa = 1, theta = 1/2, t = x_target[a*]
  head = ('qr', np.array([0.5], np.float32), 1.0)
  out_t = np.array([[[0.25, 2.0]]])  # [B, N, A]: the target's greedy action is 1
  out_s = np.array([[[1.0, 0.0]]])
  out_o = np.array([[[0.5, -3.0]]])
  sel = wide_per_ref.selector(head, out_s)
  assert sel.tolist() == [0] and wide_per_ref.selector(head, out_t).tolist() == [1]
  double = wide_per_ref.head_loss(head, out_o, [0], [0.0], [1.0], out_t, sel, [0.25])
  plain = wide_per_ref.head_loss(head, out_o, [0], [0.0], [1.0], out_t, None, [0.25])
  assert double['loss_b'][0] == 0.5 * 0.5 * 0.25**2  # delta = -1/4 inside kappa, w = |1/2 - 1|
  assert plain['loss_b'][0] == 0.5 * (0.5 + 1.0 * 0.5)  # delta = 3/2 beyond kappa, w = 1/2
  assert double['wloss'] == 0.25 * double['loss_b'][0]
  assert double['dtaken'][0, 0] == 0.5 * 0.25 and double['wdtaken'][0, 0] == 0.25 * 0.5 * 0.25
  assert double['priorities'][0] == double['loss_b'][0]
  big = wide_per_ref.head_loss(head, out_o, [0], [500.0], [1.0], out_t, sel)
  assert big['loss_b'][0] > 100.0 and big['priorities'][0] == 100.0


# -- the n-step accumulator against the reference's own class ---------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'nstep_golden.json')


def _golden():
  with open(GOLDEN) as f:
    return json.load(f)


def _timestep(step_type, reward, discount, obs):
  from dqn_mgsc_zoo_amd import parts
  kinds = (parts.StepType.FIRST, parts.StepType.MID, parts.StepType.LAST)
  return parts.TimeStep(kinds[step_type], reward, discount, obs)


def test_n_step_accumulator_matches_the_reference_golden():
  from dqn_mgsc_zoo_amd import replay as replay_lib
  doc = _golden()
  seen_n, total = set(), 0
  for case in doc['cases']:
    n = case['n']
    seen_n.add(n)
    acc = replay_lib.NStepTransitionAccumulator(n)
    episode_t = 0
    for (step_type, reward, discount, obs, action), want in zip(case['stream'], case['yields']):
      got = list(acc.step(_timestep(step_type, reward, discount, obs), action))
      assert len(got) == len(want), (case['name'], n, obs)
      for g, w in zip(got, want):
        assert [g.s_tm1, g.a_tm1, g.s_t] == [w[0], w[1], w[4]]
        # bit for bit: the reference's order of the sum and the product
        assert np.float64(g.r_t).tobytes() == np.float64(w[2]).tobytes(), (case['name'], n, obs)
        assert np.float64(g.discount_t).tobytes() == np.float64(w[3]).tobytes(), (case['name'], n, obs)
      # the contract, restated: nothing on FIRST, one per MID once n steps are held, min(n, T) .. 1 on LAST
      episode_t = 0 if step_type == 0 else episode_t + 1
      if step_type == 0:
        assert not got
      elif step_type == 1:
        assert len(got) == (1 if episode_t >= n else 0)
        assert not got or got[0].s_t - got[0].s_tm1 == n
      else:
        assert [g.s_t - g.s_tm1 for g in got] == list(range(min(n, episode_t), 0, -1))
        assert all(g.s_t == obs for g in got)
      total += len(got)
  assert seen_n == {1, 3, 5} and total > 50
  names = {(c['name'], c['n']) for c in doc['cases']}
  assert {('first_mid_stream', n) for n in (1, 3, 5)} <= names
  for case in doc['cases']:  # the cases hold what their names say
    lengths, t = [], 0
    for step_type, *_ in case['stream']:
      if step_type == 0 and t:
        lengths.append(t)
      t = 0 if step_type == 0 else t + 1
    lengths.append(t)
    if case['name'] == 'episodes':
      n = case['n']
      assert any(x < n for x in lengths) or n == 1
      assert n in lengths and any(x > n for x in lengths)
    else:  # the first episode has no LAST
      firsts = [i for i, s in enumerate(case['stream']) if s[0] == 0]
      assert len(firsts) == 2 and case['stream'][firsts[1] - 1][0] == 1


def test_n_step_accumulator_needs_a_first_timestep():
  from dqn_mgsc_zoo_amd import replay as replay_lib
  doc = _golden()
  assert doc['non_first_start']['error'] == 'ValueError'
  acc = replay_lib.NStepTransitionAccumulator(3)
  with pytest.raises(ValueError, match='Expected FIRST timestep'):
    list(acc.step(_timestep(1, 0.0, 0.99, 0), 0))
  assert doc['non_first_start']['message'].startswith('Expected FIRST timestep')
  acc.reset()
  assert not list(acc.step(_timestep(0, None, None, 0), 0))
  with pytest.raises(ValueError, match='positive integer'):
    replay_lib.NStepTransitionAccumulator(0)


def test_one_step_accumulator_is_the_n_equal_one_case():
  from dqn_mgsc_zoo_amd import replay as replay_lib
  one, n1 = replay_lib.TransitionAccumulator(), replay_lib.NStepTransitionAccumulator(1)
  case = [c for c in _golden()['cases'] if c['n'] == 1 and c['name'] == 'episodes'][0]
  for step_type, reward, discount, obs, action in case['stream']:
    ts = _timestep(step_type, reward, discount, obs)
    assert list(one.step(ts, action)) == list(n1.step(ts, action))


# -- refusals before any device call -------------------------------------------

@pytest.fixture(scope='module')
def lib():
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  if not os.path.exists(_native.LIB_PATH):
    import __graft_entry__  # pylint: disable=g-import-not-at-top
    __graft_entry__._compile_lib()  # pylint: disable=protected-access
  return _native.lib()


_WORD = ctypes.c_int64(0)
P = ctypes.cast(ctypes.pointer(_WORD), ctypes.c_void_p)  # any non-null address
NOUN = {'c51': 'categorical', 'qr': 'quantile'}
# what the two heads word differently beyond the noun (learner_impl.hpp kWide)
WORDS = {
    'c51': dict(meta='the categorical head has no MGSC meta mode',
                unit='the categorical head has no unit-cotangent pass',
                wb='the categorical head has no TD error to write back as a priority',
                fused='the categorical head runs in gradient mode only (no fused centered RMSProp)'),
    'qr': dict(meta='the quantile head takes no MGSC meta mode',
               unit='the quantile head takes no unit-cotangent pass',
               wb='the quantile head takes no PER priority write-back',
               fused='the quantile head takes no fused centered RMSProp (it runs in gradient mode only)')}


def _check_opt(lib, kind, batch, modes, double_q, weighted):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  request = 0
  for m in modes:
    request |= _native.C51_REQ[m]
  opt = _native.DqzWideOptions(double_q, weighted)
  rc = getattr(lib, 'dqz_%s_debug_check_opt' % kind)(batch, request, ctypes.byref(opt))
  return rc, lib.dqz_last_error().decode()


@pytest.mark.parametrize('kind', HEADS)
def test_check_step_with_options(lib, kind):
  noun, words = NOUN[kind], WORDS[kind]
  # what passes: weights on a weighted head, none on another, with or without double_q
  for double_q in (0, 1):
    assert _check_opt(lib, kind, 8, ['weights'], double_q, 1)[0] == 0
    assert _check_opt(lib, kind, 8, [], double_q, 0)[0] == 0
    assert _check_opt(lib, kind, 2, ['weights'], double_q, 1)[0] == 0
    # weights only on a weighted head; a weighted head never without
    assert _check_opt(lib, kind, 8, ['weights'], double_q, 0) == (
        INVALID, 'the %s head takes no importance weights' % noun)
    assert _check_opt(lib, kind, 8, [], double_q, 1) == (INVALID, 'a weighted %s step needs is_weights' % noun)
  # what stays refused, in the plain heads' words, whatever the options
  refused = [
      (['per_draw'], 'the %s head takes no prioritized draw' % noun),
      (['uniform_draw'], 'the %s head takes no in-launch batch draw' % noun),
      (['logit_draw'], 'the %s head takes no in-launch batch draw' % noun),
      (['exact_draw'], 'the %s head takes no in-launch batch draw' % noun),
      (['meta_p'], words['meta']), (['meta_epi'], words['meta']), (['meta_softmax'], words['meta']),
      (['unit'], words['unit']), (['write_back'], words['wb']), (['fused_rmsprop'], words['fused'])]
  for double_q, weighted in ((1, 1), (0, 1), (1, 0)):
    base = ['weights'] if weighted else []
    for modes, message in refused:
      assert _check_opt(lib, kind, 8, base + modes, double_q, weighted) == (INVALID, message), (modes, double_q)
    assert _check_opt(lib, kind, 1, base, double_q, weighted) == (INVALID, 'the %s head needs batch >= 2' % noun)


@pytest.mark.parametrize('kind', HEADS)
def test_options_are_checked(lib, kind):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  check = getattr(lib, 'dqz_%s_debug_check_opt' % kind)
  assert check(8, 0, None) == INVALID and lib.dqz_last_error() == b'null argument'
  for bad in ((2, 0), (0, -1), (1, 3)):
    opt = _native.DqzWideOptions(*bad)
    assert check(8, 0, ctypes.byref(opt)) == INVALID
    assert lib.dqz_last_error() == b'double_q and weighted must be 0 or 1'


@pytest.mark.parametrize('kind', HEADS)
def test_the_old_probe_still_refuses_weights(lib, kind):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  check = getattr(lib, 'dqz_%s_debug_check' % kind)
  assert check(8, 0) == 0
  assert check(8, _native.C51_REQ['weights']) == INVALID
  assert lib.dqz_last_error().decode() == 'the %s head takes no importance weights' % NOUN[kind]


def _null_refusals(kind):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  h = ctypes.c_void_p()
  out = ctypes.byref(h)
  cfg = _native.DqzLearnerConfig(8, 6, 0, 2.5e-4, 0.0, 1e-4, 0.0)
  double = _native.DqzLearnerConfig(8, 6, 1, 2.5e-4, 0.0, 1e-4, 0.0)
  opt = _native.DqzWideOptions(1, 1)
  bad = _native.DqzWideOptions(1, 2)
  extra = () if kind == 'c51' else (ctypes.c_float(1.0),)
  pre = 'dqz_%s_' % kind
  create = lambda c, n, o: (pre + 'create_opt', (ctypes.byref(c), n, P) + extra + (o, out))
  count = 'num_atoms must be in [2, 64]' if kind == 'c51' else 'num_quantiles must be in [1, 256]'
  return [
      ('create-null-options', create(cfg, 51, None), 'null argument'),
      ('create-bad-options', create(cfg, 51, ctypes.byref(bad)), 'double_q and weighted must be 0 or 1'),
      ('create-null-config', (pre + 'create_opt', (None, 51, P) + extra + (ctypes.byref(opt), out)),
       'null argument'),
      ('create-too-many', create(cfg, 65 if kind == 'c51' else 257, ctypes.byref(opt)), count),
      ('create-batch-one', create(_native.DqzLearnerConfig(1, 6, 0, 2.5e-4, 0.0, 1e-4, 0.0), 51,
                                  ctypes.byref(opt)), 'batch must be in [2, 256]'),
      # double_q is an option, not the configuration's algo
      ('create-algo-double', create(double, 51, ctypes.byref(opt)), 'the %s head runs on a DQN learner' % NOUN[kind]),
      ('step-null-handle', (pre + 'step_w', (None, 'PARAMS', 'STORE', P, P, P, P, None)), 'null argument'),
      ('step-null-weights', (pre + 'step_w', (P, 'PARAMS', 'STORE', P, None, P, P, None)), 'null argument'),
      ('grad-null-handle', (pre + 'grad_w', (None, 'PARAMS', 'STORE', P, P, P, None)), 'null argument'),
      ('grad-null-weights', (pre + 'grad_w', (P, 'PARAMS', 'STORE', P, None, P, None)), 'null argument'),
      ('profile-null-weights', (pre + 'profile_w', (P, 'PARAMS', 'STORE', P, None, P, 1, None, None)),
       'null argument'),
      ('outputs-null-handle', (pre + 'outputs_opt', (None, P, P, None)), 'null argument'),
  ]


_NULLS = [(k,) + r for k in HEADS for r in _null_refusals(k)]


@pytest.mark.parametrize('kind,call,fragment', [(r[0],) + r[2:] for r in _NULLS],
                         ids=['%s-%s' % r[:2] for r in _NULLS])
def test_new_entries_refuse_before_any_device_call(lib, kind, call, fragment):
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  params, store = _native.DqzParams(), _native.DqzStore()  # every pointer null
  named = {'PARAMS': ctypes.byref(params), 'STORE': ctypes.byref(store)}
  entry, args = call
  args = [named.get(x, x) if isinstance(x, str) else x for x in args]
  assert getattr(lib, entry)(*args) == INVALID
  assert fragment.encode() in lib.dqz_last_error(), lib.dqz_last_error()
