"""GPU: the quantile (QR-DQN) learner step, actor and agent (csrc/qr.hpp,
dqz_qr_*) against tests/qr_ref.py (float64), after tests/test_c51_gpu.py test
for test.

Store: tests/test_learner_gpu.py's (helpers.random_store_contents: capacity
256, 640 frames), rewards in {-1, 0, 1}, a tenth of the discounts 0, with two
edits: the last action is never taken (so every batch has an absent action),
and one slot (SPECIAL) has reward 3 and discount 0, so its every t_j is 3 and
its every |delta_ij| exceeds kappa; that slot is in every single-step batch.
Each batch also has a zero discount among the other samples and an action taken
at least twice.

Parameters (test data): networks.init's tree, the target perturbed
(helpers.perturbed_tree), with the fc2 bias of both trees edited, because the
quantile values of a freshly initialised head lie within a few tenths of 0:
then every delta of a sample has the sign of its reward, and the greedy
action's margin is a rounding matter.
  spread   bias[i A + a] += S s_i for every action, s_i = (2 tau_i - 1) /
           (2 tau_{N-1} - 1) in [-1, 1] (a sorted quantile function): S = 1.6
           online, so theta spans +-1.6 and straddles every t_j of a reward in
           {-1, 0, 1} while staying below the special sample's t = 3 - kappa;
           S = 0.2 in the target.  The spread's mean over i is 0: q_values keep
           their size.
  offset   bias[i A + a] += 0.1 for one action of each tree (_case's best_t
           and best_o, neither action 0, so `first maximum` is not what
           picks it): the best-versus-second q_values margin is then near 0.1,
           and stays there when the target is synced from the online tree.
Every test asserts, in float64 on the CPU before any device result is read:
the conditions above; that the target's best-versus-second q_values margin is
>= 100 x the end-to-end q_values tolerance (1e-4 max|x|); that at kappa = 1
pairs lie on both sides of |delta| = kappa and that deltas of both signs occur
in every sample but the special one (whose deltas all exceed +kappa: the two
conditions exclude each other there); at the small kappa (0.25) that at least
10 % of all pairs lie on each side.  The seeds below were chosen on the CPU for
that.

Stage checks, from the device's own inputs (u = 2^-24, N quantiles).  In
float32, from the same outputs x:
  q_values   an N-term sum and one division: (N + 1) u mean_i |x[i, a]|.
  theta      a copy: bit-equal to the taken column of the outputs.
  dtheta     t_j = fma(d, x, r) is rounded once, u |t_j|; the subtraction adds
             u |delta_ij|: |delta^_ij - delta_ij| <= u (|t_j| + |delta_ij|).
             g = w clip(delta) has slope <= 1 in delta (w <= 1) and its product
             one rounding, u |g_ij|; the N-term sum, the rounding of
             w = |tau_i - 1| and the division add (N + 2) u sum_j |g_ij|:
             [sum_j (u (|t_j| + |delta_ij|) + u |g_ij|) + (N + 2) u sum_j
             |g_ij|] / (N B).
  loss_b     the same with Lipschitz constant kappa (H_k's slope is at most
             kappa) and l_ij = w_ij H_k(delta_ij), whose evaluation has at most
             five roundings in either form (0.5 m^2 + k (|x| - m): m m, the
             difference, its product, the sum; or c (delta - c / 2) with c =
             clip(delta): two; then the product with w); two levels of sums,
             N terms each, and the division by N:
             sum_ij (kappa u (|t_j| + |delta_ij|) + 5 u l_ij) / N + (2 N + 2) u
             loss_b.
  dz1, dW2, db2  sums of N (dz1: the dense K holds N non-zero terms, and adding
             an exact zero costs nothing in any order) or at most B (fc2)
             products: per element (terms + 1) u sum |term|, from the device's
             own h1 and dtheta.
The fc2 product itself (the device's h1 through a float64 fc2) is held to atol
1e-5, as the issue sets.

End to end (kink-free batches, or the device's ReLU masks and a* pinned in the
oracle for the carried steps): outputs atol 1e-4, q_values atol 1e-4 max|x|,
mean loss rtol 1e-4, and after one chain(clip_by_global_norm(10), adam) step
tests/test_optimizers_gpu.py's bars: params atol 2e-6, moments rtol 1e-3 with
atol 2e-9 (m) and 1e-12 (v), grad_norm rtol 1e-4.

Corners of what dqz_qr_create accepts (batch 2 .. 256, 1 .. 32 actions, 1 ..
256 quantiles, A N <= 4096), all at kappa = 1, each on a limit or a switch of
the head's kernels:
  (2, 1, 1)      every minimum at once
  (6, 3, 9)      jn = 4: the third j-range holds one odd element and the fourth
                 is empty
  (17, 16, 256)  N = QR_MAXN: thread i of a quarter owns quantile i with none to
                 spare; A N = 4096: s_x and QR_LOADS exactly full; one sample
                 past a 16-row tile
  (33, 32, 128)  A = MAXA; A N = 4096
  (4, 20, 201)   A N = 4020: `tot` is short of the eight loads per thread, and
                 the last K group of qr_dz1_kernel is partial (4020 mod 16 = 4);
                 the last action is taken (LAST_TAKEN: this store drops action 0
                 instead), so dout's last column is not zero
  (256, 2, 8)    MAXB (the stage test only: every kernel of the head is checked
                 there from its own device input, and the torso at B = 256 is
                 tests/test_layers_gpu.py's)
Input conditions a corner makes impossible are waived by name (WAIVED), never
silently; every other condition is asserted, here and, without a GPU, in
tests/test_qr_cpu.py:
  shape         waived              why
  (2, 1, 1)     absent action       A = 1: the one action is every sample's
                best action not 0   A = 1: action 0 is the only one (a* = 0 is
                                    still asserted)
                margin              A = 1: there is no second-best q_value
                both signs          N = 1: a sample has one delta
  (256, 2, 8)   kink-free draw      not needed: the stage test takes each
                                    kernel's input from the device, and 256
                                    samples at a ReLU margin of 1e-6 are not to
                                    be had
B = 2 holds SPECIAL, a zero discount among the others and a repeated action at
once only because A = 1 makes every action a repeat; nothing is waived for it.
At N = 1 the pairs on both sides of |delta| = kappa are still asserted: the
special sample's lies outside, the other sample's inside.
Host time of the new cases (the oracle's step, computed once per shape, and
both tests' float64 references): under 2 s each; the most are (33, 32, 128)
and (256, 2, 8).
"""

import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import learner_ref
from tests import fake_env
from tests import helpers
from tests import qr_ref
from tests.test_trajectory_gpu import _batch

pytestmark = pytest.mark.gpu

LR, ADAM_EPS, B1, B2, CLIP = 5e-5, 0.01 / 32, 0.9, 0.999, 10.0  # qrdqn/run_atari.py:81-85, 213-219
KAPPA, SMALL_KAPPA = 1.0, 0.25
U = 2.0**-24
SPECIAL = 7  # the slot whose reward puts every |delta| beyond kappa
SPECIAL_REWARD = 3.0
SPREAD_ONLINE, SPREAD_TARGET, OFFSET = 1.6, 0.2, 0.1
# (B, A, N, kappa) -> seed; chosen on the CPU for the input conditions (and the kink-free draw)
CASES = {(5, 3, 7, KAPPA): 1, (6, 4, 65, KAPPA): 1, (8, 6, 201, KAPPA): 1, (8, 18, 201, KAPPA): 1,
         (32, 6, 201, KAPPA): 1, (8, 6, 201, SMALL_KAPPA): 1,
         (2, 1, 1, KAPPA): 0, (6, 3, 9, KAPPA): 0, (17, 16, 256, KAPPA): 0, (33, 32, 128, KAPPA): 0,
         (4, 20, 201, KAPPA): 0, (256, 2, 8, KAPPA): 5}
CASE_IDS = ['%dx%dx%d-kappa%g' % c for c in CASES]
CORNERS = [(2, 1, 1, KAPPA), (6, 3, 9, KAPPA), (17, 16, 256, KAPPA), (33, 32, 128, KAPPA), (4, 20, 201, KAPPA),
           (256, 2, 8, KAPPA)]
STAGE_ONLY = [(256, 2, 8, KAPPA)]  # no end-to-end step: see the docstring
# Shapes whose store never takes action 0 instead of the last one, and whose batch holds the last action: only
# then is the last column of dout (quantile N - 1 of action A - 1) non-zero, so that a tail of qr_dz1_kernel or
# qr_fc2_grad_kernel that is one column short shows.  With one action (2, 1, 1) shows it too.
LAST_TAKEN = [(4, 20, 201, KAPPA)]
STEP_CASES = [c for c in CASES if c not in STAGE_ONLY]
WAIVED = {(2, 1, 1, KAPPA): {'absent action', 'best action not 0', 'margin', 'both signs'},
          (256, 2, 8, KAPPA): {'kink-free draw'}}
HEAD = 'sequential/sequential_1/linear_1'


def _f32(x):
  return float(np.float32(x))


def _optimizer(clip=CLIP):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  opt = learner_lib.adam(LR, B1, B2, ADAM_EPS)
  return opt if clip is None else learner_lib.chain(learner_lib.clip_by_global_norm(clip), opt)


def _margin(q):
  s = np.sort(np.asarray(q, np.float64), axis=1)
  return float((s[:, -1] - s[:, -2]).min())


def _waived(case, what):
  return what in WAIVED.get(case['shape'], ())


def _store_contents(a, seed, last_taken=False):
  frames, fidx, action, reward, discount = helpers.random_store_contents(256, 640, a, seed + 3)
  if last_taken:
    action[action == 0] = a - 1
  else:
    action[action == a - 1] = 0
  reward[SPECIAL] = SPECIAL_REWARD
  discount[SPECIAL] = 0.0
  return dict(frames=frames, fidx=fidx, action=action, reward=reward, discount=discount)


def _edit_bias(tree, tau, a, spread, best):
  """The docstring's spread and offset on a copy of `tree`'s fc2 bias."""
  tree = {m: dict(d) for m, d in tree.items()}
  s = (2.0 * tau.astype(np.float64) - 1.0)
  s = s / s[-1] if s[-1] > 0 else s
  bias = tree[HEAD]['b'].astype(np.float64).reshape(len(tau), a) + spread * s[:, None]
  bias[:, best] += OFFSET
  tree[HEAD]['b'] = bias.reshape(-1).astype(np.float32)
  return tree


@functools.lru_cache(maxsize=None)
def _case(b, a, n, kappa):
  """Host side of one case, computed once: parameters, store contents, a
  kink-free batch meeting the input conditions, and the oracle's step from
  zero moments.  Nothing in it is modified by the tests."""
  from dqn_mgsc_zoo_amd import networks
  seed = CASES[(b, a, n, kappa)]
  tau = qr_ref.make_quantiles(n)
  net = networks.qr_atari_network(a, tau)
  best_t, best_o = (1 + seed % (a - 1), 1 + (seed + 1) % (a - 1)) if a > 1 else (0, 0)
  init = net.init(seed)
  online = _edit_bias(init, tau, a, SPREAD_ONLINE, best_o)
  target = _edit_bias(helpers.perturbed_tree(init, seed + 1), tau, a, SPREAD_TARGET, best_t)
  last_taken = (b, a, n, kappa) in LAST_TAKEN
  host = _store_contents(a, seed, last_taken)
  rng = np.random.default_rng(seed + 5)
  for _ in range(400):
    slots = rng.integers(0, 256, size=b).astype(np.int32)
    slots[0] = SPECIAL
    counts = np.bincount(host['action'][slots], minlength=a)
    if not (host['discount'][slots[1:]] == 0).any() or counts.max() < 2 or (last_taken and counts[-1] == 0):
      continue
    if 'kink-free draw' in WAIVED.get((b, a, n, kappa), ()):
      break
    if learner_ref.relu_margin(online, helpers.stacks_from(host['frames'], host['fidx'], slots, 0)) >= 1e-6:
      break
  else:
    raise AssertionError('no batch meets the input conditions')
  zeros = learner_ref.zeros_like_tree(online)
  ref = qr_ref.learner_step(online, target, zeros, zeros, 0, _batch(host, slots), tau, kappa, a,
                            _f32(LR), _f32(B1), _f32(B2), _f32(ADAM_EPS), clip=_f32(CLIP))
  return dict(net=net, tau=tau, kappa=kappa, online=online, target=target, host=host, slots=slots, ref=ref,
              zeros=zeros, best_t=best_t, shape=(b, a, n, kappa), absent=0 if last_taken else a - 1)


def _xmax(ref):
  return float(max(np.abs(ref['out_tm1']).max(), np.abs(ref['out_target_t']).max()))


def _check_conditions(case, ref=None, slots=None, single=True):
  """The input conditions, from the float64 oracle alone."""
  ref = case['ref'] if ref is None else ref
  slots = case['slots'] if slots is None else slots
  host, kappa = case['host'], case['kappa']
  if not _waived(case, 'margin'):
    margin, need = _margin(ref['q_target_t']), 100 * 1e-4 * _xmax(ref)
    print('target q_values margin %.3e, 100 x the q_values tolerance %.3e' % (margin, need))
    assert margin >= need
  assert set(np.unique(host['reward'][np.arange(256) != SPECIAL])) <= {-1.0, 0.0, 1.0}
  if not single:
    return
  counts = np.bincount(host['action'][slots], minlength=case['net'].num_actions)
  assert counts.max() >= 2
  assert counts[case['absent']] == 0 or _waived(case, 'absent action')
  assert counts[-1] >= 1 or case['shape'] not in LAST_TAKEN
  i = list(slots).index(SPECIAL)
  others = np.arange(len(slots)) != i
  assert (host['discount'][slots][others] == 0).any()
  assert host['reward'][SPECIAL] == SPECIAL_REWARD and (np.abs(ref['delta'][i]) > kappa).all()
  assert (ref['a_star'] == case['best_t']).all()
  assert case['best_t'] != 0 or _waived(case, 'best action not 0')
  inside = np.abs(ref['delta']) < kappa
  print('pairs inside kappa: %.1f %%' % (100 * inside.mean()))
  if kappa == KAPPA:
    assert inside.any() and (~inside).any()
  else:
    assert inside.mean() >= 0.1 and (~inside).mean() >= 0.1
  if not _waived(case, 'both signs'):
    for s in np.flatnonzero(others):
      assert (ref['delta'][s] < 0).any() and (ref['delta'][s] > 0).any(), s


def _device(case, device, batch=None, clip=CLIP, optimizer=None):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import store as store_lib
  lrn = learner_lib.QrLearner(case['net'], len(case['slots']) if batch is None else batch,
                              huber_param=case['kappa'], optimizer=optimizer or _optimizer(clip), device=device)
  lrn.set_params(case['online'], case['target'])
  st = store_lib.FrameStore(256, 640)
  for name, arr in case['host'].items():
    getattr(st, name).copy_(torch.from_numpy(arr))
  return lrn, st


def _compare_tree(got, want, atol, rtol=0.0, what=''):
  for m in want:
    for n in want[m]:
      np.testing.assert_allclose(got[m][n], want[m][n], atol=atol, rtol=rtol,
                                 err_msg='%s %s/%s' % (what, m, n))


def _np(t):
  return t.detach().cpu().numpy()


def _bits(t):
  return _np(t).view(np.int32).copy()


def _within(got, want, bound, what):
  err = np.abs(np.asarray(got, np.float64) - want)
  bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
  worst = int(np.argmax(err / np.maximum(bound, 1e-300)))
  print('%s: err / bound at most %.3f (err %.3e, bound %.3e)' % (
      what, err.flat[worst] / max(bound.flat[worst], 1e-300), err.flat[worst], bound.flat[worst]))
  assert (err <= bound).all(), (what, worst, err.flat[worst], bound.flat[worst])


@pytest.mark.parametrize('shape', list(CASES), ids=CASE_IDS)
def test_stages_from_the_devices_own_inputs(device, shape):
  b, a, n, kappa = shape
  case = _case(*shape)
  _check_conditions(case)
  lrn, st = _device(case, device)
  host, slots, tau = case['host'], case['slots'], case['tau'].astype(np.float64)
  g = lrn.grad(st, torch.from_numpy(slots).to(device))
  theta, qv, loss_b, loss, a_star = [_np(x) for x in lrn.fetch_outputs()]
  out, dth = [_np(x) for x in lrn.fetch_head()]
  act0 = lrn.fetch_activations(0, backward=True)
  h1 = [_np(act0['h1']).astype(np.float64), _np(lrn.fetch_activations(1)['h1']).astype(np.float64)]
  dz1 = _np(act0['dz1'])
  assert lrn.sync_status() == 0
  # fc2: the device's h1 through a float64 fc2
  for zc, tree in enumerate((case['online'], case['target'])):
    want = h1[zc] @ tree[HEAD]['w'].astype(np.float64) + tree[HEAD]['b'].astype(np.float64)
    np.testing.assert_allclose(out[zc].reshape(b, -1), want, atol=1e-5, err_msg='outputs of copy %d' % zc)
  # everything behind the outputs, from the device's outputs
  acts, r, d = host['action'][slots], host['reward'][slots], host['discount'][slots]
  ref = qr_ref.quantile_loss(out[0], acts, r, d, out[1], tau, kappa)
  assert _waived(case, 'margin') or _margin(ref['q_target_t']) >= 100 * 1e-4 * float(np.abs(out).max())
  np.testing.assert_array_equal(a_star, ref['a_star'])
  assert np.array_equal(theta.view(np.int32), out[0][np.arange(b), :, acts].view(np.int32))
  for zc, name in enumerate(('q_tm1', 'q_target_t')):
    _within(qv[zc], ref[name], (n + 1) * U * np.abs(out[zc]).astype(np.float64).mean(axis=1), 'q_values %d' % zc)
  t_abs = np.abs(ref['t'])[:, None, :]  # [B, 1, j]
  d_abs, g_abs = np.abs(ref['delta']), np.abs(ref['g'])
  bound = ((U * (t_abs + d_abs) + U * g_abs).sum(axis=2) + (n + 2) * U * g_abs.sum(axis=2)) / (n * b)
  _within(dth, ref['dtheta'], bound, 'dtheta')
  l = np.abs(tau[None, :, None] - (ref['delta'] < 0)) * qr_ref.huber(ref['delta'], kappa)
  bound = (kappa * U * (t_abs + d_abs) + 5 * U * l).sum(axis=(1, 2)) / n + (2 * n + 2) * U * ref['loss_b']
  _within(loss_b, ref['loss_b'], bound, 'loss_b')
  _within(loss[0], np.mean(loss_b.astype(np.float64)), (b + 1) * U * np.abs(loss_b).mean(), 'mean loss')
  # dz1 and the fc2 gradient leaves, from the device's h1 and dtheta
  w2 = case['online'][HEAD]['w'].astype(np.float64).reshape(512, n, a)
  d64 = dth.astype(np.float64)
  wa = w2[:, :, acts].transpose(2, 0, 1)  # [B, 512, N]
  mask = h1[0] > 0
  _within(dz1, np.einsum('bi,bji->bj', d64, wa) * mask,
          (n + 1) * U * np.einsum('bi,bji->bj', np.abs(d64), np.abs(wa)) + 1e-45, 'dz1')
  onehot = (acts[:, None] == np.arange(a)[None, :]).astype(np.float64)  # [B, A]
  gw = np.einsum('bj,ba,bi->jia', h1[0], onehot, d64).reshape(512, n * a)
  gw_abs = np.einsum('bj,ba,bi->jia', np.abs(h1[0]), onehot, np.abs(d64)).reshape(512, n * a)
  gb = np.einsum('ba,bi->ia', onehot, d64).reshape(-1)
  gb_abs = np.einsum('ba,bi->ia', onehot, np.abs(d64)).reshape(-1)
  got = case['net'].unflatten(_np(g))
  _within(got[HEAD]['w'], gw, (b + 1) * U * gw_abs + 1e-45, 'dW2')
  _within(got[HEAD]['b'], gb, (b + 1) * U * gb_abs + 1e-45, 'db2')
  absent = np.flatnonzero(onehot.sum(0) == 0)
  assert (absent.size >= 1 and case['absent'] in absent) or _waived(case, 'absent action')
  for aa in absent:  # all-zero bits for an action the batch does not take
    assert not got[HEAD]['w'].reshape(512, n, a)[:, :, aa].view(np.int32).any()
    assert not got[HEAD]['b'].reshape(n, a)[:, aa].view(np.int32).any()
  # every element of every leaf is written: a second call into a poisoned buffer gives the same bytes
  g2 = torch.full_like(g, float('nan'))
  lrn.grad(st, torch.from_numpy(slots).to(device), out=g2)
  offs, sizes, _ = case['net'].layout()
  for o, s in zip(offs, sizes):
    assert torch.equal(g[o:o + s].view(torch.int32), g2[o:o + s].view(torch.int32))


def _check_step(lrn, ref, what, head=None):
  """One device step against qr_ref.learner_step's result `ref`."""
  theta, qv, loss_b, loss, a_star = [_np(x) for x in lrn.fetch_outputs()]
  xmax = _xmax(ref)
  np.testing.assert_array_equal(a_star, ref['a_star'])
  np.testing.assert_allclose(theta, ref['theta'], atol=1e-4, err_msg=what)
  if head is not None:
    np.testing.assert_allclose(head[0], ref['out_tm1'], atol=1e-4, err_msg=what)
    np.testing.assert_allclose(head[1], ref['out_target_t'], atol=1e-4, err_msg=what)
  np.testing.assert_allclose(qv[0], ref['q_tm1'], atol=1e-4 * xmax, err_msg=what)
  np.testing.assert_allclose(qv[1], ref['q_target_t'], atol=1e-4 * xmax, err_msg=what)
  np.testing.assert_allclose(loss[0], ref['loss'], rtol=1e-4, err_msg=what)
  np.testing.assert_allclose(float(lrn.grad_norm().item()), ref['grad_norm'], rtol=1e-4, err_msg=what)
  assert int(lrn.count.item()) == ref['count']
  _compare_tree(lrn.params_tree('online'), ref['params'], 2e-6, what=what + ' params')
  _compare_tree(lrn.params_tree('mu'), ref['mu'], 2e-9, 1e-3, what=what + ' m')
  _compare_tree(lrn.params_tree('nu'), ref['nu'], 1e-12, 1e-3, what=what + ' v')


@pytest.mark.parametrize('shape', STEP_CASES, ids=['%dx%dx%d-kappa%g' % c for c in STEP_CASES])
def test_one_step_matches_the_oracle(device, shape):
  case = _case(*shape)
  _check_conditions(case)
  lrn, st = _device(case, device)
  lrn.step(st, torch.from_numpy(case['slots']).to(device))
  head = [_np(x) for x in lrn.fetch_head()][0]
  _check_step(lrn, case['ref'], 'x'.join(map(str, shape)), head)
  _compare_tree(lrn.params_tree('target'), case['target'], 0.0, what='target')
  assert lrn.sync_status() == 0
  print('loss %.6f, gradient norm %.4f' % (case['ref']['loss'], case['ref']['grad_norm']))


TRAJ_SEED = 21  # the ten batches' draws; chosen on the CPU for the margin on every step
TRAJ_CASE = STD = (8, 6, 201, KAPPA)  # the reference's sizes at batch 8
ODD = (5, 3, 7, KAPPA)


def test_ten_carried_steps(device):
  """tests/test_trajectory_gpu.py's manner: every step the oracle starts from
  the device's own state, with the device's ReLU masks and a*; unfiltered
  batches; a target sync after step 5, bit-equal."""
  case = _case(*TRAJ_CASE)
  b, a = TRAJ_CASE[:2]
  lrn, st = _device(case, device)
  rng = np.random.default_rng(TRAJ_SEED)
  hp = [_f32(x) for x in (LR, B1, B2, ADAM_EPS)]
  for step in range(10):
    slots = rng.integers(0, 256, size=b).astype(np.int32)
    torch.cuda.synchronize()
    state = [lrn.params_tree(w) for w in ('online', 'target', 'mu', 'nu')]
    count = int(lrn.count.item())
    lrn.step(st, torch.from_numpy(slots).to(device))
    act = lrn.fetch_activations(0)
    masks = [_np(act[k]) > 0 for k in ('y1', 'y2', 'y3', 'h1')]
    a_star = _np(lrn.fetch_outputs()[4])
    ref = qr_ref.learner_step(state[0], state[1], state[2], state[3], count, _batch(case['host'], slots),
                              case['tau'], KAPPA, a, *hp, clip=_f32(CLIP), masks=masks, select=a_star)
    _check_conditions(case, ref, slots, single=False)
    np.testing.assert_array_equal(a_star, np.argmax(ref['q_target_t'], axis=1))
    _check_step(lrn, ref, 'step %d' % step, [_np(x) for x in lrn.fetch_head()][0])
    if step == 5:
      lrn.sync_target()
      torch.cuda.synchronize()
      assert torch.equal(lrn.online.view(torch.int32), lrn.target.view(torch.int32))
  assert int(lrn.count.item()) == 10 and lrn.sync_status() == 0


def _snapshot(lrn):
  return [t.clone() for t in (lrn.online, lrn.mu, lrn.nu, lrn.count)]


def _restore(lrn, snap):
  for t, s in zip((lrn.online, lrn.mu, lrn.nu, lrn.count), snap):
    t.copy_(s)


def _all_bits(lrn):
  out = [_bits(t) for t in (lrn.online, lrn.mu, lrn.nu, lrn.count, lrn.target)]
  out += [_bits(t) for t in lrn.fetch_outputs()]
  out += [_bits(t) for t in lrn.fetch_head()]
  out.append(_bits(lrn.grad_norm()))
  return out


def test_a_step_is_bit_reproducible(device):
  case = _case(*STD)
  lrn, st = _device(case, device)
  slots = torch.from_numpy(case['slots']).to(device)
  lrn.step(st, slots)  # carried moments under the repeated step
  snap = _snapshot(lrn)
  runs = []
  for _ in range(2):
    _restore(lrn, snap)
    lrn.step(st, slots)
    torch.cuda.synchronize()
    runs.append(_all_bits(lrn))
  for x, y in zip(*runs):
    assert np.array_equal(x, y)
  assert not np.array_equal(runs[0][0], _bits(snap[0]))


BINDING_CLIP = 0.1  # below the (5, 3, 7) case's gradient norm in the oracle (asserted), so the clip scales


@pytest.mark.parametrize('optimizer', ['clip_adam', 'rmsprop'])
def test_a_step_is_its_gradient_then_apply(device, optimizer):
  """tests/test_optimizers_gpu.py's test_step_opt_is_grad_then_apply for the
  quantile head: QrLearner.step leaves the bits of QrLearner.grad followed by
  dqz_optimizer_apply on the learner's own optimizer handle."""
  from dqn_mgsc_zoo_amd import _native
  from dqn_mgsc_zoo_amd import learner as learner_lib
  case = _case(*ODD)
  assert case['ref']['grad_norm'] > 2 * BINDING_CLIP
  opt = _optimizer(BINDING_CLIP) if optimizer == 'clip_adam' else learner_lib.rmsprop(LR, 0.95, 1e-6, centered=False)
  lrn, st = _device(case, device, optimizer=opt)
  slots = torch.from_numpy(case['slots']).to(device)
  for step in range(2):  # the second from carried moments
    snap = _snapshot(lrn)
    lrn.step(st, slots)
    after = _snapshot(lrn)
    gn = lrn.grad_norm().clone()
    _restore(lrn, snap)
    g = lrn.grad(st, slots)
    _native.check(_native.lib().dqz_optimizer_apply(
        lrn._opt_h, _native.ptr(lrn.online), _native.ptr(g), _native.ptr(lrn.mu),  # pylint: disable=protected-access
        _native.ptr(lrn.nu), _native.ptr(lrn.count), _native.stream_handle()))
    torch.cuda.synchronize()
    for x, y in zip(after, _snapshot(lrn)):
      assert torch.equal(x, y), step
    assert torch.equal(gn, lrn.grad_norm())
    torch.cuda.synchronize()
    assert not torch.equal(snap[0], after[0])
    if optimizer == 'clip_adam':
      assert float(gn.item()) > BINDING_CLIP and int(lrn.count.item()) == step + 1
    assert lrn.sync_status() == 0


def test_profile_names_the_heads_launches(device):
  """QrLearner.profile reports the step's own launches and the quantile
  head's four (dz1 in slot 2) under their names, and changes no state."""
  case = _case(*ODD)
  lrn, st = _device(case, device)
  slots = torch.from_numpy(case['slots']).to(device)
  state = (lrn.online, lrn.target, lrn.mu, lrn.nu, lrn.count)
  before = [t.clone() for t in state]
  ms = lrn.profile(st, slots, iters=2)
  torch.cuda.synchronize()
  print(sorted(ms))
  assert set(ms) == {
      'conv1_fwd', 'fc1_fwd', 'fc1_dx',
      'conv3_dx+conv2_dx+fc1_dw+conv3_dw+conv2_dw+conv1_dw', 'update',
      'qr_outputs', 'qr_head', 'qr_dz1', 'qr_fc2_grad'}
  for t, b in zip(state, before):
    assert np.array_equal(_bits(t), _bits(b))


def test_three_captured_steps_equal_three_eager_steps(device):
  case = _case(*STD)
  lrn, st = _device(case, device)
  slots = torch.from_numpy(case['slots']).to(device)
  snap = _snapshot(lrn)
  for _ in range(3):
    lrn.step(st, slots)
  torch.cuda.synchronize()
  eager = _all_bits(lrn)
  side = torch.cuda.Stream(device)
  side.wait_stream(torch.cuda.current_stream(device))
  with torch.cuda.stream(side):  # warm-up off the default stream, as capture requires
    lrn.step(st, slots)
  torch.cuda.current_stream(device).wait_stream(side)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(3):
      lrn.step(st, slots)
  torch.cuda.synchronize()
  _restore(lrn, snap)
  g.replay()
  torch.cuda.synchronize()
  for x, y in zip(eager, _all_bits(lrn)):
    assert np.array_equal(x, y)
  assert int(lrn.count.item()) == 3


def test_dqn_and_c51_steps_unchanged_beside_a_qr_learner(device):
  """One Learner(algo='dqn') step and one C51Learner step before and after a
  QR learner has run in the same process: identical bytes."""
  from tests import test_c51_gpu
  from tests.test_learner_gpu import _setup

  def dqn_step():
    _, lrn, st, _, _, _, _, _ = _setup('dqn', 8, seed=3)
    slots = torch.from_numpy(np.random.default_rng(5).integers(0, 256, 8).astype(np.int32)).to(device)
    lrn.step(st, slots)
    torch.cuda.synchronize()
    return [_bits(t) for t in (lrn.online, lrn.mu, lrn.nu) + tuple(lrn.fetch_outputs())]

  def c51_step():
    c51_case = test_c51_gpu._case(5, 3, 7)  # pylint: disable=protected-access
    lrn, st = test_c51_gpu._device(c51_case, device)  # pylint: disable=protected-access
    lrn.step(st, torch.from_numpy(c51_case['slots']).to(device))
    torch.cuda.synchronize()
    return [_bits(t) for t in (lrn.online, lrn.mu, lrn.nu, lrn.count) + tuple(lrn.fetch_outputs()) +
            tuple(lrn.fetch_head())]

  before = dqn_step() + c51_step()
  case = _case(*STD)
  qr, st = _device(case, device)
  qr.step(st, torch.from_numpy(case['slots']).to(device))
  qr.q_values_slots(st, torch.from_numpy(case['slots']).to(device), 0)
  torch.cuda.synchronize()
  for x, y in zip(before, dqn_step() + c51_step()):
    assert np.array_equal(x, y)


def test_actor(device):
  shape = STD[:3]
  case = _case(*STD)
  lrn, st = _device(case, device)
  host, slots = case['host'], case['slots']
  s_t = helpers.stacks_from(host['frames'], host['fidx'], slots, 1)
  out, _ = learner_ref.forward(case['online'], s_t)
  out = out.reshape(len(slots), shape[2], shape[1])
  q_ref = qr_ref.q_values(out)
  xmax = float(np.abs(out).max())
  assert _margin(q_ref) >= 100 * 1e-4 * xmax
  q_direct = lrn.q_values(torch.from_numpy(s_t).to(device))
  q_slots = lrn.q_values_slots(st, torch.from_numpy(slots).to(device), 1)
  np.testing.assert_allclose(_np(q_direct), q_ref, atol=1e-4 * xmax)
  assert torch.equal(q_direct, q_slots)
  q1 = lrn.q_values(torch.from_numpy(s_t[2:3]).to(device))  # n below the batch
  np.testing.assert_allclose(_np(q1), q_ref[2:3], atol=1e-4 * xmax)
  for i in range(3):  # greedy: argmax q_values, state_value = max_a q_values
    action, value = lrn.act(s_t[i], 0.0, seed=9, counter=i)
    assert action == int(np.argmax(q_ref[i]))
    assert abs(value - q_ref[i].max()) <= 1e-4 * xmax
  counts = np.zeros(shape[1], np.int64)
  for i in range(600):  # uniform at eps = 1: every count within 5 sd of 100
    action, value = lrn.act(s_t[0], 1.0, seed=9, counter=100 + i)
    counts[action] += 1
    assert abs(value - q_ref[0].max()) <= 1e-4 * xmax
  sd = np.sqrt(600 * (1 / 6) * (5 / 6))
  print('eps = 1 action counts', counts)
  assert (np.abs(counts - 100) <= 5 * sd).all()


def test_create_refuses_bad_quantiles_and_kappa(device):
  from dqn_mgsc_zoo_amd import _native
  lib = _native.lib()
  cfg = _native.DqzLearnerConfig(8, 6, _native.ALGO_DQN, LR, 0.0, ADAM_EPS, 0.0)
  h = ctypes.c_void_p()
  for bad, index in (([0.25, 0.0, 0.75], 1), ([0.25, 0.5, 1.0], 2), ([float('nan'), 0.5], 0)):
    tau = torch.tensor(bad, dtype=torch.float32, device=device)
    assert lib.dqz_qr_create(ctypes.byref(cfg), len(bad), _native.ptr(tau), 1.0, ctypes.byref(h)) == -1
    assert lib.dqz_last_error() == b'quantiles must be finite and strictly inside (0, 1) (quantile %d)' % index
  tau = torch.tensor([0.25, 0.75], dtype=torch.float32, device=device)
  for kappa in (0.0, float('nan')):
    assert lib.dqz_qr_create(ctypes.byref(cfg), 2, _native.ptr(tau), kappa, ctypes.byref(h)) == -1
    assert lib.dqz_last_error().startswith(
        b'huber_param must be finite and > 0 (huber_param = 0, rlax\'s plain |delta| branch, is not built)')
  # the first value past each limit, with good quantiles of that length on the device
  past = [(8, 6, 257, b'num_quantiles must be in [1, 256]'),
          (8, 17, 241, b'num_actions * num_quantiles must be <= 4096'),  # A N = 4097, N inside its own limit
          (8, 33, 124, b'num_actions must be in [1, 32]'),
          (1, 6, 201, b'batch must be in [2, 256]'),
          (257, 6, 201, b'batch must be in [2, 256]')]
  for batch, a, n, message in past:
    cfg = _native.DqzLearnerConfig(batch, a, _native.ALGO_DQN, LR, 0.0, ADAM_EPS, 0.0)
    tau = torch.from_numpy(qr_ref.make_quantiles(n)).to(device)
    assert lib.dqz_qr_create(ctypes.byref(cfg), n, _native.ptr(tau), 1.0, ctypes.byref(h)) == -1
    assert lib.dqz_last_error() == message, (batch, a, n, lib.dqz_last_error())
  # and the last value inside each is taken (the corner shapes above run on them)
  for batch, a, n in ((256, 2, 8), (2, 1, 1), (17, 16, 256), (33, 32, 128)):
    cfg = _native.DqzLearnerConfig(batch, a, _native.ALGO_DQN, LR, 0.0, ADAM_EPS, 0.0)
    tau = torch.from_numpy(qr_ref.make_quantiles(n)).to(device)
    assert lib.dqz_qr_create(ctypes.byref(cfg), n, _native.ptr(tau), 1.0, ctypes.byref(h)) == 0, lib.dqz_last_error()
    assert lib.dqz_qr_destroy(h) == 0


# -- the agent -------------------------------------------------------------------

def _agent(seed, optimizer=None, num_quantiles=201):
  from dqn_mgsc_zoo_amd import networks
  from dqn_mgsc_zoo_amd import parts
  from dqn_mgsc_zoo_amd import replay as replay_lib
  from dqn_mgsc_zoo_amd.qrdqn import agent as agent_lib
  tau = qr_ref.make_quantiles(num_quantiles)
  replay = replay_lib.TransitionReplay(1000, replay_lib.Transition(None, None, None, None, None),
                                       np.random.RandomState(seed))
  agent = agent_lib.QrDqn(
      preprocessor=fake_env.FrameStacker(),
      sample_network_input=np.zeros((84, 84, 4), np.uint8),
      network=networks.qr_atari_network(6, tau), quantiles=tau,
      optimizer=optimizer or _optimizer(),
      transition_accumulator=replay_lib.TransitionAccumulator(),
      replay=replay, batch_size=10,
      exploration_epsilon=parts.LinearSchedule(begin_t=40, decay_steps=100, begin_value=1.0, end_value=0.1),
      min_replay_capacity_fraction=0.05, learn_period=2, target_network_update_period=4,
      huber_param=1.0, rng_key=np.array([0, seed], np.uint32))
  return agent, replay


def _run(agent, num_steps, seed=1, episode_len=23):
  from dqn_mgsc_zoo_amd import parts
  env = fake_env.FakeAtari(episode_len=episode_len, seed=seed)
  loop = parts.run_loop(agent, env, max_steps_per_episode=0)
  for _ in range(num_steps):
    next(loop)


def test_agent_learns_and_syncs_the_target(device):
  """qrdqn/run_atari_test.py's sizes: replay 1000, batch 10, learn period 2,
  target period 4, N = 201."""
  agent, replay = _agent(0)
  lrn = agent.learner
  p0 = lrn.online.clone()
  assert torch.equal(lrn.online, lrn.target)  # the reference's alias at construction
  synced = []
  sync_target = lrn.sync_target

  def spy(*args, **kwargs):
    sync_target(*args, **kwargs)
    synced.append((agent._frame_t, lrn.online.clone()))  # pylint: disable=protected-access

  lrn.sync_target = spy
  _run(agent, 100)
  assert replay.size >= 50
  assert int(lrn.count.item()) >= 20  # every second frame once 50 transitions are stored
  assert not torch.equal(p0, lrn.online) and torch.isfinite(lrn.online).all()
  assert len(synced) >= 10 and all(t % 4 == 0 for t, _ in synced)
  assert torch.equal(lrn.target, synced[-1][1]) and not torch.equal(p0, lrn.target)
  assert np.isfinite(agent.statistics['state_value'])
  assert set(agent.get_state()) == {'rng_key', 'frame_t', 'opt_state', 'online_params', 'target_params', 'replay'}
  assert agent.check_learner_health() == 0


def test_agent_state_round_trip_and_checkpoint_kinds(device):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import optim_state
  a1, r1 = _agent(4)
  _run(a1, 90, seed=5)
  state = copy.deepcopy(a1.get_state())
  inner = optim_state.chained_inner(state['opt_state'])
  assert isinstance(inner[0], optim_state.ScaleByAdamState) and int(inner[0].count) > 0
  a2, r2 = _agent(99)
  a2.set_state(state)  # a checkpoint with an Adam state restores
  r2._random_state.set_state(r1._random_state.get_state())  # pylint: disable=protected-access
  assert int(a2.learner.count.item()) == int(a1.learner.count.item())
  env = fake_env.FakeAtari(episode_len=17, seed=6)
  steps = [env.reset()]
  for t in range(20):
    steps.append(env.step(t % 6) if not steps[-1].last() else env.reset())
  for ts in steps:
    if ts.first():
      a1.reset()
      a2.reset()
    assert a1.step(ts) == a2.step(ts)
  for which in ('online', 'target', 'mu', 'nu', 'count'):
    assert torch.equal(getattr(a1.learner, which), getattr(a2.learner, which))
  assert int(a1.learner.count.item()) > int(inner[0].count)  # they learned on the way
  # a DQN agent's checkpoint (centered RMSProp) is refused by name, clipped or not
  zeros = a1.learner.params_tree('mu')
  bad = dict(state, opt_state=optim_state.rmsprop_state(zeros, zeros))
  with pytest.raises(ValueError, match='centered-RMSProp state'):
    a2.set_state(bad)
  a3, _ = _agent(5, optimizer=learner_lib.adam(LR, eps=ADAM_EPS))
  with pytest.raises(ValueError, match='centered-RMSProp state'):
    a3.learner.load_opt_state(optim_state.rmsprop_state(zeros, zeros))
  with pytest.raises(NotImplementedError, match='centered'):
    _agent(6, optimizer=learner_lib.rmsprop(LR, 0.95, 1e-5, centered=True))
