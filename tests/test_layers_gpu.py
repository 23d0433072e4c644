"""GPU: every kernel of the learner step against the plain operation applied
to the kernel's own device input.

The other parity tests see a forward layer only through the whole network
(q at atol 1e-4) and a backward kernel only through a per-leaf norm of the
gradient; when one of them fails nothing says which kernel did it.  Here one
gradient call and one learner step run at each of the small shapes at which
the kernels branch, the intermediates of both are read back
(Learner.fetch_activations, dqz_learner_debug_activations), and

  * the two sets are bit-equal (gradient mode and step mode run the same
    forward and backward);
  * forward: y1 from the pixels, y2 from the device's y1, y3 from y2, h1 from
    y3, q from h1, for every network copy (the target's parameters for copy
    1);
  * td, loss and dz1 from the device's q and its h1 mask;
  * backward dX: dy3 from the device's dz1 and y3 > 0, dy2 from dy3 and
    y2 > 0, dy1 from dy2 and y1 > 0;
  * backward dW, db: every leaf of the flat gradient from the device's dy
    arrays (each already multiplied by its ReLU mask) and its activations.

Each comparison takes the kernel's input from the device, so no error is
inherited from the layer before and no ReLU or argmax decision can differ.
The products are held to the two bars of tests/layer_checks.py (elementwise
a-priori bound; RMS <= 4 x a sequential float32 accumulation), both
computed from the reference alone.  td, loss and dz1 are a handful of
elementwise operations with no summation order to vary, so they get the
elementwise bound only, counted operation by operation below (the RMS bar
exists to see what a (K + 3) bound with K in the hundreds cannot; with K <=
8 the bound is itself within a few roundings).

  ('dqn', 1, 6)      fc1_gemv_kernel; the 8-jobs-per-sample conv path; the
                     one-sample head + fc1 dX launch
  ('double', 5, 6)   Z = 3, shared bias, 8-job path, a partial 32-row group
  ('dqn', 32, 6)     the workload's own shape
  ('per', 40, 18)    second row group partial; 18 actions; IS weights

and at the corners of what dqz_learner_create accepts (batch 1 .. MAXB = 256,
1 .. MAXA = 32 actions), each on a limit or on the first shape past a switch:

  ('dqn', 4, 1)      the last fc1_gemv_kernel batch, all four of its rows live;
                     A = 1: max and argmax over one action, fc2 K = Z A = 2
  ('dqn', 8, 8)      Z B = 16, the last 8-job forward (fwd_conv_jobs); Z A = 16,
                     the last T = 32 reduction of head_body (lgT); the last A
                     of launch_head_z's AMAX = 8 instantiation
  ('double', 6, 8)   Z B = 18, the first 4-job forward; Z A = 24, T = 16 inside
                     AMAX = 8; shared bias
  ('per', 17, 9)     the first A on the MAXA instantiation; one row past a
                     16-row group; conv1 slabs 4 B = 68, the first
                     sum_split2_r<2> of sum_slabs
  ('double', 65, 32) the first batch off the chain grid (BWD_CHAIN_MAXB = 64);
                     conv2 / conv3 slabs 65, their first sum_split2_r<2>; A = 32
                     with Z = 3: all 96 q threads and every s_red column live;
                     conv1 slabs 260, the loop form with a tail
  ('dqn', 129, 32)   conv2 / conv3 slabs 129, their first loop form; 32
                     separate fc2 biases (nb2 = 32)
  ('per', 256, 18)   MAXB: sixteen full 16-row groups, all LR = 4 rounds of the
                     update kernel's loss partials, conv1 slabs 1024; IS weights

The GPU side of every shape is one gradient call and one step.  On the host,
above 64 samples the per-sample products (forward, dX) are checked on
layer_checks.boundary_samples(B) only, and the dW / db products, which sum
over every sample, take K in pieces of 16 samples (tests/layer_checks.py).
Host time of a shape's fixture and five tests together, as pytest's durations
report it (HOST_SECONDS below): under 2 s for every shape, the whole file
10 s, with under 1 GB resident.
"""

import types

import numpy as np
import pytest
import torch

from oracle import learner_ref
from tests import helpers
from tests import layer_checks as lc

pytestmark = pytest.mark.gpu

SHAPES = [('dqn', 1, 6), ('double', 5, 6), ('dqn', 32, 6), ('per', 40, 18),
          ('dqn', 4, 1), ('dqn', 8, 8), ('double', 6, 8), ('per', 17, 9),
          ('double', 65, 32), ('dqn', 129, 32), ('per', 256, 18)]
# measured host seconds per new shape: the fixture's host work and the five tests (the GPU's share is one
# gradient call and one step, under 10 ms)
HOST_SECONDS = {('dqn', 4, 1): 0.1, ('dqn', 8, 8): 0.3, ('double', 6, 8): 0.3, ('per', 17, 9): 0.6,
                ('double', 65, 32): 0.7, ('dqn', 129, 32): 1.0, ('per', 256, 18): 1.8}
DW_CHUNK = 16  # samples per piece of K in the dW products
FWD = ('y1', 'y2', 'y3', 'h1', 'q')
BWD = ('dz1', 'dy3', 'dy2', 'dy1')
_FC1 = 'sequential/sequential_1/linear'
_FC2 = 'sequential/sequential_1/linear_1'
BOUND = 1.0 / 32


def _fetch_all(lrn, copies):
  out = []
  for z in range(copies):
    act = lrn.fetch_activations(z, backward=z == 0)
    out.append({k: v.cpu().numpy() for k, v in act.items()})
  return out


@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: '%s-%d-%d' % s)
def run(request, device):
  """One gradient call, then one learner step from the same state, with
  everything either leaves behind, on an unfiltered batch."""
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import networks
  from dqn_mgsc_zoo_amd import store as store_lib
  algo, batch, a = request.param
  seed = 31 + batch
  net = networks.dqn_atari_network(a) if algo == 'dqn' else networks.double_dqn_atari_network(a)
  online = net.init(seed)
  target = helpers.perturbed_tree(online, seed + 1)
  lrn = learner_lib.Learner(net, batch, algo=algo)
  lrn.set_params(online, target)
  frames, fidx, action, reward, discount = helpers.random_store_contents(96, 260, a, seed + 3)
  st = store_lib.FrameStore(96, 260)
  for name, arr in (('frames', frames), ('fidx', fidx), ('action', action),
                    ('reward', reward), ('discount', discount)):
    getattr(st, name).copy_(torch.from_numpy(arr))
  rng = np.random.default_rng(batch)
  slots = rng.integers(0, 96, size=batch).astype(np.int32)
  weights = rng.uniform(0.2, 1.0, size=batch).astype(np.float32) if algo == 'per' else None
  slots_d = torch.from_numpy(slots).to(device)
  w_d = None if weights is None else torch.from_numpy(weights).to(device)
  copies = 2 if algo == 'dqn' else 3
  grad = lrn.grad(st, slots_d, w_d)
  after_grad = _fetch_all(lrn, copies)
  lrn.step(st, slots_d, w_d)
  q, td, loss = [x.cpu().numpy() for x in lrn.fetch_outputs()]
  after_step = _fetch_all(lrn, copies)
  assert lrn.sync_status() == 0
  return types.SimpleNamespace(
      algo=algo, batch=batch, a=a, copies=copies, online=online, target=target,
      s=(helpers.stacks_from(frames, fidx, slots, 0), helpers.stacks_from(frames, fidx, slots, 1)),
      action=action[slots].astype(np.int64), reward=reward[slots], discount=discount[slots],
      weights=np.ones(batch, np.float32) if weights is None else weights,
      grad=net.unflatten(grad.cpu().numpy()), act=after_grad, act_step=after_step,
      td=td, loss=loss, lrn=lrn, net=net, sel=lc.sample_subset(batch))


def test_gradient_and_step_leave_the_same_intermediates(run):
  for z in range(run.copies):
    for k in FWD + (BWD if z == 0 else ()):
      g, s = run.act[z][k], run.act_step[z][k]
      assert np.array_equal(g.view(np.uint32), s.view(np.uint32)), (z, k)
  np.testing.assert_array_equal(run.act[0]['q'].shape, (run.batch, run.a))
  # the outputs the step publishes are the same arrays
  np.testing.assert_array_equal(run.lrn.fetch_outputs()[0].cpu().numpy(), run.act_step[0]['q'])


def test_a_network_copy_the_learner_does_not_have_is_refused(run):
  from dqn_mgsc_zoo_amd import _native
  for z in (-1, run.copies):
    with pytest.raises(_native.NativeLibraryError, match='z must be in'):
      run.lrn.fetch_activations(z)


def _b2(params, shared):
  return params['sequential/sequential_1']['b'] if shared else params[_FC2]['b']


def test_forward_kernels(run):
  rows = []
  for z in range(run.copies):
    p = run.target if z == 1 else run.online
    act = {k: lc.take_samples(v, run.batch, run.sel) for k, v in run.act[z].items() if k in FWD}
    x = np.asarray(run.s[0 if z == 0 else 1][run.sel], np.float64) / 255.0
    for i, name in enumerate(learner_ref.CONV_NAMES):
      w = p[name]['w']
      y = act['y%d' % (i + 1)]
      rows.append(('z%d conv%d' % (z, i + 1), lc.product_check(
          y, lc.conv_cols(x, i), w.reshape(-1, w.shape[-1]), p[name]['b'], relu=True)))
      x = y
    flat = act['y3'].reshape(len(run.sel), -1)
    rows.append(('z%d fc1' % z, lc.product_check(act['h1'], flat, p[_FC1]['w'], p[_FC1]['b'],
                                                 relu=True)))
    rows.append(('z%d fc2' % z, lc.product_check(act['q'], act['h1'], p[_FC2]['w'],
                                                 _b2(p, run.algo != 'dqn'))))
  lc.report(rows)


def _head(run, dtype):
  """td, per-sample loss terms and the cotangent g at td from the device's q,
  in `dtype` arithmetic, operation by operation as head.hpp states them
  (without its fused multiply-add when dtype is float32); also M, the
  magnitude td's rounding is relative to."""
  f = dtype
  idx = np.arange(run.batch)
  q0 = run.act[0]['q'].astype(f)
  q1 = run.act[1]['q'].astype(f)
  if run.algo == 'dqn':
    v = q1.max(axis=1)
  else:  # first maximum of the device's own online q(s_t): no near-tie can differ
    v = q1[idx, np.argmax(run.act[2]['q'], axis=1)]
  r, d, w = run.reward.astype(f), run.discount.astype(f), run.weights.astype(f)
  qa = q0[idx, run.action]
  td = (r + d * v) - qa
  terms = f(0.5) * td * td * w
  g = np.clip(w * td / f(run.batch), f(-BOUND), f(BOUND))
  mag = np.abs(r) + np.abs(d * v) + np.abs(qa)
  return td, terms, g, mag


def test_head_td_loss_dz1(run):
  """Bounds, in units of 2^-24: td = fl(fl(r + d v) - qa) rounds at most
  three times (two with the kernel's fused multiply-add), each relative to
  at most M = |r| + |d v| + |qa|: 4 M with one to spare.  g = clip(fl(fl(w
  td) / B)) adds two roundings and dz1 = fl(-g W2[:, a]) one, all relative
  to at most (w / B) M: 8 (w / B) M |W2[:, a]|.  loss = (sum_b 0.5 td_b^2
  w_b) / B: each term inherits w |td| 4 M from td and rounds three times,
  the sum and the division B + 1 times."""
  td, terms, g, mag = _head(run, np.float64)
  e_td = np.abs(run.td - td) / (4 * lc.EPS * mag)
  loss = terms.mean()
  loss_bound = lc.EPS * ((run.weights * np.abs(td) * 4 * mag + 3 * terms).sum() +
                         (run.batch + 1) * terms.sum()) / run.batch
  e_loss = abs(float(run.loss[0]) - loss) / loss_bound
  w2 = np.asarray(run.online[_FC2]['w'], np.float64)[:, run.action].T  # [B, 512]
  mask = run.act[0]['h1'] > 0
  dz1 = -g[:, None] * w2 * mask
  dz_bound = 8 * lc.EPS * (run.weights / run.batch * mag)[:, None] * np.abs(w2)
  err = np.abs(run.act[0]['dz1'] - dz1)
  with np.errstate(divide='ignore', invalid='ignore'):
    e_dz = np.where(err > 0, err / dz_bound, 0.0)
  print('td max err / bound %.4f, loss err / bound %.4f, dz1 max err / bound %.4f' % (
      e_td.max(), e_loss, e_dz.max()))
  assert e_td.max() <= 1.0 and e_loss <= 1.0 and e_dz.max() <= 1.0
  np.testing.assert_array_equal(run.act[0]['dz1'][~mask], 0.0)


def test_backward_dx_kernels(run):
  p = run.online
  act = {k: lc.take_samples(v, run.batch, run.sel) for k, v in run.act[0].items()}
  rows = [('fc1 dX (dy3)', lc.product_check(
      act['dy3'], act['dz1'], p[_FC1]['w'].T, mask=act['y3'].reshape(len(run.sel), -1) > 0))]
  for layer, dy_out, dy_in, y in ((2, 'dy2', 'dy3', 'y2'), (1, 'dy1', 'dy2', 'y1')):
    a, wf, k = lc.conv_dx_operands(act[dy_in], p[learner_ref.CONV_NAMES[layer]]['w'], layer)
    rows.append(('conv%d dX (%s)' % (layer + 1, dy_out), lc.product_check(
        act[dy_out], a, wf, k_terms=k, mask=act[y].reshape(-1, act[y].shape[-1]) > 0)))
  lc.report(rows)


def test_backward_dw_kernels(run):
  act, g = run.act[0], run.grad
  n = run.batch
  rows = []
  x = run.s[0]
  for i, name in enumerate(learner_ref.CONV_NAMES):
    dy4 = act['dy%d' % (i + 1)]
    dy = dy4.reshape(-1, dy4.shape[-1])
    w = g[name]['w']

    def pieces(x=x, dy4=dy4, i=i):  # K = (sample, oh, ow), DW_CHUNK samples at a time
      for lo in range(0, n, DW_CHUNK):
        xc = np.asarray(x[lo:lo + DW_CHUNK], np.float64)
        yield (lc.conv_cols(xc / 255.0 if i == 0 else xc, i).T,
               dy4[lo:lo + DW_CHUNK].reshape(-1, dy4.shape[-1]))

    rows.append(('conv%d dW' % (i + 1), lc.product_check(w.reshape(-1, w.shape[-1]), pieces(), None)))
    rows.append(('conv%d db' % (i + 1), lc.product_check(
        g[name]['b'], np.ones((1, dy.shape[0])), dy)))
    x = act['y%d' % (i + 1)]
  rows.append(('fc1 dW', lc.product_check(g[_FC1]['w'], act['y3'].reshape(n, -1).T, act['dz1'])))
  rows.append(('fc1 db', lc.product_check(g[_FC1]['b'], np.ones((1, n)), act['dz1'])))
  # fc2: the kernel forms the cotangent dq itself (g at the taken action)
  _, _, g64, mag = _head(run, np.float64)
  _, _, g32, _ = _head(run, np.float32)
  dq, dq32, dq_mag = (np.zeros((n, run.a), t) for t in (np.float64, np.float32, np.float64))
  idx = np.arange(n)
  dq[idx, run.action] = -g64
  dq32[idx, run.action] = -g32
  dq_mag[idx, run.action] = run.weights / n * mag
  kw = dict(k_terms=n + 8, w_mag=dq_mag, w_seq=dq32)
  rows.append(('fc2 dW', lc.product_check(g[_FC2]['w'], act['h1'].T, dq, **kw)))
  if run.algo == 'dqn':
    rows.append(('fc2 db', lc.product_check(g[_FC2]['b'], np.ones((1, n)), dq, **kw)))
  else:
    rows.append(('shared bias db', lc.product_check(
        g['sequential/sequential_1']['b'], np.ones((1, n)), dq.sum(axis=1, keepdims=True),
        k_terms=n + 8, w_mag=dq_mag.sum(axis=1, keepdims=True),
        w_seq=dq32.sum(axis=1, keepdims=True))))
  lc.report(rows)


# -- the actor at the ends of the action range, on the same learners ---------------

def _observation(run):
  return np.ascontiguousarray(run.s[1][0])


@pytest.mark.parametrize('run', [('dqn', 4, 1)], indirect=True, ids=['dqn-4-1'])
def test_act_with_one_action_returns_it_for_every_epsilon(run):
  """A = 1: the greedy action and the uniform draw over one action are both
  action 0, and max_a q is q[0]."""
  obs = _observation(run)
  dev = run.lrn.online.device
  q = run.lrn.q_values(torch.from_numpy(obs[None]).to(dev))[0].cpu().numpy()
  assert q.shape == (1,)
  for eps in (0.0, 0.3, 1.0):
    for c in range(40):
      a, v = run.lrn.act(obs, eps, seed=5, counter=c)
      assert a == 0 and v == q[0], (eps, c, a, v)


@pytest.mark.parametrize('run', [('dqn', 129, 32)], indirect=True, ids=['dqn-129-32'])
def test_act_ties_at_the_first_and_last_of_32_actions(run):
  """tests/test_actor_gpu.py's tie-spreading check at A = MAXA: W2 = 0 and
  the bias 0.25 at actions 0 and 31, 0 between, so the greedy mass is split
  between the two ends of the action range and nothing else is drawn."""
  tied = {m: {n: v.copy() for n, v in d.items()} for m, d in run.online.items()}
  tied[_FC2]['w'][...] = 0.0
  tied[_FC2]['b'][...] = 0.0
  tied[_FC2]['b'][[0, 31]] = 0.25
  obs = _observation(run)
  run.lrn.set_params(tied, run.target)
  try:
    n = 1800
    counts = np.zeros(32)
    for c in range(n):
      a, v = run.lrn.act(obs, 0.0, seed=1, counter=c)
      counts[a] += 1
      assert v == 0.25
  finally:
    run.lrn.set_params(run.online, run.target)
  print('greedy counts at actions 0 and 31:', counts[0], counts[31])
  assert counts[1:31].sum() == 0
  np.testing.assert_allclose(counts[[0, 31]] / n, [0.5, 0.5], atol=4 * np.sqrt(0.25 / n))
