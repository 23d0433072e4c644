"""CPU: the per-kernel checks of tests/layer_checks.py, run on products whose
quality is known: numpy's own float32 layers (BLAS summation order) pass
both bars with room; a dropped convolution tap breaks the elementwise bound;
conv1 weights cut to two bf16 pieces (16 significant bits) stay inside the
bound but break the RMS bar; and the conv-transpose restatement used for the
dX kernels equals the oracle's col2im backward."""

import numpy as np
import pytest

from dqn_mgsc_zoo_amd import networks
from oracle import learner_ref
from tests import helpers
from tests import layer_checks as lc


@pytest.fixture(scope='module')
def net_and_batch():
  params = networks.dqn_atari_network(6).init(500)
  frames, fidx, _, _, _ = helpers.random_store_contents(96, 260, 6, 501)
  s = helpers.stacks_from(frames, fidx, np.arange(4), 0)
  _, cache = learner_ref.forward(params, s)
  return params, s, cache


@pytest.mark.parametrize('layer', [1, 2])
def test_conv_dx_operands_restates_col2im(layer):
  k, st, ci, co = learner_ref.CONV_SPECS[layer]
  size = {1: 20, 2: 9}[layer]
  out = (size - k) // st + 1
  rng = np.random.default_rng(layer)
  dz = rng.standard_normal((3, out, out, co))
  w = rng.standard_normal((k, k, ci, co))
  a, wf, kt = lc.conv_dx_operands(dz, w, layer)
  want = learner_ref._col2im(dz @ w.reshape(-1, co).T, (3, size, size, ci), k, st)  # pylint: disable=protected-access
  np.testing.assert_allclose((a @ wf).reshape(want.shape), want, rtol=0, atol=1e-12)
  assert np.count_nonzero(a, axis=1).max() <= kt


def _layer_operands(params, s, cache):
  x = np.asarray(s, np.float64) / 255.0
  for i, name in enumerate(learner_ref.CONV_NAMES):
    w = params[name]['w']
    yield 'conv%d' % (i + 1), lc.conv_cols(x, i), w.reshape(-1, w.shape[-1]), params[name]['b']
    x = cache['y%d' % i].astype(np.float32)  # the next layer's input, as a kernel would read it
  fc1 = params['sequential/sequential_1/linear']
  yield 'fc1', x.reshape(x.shape[0], -1), fc1['w'], fc1['b']


def test_numpy_f32_layers_pass_both_bars(net_and_batch):
  rows = []
  for name, a, w, b in _layer_operands(*net_and_batch):
    got = a.astype(np.float32) @ w + b  # BLAS sgemm
    assert got.dtype == np.float32
    rows.append((name, lc.product_check(got, a, w, b)))
  lc.report(rows)
  for _, r in rows:
    assert r['max_over_bound'] < 0.1


def test_a_dropped_tap_breaks_the_bound(net_and_batch):
  for name, a, w, b in _layer_operands(*net_and_batch):
    if not name.startswith('conv'):
      continue
    cin = w.shape[0] // {'conv1': 64, 'conv2': 16, 'conv3': 9}[name]
    damaged = w.copy()
    damaged[:cin] = 0  # tap (kh, kw) = (0, 0)
    r = lc.product_check(a.astype(np.float32) @ damaged + b, a, w, b)
    print('%s without tap (0, 0): %.0f%% of the outputs over the bound' % (name, 100 * r['frac_over']))
    assert not r['ok_bound'] and r['frac_over'] > 0.3


def test_a_two_piece_weight_split_breaks_the_rms_bar(net_and_batch):
  name, a, w, b = next(_layer_operands(*net_and_batch))
  cut = (w.view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32)  # 16 significant bits
  r = lc.product_check(a.astype(np.float32) @ cut + b, a, w, b)
  print('%s with two-piece weights: max err / bound %.3f, rms / sequential rms %.0f' % (
      name, r['max_over_bound'], r['rms_ratio']))
  assert r['ok_bound'] and not r['ok_rms'] and r['rms_ratio'] > 5 * lc.RMS_MARGIN  # measured 41
