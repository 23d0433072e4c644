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


# -- the sample subset and K in pieces (the large batches of tests/test_layers_gpu.py) --

NEW_BATCHES = (4, 8, 6, 17, 65, 129, 256)


@pytest.mark.parametrize('batch', NEW_BATCHES)
def test_the_subset_holds_the_boundary_samples(batch):
  got = lc.boundary_samples(batch)
  assert list(got) == sorted(set(got)) and got[0] == 0 and got[-1] == batch - 1
  for m in (16, 32, 48, 64, 128):  # both sides of each, where the batch has them
    for s in (m - 1, m):
      assert (s in got) == (s < batch), (batch, s)
  assert len(got) <= 12
  sel = lc.sample_subset(batch)
  if batch <= lc.SUBSET_ABOVE:
    assert np.array_equal(sel, np.arange(batch))
  else:
    assert np.array_equal(sel, got)


def test_take_samples_cuts_sample_major_rows():
  arr = np.arange(5 * 3 * 2).reshape(15, 2)  # 5 samples x 3 rows
  assert np.array_equal(lc.take_samples(arr, 5, [0, 4]), np.concatenate([arr[:3], arr[12:]]))
  per_sample = np.arange(5 * 4).reshape(5, 2, 2)
  assert np.array_equal(lc.take_samples(per_sample, 5, [1, 3]), per_sample[[1, 3]])


def test_a_product_damaged_in_a_selected_sample_fails(net_and_batch):
  """conv2 of a 65-sample batch (one input tiled: the products are what
  matters), checked on the subset as tests/test_layers_gpu.py does: damage
  inside a selected sample fails both ways of damaging, the clean product
  passes."""
  params, _, cache = net_and_batch
  batch = 65
  y1 = np.tile(cache['y0'][:1].astype(np.float32), (batch, 1, 1, 1))
  y1 *= np.linspace(0.5, 1.5, batch, dtype=np.float32)[:, None, None, None]  # no two samples alike
  name = learner_ref.CONV_NAMES[1]
  w, b = params[name]['w'].reshape(-1, 64), params[name]['b']
  full = (lc.conv_cols(y1, 1).astype(np.float32) @ w + b).reshape(batch, 9, 9, 64)
  sel = lc.sample_subset(batch)
  assert 64 in sel and 63 in sel and 40 not in sel

  def check(got):
    return lc.product_check(lc.take_samples(got, batch, sel), lc.conv_cols(lc.take_samples(y1, batch, sel), 1), w, b)

  r = check(full)
  assert r['ok_bound'] and r['ok_rms']
  for s in (0, 15, 16, 63, 64):  # one element of one selected sample, off by 1e-3 of its size
    bad = full.copy()
    bad[s, 4, 4, 7] += 1e-3 * max(abs(bad[s, 4, 4, 7]), 1.0)
    assert not check(bad)['ok_bound'], s
  bad = full.copy()  # sample 64 computed from sample 63's input: a row-group tail read one row low
  bad[64] = full[63]
  assert not check(bad)['ok_bound']


def test_chunked_sequential_product_is_the_unchunked_one_bit_for_bit():
  rng = np.random.default_rng(9)
  a = rng.standard_normal((37, 403)).astype(np.float32)
  w = rng.standard_normal((403, 11)).astype(np.float32)
  b = rng.standard_normal(11).astype(np.float32)
  whole = lc.seq_f32(a, w, b)
  cuts = [0, 1, 64, 65, 200, 403]  # uneven pieces, one of a single term
  acc = None
  for lo, hi in zip(cuts[:-1], cuts[1:]):
    acc = lc.seq_f32(a[:, lo:hi], w[lo:hi], b, acc=acc, last=hi == 403)
  assert np.array_equal(acc.view(np.uint32), whole.view(np.uint32))
  # and through product_check: the same bars from the pieces as from the whole
  got = a @ w + b
  one = lc.product_check(got, a, w, b)
  blocks = lc.product_check(got, [a[:, lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])],
                            [w[lo:hi] for lo, hi in zip(cuts[:-1], cuts[1:])], b)
  pairs = lc.product_check(got, ((a[:, lo:hi], w[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])), None, b)
  for r in (blocks, pairs):
    # (the fp64 reference adds its pieces in another order: 1e-16 of the values, 1e-10 of an error of 1e-6)
    assert abs(r['rms_seq'] - one['rms_seq']) <= 1e-8 * one['rms_seq']
    assert r['ok_bound'] and r['ok_rms']
    assert abs(r['max_over_bound'] - one['max_over_bound']) <= 1e-6
  # a term dropped from one piece is seen
  short = a.copy()
  short[:, 200] = 0
  assert not lc.product_check(short @ w + b, [a[:, :200], a[:, 200:]], [w[:200], w[200:]], b)['ok_bound']
