"""CPU: the stage restatements of tests/meta_stage_checks.py and their bars,
without a device.

(a) chained in fp64 (exact optimizer constants), the restatements reproduce
    oracle.learner_ref.hvp and the v and dp of learner_ref.meta_update(
    stop_gradient=False) to 1e-12 relative, so the references the GPU test
    holds each kernel to are tied to the oracle tests/test_oracle.py ties to
    torch autograd;
(b) the same stages in numpy float32, each from the stored float32 values of
    the stages before (exactly what the GPU test does with the device's
    buffers, at its seeds and shapes), pass every bar: the bars hold for a
    plain float32 implementation;
(c) damaged stages fail the bar of their own stage: a dropped `ydot (x) d`
    term (conv2's parameter block), conv2's mask omitted in ddot2, alpha
    taken as 1 outside the clip bound, and the read/write overlap the HVP's
    third launch had (ddot1 formed with four rows of theta''s W2 replaced by
    the same rows of v).  Each is seen by the row of its own stage and by no
    row before it.  The simulated overlap (rows 200 .. 203 of W2 as [512, 64],
    bound 5, M = 8, A = 6) moves dlogits by 1.5e-2 of max |dlogits| (printed
    by test_simulated_overlap_fails_ddot1, not asserted) and by 4.6e-4 at
    bound 1/32, where clip(td') = 1/32 scales the HVP term down.  Both are
    above the end-to-end bar of 2e-5 (750 and 23 times): at these shapes the
    old tolerance would have shown a loss of four whole rows, though not
    which kernel caused it.  What it lets through is a loss some 750 (23)
    times smaller than four rows, or any wrong stage whose effect on dlogits
    is below 2e-5 of its maximum.

test_first_order_float32_restatements_pass_every_bar and
test_chunk_rows_on_a_float32_tangent_forward run the first-order rows and the
chunked tangent forward's rows the same way;
test_read_back_entries_refuse_null_arguments covers the argument checks of
dqz_meta_debug_learner / dqz_meta_debug_stages that need no device.
"""

import numpy as np
import pytest

from oracle import learner_ref
from tests import meta_stage_checks as ms

CASES = [(5.0, 8, 6), (1.0 / 32, 8, 6), (5.0, 8, 18)]


@pytest.fixture(scope='module', params=CASES, ids=lambda c: 'bound%g-M%d-A%d' % c)
def case(request):
  return ms.meta_case(*request.param)


@pytest.fixture(scope='module')
def f32_run(case):
  return ms.simulate(case, np.float32)


def _failed(rows):
  return sorted(n for n, r in rows if not (r['ok_bound'] and r['ok_rms']))


def _rel(got, want):
  got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
  return float(np.abs(got.reshape(want.shape) - want).max() / max(np.abs(want).max(), 1e-300))


def test_fp64_chain_reproduces_the_oracle():
  case = ms.meta_case(5.0, 8, 6)
  exact = ms.Consts.__new__(ms.Consts)
  exact.lr, exact.decay, exact.eps = 2.5e-4, 0.95, 0.01 / 32**2
  exact.c1 = 1.0 - exact.decay
  d = ms.simulate(case, np.float64, exact)
  f64 = lambda t: ms.tmap(lambda v: np.asarray(v, np.float64), t)
  mb = dict(s_tm1=case['s_tm1'], a_tm1=case['action'], r_t=case['reward'], discount_t=case['discount'],
            s_t=case['s_t'])
  ot = dict(s_tm1=case['ot_tm1'], a_tm1=case['oa'], r_t=case['o_r'], discount_t=case['o_d'], s_t=case['ot_t'])
  ref = learner_ref.meta_update(f64(case['online']), f64(case['target']), f64(case['mu']), f64(case['nu']), mb,
                                case['logits'], ot, np.zeros(8), np.zeros(8), 0, grad_error_bound=case['bound'],
                                stop_gradient=False)
  assert abs(d['tdp']) < case['bound']
  # H_q w against the oracle's own hvp, at the chain's theta' and w
  q1, cache1 = learner_ref.forward(d['thp'], case['ot_tm1'][None])
  e_a = np.zeros_like(q1)
  e_a[0, case['oa']] = 1.0
  want = learner_ref.hvp(d['thp'], cache1, e_a, d['nu1'])
  for mod, name in ms.LEAVES:
    assert _rel(d['hq'][mod][name], want[mod][name]) < 1e-12, (mod, name)
    assert _rel(d['G'][mod][name], ref['G'][mod][name]) < 1e-12, (mod, name)
    assert _rel(d['thp'][mod][name], ref['theta_p'][mod][name]) < 1e-12, (mod, name)
    assert _rel(d['HQ'][mod][name], ref['v'][mod][name]) < 1e-12, (mod, name)
  assert _rel(d['s'], ref['probs'] * ref['dp']) < 1e-12
  assert _rel(d['dlogits'], ref['dlogits']) < 1e-12


def test_float32_restatements_pass_every_bar(case, f32_run):
  rows = ms.second_order_rows(case, f32_run)
  ms.lc.report(rows)
  assert ms.td4_exact(case, f32_run) == (0, 0)
  names = [n for n, _ in rows]
  assert len(names) == len(set(names)) and len(names) >= 70


@pytest.mark.parametrize('damage,stage', [
    (('drop', 'hq conv2 w'), 'v conv2 w'),
    (('no_mask', 'td2'), 'td2'),
])
def test_damaged_stage_fails_its_own_bar(damage, stage):
  case = ms.meta_case(5.0, 8, 6)
  rows = ms.second_order_rows(case, ms.simulate(case, np.float32, damage=damage), batch_side=False)
  assert stage in _failed(rows), _failed(rows)
  # and the stages before it still pass: the row names the stage
  before = [n for n, _ in rows][:[n for n, _ in rows].index(stage)]
  assert not set(before) & set(_failed(rows)), _failed(rows)


def test_alpha_kept_outside_the_clip_bound_fails_v():
  case = ms.meta_case(1.0 / 32, 8, 6)
  d = ms.simulate(case, np.float32, damage='alpha_one')
  assert abs(d['tdp']) > case['bound']
  bad = _failed(ms.second_order_rows(case, d, batch_side=False))
  assert bad and all(n.startswith('v ') for n in bad), bad


def test_simulated_overlap_fails_ddot1():
  """What the old `vout == th` let through when a b1 block loses the race:
  four rows of W2 (~1e-2) read as rows of v (~1e-6)."""
  case = ms.meta_case(5.0, 8, 6)
  good = ms.simulate(case, np.float32)
  d = ms.simulate(case, np.float32, damage='overlap')
  bad = _failed(ms.second_order_rows(case, d, batch_side=False))
  assert bad == ['td1'], bad
  moved = np.abs(d['dlogits'] - good['dlogits']).max() / np.abs(good['dlogits']).max()
  print('simulated overlap: dlogits moves by %.3g of max |dlogits| (the end-to-end bar: 2e-5)' % moved)


def test_first_order_float32_restatements_pass_every_bar():
  """theta', mu', nu', J from G (the batch learner's arrays) and, as a
  chunked meta batch has to, from G recovered from mu'."""
  case = ms.meta_case(1.0 / 32, 8, 6, kink_free=True)
  d = ms.simulate(case, np.float32, second_order=False)
  rows = ms.first_order_rows(case, d, ms.g_from_batch(case, d))
  rows += [('recovered G: ' + n, r) for n, r in
           ms.first_order_rows(case, d, ms.g_from_moment(case, d), with_mu=False)]
  ms.lc.report(rows)
  assert len(rows) == 70


def test_chunk_rows_on_a_float32_tangent_forward(f32_run, case):
  """chunk_rows (the K > 1 tangent forward and s) on numpy float32: the first
  four samples of the M = 8 batch stand in for a last chunk."""
  f = np.float32
  n, act, v = 4, f32_run['act'], f32_run['HQ']
  d = dict(f32_run, v=v, act={k: a[:n] for k, a in act.items()}, q1=f32_run['q1'][:n])
  prev = (np.asarray(case['s_tm1'][:n], f) / f(255.0))
  for l in range(3):
    w = v[ms.C[l]]['w']
    z = ms.lc.conv_cols(prev, l).astype(f) @ w.reshape(-1, w.shape[-1]) + v[ms.C[l]]['b']
    d['zv%d' % (l + 1)] = z.reshape(act['y%d' % (l + 1)][:n].shape)
    prev = act['y%d' % (l + 1)][:n]
  y3 = prev.reshape(n, -1)
  d['zvp'] = np.stack([y3[:, 448 * s:448 * (s + 1)] @ v[ms.FC1]['w'][448 * s:448 * (s + 1)] for s in range(7)])
  rows = ms.chunk_rows(case, d, 0, n)
  ms.lc.report(rows)
  # s was formed from the per-sample gradients; the two forms agree to float32 sums
  assert [n for n, _ in rows] == ['zv1', 'zv2', 'zv3', 'sum zvp', 's (last chunk)']


def test_read_back_entries_refuse_null_arguments():
  """dqz_meta_debug_learner / dqz_meta_debug_stages validate before any HIP call."""
  import ctypes  # pylint: disable=g-import-not-at-top
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  lib = _native.lib()
  out = ctypes.c_void_p()
  req = _native.DqzMetaStages()
  for call in (lambda: lib.dqz_meta_debug_learner(None, 0, ctypes.byref(out)),
               lambda: lib.dqz_meta_debug_stages(None, ctypes.byref(req), None)):
    with pytest.raises(_native.NativeLibraryError, match='null argument'):
      _native.check(call())
  assert ctypes.sizeof(_native.DqzMetaStages) == 22 * ctypes.sizeof(ctypes.c_void_p)
