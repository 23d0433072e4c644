"""GPU: every stage of the MGSC meta-update against the plain operation
applied to that stage's own device input (the meta-update's counterpart of
tests/test_layers_gpu.py).

The other tests see the meta-update through probs, the loss, dlogits (2e-5 of
max |dlogits|) and the Adam-updated logits; a failure there does not say
which of csrc/meta.hpp, csrc/hvp.hpp or the Rms::meta1/2/3 epilogues did it.
Here one meta.update runs per shape, every stage buffer is read back
(MetaLearner.fetch_stages, MetaLearner.debug_learners) and each stage is
restated in fp64 from the buffers it read (tests/meta_stage_checks.py, whose
docstring derives every bar; tests/test_meta_stage_checks_cpu.py ties the
restatements to the oracle and runs the bars on numpy float32).  ReLU masks
are the device's own activations, so no decision can differ.

Second order, (bound, M, A), seeds and online action of
test_meta_gpu.test_second_order_meta_update_matches_oracle:
  (5.0, 8, 6)    |td'| < bound: alpha = 1, the s1 grad q term is live
  (1/32, 8, 6)   |td'| > bound: alpha = 0, clip(td') = +-bound
  (5.0, 8, 18)   b3's gather branch (A > 16), two put batches in hvp_g_hidden
  (5.0, 260, 6)  two chunks of 256: meta_rms1_kernel, accumulated G,
                 tangent_fwd_kernel + meta_dot_kernel (zv1 .. zvp and s of the
                 last chunk's four real samples; p = s = 0 on the padding)
Checked per shape, every stage from the device's own inputs: G per leaf (one
chunk); theta', J from G; v_dir, w, s1 from G, grad q, td'; ty1 from the
pixels and w, ty2, ty3, the sum of hpart, ddot4 (bit-equal), ddot3 .. ddot1;
every leaf of v against the bound of its HVP term |J clip(td')| b(H_q w) plus
the combine's roundings (not against |v|); s and dlogits.  theta' surviving a
second-order update is the `theta'` rows (thp is no longer overwritten by v).

First order, M = 8 (kink-free slots) and M = 260: theta', mu', nu', J from G
(M = 8: the batch learner's arrays; M = 260: G recovered from mu', the first
order keeps no G and the batch learner only its last chunk), and at M = 8
every leaf of v (in the G buffer) against learner_ref.meta_update's v at the
every-step gradient bar of tests/test_trajectory_gpu.py (relative Frobenius
norm 1e-5), or 4 x the numpy float32 restatement's own error where that
restatement misses 1e-5 itself.  v at M = 260 has no check of its own here
(the oracle's 260 per-example backwards are not a few seconds; its stages are
those of M = 8 after meta_rms1_kernel, which the M = 260 rows cover).
"""

import types

import numpy as np
import pytest
import torch

from oracle import learner_ref
from tests import helpers
from tests import meta_stage_checks as ms

pytestmark = pytest.mark.gpu

SECOND = [(5.0, 8, 6), (1.0 / 32, 8, 6), (5.0, 8, 18), (5.0, 260, 6)]
FIRST = [8, 260]
STEP_GRAD_BAR = 1e-5  # tests/test_trajectory_gpu.py: every step's gradient, relative Frobenius norm per leaf


def _np(d, rows=None):
  return {k: (v if rows is None else v[rows]).cpu().numpy() for k, v in d.items()}


def _run(case, device, second_order):
  """One meta.update on `case`; returns (meta, the update's inputs for a
  repeat, what it left behind as meta_stage_checks' device-like dict)."""
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import replay as replay_lib
  from dqn_mgsc_zoo_amd import store as store_lib
  net, m = case['net'], len(case['slots'])
  lrn = learner_lib.Learner(net, 32, algo='dqn', grad_error_bound=case['bound'])
  lrn.set_params(case['online'], case['target'])
  lrn.set_opt_state(case['mu'], case['nu'])
  meta = learner_lib.MetaLearner(lrn, m, learner_lib.adam(2.5e-4), second_order=second_order)
  st = store_lib.FrameStore(case['capacity'], case['store']['frames'].shape[0])
  for name, arr in case['store'].items():
    getattr(st, name).copy_(torch.from_numpy(arr))
  meta.set_online_transition(replay_lib.Transition(case['ot_tm1'], case['oa'], case['o_r'], case['o_d'],
                                                   case['ot_t']))
  args = (st, torch.from_numpy(case['slots']).to(device), torch.from_numpy(case['all_logits']).to(device),
          torch.from_numpy(case['pos']).to(device))
  meta.update(*args)
  return meta, args, _fetch(case, meta)


def _fetch(case, meta):
  net, m = case['net'], len(case['slots'])
  probs, dlogits, td, loss = [t.cpu().numpy().copy() for t in meta.fetch_outputs()]
  stg = meta.fetch_stages()
  lm, l1 = meta.debug_learners()
  c = min(m, 256)
  real = slice(0, m - (m - 1) // c * c)  # the last chunk's real samples (all of them with one chunk)
  d = {k: ms.tree_of(net, v.cpu().numpy()) for k, v in stg.items() if k in ('G', 'thp', 'mu1', 'nu1', 'J', 'GQ', 'HQ')}
  d.update({k: v.cpu().numpy() for k, v in stg.items()
            if k in ('ty1', 'ty2', 'ty3', 'hpart', 'td4', 'td3', 'td2', 'td1', 'p', 's')})
  d.update({k: stg[k][real].cpu().numpy() for k in ('zv1', 'zv2', 'zv3') if k in stg})
  if 'zvp' in stg:
    d['zvp'] = stg['zvp'][:, real].cpu().numpy()
  if 's1' in stg:
    d['s1'] = float(stg['s1'].cpu().numpy()[0])
  d['act'] = _np(lm.fetch_activations(0, backward=True), real)
  d['q1'] = lm.fetch_activations(1)['q'][real].cpu().numpy()
  d['act1'] = _np(l1.fetch_activations(0, backward=True))
  d['tdp'] = float(l1.fetch_outputs()[1].cpu().numpy()[0])
  d.update(dlogits=dlogits, probs=probs, td=td, loss=loss)
  assert meta.sync_status() == 0
  return d


_RUNS = {}


def _cached(key, device):
  """One update per shape for the whole module (key: a SECOND entry, or
  ('first', M))."""
  if key not in _RUNS:
    if key[0] == 'first':
      case = ms.meta_case(1.0 / 32, key[1], 6, kink_free=key[1] == 8)
      meta, args, d = _run(case, device, False)
    else:
      case = ms.meta_case(*key)
      meta, args, d = _run(case, device, True)
    _RUNS[key] = types.SimpleNamespace(case=case, d=d, m=key[1], meta=meta, args=args)
  return _RUNS[key]


@pytest.fixture(scope='module', params=SECOND, ids=lambda c: 'bound%g-M%d-A%d' % c)
def second(request, device):
  return _cached(request.param, device)


def test_second_order_stages(second):
  case, d = second.case, second.d
  one = second.m <= 256
  rows = ms.second_order_rows(case, d, batch_side=one)
  if not one:
    first = (second.m - 1) // 256 * 256
    rows += ms.chunk_rows(case, dict(d, v=d['HQ']), first, second.m - first)
  ms.lc.report(rows)


def test_theta_prime_survives_a_second_order_update(second):
  """thp is theta' within the restated meta1's bar on every leaf, and v is
  elsewhere (HQ): the HVP's third launch no longer stores v over the conv2
  weights its b1 blocks read."""
  d = second.d
  ms.lc.report(ms.theta_rows(second.case, d))
  for mod, name in ms.LEAVES:
    step = np.abs(d['thp'][mod][name].astype(np.float64) - second.case['online'][mod][name]).max()
    assert 0 < step < 1e-2, (mod, name, step)  # theta' = theta + an RMSProp step of lr / sqrt(eps) = 0.08 |G| at most
    assert not np.array_equal(d['thp'][mod][name], d['HQ'][mod][name]), (mod, name)


def test_ddot4_is_the_masked_column_bit_for_bit(second):
  assert ms.td4_exact(second.case, second.d) == (0, 0)  # (bits that differ, values that differ)


def test_td_error_is_on_the_intended_side_of_the_clip_bound(second):
  """alpha = 1 (both terms of the online transition's Hessian live) for the
  bound-5 shapes, alpha = 0 for bound 1/32, read off the device's td'."""
  td, bound = abs(second.d['tdp']), second.case['bound']
  print("|td'| = %.6f, bound %.6f" % (td, bound))
  assert td < bound if bound > 1 else td > bound


def test_probabilities_and_padding(second):
  d, m = second.d, second.m
  np.testing.assert_array_equal(d['p'][:m], d['probs'])
  np.testing.assert_array_equal(d['p'][m:], 0.0)
  np.testing.assert_array_equal(d['s'][m:], 0.0)
  assert d['p'].size == -(-m // 256) * min(m, 256)


def test_fetching_leaves_the_next_update_bit_identical(device):
  """The second update follows a fetch of every stage buffer, the first
  followed none: same state, same bits."""
  second = _cached(SECOND[0], device)
  meta, (st, slots, _, pos) = second.meta, second.args
  meta.set_state({'count': 0, 'mu': np.zeros(second.m, np.float32), 'nu': np.zeros(second.m, np.float32)})
  logits = torch.from_numpy(second.case['all_logits']).to(device)
  meta.update(st, slots, logits, pos)
  again = _fetch(second.case, meta)
  for k in ('probs', 'dlogits', 'td', 'loss', 's', 'td1', 'hpart'):
    assert np.array_equal(again[k].view(np.uint32), second.d[k].view(np.uint32)), k
  for k in ('HQ', 'thp', 'G'):
    for mod, name in ms.LEAVES:
      assert np.array_equal(again[k][mod][name].view(np.uint32), second.d[k][mod][name].view(np.uint32)), (k, mod, name)
  np.testing.assert_array_equal(logits.cpu().numpy(), second.args[2].cpu().numpy())


def test_buffers_the_configuration_lacks_are_refused(device):
  import ctypes
  from dqn_mgsc_zoo_amd import _native
  from dqn_mgsc_zoo_amd import learner as learner_lib
  second = _cached(SECOND[0], device)
  buf = torch.zeros(16, dtype=torch.float32, device=device)
  lib = _native.lib()
  req = _native.DqzMetaStages(zv1=buf.data_ptr())  # one chunk: never written
  with pytest.raises(_native.NativeLibraryError, match='more than one chunk'):
    _native.check(lib.dqz_meta_debug_stages(second.meta._h, ctypes.byref(req), None))  # pylint: disable=protected-access
  first = learner_lib.MetaLearner(second.meta.learner, 8, learner_lib.adam(2.5e-4))
  req = _native.DqzMetaStages(HQ=buf.data_ptr())
  with pytest.raises(_native.NativeLibraryError, match='second-order'):
    _native.check(lib.dqz_meta_debug_stages(first._h, ctypes.byref(req), None))  # pylint: disable=protected-access
  out = ctypes.c_void_p()
  with pytest.raises(_native.NativeLibraryError, match='which must be'):
    _native.check(lib.dqz_meta_debug_learner(first._h, 2, ctypes.byref(out)))  # pylint: disable=protected-access


@pytest.fixture(scope='module', params=FIRST, ids=lambda m: 'M%d' % m)
def first(request, device):
  return _cached(('first', request.param), device)


def test_first_order_stages(first):
  case, d = first.case, first.d
  if first.m <= 256:
    rows = ms.first_order_rows(case, d, ms.g_from_batch(case, d))
  else:
    rows = ms.first_order_rows(case, d, ms.g_from_moment(case, d), with_mu=False)
  ms.lc.report(rows)


def test_first_order_v_matches_the_oracle(device):
  """v = dL/dG (left in the G buffer) per leaf against the fp64 oracle on
  kink-free slots, bar 1e-5 relative Frobenius norm (the project's
  every-step gradient bar), or 4 x the error of the numpy float32
  restatement of the same stages where that alone misses 1e-5."""
  first = _cached(('first', 8), device)
  case, d = first.case, first.d
  f64 = lambda t: ms.tmap(lambda v: np.asarray(v, np.float64), t)
  mb = dict(s_tm1=case['s_tm1'], a_tm1=case['action'], r_t=case['reward'], discount_t=case['discount'],
            s_t=case['s_t'])
  ot = dict(s_tm1=case['ot_tm1'], a_tm1=case['oa'], r_t=case['o_r'], discount_t=case['o_d'], s_t=case['ot_t'])
  ref = learner_ref.meta_update(f64(case['online']), f64(case['target']), f64(case['mu']), f64(case['nu']), mb,
                                case['logits'], ot, np.zeros(8), np.zeros(8), 0, grad_error_bound=case['bound'])
  assert learner_ref.relu_margin(ref['theta_p'], case['ot_tm1'][None]) >= 1e-6  # the one transition too
  sim = ms.simulate(case, np.float32, second_order=False)
  got, floor = helpers.tree_rel_errs(d['G'], ref['v']), helpers.tree_rel_errs(sim['G'], ref['v'])
  bad = []
  for leaf in sorted(got):
    bar = STEP_GRAD_BAR if floor[leaf] <= STEP_GRAD_BAR else 4 * floor[leaf]
    print('v %-45s device %.3e   numpy float32 %.3e   bar %.3e' % (leaf, got[leaf], floor[leaf], bar))
    if got[leaf] > bar:
      bad.append((leaf, got[leaf], bar))
  assert not bad, bad
