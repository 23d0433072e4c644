"""GPU parity over long trajectories: 50 carried-state steps per algorithm
against the fp64 oracle stepped in lockstep, with the
device's own discrete decisions pinned in the oracle (VERDICT r06 "Next
round" item 2).

Every step feeds the device and the oracle the same replay slots, drawn
unfiltered (plain rng draws, no kink filter).  The oracle is stepped from
the device's own carried state (online, target, mu, nu, and for PER the sum
tree, for MGSC the logits and the Adam moments): a free-running fp64
trajectory is not a usable reference here, because a ReLU pre-activation
within f32 rounding of 0 can take the other branch than in fp64, and when
that unit's parameters carry a near-zero centered-RMSProp denominator the
two updates differ by O(lr) at once.  Stepping from the device's state
checks every one of the 50 updates, with realistic carried moments (nu -
mu^2 small under the sqrt) and a target sync in the middle
(dqn/agent.py:155-156).

The same discontinuity would make a single step incomparable too: on an
unfiltered batch one ReLU unit of the online(s_tm1) pass can fall on the
other side of 0 on the device than in fp64, or (double-Q, PER) a near-tie
of the online argmax at s_t can select the other action, and then the
step's gradient differs in a whole unit's contribution.  So after the
device step the test reads the device's four post-ReLU activations of copy
0 and, for double-Q / PER, its online q(s_t) (Learner.fetch_activations),
forms masks = y > 0 and select = argmax (first maximum, as head.hpp) and
steps the oracle with them (learner_ref.learner_step masks= / select=;
tests/test_mask_pinned_cpu.py checks the pinning and that an independent
f32 implementation then meets these bars on every step).  What is left is
rounding, and every step is held to one level:

  q, td: atol 1e-4; loss rtol 1e-4;
  update p_new - p_old per leaf, relative Frobenius norm <= 1e-4;
  mu, nu per leaf <= 1e-5.

One exception, not a kink: PER's optimizer (prioritized/run_atari.py) has a
quarter of the learning rate, so the float32 rounding of the stored
parameter (half an ulp of p per element) is four times as large beside its
update, and on the one-element shared-bias leaf nothing averages it (on a
step where that leaf's update is 8e-7 beside a parameter of 0.039, half an
ulp of the parameter is 2e-3 of the update).  No float32 implementation can
meet 1e-4 there, so on the PER trajectory each leaf's bar on each step is
the larger of 1e-4 and twice what float32 storage alone costs from that
same state: float32 RMSProp of the oracle's own fp64 gradient, correctly
rounded, from the device's carried p, mu, nu (helpers.f32_update_floor),
measured like the device's update.  The 2x is the margin an independent
f32 implementation has under 1e-4 on the double-Q trajectory
(tests/test_mask_pinned_cpu.py).  That bar comes from the oracle and the
state alone; a leaf whose floor is below 5e-5 keeps 1e-4; every such step
prints both figures and how many stored elements differ from that
replay's.  The median step stays within 1e-4, mu and nu keep 1e-5, and the
other four trajectories have no exception.

Each trajectory prints how many decisions differed from the unpinned oracle
and on which steps, and for those steps the unpinned error beside the pinned
one.

PER also checks the sum tree after every priority write-back
(prioritized/agent.py:187-206), MGSC the logits and the Adam moments after
every meta-update (dqn_mgsc_batched/agent.py:253-275, 302-357).
Reference paths: dqn/agent.py:109-119,133-158,179-189.
"""

import numpy as np
import pytest
import torch

from oracle import learner_ref
from oracle import replay_ref
from tests import helpers

pytestmark = pytest.mark.gpu

STEPS = 50
SYNC_AT = 25  # target <- online after this step's learn
STEP_UPDATE_BAR, STEP_MOMENT_BAR = helpers.STEP_UPDATE_BAR, helpers.STEP_MOMENT_BAR

_rel_err = helpers.tree_rel_err
_delta = helpers.tree_delta


def _setup(algo, seed, capacity=256, num_frames=640, a=6, optimizer=None):
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import networks
  from dqn_mgsc_zoo_amd import store as store_lib
  net = (networks.dqn_atari_network(a) if algo in ('dqn', 'mgsc') else
         networks.double_dqn_atari_network(a))
  online = net.init(seed)
  target = helpers.perturbed_tree(online, seed + 1)
  lrn = learner_lib.Learner(net, 32, algo='dqn' if algo == 'mgsc' else algo,
                            optimizer=optimizer)
  lrn.set_params(online, target)
  frames, fidx, action, reward, discount = helpers.random_store_contents(
      capacity, num_frames, a, seed + 2)
  st = store_lib.FrameStore(capacity, num_frames)
  for name, arr in (('frames', frames), ('fidx', fidx), ('action', action),
                    ('reward', reward), ('discount', discount)):
    getattr(st, name).copy_(torch.from_numpy(arr))
  host = dict(frames=frames, fidx=fidx, action=action, reward=reward,
              discount=discount)
  return lrn, st, host


def _batch(host, slots):
  return (helpers.stacks_from(host['frames'], host['fidx'], slots, 0),
          host['action'][slots], host['reward'][slots], host['discount'][slots],
          helpers.stacks_from(host['frames'], host['fidx'], slots, 1))


def _state(lrn):
  torch.cuda.synchronize()
  return tuple(lrn.params_tree(w) for w in ('online', 'target', 'mu', 'nu'))


class _Worst:
  """Every step's error of each kind, and the steps on which a decision of
  the device differed from the unpinned oracle's; printed and checked at the
  end, so a failing run still logs all of its steps.

  f32_floor (the PER trajectory): a leaf's update bar on a step is the larger
  of STEP_UPDATE_BAR and twice helpers.f32_update_floor of that leaf on that
  step, which comes from the oracle and the carried state alone."""

  def __init__(self, f32_floor=False):
    self.v = {}
    self.leaf = {}  # leaf -> every step's (update error, bar)
    self.flips = []  # (step, ReLU units, actions)
    self.f32_floor = f32_floor

  def add(self, k, x):
    self.v.setdefault(k, []).append(float(x))

  def add_update(self, by_leaf, floor=None):
    for k, x in by_leaf.items():
      bar = STEP_UPDATE_BAR if floor is None else max(STEP_UPDATE_BAR, 2 * floor[k])
      self.leaf.setdefault(k, []).append((x, bar))
    self.add('update', max(by_leaf.values()))

  def report(self, label):
    print('%s over %d steps (median / worst): %s' % (
        label, STEPS, ', '.join('%s %.2e / %.2e' % (k, np.median(v), max(v))
                                for k, v in sorted(self.v.items()))))
    print('%s: %d ReLU unit(s) and %d selected action(s) differed from the unpinned '
          'oracle, on steps %s' % (label, sum(f[1] for f in self.flips),
                                   sum(f[2] for f in self.flips), [f[0] for f in self.flips]))
    for k, v in self.leaf.items():
      over = [(i, x, bar) for i, (x, bar) in enumerate(v) if not x <= bar]
      assert not over, '%s: update of %s above its bar on (step, error, bar) %s' % (label, k, over)
    assert np.median(self.v['update']) <= STEP_UPDATE_BAR, (label, np.median(self.v['update']))
    for k in ('mu', 'nu'):
      over = [(i, x) for i, x in enumerate(self.v[k]) if not x <= STEP_MOMENT_BAR]
      assert not over, '%s: %s above %.0e on (step, error) %s' % (label, k, STEP_MOMENT_BAR, over)


def _learn_and_check(lrn, st, host, slots, device, worst, algo='dqn', weights=None,
                     write_back=None, lr=2.5e-4, eps=0.01 / 32**2):
  """One device step from its carried state against one oracle step from the
  same state with the device's ReLU masks and action selection; returns the
  oracle's result."""
  p, t, mu, nu = _state(lrn)
  batch = _batch(host, slots)
  slots_d = torch.from_numpy(slots).to(device)
  w_d = None if weights is None else torch.from_numpy(weights).to(device)
  if write_back is not None:
    lrn.step(st, slots_d, w_d, write_back=write_back(slots_d))
  else:
    lrn.step(st, slots_d, w_d)
  q, td, loss = [x.cpu().numpy() for x in lrn.fetch_outputs()]
  act = lrn.fetch_activations(0)
  masks = [act[k].cpu().numpy() > 0 for k in ('y1', 'y2', 'y3', 'h1')]
  select = None
  if algo != 'dqn':  # first maximum, as head.hpp's selection loop
    select = np.argmax(lrn.fetch_activations(2)['q'].cpu().numpy(), axis=1)
  kw = dict(algo=algo, weights=weights, lr=lr, eps=eps)
  ref = learner_ref.learner_step(p, t, mu, nu, *batch, masks=masks, select=select, **kw)
  np.testing.assert_allclose(q, ref['q_tm1'], atol=1e-4)
  np.testing.assert_allclose(td, ref['td'], atol=1e-4)
  np.testing.assert_allclose(loss[0], ref['loss'], rtol=1e-4, atol=1e-7)
  worst.add('td', np.abs(td - ref['td']).max())
  p1, t1, mu1, nu1 = _state(lrn)

  def errs(r):
    by_leaf = helpers.tree_rel_errs(_delta(p1, p), _delta(r['params'], p))
    return by_leaf, (max(by_leaf.values()), _rel_err(mu1, r['mu']), _rel_err(nu1, r['nu']))

  by_leaf, (ue, me, ne) = errs(ref)
  step = len(worst.v.get('update', ()))
  floor = None
  if worst.f32_floor:
    floor, p_f32 = helpers.f32_update_floor(p, mu, nu, ref, lr, 0.95, eps)
    for k in by_leaf:
      if max(by_leaf[k], floor[k]) > STEP_UPDATE_BAR:
        m, n = k.rsplit('/', 1)
        print('  step %d %s: update error %.2e on the device, %.2e for float32 RMSProp of the '
              "oracle's gradient from the same state (%d of %d stored elements differ)" % (
                  step, k, by_leaf[k], floor[k],
                  np.count_nonzero(p1[m][n] != p_f32[m][n]), p1[m][n].size))
  worst.add_update(by_leaf, floor)
  worst.add('mu', me)
  worst.add('nu', ne)
  # the unpinned oracle's decisions: its own masks of the online(s_tm1) pass
  # (the selector pass at s_t is not pinned, so ref's is the unpinned one)
  _, cache = learner_ref.forward(p, batch[0], algo != 'dqn')
  units, actions = helpers.decision_flips(
      masks, select, dict(masks=cache['masks'], q_selector_t=ref['q_selector_t']))
  if units or actions:
    worst.flips.append((step, units, actions))
    free = errs(learner_ref.learner_step(p, t, mu, nu, *batch, **kw))[1]
    print('  step %d: %d ReLU unit(s), %d action(s) differ from the unpinned oracle; update / '
          'mu / nu unpinned %.2e / %.2e / %.2e, pinned %.2e / %.2e / %.2e' % (
              (step, units, actions) + free + (ue, me, ne)))
  elif ue > STEP_UPDATE_BAR or me > STEP_MOMENT_BAR or ne > STEP_MOMENT_BAR:
    print('  step %d without a flip: update %.2e (%s) mu %.2e nu %.2e' % (
        step, ue, max(by_leaf, key=by_leaf.get), me, ne))
  for m in t:  # a learner step leaves the target alone
    for n in t[m]:
      np.testing.assert_array_equal(t1[m][n], t[m][n])
  return ref, td


def _sync(lrn, step):
  if step + 1 == SYNC_AT:
    lrn.sync_target()
    p, t, _, _ = _state(lrn)
    for m in p:
      for n in p[m]:
        np.testing.assert_array_equal(t[m][n], p[m][n])


@pytest.mark.parametrize('algo', ['dqn', 'double'])
def test_fifty_step_trajectory(device, algo):
  lrn, st, host = _setup(algo, seed=300 if algo == 'dqn' else 310)
  rng = np.random.default_rng(301)
  worst = _Worst()
  for step in range(STEPS):
    slots = rng.integers(0, st.capacity, size=32).astype(np.int32)
    _learn_and_check(lrn, st, host, slots, device, worst, algo=algo)
    _sync(lrn, step)
  worst.report(algo)
  assert lrn.sync_status() == 0


def test_fifty_step_per_trajectory_with_tree(device):
  """Config 4 over 50 steps: PrioritizedDistribution.sample on the device's
  tree (the oracle's restatement given the reference's three draws,
  replay.py:680-716), IS weights (replay.py:344-376, beta 0.4, normalised by
  the max), the double-Q IS-weighted step, and the |td|^alpha write-back +
  max_seen_priority on the device tree inside the backward launch
  (dqz_learner_step_per): after every step the written leaves are
  |td|^alpha of the device's td (the last draw of a repeated slot wins),
  the others unchanged, and every internal node is left + right exactly."""
  from dqn_mgsc_zoo_amd import _native
  from dqn_mgsc_zoo_amd import learner as learner_lib
  alpha, beta, usp = 0.6, 0.4, 1e-3
  lr, eps = 6.25e-5, 0.01 / 32**2 / 16  # prioritized/run_atari.py:85-88
  lrn, st, host = _setup('per', seed=320,
                         optimizer=learner_lib.rmsprop(lr, 0.95, eps, centered=True))
  cap = st.capacity
  rng = np.random.default_rng(321)
  leaves0 = rng.uniform(0.01, 2.0, size=cap) ** alpha
  tree = torch.zeros((2 * cap,), dtype=torch.float64, device=device)
  idx_all = torch.arange(cap, dtype=torch.int64, device=device)
  _native.check(_native.lib().dqz_sumtree_set(
      _native.ptr(tree), cap, _native.ptr(idx_all),
      _native.ptr(torch.from_numpy(leaves0).to(device)), cap, _native.stream_handle()))
  max_seen = torch.ones((1,), dtype=torch.float64, device=device)
  active = np.arange(cap)
  worst = _Worst(f32_floor=True)
  for step in range(STEPS):
    torch.cuda.synchronize()
    before = tree.cpu().numpy()
    ms_before = float(max_seen.item())
    idx, probs = replay_ref.per_sample(before[cap:], active, rng.integers(0, cap, 32),
                                       rng.random(32), rng.random(32), usp)
    w = (1.0 / cap / probs) ** beta
    w = (w / w.max()).astype(np.float32)
    slots = idx.astype(np.int32)
    _, td = _learn_and_check(lrn, st, host, slots, device, worst, algo='per', weights=w,
                             write_back=lambda sd: (tree, cap, sd, alpha, max_seen),
                             lr=lr, eps=eps)
    torch.cuda.synchronize()
    got = tree.cpu().numpy()
    want = before[cap:].copy()
    pri = np.abs(td.astype(np.float64))
    want[slots] = np.where(pri == 0.0, 0.0, pri ** alpha)  # numpy order: last draw wins
    np.testing.assert_allclose(got[cap:], want, rtol=1e-12, atol=0)
    for i in range(1, cap):
      assert got[i] == got[2 * i] + got[2 * i + 1], (step, i)
    assert float(max_seen.item()) == max(ms_before, float(pri.max()))
    _sync(lrn, step)
  worst.report('per')
  assert lrn.sync_status() == 0


@pytest.mark.parametrize('second_order', [False, True])
def test_fifty_step_mgsc_trajectory(device, second_order):
  """Config 3's learn frame 50 times in the reference's order
  (dqn_mgsc_batched/agent.py:253-275): the meta-update on a uniform meta
  batch without replacement (M = 8, a fresh online transition each step,
  logits written back at the meta positions), then a learner batch drawn by
  softmax over the device's logits, then the DQN step.  After every
  meta-update the written logits, the Adam moments and count match the
  oracle's meta_update from the same state, the other logits are untouched
  and the buffer's running log-sum-exp equals a fresh scan.
  second_order: the reservoir agent's meta-gradient (no stop_gradient)."""
  from dqn_mgsc_zoo_amd import learner as learner_lib
  from dqn_mgsc_zoo_amd import replay as replay_lib
  from dqn_mgsc_zoo_amd import replay_circular as rc
  m = 8
  lrn, st, host = _setup('mgsc', seed=330 + int(second_order))
  cap = st.capacity
  meta = learner_lib.MetaLearner(lrn, m, learner_lib.adam(2.5e-4),
                                 second_order=second_order)
  rng = np.random.default_rng(331)
  dev = rc._DeviceLogits(cap, device, max_queries=32)  # pylint: disable=protected-access
  dev.load(rng.standard_normal(cap).astype(np.float32))
  dev.sample_abs(rng.random(32))  # re-seed: the running state is known
  worst = _Worst()
  label = 'mgsc %s order' % ('second' if second_order else 'first')
  for step in range(STEPS):
    pos = rng.choice(cap, m, replace=False).astype(np.int32)  # reservoir: slot = position
    ot_tm1 = rng.integers(0, 256, (84, 84, 4), dtype=np.uint8)
    ot_t = rng.integers(0, 256, (84, 84, 4), dtype=np.uint8)
    oa, orr = int(rng.integers(0, 6)), float(rng.choice([-1.0, 0.0, 1.0]))
    p, t, mu, nu = _state(lrn)
    logits = dev.logits.cpu().numpy()
    ad = meta.get_state()[0]
    s_tm1, a_tm1, r_t, d_t, s_t = _batch(host, pos)
    mref = learner_ref.meta_update(
        p, t, mu, nu, dict(s_tm1=s_tm1, a_tm1=a_tm1, r_t=r_t, discount_t=d_t, s_t=s_t),
        logits[pos], dict(s_tm1=ot_tm1, a_tm1=oa, r_t=orr, discount_t=0.99, s_t=ot_t),
        np.asarray(ad.mu, np.float64), np.asarray(ad.nu, np.float64), int(ad.count),
        stop_gradient=not second_order)
    meta.set_online_transition(replay_lib.Transition(ot_tm1, oa, orr, 0.99, ot_t))
    pos_d = torch.from_numpy(pos).to(device)
    meta.update(st, pos_d, dev.logits, pos_d, logit_buffer=dev)
    after = dev.logits.cpu().numpy()
    np.testing.assert_allclose(after[pos], mref['new_logits'], atol=1e-6)
    keep = np.ones(cap, bool)
    keep[pos] = False
    np.testing.assert_array_equal(after[keep], logits[keep])
    worst.add('logit', np.abs(after[pos] - mref['new_logits']).max())
    ad1 = meta.get_state()[0]
    assert int(ad1.count) == mref['adam_count']
    sm = np.abs(mref['adam_m']).max()
    # (m carries every step's dlogits, each within 2e-5 of its max: test_meta_gpu)
    np.testing.assert_allclose(ad1.mu, mref['adam_m'], atol=1e-4 * sm)
    worst.add('adam_m', np.abs(np.asarray(ad1.mu) - mref['adam_m']).max() / sm)
    run = dev.run_state()
    a64 = after.astype(np.float64)
    want = a64.max() + np.log(np.exp(a64 - a64.max()).sum())
    assert abs(run['c'] + np.log(run['S']) - want) < 1e-9 * max(1.0, abs(want))
    slots = replay_ref.softmax_choice(after, rng.random(32)).astype(np.int32)
    _learn_and_check(lrn, st, host, slots, device, worst)
    _sync(lrn, step)
  worst.report(label)
  assert lrn.sync_status() == 0 and meta.sync_status() == 0
