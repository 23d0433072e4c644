"""What the QR-DQN step costs beside the DQN and C51 steps with the same
optimizer chain.

usage (GPU box): python tools/qr_bench.py [--rounds R] [--reps N] [--capacity C] [--actions 6 18] [--double-q] [--prioritized] > out.json

For each number of actions A (6 and 18), three learners at B = 32 on one
synthetic replay, each a hipGraph of 20 learner steps (sample_uniform +
step on its slots) with chain(clip_by_global_norm(10), adam(5e-5, eps=0.01/32)):
  dqn_clip_adam_slots  Learner(algo='dqn') with that chain
  c51                  C51Learner.step, N = 51 atoms
  qrdqn                QrLearner.step, N = 201 quantiles, huber_param 1
The arms are timed in the same process, interleaved round by round (arm order
rotated), HIP events around N replays; the JSON gives each arm's median,
minimum and maximum ms per step over the rounds and QR-DQN's difference to both
other arms.  --double-q and --prioritized switch the c51 and qrdqn arms'
learners to double-Q selection (a third network copy) and to
importance-weighted steps (fixed uneven weights in (0, 1]; the priorities are
written, the sum tree is not part of the arm).

launch_us: dqz_qr_profile / dqz_c51_profile on a fixed batch, in a run of its
own after the timed rounds: each launch of the step repeated back to back
between two events (the duration a kernel trace reports), beside
dqz_learner_profile's figures of the DQN step's launches."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dqn_mgsc_zoo_amd import learner as learner_lib, networks, synthetic  # noqa: E402

B, N_ATOMS, N_QUANTILES, GRAPH_STEPS = 32, 51, 201, 20
LR, EPS, VMAX, KAPPA = 5e-5, 0.01 / 32, 10.0, 1.0
NAMES = ['dqn_clip_adam_slots', 'c51', 'qrdqn']


def optimizer():
  return learner_lib.chain(learner_lib.clip_by_global_norm(10.0), learner_lib.adam(LR, eps=EPS))


def make_arm(name, a, store, cap, dev, double_q=False, prioritized=False):
  wide = dict(optimizer=optimizer(), device=dev, double_q=double_q, prioritized=prioritized)
  weights = None
  if prioritized and name != 'dqn_clip_adam_slots':
    weights = torch.linspace(0.05, 1.0, B, dtype=torch.float32, device=dev)
  if name == 'qrdqn':
    tau = ((np.arange(N_QUANTILES, dtype=np.float32) + 0.5) / N_QUANTILES).astype(np.float32)
    net = networks.qr_atari_network(a, tau)
    lrn = learner_lib.QrLearner(net, B, huber_param=KAPPA, **wide)
  elif name == 'c51':
    net = networks.c51_atari_network(a, np.linspace(-VMAX, VMAX, N_ATOMS).astype(np.float32))
    lrn = learner_lib.C51Learner(net, B, **wide)
  else:
    net = networks.dqn_atari_network(a)
    lrn = learner_lib.Learner(net, B, algo='dqn', optimizer=optimizer(), device=dev)
  lrn.set_params(net.init(seed=1))
  slots = torch.zeros((B,), dtype=torch.int32, device=dev)
  ctr = torch.zeros((1,), dtype=torch.int64, device=dev)

  def fn():
    learner_lib.sample_uniform(0, cap, cap, B, 7, ctr, slots)
    lrn.step(store, slots, weights)
  for _ in range(20):
    fn()
  torch.cuda.synchronize(dev)
  side = torch.cuda.Stream(dev)
  side.wait_stream(torch.cuda.current_stream(dev))
  with torch.cuda.stream(side):
    fn()
  torch.cuda.current_stream(dev).wait_stream(side)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(GRAPH_STEPS):
      fn()
  return lrn, g, slots, weights


def time_graph(g, reps, dev):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize(dev)
  e0.record()
  for _ in range(reps):
    g.replay()
  e1.record()
  torch.cuda.synchronize(dev)
  return e0.elapsed_time(e1) / (reps * GRAPH_STEPS)


def run(a, args, dev):
  cap = args.capacity
  store = synthetic.fill_episodic(cap, a, seed=0, device=dev)
  arms = {n: make_arm(n, a, store, cap, dev, args.double_q, args.prioritized) for n in NAMES}
  ms = {n: [] for n in NAMES}
  for r in range(args.rounds):
    for n in NAMES[r % 3:] + NAMES[:r % 3]:
      ms[n].append(time_graph(arms[n][1], args.reps, dev))
  out = {'num_actions': a, 'ms_per_step': {}}
  for n in NAMES:
    out['ms_per_step'][n] = {'median': round(statistics.median(ms[n]), 5), 'min': round(min(ms[n]), 5),
                             'max': round(max(ms[n]), 5)}
  qr = out['ms_per_step']['qrdqn']['median']
  out['qrdqn_extra_us_per_step'] = {
      n: round(1e3 * (qr - out['ms_per_step'][n]['median']), 2) for n in NAMES[:2]}
  for n in NAMES:
    assert arms[n][0].sync_status() == 0 and bool(torch.isfinite(arms[n][0].online).all()), n
  # the launches' own durations, after the timed rounds (the profile synchronises between phases)
  out['launch_us'] = {}
  for n in ('qrdqn', 'c51'):
    lrn, _, slots, weights = arms[n]
    out['launch_us'][n] = {k: round(1e3 * v, 2) for k, v in lrn.profile(store, slots, weights, iters=50).items()}
  net = networks.dqn_atari_network(a)
  dqn = learner_lib.Learner(net, B, algo='dqn', device=dev)  # the profile runs the fused-RMSProp step
  dqn.set_params(net.init(seed=1))
  out['launch_us']['dqn'] = {k: round(1e3 * v, 2) for k, v in dqn.profile(store, arms['qrdqn'][2], iters=50).items()}
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=9)
  ap.add_argument('--reps', type=int, default=100, help='graph replays (of 20 steps) per arm and round')
  ap.add_argument('--capacity', type=int, default=1_000_000)
  ap.add_argument('--actions', type=int, nargs='+', default=[6, 18])
  ap.add_argument('--double-q', action='store_true', help='the c51 and qrdqn arms select a* with online(s_t)')
  ap.add_argument('--prioritized', action='store_true', help='the c51 and qrdqn arms take importance weights')
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  out = {'double_q': args.double_q, 'prioritized': args.prioritized, 'batch': B, 'num_atoms': N_ATOMS, 'num_quantiles': N_QUANTILES, 'huber_param': KAPPA,
         'capacity': args.capacity, 'graph_steps': GRAPH_STEPS,
         'steps_per_arm_and_round': args.reps * GRAPH_STEPS, 'rounds': args.rounds, 'by_num_actions': []}
  for a in args.actions:
    out['by_num_actions'].append(run(a, args, dev))
    torch.cuda.empty_cache()
  print(json.dumps(out))


if __name__ == '__main__':
  main()
