"""What the C51 step costs beside the DQN step with the same optimizer.

usage (GPU box): python tools/c51_bench.py [--rounds R] [--reps N] [--capacity C] [--double-q] [--prioritized] > out.json

Three learners (B = 32, A = 6) on one synthetic replay, each a hipGraph of 20
learner steps with chain(clip_by_global_norm(10), adam(2.5e-4, eps=0.01/32)):
  dqn_clip_adam        tools/optimizer_bench.py's "clip + Adam" line:
                       step_uniform, the draw inside the forward launch
  dqn_clip_adam_slots  the same step on slots from a sampler launch of its own
                       (sample_uniform + step): what the C51 step is built like
  c51                  sample_uniform + C51Learner.step, N = 51 atoms
The arms are timed in the same process, interleaved round by round (arm order
rotated), HIP events around N replays; the JSON gives each arm's median,
minimum and maximum ms per step over the rounds and C51's difference to both
DQN arms.  --double-q and --prioritized switch the c51 arm's learner to
double-Q selection (a third network copy) and to importance-weighted steps
(fixed uneven weights in (0, 1]; the priorities are written, the sum tree is not
part of the arm).

launch_us: dqz_c51_profile on a fixed batch, in a run of its own after the
timed rounds: each launch of the step repeated back to back between two events
(the duration a kernel trace reports), beside dqz_learner_profile's figures of
the DQN step's launches."""
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

B, A, N, GRAPH_STEPS = 32, 6, 51, 20
LR, EPS, VMAX = 2.5e-4, 0.01 / 32, 10.0


def optimizer():
  return learner_lib.chain(learner_lib.clip_by_global_norm(10.0), learner_lib.adam(LR, eps=EPS))


def make_arm(name, store, cap, dev, double_q=False, prioritized=False):
  weights = None
  if name == 'c51':
    net = networks.c51_atari_network(A, np.linspace(-VMAX, VMAX, N).astype(np.float32))
    lrn = learner_lib.C51Learner(net, B, optimizer=optimizer(), device=dev, double_q=double_q,
                                 prioritized=prioritized)
    if prioritized:
      weights = torch.linspace(0.05, 1.0, B, dtype=torch.float32, device=dev)
  else:
    net = networks.dqn_atari_network(A)
    lrn = learner_lib.Learner(net, B, algo='dqn', optimizer=optimizer(), device=dev)
  lrn.set_params(net.init(seed=1))
  slots = torch.zeros((B,), dtype=torch.int32, device=dev)
  ctr = torch.zeros((1,), dtype=torch.int64, device=dev)
  if name == 'dqn_clip_adam':
    fn = lambda: lrn.step_uniform(store, 0, cap, cap, 7, ctr, slots)
  else:
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=9)
  ap.add_argument('--reps', type=int, default=100, help='graph replays (of 20 steps) per arm and round')
  ap.add_argument('--capacity', type=int, default=1_000_000)
  ap.add_argument('--double-q', action='store_true', help='the c51 arm selects a* with online(s_t)')
  ap.add_argument('--prioritized', action='store_true', help='the c51 arm takes importance weights')
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  cap = args.capacity
  store = synthetic.fill_episodic(cap, A, seed=0, device=dev)
  names = ['dqn_clip_adam', 'dqn_clip_adam_slots', 'c51']
  arms = {n: make_arm(n, store, cap, dev, args.double_q, args.prioritized) for n in names}
  ms = {n: [] for n in names}
  for r in range(args.rounds):
    for n in names[r % 3:] + names[:r % 3]:
      ms[n].append(time_graph(arms[n][1], args.reps, dev))
  out = {'batch': B, 'num_actions': A, 'num_atoms': N, 'double_q': args.double_q, 'prioritized': args.prioritized,
         'capacity': cap, 'graph_steps': GRAPH_STEPS,
         'steps_per_arm_and_round': args.reps * GRAPH_STEPS, 'rounds': args.rounds, 'ms_per_step': {}}
  for n in names:
    out['ms_per_step'][n] = {'median': round(statistics.median(ms[n]), 5), 'min': round(min(ms[n]), 5),
                             'max': round(max(ms[n]), 5)}
  c51 = out['ms_per_step']['c51']['median']
  out['c51_extra_us_per_step'] = {
      n: round(1e3 * (c51 - out['ms_per_step'][n]['median']), 2) for n in names[:2]}
  for n in names:
    assert arms[n][0].sync_status() == 0 and bool(torch.isfinite(arms[n][0].online).all()), n
  # the launches' own durations, after the timed rounds (the profile synchronises between phases)
  lrn, _, slots, weights = arms['c51']
  out['launch_us'] = {'c51': {k: round(1e3 * v, 2) for k, v in lrn.profile(store, slots, weights, iters=50).items()}}
  net = networks.dqn_atari_network(A)
  dqn = learner_lib.Learner(net, B, algo='dqn', device=dev)  # the profile runs the fused-RMSProp step
  dqn.set_params(net.init(seed=1))
  out['launch_us']['dqn'] = {k: round(1e3 * v, 2) for k, v in dqn.profile(store, slots, iters=50).items()}
  print(json.dumps(out))


if __name__ == '__main__':
  main()
