"""What the Rainbow step costs beside the prioritized double-Q C51 step with
the same optimizer.

usage (GPU box): python tools/rainbow_bench.py [--rounds R] [--reps N] [--capacity C] [--actions A] > out.json

Two learners (B = 32, N = 51 atoms) on one synthetic replay, each a hipGraph of
20 learner steps with chain(clip_by_global_norm(10), adam(6.25e-5,
eps=0.005/32)), fixed uneven importance weights in (0, 1]:
  prioritized_c51  sample_uniform + C51Learner(double_q, prioritized).step
  rainbow          sample_uniform + dqz_rainbow_noise (three applications) +
                   RainbowLearner.step: the noisy dueling network
The arms are timed in the same process, interleaved round by round (arm order
alternating), HIP events around N replays; the JSON gives each arm's median,
minimum and maximum ms per step over the rounds and Rainbow's difference.  The
priorities are written by both, the sum tree is part of neither.

launch_us: each learner's profile entry on a fixed batch, in a run of its own
after the timed rounds: each launch of the step repeated back to back between
two events.  Rainbow's slots: rb_noisy_forward (the e_in scaling, three fc1
products, both hidden layers, both noisy fc2 layers and the dueling combine),
c51_head, rb_dhidden, rb_fc1_dx (four dX products and their combine),
rb_fc_grad (the fc2 leaves and three fc1 dW products)."""
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

B, N, GRAPH_STEPS = 32, 51, 20
LR, EPS, VMAX = 6.25e-5, 0.005 / 32, 10.0


def optimizer():
  return learner_lib.chain(learner_lib.clip_by_global_norm(10.0), learner_lib.adam(LR, eps=EPS))


def make_arm(name, a, store, cap, dev):
  support = np.linspace(-VMAX, VMAX, N).astype(np.float32)
  weights = torch.linspace(0.05, 1.0, B, dtype=torch.float32, device=dev)
  slots = torch.zeros((B,), dtype=torch.int32, device=dev)
  ctr = torch.zeros((1,), dtype=torch.int64, device=dev)
  if name == 'rainbow':
    net = networks.rainbow_atari_network(a, support, 0.1)
    lrn = learner_lib.RainbowLearner(net, B, optimizer=optimizer(), device=dev)
    nctr = torch.zeros((1,), dtype=torch.int64, device=dev)
    noise = torch.zeros((3, lrn.noise_len), dtype=torch.float32, device=dev)

    def fn():
      learner_lib.sample_uniform(0, cap, cap, B, 7, ctr, slots)
      lrn.make_noise(11, nctr, 3, out=noise)
      lrn.step(store, slots, weights, noise)
    extra = dict(noise=noise)
  else:
    net = networks.c51_atari_network(a, support)
    lrn = learner_lib.C51Learner(net, B, optimizer=optimizer(), device=dev, double_q=True, prioritized=True)

    def fn():
      learner_lib.sample_uniform(0, cap, cap, B, 7, ctr, slots)
      lrn.step(store, slots, weights)
    extra = {}
  lrn.set_params(net.init(seed=1))
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
  return lrn, g, slots, weights, extra


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
  ap.add_argument('--reps', type=int, default=50, help='graph replays (of 20 steps) per arm and round')
  ap.add_argument('--capacity', type=int, default=100_000)
  ap.add_argument('--actions', type=int, default=6)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  cap, a = args.capacity, args.actions
  store = synthetic.fill_episodic(cap, a, seed=0, device=dev)
  names = ['prioritized_c51', 'rainbow']
  arms = {n: make_arm(n, a, store, cap, dev) for n in names}
  ms = {n: [] for n in names}
  for r in range(args.rounds):
    for n in names[r % 2:] + names[:r % 2]:
      ms[n].append(time_graph(arms[n][1], args.reps, dev))
  out = {'batch': B, 'num_actions': a, 'num_atoms': N, 'capacity': cap, 'graph_steps': GRAPH_STEPS,
         'steps_per_arm_and_round': args.reps * GRAPH_STEPS, 'rounds': args.rounds, 'ms_per_step': {}}
  for n in names:
    out['ms_per_step'][n] = {'median': round(statistics.median(ms[n]), 5), 'min': round(min(ms[n]), 5),
                             'max': round(max(ms[n]), 5)}
  out['rainbow_extra_us_per_step'] = round(
      1e3 * (out['ms_per_step']['rainbow']['median'] - out['ms_per_step']['prioritized_c51']['median']), 2)
  for n in names:
    assert arms[n][0].sync_status() == 0 and bool(torch.isfinite(arms[n][0].online).all()), n
  out['launch_us'] = {}
  for n in names:
    lrn, _, slots, weights, extra = arms[n]
    out['launch_us'][n] = {k: round(1e3 * v, 2) for k, v in lrn.profile(store, slots, weights, iters=50, **extra).items()}
  print(json.dumps(out))


if __name__ == '__main__':
  main()
