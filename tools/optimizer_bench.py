"""What Adam and clip + Adam cost beside the fused centered-RMSProp step.

usage (GPU box): python tools/optimizer_bench.py [--rounds R] [--reps N] [--capacity C] > out.json

Three learners (DQN, B = 32, A = 6) on one synthetic replay, each a hipGraph
of 50 uniform-draw learner steps:
  rmsprop    step_uniform, centered RMSProp fused into the step's kernels
  adam       step_opt_uniform: the step in gradient mode + opt_adam_kernel
  clip_adam  the same behind clip_by_global_norm(10): + opt_norm_kernel
The arms are timed in the same process, interleaved round by round (arm order
rotated), HIP events around N replays; the JSON gives each arm's median and
minimum ms per step over the rounds and the differences to rmsprop.

kernels_us: the optimizer's own launches on a fixed gradient, back to back in
a saturated stream between two events (the duration a kernel trace reports):
apply = dqz_optimizer_apply without clipping (opt_adam_kernel), norm = what
clipping adds (opt_norm_kernel), and the bytes each moves over that time."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dqn_mgsc_zoo_amd import _native, learner as learner_lib, networks, synthetic  # noqa: E402

B, A, GRAPH_STEPS = 32, 6, 50
LR, EPS = 2.5e-4, 0.01 / 32


def make_arm(name, store, cap, dev):
  opt = {'rmsprop': None,
         'adam': learner_lib.adam(LR, eps=EPS),
         'clip_adam': learner_lib.chain(learner_lib.clip_by_global_norm(10.0), learner_lib.adam(LR, eps=EPS))}[name]
  net = networks.dqn_atari_network(A)
  lrn = learner_lib.Learner(net, B, algo='dqn', optimizer=opt, device=dev)
  lrn.set_params(net.init(seed=1))
  slots = torch.zeros((B,), dtype=torch.int32, device=dev)
  ctr = torch.zeros((1,), dtype=torch.int64, device=dev)
  fn = lambda: lrn.step_uniform(store, 0, cap, cap, 7, ctr, slots)
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
  return lrn, g


def time_graph(g, reps, dev):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  torch.cuda.synchronize(dev)
  e0.record()
  for _ in range(reps):
    g.replay()
  e1.record()
  torch.cuda.synchronize(dev)
  return e0.elapsed_time(e1) / (reps * GRAPH_STEPS)


def time_apply(clip, total, n, dev):
  """us per dqz_optimizer_apply on a fixed gradient, n launches back to back."""
  cfg = _native.DqzOptimizerConfig(_native.OPT_ADAM, LR, 0.9, 0.999, 0.0, EPS, clip, A, 0)
  h = ctypes.c_void_p()
  _native.check(_native.lib().dqz_optimizer_create(ctypes.byref(cfg), ctypes.byref(h)))
  th, m, v = (torch.zeros((total,), dtype=torch.float32, device=dev) for _ in range(3))
  g = 1e-3 * torch.randn((total,), dtype=torch.float32, device=dev)
  count = torch.zeros((1,), dtype=torch.int32, device=dev)
  call = lambda: _native.check(_native.lib().dqz_optimizer_apply(
      h, _native.ptr(th), _native.ptr(g), _native.ptr(m), _native.ptr(v), _native.ptr(count),
      _native.stream_handle()))
  for _ in range(20):
    call()
  best = float('inf')
  for _ in range(3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(n):
      call()
    e1.record()
    torch.cuda.synchronize(dev)
    best = min(best, 1e3 * e0.elapsed_time(e1) / n)
  _native.lib().dqz_optimizer_destroy(h)
  return best


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=9)
  ap.add_argument('--reps', type=int, default=40, help='graph replays (of 50 steps) per arm and round')
  ap.add_argument('--capacity', type=int, default=100_000)
  args = ap.parse_args()
  dev = torch.device('cuda:0')
  cap = args.capacity
  store = synthetic.fill_episodic(cap, A, seed=0, device=dev)
  names = ['rmsprop', 'adam', 'clip_adam']
  arms = {n: make_arm(n, store, cap, dev) for n in names}
  ms = {n: [] for n in names}
  for r in range(args.rounds):
    for n in names[r % 3:] + names[:r % 3]:
      ms[n].append(time_graph(arms[n][1], args.reps, dev))
  out = {'batch': B, 'num_actions': A, 'capacity': cap, 'graph_steps': GRAPH_STEPS,
         'steps_per_arm_and_round': args.reps * GRAPH_STEPS, 'rounds': args.rounds, 'ms_per_step': {}}
  for n in names:
    out['ms_per_step'][n] = {'median': round(statistics.median(ms[n]), 5), 'min': round(min(ms[n]), 5),
                             'max': round(max(ms[n]), 5)}
  base = out['ms_per_step']['rmsprop']['median']
  out['extra_us_per_step_vs_rmsprop'] = {
      n: round(1e3 * (out['ms_per_step'][n]['median'] - base), 2) for n in names[1:]}
  for n in names:
    assert arms[n][0].sync_status() == 0 and bool(torch.isfinite(arms[n][0].online).all()), n
  total = arms['adam'][0].total
  apply_us = time_apply(0.0, total, 500, dev)
  both_us = time_apply(10.0, total, 500, dev)
  out['kernels_us'] = {
      'apply': round(apply_us, 2), 'norm': round(both_us - apply_us, 2),
      'apply_GBps': round(7 * 4 * total / apply_us / 1e3, 1),
      'norm_GBps': round(4 * total / max(both_us - apply_us, 1e-9) / 1e3, 1),
      'param_floats': total}
  print(json.dumps(out))


if __name__ == '__main__':
  main()
