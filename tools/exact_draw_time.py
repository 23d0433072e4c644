"""Device time of the learned-logit exact mode at 1M slots against the default.

usage (GPU box): python tools/exact_draw_time.py [--skip-calls] [--label NAME]

1. The stand-alone calls, 200 back to back between two events: the exact
   draw / add (dqz_logits_sample_exact / _add_exact) and the default ones
   (a draw: 32 queries, including the host-to-device copy of the uniforms).
2. Whole learn calls at B = 32 on a synthetic store, each as a captured graph
   of 20 calls, the graph replayed 50 times between device synchronisations:
     two_call   dqz_logits_sample_exact -> int32 copy -> Learner.step
     fused      Learner.step_logits(uniforms, exact=True)
                (dqz_learner_step_logits_exact; skipped, with a note, where
                the library does not have it)
     default    Learner.step_logits(uniforms), the running-state draw
   Five repeats, the three interleaved within each; prints one JSON line with
   the median and the (min, max) of the five, in us per learn call.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dqn_mgsc_zoo_amd import _native, learner as learner_lib, networks, synthetic  # noqa: E402
from dqn_mgsc_zoo_amd import replay_circular as rc  # noqa: E402

CAP, B = 1_000_000, 32
CALLS_PER_GRAPH, REPLAYS, REPEATS = 20, 50, 5


def time_calls(dev_logits, rng):
  u = rng.random(B)
  for _ in range(5):
    dev_logits.sample_exact(u)
    dev_logits.sample_abs(u)
  torch.cuda.synchronize()
  for name, fn in (('exact draw', lambda: dev_logits.sample_exact(u)),
                   ('default draw', lambda: dev_logits.sample_abs(u)),
                   ('exact add', lambda: dev_logits.add_default_exact(5, CAP - 10)),
                   ('default add', lambda: dev_logits.add_default(5, CAP - 10))):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200):
      fn()
    e1.record()
    torch.cuda.synchronize()
    print(name, 'us per call (a draw: 32 queries, incl. the H2D copy of u):',
          round(e0.elapsed_time(e1) / 200 * 1e3, 2))


def capture(fn):
  """A graph of CALLS_PER_GRAPH calls of fn, warmed up on a side stream."""
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(3):
      fn()
  torch.cuda.current_stream().wait_stream(side)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(CALLS_PER_GRAPH):
      fn()
  g.replay()
  torch.cuda.synchronize()
  return g


def us_per_call(g):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(REPLAYS):
    g.replay()
  torch.cuda.synchronize()
  return 1e6 * (time.perf_counter() - t0) / (REPLAYS * CALLS_PER_GRAPH)


def time_learns(dev_logits, rng, label):
  dev = dev_logits.device
  lib = _native.lib()
  store = synthetic.fill_episodic(CAP, 6, seed=0, device=dev)
  net = networks.dqn_atari_network(6)
  lrn = learner_lib.Learner(net, B, algo='dqn', device=dev)
  lrn.set_params(net.init(0))
  u = torch.from_numpy(rng.random(B)).to(dev)
  idx = torch.zeros((B,), dtype=torch.int64, device=dev)
  slots = torch.zeros((B,), dtype=torch.int32, device=dev)

  def two_call():
    _native.check(lib.dqz_logits_sample_exact(dev_logits.handle, _native.ptr(dev_logits.logits),
                                              _native.ptr(u), B, _native.ptr(idx), None,
                                              _native.stream_handle()))
    lrn.step(store, idx.to(torch.int32))

  forms = {'two_call': two_call}
  if 'dqz_learner_step_logits_exact' in _native.SIGNATURES:
    forms['fused'] = lambda: lrn.step_logits(store, dev_logits, slots, uniforms=u, exact=True)
  else:
    print('fused: this library has no dqz_learner_step_logits_exact; skipped')
  forms['default'] = lambda: lrn.step_logits(store, dev_logits, slots, uniforms=u)
  graphs = {k: capture(fn) for k, fn in forms.items()}
  samples = {k: [] for k in graphs}
  for _ in range(REPEATS):
    for k, g in graphs.items():
      samples[k].append(us_per_call(g))
  assert lrn.sync_status() == 0
  out = {'label': label, 'slots': CAP, 'batch': B, 'calls_per_graph': CALLS_PER_GRAPH,
         'replays': REPLAYS, 'repeats': REPEATS}
  for k, v in samples.items():
    out[k + '_us'] = {'median': round(statistics.median(v), 2), 'min': round(min(v), 2),
                      'max': round(max(v), 2)}
  print(json.dumps(out))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--skip-calls', action='store_true', help='only the learn-call timings')
  ap.add_argument('--label', default='', help='copied into the JSON line')
  args = ap.parse_args()
  rng = np.random.default_rng(0)
  dev_logits = rc._DeviceLogits(CAP, max_queries=64)  # pylint: disable=protected-access
  dev_logits.load(rng.standard_normal(CAP).astype(np.float32))
  if not args.skip_calls:
    time_calls(dev_logits, rng)
    dev_logits.load(rng.standard_normal(CAP).astype(np.float32))  # the adds wrote slot 5
  time_learns(dev_logits, rng, args.label)


if __name__ == '__main__':
  main()
