"""us per logit census and per jumbled add at the reference's 1M capacity
(GPU box).

`dqz_logits_census` (three launches over 4 MB of logits + 1 MB of flags) beside
an existing full-buffer pass, `dqz_logits_probs` (one launch: reads the logits,
writes 4 MB of probabilities), and `dqz_store_jumble` (eight 7 KB row copies in
one launch).  Device time from HIP events over back-to-back calls in a
saturated stream (medians of 5 repeats of 500 calls), host time per call from
perf_counter.  Prints one JSON line.
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dqn_mgsc_zoo_amd import replay_circular as rc  # noqa: E402
from dqn_mgsc_zoo_amd import replay_circular_nonsense as rcn  # noqa: E402
from dqn_mgsc_zoo_amd import _native  # noqa: E402
from dqn_mgsc_zoo_amd import store as store_lib  # noqa: E402

CAP, CALLS, REPEATS = 1_000_000, 500, 5


def timed(fn):
  for _ in range(20):
    fn()
  torch.cuda.synchronize()
  dev, host = [], []
  for _ in range(REPEATS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t = time.perf_counter()
    e0.record()
    for _ in range(CALLS):
      fn()
    e1.record()
    host.append((time.perf_counter() - t) * 1e6 / CALLS)
    torch.cuda.synchronize()
    dev.append(e0.elapsed_time(e1) * 1e3 / CALLS)
  return {'device_us': round(statistics.median(dev), 2), 'host_us': round(statistics.median(host), 2)}


def main():
  rng = np.random.default_rng(0)
  dl = rc._DeviceLogits(CAP)  # pylint: disable=protected-access
  dl.load((3 * rng.standard_normal(CAP)).astype(np.float32))
  flags = torch.from_numpy((rng.random(CAP) < 0.02).astype(np.uint8)).cuda()
  acc = rcn.Census()
  lib = _native.lib()
  out = {'capacity': CAP, 'calls': CALLS, 'repeats': REPEATS}

  def census(left_head, size):
    _native.check(lib.dqz_logits_census(dl.handle, _native.ptr(dl.logits), _native.ptr(flags), left_head, size,
                                        _native.ptr(acc.tensor), _native.stream_handle()))

  out['census_full'] = timed(lambda: census(0, CAP))
  out['census_wrapped'] = timed(lambda: census(CAP - 12345, CAP))
  out['census_empty'] = timed(lambda: census(0, 0))  # the final launch alone
  dl.probs()  # seeds the running state: the timed calls are the one pass
  out['logits_probs'] = timed(dl.probs)

  st = store_lib.FrameStore(1024, 4096)
  st.fidx.copy_(torch.from_numpy(np.stack([np.arange(8) + 2 * i for i in range(1024)]).astype(np.int32)))
  out['store_jumble'] = timed(lambda: st.jumble(7, 0, 1000, 250, 333, 500, range(3000, 3008)))
  print(json.dumps(out))


if __name__ == '__main__':
  main()
