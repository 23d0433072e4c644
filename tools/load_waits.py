"""Flags kernels whose loads before the first barrier are split by vmcnt
waits (a load issued after a wait costs an extra memory round trip).
usage: python tools/load_waits.py [asm.s]   (builds both units' device asm if omitted)"""
import re
import subprocess
import sys

import device_code

lines = open(sys.argv[1]) if len(sys.argv) > 1 else device_code.asm_lines()
cur, seen_barrier, waited, late = None, False, False, {}
for line in lines:
  m = re.match(r'^(_Z\w+):', line)
  if m:
    cur, seen_barrier, waited = m.group(1), False, False
    late[cur] = 0
    continue
  if cur is None or seen_barrier:
    continue
  if 's_barrier' in line:
    seen_barrier = True
  elif re.search(r's_waitcnt.*vmcnt', line):
    waited = True
  elif ('global_load' in line or 'buffer_load' in line) and waited:
    late[cur] += 1
for k, v in late.items():
  if v:
    name = subprocess.run(['c++filt', k], capture_output=True, text=True).stdout.strip().split('(')[0]
    print('%-50s loads issued after a vmcnt wait (before 1st barrier): %d' % (name, v))
