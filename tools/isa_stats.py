"""Per-kernel ISA counters of libdqz's two code objects (integer-division
expansions, float divisions, vmcnt(0) drains, loads, MFMAs).
usage: python tools/isa_stats.py [substring of the kernel's name]"""
import re
import subprocess
import sys

import device_code

stats, cur = {}, None
for line in device_code.asm_lines():
  m = re.match(r'^(_Z\w+):', line)
  if m:
    cur = m.group(1)
    stats[cur] = dict(lines=0, loads=0, vmcnt0=0, idiv=0, fdiv=0, mfma=0)
    continue
  if cur is None:
    continue
  st = stats[cur]
  st['lines'] += 1
  st['loads'] += ('global_load' in line) or ('buffer_load' in line)
  st['vmcnt0'] += 's_waitcnt vmcnt(0)' in line
  st['idiv'] += 'v_rcp_iflag' in line
  st['fdiv'] += 'v_div_scale' in line
  st['mfma'] += 'v_mfma' in line
  if 's_endpgm' in line:
    cur = None
filt = sys.argv[1] if len(sys.argv) > 1 else ''
for k, v in stats.items():
  name = subprocess.run(['c++filt', k], capture_output=True, text=True).stdout.strip()
  if filt in name:
    print('%-58s %s' % (name.split('(')[0][:58], ' '.join('%s=%d' % kv for kv in v.items())))
