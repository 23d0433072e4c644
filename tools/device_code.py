"""Device-only gfx950 builds of the product's translation units
(__graft_entry__.SRCS, with the product build's flags): assembly for the ISA
tools, unbundled ELFs for the code identity check.

usage: python tools/device_code.py [extra hipcc flags, e.g. -DDQZ_TRACE]
prints each unit's .text SHA-256 and size.  Two trees whose lines agree run
the same device code; the build id and the __hip_cuid symbol live outside
.text and differ by design."""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # pylint: disable=g-import-not-at-top

OBJCOPY = shutil.which('llvm-objcopy') or os.path.join(
    os.path.dirname(os.path.dirname(os.path.realpath(entry.HIPCC))), 'lib', 'llvm', 'bin', 'llvm-objcopy')


def unit_name(src):
  return os.path.splitext(os.path.basename(src))[0]


def _compile(src, out, mode, extra):
  subprocess.check_call([entry.HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', *extra,
                         '-I' + os.path.join(ROOT, 'include'), '--cuda-device-only', *mode, '-o', out, src],
                        stderr=subprocess.DEVNULL)
  return out


def asm(outdir, extra=()):
  """{unit: path of its device assembly}, written under outdir."""
  return {unit_name(s): _compile(s, os.path.join(outdir, unit_name(s) + '.s'), ['-S'], extra) for s in entry.SRCS}


def asm_lines(extra=()):
  """The device assembly of every unit, one list of lines."""
  with tempfile.TemporaryDirectory() as d:
    return [line for path in asm(d, extra).values() for line in open(path)]


def elf(outdir, extra=()):
  """{unit: path of its unbundled device ELF}, written under outdir."""
  mode = ['--no-gpu-bundle-output', '-c']
  return {unit_name(s): _compile(s, os.path.join(outdir, unit_name(s) + '.co'), mode, extra) for s in entry.SRCS}


def text_hashes(extra=()):
  """{unit: (SHA-256 of the device ELF's .text, its size in bytes)}."""
  out = {}
  with tempfile.TemporaryDirectory() as d:
    for unit, path in elf(d, extra).items():
      text = path + '.text'
      subprocess.check_call([OBJCOPY, '-O', 'binary', '--only-section=.text', path, text])
      data = open(text, 'rb').read()
      out[unit] = (hashlib.sha256(data).hexdigest(), len(data))
  return out


if __name__ == '__main__':
  for name, (sha, size) in text_hashes(sys.argv[1:]).items():
    print('%-14s .text sha256 %s  %d bytes' % (name, sha, size))
