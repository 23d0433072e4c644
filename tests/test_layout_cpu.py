"""CPU: csrc/layout.hpp names the hand-off words where the kernels expect them
and carves scratch into aligned, ordered, non-overlapping blocks.

tests/layout_check.cpp holds the checks (plain host C++, no device call); this
compiles it with the project's hipcc and runs it."""

import os
import subprocess


def test_layout_header_is_a_source_of_the_build_id():
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  assert 'layout.hpp' in [os.path.basename(f) for f in _native.source_files()]


def test_sync_words_and_carver(tmp_path):
  import __graft_entry__ as entry  # pylint: disable=g-import-not-at-top
  here = os.path.dirname(os.path.abspath(__file__))
  exe = str(tmp_path / 'layout_check')
  subprocess.check_call([entry.HIPCC, '-x', 'c++', '-std=c++17', '-O1', '-Wall',
                         '-I' + os.path.join(entry.PKG, 'csrc'), os.path.join(here, 'layout_check.cpp'), '-o', exe])
  run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=False)
  assert run.returncode == 0 and 'layout ok' in run.stdout, run.stdout
