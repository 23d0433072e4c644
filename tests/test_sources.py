"""CPU: the library's sources test no build option beyond the listed ones.

csrc/ holds the product; a timing-only switch or a non-default variant lives
in the commit that measured it and in DESIGN §4, not behind an #if here."""

import re

BUILD_OPTIONS = {'DQZ_STEP_TU', 'DQZ_TRACE', 'DQZ_BUILD_ID'}


def _tested_names(text):
  """Identifiers tested on #if / #ifdef / #ifndef / #elif lines (defined(...)
  included), without a header's own include guard (#ifndef X, #define X)."""
  text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
  text = text.replace('\\\n', ' ')
  lines = text.split('\n')
  names = set()
  for i, line in enumerate(lines):
    m = re.match(r'\s*#\s*(if|ifdef|ifndef|elif)\b(.*)', line)
    if not m:
      continue
    ids = set(re.findall(r'[A-Za-z_]\w*', m.group(2).split('//')[0])) - {'defined'}
    nxt = lines[i + 1] if i + 1 < len(lines) else ''
    if m.group(1) == 'ifndef' and len(ids) == 1 and re.fullmatch(r'\s*#\s*define\s+%s\s*' % min(ids), nxt):
      continue
    names |= ids
  return names


_EVERY_FORM = ('#ifndef DQZ_GUARD_H_\n#define DQZ_GUARD_H_\n#ifndef DQZ_A\n#define DQZ_A 0\n#endif\n'
               '#if defined(DQZ_B) && \\\n    !defined( DQZ_C )\n# elif DQZ_D > 1  // DQZ_NOT\n#endif\n'
               '#ifdef DQZ_E\n#endif\nif (DQZ_F) {}\n#endif\n')


def test_sources_test_only_the_listed_build_options():
  from dqn_mgsc_zoo_amd import _native  # pylint: disable=g-import-not-at-top
  assert _tested_names(_EVERY_FORM) == {'DQZ_A', 'DQZ_B', 'DQZ_C', 'DQZ_D', 'DQZ_E'}
  found = {}
  for path in _native.source_files():
    for name in _tested_names(open(path).read()):
      if name.startswith('DQZ_'):
        found.setdefault(name, path)
  assert set(found) == BUILD_OPTIONS, (
      'build options tested by the sources: %s; allowed: %s.  An experiment switch or a variant '
      'kernel does not stay in csrc/: record it in DESIGN §4 with the commit that carried it; a '
      'real build option is a deliberate edit of BUILD_OPTIONS.' % (found, sorted(BUILD_OPTIONS)))
