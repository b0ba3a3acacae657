"""Every LDG_* / LDGPU_LIB environment variable the library and the host package read is a
row of INTEGRATION.md's "Environment variables" table, and the table names nothing else:
an undocumented probe cannot come back unnoticed."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'ld-decode_amd')


def sources(top, exts):
    for d, _, files in os.walk(top):
        for f in files:
            if f.endswith(exts):
                with open(os.path.join(d, f), encoding='utf-8') as fh:
                    yield fh.read()


def names_read():
    names = set()
    for text in sources(os.path.join(PKG, 'csrc'), ('.hip', '.hpp', '.inc')):
        names.update(re.findall(r'getenv\(\s*"(LDG\w*)"', text))
    for text in sources(PKG, ('.py',)):
        names.update(re.findall(r'''environ(?:\.get\(|\[)\s*['"](LDG\w*)['"]''', text))
    return names


def names_documented():
    with open(os.path.join(ROOT, 'INTEGRATION.md'), encoding='utf-8') as fh:
        section = fh.read().split('## Environment variables', 1)[1].split('\n## ', 1)[0]
    return set(re.findall(r'^\| `(LDG\w*)` \|', section, re.M))


def test_environment_variables_match_the_table():
    read, documented = names_read(), names_documented()
    assert len(read) > 10                  # the patterns still find the reads
    assert read == documented, (sorted(read - documented), sorted(documented - read))
