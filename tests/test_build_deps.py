"""What mapdamage_amd.build knows of csrc/: build_lib keeps an object that is newer than its source and the listed headers,
so a header missing from HEADERS, or a source missing from SOURCES, is a stale object in the next build."""

import pathlib
import re

from mapdamage_amd import build

CSRC = build.CSRC
INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def test_every_quoted_include_is_a_listed_header():
    headers = {pathlib.Path(h).resolve() for h in build.HEADERS}
    files = sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".cpp", ".h"))
    assert files
    seen = 0
    for f in files:
        for inc in INCLUDE.findall(f.read_text()):
            seen += 1
            target = (f.parent / inc).resolve()
            assert target.is_file(), "%s includes %s, which does not exist" % (f.name, inc)
            assert target in headers, "%s includes %s, which build.HEADERS does not list" % (f.name, inc)
    assert seen >= len(build.SOURCES)       # (every unit includes the internal interface at least)


def test_every_source_in_csrc_is_built():
    on_disk = sorted(p.name for p in CSRC.iterdir() if p.suffix in (".hip", ".cpp"))
    assert on_disk == sorted(build.SOURCES)
