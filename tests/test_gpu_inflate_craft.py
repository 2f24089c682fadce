"""gbam_inflate_kernel (csrc/mdx_gbam.hip, the device build of csrc/mdx_inflate.h) on the hand-built DEFLATE streams of
tests/deflate_craft.py — codes, matches, headers and block sequences the format allows and zlib never writes — laid out as
the decode path lays blocks out: payloads back to back, outputs at any alignment, other blocks' outputs right beside them.

The rule is the one the host build meets on the same streams (tests/test_deflate_craft.py), accept / refuse parity with
zlib: where zlib inflates the whole stream to exactly ISIZE bytes (at most 65536) the status is ISIZE, the bytes are zlib's
and the CRC32 passes; everything else — refused by zlib, input that ends early, more than 65536 bytes, another length than
ISIZE — has a negative status.  Whatever the verdict, no byte outside [offset, offset + ISIZE) of any block is written:
the library fills the output with 0xEE before the launch, and the gaps between the blocks still hold it afterwards.  A
second launch over the same cases in reversed order at other offsets gives every case the same status and bytes.

(A block of ISIZE 0 is not decoded at all — the kernel skips it, as the decode path skips the empty EOF block: streams to
be refused are declared with a size of at least 1.)"""
import zlib

import numpy as np
import pytest

from tests import deflate_craft as dc
from tests.inflate_util import inflate_blocks

pytestmark = pytest.mark.gpu

LAUNCH = 512                 # blocks per launch
FILL = 0xEE


@pytest.fixture(scope="module")
def eng():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine([("s", "l")]) as e:
        yield e


def zlib_says(comp):
    try:
        z = zlib.decompressobj(-15)
        out = z.decompress(comp, dc.CAP + 1)
        if z.eof and len(out) <= dc.CAP:
            return out
    except zlib.error:
        pass
    return None


def _first_difference(a, b):
    a, b = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    n = min(len(a), len(b))
    d = np.flatnonzero(a[:n] != b[:n])
    return int(d[0]) if len(d) else n


def _launch(eng, jobs, phase):
    """jobs: [(label, stream, isize, zlib's bytes or None)] -> [(status, bytes, crc ok)]; asserts the guards.  The outputs lie
    at offsets that take every residue of 16 in turn (from `phase` on), at least 64 bytes apart."""
    offs, at = [], 64
    for i, (_, _, isize, _) in enumerate(jobs):
        at += -(at - (phase + i)) % 16                       # at % 16 == (phase + i) % 16
        offs.append(at)
        at += isize + 64 + (i * 7) % 48
    total = at + 64
    assert all(o % 16 == (phase + i) % 16 for i, o in enumerate(offs))
    cases = [(stream, isize, zlib.crc32(z if z is not None else b"") & 0xFFFFFFFF) for _, stream, isize, z in jobs]
    status, out, crc_ok, got_offs = inflate_blocks(eng, cases, offs, total)
    assert list(got_offs) == offs
    guard = np.ones(total, bool)
    for o, (_, _, isize, _) in zip(offs, jobs):
        guard[o:o + isize] = False
    hit = np.flatnonzero(guard & (out != FILL))
    if len(hit):
        owner = max(i for i, o in enumerate(offs) if o <= hit[0]) if hit[0] >= offs[0] else 0
        raise AssertionError("byte %d outside every block's output was written: %d bytes behind the start of %r (ISIZE %d), status %d"
                             % (hit[0], hit[0] - offs[owner], jobs[owner][0], jobs[owner][2], status[owner]))
    return [(int(status[i]), out[offs[i]:offs[i] + jobs[i][2]].tobytes(), bool(crc_ok[i])) for i in range(len(jobs))]


def _jobs(cases):
    """every case under its own size, and a spread of the valid ones under four wrong sizes"""
    jobs = []
    for i, c in enumerate(cases):
        z = zlib_says(c.stream)
        if c.expected is not None:
            assert z == c.expected, c
        size = len(z) if (z is not None and (c.expected is not None or len(z) > 0)) else c.size
        jobs.append((c.label, c.stream, size, z if z is not None and len(z) == size else None))
        if c.expected is not None and len(c.expected) >= 4 and i % 5 == 0:
            true = len(c.expected)
            for wrong in (true - 1, true + 1, true // 2, 1):
                if wrong <= dc.CAP:
                    jobs.append(("%s, ISIZE %d for %d" % (c.label, wrong, true), c.stream, wrong, None))
    return jobs


def _check(eng, cases):
    jobs = _jobs(cases)
    bad = []
    forward = []
    for lo in range(0, len(jobs), LAUNCH):
        forward += _launch(eng, jobs[lo:lo + LAUNCH], phase=lo // LAUNCH)
    for (label, _, isize, z), (status, got, crc_ok) in zip(jobs, forward):
        if z is not None:
            if status != isize or got != z or not crc_ok:
                bad.append("%s: status %d for %d bytes, first difference at %d, crc %s" % (label, status, isize, _first_difference(got, z), crc_ok))
        elif status >= 0:
            bad.append("%s: status %d (ISIZE %d) for a stream to be refused" % (label, status, isize))
    assert not bad, "%d of %d:\n" % (len(bad), len(jobs)) + "\n".join(bad[:12])
    # the other way round, at other offsets: nothing depends on the neighbours
    back = []
    rev = jobs[::-1]
    for lo in range(0, len(rev), LAUNCH):
        back += _launch(eng, rev[lo:lo + LAUNCH], phase=5 + lo // LAUNCH)
    for (label, _, isize, z), a, b in zip(jobs, forward, back[::-1]):
        # (of a refused block too: what it wrote before it stopped depends on the stream alone)
        assert a[0] == b[0] and a[1] == b[1],"%s: status %d, then %d in reversed order; first difference at %d" % (label, a[0], b[0], _first_difference(a[1], b[1]))
    return len(jobs)


@pytest.mark.parametrize("theme", list(dc.THEMES))
def test_device_inflate_on_crafted_streams(eng, theme):
    n = _check(eng, dc.THEMES[theme]())
    assert n >= len(dc.THEMES[theme]())


@pytest.mark.parametrize("seed", dc.RANDOM_SEEDS)
def test_device_inflate_on_random_crafted_streams_and_damaged_twins(eng, seed):
    cases = dc.random_corpus(seed)
    _check(eng, cases)
    verdicts = [zlib_says(c.stream) is not None for c in cases if c.expected is None]
    assert 6 * sum(verdicts) >= len(verdicts) and 6 * (len(verdicts) - sum(verdicts)) >= len(verdicts)
