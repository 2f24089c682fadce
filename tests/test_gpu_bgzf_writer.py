"""The device BGZF writer (include/mdx.h ``mdx_bgzf_deflate``; ``bgzf_deflate_kernel`` / ``bgzf_gather_kernel`` in
csrc/mdx_gbam.hip, the launch loop ``bgzf_deflate_impl`` in csrc/mdx_bamio.cpp) held, byte for byte, to the host build of the
same encoder (csrc/mdx_deflate.h ``bgzf_member_in_pieces`` through tests/native/deflate_check.cpp, whose members zlib has
inflated): the encoder is integer arithmetic and has one answer, so whatever the device writes differently — another match, a
longer code, a stored piece, a byte left from the launch before — is wrong even where it inflates to the right bytes.

The inputs are tests/deflate_corpus.py's (tests/test_deflate_paths.py: every path of the encoder is reached by them); then the
launch loop at more than one launch (``MDX_BGZF_BATCH``), its bounds, and the three routes that hand it a stream in HBM."""
import ctypes
import gzip
import struct

import numpy as np
import pytest

from mapdamage_amd import sam
from tests import deflate_corpus as C
from tests.test_deflate_paths import compile_native, run_checker

pytestmark = pytest.mark.gpu

MEMBER = C.MAX_IN
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CHUNKS = 8


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """inputs -> the members the host build writes for them, one each (an input is at most a member's bytes)."""
    folder = tmp_path_factory.mktemp("bgzf_writer")
    exe = compile_native(folder, "deflate_check")

    def members_of(datas):
        emit = folder / "members.bin"
        run_checker(exe, folder, [("", d) for d in datas], emit=emit)
        members = C.read_members(emit)
        assert len(members) == len(datas)
        return members
    return members_of


@pytest.fixture(scope="module")
def corpus(host):
    """(label, input, the host build's member) — of an empty input the writer writes nothing (the end-of-file marker is the
    caller's)."""
    cases = C.corpus()
    return [(label, d, m if d else b"") for (label, d), m in zip(cases, host([d for _, d in cases]))]


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine([("s", "l")]) as eng:
        yield eng


def same(got, want, label):
    got, want = bytes(got), bytes(want)
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail("%s: %d bytes from the device, %d from the host build, first difference at byte %d: %s against %s"
                    % (label, len(got), len(want), at, got[at:at + 16].hex(), want[at:at + 16].hex()))


def slices(stream):
    return [stream[lo:lo + MEMBER] for lo in range(0, len(stream), MEMBER)]


def split_members(data):
    """A BGZF file's members by their BSIZE fields."""
    out, at = [], 0
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00", at
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        out.append(data[at:at + size])
        at += size
    assert at == len(data)
    return out


def check_members_of_file(data, host, label, marker=True):
    """Every member of what a route wrote, the end-of-file block apart, against the host build's member of the bytes it
    inflates to; returns the inflated sizes."""
    members = split_members(bytes(data))
    if marker:
        assert members[-1] == EOF_MARKER
        members = members[:-1]
    inflated = [gzip.decompress(m) for m in members]
    assert all(inflated)
    for k, (got, want) in enumerate(zip(members, host(inflated))):
        same(got, want, "%s, member %d" % (label, k))
    return [len(d) for d in inflated]


# ---------------------------------------------------------------------- 1. byte for byte
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_every_input_byte_for_byte(engine, corpus, chunk):
    mine = corpus[chunk::CHUNKS]
    assert mine
    for label, data, want in mine:
        same(engine.bgzf_deflate(data), want, label)


def test_inputs_side_by_side(engine, corpus, host):
    """One call, many members: the inputs back to back, the member borders wherever they fall — and every input filled up
    with zeros to whole members, so that each starts one."""
    plain = b"".join(d for _, d, _ in corpus)
    padded = b"".join(d + b"\0" * (-len(d) % MEMBER) for _, d, _ in corpus)
    assert len(padded) % MEMBER == 0 and len(plain) % MEMBER
    for name, stream in (("back to back", plain), ("filled up", padded)):
        got = bytes(engine.bgzf_deflate(stream))
        want = host(slices(stream))
        at = 0
        for k, m in enumerate(want):
            same(got[at:at + len(m)], m, "%s, member %d" % (name, k))
            at += len(m)
        assert at == len(got)


# ---------------------------------------------------------------------- 2. no stale state
@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_nothing_is_left_from_the_call_before(engine, corpus, chunk):
    """The scratch, the slots and the sizes are the process's and are used again by every call: an input gives the same bytes
    whatever went through them before — the input in front of it in the list, the one behind it, a member of four stored
    pieces."""
    mine = corpus[chunk::CHUNKS]
    full = next(d for label, d, _ in corpus if label == "noise of %d" % MEMBER)
    for label, data, want in mine:
        same(engine.bgzf_deflate(data), want, label + " (in order)")
    for label, data, want in reversed(mine):
        same(engine.bgzf_deflate(data), want, label + " (in reverse order)")
    for label, data, want in mine:
        assert len(engine.bgzf_deflate(full)) == MEMBER + 5 * C.PIECES + 26
        same(engine.bgzf_deflate(data), want, label + " (behind a stored member)")


# ---------------------------------------------------------------------- 3. several launches
@pytest.mark.parametrize("batch,n", [(3, 7 * MEMBER + 1), (1, 3 * MEMBER)])
def test_several_launches(engine, corpus, host, monkeypatch, batch, n):
    """MDX_BGZF_BATCH members per launch: the second trip of the launch loop and a short last one (3 + 3 + 2 members, the
    eighth of one byte; 1 + 1 + 1) write what one launch writes."""
    stream = b"".join(d for _, d, _ in corpus if len(d) > 1000)[5 * MEMBER + 123:][:n]
    assert len(stream) == n
    monkeypatch.delenv("MDX_BGZF_BATCH", raising=False)
    one = bytes(engine.bgzf_deflate(stream))
    monkeypatch.setenv("MDX_BGZF_BATCH", str(batch))
    several = bytes(engine.bgzf_deflate(stream))
    monkeypatch.delenv("MDX_BGZF_BATCH")
    again = bytes(engine.bgzf_deflate(stream))
    want = b"".join(host(slices(stream)))
    same(one, want, "one launch")
    same(several, want, "%d members a launch" % batch)
    same(again, want, "one launch again")
    assert gzip.decompress(several) == stream


# ---------------------------------------------------------------------- 4. bounds
def call(engine, data, out, cap):
    fn = engine._lib.mdx_bgzf_deflate
    fn.restype = ctypes.c_int
    out_len = ctypes.c_int64(-7)
    view = np.frombuffer(data, np.uint8)
    rc = fn(engine._ctx, ctypes.c_void_p(view.ctypes.data), ctypes.c_int64(len(data)), ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(cap),
            ctypes.byref(out_len))
    return rc, out_len.value


@pytest.mark.parametrize("batch", [None, 1])
def test_nothing_is_written_behind_the_output(engine, corpus, host, monkeypatch, batch):
    """``out_cap`` exactly what the members take: nothing behind it is touched; a byte less: MDX_ERR_ARG (-1), no fault, nothing
    written behind the shorter end either — in one launch, and where the shortage shows in the third one — and the context
    encodes on."""
    if batch is None:
        monkeypatch.delenv("MDX_BGZF_BATCH", raising=False)
    else:
        monkeypatch.setenv("MDX_BGZF_BATCH", str(batch))
    stream = b"".join(d for _, d, _ in corpus if len(d) > 1000)[2 * MEMBER + 77:][:2 * MEMBER + 4321]
    want = b"".join(host(slices(stream)))
    need = len(want)
    for cap, rc_want in ((need, 0), (need - 1, -1), (need, 0)):
        out = np.full(need + 4096, 0xEE, np.uint8)
        rc, out_len = call(engine, stream, out, cap)
        assert rc == rc_want, (cap, rc)
        assert (out[cap:] == 0xEE).all(), cap
        if rc == 0:
            assert out_len == need
            same(out[:need].tobytes(), want, "a buffer of exactly %d bytes" % need)
        else:
            assert out_len == 0


@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("k", [1, 3])
def test_the_engines_buffer_holds_stored_members(engine, host, k, extra):
    """``DamageEngine.bgzf_deflate`` sizes its buffer without knowing how the bytes compress: members of nothing but stored pieces
    — 5 bytes a piece and 26 a member more than went in — fit, with and without a member of one byte behind them."""
    data = C.noise(k * MEMBER + extra, 900 + k)
    want = b"".join(host(slices(data)))
    assert len(want) == len(data) + k * (5 * C.PIECES + 26) + extra * (5 + 26)
    assert len(want) <= len(data) + (len(data) // 0xFF00 + 1) * 64         # (the formula of engine.py)
    same(engine.bgzf_deflate(data), want, "%d stored members and %d bytes" % (k, extra))


# ---------------------------------------------------------------------- 5. the routes that pass a stream already in HBM
@pytest.mark.parametrize("index", [False, True])
def test_write_kept_members(engine, host, tmp_path, index):
    """--write-kept at the library level, without and with --write-index: 4000 sorted records, a fifth of them dropped, in
    several slabs; every member of the written file is the host build's.  (With the index: its virtual offsets against the file,
    as tests/test_gpu_write_index.py checks them.)"""
    from tests import test_gpu_write_index as W
    from tests.test_write_index import record, write_sorted_input
    refs = [("chr1", 3_000_000), ("chr2", 100), ("chr3", 600_000)]
    rng = np.random.default_rng(31)
    n = 4000
    tid = np.where(np.arange(n) < 3000, 0, 2)
    pos = np.concatenate([np.sort(rng.integers(0, 2_990_000, 3000)), np.sort(rng.integers(0, 590_000, 1000))])
    records = [record(int(t), int(p), [(int(rng.integers(1, 5000)), "M")], b"s%d" % i, size=100 + int(rng.integers(0, 300)))
               for i, (t, p) in enumerate(zip(tid, pos))]
    keep = rng.random(n) < 0.8
    records = W.with_flags(records, keep)
    write_sorted_input(tmp_path / "in.bam", refs, records, block_bytes=5000, level=0)
    out = tmp_path / "kept.bam"
    if index:
        W.check(engine, tmp_path / "in.bam", out, int(keep.sum()), chunk_bytes=1 << 18)
        data = out.read_bytes()
    else:
        pieces = []
        with W.open_stream(engine, tmp_path / "in.bam", 1 << 18) as stream:
            pieces.append(bytes(engine.bgzf_deflate(sam.bam_header_bytes(stream.header))))
            while True:
                view = stream.next_view()
                if view is None:
                    break
                pieces.append(bytes(stream.write_kept(view)[0]))
        assert sum(1 for p in pieces if p) >= 4
        data = b"".join(pieces) + EOF_MARKER
    sizes = check_members_of_file(data, host, "--write-kept")
    assert sum(sizes) > 8 * MEMBER and sum(1 for s in sizes if s < MEMBER) >= 4        # (the header and three slabs at least)
    kept = [r for r, k in zip(records, keep) if k]
    assert b"".join(gzip.decompress(m) for m in split_members(data)).endswith(b"".join(kept))


def test_rescaled_file_members(host, tmp_path):
    """``rescale_bam_on_device`` (--rescale-only) in slabs of 64 KiB, the smallest there are, of an input whose blocks are
    stored ones, so that its 230 KB make four of them: the header's member and every slab's."""
    from mapdamage_amd.engine import DamageEngine
    from mapdamage_amd.rescale import rescale_bam_on_device
    from tests.test_gpu_write_kept import write_bgzf
    from tests.test_rescale import load
    ref, batch, model, _, _, _ = load(tmp_path)
    sam.write_bam(tmp_path / "compressed.bam", batch, ref.names, ref.lengths, [], None)
    write_bgzf(tmp_path / "in.bam", gzip.decompress((tmp_path / "compressed.bam").read_bytes()), 30011, level=0)
    with DamageEngine([("*", "*")]) as eng:
        rescale_bam_on_device(eng, ref, tmp_path / "in.bam", tmp_path / "out.bam", model, slab_bytes=1 << 16)
    sizes = check_members_of_file((tmp_path / "out.bam").read_bytes(), host, "rescale_bam_on_device")
    assert sum(1 for s in sizes if s < MEMBER) >= 4, sizes                               # (the header and three slabs at least)


def test_bgzf_writer_with_an_engine(engine, corpus, host, tmp_path):
    """``sam.BgzfWriter(engine=...)``: every write compressed on its own, its last member as short as it comes."""
    stream = b"".join(d for _, d, _ in corpus if len(d) > 1000)[:6 * MEMBER]
    cuts = [0, 100, 100 + MEMBER, 100 + 3 * MEMBER + 17, 5 * MEMBER, 5 * MEMBER + 1, 6 * MEMBER]
    with sam.BgzfWriter(tmp_path / "out.gz", engine=engine) as out:
        for lo, hi in zip(cuts, cuts[1:]):
            out.write(stream[lo:hi])
    data = (tmp_path / "out.gz").read_bytes()
    sizes = check_members_of_file(data, host, "BgzfWriter")
    want_sizes = [len(s) for lo, hi in zip(cuts, cuts[1:]) for s in slices(stream[lo:hi])]
    assert sizes == want_sizes and gzip.decompress(data) == stream
