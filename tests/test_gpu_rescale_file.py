"""The rescaled file of --rescale / --rescale-only on the route that never brings a record to the host
(``rescale_bam_on_device`` -> include/mdx.h ``mdx_gbam_rescale_slab``): the rescale kernels in patch mode, ``gbam_patch_qual_kernel``,
``gbam_out_sizes_kernel`` and the host's prefix sum, ``gbam_write_back_kernel``, the device's BGZF writer.

The yardstick is tests/rescale_file_rule.py over the oracle's outputs (held against the host write-back and the reference's
golden by tests/test_rescale_file_rule.py).  Every comparison is equality: of encoded record bytes, of counts, of log lines.

The kernels' constants, with where they stand:
  WRITE_BACK_RECORDS  records per block of gbam_write_back_kernel   csrc/mdx_gbam.hip, mdx_k_gbam_write_back: (n_rec + 31) / 32 blocks
                      of 256 threads, eight lanes per record
  OUT_SIZES_RECORDS   records per block of gbam_out_sizes_kernel    csrc/mdx_gbam.hip, mdx_k_gbam_out_sizes: (n_rec + 255) / 256
  RS_TILE, RS_BLOCK   records per tile and per block of the rescale kernels   csrc/mdx_rescale.hip: "tiles of 64 records",
                      #define RS_BLOCK 512 threads, a lane per record
  RS_BPC              blocks per compute unit of their grid           csrc/mdx_rescale.hip: #define RS_BPC 3
  PARTS, PART_FLOOR   parts of the patch list and the least entries of one   csrc/mdx_bamio.cpp, mdx_gbam_rescale_slab:
                      parts = 256, cap = max(4096, 8 * n / parts)
  PATCH_GRID          threads of gbam_patch_qual_kernel per part     csrc/mdx_gbam.hip, mdx_k_gbam_patch_qual: dim3(16, parts) x 256"""

import ctypes
import gzip
import struct

import numpy as np
import pytest

from mapdamage_amd import fasta, sam
from mapdamage_amd.batch import Reference
from tests import rescale_file_rule as F
from tests.test_gpu_write_kept import write_bgzf

pytestmark = pytest.mark.gpu

WRITE_BACK_RECORDS, OUT_SIZES_RECORDS, RS_TILE, RS_BLOCK, RS_BPC, PARTS, PART_FLOOR, PATCH_GRID = 32, 256, 64, 512, 3, 256, 4096, 16 * 256
SLAB = 1 << 16


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine([("*", "*")]) as eng:
        yield eng


@pytest.fixture(scope="module")
def model():
    return F.make_model()


@pytest.fixture(scope="module")
def mix():
    return F.make_mix()


def write_input(path, header, bodies, layout):
    """``htslib``: members of 0xFF00 inflated bytes; ``3001``: of 3001, level 6 — either way cut wherever the bytes run out, so
    that records straddle blocks, and slabs."""
    if layout == "htslib":
        sam.write_bam_raw(str(path), header, bodies)
    else:
        write_bgzf(path, header + F.stream_of(bodies), 3001)


def expectation(ref, path, corr):
    """(records of the file, the rule's records or the index of the clash, counts, summary lines, status) by the oracle."""
    from oracle import oracle
    al = sam.read_bam(path, keep_raw=True)
    qual_out, mr, status, counts, pvals = oracle.rescale_with_subs(ref, al.batch, corr, F.L5, F.L3)
    want = F.rule(al.raw, al.batch.seq_off, qual_out, mr, status)
    return al, want, F.counts_of(status), oracle.subs_log_lines(counts, pvals), status


def records_of(path):
    return [bytes(r) for r in sam.read_bam(path, keep_raw=True).raw]


def run_route(eng, route, ref, path, out, model, slab):
    from mapdamage_amd.rescale import rescale_bam, rescale_bam_on_device
    eng.reset()
    if route == "device":
        return rescale_bam_on_device(eng, ref, path, out, model, slab_bytes=slab)
    return rescale_bam(eng, ref, path, out, model, chunk_bytes=slab)


def check_file(eng, ref, path, tmp_path, model, slabs=(256 << 20,), routes=("device", "host")):
    """Both routes write the rule's file, count what the oracle counts and log what it logs."""
    al, want, counts, lines, status = expectation(ref, path, model[1])
    assert isinstance(want, list)
    for slab in slabs:
        for route in routes:
            out = tmp_path / ("%s_%d.bam" % (route, slab))
            summary, got_counts = run_route(eng, route, ref, path, out, model[0], slab)
            got = records_of(out)
            assert len(got) == len(want), (route, slab)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w, (route, slab, i, al.qname_at(i))
            assert got_counts == counts, (route, slab)
            assert summary.log_lines() == lines, (route, slab)
            assert sam.read_bam(out, keep_raw=True).raw_header == al.raw_header
    return al, want, status


def slab_records(eng, path, slab):
    """Records per slab of the device decoder."""
    out = []
    with sam.GpuBamStream(eng, str(path), readgroups=[], lib_default=0, chunk_bytes=slab, want_qual=True, want_mate=True, packed=False) as stream:
        while True:
            view = stream.next_view()
            if view is None:
                return out
            out.append(int(view.n_reads))


# ---------------------------------------------------------------------- 1. sizes where the kernels turn
SIZES = [0, 1, 2, WRITE_BACK_RECORDS - 1, WRITE_BACK_RECORDS, WRITE_BACK_RECORDS + 1, RS_TILE - 1, RS_TILE, RS_TILE + 1, OUT_SIZES_RECORDS - 1,
         OUT_SIZES_RECORDS, OUT_SIZES_RECORDS + 1, RS_BLOCK - 1, RS_BLOCK, RS_BLOCK + 1, 1025]


@pytest.mark.parametrize("layout", ["htslib", "3001"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_where_the_kernels_turn(engine, model, mix, tmp_path, n, layout):
    """The first ``n`` records of the mix (0: a header-only file), in one slab and in 64 KiB slabs."""
    ref, header, bodies, _ = mix
    assert SIZES == [0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
    path = tmp_path / "in.bam"
    write_input(path, header, bodies[:n], layout)
    check_file(engine, ref, path, tmp_path, model, slabs=(256 << 20, SLAB))


def test_every_record_unmapped(engine, model, mix, tmp_path):
    """No entry in any part of the list, no record grows: the file comes back byte for byte."""
    ref, header, bodies, kinds = mix
    unmapped = [b for b, k in zip(bodies, kinds) if k == "unmapped"] * 4
    assert len(unmapped) > OUT_SIZES_RECORDS
    for layout in ("htslib", "3001"):
        path = tmp_path / (layout + ".bam")
        write_input(path, header, unmapped, layout)
        _, want, status = check_file(engine, ref, path, tmp_path, model, slabs=(256 << 20, SLAB))
        assert want == unmapped and not status.any()


# ---------------------------------------------------------------------- 2. many slabs
@pytest.mark.parametrize("layout", ["htslib", "3001"])
def test_many_slabs(engine, model, tmp_path, layout):
    """Records without bases interleaved (equal entries of seq_off under gbam_patch_qual_kernel's binary search), rescaled
    records across the slab ends: the head a slab carries over to the next must reach it unpatched."""
    ref, header, bodies, _ = F.make_mix(n=2400, seed=29, interleave_empty=True)
    path = tmp_path / "in.bam"
    write_input(path, header, bodies, layout)
    assert len(header) + len(F.stream_of(bodies)) > 300_000
    per_slab = slab_records(engine, path, SLAB)
    assert len(per_slab) >= 4 and sum(per_slab) == len(bodies)
    al, want, status = check_file(engine, ref, path, tmp_path, model, slabs=(SLAB,))
    # the first record of a later slab whose first byte does not begin a BGZF block: its head lay in the slab in front
    block = 0xFF00 if layout == "htslib" else 3001
    starts = len(header) + np.concatenate([[0], np.cumsum([len(b) + 4 for b in bodies])])
    firsts = np.cumsum(per_slab)[:-1]
    carried = [int(r) for r in firsts if starts[r] % block != 0]
    assert any(status[r] in (F.SINGLE_END, F.INWARD_PAIR) for r in carried), (carried, [int(status[r]) for r in carried])
    lens = np.diff(al.batch.seq_off.astype(np.int64))
    assert (lens == 0).sum() > 1000 and status[lens == 0].tolist() == [F.NO_QUAL] * int((lens == 0).sum())


# ---------------------------------------------------------------------- 3. long records
@pytest.fixture(scope="module")
def long_ref():
    rng = np.random.default_rng(41)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return Reference(["chrR", "chrS"], [rng.choice(acgt, 100_000).tobytes(), rng.choice(acgt, 8_000).tobytes()])


def long_record(ref, n_bases, tags=b"", name=b"long"):
    rng = np.random.default_rng(n_bases)
    seq = np.frombuffer(ref.seqs[0], np.uint8)[1000:1000 + n_bases].copy()
    ends = (np.arange(n_bases) < 12) | (np.arange(n_bases) >= n_bases - 12)
    seq = np.where(ends & (seq == ord("C")), ord("T"), np.where(ends & (seq == ord("G")), ord("A"), seq)).astype(np.uint8)
    return F.encode(name, 0, 0, 1000, [("M", n_bases)], seq.tobytes(), rng.integers(2, 42, n_bases).astype(np.uint8), tags=tags)


@pytest.mark.parametrize("where", ["start", "middle", "end"])
def test_a_record_of_70000_bases(engine, model, long_ref, tmp_path, where):
    ref, header, bodies, _ = F.make_mix(n=280, seed=31, ref=long_ref)
    at = {"start": 0, "middle": 140, "end": 280}[where]
    bodies = bodies[:at] + [long_record(ref, 70_000)] + bodies[at:]
    for layout in ("htslib", "3001"):
        path = tmp_path / (layout + ".bam")
        write_input(path, header, bodies, layout)
        _, want, status = check_file(engine, ref, path, tmp_path, model, slabs=(SLAB,))
        assert status[at] == F.SINGLE_END and want[at] != bodies[at] and len(want[at]) == len(bodies[at]) + 7 > 105_000


def test_mr_lands_behind_a_tag_of_300000_bytes(engine, model, long_ref, tmp_path):
    ref, header, bodies, _ = F.make_mix(n=140, seed=37, ref=long_ref)
    z = b"XLZ" + bytes(np.random.default_rng(3).integers(33, 127, 300_000, dtype=np.uint8)) + b"\0"
    bodies = bodies[:70] + [long_record(ref, 60, tags=b"NMC\x01" + z, name=b"tagged")] + bodies[70:]
    path = tmp_path / "in.bam"
    write_input(path, header, bodies, "htslib")
    _, want, status = check_file(engine, ref, path, tmp_path, model, slabs=(256 << 20, SLAB))
    assert status[70] == F.SINGLE_END and want[70][-8:-4] == b"\0MRf" and len(want[70]) > 300_000


# ---------------------------------------------------------------------- 4. tags and the capacity of the output
@pytest.fixture(scope="module")
def heavy(tmp_path_factory, long_ref):
    """2 000 rescaled records with 2 000 bytes of B:C that do not compress and names of 254 characters: 2.3 KB of name and tags
    a record, which no guess from bases and operations covers."""
    rng = np.random.default_rng(43)
    contig = np.frombuffer(long_ref.seqs[0], np.uint8)
    bodies = []
    for i in range(2000):
        pos = int(rng.integers(0, 90_000))
        seq = contig[pos:pos + 50].copy()
        seq[:12] = np.where(seq[:12] == ord("C"), ord("T"), seq[:12])
        name = (b"h%d_" % i + bytes(rng.integers(97, 123, 254, dtype=np.uint8)))[:254]
        tags = b"XRBC" + struct.pack("<i", 2000) + rng.integers(0, 256, 2000, dtype=np.uint8).tobytes()
        bodies.append(F.encode(name, 0, 0, pos, [("M", 50)], seq.tobytes(), rng.integers(2, 42, 50).astype(np.uint8), tags=tags))
    d = tmp_path_factory.mktemp("heavy")
    sam.write_bam_raw(str(d / "in.bam"), F.raw_header(long_ref), bodies)
    return d / "in.bam", bodies


def test_records_heavy_with_tags_fit_the_output(engine, model, long_ref, heavy, tmp_path):
    """``GpuBamStream.rescale_slab`` takes the capacity of its output from the handle (``mdx_gbam_kept_bound_tagged(g, 7, ..)``: the
    bound include/mdx.h states).  With the guess it made before — 1.5 x bases + 4 x operations + 400 x records + 1 MiB, 2.0 MB
    for this 4.8 MB slab — the BGZF writer ran out of room and the route raised ValueError."""
    path, bodies = heavy
    _, want, status = check_file(engine, long_ref, path, tmp_path, model, routes=("device",))
    assert (status == F.SINGLE_END).all() and sum(len(w) for w in want) > 4_500_000


def cli_rescale(tmp_path, ref, path, model, name, extra=()):
    """``--rescale-only`` through the command line: (exit code, log text, records written)."""
    from mapdamage_amd.main import main
    if not (tmp_path / "ref.fa").exists():
        fasta.write_fasta(tmp_path / "ref.fa", ref)
    folder = tmp_path / name
    folder.mkdir()
    F.write_corr_csv(folder / "Stats_out_MCMC_correct_prob.csv", model[2])
    rc = main(["-i", str(path), "-r", str(tmp_path / "ref.fa"), "-d", str(folder), "--rescale-only", "--rescale-length-5p", str(F.L5),
               "--rescale-length-3p", str(F.L3)] + list(extra))
    return rc, (folder / "Runtime_log.txt").read_text(), folder / (path.stem + ".rescaled.bam")


def summary_lines(log):
    lines = [line.split(" INFO ", 1)[1] for line in log.splitlines() if " INFO " in line]
    return lines[lines.index("Expected substition frequencies before and after rescaling:"):][:16]


def test_records_heavy_with_tags_through_the_command_line(model, long_ref, heavy, tmp_path):
    path, _ = heavy
    _, want, _, lines, _ = expectation(long_ref, path, model[1])
    rc, log, out = cli_rescale(tmp_path, long_ref, path, model, "res")
    assert rc == 0 and "gave up" not in log
    assert records_of(out) == want and summary_lines(log) == lines


# ---------------------------------------------------------------------- 5. mdx_gbam_write_rescaled on its own
@pytest.fixture(scope="module")
def small_file(tmp_path_factory, mix):
    ref, header, bodies, _ = mix
    path = tmp_path_factory.mktemp("write_rescaled") / "in.bam"
    sam.write_bam_raw(str(path), header, bodies[:400])
    return path, sam.read_bam(path, keep_raw=True)


MR_VALUES = np.array([0.0, 1e-40, 1e-5, 2e-5, np.float32(float("%.5f" % 0.123455)), 0.12346, 3.0, np.float32(float("%.5f" % (1e10 / 3)))], np.float32)


def write_rescaled(eng, path, n, entries, counts, cap, mr, rescaled):
    """The file's one slab decoded, then ``mdx_gbam_write_rescaled`` with a patch list made by hand: ``entries`` (uint64, parts x
    cap, or None) and ``counts`` (uint64 per part) go to the engine's device as torch tensors.  -> the inflated stream."""
    import torch
    lib = eng._lib
    dev = torch.device("cuda", 0)
    with sam.GpuBamStream(eng, str(path), readgroups=[], lib_default=0, want_qual=True, want_mate=True, packed=False) as stream:
        view = stream.next_view()
        eng.sync()
        assert int(view.n_reads) == n
        bound = ctypes.c_int64(0)
        lib.mdx_gbam_kept_bound_tagged.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
        assert lib.mdx_gbam_kept_bound_tagged(stream._g, 7, ctypes.byref(bound)) == 0
        out = np.empty(bound.value, np.uint8)
        n_parts = 0 if entries is None else len(counts)
        d_patch = d_count = None
        if n_parts:
            assert entries.shape == (n_parts * cap,)
            d_patch = torch.from_numpy(entries.view(np.int64).copy()).to(dev)
            d_count = torch.from_numpy(np.asarray(counts, np.uint64).view(np.int64).copy()).to(dev)
            torch.cuda.synchronize()
        mr = np.ascontiguousarray(mr, np.float32)
        rescaled = np.ascontiguousarray(rescaled, np.uint8)
        out_len, clash = ctypes.c_int64(0), ctypes.c_int64(-1)
        fn = lib.mdx_gbam_write_rescaled
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                       ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
        fn.restype = ctypes.c_int
        rc = fn(stream._g, d_patch.data_ptr() if n_parts else None, cap, n_parts, d_count.data_ptr() if n_parts else None, mr.ctypes.data,
                rescaled.ctypes.data, out.ctypes.data, out.shape[0], ctypes.byref(out_len), ctypes.byref(clash))
        assert rc == 0 and clash.value == -1, (rc, clash.value, stream._error())
        assert stream.next_view() is None
    return gzip.decompress(bytes(out[:out_len.value])) if out_len.value else b""


def patch_case(al, what):
    """(entries or None, counts, cap, the (index, new quality) pairs that are to be applied) over the records flagged by hand."""
    n = al.batch.n
    off = al.batch.seq_off.astype(np.int64)
    free = np.array([not F.has_tag(bytes(b)) for b in al.raw])
    rescaled = free & (np.arange(n) % 3 != 1)              # by hand: whatever the flags say, records without bases included
    assert (rescaled & (np.diff(off) == 0)).sum() > 5
    inside = np.concatenate([np.arange(off[i], off[i + 1]) for i in np.flatnonzero(rescaled)])      # every index stays inside the column
    assert inside.max() < off[-1] and len(inside) > 6000
    rng = np.random.default_rng(len(what))
    newq = lambda k: rng.integers(0, 94, k).astype(np.uint64)

    def part(indices):
        return indices.astype(np.uint64) | (newq(len(indices)) << np.uint64(32))
    hole = np.uint64(0xFFFFFFFFFFFFFFFF)
    if what == "no parts":
        return rescaled, None, [], 0, np.zeros(0, np.uint64)
    if what == "one part, 5000 entries":
        # (gbam_patch_qual_kernel: 16 blocks x 256 lanes per part, so entry 4096 on is the second trip of the grid-stride loop)
        assert 5000 > PATCH_GRID
        e = part(rng.choice(inside, 5000, replace=False))
        return rescaled, e, [5000], 5000, e
    if what == "more entries counted than the list holds":
        e = part(rng.choice(inside, 700, replace=False))
        return rescaled, e, [1000], 700, e
    if what == "uneven parts":
        counts, cap = [0, 130, 0, 1, 300, 0, 299, 0], 300
        picked = rng.choice(inside, sum(counts), replace=False)
        entries, applied, lo = np.full(len(counts) * cap, hole), [], 0
        for p, c in enumerate(counts):
            e = part(picked[lo:lo + c])
            entries[p * cap:p * cap + c] = e
            applied.append(e)
            lo += c
        return rescaled, entries, counts, cap, np.concatenate(applied)
    assert what == "two bytes of one record in different parts"
    r = int(np.flatnonzero(rescaled & (np.diff(off) > 20))[7])
    cap, entries = 4, np.full(4 * 4, hole)
    a, b = part(np.array([off[r]])), part(np.array([off[r + 1] - 1]))
    entries[0], entries[3 * cap] = a[0], b[0]
    return rescaled, entries, [1, 0, 0, 1], cap, np.concatenate([a, b])


@pytest.mark.parametrize("what", ["no parts", "one part, 5000 entries", "more entries counted than the list holds", "uneven parts",
                                  "two bytes of one record in different parts"])
def test_write_rescaled_on_its_own(engine, small_file, what):
    path, al = small_file
    rescaled, entries, counts, cap, applied = patch_case(al, what)
    qual = al.batch.qual.copy()
    idx = (applied & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert len(np.unique(idx)) == len(idx)
    qual[idx] = (applied >> np.uint64(32)).astype(np.uint8)
    assert what == "no parts" or (qual != al.batch.qual).sum() > len(idx) // 2
    mr = MR_VALUES[np.arange(al.batch.n) % len(MR_VALUES)]
    assert 0 < struct.unpack("<I", struct.pack("<f", MR_VALUES[1]))[0] < 0x00800000            # a subnormal float32
    want = F.rule(al.raw, al.batch.seq_off, qual, mr, np.where(rescaled, F.SINGLE_END, F.UNMAPPED), rounded=True)
    got = write_rescaled(engine, path, al.batch.n, entries, counts, cap, mr, rescaled)
    assert got == F.stream_of(want)


# ---------------------------------------------------------------------- 6. the list's limit
# Which records a block of the rescale kernels takes (csrc/mdx_rescale.hip, mdx_k_rescale and the kernels' tile loops): the grid is
# min(ceil(n / RS_BLOCK), RS_BPC x compute units) blocks of RS_BLOCK / 64 = 8 wavefronts; tile t — records 64 t .. 64 t + 63 — goes to
# wavefront t mod (8 x grid), a lane per record, and wavefront w sits in block w / 8.  The walk kernel behind the fast one takes
# the records a wavefront left out in that same wavefront.  Up to 512 x RS_BPC x compute units records the grid has a wavefront per
# tile, so block b takes records 512 b .. 512 b + 511, and it appends to part b mod 256 (patch_put, csrc/mdx_device.h).  On a grid
# of 3 blocks (one compute unit) tile 24 comes round to wavefront 0: block 0 takes records 0 .. 511 and 1536 .. 1599.
LIMIT_N = 1600


@pytest.fixture(scope="module")
def limit_model():
    return F.make_model(value=0.5)


LIMIT_REF = Reference(["chrC", "chrS"], [b"A" * 100 + b"C" * 3000 + b"A" * 100, b"ACGT" * 50])


def limit_file(changes):
    """LIMIT_N records of 24 bases, all T over the run of C, forward and unpaired: record r changes ``changes.get(r, 0)`` bytes —
    those of quality 30 (the model takes them to 3); a quality of 0 stays 0 at any probability."""
    bodies = []
    for r in range(LIMIT_N):
        k = changes.get(r, 0)
        bodies.append(F.encode(b"t%d" % r, 0, 0, 100 + r, [("M", 24)], b"T" * 24, bytes([30] * k + [0] * (24 - k))))
    return bodies


def limit_changes(block0_tiles_0_to_7, tile_24=0):
    full, rest = divmod(block0_tiles_0_to_7, 24)
    assert full + 1 < RS_BLOCK
    changes = {r: 24 for r in range(full)}
    changes[full] = rest
    changes.update({RS_BLOCK + r: 24 for r in range(10)})           # block 1
    changes.update({2 * RS_BLOCK + 7 * r: 3 for r in range(5)})      # block 2
    if tile_24:
        changes[24 * RS_TILE + 5] = tile_24
    return changes


def check_limit_file(ref, path, corr, changes):
    """The oracle first: every window byte of quality 30 changes, nothing else does."""
    al, want, counts, lines, status = expectation(ref, path, corr)
    from oracle import oracle
    qual_out, _, _ = oracle.rescale(ref, al.batch, corr, F.L5, F.L3)
    per_record = (qual_out != al.batch.qual).reshape(LIMIT_N, 24).sum(axis=1)
    assert per_record.tolist() == [changes.get(r, 0) for r in range(LIMIT_N)] and (status == F.SINGLE_END).all()
    return want, counts, lines, per_record


def test_a_part_exactly_full(engine, limit_model, tmp_path, monkeypatch):
    """(a) records 0 .. 511 change PART_FLOOR bytes between them, so part 0 receives exactly as many entries as it holds: the
    device route writes the rule's file.  Then the same file, and one whose tile 24 brings part 0 to exactly full, on a grid of
    three blocks — fewer than the parts."""
    from mapdamage_amd.engine import DamageEngine
    assert 8 * LIMIT_N // PARTS < PART_FLOOR and LIMIT_N > RS_BLOCK * RS_BPC and LIMIT_N <= 25 * RS_TILE
    changes = limit_changes(PART_FLOOR)
    assert changes[0] == 24 and sum(changes.get(r, 0) for r in range(RS_BLOCK)) == PART_FLOOR
    path = tmp_path / "full.bam"
    sam.write_bam_raw(str(path), F.raw_header(LIMIT_REF), limit_file(changes))
    want, counts, lines, per_record = check_limit_file(LIMIT_REF, path, limit_model[1], changes)
    assert per_record.max() == 24
    check_file(engine, LIMIT_REF, path, tmp_path, limit_model)
    # on one compute unit: block 0 takes tiles 0 .. 7 and 24
    wrapped = limit_changes(PART_FLOOR - 24, tile_24=24)
    assert sum(wrapped.get(r, 0) for r in list(range(RS_BLOCK)) + list(range(24 * RS_TILE, LIMIT_N))) == PART_FLOOR
    path2 = tmp_path / "wrapped.bam"
    sam.write_bam_raw(str(path2), F.raw_header(LIMIT_REF), limit_file(wrapped))
    check_limit_file(LIMIT_REF, path2, limit_model[1], wrapped)
    monkeypatch.setenv("MDX_TEST_CUS", "1")
    with DamageEngine([("*", "*")]) as few:
        for p in (path, path2):
            d = tmp_path / ("few_" + p.stem)
            d.mkdir()
            check_file(few, LIMIT_REF, p, d, limit_model, routes=("device",))


def test_one_entry_more_than_a_part_holds(engine, limit_model, tmp_path):
    """(b) one changed byte more in part 0: the device route raises, naming the list; the command line says that it gave up,
    exits 0, writes the rule's file — and logs the summary of a --host-decode run: nothing is counted twice."""
    from mapdamage_amd.rescale import rescale_bam_on_device
    changes = limit_changes(PART_FLOOR + 1)
    path = tmp_path / "over.bam"
    sam.write_bam_raw(str(path), F.raw_header(LIMIT_REF), limit_file(changes))
    want, counts, lines, _ = check_limit_file(LIMIT_REF, path, limit_model[1], changes)
    engine.reset()
    with pytest.raises(ValueError, match="more rescaled bytes than the list holds"):
        rescale_bam_on_device(engine, LIMIT_REF, path, tmp_path / "never.bam", limit_model[0])
    check_file(engine, LIMIT_REF, path, tmp_path, limit_model, routes=("host",))       # (and the engine is as good as new)
    rc, log, out = cli_rescale(tmp_path, LIMIT_REF, path, limit_model, "default")
    assert rc == 0 and log.count("GPU decode path gave up") == 1 and "more rescaled bytes than the list holds" in log
    assert records_of(out) == want
    rc2, log2, out2 = cli_rescale(tmp_path, LIMIT_REF, path, limit_model, "host", ["--host-decode"])
    assert rc2 == 0 and "gave up" not in log2 and records_of(out2) == want
    assert summary_lines(log) == summary_lines(log2) == lines


# ---------------------------------------------------------------------- 7. clashes
def with_mr(body, kind):
    tag = {"MR:f": b"MRf" + struct.pack("<f", 0.5), "MR:i": b"MRi" + struct.pack("<i", 3), "MR:Z": b"MRZx\0"}[kind]
    return body + tag if kind == "MR:Z" else body[:F.tags_at(body)] + tag + body[F.tags_at(body):]


@pytest.mark.parametrize("kind,name", [("MR:f", b"Q"), ("MR:i", b"n" * 254), ("MR:Z", b"clashing")],
                         ids=["MR:f, a name of 1", "MR:i, a name of 254", "MR:Z"])
def test_a_clash_in_the_third_slab(engine, model, tmp_path, kind, name):
    """Earlier slabs hold MR tags on records that are not rescaled, and the look-alikes; the third holds a rescaled record with
    an MR tag, and a second one behind it in the same slab: both routes stop with the reference's message, naming the first."""
    from mapdamage_amd.rescale import rescale_bam, rescale_bam_on_device
    ref, header, bodies, kinds = F.make_mix(n=2400, seed=47)
    path = tmp_path / "in.bam"
    sam.write_bam_raw(str(path), header, bodies)
    per_slab = slab_records(engine, path, SLAB)
    assert len(per_slab) >= 3
    lo, hi = per_slab[0] + per_slab[1], per_slab[0] + per_slab[1] + per_slab[2]
    mid = (lo + hi) // 2
    first = next(r for r in range(mid, hi) if kinds[r] == "forward")
    second = next(r for r in range(first + 1, hi) if kinds[r] == "reverse")
    f = F.fields(bodies[first])
    old = bodies[first]
    renamed = old[:8] + bytes([len(name) + 1]) + old[9:32] + name + b"\0" + old[32 + f["l_name"]:]
    bodies[first], bodies[second] = with_mr(renamed, kind), with_mr(bodies[second], "MR:f")
    sam.write_bam_raw(str(path), header, bodies)
    per_slab = slab_records(engine, path, SLAB)
    assert per_slab[0] + per_slab[1] <= first < second < sum(per_slab[:3])             # both in the third slab
    al, want, _, _, status = expectation(ref, path, model[1])
    assert want == first and status[first] == status[second] == F.SINGLE_END
    carrying = [r for r in range(per_slab[0] + per_slab[1]) if F.has_tag(bodies[r])]
    assert len(carrying) > 20 and not any(status[r] in (F.SINGLE_END, F.INWARD_PAIR) for r in carrying)
    for fn, kw in ((rescale_bam_on_device, dict(slab_bytes=SLAB)), (rescale_bam, dict(chunk_bytes=SLAB))):
        engine.reset()
        with pytest.raises(SystemExit) as err:
            fn(engine, ref, path, tmp_path / "never.bam", model[0], **kw)
        assert str(err.value) == "Read: %s already has a MR tag, can't rescale" % name.decode()
    # ... and mdx_gbam_record_name on the slab itself
    with sam.GpuBamStream(engine, str(path), readgroups=[], lib_default=0, chunk_bytes=SLAB, want_qual=True, want_mate=True, packed=False) as stream:
        for _ in range(3):
            view = stream.next_view()
        buf = ctypes.create_string_buffer(256)
        assert engine._lib.mdx_gbam_record_name(stream._g, ctypes.c_int64(first - per_slab[0] - per_slab[1]), buf, 256) == 0
        assert buf.value == name


# ---------------------------------------------------------------------- 8. one engine, two files
def test_two_files_through_one_engine(engine, model, limit_model, mix, tmp_path):
    """The second file's records, counts and summary are its own — after another model, and after the same one."""
    ref, header, bodies, _ = mix
    a, b, c = tmp_path / "a.bam", tmp_path / "b.bam", tmp_path / "c.bam"
    sam.write_bam_raw(str(a), header, bodies[:700])
    sam.write_bam_raw(str(b), F.raw_header(LIMIT_REF), limit_file(limit_changes(100)))
    sam.write_bam_raw(str(c), header, bodies[700:])
    for k, (path, r, m) in enumerate(((a, ref, model), (b, LIMIT_REF, limit_model), (c, ref, model), (a, ref, model))):
        d = tmp_path / str(k)
        d.mkdir()
        check_file(engine, r, path, d, m, slabs=(SLAB,), routes=("device",))
