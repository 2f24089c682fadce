"""--mask-ends on the GPU (include/mdx.h ``mdx_gbam_set_kept_mask`` / ``mdx_gbam_kept_mask_counts``; csrc/mdx_kept_mask.h): the
written records handed on with their molecules' ends masked, in place in the stream ``write_kept`` compresses.

The expectation is the restatement of tests/mask_rule.py applied to the records an unmasked write gives (or to the bytes the
test encoded): the readers and encoders are those of tests/test_gpu_write_kept.py, the crafted records and the random pool
those of tests/test_mask_ends.py."""

import struct

import numpy as np
import pytest

from mapdamage_amd import sam
from mapdamage_amd.batch import Reference
from tests import bai_util as Y
from tests import mask_rule as M
from tests.test_gpu_write_index import first_difference, sorted_data, write_and_index  # noqa: F401
from tests.test_gpu_write_kept import (DEVICE, DROP_BITS, KEPT_TILE, KEPT_WAVE_BYTES, LIBS, RAW_HEADER, flags_of, lib_data, lib_stream,  # noqa: F401
                                       members_stream, open_stream, patterns, plain_bodies, read_bam_file, run, split_stream, strata_engine,
                                       tables, with_flag)
from tests.test_gpu_write_tags import big_genome, tree
from tests.test_mask_ends import crafted, every_other, from_ref, genome, pool

pytestmark = pytest.mark.gpu

NAMES = ("m0", "m1", "m2")
CASES = [(2, 2, 0), (3, 1, 1), (255, 255, 0), (1, 0, 0), (0, 1, 1)]


def raw_header():
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in zip(NAMES, genome())) + "@RG\tID:rgA\tSM:s\tLB:l\n"
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(NAMES))
    for n, s in zip(NAMES, genome()):
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", len(s))
    return out


def in_a_file(body):
    """Can the record stand in a BAM file under the header above?  (a record cut short or of a sequence the header does not
    have is the CPU test's alone)"""
    if len(body) < 32:
        return False
    tid, _pos, l_name, _q, _b, n_cig, _f, l_seq = struct.unpack_from("<iiBBHHHI", body, 0)
    return tid < len(NAMES) and 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq <= len(body)


def long_record(flag):
    """A record above KEPT_WAVE_BYTES: forty bases and a long tag."""
    seq = from_ref("40M", 0, 10, every_other)
    return M.make_record("40M", seq, flag=flag, pos=10, name=b"long", tags=b"ZZZ" + b"z" * (KEPT_WAVE_BYTES + 900) + b"\0")


@pytest.fixture(scope="module")
def bodies():
    """The crafted records and the pool with a long record among them, and which of them the flag filter drops: one in three,
    written ones between dropped ones and the reverse."""
    plain = [c[1] for c in crafted() if in_a_file(c[1])] + [b for b in pool() if in_a_file(b)]
    at = len(plain) // 2
    plain[at:at] = [long_record(0x10), long_record(0), long_record(0)]
    keep = np.arange(len(plain)) % 3 != 1
    keep[at:at + 3] = [True, False, True]
    assert len(plain) > 4 * KEPT_TILE and all(len(b) + 4 > KEPT_WAVE_BYTES for b in plain[at:at + 3])
    out = []
    for i, (b, k) in enumerate(zip(plain, keep)):
        flag = struct.unpack_from("<H", b, 14)[0]
        out.append(b if k else with_flag(b, flag | DROP_BITS[i % 5]))
    return out, keep


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine([("s", "l")]) as eng:
        eng.set_reference(Reference(list(NAMES), [s.encode() for s in genome()]))
        yield eng


def upper(ref):
    """The sequences of a ``Reference`` as the restatement reads them: the context's reference is upper case."""
    return [bytes(s).decode().upper() for s in ref.seqs]


def masked_streams(eng, path, k5, k3, what, ss, chunk_bytes=256 << 20):
    """Every slab's masked ``write_kept``: (inflated streams per slab, records written, the stream's counts)."""
    streams, n_written = [], 0
    with open_stream(eng, path, chunk_bytes) as stream:
        stream.set_kept_mask(k5, k3, what, bool(ss))
        assert stream.kept_mask_counts() == (0, 0)
        while True:
            view = stream.next_view()
            if view is None:
                break
            bound = stream.kept_bound()
            members, n, raw = stream.write_kept(view)
            assert len(members) <= bound
            streams.append(members_stream(members))
            assert len(streams[-1]) == raw and len(split_stream(streams[-1])) == n
            n_written += n
        counts = stream.kept_mask_counts()
        assert stream.kept_mask_counts() == counts
    return streams, n_written, counts


def expected(records, keep, k5, k3, what, ss, ref=None):
    """(the written records masked, with their block_size fields; records with a masked base; masked bases)"""
    want, n_records, n_bases = [], 0, 0
    for body, k in zip(records, keep):
        if not k:
            continue
        masked, count = M.apply(body, k5, k3, what, bool(ss), genome() if ref is None else ref)
        want.append(struct.pack("<i", len(masked)) + masked)
        n_records += count > 0
        n_bases += count
    return want, n_records, n_bases


def check(eng, path, records, keep, k5, k3, what, ss, chunk_bytes=256 << 20):
    want, n_records, n_bases = expected(records, keep, k5, k3, what, ss)
    streams, n_written, counts = masked_streams(eng, path, k5, k3, what, ss, chunk_bytes)
    got = split_stream(b"".join(streams))
    assert n_written == len(want) == len(got)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g.hex(), w.hex())
    assert counts == (n_records, n_bases)
    return streams, counts


# ---------------------------------------------------------------------- 1. through GpuBamStream
@pytest.mark.parametrize("k5,k3,ss", CASES)
@pytest.mark.parametrize("what", M.MODES)
def test_every_mode(engine, bodies, tmp_path, what, k5, k3, ss):
    """The crafted records and the pool, written records between dropped ones, a long record written and one dropped."""
    records, keep = bodies
    sam.write_bam_raw(str(tmp_path / "in.bam"), raw_header(), records)
    _, counts = check(engine, tmp_path / "in.bam", records, keep, k5, k3, what, ss)
    assert counts[0] > 50 and counts[1] >= counts[0]


@pytest.mark.parametrize("what", M.MODES)
def test_several_slabs(engine, bodies, tmp_path, what):
    """The counts accumulate over the slabs (the records four times over: half a megabyte in slabs of 64 KiB)."""
    records, keep = bodies[0] * 4, np.tile(bodies[1], 4)
    sam.write_bam_raw(str(tmp_path / "in.bam"), raw_header(), records)
    streams, counts = check(engine, tmp_path / "in.bam", records, keep, 2, 2, what, 0, chunk_bytes=65536)
    assert len(streams) >= 3 and sum(1 for s in streams if s) >= 3 and counts[0] > 100


@pytest.mark.parametrize("what", M.MODES)
def test_small_views(engine, tmp_path, what):
    """A view of one record; a view of which nothing is written; a tile and one record."""
    one = [M.make_record("6M", from_ref("6M", 0, 4, every_other), pos=4)]
    sam.write_bam_raw(str(tmp_path / "one.bam"), raw_header(), one)
    _, counts = check(engine, tmp_path / "one.bam", one, [True], 2, 2, what, 0)
    assert counts[0] == 1
    none = [with_flag(one[0], 0x400)] * 5
    sam.write_bam_raw(str(tmp_path / "none.bam"), raw_header(), none)
    streams, counts = check(engine, tmp_path / "none.bam", none, [False] * 5, 2, 2, what, 0)
    assert counts == (0, 0) and streams == [b""]
    many = [M.make_record("6M", from_ref("6M", 0, i % 50, every_other), pos=i % 50, flag=0x10 * (i % 2)) for i in range(KEPT_TILE + 1)]
    sam.write_bam_raw(str(tmp_path / "many.bam"), raw_header(), many)
    check(engine, tmp_path / "many.bam", many, [True] * len(many), 1, 1, what, 0)


@pytest.mark.parametrize("what", M.MODES)
def test_the_pools_of_write_kept(tmp_path, what):
    """The records tests/test_gpu_write_kept.py encodes — every length from 0 to 200 bases, random nibbles (=, IUPAC and N among
    them), every alignment of the record in the stream — over the two sequences its header names, kept by a coin."""
    from mapdamage_amd.engine import DamageEngine
    n = 4 * KEPT_TILE + 1
    keep = patterns(n)["coin"]
    records = [with_flag(b, int(f)) for b, f in zip(plain_bodies(False)[:n], flags_of(keep))]
    sam.write_bam_raw(str(tmp_path / "in.bam"), RAW_HEADER, records)
    ref = upper(big_genome())
    want, n_records, n_bases = expected(records, keep, 3, 2, what, 0, ref)
    with DamageEngine([("s", "l")]) as eng:
        eng.set_reference(big_genome())
        streams, n_written, counts = masked_streams(eng, tmp_path / "in.bam", 3, 2, what, 0)
    assert split_stream(b"".join(streams)) == want and n_written == len(want)
    assert counts == (n_records, n_bases) and n_records > (5 if what == M.MISMATCHES else 50)


# ---------------------------------------------------------------------- 2. misuse
def test_mismatches_need_a_reference(bodies, tmp_path):
    from mapdamage_amd.engine import DamageEngine, MdxError
    records, keep = bodies
    sam.write_bam_raw(str(tmp_path / "in.bam"), raw_header(), records)
    with DamageEngine([("s", "l")]) as eng:
        with open_stream(eng, tmp_path / "in.bam") as stream:
            stream.set_kept_mask(2, 2, M.MISMATCHES)
            view = stream.next_view()
            with pytest.raises(MdxError, match="without a resident reference") as err:
                stream.write_kept(view)
            assert err.value.code == -3 and stream.kept_mask_counts() == (0, 0)
            # ... the other modes need none
            stream.set_kept_mask(2, 2, M.TRANSITIONS)
            members, n, _ = stream.write_kept(view)
            want, n_records, n_bases = expected(records, keep, 2, 2, M.TRANSITIONS, 0)
            assert split_stream(members_stream(members)) == want and n == len(want)
            assert stream.kept_mask_counts() == (n_records, n_bases)


def test_set_and_clear(engine, bodies, tmp_path):
    from mapdamage_amd.engine import MdxError
    records, keep = bodies
    sam.write_bam_raw(str(tmp_path / "in.bam"), raw_header(), records)
    plain = [struct.pack("<i", len(b)) + b for b, k in zip(records, keep) if k]
    with open_stream(engine, tmp_path / "in.bam") as stream:
        view = stream.next_view()
        assert stream.kept_mask_counts() == (0, 0)
        assert split_stream(members_stream(stream.write_kept(view)[0])) == plain
        for bad in ((256, 0, M.ALL, 0), (0, 256, M.ALL, 0), (-1, 2, M.ALL, 0), (2, -1, M.ALL, 0)):
            with pytest.raises(MdxError) as err:
                stream.set_kept_mask(*bad)
            assert err.value.code == -1
        with pytest.raises(ValueError):
            stream.set_kept_mask(2, 2, "everything")
        assert split_stream(members_stream(stream.write_kept(view)[0])) == plain          # (a refused mask is none)
        stream.set_kept_mask(3, 1, M.ALL)
        want, n_records, n_bases = expected(records, keep, 3, 1, M.ALL, 0)
        assert split_stream(members_stream(stream.write_kept(view)[0])) == want
        assert stream.kept_mask_counts() == (n_records, n_bases)
        assert split_stream(members_stream(stream.write_kept(view)[0])) == want          # the slab's own records stayed as they were
        assert stream.kept_mask_counts() == (2 * n_records, 2 * n_bases)
        stream.set_kept_mask(0, 0)
        assert stream.kept_mask_counts() == (0, 0)
        assert split_stream(members_stream(stream.write_kept(view)[0])) == plain
        assert stream.kept_mask_counts() == (0, 0)
        stream.set_kept_mask(0, 1, M.MISMATCHES, True)                                      # setting again starts the counts again
        want, n_records, n_bases = expected(records, keep, 0, 1, M.MISMATCHES, 1)
        assert split_stream(members_stream(stream.write_kept(view)[0])) == want
        assert stream.kept_mask_counts() == (n_records, n_bases)


# ---------------------------------------------------------------------- 3. composition
@pytest.mark.parametrize("what", M.MODES)
def test_with_tags_and_a_selection(lib_data, what):
    """Both tags and a selection of groups: the tags are those of the unmasked write, the record in front of them is masked."""
    eng, n_groups = strata_engine("pmd", lib_data["ref"])
    ref = upper(lib_data["ref"])
    kw = dict(groups=(1, 2), n_groups=n_groups, group_tag="XG", score_tag="DS")
    n_views = n_records = n_bases = n_written = 0
    with eng:
        eng.keep_pmd_scores(True)
        with lib_stream(eng, lib_data["dir"] / "in.bam", "pmd") as stream:
            while True:
                view = stream.next_view()
                if view is None:
                    break
                n_views += 1
                eng.tabulate_view(view)
                stream.set_kept_mask(0, 0)
                plain = split_stream(members_stream(stream.write_kept(view, **kw)[0]))
                stream.set_kept_mask(8, 8, what)
                got = split_stream(members_stream(stream.write_kept(view, **kw)[0]))
                want, r, b = expected([p[4:] for p in plain], [True] * len(plain), 8, 8, what, 0, ref)
                assert got == want and all(g[-12:-10] == b"XG" and g[-7:-4] == b"DSf" for g in got)
                assert stream.kept_mask_counts() == (r, b)
                n_records, n_bases, n_written = n_records + r, n_bases + b, n_written + len(got)
            eng.sync()
    # (the synthetic reads' damage is sparse: of the records of two PMD groups a few dozen show a mismatch in eight bases)
    assert n_views >= 5 and n_written > 200 and n_records >= 10 and n_bases >= n_records


def test_with_an_index(sorted_data, tmp_path):
    """--write-index: the index is that of the written file, by the derivation of tests/test_gpu_write_index.py — no size and
    no offset moved."""
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(LIBS) as eng:
        eng.set_reference(sorted_data["ref"])
        with lib_stream(eng, sorted_data["dir"] / "in.bam", "reference") as stream:
            write_and_index(eng, stream, tmp_path / "plain.bam")
        with lib_stream(eng, sorted_data["dir"] / "in.bam", "reference") as stream:
            stream.set_kept_mask(2, 2, M.MISMATCHES)
            index, n_slabs, n_views = write_and_index(eng, stream, tmp_path / "kept.bam")
            counts = stream.kept_mask_counts()
    assert n_views >= 3 and n_slabs >= 3
    bam = Y.Bam(tmp_path / "kept.bam")
    want = Y.build_index(bam)
    assert index == want, first_difference(index, want)
    records = read_bam_file(tmp_path / "plain.bam")[1]
    masked, n_records, n_bases = expected([r[4:] for r in records], [True] * len(records), 2, 2, M.MISMATCHES, 0, upper(sorted_data["ref"]))
    assert read_bam_file(tmp_path / "kept.bam")[1] == masked and counts == (n_records, n_bases) and n_records > 50


# ---------------------------------------------------------------------- 4. the command line
def test_command_line(lib_data, tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain = run(lib_data, tmp_path / "out_plain", "in.bam", "--by-pmd-score", "--write-kept", tmp_path / "a" / "kept.bam")
    out = run(lib_data, tmp_path / "out", "in.bam", "--by-pmd-score", "--write-kept", tmp_path / "b" / "kept.bam",
              "--mask-ends", "2,1", "--mask-what", "mismatches")
    kept = tmp_path / "b" / "kept.bam"
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["kept.bam"]
    log, plain_log = (out / "Runtime_log.txt").read_text(), (plain / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log
    # the run measures the reads as they are
    assert tables(out) == tables(plain) and tree(out) == tree(plain) and len(tree(out)) > 4
    assert (out / "write_kept.tsv").read_text().replace(str(tmp_path / "b"), "") == (plain / "write_kept.tsv").read_text().replace(str(tmp_path / "a"), "")
    # ... and hands them on masked
    header, records = read_bam_file(tmp_path / "a" / "kept.bam")
    assert records == [r for r, k in zip(lib_data["records"], lib_data["kept"]) if k]
    want, n_records, n_bases = expected([r[4:] for r in records], [True] * len(records), 2, 1, M.MISMATCHES, 0, upper(lib_data["ref"]))
    assert read_bam_file(kept) == (header, want) and 50 < n_records <= n_bases and want != records
    assert (out / "mask_ends.tsv").read_text() == "path\tk5\tk3\twhat\tsingle_stranded\trecords\tbases\n%s\t2\t1\tmismatches\t0\t%d\t%d\n" % (
        kept, n_records, n_bases)
    assert "Wrote %d records to %s (groups: all)" % (len(records), kept) in log
    assert "Masked %d bases in %d of %d written records (5p 2, 3p 1: mismatches)" % (n_bases, n_records, len(records)) in log
    assert "Masked" not in plain_log and not (plain / "mask_ends.tsv").exists()
    assert sorted(p.name for p in out.iterdir()) == sorted([p.name for p in plain.iterdir()] + ["mask_ends.tsv"])
