"""--calmd on the GPU (include/mdx.h ``mdx_gbam_set_kept_md`` / ``mdx_gbam_kept_md_counts`` / ``mdx_gbam_kept_bound_md``;
csrc/mdx_kept_md.h): the written records handed on with NM and MD recomputed, in the stream ``write_kept`` compresses.

The expectation is the restatement of tests/md_rule.py applied to the records a write without the stage gives (or to the bytes
the test encoded), behind the restatement of tests/mask_rule.py where a mask is set; every recomputed record also goes through
the restatement's inverse.  The readers and encoders are those of tests/test_gpu_write_kept.py and tests/test_gpu_mask_ends.py,
the crafted records and the random pool those of tests/test_calmd.py and tests/test_mask_ends.py."""

import struct

import numpy as np
import pytest

from mapdamage_amd import sam
from tests import bai_util as Y
from tests import mask_rule as M
from tests import md_rule as R
from tests.test_calmd import crafted
from tests.test_gpu_mask_ends import engine, in_a_file, long_record, raw_header, upper  # noqa: F401
from tests.test_gpu_write_index import first_difference, sorted_data, write_and_index  # noqa: F401
from tests.test_gpu_write_kept import (DEVICE, DROP_BITS, KEPT_TILE, KEPT_WAVE_BYTES, LIBS, lib_data, lib_stream, members_stream,  # noqa: F401
                                       open_stream, read_bam_file, run, split_stream, strata_engine, tables, with_flag)
from tests.test_gpu_write_tags import tree
from tests.test_mask_ends import crafted as mask_crafted
from tests.test_mask_ends import from_ref, genome, pool

pytestmark = pytest.mark.gpu


def never(q, n):
    return False


def long_in_the_middle(flag):
    """A record above KEPT_WAVE_BYTES whose NM and MD stand between two long tags: two stretches for a whole wavefront each."""
    long_tag = b"z" * (KEPT_WAVE_BYTES + 300) + b"\0"
    return M.make_record("5M2D35M", from_ref("5M2D35M", 0, 10, never), flag=flag, pos=10, name=b"middle",
                         tags=b"ZAZ" + long_tag + b"NMC\x07" + b"ZBZ" + long_tag + b"MDZ" + b"10A" * 10 + b"9\0" + b"XAi\x01\x02\x03\x04")


@pytest.fixture(scope="module")
def bodies():
    """The crafted records of both CPU tests and the pool, long records among them, and which of them the flag filter drops:
    one in three, written ones between dropped ones and the reverse; one long record written, one dropped."""
    plain = [c[1] for c in crafted() if in_a_file(c[1])] + [c[1] for c in mask_crafted() if in_a_file(c[1])] + [b for b in pool() if in_a_file(b)]
    at = len(plain) // 2
    plain[at:at] = [long_record(0x10), long_record(0), long_in_the_middle(0), long_in_the_middle(0x10), long_in_the_middle(0)]
    keep = np.arange(len(plain)) % 3 != 1
    keep[at:at + 5] = [True, False, True, False, True]
    assert len(plain) > 4 * KEPT_TILE and all(len(b) + 4 > KEPT_WAVE_BYTES for b in plain[at:at + 5])
    out = []
    for i, (b, k) in enumerate(zip(plain, keep)):
        flag = struct.unpack_from("<H", b, 14)[0]
        out.append(b if k else with_flag(b, flag | DROP_BITS[i % 5]))
    return out, keep


def expected(records, keep, ref=None, mask=None):
    """(the written records recomputed, with their block_size fields; the three counts)"""
    ref = genome() if ref is None else ref
    want, counts = [], [0, 0, 0]
    for body, k in zip(records, keep):
        if not k:
            continue
        if mask is not None:
            body = M.apply(body, mask[0], mask[1], mask[2], False, ref)[0]
        new, done, had = R.outcome(body, ref)
        if done:
            R.check_inverse(new, ref)
        want.append(struct.pack("<i", len(new)) + new)
        counts[0 if done else 1] += 1
        counts[2] += had
    return want, tuple(counts)


def calmd_streams(eng, path, chunk_bytes=256 << 20, mask=None):
    """Every slab's ``write_kept`` with the stage on: (inflated streams per slab, records written, the stream's counts)."""
    streams, n_written = [], 0
    with open_stream(eng, path, chunk_bytes) as stream:
        plain_bound = None
        stream.set_kept_md(True)
        if mask is not None:
            stream.set_kept_mask(mask[0], mask[1], mask[2])
        assert stream.kept_md_counts() == (0, 0, 0)
        while True:
            view = stream.next_view()
            if view is None:
                break
            bound, plain_bound = stream.kept_bound(), stream.kept_bound(calmd=False)
            assert bound > plain_bound and bound == stream.kept_bound(calmd=True)
            members, n, raw = stream.write_kept(view)
            assert len(members) <= bound
            streams.append(members_stream(members))
            assert len(streams[-1]) == raw and len(split_stream(streams[-1])) == n
            n_written += n
        counts = stream.kept_md_counts()
        assert stream.kept_md_counts() == counts
    return streams, n_written, counts


def check(eng, path, records, keep, chunk_bytes=256 << 20, mask=None):
    want, counts = expected(records, keep, mask=mask)
    streams, n_written, got_counts = calmd_streams(eng, path, chunk_bytes, mask)
    got = split_stream(b"".join(streams))
    assert n_written == len(want) == len(got)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g[:400].hex(), w[:400].hex())
    assert got_counts == counts
    return streams, counts, want


# ---------------------------------------------------------------------- 1. through GpuBamStream
def test_crafted_records_and_the_pool(engine, bodies, tmp_path):
    """Written records between dropped ones, long records written and dropped, records that shrink beside records that grow."""
    records, keep = bodies
    sam.write_bam_raw(str(tmp_path / "in.bam"), raw_header(), records)
    _, counts, want = check(engine, tmp_path / "in.bam", records, keep)
    assert counts[0] > 1500 and counts[1] > 50 and counts[2] > 800
    written = [b for b, k in zip(records, keep) if k]
    change = np.sign([len(w) - 4 - len(b) for w, b in zip(want, written)])
    assert (change < 0).sum() >= 3 and (change > 0).sum() > 1000 and (change == 0).sum() > 50
    assert any(a * b < 0 for a, b in zip(change[:-1], change[1:]))
    long_ones = [(len(w) - 4 - len(b)) for w, b in zip(want, written) if len(b) + 4 > KEPT_WAVE_BYTES]
    assert len(long_ones) >= 4 and min(long_ones) < 0 < max(long_ones)


def test_several_slabs(engine, bodies, tmp_path):
    """The counts accumulate over the slabs, and every slab's stream begins at its own offset 0 (slabs of 64 KiB; without the
    records a slab of that size cannot hold)."""
    short = [(b, k) for b, k in zip(*bodies) if len(b) < 30000]
    records, keep = [b for b, _ in short] * 3, [k for _, k in short] * 3
    sam.write_bam_raw(str(tmp_path / "in.bam"), raw_header(), records)
    streams, counts, _ = check(engine, tmp_path / "in.bam", records, keep, chunk_bytes=65536)
    assert len(streams) >= 3 and sum(1 for s in streams if s) >= 3 and counts[0] > 4500


def test_small_views(engine, tmp_path):
    """A view of one record; a view of which nothing is written; one in which every written record is skipped; a tile and one."""
    one = [M.make_record("6M", from_ref("6M", 0, 4, never), pos=4)]
    sam.write_bam_raw(str(tmp_path / "one.bam"), raw_header(), one)
    _, counts, _ = check(engine, tmp_path / "one.bam", one, [True])
    assert counts == (1, 0, 0)
    none = [with_flag(one[0], 0x400)] * 5
    sam.write_bam_raw(str(tmp_path / "none.bam"), raw_header(), none)
    streams, counts, _ = check(engine, tmp_path / "none.bam", none, [False] * 5)
    assert counts == (0, 0, 0) and streams == [b""]
    skipped = [c[1] for c in crafted() if c[0].startswith("skip:") and in_a_file(c[1])] * 3
    assert len(skipped) > 40
    sam.write_bam_raw(str(tmp_path / "skipped.bam"), raw_header(), skipped)
    streams, counts, _ = check(engine, tmp_path / "skipped.bam", skipped, [True] * len(skipped))
    assert counts[:2] == (0, len(skipped)) and split_stream(streams[0]) == [struct.pack("<i", len(b)) + b for b in skipped]
    many = [M.make_record("3M1D3M", from_ref("3M1D3M", 0, i % 50, never), pos=i % 50, flag=0x10 * (i % 2), tags=b"NMC\x01" * (i % 3))
            for i in range(KEPT_TILE + 1)]
    sam.write_bam_raw(str(tmp_path / "many.bam"), raw_header(), many)
    check(engine, tmp_path / "many.bam", many, [True] * len(many))


@pytest.mark.parametrize("what", M.MODES)
def test_behind_the_mask(engine, bodies, tmp_path, what):
    """With each --mask-ends mode: NM and MD are those of the masked bytes."""
    records, keep = bodies
    sam.write_bam_raw(str(tmp_path / "in.bam"), raw_header(), records)
    _, counts, want = check(engine, tmp_path / "in.bam", records, keep, mask=(2, 3, what))
    plain, _ = expected(records, keep)
    assert counts[0] > 1500 and sum(a != b for a, b in zip(want, plain)) > (20 if what == M.MISMATCHES else 500)


def test_switched_off_is_as_never_heard_of(engine, bodies, tmp_path):
    """With the stage off the members are byte for byte those of a stream that never heard of it; on again, the counts begin
    again."""
    records, keep = bodies
    sam.write_bam_raw(str(tmp_path / "in.bam"), raw_header(), records)
    with open_stream(engine, tmp_path / "in.bam") as stream:
        view = stream.next_view()
        never_heard = bytes(stream.write_kept(view)[0])
        assert stream.kept_md_counts() == (0, 0, 0)
    want, counts = expected(records, keep)
    with open_stream(engine, tmp_path / "in.bam") as stream:
        view = stream.next_view()
        stream.set_kept_md(True)
        members, n, raw = stream.write_kept(view)
        assert split_stream(members_stream(members)) == want and raw == sum(len(w) for w in want) and stream.kept_md_counts() == counts
        assert split_stream(members_stream(stream.write_kept(view)[0])) == want        # the slab's own records stayed as they were
        assert stream.kept_md_counts() == tuple(2 * c for c in counts)
        stream.set_kept_md(False)
        assert stream.kept_md_counts() == (0, 0, 0) and stream.kept_bound() == stream.kept_bound(calmd=False)
        members, n, raw = stream.write_kept(view)
        assert bytes(members) == never_heard and raw == sum(len(b) + 4 for b, k in zip(records, keep) if k)
        assert stream.kept_md_counts() == (0, 0, 0)
        stream.set_kept_md(True)
        assert split_stream(members_stream(stream.write_kept(view)[0])) == want and stream.kept_md_counts() == counts


def test_needs_a_reference(bodies, tmp_path):
    from mapdamage_amd.engine import DamageEngine, MdxError
    records, keep = bodies
    sam.write_bam_raw(str(tmp_path / "in.bam"), raw_header(), records)
    with DamageEngine([("s", "l")]) as eng:
        with open_stream(eng, tmp_path / "in.bam") as stream:
            stream.set_kept_md(True)
            view = stream.next_view()
            with pytest.raises(MdxError, match="resident reference") as err:
                stream.write_kept(view)
            assert err.value.code == -3 and stream.kept_md_counts() == (0, 0, 0)
            stream.set_kept_md(False)
            assert split_stream(members_stream(stream.write_kept(view)[0])) == [struct.pack("<i", len(b)) + b for b, k in zip(records, keep) if k]


# ---------------------------------------------------------------------- 2. composition
def test_with_tags_and_a_selection(lib_data):
    """Both tags and a selection of groups: NM and MD follow the tags the write appended."""
    eng, n_groups = strata_engine("pmd", lib_data["ref"])
    ref = upper(lib_data["ref"])
    kw = dict(groups=(1, 2), n_groups=n_groups, group_tag="XG", score_tag="DS")
    n_views = n_written = 0
    total = [0, 0, 0]
    with eng:
        eng.keep_pmd_scores(True)
        with lib_stream(eng, lib_data["dir"] / "in.bam", "pmd") as stream:
            while True:
                view = stream.next_view()
                if view is None:
                    break
                n_views += 1
                eng.tabulate_view(view)
                stream.set_kept_md(False)
                plain = split_stream(members_stream(stream.write_kept(view, **kw)[0]))
                stream.set_kept_md(True)
                assert stream.kept_bound("XG", "DS") > stream.kept_bound("XG", "DS", calmd=False)
                got = split_stream(members_stream(stream.write_kept(view, **kw)[0]))
                want, counts = expected([p[4:] for p in plain], [True] * len(plain), ref)
                assert got == want and stream.kept_md_counts() == counts
                for g in got:
                    f = R.fields(g[4:])
                    names = [t[0] for t in R.tags(g[4:], f["tags_at"])]
                    assert names[-4:] == [b"XG", b"DS", b"NM", b"MD"] and names.count(b"NM") == 1 and names.count(b"MD") == 1
                total = [a + b for a, b in zip(total, counts)]
                n_written += len(got)
            eng.sync()
    assert n_views >= 5 and n_written > 200 and total[0] == n_written


def test_with_an_index(sorted_data, tmp_path):
    """--write-index: the index is that of the written file — its records are the new ones, with their new sizes and offsets."""
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(LIBS) as eng:
        eng.set_reference(sorted_data["ref"])
        with lib_stream(eng, sorted_data["dir"] / "in.bam", "reference") as stream:
            plain_index, _, _ = write_and_index(eng, stream, tmp_path / "plain.bam")
        with lib_stream(eng, sorted_data["dir"] / "in.bam", "reference") as stream:
            stream.set_kept_md(True)
            index, n_slabs, n_views = write_and_index(eng, stream, tmp_path / "kept.bam")
            counts = stream.kept_md_counts()
    assert n_views >= 3 and n_slabs >= 3
    bam = Y.Bam(tmp_path / "kept.bam")
    want = Y.build_index(bam)
    assert index == want, first_difference(index, want)
    records = read_bam_file(tmp_path / "plain.bam")[1]
    new, want_counts = expected([r[4:] for r in records], [True] * len(records), upper(sorted_data["ref"]))
    assert read_bam_file(tmp_path / "kept.bam")[1] == new and counts == want_counts and counts[0] > 50
    assert new != records and index != plain_index


# ---------------------------------------------------------------------- 3. the command line
def test_command_line(lib_data, tmp_path):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    plain = run(lib_data, tmp_path / "out_plain", "in.bam", "--by-pmd-score", "--write-kept", tmp_path / "a" / "kept.bam", "--mask-ends", "2,1")
    out = run(lib_data, tmp_path / "out", "in.bam", "--by-pmd-score", "--write-kept", tmp_path / "b" / "kept.bam", "--mask-ends", "2,1", "--calmd")
    kept = tmp_path / "b" / "kept.bam"
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["kept.bam"]
    log, plain_log = (out / "Runtime_log.txt").read_text(), (plain / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log
    # the run measures the reads as they are
    assert tables(out) == tables(plain) and tree(out) == tree(plain) and len(tree(out)) > 4
    rows = [(folder / "write_kept.tsv").read_text().replace(str(where), "").splitlines() for folder, where in ((out, tmp_path / "b"), (plain, tmp_path / "a"))]
    assert rows[0][0] == rows[1][0] and rows[0][1].split("\t")[:3] == rows[1][1].split("\t")[:3]
    assert (out / "mask_ends.tsv").read_text().replace(str(tmp_path / "b"), "") == (plain / "mask_ends.tsv").read_text().replace(str(tmp_path / "a"), "")
    # ... and hands them on with NM and MD recomputed
    header, records = read_bam_file(tmp_path / "a" / "kept.bam")
    want, counts = expected([r[4:] for r in records], [True] * len(records), upper(lib_data["ref"]))
    assert read_bam_file(kept) == (header, want) and counts[0] > 50 and want != records
    assert int(rows[0][1].split("\t")[3]) == sum(len(w) for w in want) != int(rows[1][1].split("\t")[3])
    assert (out / "calmd.tsv").read_text() == "path\trecords\trecomputed\tskipped\thad_tags\n%s\t%d\t%d\t%d\t%d\n" % ((kept, len(records)) + counts)
    assert "Recomputed NM and MD of %d of %d written records (%d left as they are)" % (counts[0], len(records), counts[1]) in log
    assert "Recomputed" not in plain_log and not (plain / "calmd.tsv").exists()
    assert sorted(p.name for p in out.iterdir()) == sorted([p.name for p in plain.iterdir()] + ["calmd.tsv"])
