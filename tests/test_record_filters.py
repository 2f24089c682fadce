"""Record filters (--min-mapq, --require-flags, --exclude-flags, --min-read-length, --max-read-length) without a GPU: the
command line's arguments, ``sam.RecordFilter.drops`` on records written by hand, and the host decoders — ``read_sam``, the
Python BAM reader, the native decoder with ``mdx_bam_apply_record_filter``, ``reader.BAMReader`` — against a predicate
written here in numpy.  The yardstick of a filtered run is the same run without filters on a file that holds only the
records that pass, in the same order."""

import numpy as np
import pytest

from mapdamage_amd import sam, synth
from mapdamage_amd.batch import batch_from_records, concat_batches
from mapdamage_amd.sam import RecordFilter

RGS = [{"ID": "rgA", "SM": "s1", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s1", "LB": "lib2"}]
MAPQS = (0, 1, 24, 25, 29, 30, 37, 60, 255)
FILTERS = [RecordFilter(min_mapq=25), RecordFilter(require_flags=0x11), RecordFilter(exclude_flags=0x8400),
           RecordFilter(min_length=35), RecordFilter(max_length=100),
           RecordFilter(min_mapq=25, require_flags=0x1, exclude_flags=0x400, min_length=31, max_length=140)]


def predicate(flt, flag16, mapq, l_seq):
    """The issue's table, one reason after the other: the index of the first that drops the record, or -1."""
    out = np.full(len(flag16), -1, np.int64)
    for i, (f, q, n) in enumerate(zip(flag16.tolist(), mapq.tolist(), l_seq.tolist())):
        if (f & flt.require_flags) != flt.require_flags:
            out[i] = 0
        elif (f & flt.exclude_flags) != 0:
            out[i] = 1
        elif q < flt.min_mapq:
            out[i] = 2
        elif n < flt.min_length:
            out[i] = 3
        elif flt.max_length and n > flt.max_length:
            out[i] = 4
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A small file, every way: reads of 30..150 bases and of none, extra flag bits (the file's bits 14 and 15 among them),
    MAPQ of the whole list."""
    d = tmp_path_factory.mktemp("record_filters")
    ref = synth.small_genome()
    b = concat_batches([synth.make_reads(ref, 600, 5, len_range=(30, 150), nlib=2, frac_softclip=0.1, frac_ins=0.05, frac_filtered=0.05,
                                         with_qual=True),
                        synth.make_edge_reads(ref, with_qual=True, nlib=2),
                        batch_from_records([dict(flag=0, lib=k % 2, tid=0, pos=100 + k, cigar=[(0, 30)], seq="") for k in range(6)],
                                           with_qual=True)])
    rng = np.random.default_rng(11)
    flag16 = b.flag.astype(np.int64)
    for bit in (0x1, 0x10, 0x400, 0x800, 0x4000, 0x8000):
        flag16 |= np.where(rng.random(b.n) < 0.15, bit, 0)
    mapq = rng.choice(MAPQS, b.n)
    import dataclasses
    full = dataclasses.replace(b, flag=flag16.astype(np.uint16))
    rg = [RGS[int(i)]["ID"] for i in b.lib]
    sam.write_bam(str(d / "in.bam"), full, ref.names, ref.lengths, RGS, rg, mapq=mapq)
    sam.write_bam(str(d / "straddle.bam"), full, ref.names, ref.lengths, RGS, rg, mapq=mapq, htslib_blocks=False, block_bytes=3001)
    sam.write_sam(str(d / "in.sam"), full, ref.names, ref.lengths, RGS, rg, mapq=mapq)
    lens = np.diff(b.seq_off.astype(np.int64))
    assert (lens == 0).sum() >= 6 and lens.max() > 140 and set(mapq.tolist()) == set(MAPQS)
    return dict(dir=d, ref=ref, batch=full, flag16=flag16, mapq=mapq, lens=lens, rg=rg)


# ---------------------------------------------------------------------- the command line
def parse(tmp_path, *args):
    from mapdamage_amd.main import parse_args
    return parse_args(["-i", "x.bam", "-r", "ref.fa", "-d", str(tmp_path / "out")] + list(args))


def test_arguments(tmp_path):
    o = parse(tmp_path)
    assert o.record_filter == RecordFilter() and not o.record_filter.active
    o = parse(tmp_path, "--min-mapq", "25", "--require-flags", "0x11", "--exclude-flags", "1024", "--min-read-length", "30",
              "--max-read-length", "150")
    assert o.record_filter == RecordFilter(25, 0x11, 0x400, 30, 150) and o.record_filter.active
    assert parse(tmp_path, "--exclude-flags", "0XfFfF").record_filter.exclude_flags == 65535
    assert parse(tmp_path, "--min-mapq", "255").record_filter.min_mapq == 255
    assert parse(tmp_path, "--min-read-length", "40", "--max-read-length", "40").record_filter.active
    # (min alone above any max of 0: no upper bound)
    assert parse(tmp_path, "--min-read-length", "400").record_filter == RecordFilter(min_length=400)


@pytest.mark.parametrize("args", [
    ["--min-mapq", "-1"], ["--min-mapq", "256"], ["--min-mapq", "x"],
    ["--require-flags", "65536"], ["--require-flags", "-1"], ["--require-flags", "0x10000"], ["--require-flags", "0xZ"],
    ["--exclude-flags", "65536"], ["--exclude-flags", "1e3"], ["--exclude-flags", "PAIRED"],
    ["--min-read-length", "-1"], ["--max-read-length", "-5"],
    ["--min-read-length", "50", "--max-read-length", "49"],
    ["--min-mapq", "25", "--rescale-only"], ["--exclude-flags", "0x400", "--rescale-only"],
    ["--min-mapq", "25", "--stats-only", "--fix-nicks"], ["--max-read-length", "90", "--stats-only", "--fix-nicks"]])
def test_argument_errors(tmp_path, args, capsys):
    with pytest.raises(SystemExit) as err:
        parse(tmp_path, *args)
    assert err.value.code == 2
    if "--rescale-only" in args or "--stats-only" in args:
        assert "counts records" in capsys.readouterr().err


def test_help_says_none_is_a_reference_option():
    from mapdamage_amd.main import build_parser
    text = " ".join(build_parser().format_help().split())
    for option in ("--min-mapq", "--require-flags", "--exclude-flags", "--min-read-length", "--max-read-length"):
        assert option in text
    assert "Not a reference option" in text and "not the query length of the CIGAR" in text
    assert "still rewrites every record" in text


# ---------------------------------------------------------------------- RecordFilter
def test_record_filter_values():
    for bad in (dict(min_mapq=256), dict(min_mapq=-1), dict(require_flags=65536), dict(exclude_flags=-1), dict(min_length=-1),
                dict(max_length=-1), dict(min_length=10, max_length=9)):
        with pytest.raises(ValueError):
            RecordFilter(**bad)
    assert not RecordFilter().active
    for name in ("min_mapq", "require_flags", "exclude_flags", "min_length", "max_length"):
        assert RecordFilter(**{name: 1}).active
    with pytest.raises(Exception):
        RecordFilter().min_mapq = 3          # frozen
    s = RecordFilter(25, 0x11, 0x400, 30, 150).as_struct()
    assert (s.min_mapq, s.require_flags, s.exclude_flags, s.min_length, s.max_length) == (25, 0x11, 0x400, 30, 150)


def test_drops_by_hand():
    q = RecordFilter(min_mapq=25)
    assert q.drops([0, 0, 0, 0], [24, 25, 255, 0], [50, 50, 50, 50]).tolist() == [2, -1, -1, 2]
    # two required bits, one present
    r = RecordFilter(require_flags=0x11)
    assert r.drops([0x1, 0x10, 0x11, 0x13, 0], [30] * 5, [50] * 5).tolist() == [0, 0, -1, -1, 0]
    x = RecordFilter(exclude_flags=0x410)
    assert x.drops([0x400, 0x10, 0x1, 0], [30] * 4, [50] * 4).tolist() == [1, 1, -1, -1]
    # l_seq 0
    assert RecordFilter(min_length=1).drops([0, 0], [30, 30], [0, 1]).tolist() == [3, -1]
    assert RecordFilter(max_length=40).drops([0, 0, 0], [30] * 3, [0, 40, 41]).tolist() == [-1, -1, 4]
    assert RecordFilter(min_length=30).drops([0], [30], [2 ** 31 - 1]).tolist() == [-1]
    # the file's bits 14 and 15 are tested as the file carries them
    hi = RecordFilter(require_flags=0x4000, exclude_flags=0x8000)
    assert hi.drops([0x4000, 0xC000, 0x0, 0x8000], [30] * 4, [50] * 4).tolist() == [-1, 1, 0, 0]
    # the first reason in the order require, exclude, MAPQ, shortest, longest
    every = RecordFilter(min_mapq=25, require_flags=0x1, exclude_flags=0x400, min_length=30, max_length=100)
    flags = [0x400, 0x401, 0x1, 0x1, 0x1, 0x1]
    assert every.drops(flags, [0, 0, 0, 25, 25, 25], [10, 10, 10, 10, 101, 100]).tolist() == [0, 1, 2, 3, 4, -1]
    assert every.counts(flags, [0, 0, 0, 25, 25, 25], [10, 10, 10, 10, 101, 100]).tolist() == [6, 1, 1, 1, 1, 1]
    assert RecordFilter().drops([0xFFFF], [0], [0]).tolist() == [-1]


@pytest.mark.parametrize("flt", FILTERS)
def test_drops_is_the_predicate(files, flt):
    want = predicate(flt, files["flag16"], files["mapq"], files["lens"])
    np.testing.assert_array_equal(flt.drops(files["flag16"], files["mapq"], files["lens"]), want)
    assert (want >= 0).any() and (want < 0).any()


# ---------------------------------------------------------------------- the parsers
def expect_flags(plain_flags, why):
    return np.where(why >= 0, plain_flags | 0x200, plain_flags).astype(np.uint16)


def expect_counts(why):
    return np.concatenate([[len(why)], np.bincount(why[why >= 0], minlength=5)]).astype(np.uint64)


@pytest.mark.parametrize("flt", FILTERS)
def test_python_parsers(files, flt):
    d = files["dir"]
    why = predicate(flt, files["flag16"], files["mapq"], files["lens"])
    for plain, got in ((sam.read_sam(str(d / "in.sam")), sam.read_sam(str(d / "in.sam"), record_filter=flt)),
                       (sam.read_bam(str(d / "in.bam")), sam.read_bam(str(d / "in.bam"), record_filter=flt)),
                       (sam.read_bam(str(d / "straddle.bam")), sam.read_bam(str(d / "straddle.bam"), record_filter=flt))):
        assert not hasattr(plain, "filter_counts")
        np.testing.assert_array_equal(plain.batch.flag, (files["flag16"] & 0x3FFF).astype(np.uint16))
        np.testing.assert_array_equal(got.batch.flag, expect_flags(plain.batch.flag, why))
        np.testing.assert_array_equal(got.filter_counts, expect_counts(why))
        for name in ("tid", "pos", "tlen", "cigar", "seq", "qual", "seq_off"):
            np.testing.assert_array_equal(getattr(got.batch, name), getattr(plain.batch, name))


def test_read_sam_reads_mapq_only_under_a_threshold(tmp_path):
    text = "@SQ\tSN:c1\tLN:100\nr0\t0\tc1\t1\t%s\t4M\t*\t0\t0\tACGT\tIIII\n"
    for bad in ("x", "", "2.5", "3O", "+5", " 7", "1_0", "٣"):
        (tmp_path / "bad.sam").write_text(text % bad)
        for flt in (None, RecordFilter(), RecordFilter(exclude_flags=0x400), RecordFilter(min_length=2)):
            assert sam.read_sam(str(tmp_path / "bad.sam"), record_filter=flt).batch.n == 1
        with pytest.raises(sam.BAMError, match="MAPQ"):
            sam.read_sam(str(tmp_path / "bad.sam"), record_filter=RecordFilter(min_mapq=1))
    # a number is compared as a number, whatever its size (the device parser leaves such a line to this one)
    for value, flag in (("1000", 0), ("256", 0), ("-1", 0x200), ("007", 0x200)):
        (tmp_path / "odd.sam").write_text(text % value)
        assert sam.read_sam(str(tmp_path / "odd.sam"), record_filter=RecordFilter(min_mapq=25)).batch.flag.tolist() == [flag]
    (tmp_path / "ok.sam").write_text(text % "255")
    assert sam.read_sam(str(tmp_path / "ok.sam"), record_filter=RecordFilter(min_mapq=255)).batch.flag.tolist() == [0]
    (tmp_path / "star.sam").write_text("@SQ\tSN:c1\tLN:100\nr0\t0\tc1\t1\t30\t4M\t*\t0\t0\t*\t*\n")
    assert sam.read_sam(str(tmp_path / "star.sam"), record_filter=RecordFilter(min_length=1)).batch.flag.tolist() == [0x200]


@pytest.mark.parametrize("flt", FILTERS)
@pytest.mark.parametrize("name", ["in.bam", "straddle.bam"])
def test_native_host_decoder(files, flt, name, monkeypatch):
    """``mdx_bam_apply_record_filter`` over the one-piece decode and over every chunk of the streaming one."""
    monkeypatch.setenv("MDX_BAM_PARALLEL_SCAN_MIN", "0")
    path = str(files["dir"] / name)
    why = predicate(flt, files["flag16"], files["mapq"], files["lens"])
    plain = (files["flag16"] & 0x3FFF).astype(np.uint16)
    al = sam.read_bam_native(path)
    np.testing.assert_array_equal(al.batch.flag, plain)
    counts = sam.apply_record_filter(al, flt)
    np.testing.assert_array_equal(al.batch.flag, expect_flags(plain, why))
    np.testing.assert_array_equal(counts, expect_counts(why))
    # in chunks: the counts add up over the calls
    counts, flags = np.zeros(6, np.uint64), []
    with sam.BamStream(path, chunk_bytes=20000) as stream:
        for chunk in stream:
            sam.apply_record_filter(chunk, flt, counts)
            flags.append(chunk.batch.flag.copy())
    assert len(flags) > 3
    np.testing.assert_array_equal(np.concatenate(flags), expect_flags(plain, why))
    np.testing.assert_array_equal(counts, expect_counts(why))


def test_native_host_decoder_off_and_bad(files):
    import ctypes

    from mapdamage_amd.engine import load_library
    al = sam.read_bam_native(str(files["dir"] / "in.bam"))
    before = al.batch.flag.copy()
    counts = np.zeros(6, np.uint64)
    sam.apply_record_filter(al, RecordFilter(), counts)            # all zero: off
    sam.apply_record_filter(al, None, counts)                      # NULL: off
    np.testing.assert_array_equal(al.batch.flag, before)
    assert counts.tolist() == [2 * al.batch.n, 0, 0, 0, 0, 0]
    lib = load_library()
    for bad in ((256, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (0, 65536, 0, 0, 0), (0, 0, 65536, 0, 0), (0, 0, 0, -1, 0), (0, 0, 0, 9, 8)):
        flt = sam.MdxRecordFilter(*bad)
        assert lib.mdx_bam_apply_record_filter(al.native, ctypes.byref(flt), None) == -1
    np.testing.assert_array_equal(al.batch.flag, before)
    assert lib.mdx_bam_apply_record_filter(None, None, None) == -1


# ---------------------------------------------------------------------- reader.BAMReader: the host routes' batches
def passing_file(files, flt, tmp_path, kind):
    """The file that holds only the records that pass, in the same order (written by the same writer)."""
    why = predicate(flt, files["flag16"], files["mapq"], files["lens"])
    keep = np.nonzero(why < 0)[0]
    b, ref = files["batch"].take(keep), files["ref"]
    rg = [files["rg"][i] for i in keep]
    path = str(tmp_path / ("pass." + kind))
    (sam.write_bam if kind == "bam" else sam.write_sam)(path, b, ref.names, ref.lengths, RGS, rg, mapq=files["mapq"][keep])
    return path


def batches_equal(a, b):
    assert a.n == b.n
    for name in ("flag", "lib", "tid", "pos", "tlen", "cigar_off", "cigar", "seq_off", "seq", "qual"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name), err_msg=name)


@pytest.mark.parametrize("down", [None, 0.5, 100])
@pytest.mark.parametrize("kind,chunk", [("bam", 20000), ("bam", 0), ("sam", 0)])
def test_reader_is_the_reader_of_the_passing_file(files, tmp_path, kind, chunk, down):
    """Filters in front of the flag filter and of the draws: the same batches — the same --downsample draws — as the run
    without filters over the pre-filtered file; the counts are the predicate's."""
    from mapdamage_amd.reader import BAMReader
    flt = FILTERS[-1]
    why = predicate(flt, files["flag16"], files["mapq"], files["lens"])
    got = BAMReader(str(files["dir"] / ("in." + kind)), downsample_to=down, downsample_seed=3, chunk_bytes=chunk, record_filter=flt)
    want = BAMReader(passing_file(files, flt, tmp_path, kind), downsample_to=down, downsample_seed=3, chunk_bytes=chunk)
    a, b = concat_batches(list(got.iter_batches())), concat_batches(list(want.iter_batches()))
    assert 0 < a.n < files["batch"].n
    batches_equal(a, b)
    np.testing.assert_array_equal(got.filter_counts, expect_counts(why))
    assert not want.filter_counts.any()
    got.close(), want.close()


def test_a_dropped_record_without_read_group_is_no_error(files, tmp_path):
    from mapdamage_amd.reader import BAMReader
    ref, b = files["ref"], files["batch"].slice(0, 40)
    rg = list(files["rg"][:40])
    rg[3], rg[7] = None, "unlisted"
    mapq = np.full(40, 30)
    mapq[[3, 7]] = 2
    for kind, write in (("bam", sam.write_bam), ("sam", sam.write_sam)):
        path = str(tmp_path / ("rg." + kind))
        write(path, b, ref.names, ref.lengths, RGS, rg, mapq=mapq)
        with pytest.raises(sam.BAMError):
            list(BAMReader(path, chunk_bytes=1 << 20).iter_batches())
        reader = BAMReader(path, chunk_bytes=1 << 20, record_filter=RecordFilter(min_mapq=3))
        assert sum(x.n for x in reader.iter_batches()) == int(((b.flag & 0xF04) == 0).sum()) - int(((b.flag[[3, 7]] & 0xF04) == 0).sum())
        assert reader.filter_counts.tolist() == [40, 0, 0, 2, 0, 0]
        reader.close()


def test_the_host_filter_tests_the_files_bits_not_the_column(files):
    """A mark made in the column since the decode (--downsample's 0x200, the filter's own) is not the file's bit."""
    al = sam.read_bam_native(str(files["dir"] / "in.bam"))
    flt = RecordFilter(exclude_flags=0x200)
    want = predicate(flt, files["flag16"], files["mapq"], files["lens"])
    al.batch.flag[::3] |= 0x200
    counts = sam.apply_record_filter(al, flt)
    np.testing.assert_array_equal(counts, expect_counts(want))
    assert 0 < counts[2] < al.batch.n // 3


def test_reader_counts_a_one_piece_file_once(files):
    from mapdamage_amd.reader import BAMReader
    flt = FILTERS[0]
    want = expect_counts(predicate(flt, files["flag16"], files["mapq"], files["lens"]))
    reader = BAMReader(str(files["dir"] / "in.bam"), chunk_bytes=0, record_filter=flt)
    np.testing.assert_array_equal(reader.filter_counts, want)
    for _ in range(2):
        list(reader.iter_batches())
    np.testing.assert_array_equal(reader.filter_counts, want)
    reader.close()


def test_write_bam_mapq_forms(files, tmp_path):
    """One value; one per record of a single batch; with a list of batches — of one batch too — a list per batch."""
    import struct
    ref, b = files["ref"], files["batch"]
    parts = [b.slice(0, 40), b.slice(40, 100)]
    per = [np.arange(40) % 256, (7 * np.arange(60)) % 256]

    def mapqs(path):
        return [struct.unpack_from("<B", r, 9)[0] for r in sam.read_bam(str(path), keep_raw=True).raw]
    for workers in (1, 2):
        sam.write_bam(str(tmp_path / "one.bam"), [parts[0]], ref.names, ref.lengths, RGS, "rgA", workers=workers, mapq=[per[0]])
        assert mapqs(tmp_path / "one.bam") == per[0].tolist()
        sam.write_bam(str(tmp_path / "flat.bam"), parts[0], ref.names, ref.lengths, RGS, "rgA", workers=workers, mapq=per[0])
        assert mapqs(tmp_path / "flat.bam") == per[0].tolist()
        sam.write_bam(str(tmp_path / "value.bam"), [parts[0]], ref.names, ref.lengths, RGS, "rgA", workers=workers, mapq=7)
        assert mapqs(tmp_path / "value.bam") == [7] * 40
    sam.write_bam(str(tmp_path / "two.bam"), parts, ref.names, ref.lengths, RGS, "rgA", workers=2, mapq=per)
    assert mapqs(tmp_path / "two.bam") == per[0].tolist() + per[1].tolist()
    with pytest.raises(ValueError):
        sam.write_bam(str(tmp_path / "bad.bam"), parts, ref.names, ref.lengths, RGS, "rgA", workers=2, mapq=per[0])
    with pytest.raises(ValueError):
        sam.write_bam(str(tmp_path / "bad.bam"), parts[0], ref.names, ref.lengths, RGS, "rgA", mapq=per[1])


def test_writers_default_mapq_is_30(files, tmp_path):
    import struct
    ref, b = files["ref"], files["batch"].slice(0, 5)
    sam.write_sam(str(tmp_path / "a.sam"), b, ref.names, ref.lengths, RGS, files["rg"][:5])
    assert all(line.split("\t")[4] == "30" for line in (tmp_path / "a.sam").read_text().splitlines() if not line.startswith("@"))
    sam.write_bam(str(tmp_path / "a.bam"), b, ref.names, ref.lengths, RGS, files["rg"][:5])
    assert [struct.unpack_from("<B", r, 9)[0] for r in sam.read_bam(str(tmp_path / "a.bam"), keep_raw=True).raw] == [30] * 5
    sam.write_bam(str(tmp_path / "b.bam"), b, ref.names, ref.lengths, RGS, files["rg"][:5], mapq=[0, 1, 2, 255, 60])
    assert [struct.unpack_from("<B", r, 9)[0] for r in sam.read_bam(str(tmp_path / "b.bam"), keep_raw=True).raw] == [0, 1, 2, 255, 60]
