"""Record filters in the decoders (--min-mapq, --require-flags, --exclude-flags, --min-read-length, --max-read-length;
include/mdx.h ``mdx_record_filter``) on the GPU, through every input route of the command line.

The yardstick has two halves that share nothing with the product.  (1) The oracle over the batch with FLAG 0x4 set wherever
``dropped`` — a numpy predicate written here from the issue's table — says so: the reference's flag filter drops those
records, what is left is the filtered run.  (2) The command run WITHOUT filters on a file that holds only the passing
records, in the same order: the output files byte for byte, the log's warnings, the exit code.

The input (once per module): 20 000 reads over five sequences plus ``synth.make_edge_reads``, three libraries, qualities
on, MAPQ drawn from {0, 1, 24, 25, 29, 30, 37, 60, 255} (a stretch in the middle of the file from {0, 1, 24} only: whole slabs
that ``--min-mapq 25`` empties), extra flag bits 0x1, 0x10, 0x400, 0x800 and the file's bits 14 and 15, lengths 0 and 30..150,
records with ``SEQ *``; written as BAM in htslib's layout, BAM whose records straddle blocks, SAM text and bgzipped SAM.
The records with an unlisted read group, or none, live in a second, small file of the same kinds (``badrg.*``): no single
record can be dropped by --min-read-length alone and by --max-read-length alone, so a file that holds them cannot go through
"each filter alone" — that file goes through every route under the filters that do drop them."""

import ctypes
import dataclasses
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from mapdamage_amd import fasta, sam, synth
from mapdamage_amd.batch import batch_from_records, concat_batches
from tests.test_fasta_bgzf import _bgzip
from tests.test_gpu_pipe_input import _main_on_pipe
from tests.test_gpu_strata import MIXED, genome5
from tests.util import assert_tables_equal, oracle_tableset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 10
FILES = ("misincorporation.txt", "dnacomp.txt", "lgdistribution.txt")
RGS = [{"ID": "rgA", "SM": "s1", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s1", "LB": "lib2"}, {"ID": "c", "SM": "s2", "LB": "lib1"}]
LIBS = [("s1", "lib1"), ("s1", "lib2"), ("s2", "lib1")]
MAPQS = (0, 1, 24, 25, 29, 30, 37, 60, 255)
DEVICE = "Decode path: device; fallbacks from the device path: 0"

# name -> (min_mapq, require, exclude, min_length, max_length), and the command line's spelling (decimal and hex)
FILTERS = {"mapq": (25, 0, 0, 0, 0), "require": (0, 0x11, 0, 0, 0), "exclude": (0, 0, 0x8400, 0, 0), "shortest": (0, 0, 0, 35, 0),
           "longest": (0, 0, 0, 0, 100), "all": (25, 0x10, 0x400, 31, 140), "nothing": (0, 0, 0, 1000, 0)}
ARGS = {"mapq": ["--min-mapq", "25"], "require": ["--require-flags", "17"], "exclude": ["--exclude-flags", "0x8400"],
        "shortest": ["--min-read-length", "35"], "longest": ["--max-read-length", "100"],
        "all": ["--min-mapq", "25", "--require-flags", "0x10", "--exclude-flags", "1024", "--min-read-length", "31",
                "--max-read-length", "140"],
        "nothing": ["--min-read-length", "1000"]}
# route -> (the input's name, options, what the log says about the decode path)
ROUTES = {"bam": ("in.bam", [], DEVICE), "bam-straddle": ("straddle.bam", [], DEVICE), "bam-host": ("in.bam", ["--host-decode"], None),
          "bam-chunk0": ("in.bam", ["--chunk-mb", "0"], DEVICE), "bam-host-chunk0": ("in.bam", ["--host-decode", "--chunk-mb", "0"], None),
          "sam": ("in.sam", [], DEVICE), "sam-bgzf": ("in.sam.gz", [], DEVICE), "sam-host": ("in.sam", ["--host-decode"], None),
          "bam-pipe": ("in.bam", [], DEVICE)}


def dropped(name, flag16, mapq, l_seq):
    """The issue's table: the index of the first reason (require, exclude, MAPQ, shortest, longest) that drops each record,
    -1 for a record that passes."""
    q, req, exc, lo, hi = FILTERS[name]
    why = np.full(len(flag16), -1, np.int64)
    why[(l_seq > hi) & (hi > 0)] = 4
    why[l_seq < lo] = 3
    why[mapq < q] = 2
    why[(flag16 & exc) != 0] = 1
    why[(flag16 & req) != req] = 0
    return why


def counts_of(why):
    return [len(why)] + np.bincount(why[why >= 0], minlength=5).tolist()


def write_all(d, stem, batch, ref, rg, mapq):
    sam.write_bam(str(d / (stem + ".bam")), batch, ref.names, ref.lengths, RGS, rg, mapq=mapq)
    sam.write_sam(str(d / (stem + ".sam")), batch, ref.names, ref.lengths, RGS, rg, mapq=mapq)
    _bgzip(d / (stem + ".sam"), d / (stem + ".sam.gz"))


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("record_filters")
    ref = genome5()
    rng = np.random.default_rng(2025)
    mixed = synth.make_reads(ref, 20_000, 91, nlib=3, with_qual=True, **dict(MIXED, len_range=(30, 150)))
    nb = mixed.seq.shape[0]
    mixed.qual = np.where(rng.random(nb) < 0.05, rng.integers(2, 20, nb), rng.integers(20, 42, nb)).astype(np.uint8)
    edge = synth.make_edge_reads(ref, with_qual=True, nlib=3)
    # SEQ '*': as aligners write it, on secondary alignments and on unmapped records (which the reference's flag filter drops:
    # the filters still count them; a primary record with an M operation and no bases is one the reference cannot process)
    star = batch_from_records([dict(flag=0x100 if k % 4 else 0x4, lib=k % 3, tid=k % 5, pos=200 + k, cigar=[(0, 30)], seq="")
                               for k in range(24)], with_qual=True)
    b = concat_batches([mixed.slice(0, 12_000), edge, star, mixed.slice(12_000, 20_000)])
    n = b.n
    flag16 = b.flag.astype(np.int64)
    for bit in (0x1, 0x10, 0x400, 0x800, 0x4000, 0x8000):
        flag16 |= np.where(rng.random(n) < 0.1, bit, 0)
    mapq = rng.choice(MAPQS, n)
    mapq[5000:9000] = rng.choice(MAPQS[:3], 4000)
    lens = np.diff(b.seq_off.astype(np.int64))
    # the records without qualities (and those without bases, which have none either): MAPQ 0 — the -Q 20 cases choose
    # whether one of them is kept
    first = np.minimum(b.seq_off[:-1].astype(np.int64), b.seq.shape[0] - 1)
    noqual = (lens == 0) | (b.qual[first] == 0xFF)
    # (those the flag filter keeps stay kept: none of the drawn bits that --exclude-flags 0x8400 or the flag filter looks at)
    flag16[noqual & ((b.flag & 0xF04) == 0)] &= ~0x8C00
    assert 4 <= int((noqual & ((flag16 & 0xF04) == 0)).sum())
    mapq[noqual] = 0
    full = dataclasses.replace(b, flag=flag16.astype(np.uint16))
    rg = [RGS[int(i)]["ID"] for i in b.lib]
    write_all(d, "in", full, ref, rg, mapq)
    sam.write_bam(str(d / "straddle.bam"), full, ref.names, ref.lengths, RGS, rg, mapq=mapq, htslib_blocks=False, block_bytes=30_001)
    fasta.write_fasta(d / "ref.fa", ref)
    (d / "panel.bed").write_text("chr1\t100\t3000\nchr2\t0\t2000\nchrM\t500\t501\n")
    assert set(mapq.tolist()) == set(MAPQS) and (lens == 0).sum() == 24 and lens[lens > 0].min() <= 30 and lens.max() == 150
    # the file with the read groups no header lists: its first records and last ones, six bad ones among them
    k = 700
    small = full.slice(0, k)
    srg, smapq = list(rg[:k]), mapq[:k].copy()
    bad = [5, 130, 131, 400, 650, 699]
    for i, x in zip(bad, (None, "unlisted", None, "rgA ", None, "RGA")):
        srg[i] = x
    sflag = small.flag.copy()
    sflag[bad] = 0                        # (records the flag filter keeps, forward strand: no bit 0x10)
    smapq[bad] = [0, 1, 24, 0, 1, 24]
    small = dataclasses.replace(small, flag=sflag)
    write_all(d, "badrg", small, ref, srg, smapq)
    return dict(dir=d, ref=ref, batch=full, flag16=flag16, mapq=mapq, lens=lens, rg=rg, noqual=noqual,
                small=dict(batch=small, flag16=sflag.astype(np.int64), mapq=smapq, lens=lens[:k], rg=srg, bad=bad), passing={})


def why_of(data, name):
    return dropped(name, data["flag16"], data["mapq"], data["lens"])


def oracle_for(data, name, minqual=0, cache={}):
    """Half one: the oracle over the batch, the dropped records flagged unmapped."""
    if (name, minqual) not in cache:
        b = data["batch"]
        flag = (data["flag16"] & 0x3FFF).astype(np.uint16)
        if name is not None:
            flag[why_of(data, name) >= 0] |= 0x4
        cache[(name, minqual)] = oracle_tableset(data["ref"], dataclasses.replace(b, flag=flag), LIBS, 70, A, minqual)
    return cache[(name, minqual)]


def passing(data, name, stem="pass"):
    """Half two's input: the records that pass, in the same order, written by the same writers (once per filter)."""
    key = (name, stem)
    if key not in data["passing"]:
        keep = np.nonzero(why_of(data, name) < 0)[0]
        write_all(data["dir"], "%s_%s" % (stem, name), data["batch"].take(keep), data["ref"], [data["rg"][i] for i in keep],
                  data["mapq"][keep])
        data["passing"][key] = "%s_%s" % (stem, name)
    return data["passing"][key]


def run(data, out, source, *args, pipe=False, rc=0):
    from mapdamage_amd.main import main
    base = ["-r", str(data["dir"] / "ref.fa"), "-d", str(out), "--log-level", "DEBUG"] + [str(a) for a in args]
    if "--stats" not in base:
        base.append("--no-stats")
    if pipe:
        assert _main_on_pipe(out.parent, (data["dir"] / source).read_bytes(), base, "fifo", seed=zlib.crc32(out.name.encode()) % 10_000) == rc
    else:
        assert main(["-i", str(data["dir"] / source)] + base) == rc
    return out


def tables(out):
    return [(out / f).read_text() for f in FILES]


def warnings(out):
    """The log's WARNING and ERROR lines without their time stamps."""
    return [line.split(" ", 1)[1] for line in (out / "Runtime_log.txt").read_text().splitlines()
            if " WARNING " in line or " ERROR " in line]


def tsv_counts(out):
    rows = [line.split("\t") for line in (out / "record_filters.tsv").read_text().splitlines()[1:]]
    by = {r[0]: int(r[2]) for r in rows}
    return [by["records-read"], by["require-flags"], by["exclude-flags"], by["min-mapq"], by["min-read-length"], by["max-read-length"]]


def check_against_oracle(out, want):
    assert (out / "misincorporation.txt").read_text() == want.misincorporation_text()
    assert (out / "dnacomp.txt").read_text() == want.dnacomp_text()
    assert (out / "lgdistribution.txt").read_text() == want.lgdistribution_text()


def source_of(route, stem):
    """The input of ``route`` among the files written as ``stem``.* (the routes that read in.*)."""
    name = ROUTES[route][0]
    assert name.startswith("in.")
    return stem + name[2:]


# ---------------------------------------------------------------------- 1. each filter alone and all five, on every route
@pytest.fixture(scope="module")
def prefiltered(data, tmp_path_factory):
    """The run without filters over the passing file of each filter (from BAM on the device path), once."""
    done = {}

    def get(name):
        if name not in done:
            out = tmp_path_factory.mktemp("want_" + name) / "out"
            done[name] = run(data, out, passing(data, name) + ".bam")
            assert not (out / "record_filters.tsv").exists()
            assert "Record filters" not in (out / "Runtime_log.txt").read_text()
        return done[name]
    return get


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["mapq", "require", "exclude", "shortest", "longest", "all"])
def test_every_route(data, prefiltered, tmp_path, name, route):
    source, opts, says = ROUTES[route]
    why = why_of(data, name)
    assert (why >= 0).sum() > 500 and (why < 0).sum() > 500
    out = run(data, tmp_path / "out", source, *opts, *ARGS[name], pipe=route == "bam-pipe")
    log = (out / "Runtime_log.txt").read_text()
    # (a run with --host-decode has no decode path to report)
    assert (says in log if says else "Decode path" not in log) and "gave up" not in log, route
    want = oracle_for(data, name)
    assert 0 < want.n_kept < oracle_for(data, None).n_kept
    check_against_oracle(out, want)
    pre = prefiltered(name)
    assert tables(out) == tables(pre)
    assert warnings(out) == warnings(pre)
    assert tsv_counts(out) == counts_of(why)
    q, _, _, lo, hi = FILTERS[name]
    c = counts_of(why)
    assert ("Record filters: %d records read; dropped: %d require-flags, %d exclude-flags, %d MAPQ < %d, %d shorter than %d, "
            "%d longer than %d" % (c[0], c[1], c[2], c[3], q, c[4], lo, c[5], hi)) in log
    if name == "all":
        assert all(x > 0 for x in c[1:])


def test_no_filter_no_change(data, tmp_path):
    out = run(data, tmp_path / "out", "in.bam")
    check_against_oracle(out, oracle_for(data, None))
    assert not (out / "record_filters.tsv").exists() and "Record filters" not in (out / "Runtime_log.txt").read_text()
    # zeros are no filters either
    out = run(data, tmp_path / "zero", "in.sam", "--min-mapq", "0", "--exclude-flags", "0x0", "--max-read-length", "0")
    check_against_oracle(out, oracle_for(data, None))
    assert not (out / "record_filters.tsv").exists()


# ---------------------------------------------------------------------- 2. tables bit for bit, slab by slab, through the streams
@pytest.mark.parametrize("source", ["in.bam", "straddle.bam", "in.sam", "in.sam.gz"])
@pytest.mark.parametrize("name", ["mapq", "all"])
def test_streams_tables_bit_for_bit(data, name, source):
    """``GpuBamStream`` / ``GpuSamStream`` with ``record_filter=`` in slabs of 64 KiB: every view's flag column has 0x200
    exactly on the predicate's records, --min-mapq 25 empties whole slabs, the tables are the oracle's, the counts the
    predicate's."""
    from mapdamage_amd.engine import DamageEngine
    flt = sam.RecordFilter(*FILTERS[name])
    why = why_of(data, name)
    Stream = sam.GpuBamStream if source.endswith(".bam") else sam.GpuSamStream
    rgs = [(rg["ID"], LIBS.index((rg["SM"], rg["LB"]))) for rg in RGS]
    flags, emptied = [], 0
    with DamageEngine(LIBS, 70, A, 0) as eng:
        eng.set_reference(data["ref"])
        with Stream(eng, str(data["dir"] / source), readgroups=rgs, chunk_bytes=65536, record_filter=flt) as stream:
            while True:
                view = stream.next_view()
                if view is None:
                    break
                f = stream.view_flags(view)
                flags.append(f)
                emptied += int(len(f) > 0 and bool(((f & 0x200) != 0).all()))
                eng.tabulate_view(view)
                eng.sync()
            counts = stream.filter_counts()
        got = eng.finish()
    assert len(flags) > 8
    np.testing.assert_array_equal(np.concatenate(flags) & 0x3FFF, np.where(why >= 0, (data["flag16"] & 0x3FFF) | 0x200, data["flag16"] & 0x3FFF))
    assert emptied >= 1
    assert counts.tolist() == counts_of(why)
    assert_tables_equal(got, oracle_for(data, name))


# ---------------------------------------------------------------------- 3. slab shapes
@pytest.mark.parametrize("route", ["bam", "bam-straddle", "sam", "sam-bgzf", "bam-pipe"])
def test_many_slabs_one_of_them_emptied(data, prefiltered, tmp_path, route, monkeypatch):
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    source, opts, says = ROUTES[route]
    out = run(data, tmp_path / "out", source, *opts, *ARGS["mapq"], pipe=route == "bam-pipe")
    assert says in (out / "Runtime_log.txt").read_text()
    check_against_oracle(out, oracle_for(data, "mapq"))
    assert tables(out) == tables(prefiltered("mapq"))
    assert tsv_counts(out) == counts_of(why_of(data, "mapq"))


@pytest.mark.parametrize("route", list(ROUTES))
def test_everything_dropped(data, tmp_path, route, monkeypatch):
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    source, opts, _ = ROUTES[route]
    out = run(data, tmp_path / "out", source, *opts, *ARGS["nothing"], pipe=route == "bam-pipe")
    want = oracle_for(data, "nothing")
    assert want.n_kept == 0 and not want.mis.any() and not want.comp.any() and not want.lgd.any()
    check_against_oracle(out, want)
    n = data["batch"].n
    assert tsv_counts(out) == [n, 0, 0, 0, n, 0]


# ---------------------------------------------------------------------- 4. -Q 20
@pytest.mark.parametrize("route", ["bam", "bam-host", "sam", "sam-bgzf", "sam-host", "bam-pipe"])
def test_min_basequal_and_its_warning(data, tmp_path, route):
    """Every record without qualities has MAPQ 0: under --min-mapq 1 the only ones are dropped ones and the warning stays
    away; under --exclude-flags alone one is kept and the warning comes."""
    source, opts, _ = ROUTES[route]
    text = "Reads without PHRED scores found; cannot filter by --min-basequal"
    quiet = run(data, tmp_path / "quiet", source, *opts, "-Q", "20", "--min-mapq", "1", pipe=route == "bam-pipe")
    why = np.where(data["mapq"] < 1, 2, -1)
    assert (why[data["noqual"]] >= 0).all()
    flag = (data["flag16"] & 0x3FFF).astype(np.uint16)
    flag[why >= 0] |= 0x4
    check_against_oracle(quiet, oracle_tableset(data["ref"], dataclasses.replace(data["batch"], flag=flag), LIBS, 70, A, 20))
    assert text not in (quiet / "Runtime_log.txt").read_text()
    assert tsv_counts(quiet) == counts_of(why)
    loud = run(data, tmp_path / "loud", source, *opts, "-Q", "20", *ARGS["exclude"], pipe=route == "bam-pipe")
    kept = (why_of(data, "exclude") < 0) & ((data["flag16"] & 0xF04) == 0)
    assert (kept & data["noqual"]).any()
    check_against_oracle(loud, oracle_for(data, "exclude", 20))
    assert (loud / "Runtime_log.txt").read_text().count(text) == 1


# ---------------------------------------------------------------------- 5. draw parity
@pytest.mark.parametrize("route", ["bam", "bam-host", "bam-host-chunk0", "sam", "sam-host", "bam-pipe"])
def test_downsample_fraction_draws_once_per_kept_record(data, tmp_path, route, monkeypatch):
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    source, opts, _ = ROUTES[route]
    down = ["--downsample", "0.5", "--downsample-seed", "3"]
    got = run(data, tmp_path / "got", source, *opts, *down, *ARGS["all"], pipe=route == "bam-pipe")
    want = run(data, tmp_path / "want", source_of(route, passing(data, "all")), *opts, *down, pipe=route == "bam-pipe")
    assert tables(got) == tables(want)
    assert tables(got) != tables(run(data, tmp_path / "plain", source, *opts, *ARGS["all"], pipe=route == "bam-pipe"))
    assert warnings(got) == warnings(want)
    assert tsv_counts(got) == counts_of(why_of(data, "all"))


@pytest.mark.parametrize("source", ["in.bam", "in.sam"])
def test_downsample_to_a_number(data, tmp_path, source):
    down = ["-n", "500", "--downsample-seed", "3"]
    got = run(data, tmp_path / "got", source, *down, *ARGS["all"])
    want = run(data, tmp_path / "want", passing(data, "all") + source[source.index("."):], *down)
    assert tables(got) == tables(want)
    assert tsv_counts(got) == counts_of(why_of(data, "all"))


# ---------------------------------------------------------------------- 6. --regions, --by-reference, --stats
def tree(folder):
    return {str(p.relative_to(folder)): p.read_text() for p in sorted(folder.rglob("*")) if p.is_file()}


@pytest.mark.parametrize("route", ["bam", "bam-host", "sam"])
def test_regions_and_by_reference(data, tmp_path, route):
    source, opts, _ = ROUTES[route]
    for sub, extra in (("by_region", ["--regions", data["dir"] / "panel.bed"]), ("by_reference", ["--by-reference"])):
        got = run(data, tmp_path / ("got_" + sub), source, *opts, *extra, *ARGS["all"])
        want = run(data, tmp_path / ("want_" + sub), source_of(route, passing(data, "all")), *opts, *extra)
        assert tree(got / sub) == tree(want / sub) and "groups.tsv" in tree(got / sub)
        assert tables(got) == tables(want)
        if sub == "by_region":
            kept = [int(line.split("\t")[-1]) for line in (got / sub / "groups.tsv").read_text().splitlines()[1:]]
            assert sum(kept) == oracle_for(data, "all").n_kept


def test_stats_files_for_a_seed(data, tmp_path):
    fast = ["--stats", "--fix-nicks", "--rand", "4", "--adjust", "2", "--burn", "100", "--iter", "200", "--stats-seed", "9"]
    got = run(data, tmp_path / "got", "in.bam", *fast, *ARGS["mapq"])
    want = run(data, tmp_path / "want", passing(data, "mapq") + ".bam", *fast)
    names = sorted(p.name for p in want.iterdir() if p.name.startswith("Stats_out"))
    assert len(names) >= 3
    for name in names:
        assert (got / name).read_bytes() == (want / name).read_bytes(), name
    assert tables(got) == tables(want)


# ---------------------------------------------------------------------- 7. dropped records are never an error
@pytest.mark.parametrize("route", [r for r in ROUTES if r != "bam-straddle"])
def test_a_dropped_record_with_a_bad_read_group_is_no_error(data, tmp_path, route, monkeypatch):
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    source, opts, _ = ROUTES[route]
    source = source_of(route, "badrg")
    s = data["small"]
    pipe = route == "bam-pipe"
    from mapdamage_amd.sam import BAMError
    if not pipe:
        with pytest.raises(BAMError, match="read-group"):       # (without filters the file is the reference's error)
            run(data, tmp_path / "plain", source, *opts)
    for name in ("mapq", "all"):
        why = dropped(name, s["flag16"], s["mapq"], s["lens"])
        assert (why[s["bad"]] >= 0).all()
        out = run(data, tmp_path / name, source, *opts, *ARGS[name], pipe=pipe)
        flag = (s["flag16"] & 0x3FFF).astype(np.uint16)
        flag[why >= 0] |= 0x4
        lib = s["batch"].lib.copy()
        check_against_oracle(out, oracle_tableset(data["ref"], dataclasses.replace(s["batch"], flag=flag, lib=lib), LIBS, 70, A, 0))
        assert tsv_counts(out) == counts_of(why)


# ---------------------------------------------------------------------- 8. the device path gives up part of the way
def test_fallback_mid_file_counts_once(data, tmp_path, monkeypatch):
    """A line whose MAPQ is 1000 — a number, but none the device parser takes — late in the file: from a file the host reads
    the whole file again and the counts start again; from a pipe it takes over at that slab and the counts of the slabs in
    front are carried.  Either way the tables and the counts are the host-only run's."""
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    d = data["dir"]
    lines = (d / "in.sam").read_text().splitlines(keepends=True)
    head = sum(1 for x in lines if x.startswith("@"))
    at = head + 15_000
    f = lines[at].split("\t")
    assert int(f[1]) & 0xF04 == 0
    f[4] = "1000"
    lines[at] = "\t".join(f)
    (d / "odd.sam").write_text("".join(lines))
    mapq = data["mapq"].copy()
    mapq[15_000] = 1000
    why = dropped("mapq", data["flag16"], mapq, data["lens"])
    host = run(data, tmp_path / "host", "odd.sam", "--host-decode", *ARGS["mapq"])
    assert tsv_counts(host) == counts_of(why)
    flag = (data["flag16"] & 0x3FFF).astype(np.uint16)
    flag[why >= 0] |= 0x4
    check_against_oracle(host, oracle_tableset(data["ref"], dataclasses.replace(data["batch"], flag=flag), LIBS, 70, A, 0))
    for name, pipe in (("file", False), ("pipe", True)):
        out = run(data, tmp_path / name, "odd.sam", *ARGS["mapq"], pipe=pipe)
        log = (out / "Runtime_log.txt").read_text()
        assert log.count("GPU decode path gave up") == 1 and "MAPQ is not 1-3 digits" in log, name
        assert ("records are counted" in log) if pipe else ("the whole file again" in log)
        assert tables(out) == tables(host), name
        assert tsv_counts(out) == counts_of(why), name


# ---------------------------------------------------------------------- 9. two ranks
@pytest.mark.parametrize("decode", ["--gpu-decode", "--host-decode"])
def test_two_ranks_sum_the_counts_once(data, tmp_path, decode):
    d = data["dir"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="1", MDX_GBAM_SLAB_BYTES="65536")
    out = tmp_path / "two"
    cmd = [sys.executable, "-m", "mapdamage_amd", "-i", str(d / "in.bam"), "-r", str(d / "ref.fa"), "-d", str(out), "--no-stats",
           "--log-level", "DEBUG", decode, "--gpus", "2", "--share-gpu", "--dist-backend", "gloo"] + ARGS["all"]
    done = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-6000:]
    check_against_oracle(out, oracle_for(data, "all"))
    assert tsv_counts(out) == counts_of(why_of(data, "all"))
    if decode == "--gpu-decode":
        assert DEVICE in (out / "Runtime_log.txt").read_text()


# ---------------------------------------------------------------------- 10. the C ABI, without the command line
def test_c_abi(data):
    from mapdamage_amd.engine import DamageEngine, MdxBatch
    why = why_of(data, "all")
    flt = sam.MdxRecordFilter(*FILTERS["all"])
    with DamageEngine(LIBS, 70, A, 0) as eng:
        lib, g = eng._lib, ctypes.c_void_p()
        assert lib.mdx_gbam_open(eng._ctx, str(data["dir"] / "in.bam").encode(), ctypes.byref(g)) == 0
        try:
            ids = (ctypes.c_char_p * 3)(*[rg["ID"].encode() for rg in RGS])
            libs = (ctypes.c_int32 * 3)(0, 1, 2)
            assert lib.mdx_gbam_configure(g, 3, ids, libs, -1, 0, 0) == 0
            for bad in ((256, 0, 0, 0, 0), (0, 65536, 0, 0, 0), (0, 0, 0, 50, 49), (0, 0, 0, -1, 0)):
                assert lib.mdx_gbam_set_record_filter(g, ctypes.byref(sam.MdxRecordFilter(*bad))) == -1
            assert lib.mdx_gbam_set_record_filter(g, ctypes.byref(sam.MdxRecordFilter(*FILTERS["mapq"]))) == 0
            assert lib.mdx_gbam_set_record_filter(g, None) == 0                     # off again
            assert lib.mdx_gbam_set_record_filter(g, ctypes.byref(flt)) == 0        # any time before the first slab
            flags = []
            while True:
                view = MdxBatch()
                assert lib.mdx_gbam_next(g, 1 << 18, ctypes.byref(view), None, None) == 0
                if view.n_reads == 0 and lib.mdx_gbam_at_end(g):
                    break
                f = np.empty(int(view.n_reads), np.uint16)
                assert lib.mdx_gbam_view_flags(g, ctypes.c_void_p(f.ctypes.data), ctypes.c_int64(f.shape[0])) == 0
                flags.append(f)
                assert lib.mdx_gbam_set_record_filter(g, ctypes.byref(flt)) == -3    # MDX_ERR_STATE behind the first slab
            got = np.concatenate(flags)
            assert len(flags) > 2
            np.testing.assert_array_equal((got & 0x200) != 0, (why >= 0) | ((data["flag16"] & 0x200) != 0))
            np.testing.assert_array_equal(got & 0x3DFF, data["flag16"] & 0x3DFF)
            counts = np.zeros(6, np.uint64)
            assert lib.mdx_gbam_filter_counts(g, ctypes.c_void_p(counts.ctypes.data)) == 0
            assert counts.tolist() == counts_of(why)
        finally:
            lib.mdx_gbam_close(g)
