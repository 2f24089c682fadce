"""--pileup-sites on the device (mapdamage_amd/csrc/mdx_pileup.hip): the counters, the reference's letters, the depths and the
calls of ``pileup_finish`` over small BAM files against the brute force of tests/pileup_rule.py — the hand-written table, dense
sites where the add kernel's list turns, sparse sites, contention, record counts around the block size, one slab and many,
marked flags, the state rules —, and the command line's files against the rule's.  The rule on the host, the parser and the
emitters: tests/test_pileup.py."""

import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from mapdamage_amd import sam
from tests import pileup_rule as PR
from tests.test_gpu_depth import names_of, raw_header, reference
from tests.test_gpu_remove_duplicates import LIBS3, RG3, dup_data      # noqa: F401  (dup_data: a fixture)
from tests.test_gpu_write_kept import DEVICE, FILES, read_bam_file, run, tables
from tests.test_pileup import HAND_LENGTHS, HAND_LIBRARIES, HAND_RECORDS, HAND_SETTINGS, HAND_SITES, rec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D, N, S, H, P, EQ, X = range(9)
ERR_ARG, ERR_STATE = -1, -3
NIBBLES = "=ACMGRSVTWYHKDBN"


# ---------------------------------------------------------------------- files, sites, results
def body(record, rg, salt):
    """A BAM record without its block_size from a record of the rule, an RG:Z tag for ``rg``."""
    flag, _, tid, pos, cigar, seq, qual = record
    n = len(seq)
    nib = [NIBBLES.index(c) for c in seq] + [0]
    name = b"r%d" % salt
    out = struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, 60, 4680, len(cigar), flag, n, -1, -1, 0)
    out += name + b"\0" + b"".join(struct.pack("<I", ln << 4 | op) for op, ln in cigar)
    out += bytes(nib[i] << 4 | nib[i + 1] for i in range(0, n, 2)) + (bytes(qual) if qual is not None else b"\xff" * n)
    return out + b"RGZ" + rg.encode() + b"\0"


def write_records(path, records, names, lengths):
    """``records`` of the rule in file order; a library beyond the three gets a read group nobody knows."""
    sam.write_bam_raw(str(path), raw_header(names, lengths), [body(r, RG3[r[1]] if r[1] < 3 else "zz", i) for i, r in enumerate(records)])


def site_columns(sites, n_contig):
    off = np.zeros(n_contig + 1, np.int64)
    off[1:] = np.cumsum(np.bincount([t for t, _ in sites], minlength=n_contig)) if sites else 0
    return np.array([p for _, p in sites], np.int32), off


def begin(eng, lengths, sites, alleles=None, ref=None, **options):
    """The reference of these lengths resident, the sites and their zeroed counters beside it."""
    ref = reference(lengths) if ref is None else ref
    eng.set_reference(ref)
    pos, off = site_columns(sites, len(lengths))
    eng.pileup_begin(pos, off, None if alleles is None else np.array([[PR.BASES.index(a) for a in pair] for pair in alleles], np.uint8), **options)
    return ref


def add_file(eng, path, chunk_bytes=256 << 20, before=None, want_qual=True, packed=True, min_basequal=0):
    """Every slab of the file through ``pileup_add``; ``before(stream, view, first record)`` runs in front of each add.  -> the slabs' sizes."""
    slabs = []
    with sam.GpuBamStream(eng, str(path), readgroups=[(rg, i) for i, rg in enumerate(RG3)], chunk_bytes=chunk_bytes, want_qual=want_qual, packed=packed,
                          min_basequal=min_basequal) as stream:
        while True:
            view = stream.next_view()
            if view is None:
                break
            if before is not None:
                before(stream, view, sum(slabs))
            eng.pileup_add(view)
            slabs.append(int(view.n_reads))
        eng.sync()
    return slabs


def check(got, records, lengths, sites, ref, n_libraries=3, k5=0, k3=0, min_qual=0, fold_q=0, mode="random", seed=0, min_depth=1, alleles=None,
          single_strand=False):
    counters, refbase, call, depth, counts = got
    want, want_counts = PR.brute(records, n_libraries, lengths, sites, k5, k3, min_qual, fold_q)
    assert counters.shape == want.shape and counters.dtype == np.uint32
    assert (counters == want).all(), [(sites[g], counters[g].tolist(), want[g].tolist()) for g in np.flatnonzero((counters != want).any(axis=1))[:5]]
    assert counts == want_counts, (counts, want_counts)
    assert (depth == PR.depths(want)).all() and depth.dtype == np.uint32
    assert refbase.astype("U1").tolist() == PR.refbases(ref.seqs, sites)
    assert call.astype("U1").tolist() == PR.calls(want, sites, mode, seed, min_depth, alleles, single_strand)
    return want, want_counts


def spread(n, lengths, seed, n_libraries=3):
    """``n`` records over the sequences, a few shapes of CIGAR, some at either end of their sequence, one of twenty not counted,
    one of ten without qualities, symbols that are no base and low qualities among the rest."""
    rng = np.random.default_rng(seed)
    placed = [t for t, length in enumerate(lengths) if length >= 80]
    out = []
    for i in range(n):
        t = placed[int(rng.integers(0, len(placed)))]
        cigar = [[(M, 50)], [(M, 20), (D, 5), (M, 20)], [(S, 5), (M, 30), (I, 2), (EQ, 30)], [(M, 10), (N, 30), (X, 1), (M, 9)], [(M, 1)],
                 [(H, 2), (S, 1), (M, 12), (S, 3)]][int(rng.integers(0, 6))]
        span = sum(ln for op, ln in cigar if op in (M, D, N, EQ, X))
        n_seq = sum(ln for op, ln in cigar if op in (M, I, S, EQ, X))
        where = rng.random()
        pos = 0 if where < 0.05 else lengths[t] - span if where < 0.1 else int(rng.integers(0, lengths[t] - span + 1))
        flag = int(rng.choice((0, 0x10))) | (int(rng.choice((0x4, 0x400, 0x200, 0x100))) if rng.random() < 0.05 else 0)
        seq = "".join(rng.choice(list("ACGT" * 6 + "NR"), n_seq))
        qual = None if rng.random() < 0.1 else [int(x) for x in rng.choice((2, 19, 20, 21, 30, 41), n_seq)]
        out.append((flag, i % n_libraries, t, pos, cigar, seq, qual))
    return out


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(LIBS3) as eng:
        yield eng


@pytest.fixture(scope="module")
def turns(engine):
    """The pairs the add kernel's list holds and the records a block of it takes, as the library tells them (``mdx_pileup_info``)."""
    begin(engine, [100], [(0, 5)])
    info = engine.pileup_info()
    assert 64 <= info["block_records"] <= 1024 and 64 <= info["list_pairs"] <= 1 << 16 and info["sites"] == 1 and info["bytes"] >= 48
    return dict(block=info["block_records"], list=info["list_pairs"])


# ---------------------------------------------------------------------- 1. the rule on the device
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "ascii"])
def test_hand_written_records_on_the_device(engine, tmp_path, packed):
    """The CPU test's table as a file, in one slab.  Its header names one sequence more than the reference holds, so that a record
    can carry tid = n_contig."""
    write_records(tmp_path / "in.bam", HAND_RECORDS, names_of(HAND_LENGTHS + [50]), HAND_LENGTHS + [50])
    alleles = [("CT", "GA", "AC", "TG")[g % 4] for g in range(len(HAND_SITES))]
    for n, (k5, k3, q) in enumerate(HAND_SETTINGS):
        options = dict(mode=("random", "majority", "none")[n % 3], seed=n, min_depth=1 + n % 2, single_strand=bool(n % 2))
        ref = begin(engine, HAND_LENGTHS, HAND_SITES, alleles, min_basequal=q, mask_ends=(k5, k3), call=options["mode"], seed=n,
                    min_depth=options["min_depth"], single_strand=options["single_strand"])
        assert add_file(engine, tmp_path / "in.bam", packed=packed) == [len(HAND_RECORDS)]
        check(engine.pileup_finish(), HAND_RECORDS, HAND_LENGTHS, HAND_SITES, ref, HAND_LIBRARIES, k5, k3, q, alleles=alleles, **options)


def test_a_column_with_the_quality_mask_folded_in(tmp_path):
    """An engine with --min-basequal 20 hands MDX_SEQ_4BITQ columns over: a base below 20 is a complemented nibble, so Other."""
    from mapdamage_amd.engine import DamageEngine
    write_records(tmp_path / "in.bam", HAND_RECORDS, names_of(HAND_LENGTHS + [50]), HAND_LENGTHS + [50])
    with DamageEngine(LIBS3, minqual=20) as eng:
        ref = begin(eng, HAND_LENGTHS, HAND_SITES, min_basequal=20, mask_ends=(1, 1))
        add_file(eng, tmp_path / "in.bam", packed=True, min_basequal=20)
        want, _ = check(eng.pileup_finish(), HAND_RECORDS, HAND_LENGTHS, HAND_SITES, ref, HAND_LIBRARIES, 1, 1, 20, fold_q=20)
    # (Other: the N at 406, the R at 408 and the quality 19 at 396; the = at 410 and the qualities 19 and 0 at 395 and 398 are Masked)
    assert want[:, PR.LOWQUAL].sum() == 0 and want[:, PR.OTHER].sum() == 3


# ---------------------------------------------------------------------- 2. dense sites: the list's rounds
DENSE_LENGTHS = [300, 40]           # (the records all lie on the first: `spread` places none on a sequence below 80 bases)
DENSE_SITES = [(0, p) for p in range(300)]


def dense_records():
    return spread(2000, DENSE_LENGTHS, 77)


def exact_records(pairs):
    """Records of one block over DENSE_SITES with ``pairs`` (record, site) pairs in all: M 1 records, the last one longer."""
    assert 2 <= pairs <= 290 + 200
    if pairs <= 200:
        return [rec(0x10 * (i % 2), i % 3, 0, i, [(M, 1)]) for i in range(pairs)]
    return [rec(0x10 * (i % 2), i % 3, 0, i, [(M, 1)]) for i in range(199)] + [rec(0, 1, 0, 5, [(M, 3), (D, 2), (M, pairs - 199 - 5)])]


@pytest.fixture(scope="module")
def small_list(tmp_path_factory):
    """A child process whose add kernel's list holds 48 pairs (MDX_TEST_PILEUP_LIST is read at ``pileup_begin``): the dense file,
    a block whose pairs fill the list exactly, one pair more, and one record alone with more pairs than the list."""
    d = tmp_path_factory.mktemp("pileup_list")
    cases = {"dense": dense_records(), "exact": exact_records(48), "over": exact_records(49), "twice": exact_records(96), "alone": [rec(0x10, 0, 0, 20, [(M, 250)])],
             "alone_among": exact_records(20) + [rec(0, 2, 0, 0, [(M, 150), (N, 20), (M, 130)])] + exact_records(30)}
    for name, records in cases.items():
        write_records(d / (name + ".bam"), records, names_of(DENSE_LENGTHS), DENSE_LENGTHS)
    done = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_pileup_worker.py"), str(d)] + sorted(cases), cwd=ROOT,
                          env=dict(os.environ, PYTHONPATH=ROOT, MDX_TEST_PILEUP_LIST="48"), capture_output=True, timeout=300)
    assert done.returncode == 0, done.stderr.decode()[-3000:]
    return d, cases


@pytest.mark.parametrize("case", ["dense", "exact", "over", "twice", "alone", "alone_among"])
def test_pairs_where_the_list_turns(small_list, case):
    d, cases = small_list
    z = np.load(d / (case + ".npz"))
    assert int(z["info"][0]) == 48
    counts = dict(zip(("counted", "outside", "over_a_site", "pairs"), (int(x) for x in z["counts"])))
    _, want_counts = check((z["counters"], z["refbase"], z["call"], z["depth"], counts), cases[case], DENSE_LENGTHS, DENSE_SITES, reference(DENSE_LENGTHS),
                           k5=2, k3=1, min_qual=20, mode="majority", seed=3)
    assert want_counts["pairs"] == {"exact": 48, "over": 49, "twice": 96, "alone": 250}.get(case, want_counts["pairs"])
    assert case != "dense" or want_counts["pairs"] > 40_000


def test_dense_sites_with_the_whole_list(engine, turns, tmp_path):
    records = dense_records()
    write_records(tmp_path / "in.bam", records, names_of(DENSE_LENGTHS), DENSE_LENGTHS)
    ref = begin(engine, DENSE_LENGTHS, DENSE_SITES, min_basequal=20, mask_ends=(2, 1), call="majority", seed=3)
    assert add_file(engine, tmp_path / "in.bam") == [2000]
    _, counts = check(engine.pileup_finish(), records, DENSE_LENGTHS, DENSE_SITES, ref, k5=2, k3=1, min_qual=20, mode="majority", seed=3)
    # (a block's 256 records bring more pairs than the list holds: several rounds with the list as it is built, too)
    assert counts["pairs"] * turns["block"] / 2000 > turns["list"]


# ---------------------------------------------------------------------- 3. sparse sites
def test_sites_on_one_sequence_of_four(engine, tmp_path):
    lengths = [400, 90, 600, 200]
    sites = [(2, p) for p in (0, 7, 8, 150, 151, 300, 598, 599)]
    records = spread(1500, lengths, 21) + [rec(0, 0, 2, 0, [(M, 1)]), rec(0x10, 1, 2, 599, [(M, 1)]), rec(0, 2, 3, 0, [(M, 200)]), rec(0, 2, 1, 0, [(M, 90)])]
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    ref = begin(engine, lengths, sites)
    add_file(engine, tmp_path / "in.bam")
    want, counts = check(engine.pileup_finish(), records, lengths, sites, ref)
    assert 0 < counts["over_a_site"] < counts["counted"] / 2 and (PR.depths(want) > 0).all()
    assert len({r[2] for r in records}) == 4


# ---------------------------------------------------------------------- 4. contention
def test_three_thousand_records_over_one_site(engine, tmp_path):
    lengths = [500]
    records = [rec(0x10 * (i % 2), i % 3, 0, 100 + i % 7, [(M, 10)], "ACGTACGTAC") for i in range(3000)]
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    ref = begin(engine, lengths, [(0, 108)], call="majority")
    add_file(engine, tmp_path / "in.bam")
    want, counts = check(engine.pileup_finish(), records, lengths, [(0, 108)], ref, mode="majority")
    assert counts["pairs"] == 3000 and int(want[0, :4].sum()) == 1500 and int(want[0, 4:8].sum()) == 1500


# ---------------------------------------------------------------------- 5. record counts around the block size
@pytest.mark.parametrize("size", ["1", "63", "64", "65", "block-1", "block", "block+1", "2*block+1"])
def test_record_counts_where_the_add_kernel_turns(engine, turns, tmp_path, size):
    n = int(eval(size, {"__builtins__": {}}, dict(turns)))
    lengths = [900, 500]
    sites = sorted({(0, p) for p in range(0, 900, 7)} | {(1, p) for p in range(3, 500, 11)} | {(1, 499)})
    records = spread(n, lengths, 100 + n)
    records[-1] = rec(0, 0, 1, 450, [(M, 50)])                  # (the last lane's record lies over a site, whatever chance gave)
    write_records(tmp_path / "in.bam", records, names_of(lengths), lengths)
    ref = begin(engine, lengths, sites, min_basequal=20, mask_ends=(1, 1))
    assert add_file(engine, tmp_path / "in.bam") == [n]
    _, counts = check(engine.pileup_finish(), records, lengths, sites, ref, k5=1, k3=1, min_qual=20)
    assert counts["over_a_site"] >= 1


# ---------------------------------------------------------------------- 6. slabs, flags, state
@pytest.fixture(scope="module")
def clustered(tmp_path_factory):
    lengths = [3000, 1, 1200]
    records = spread(12_000, lengths, 41)
    rng = np.random.default_rng(4)
    sites = sorted({(0, int(p)) for p in rng.choice(3000, 400, replace=False)} | {(1, 0)} | {(2, p) for p in range(100, 400)})
    d = tmp_path_factory.mktemp("pileup_clustered")
    write_records(d / "in.bam", records, names_of(lengths), lengths)
    return dict(dir=d, records=records, lengths=lengths, sites=sites)


def test_one_slab_and_many(engine, clustered):
    lengths, records, sites = clustered["lengths"], clustered["records"], clustered["sites"]
    ref = begin(engine, lengths, sites, min_basequal=21, mask_ends=(3, 0), seed=9)
    assert len(add_file(engine, clustered["dir"] / "in.bam")) == 1
    one = engine.pileup_finish()
    again = engine.pileup_finish()                      # (a finish leaves the counters as they are)
    engine.reset()                                      # (mdx_reset zeroes them)
    zero = engine.pileup_finish()
    assert not zero[0].any() and not zero[3].any() and zero[4] == dict(counted=0, outside=0, over_a_site=0, pairs=0) and set(zero[2].astype("U1")) == {"N"}
    assert len(add_file(engine, clustered["dir"] / "in.bam", 1 << 16)) >= 5
    many = engine.pileup_finish()
    check(one, records, lengths, sites, ref, k5=3, k3=0, min_qual=21, seed=9)
    for other in (again, many):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one[:4], other[:4])) and one[4] == other[4]
    # a second begin starts from zero, with other sites
    pos, off = site_columns(sites[:10], len(lengths))
    engine.pileup_begin(pos, off)
    fresh = engine.pileup_finish()
    assert fresh[0].shape == (10, 12) and not fresh[0].any() and fresh[4]["counted"] == 0


def test_the_flags_as_they_stand(engine, clustered):
    """0x200 and 0x400 on chosen records in front of the add, as the draws of -n and the duplicates' marks leave them: such records
    add nothing."""
    lengths, records, sites = clustered["lengths"], clustered["records"][:5000], clustered["sites"]
    rng = np.random.default_rng(9)
    bits = np.zeros(len(records), np.uint16)
    bits[rng.choice(len(records), 1500, replace=False)] = 0x200
    bits[rng.choice(len(records), 1000, replace=False)] |= 0x400

    def before(stream, view, first):
        f = stream.view_flags(view)
        f |= bits[first:first + len(f)]
        stream.set_view_flags(view, f)

    path = clustered["dir"] / "first.bam"
    write_records(path, records, names_of(lengths), lengths)
    ref = begin(engine, lengths, sites)
    assert len(add_file(engine, path, 1 << 16, before=before)) >= 3
    marked = [(r[0] | int(b),) + r[1:] for r, b in zip(records, bits)]
    _, counts = check(engine.pileup_finish(), marked, lengths, sites, ref)
    assert counts["counted"] < PR.brute(records, 3, lengths, sites)[1]["counted"] - 1500


def test_call_order_and_the_sites_that_are_refused(clustered):
    from mapdamage_amd.engine import DamageEngine, MdxError
    lengths, sites = clustered["lengths"], clustered["sites"]
    pos, off = site_columns(sites, len(lengths))
    with DamageEngine(LIBS3) as other:
        with pytest.raises(MdxError) as error:
            other.pileup_begin(pos, off)                # no reference yet
        assert error.value.code == ERR_STATE
        other.set_reference(reference(lengths))
        with sam.GpuBamStream(other, str(clustered["dir"] / "in.bam"), readgroups=[(rg, i) for i, rg in enumerate(RG3)]) as stream:
            with pytest.raises(MdxError) as error:
                other.pileup_add(stream.next_view())
        assert error.value.code == ERR_STATE and "mdx_pileup_begin" in str(error.value)
        for call in (other.pileup_finish, other.pileup_info):
            with pytest.raises(MdxError) as error:
                call()
            assert error.value.code == ERR_STATE
        for bad_pos, bad_off, words in (([5, 4], [0, 2, 2, 2], "site 1 (sequence 0, position 4) is not sorted"), ([5, 5], [0, 2, 2, 2], "site 1 (sequence 0, position 5) repeats"),
                                        ([5, 3000], [0, 2, 2, 2], "site 1 (sequence 0, position 3000) lies outside its sequence of 3000 bases"),
                                        ([1], [0, 0, 1, 1], "site 0 (sequence 1, position 1) lies outside its sequence of 1 bases"),
                                        ([-1], [0, 1, 1, 1], "site 0 (sequence 0, position -1) lies outside"), ([5], [0, 1, 1], "laid out for 2 sequences"),
                                        ([], [0, 0, 0, 0], "no site")):
            with pytest.raises(MdxError) as error:
                other.pileup_begin(np.array(bad_pos, np.int32), np.array(bad_off, np.int64))
            assert error.value.code == ERR_ARG and words in str(error.value), str(error.value)
        with pytest.raises(MdxError) as error:
            other.pileup_begin(pos, off, single_strand=True)
        assert error.value.code == ERR_ARG and "single_strand needs" in str(error.value)
        other.pileup_begin(pos, off)
        assert other.pileup_info()["sites"] == len(sites)
        # a new reference releases the sites that were held to the old one's lengths
        other.set_reference(reference([500]))
        with pytest.raises(MdxError) as error:
            other.pileup_finish()
        assert error.value.code == ERR_STATE


# ---------------------------------------------------------------------- 7. the command line
def rule_record(raw, lib):
    """A BAM record (with its block_size field) as a record of the rule."""
    tid, pos, l_name, _, _, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", raw, 4)
    at = 36 + l_name
    cigar = [(w & 15, w >> 4) for w in struct.unpack_from("<%dI" % n_cigar, raw, at)]
    at += 4 * n_cigar
    packed = raw[at:at + (l_seq + 1) // 2]
    seq = "".join(NIBBLES[(packed[i >> 1] >> (0 if i & 1 else 4)) & 15] for i in range(l_seq))
    qual = list(raw[at + (l_seq + 1) // 2:at + (l_seq + 1) // 2 + l_seq])
    return (flag, lib, tid, pos, cigar, seq, None if l_seq and qual[0] == 0xFF else qual)


@pytest.fixture(scope="module")
def panel(dup_data):
    """A list of sites over the reference of ``dup_data`` in no order, with alleles — the reference's letter and another, at one
    site in ten two others —, and the input's records as records of the rule."""
    ref = dup_data["ref"]
    rng = np.random.default_rng(12)
    names, lengths = list(ref.names), [int(x) for x in ref.lengths]
    sites = sorted({(t, int(p)) for t in range(len(lengths)) for p in rng.choice(lengths[t], lengths[t] // 6, replace=False)})
    alleles = []
    for g, (t, p) in enumerate(sites):
        letter = chr(ref.seqs[t][p]).upper()         # (the resident reference is upper case, as ref.fetch(...).upper() is)
        letter = letter if letter in PR.BASES else "A"
        others = [b for b in PR.BASES if b != letter]
        alleles.append((letter, others[g % 3]) if g % 10 else (others[0], others[1]))
    lines = ["# a panel", ""] + ["%s\t%d\t%s\t%s%s" % (names[t], p + 1, a, b, "\trs%d" % g if g % 3 else "") for g, ((t, p), (a, b)) in enumerate(zip(sites, alleles))]
    order = rng.permutation(len(lines))
    path = dup_data["dir"] / "panel.txt"
    path.write_text("\n".join(lines[k] for k in order) + "\n")
    (dup_data["dir"] / "plain.txt").write_text("".join("%s\t%d\n" % (names[t], p + 1) for t, p in sites[::-1]))
    ids = ["rs%d" % g if g % 3 else "." for g in range(len(sites))]
    records = [rule_record(raw, r[1]) for raw, r in zip(read_bam_file(dup_data["dir"] / "in.bam")[1], dup_data["records"])]
    return dict(path=path, plain=dup_data["dir"] / "plain.txt", sites=sites, alleles=alleles, ids=ids, names=names, lengths=lengths, records=records)


def expected_files(out, panel, records, n_libraries, path, k5=0, k3=0, q=0, mode="random", seed=0, min_depth=1, single_strand=False, alleles=True):
    sites, names = panel["sites"], panel["names"]
    pairs = panel["alleles"] if alleles else None
    want, counts = PR.brute(records, n_libraries, panel["lengths"], sites, k5, k3, q)
    letters = PR.calls(want, sites, mode, seed, min_depth, pairs, single_strand) if mode != "none" else None
    refbase = PR.refbases(panel["ref"].seqs, sites)
    assert (out / "pileup.tsv").read_text() == PR.pileup_text(names, sites, panel["ids"] if alleles else None, pairs, refbase, want, letters)
    assert (out / "pileup_summary.tsv").read_text() == PR.summary_text(path, q, k5, k3, mode, seed, min_depth, single_strand, want, letters, counts)
    log = (out / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log
    assert PR.log_line(mode, seed, want, letters, counts) in log
    assert sorted(f for f in os.listdir(out) if f.startswith("pileup")) == ["pileup.tsv", "pileup_summary.tsv"]       # (no temporary file left)
    return want, counts, letters


def test_command_line(dup_data, panel, tmp_path):
    panel = dict(panel, ref=dup_data["ref"])
    with_option = run(dup_data, tmp_path / "with", "in.bam", "--pileup-sites", panel["path"], "--pileup-min-basequal", "20", "--pileup-mask-ends", "2,1",
                      "--pileup-seed", "5", "--by-reference")
    without = run(dup_data, tmp_path / "without", "in.bam", "--by-reference")
    want, counts, letters = expected_files(with_option, panel, panel["records"], 3, panel["path"], 2, 1, 20, seed=5)
    assert counts["over_a_site"] > 1000 and want[:, PR.MASKED].sum() > 100 and want[:, PR.LOWQUAL].sum() > 100 and letters.count("N") < len(letters) / 2
    # one site in ten was written with alleles that are not the reference's; so is a site where the reference holds no base
    strangers = sum(1 for letter, pair in zip(PR.refbases(panel["ref"].seqs, panel["sites"]), panel["alleles"]) if letter not in pair)
    assert strangers >= sum(1 for g in range(len(panel["sites"])) if g % 10 == 0)
    assert "at %d of %d sites the reference's base is neither Ref nor Alt" % (strangers, len(panel["sites"])) in (with_option / "Runtime_log.txt").read_text()
    # nothing else differs: the three usual files and groups.tsv byte for byte, and without the option neither file nor line
    assert tables(with_option) == tables(without)
    assert (with_option / "by_reference" / "groups.tsv").read_bytes() == (without / "by_reference" / "groups.tsv").read_bytes()
    assert not (without / "pileup.tsv").exists() and not (without / "pileup_summary.tsv").exists()
    assert "Pileup" not in (without / "Runtime_log.txt").read_text() and "pileup" not in (without / "Runtime_log.txt").read_text()
    # the same seed: the same file; another seed: another call at a site with two eligible alleles
    again = run(dup_data, tmp_path / "again", "in.bam", "--pileup-sites", panel["path"], "--pileup-min-basequal", "20", "--pileup-mask-ends", "2,1", "--pileup-seed", "5")
    assert (again / "pileup.tsv").read_bytes() == (with_option / "pileup.tsv").read_bytes()
    other = run(dup_data, tmp_path / "other", "in.bam", "--pileup-sites", panel["path"], "--pileup-min-basequal", "20", "--pileup-mask-ends", "2,1", "--pileup-seed", "6")
    _, _, other_letters = expected_files(other, panel, panel["records"], 3, panel["path"], 2, 1, 20, seed=6)
    changed = [g for g, (a, b) in enumerate(zip(letters, other_letters)) if a != b]
    assert changed and all(sum(1 for b in range(4) if PR.BASES[b] in panel["alleles"][g] and want[g, b] + want[g, 4 + b]) == 2 for g in changed)


def test_command_line_without_alleles_and_without_calls(dup_data, panel, tmp_path):
    panel = dict(panel, ref=dup_data["ref"])
    out = run(dup_data, tmp_path / "none", "in.bam", "--pileup-sites", panel["plain"], "--pileup-call", "none", "--chunk-mb", "0.0625")
    expected_files(out, panel, panel["records"], 3, panel["plain"], mode="none", alleles=False)
    assert "neither Ref nor Alt" not in (out / "Runtime_log.txt").read_text()
    out = run(dup_data, tmp_path / "majority", "in.bam", "--pileup-sites", panel["plain"], "--pileup-call", "majority", "--pileup-min-depth", "2")
    expected_files(out, panel, panel["records"], 3, panel["plain"], mode="majority", min_depth=2, alleles=False)


def test_command_line_beside_the_pipeline(dup_data, panel, tmp_path):
    """With --remove-duplicates --depth --write-kept the pileup is the brute force over the records of the written file, and every
    other file is what it is without the option."""
    panel = dict(panel, ref=dup_data["ref"])
    args = ["--remove-duplicates", "--min-mapq", "25", "--depth", "--write-kept"]
    with_option = run(dup_data, tmp_path / "with", "in.bam", *args, tmp_path / "kept.bam", "--pileup-sites", panel["path"], "--pileup-single-strand-mode",
                      "--pileup-call", "majority")
    without = run(dup_data, tmp_path / "without", "in.bam", *args, tmp_path / "kept0.bam")
    written = [rule_record(raw, 0) for raw in read_bam_file(tmp_path / "kept.bam")[1]]
    assert len(written) > 500
    _, counts, _ = expected_files(with_option, panel, written, 1, panel["path"], mode="majority", single_strand=True)
    assert counts["counted"] == len(written) and counts["outside"] == 0
    assert tables(with_option) == tables(without) and (tmp_path / "kept.bam").read_bytes() == (tmp_path / "kept0.bam").read_bytes()
    for name in ("coverage.tsv", "depth_histogram.tsv", "duplicates.tsv", "duplicates_histogram.tsv"):
        assert (with_option / name).read_bytes() == (without / name).read_bytes(), name


def test_sam_text_is_refused(dup_data, panel, tmp_path):
    from tests.test_gpu_write_kept import RGS
    b, ref = dup_data["batch"].slice(0, 200), dup_data["ref"]
    sam.write_sam(str(tmp_path / "in.sam"), b, ref.names, ref.lengths, RGS, [RGS[int(i)]["ID"] for i in b.lib])
    out = run(dup_data, tmp_path / "sam", tmp_path / "in.sam", "--pileup-sites", panel["path"], rc=1)
    assert "--pileup-sites needs BAM input" in (out / "Runtime_log.txt").read_text()
    assert not any((out / f).exists() for f in FILES + ("pileup.tsv", "pileup_summary.tsv"))


def test_a_sites_file_the_header_refuses_ends_the_run(dup_data, tmp_path):
    (tmp_path / "sites.txt").write_text("chr1\t5\nchr77\t9\n")
    out = run(dup_data, tmp_path / "out", "in.bam", "--pileup-sites", tmp_path / "sites.txt", rc=1)
    assert "line 2: sequence 'chr77' is not in the input's header" in (out / "Runtime_log.txt").read_text()
    assert not any((out / f).exists() for f in FILES + ("pileup.tsv", "pileup_summary.tsv"))


def test_a_slab_the_device_path_gives_up_on_ends_the_run(dup_data, panel, tmp_path, monkeypatch):
    from mapdamage_amd.main import main
    monkeypatch.setenv("MDX_GBAM_FAIL_AT", "0")             # (its first slab)
    out = tmp_path / "out"
    assert main(["-i", str(dup_data["dir"] / "in.bam"), "-r", str(dup_data["dir"] / "ref.fa"), "-d", str(out), "--no-stats", "--pileup-sites", str(panel["path"])]) == 1
    monkeypatch.delenv("MDX_GBAM_FAIL_AT")
    log = (out / "Runtime_log.txt").read_text()
    assert "GPU decode path gave up" in log
    assert "--pileup-sites is gathered on the device decode path" in log.split("GPU decode path gave up")[1]
    assert not any((out / f).exists() for f in FILES + ("pileup.tsv", "pileup_summary.tsv"))
