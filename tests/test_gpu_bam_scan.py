"""The device BAM record scan where its guesses are wrong (csrc/mdx_gbam.hip gbam_scan_kernel; the walk of gbam_half_b and
mdx_gbam_skip in csrc/mdx_bamio.cpp).  One lane per BGZF block guesses where the block's first record starts — the first
offset at which three plausible records follow one another — and the host walk rescans the blocks whose guess was another
offset than the one the chain in front of them lands on (the fixups).  The files of tests/bam_decoys.py carry byte strings
that look like chains of records inside true records, cut so that a block's first such triple is a decoy: the fixups run,
the decoy chains the walk steps over count nothing, a rank of a sharded run that would start from a decoy is told so by the
rank in front of it (MDX_ERR_UNSUPPORTED from ``skip``), and the command line falls back to the host decoder behind that.
Every comparison is exact equality with the truth the files were built from (tests/test_bam_decoys.py checks the files
themselves on the host), or with the oracle's tables over that truth."""
import functools

import numpy as np
import pytest

from mapdamage_amd import sam
from mapdamage_amd.batch import ReadBatch, Reference
from tests import bam_decoys as D
from tests.test_gpu_decode import _d2h

pytestmark = pytest.mark.gpu

FILES = ("misincorporation.txt", "dnacomp.txt", "lgdistribution.txt")
# MDX_SEQ_4BIT (include/mdx.h): code 1 = 'A', 2 = 'C', 4 = 'T', 8 = 'G', 0 for every other symbol — of BAM's nibbles "=ACMGRSVTWYHKDBN"
CODE_OF_NIBBLE = np.zeros(16, np.uint8)
CODE_OF_NIBBLE[[1, 2, 4, 8]] = [1, 2, 8, 4]


@functools.lru_cache(maxsize=None)
def reference():
    return Reference([r[0] for r in D.REFS], D.genome())


@pytest.fixture(scope="module")
def engine():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(D.LIBRARIES) as eng:
        eng.set_reference(reference())
        yield eng


def open_stream(eng, path, chunk, packed=False, **kw):
    return sam.GpuBamStream(eng, str(path), readgroups=list(D.LIB_OF_RG.items()), chunk_bytes=chunk, want_qual=True, want_mate=True,
                            packed=packed, **kw)


def slab_of(eng, view):
    """The columns of a view on the host; a 4-bit SEQ column expanded nibble by nibble, the low nibble first."""
    eng.sync()
    k, nb, nc = int(view.n_reads), int(view.n_bases), int(view.n_cigar)
    s = dict(n=k, n_bases=nb, seq_format=int(view.seq_format), flag=_d2h(view.flag, k, np.uint16), lib=_d2h(view.lib, k, np.uint16))
    for name in ("tid", "pos", "tlen", "mtid", "mpos"):
        s[name] = _d2h(getattr(view, name), k, np.int32)
    s["cigar_off"], s["seq_off"] = _d2h(view.cigar_off, k + 1, np.uint32), _d2h(view.seq_off, k + 1, np.uint32)
    assert s["cigar_off"][0] == 0 and s["seq_off"][0] == 0 and s["cigar_off"][-1] == nc and s["seq_off"][-1] == nb
    s["cigar"] = _d2h(view.cigar, nc, np.uint32)
    if s["seq_format"] == 0:
        s["seq"] = _d2h(view.seq, nb, np.uint8)
    else:
        col = _d2h(view.seq, (nb + 1) // 2, np.uint8)
        s["seq"] = np.stack([col & 15, col >> 4], axis=1).reshape(-1)[:nb]
    s["qual"] = _d2h(view.qual, nb, np.uint8) if view.qual else None
    return s


def slab_is_truth(b, s, at, minqual=0, why=None):
    """Is slab ``s`` exactly the truth's records from record ``at`` on?  (``why``: a list that takes the first difference.)"""
    k = s["n"]

    def same(name, got, want):
        ok = len(got) == len(want) and bool(np.array_equal(np.asarray(got), np.asarray(want)))
        if not ok and why is not None and not why:
            why.append("%s of the slab at record %d" % (name, at))
        return ok
    if at + k > b.n:
        return same("record count", [k], [b.n - at])
    c0, s0 = int(b.cigar_off[at]), int(b.seq_off[at])
    nb, nc = int(b.seq_off[at + k]) - s0, int(b.cigar_off[at + k]) - c0
    lens = np.diff(b.seq_off[at:at + k + 1].astype(np.int64))
    qual = b.qual[s0:s0 + nb]
    first = qual[np.minimum(b.seq_off[at:at + k].astype(np.int64) - s0, max(0, nb - 1))] if nb else np.zeros(k, np.uint8)
    ok = same("flag", s["flag"] & np.uint16(0x3FFF), b.flag[at:at + k])
    # MDX_FLAG_HAS_QUAL: at least one base and a first quality byte that is not 0xFF
    ok = ok and same("0x4000", (s["flag"] & 0x4000) != 0, (lens > 0) & (first != 0xFF))
    if minqual:
        # MDX_FLAG_QUAL_ABOVE_MIN: every base quality of the record is at least the threshold (0xFF is below none)
        above = np.asarray([bool((qual[int(o) - s0:int(o) - s0 + int(n)] >= minqual).all()) for o, n in zip(b.seq_off[at:at + k], lens)], bool)
        ok = ok and same("0x8000", (s["flag"] & 0x8000) != 0, above)
    else:
        ok = ok and same("0x8000", (s["flag"] & 0x8000) != 0, np.zeros(k, bool))
    for name in ("lib", "tid", "pos", "tlen", "mtid", "mpos"):
        ok = ok and same(name, s[name], getattr(b, name)[at:at + k])
    ok = ok and same("cigar_off", s["cigar_off"].astype(np.int64), b.cigar_off[at:at + k + 1].astype(np.int64) - c0)
    ok = ok and same("seq_off", s["seq_off"].astype(np.int64), b.seq_off[at:at + k + 1].astype(np.int64) - s0)
    ok = ok and same("cigar", s["cigar"], b.cigar[c0:c0 + nc])
    nib = b.nib[s0:s0 + nb]
    if s["seq_format"] == 0:
        want = D.SEQ_LETTERS[nib]
    elif s["seq_format"] == 1:
        want = CODE_OF_NIBBLE[nib]
    else:
        # MDX_SEQ_4BITQ: a symbol whose quality is below the threshold is stored as the complement of its code
        want = np.where(qual < minqual, CODE_OF_NIBBLE[nib] ^ 15, CODE_OF_NIBBLE[nib])
    ok = ok and same("seq (format %d)" % s["seq_format"], s["seq"], want)
    if s["qual"] is not None:
        ok = ok and same("qual", s["qual"], qual)
    return ok


def decode_whole(eng, b, path, chunk, packed=False, minqual=0, **kw):
    """One handle over the whole file: every slab is the truth's next records; returns (slabs, fixups)."""
    at, slabs = 0, []
    with open_stream(eng, path, chunk, packed, **kw) as g:
        assert g.header.references == [r[0] for r in D.REFS]
        while (view := g.next_view()) is not None:
            s = slab_of(eng, view)
            assert not (s["pos"] >= D.DECOY_POS).any(), "a decoy was counted as a record"
            why = []
            assert slab_is_truth(b, s, at, minqual, why), why
            at += s["n"]
            slabs.append(s)
        fixups = g.fixups()
    assert at == b.n
    return slabs, fixups


# ------------------------------------------------------------------------------------------------ fixups: one handle
@pytest.mark.parametrize("chunk", [1 << 16, 1 << 28])
@pytest.mark.parametrize("where", ["front", "mid", "long"])
@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
def test_a_block_that_starts_with_a_decoy_is_rescanned(tmp_path, engine, kind, where, chunk):
    """A cut in front of a decoy chain (in front of its first image; inside the image region; uniform cuts through a carrier of
    ten blocks, whose inner blocks the walk steps over): the block's guess is the decoy, the walk rescans it from the record
    the chain in front lands on — fixups() says that it did — and the columns are the truth's, no phantom record among them."""
    b = D.decoys(kind, where)
    path = b.write(tmp_path / "f.bam")
    for packed in (False, True):
        slabs, fixups = decode_whole(engine, b, path, chunk, packed)
        assert fixups >= 1
        assert len(slabs) == 1 if chunk == 1 << 28 else len(slabs) >= 4


@pytest.mark.parametrize("chunk", [1 << 16, 1 << 18, 1 << 28])
def test_a_file_of_carriers_only(tmp_path, engine, chunk):
    """Every record a carrier, most blocks begin with a false start: columns, and the tables of the oracle over the truth."""
    from mapdamage_amd.engine import DamageEngine
    from tests.util import assert_tables_equal, oracle_tableset
    b = D.mixed()
    path = b.write(tmp_path / "mixed.bam")
    for packed in (False, True):
        slabs, fixups = decode_whole(engine, b, path, chunk, packed)
        assert fixups >= 1
    want = oracle_tableset(reference(), truth_batch(b), D.LIBRARIES, 70, 10)
    assert want.n_kept > 0.6 * b.n
    with DamageEngine(D.LIBRARIES) as eng:
        eng.set_reference(reference())
        with sam.GpuBamStream(eng, str(path), readgroups=list(D.LIB_OF_RG.items()), chunk_bytes=chunk) as g:
            while (view := g.next_view()) is not None:
                eng.tabulate_view(view)
            assert g.fixups() >= 1
        assert_tables_equal(eng.finish(), want)


def truth_batch(b):
    return ReadBatch(b.flag.copy(), b.lib.copy(), b.tid.copy(), b.pos.copy(), b.tlen.copy(), b.cigar_off.copy(), b.cigar.copy(),
                     b.seq_off.copy(), b.seq.copy(), b.qual.copy())


@pytest.mark.parametrize("chunk", [1 << 16, 1 << 28])
@pytest.mark.parametrize("spec", [("decoys", "e", "front"), ("plain", "htslib")], ids=["two_images", "htslib"])
def test_no_fixup_where_nothing_misleads(tmp_path, engine, spec, chunk):
    """Two images are no three records in a row, and an htslib file starts every block at a record: nothing is rescanned."""
    b = getattr(D, spec[0])(*spec[1:])
    _, fixups = decode_whole(engine, b, b.write(tmp_path / "f.bam"), chunk)
    assert fixups == 0


# ------------------------------------------------------------------------------------------------ cuts and empty members
@pytest.mark.parametrize("chunk", [1 << 16, 1 << 28])
@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "4bit"])
def test_cuts_at_every_phase_of_a_record_and_empty_members(tmp_path, engine, packed, chunk):
    """Cuts 0 to 3 bytes into a block_size field, inside the fixed fields, the name, the CIGAR, the nibbles, the qualities, the
    tags, the last one fewer than 36 bytes before the end of the data; empty members in front of the first record, between two
    records, inside one, twice in a row and in front of the end-of-file marker: a valid file, decoded as its truth (any error
    — "truncated BAM file", "corrupt BAM record" — fails the test)."""
    b = D.phases()
    decode_whole(engine, b, b.write(tmp_path / "f.bam"), chunk, packed)


@pytest.mark.parametrize("layout", ["65498", "90"])
def test_decoy_free_files_cut_anywhere(tmp_path, engine, layout):
    b = D.plain(layout)
    decode_whole(engine, b, b.write(tmp_path / "f.bam"), 1 << 16)


# ------------------------------------------------------------------------------------------------ short sequences
@pytest.mark.parametrize("form", ["ascii", "4bit", "4bitq"])
def test_sequences_of_0_to_24_bases(tmp_path, engine, form):
    """gbam_unpack_kernel's tails: every l_seq from 0 to 24 at both nibble parities of seq_off, ambiguity codes and '=' among
    the nibbles, in the file's form, as MDX_SEQ_4BIT and as MDX_SEQ_4BITQ (--min-basequal folded in: qualities one below, at
    and above the threshold, or 0xFF), with the flag hints 0x4000 and 0x8000 by their definitions in include/mdx.h."""
    from mapdamage_amd.engine import DamageEngine
    b = D.short_sequences()
    path = b.write(tmp_path / "f.bam")
    if form != "4bitq":
        slabs, _ = decode_whole(engine, b, path, 1 << 28, packed=form == "4bit")
        assert [s["seq_format"] for s in slabs] == [0 if form == "ascii" else 1]
        return
    with DamageEngine(D.LIBRARIES, 70, 10, D.SHORT_THRESHOLD) as eng:
        eng.set_reference(reference())
        slabs, _ = decode_whole(eng, b, path, 1 << 28, packed=True, minqual=D.SHORT_THRESHOLD, min_basequal=D.SHORT_THRESHOLD)
        assert [s["seq_format"] for s in slabs] == [2]
        assert (slabs[0]["seq"] > 8).any()          # (complemented codes among them)


# ------------------------------------------------------------------------------------------------ the sharded check
def emulate_ranks(eng, b, path, world):
    """``world`` handles on one file, handle r decoding the slabs r, r + world, ... and stepping over the others — the calls
    main.py makes per rank, slab by slab.  The handle that decoded the slab in front is the one that knows where the next
    slab's first record starts: if the slab a handle hands out is not exactly the truth's records from where the slab in front
    ended, that handle must have raised from its skip() of that very slab — the emulation stops there, as the ranks would.
    Returns (records handed out, all exact and disjoint; the slab at which a skip() raised, or None)."""
    handles = [open_stream(eng, path, 1 << 16) for _ in range(world)]
    try:
        at, slab = 0, 0
        while True:
            owner = slab % world
            for r in range(world):
                if r == owner:
                    continue
                try:
                    handles[r].skip()
                except sam.GpuDecodeUnsupported as error:
                    # only the handle that has seen the slab in front can tell
                    assert slab > 0 and r == (slab - 1) % world, (slab, r)
                    assert "cannot be found without the slab in front" in str(error)
                    return at, slab
            try:
                view = handles[owner].next_view()
            except ValueError as error:
                raise AssertionError("slab %d: its first record was a wrong guess (%s) and nobody said so" % (slab, error))
            if view is None:
                return at, None
            s = slab_of(eng, view)
            why = []
            if s["n"]:
                assert s["pos"][0] == at and slab_is_truth(b, s, at, why=why), \
                    "slab %d starts at record %d, not %d (%s), and the handle in front did not raise" % (slab, int(s["pos"][0]), at, why)
            at += s["n"]
            slab += 1
    finally:
        for g in handles:
            g.close()


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("layout", ["htslib", "65498", "90"])
def test_ranks_agree_on_the_borders_of_decoy_free_files(tmp_path, engine, layout, world):
    """Nothing misleads: no skip() raises, and the slabs are the truth, each record once.  (The htslib file and the one cut at
    65 498 end in a slab that holds the end-of-file marker and nothing else: there is no record behind the border for the
    handle in front to vouch for, which it once took for a guess it could not confirm.)"""
    b = D.plain(layout)
    at, raised = emulate_ranks(engine, b, b.write(tmp_path / "f.bam"), world)
    assert raised is None and at == b.n


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("spec", [("mixed",)] + [("decoys", kind, where) for kind in "abcd" for where in ("front", "long")],
                         ids=lambda s: "_".join(s))
def test_a_rank_is_told_when_its_guess_would_be_a_decoy(tmp_path, engine, spec, world):
    """Slabs whose first block starts with a decoy: whatever a handle hands out before a skip() raises is exact (the invariant
    is asserted inside emulate_ranks).  On the file of carriers only, where most blocks begin with a false start, the
    verification must say no at least once."""
    b = getattr(D, spec[0])(*spec[1:])
    at, raised = emulate_ranks(engine, b, b.write(tmp_path / "f.bam"), world)
    if spec[0] == "mixed":
        assert raised is not None
    assert at == b.n if raised is None else at < b.n


# ------------------------------------------------------------------------------------------------ the product
def test_the_command_line_on_a_file_of_carriers(tmp_path, monkeypatch):
    """`python -m mapdamage_amd` over the file of carriers only, in slabs of 64 KiB: one rank rescans blocks and writes the
    oracle's tables; two ranks fall back to the host decoder — a rank's guess would have been a decoy — and write the same bytes."""
    from mapdamage_amd import fasta
    from tests.test_gpu_distributed import _cli
    from tests.util import oracle_tableset
    b = D.mixed()
    path = b.write(tmp_path / "mixed.bam")
    assert path.stat().st_size < 4 << 20
    fasta.write_fasta(tmp_path / "ref.fa", reference())
    want = oracle_tableset(reference(), truth_batch(b), D.LIBRARIES, 70, 10)
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", str(1 << 16))
    common = ["-i", path, "-r", tmp_path / "ref.fa", "--no-stats", "--gpu-decode", "--chunk-mb", "4", "--log-level", "DEBUG"]
    one, two = tmp_path / "one", tmp_path / "two"
    _cli(common + ["-d", one])
    assert [(one / f).read_text() for f in FILES] == [want.misincorporation_text(), want.dnacomp_text(), want.lgdistribution_text()]
    log = (one / "Runtime_log.txt").read_text()
    assert "BGZF blocks rescanned" in log and "Decode path: device; fallbacks from the device path: 0" in log
    _cli(common + ["-d", two], gpus=2, port=29561)
    for f in FILES:
        assert (one / f).read_bytes() == (two / f).read_bytes(), f
    log = (two / "Runtime_log.txt").read_text()
    import re
    assert re.search(r"fallbacks from the device path: [1-9]", log), log[-3000:]
    assert "GPU decode path gave up" in log
