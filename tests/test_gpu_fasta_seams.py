"""The resident reference at its seams: every case of tests/fasta_seams.py, as a plain file and as its BGZF twins, through
the library's loader (include/mdx.h mdx_set_reference_fasta: fasta_strip_kernel over pieces and inflated slabs), then

  a. the bytes of every wanted sequence against the model's fetch (faidx restated),
  b. the per-sequence base counts of genome_comp_kernel against a numpy count of the model's sequences,
  c. the loader's own account of what it uploaded and inflated against the model's pieces and slabs — for every case, though
     ``gaps`` is the class built for it: pieces and blocks between wanted sequences stay on disk,
  d. for ``crowded`` and ``tail`` the tables of perfect-match reads over contigs shorter than --around, under the ASCII and
     the packed kernel (the 4-bit form of the reference: ref_finish's encode_ref4), against the C oracle over the model's
     sequences: a flank position holds nothing, not a neighbour's bases and not a guard byte,
  e. for ``overlap`` — index rows that share bytes of the file — a refusal (or the model's bytes), never 'N' in silence.

All comparisons are exact.  One engine serves the module; MDX_FASTA_PIECE_BYTES is set per case (the loader reads it on
every call)."""
import pathlib
import time

import numpy as np
import pytest

from mapdamage_amd import fasta
from mapdamage_amd.batch import Reference, batch_from_records
from tests import fasta_seams as F
from tests.test_fasta_bgzf import _write_blocks
from util import assert_tables_equal, oracle_tableset

pytestmark = pytest.mark.gpu

LIBRARIES = [("s", "l")]


@pytest.fixture(scope="module")
def eng():
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(LIBRARIES, 70, 10, 0) as engine:
        yield engine


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return tmp_path_factory.mktemp("fasta_seams")


_FILES = {}


def _file(root, case):
    """The case's file with its .fai (the model's rows: tests/test_fasta_seams_cases.py holds them against the index the
    library builds) -> (path, the writer's block starts or None); a twin's .gzi is built by the library where the case wants one."""
    key = (case.cls, case.label)
    if key not in _FILES:
        path = root / ("%s_%04d%s" % (case.cls, len(_FILES), ".fa" if case.block is None else ".fa.gz"))
        starts = None
        if case.block is None:
            path.write_bytes(case.text)
        else:
            starts = _write_blocks(path, case.text, size=case.block)
        pathlib.Path(str(path) + ".fai").write_bytes(F.fai_text(case.fai))
        if case.gzi:
            fasta.ensure_fasta_index(path)
            assert pathlib.Path(str(path) + ".gzi").exists()
        _FILES[key] = (path, starts)
    return _FILES[key]


def _load(eng, monkeypatch, case, path):
    if case.piece is None:
        monkeypatch.delenv("MDX_FASTA_PIECE_BYTES", raising=False)
    else:
        monkeypatch.setenv("MDX_FASTA_PIECE_BYTES", str(case.piece))
    on_disk = fasta.FastaOnDisk(path, case.order, [0] * len(case.order), missing_ok=True)
    eng.set_reference(on_disk)
    return on_disk


def _bytes_and_composition(eng, case, on_disk):
    """Checks a and b -> what is wrong, in words (None: nothing)."""
    want = F.sequences(case)
    if on_disk.lengths != [len(s) for s in want]:
        return "lengths %r, the model's %r" % (on_disk.lengths[:12], [len(s) for s in want][:12])
    rows = {}
    for row in case.fai:
        rows.setdefault(row[0], row)
    for tid, (name, seq) in enumerate(zip(case.order, want)):
        got = eng.reference_fetch(tid, 0, len(seq))
        if got != seq:
            a, b = np.frombuffer(got, np.uint8), np.frombuffer(seq, np.uint8)
            i = int(np.flatnonzero(a != b)[0])
            return ("sequence %r (tid %d, %d bases): base %d, at offset %d of the text, is %r, the model's %r"
                    % (name, tid, len(seq), i, int(F.offsets(rows[name])[i]), got[i:i + 1], seq[i:i + 1]))
    got, model = eng.genome_composition(len(case.order)), F.composition(want)
    if not np.array_equal(got, model):
        tid = int(np.flatnonzero((got != model).any(axis=1))[0])
        return "composition of sequence %r (tid %d): %r, the model's %r" % (case.order[tid], tid, got[tid].tolist(), model[tid].tolist())
    return None


def _upload_account(eng, case, starts):
    """Check c -> what is wrong with the loader's account of its uploads (None: nothing)."""
    stats = eng.fasta_load_stats()
    if not F.wanted_rows(case):
        want = dict(blocks=0, inflated=0, slabs=0, bytes=0)           # (no base wanted: the file is not opened further)
    elif case.block is None:
        used = [(f0, n) for f0, n, any_wanted in F.pieces(case) if any_wanted]
        want = dict(blocks=0, inflated=0, slabs=len(used), bytes=sum(n for _, n in used))
    else:
        slabs = F.slabs(case)
        # a slab's compressed bytes: from its first block's start to the start of the block behind its last
        want = dict(blocks=len(starts), inflated=sum(len(s) for s in slabs), slabs=len(slabs),
                    bytes=sum(starts[s[-1] + 1][0] - starts[s[0]][0] for s in slabs))
    return None if stats == want else "the loader's account %r, the model's %r" % (stats, want)


def _run(eng, monkeypatch, root, cases):
    offenders, t0 = [], time.perf_counter()
    for case in cases:
        path, starts = _file(root, case)
        on_disk = _load(eng, monkeypatch, case, path)
        wrong = _bytes_and_composition(eng, case, on_disk)
        if wrong is None:
            wrong = _upload_account(eng, case, starts)
        if wrong:
            offenders.append("%r: %s" % (case, wrong))
    print("%d loads, %d offenders, %.2f ms per load with its checks" % (len(cases), len(offenders), 1e3 * (time.perf_counter() - t0) / max(1, len(cases))))
    assert not offenders, "%d offenders, the first ten:\n%s" % (len(offenders), "\n".join(offenders[:10]))


@pytest.mark.parametrize("eol", ["LF", "CRLF"])
@pytest.mark.parametrize("width", F.PHASE_WIDTHS)
def test_a_piece_or_slab_may_end_on_any_kind_of_byte(eng, monkeypatch, root, width, eol):
    """``phase``: the first piece of the plain file, the first slab of the twin, ends on the first or last base of a line, its
    LF or CR, the '>' of the next header or inside it, the first base of the next sequence, or with the file."""
    prefix = "width %d, %s," % (width, eol)
    mine = [x for x in F.cases("phase") + F.twins("phase") if x.label.startswith(prefix)]
    assert len(mine) == 3 * (8 if eol == "CRLF" else 7)
    _run(eng, monkeypatch, root, mine)


@pytest.mark.parametrize("cls", ["crowded", "alphabet", "tail"])
def test_sequences_end_inside_a_lane(eng, monkeypatch, root, cls):
    """Hundreds of sequences of 0 to 3 bases, wanted ones and others interleaved; every byte value in every place of a unit;
    every residue of the genome's length and of the last piece's."""
    _run(eng, monkeypatch, root, F.cases(cls) + F.twins(cls))


@pytest.mark.parametrize("part", [0, 1, 2])
def test_every_line_shape_loads(eng, monkeypatch, root, part):
    """``geometry``: lines of 1 to piece + 1 bases, line ends of 0, 1 and 2 bytes, full and short last lines, with and without
    a line end at the file's end."""
    _run(eng, monkeypatch, root, (F.cases("geometry") + F.twins("geometry"))[part::3])


def test_what_lies_between_wanted_sequences_stays_on_disk(eng, monkeypatch, root):
    """``gaps``: pieces without a wanted byte are not uploaded, blocks no wanted sequence reaches into are not inflated."""
    _run(eng, monkeypatch, root, F.cases("gaps") + F.twins("gaps"))


def _perfect_reads(seqs):
    """One read per non-empty sequence covering it whole, and for those of two bases and more one on each strand at either
    end; a read's base is the sequence's where that is one of the four, 'N' elsewhere."""
    records = []
    for tid, seq in enumerate(seqs):
        n = len(seq)
        if n == 0:
            continue
        bases = "".join(chr(c) if c in b"ACGT" else "N" for c in seq)
        spans = [(0, n, 0)]
        if n >= 2:
            k = max(1, n // 2)
            spans += [(0, k, 0), (0, k, 16), (n - k, n, 0), (n - k, n, 16)]
        for lo, hi, flag in spans:
            records.append(dict(flag=flag, lib=0, tid=tid, pos=lo, tlen=0, cigar=[(0, hi - lo)], seq=bases[lo:hi]))
    return batch_from_records(records, with_qual=False)


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "ascii"])
@pytest.mark.parametrize("cls", ["crowded", "tail"])
def test_flanks_of_short_contigs_hold_nothing(eng, monkeypatch, root, cls, packed):
    """Contigs shorter than --around on both sides of a read: what the kernels read beyond a contig's ends — the neighbour's
    bases in ``d_ref`` and its nibbles in ``d_ref4``, the guard byte behind an odd genome — must not be counted."""
    offenders = []
    for case in F.cases(cls) + F.twins(cls):
        seqs = F.sequences(case)
        path, _ = _file(root, case)
        _load(eng, monkeypatch, case, path)
        batch = _perfect_reads(seqs)
        want = oracle_tableset(Reference(list(case.order), seqs), batch, LIBRARIES, 70, 10)
        eng.reset()
        before = eng.packed_launches()
        eng.tabulate(batch, packed=packed)
        got = eng.finish()
        assert (eng.packed_launches() > before) == packed
        try:
            assert_tables_equal(got, want)
        except AssertionError as exc:
            offenders.append("%r (%d reads): %s" % (case, batch.n, str(exc)[:600]))
    eng.reset()
    assert not offenders, "%d offenders, the first three:\n%s" % (len(offenders), "\n".join(offenders[:3]))


def test_index_rows_that_share_bytes_are_refused(eng, monkeypatch, root):
    """``overlap``: a byte of the file goes to one sequence.  (Before the refusal the shared bytes went to the row that
    starts last and the rest of the other row kept its fill: 'N' where the file holds bases, and no error.)"""
    from mapdamage_amd.engine import MdxError
    for case in F.cases("overlap"):
        path, _ = _file(root, case)
        if case.label == "touching":
            on_disk = _load(eng, monkeypatch, case, path)
            assert _bytes_and_composition(eng, case, on_disk) is None
            continue
        try:
            on_disk = _load(eng, monkeypatch, case, path)
        except MdxError as exc:
            assert "re-index" in str(exc) and "samtools faidx" in str(exc) and "named twice" not in str(exc), exc
            # the message names the two sequences (in all three indexes row b begins inside row a)
            assert "'a'" in str(exc) and "'b'" in str(exc), exc
            print("%r refused: %s" % (case, exc))
            continue
        wrong = _bytes_and_composition(eng, case, on_disk)
        assert wrong is None, "%r loaded without an error: %s" % (case, wrong)
    # the refusal of a sequence wanted twice stays as it was
    case = F.cases("overlap")[0]
    twice = root / "twice.fa"
    twice.write_bytes(case.text)
    pathlib.Path(str(twice) + ".fai").write_bytes(F.fai_text([("a", 100, 3, 100, 101), ("b", 50, 3, 100, 101)]))
    with pytest.raises(MdxError, match="named twice"):
        eng.set_reference(fasta.FastaOnDisk(twice, ["a", "b"], [0, 0], missing_ok=True))
    # ... and the engine takes the next reference
    path, _ = _file(root, F.cases("overlap")[-1])
    assert _bytes_and_composition(eng, F.cases("overlap")[-1], _load(eng, monkeypatch, F.cases("overlap")[-1], path)) is None
