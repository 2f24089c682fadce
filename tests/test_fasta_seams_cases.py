"""The cases of tests/fasta_seams.py are what tests/test_gpu_fasta_seams.py needs them to be (no GPU here): the same bytes
from the same seed; the model's sequences are the Python reader's and its index rows are, byte for byte, the .fai the
library builds — for the plain files and for their BGZF twins, whose .gzi holds the block starts the writer returned —; and
every seam the classes are there for is in them, stated by the model alone, so that an edit of the generator cannot lose one
without a failure here."""
import pathlib

import numpy as np
import pytest

from mapdamage_amd import fasta
from tests import fasta_seams as F
from tests.test_fasta_bgzf import _read_gzi, _write_blocks

GENERATED = [c for c in F.CLASSES if c != "overlap"]


def _key(case):
    return (case.cls, case.label, case.text, tuple(case.fai), tuple(case.order), case.piece, case.kind, case.block, case.gzi)


@pytest.mark.parametrize("cls", F.CLASSES)
def test_same_seed_same_bytes(cls):
    assert [_key(x) for x in F.generate(cls, 0)] == [_key(x) for x in F.generate(cls, 0)] == [_key(x) for x in F.cases(cls)]
    assert [x.label for x in F.generate(cls, 1)] == [x.label for x in F.cases(cls)]
    if cls != "overlap":
        assert [x.text for x in F.generate(cls, 1)] != [x.text for x in F.cases(cls)]


@pytest.mark.parametrize("cls", F.CLASSES)
def test_cases_have_the_shape_the_issue_states(cls):
    cases, twins = F.cases(cls), F.twins(cls)
    assert cases and all(x.cls == cls and x.label and x.block is None and x.gzi is None for x in cases)
    assert len({x.label for x in cases}) == len(cases) and len({x.label for x in twins}) == len(twins)
    assert max(len(x.text) for x in cases + twins) <= 80_000
    assert all(x.piece in (None, F.PIECE) for x in cases + twins) and F.PIECE % 16 == 0
    if cls == "overlap":
        assert not twins and all(x.own_fai for x in cases)
        return
    assert not any(x.own_fai for x in cases + twins)
    # every text with a built .gzi and without one, and every block size in the class
    assert sorted((x.text, x.block, x.gzi) for x in twins if x.gzi) == sorted((x.text, x.block, True) for x in twins if not x.gzi)
    if len(twins) >= 2 * len(F.BLOCK_SIZES):
        assert {x.block for x in twins} == set(F.BLOCK_SIZES)
    if cls == "gaps":
        assert {(x.text, x.order[0], x.block) for x in twins} == {(x.text, x.order[0], b) for x in cases for b in F.BLOCK_SIZES}
    for x in cases + twins:
        assert len(set(x.order)) == len(x.order) and x.order
    # absent names among the wanted ones
    assert any(n not in {r[0] for r in x.fai} for x in cases for n in x.order)


def test_every_block_size_is_used():
    assert {x.block for cls in GENERATED for x in F.twins(cls)} == set(F.BLOCK_SIZES)


@pytest.mark.parametrize("cls", GENERATED)
def test_the_model_is_the_python_reader_and_the_library_index(cls, tmp_path):
    done = set()
    for i, case in enumerate(F.cases(cls) + F.twins(cls)):
        if (case.text, case.block) in done:
            continue
        done.add((case.text, case.block))
        want = F.fai_text(case.fai)
        if case.block is None:
            path = tmp_path / ("%03d.fa" % i)
            path.write_bytes(case.text)
            names, seqs = fasta.read_fasta(path)
            assert names == [r[0] for r in case.fai], case
            for row, seq in zip(case.fai, seqs):
                assert F.fetch_raw(case.text, row) == seq, (case, row)
            assert [F.fetch(case.text, r) for r in case.fai] == [F.fold(s) for s in seqs], case
        else:
            path = tmp_path / ("%03d.fa.gz" % i)
            starts = _write_blocks(path, case.text, size=case.block)
        fasta.ensure_fasta_index(path)
        assert pathlib.Path(str(path) + ".fai").read_bytes() == want, case
        if case.block is not None:
            # bgzip's .gzi: every block behind the first, without the end-of-file block
            assert _read_gzi(str(path) + ".gzi") == starts[1:-1], case
            assert [u for _, u in starts[:-1]] == F.block_bounds(case)[:-1]


def test_the_model_on_a_file_written_by_hand():
    """The index rows and fetches of a file small enough to count on one's fingers (the rows are those of
    tests/test_fasta_loader.py's CR LF file)."""
    text = b">x desc\r\nACGT\r\nAC\r\n>y\r\nGG\r\n>z\n"
    rows = F.fai_rows(text)
    assert rows == [("x", 6, 9, 4, 6), ("y", 2, 23, 2, 4), ("z", 0, 30, 0, 0)]
    assert F.fai_text(rows) == b"x\t6\t9\t4\t6\ny\t2\t23\t2\t4\nz\t0\t30\t0\t0\n"
    assert [F.fetch(text, r) for r in rows] == [b"ACGTAC", b"GG", b""]
    assert [F.raw_span(r) for r in rows] == [8, 2, 0]
    assert F.fold(b"acgtnNRY-*\x00\xe4>") == b"ACGTNNNN-NNNN"
    assert F.composition([b"AACGT-N", b""]).tolist() == [[2, 1, 1, 1], [0, 0, 0, 0]]


@pytest.mark.parametrize("eol", ["LF", "CRLF"])
def test_the_first_boundary_of_phase_visits_every_kind_of_byte(eol):
    kinds = set(F.PHASE_KINDS) - ({"cr"} if eol == "LF" else set())
    for group in (F.cases("phase"), F.twins("phase")):
        for width in F.PHASE_WIDTHS:
            mine = [x for x in group if x.label.startswith("width %d, %s," % (width, eol))]
            seen = set()
            for case in mine:
                at = F.boundary(case)
                assert case.kind in F.byte_kinds(case, at), (case, at, F.byte_kinds(case, at))
                seen.add(case.kind)
                if case.kind == "raw_end":
                    assert at == len(case.text) and not case.text.endswith(b"\n")
                else:
                    # a sequence follows the boundary: a second piece (slab) is launched
                    assert (len(F.pieces(case)) if case.block is None else len(F.slabs(case))) >= 2, case
                # the first wanted sequence starts the pieces
                assert F.wanted_rows(case)[0][0] == "p" and ("\r\n" in case.text.decode("latin-1")) == (eol == "CRLF")
            assert seen == kinds, (width, eol, seen)
    plain = F.cases("phase")
    assert all(F.boundary(x) == F.wanted_rows(x)[0][2] + F.PIECE for x in plain)


def _units(case):
    """Per sixteen-byte unit of the file, counted from the first wanted byte: (non-empty wanted sequences with a base in it —
    a lane of the strip kernel steps from each to the next —, empty wanted sequences whose place is in it)."""
    rows = {r[0]: r for r in case.fai}
    lo = F.wanted_rows(case)[0][2]
    full, empty = {}, {}
    for r in (rows[n] for n in case.order if n in rows):
        if r[1] == 0:
            empty[(r[2] - lo) // 16] = empty.get((r[2] - lo) // 16, 0) + 1
        for u in sorted(set((F.offsets(r) - lo) // 16)):
            full[int(u)] = full.get(int(u), 0) + 1
    return full, empty


def test_crowded_puts_three_sequences_and_an_empty_one_into_a_unit():
    hits = 0
    ends_in_a_chunk = 0
    for case in F.cases("crowded"):
        assert 200 <= len(case.fai) <= 400 and all(0 <= r[1] <= 3 and 1 <= len(r[0]) <= 3 for r in case.fai)
        full, empty = _units(case)
        hits += sum(1 for u, n in full.items() if n >= 3 and empty.get(u, 0) >= 1)
        # ... and of the genome: contig ends per sixteen bases, empty contigs in front, in the middle, at the end, in a row
        lens = np.asarray([len(s) for s in F.sequences(case)])
        ends = np.cumsum(lens)
        ends_in_a_chunk = max(ends_in_a_chunk, int(np.bincount(ends // 16).max()))
        if "all" in case.label:
            zero = "".join("0" if n == 0 else "1" for n in lens)
            assert "000" in zero and "101" in zero
    assert hits >= 3
    assert ends_in_a_chunk >= 12
    labels = [x.label for x in F.cases("crowded")]
    assert all(any(w in x for x in labels) for w in ("all wanted", "every other one wanted", "only the last wanted"))
    assert any(len(F.sequences(x)[0]) == 0 for x in F.cases("crowded")) and any(len(F.sequences(x)[-1]) == 0 for x in F.cases("crowded"))
    # shuffled against the file's order
    for case in F.cases("crowded"):
        at = [r[2] for n in case.order for r in case.fai if r[0] == n]
        assert "only the last" in case.label or at != sorted(at)


def test_geometry_has_every_line_shape():
    shapes = set()
    for case in F.cases("geometry"):
        g = [r for r in case.fai if r[0] == "g"][0]
        assert b">g the line shape" in case.text              # a description behind the name
        at_eof = g[2] + F.raw_span(g) == len(case.text)
        shapes.add((g[3], g[4] - g[3], "full" if g[1] % g[3] == 0 else "short", at_eof))
        if g[4] == g[3]:
            assert at_eof and g[1] == g[3]
    P = F.PIECE
    for lb in (1, 2, 15, 16, 17, 60, P - 1, P, P + 1):
        assert (lb, 0, "full", True) in shapes
        for end in (1, 2):
            for at_eof in (False, True):
                assert (lb, end, "full", at_eof) in shapes
                # (a line of one base has no shorter last line)
                assert lb == 1 or (lb, end, "short", at_eof) in shapes
    assert any(x.piece is None for x in F.cases("geometry")) and any(x.piece for x in F.cases("geometry"))


def test_alphabet_puts_every_value_into_every_place_of_a_unit():
    for case in F.cases("alphabet"):
        row = [r for r in case.fai if r[0] == "sym"][0]
        lo = F.wanted_rows(case)[0][2]
        at = F.offsets(row)
        values = np.frombuffer(case.text, np.uint8)[at]
        seen = np.zeros((256, 16), bool)
        seen[values, (at - lo) % 16] = True
        assert seen[F.alphabet_values()].all(), case
        assert not seen[[10, 13]].any()
        # '>' only away from a line's start
        text = np.frombuffer(case.text, np.uint8)
        assert not (text[at[values == ord(">")] - 1] == 10).any()


def test_tail_sees_all_sixteen_residues():
    total, last, pieces = set(), set(), set()
    for case in F.cases("tail"):
        n = sum(len(s) for s in F.sequences(case))
        p = F.pieces(case)
        total.add((n % 16, len(p) > 1))
        last.add((p[-1][1] % 16, len(p) > 1))
        pieces.add(len(p))
    assert total == {(r, far) for r in range(16) for far in (False, True)}
    assert last == {(r, far) for r in range(16) for far in (False, True)}
    assert pieces >= {1, 2}


def test_every_gaps_case_leaves_a_piece_on_disk():
    for case in F.cases("gaps"):
        p = F.pieces(case)
        assert sum(1 for _, _, any_wanted in p if not any_wanted) >= 1 and sum(1 for _, _, any_wanted in p if any_wanted) >= 2, case
        spans = sorted((r[2], r[2] + F.raw_span(r)) for r in F.wanted_rows(case))
        assert max(b[0] - a[1] for a, b in zip(spans, spans[1:])) > 2 * F.PIECE
    for case in F.twins("gaps"):
        used = sum(len(s) for s in F.slabs(case))
        assert 0 < used < len(F.block_bounds(case)) - 1 and len(F.slabs(case)) >= 2, case


def test_overlap_rows_share_bytes_or_touch():
    for case in F.cases("overlap"):
        spans = sorted((r[2], r[2] + F.raw_span(r)) for r in F.wanted_rows(case))
        shared = any(b[0] < a[1] for a, b in zip(spans, spans[1:]))
        assert shared == (case.label != "touching")
        if case.label == "touching":
            assert spans[0][1] == spans[1][0]
        # faidx serves every row
        assert all(len(s) == r[1] and set(s) <= set(b"ACGT") for s, r in zip(F.sequences(case), [dict((x[0], x) for x in case.fai)[n] for n in case.order]))
