"""The fixtures of tests/bam_decoys.py on the host.  Every file the builder makes is an ordinary BAM file: the three host
decoders — the fallback the device path relies on — read it as its construction-time truth, one record per carrier.  And the
files do to the record scan what tests/test_gpu_bam_scan.py needs of them, by the builder's own restatement of the scan's
rule: every planted decoy is the first "three records in a row" of its BGZF member, in front of a true record's start; the
two-image carriers and the decoy-free files hold no such triple anywhere but at the start of a true record."""
import numpy as np
import pytest

from mapdamage_amd import sam
from tests import bam_decoys as D

FILES = ([("plain", lay) for lay in ("htslib", "65498", "90")]
         + [("decoys", kind, where) for kind in "abcd" for where in ("front", "mid", "long")]
         + [("decoys", "e", "front"), ("mixed",), ("phases",), ("short_sequences",)])


def built(spec):
    return getattr(D, spec[0])(*spec[1:])


def check_alignments(al, b, at=0):
    """The records of ``al`` are the truth's from record ``at`` on; returns how many."""
    k = al.batch.n
    bt = al.batch
    for key in ("flag", "tid", "pos", "tlen", "mtid", "mpos"):
        np.testing.assert_array_equal(getattr(bt, key), getattr(b, key)[at:at + k], err_msg=key)
    c0, s0 = int(b.cigar_off[at]), int(b.seq_off[at])
    np.testing.assert_array_equal(bt.cigar_off.astype(np.int64), b.cigar_off[at:at + k + 1].astype(np.int64) - c0)
    np.testing.assert_array_equal(bt.seq_off.astype(np.int64), b.seq_off[at:at + k + 1].astype(np.int64) - s0)
    nc, ns = int(bt.cigar_off[-1]), int(bt.seq_off[-1])
    np.testing.assert_array_equal(bt.cigar[:nc], b.cigar[c0:c0 + nc])
    np.testing.assert_array_equal(bt.seq[:ns], b.seq[s0:s0 + ns])
    np.testing.assert_array_equal(bt.qual[:ns], b.qual[s0:s0 + ns])
    assert [al.qname_at(i) for i in range(k)] == b.names[at:at + k]
    assert list(al.rg) == b.rg[at:at + k]
    return k


@pytest.mark.parametrize("spec", FILES, ids=lambda s: "_".join(s))
def test_host_decoders_read_the_files_as_their_truth(tmp_path, spec):
    b = built(spec)
    path = str(b.write(tmp_path / "f.bam"))
    assert check_alignments(sam.read_bam_native(path), b) == b.n
    assert check_alignments(sam.read_bam(path), b) == b.n
    at = 0
    with sam.BamStream(path, chunk_bytes=3000) as stream:
        assert stream.header.references == [r[0] for r in D.REFS]
        while (chunk := stream.next_chunk()) is not None:
            at += check_alignments(chunk, b, at)
    assert at == b.n


@pytest.mark.parametrize("spec", FILES, ids=lambda s: "_".join(s))
def test_the_files_mislead_the_scan_where_they_are_meant_to(spec):
    b = built(spec)
    assert b.n <= 5000 and b.total < 4 << 20
    true_starts = set(int(s) for s in b.starts)
    assert true_starts <= set(int(t) for t in b.triples)                  # a true record is a plausible one, every time
    blocks = b.blocks()
    assert max(hi - lo for lo, hi in blocks) <= 65536
    los = np.asarray([lo for lo, _ in blocks])
    kind = spec[1] if spec[0] == "decoys" else ("a" if spec[0] == "mixed" else None)
    if kind in (None, "e"):
        # nothing but true records looks like three records in a row (the last 35 bytes of the data say nothing either way)
        stray = [int(t) for t in b.triples if int(t) not in true_starts and t + 36 <= b.total]
        assert stray == []
        assert b.false_starts() == []
        if kind == "e":
            assert len(b.decoys) >= 5
            ok, _ = D.plausible_mask(b.stream, len(D.REFS))
            for _, i, off in b.decoys:                                     # (two images: each plausible, no triple)
                assert ok[off] and b.starts[i] < off < b.ends[i] and off not in b.triples
        return
    assert len(b.decoys) >= 3
    false = {lo: (guess, true) for lo, hi, guess, true in b.false_starts()}
    hits = 0
    for _, i, off in b.decoys:
        assert b.starts[i] < off < b.ends[i]                         # inside its carrier
        assert off in b.triples
        assert D._u32_at(np.frombuffer(b.stream, np.uint8), [off + 8])[0] >= D.DECOY_POS
        lo, hi = blocks[int(np.searchsorted(los, off, side="right")) - 1]
        if spec[0] == "decoys":
            # the member's first triple is this decoy, and the carrier ends — the next true record starts — in the same member
            assert b.guess(lo, hi) == off
            if spec[2] != "long":
                assert lo > b.starts[i] and false[lo] == (off, int(b.ends[i]))
                hits += 1
    if spec[0] == "decoys" and spec[2] == "long":
        # whole members inside a carrier, each with a decoy chain of its own; the member the carrier ends in starts falsely
        for _, i, _ in b.decoys:
            inside = [(lo, hi) for lo, hi in blocks if lo > b.starts[i] and hi < b.ends[i]]
            assert len(inside) >= 8 and all(b.guess(lo, hi) not in true_starts and b.guess(lo, hi) is not None for lo, hi in inside)
            lo = max(l for l in los if l <= b.ends[i])
            assert lo in false
            hits += 1
    if spec[0] == "mixed":
        # most members begin with a false start
        with_start = [1 for lo, hi in blocks if np.searchsorted(b.starts, lo) < np.searchsorted(b.starts, hi)]
        assert len(false) > 0.3 * len(with_start)
        hits = len(false)
    assert hits >= 3


def test_the_phases_file_cuts_where_it_says():
    b = D.phases()
    blocks = b.blocks()
    # 0, 1, 2, 3 bytes into a block_size field, and inside every part of a record
    parts = set()
    for i, at in b.cut_phases:
        assert int(b.starts[i]) + at in b.cuts
        parts.add(at if at < 4 else next(k for k, (lo, hi) in b.truths[i]["parts"].items() if lo <= at < hi or (lo == hi == at)))
    assert {0, 1, 2, 3, "fixed", "name", "cigar", "nibbles", "qual", "tags"} <= parts
    assert 0 < b.total - b.cuts[-1] < 36
    # empty members: in front of the first record, between two records, inside a record, twice in a row, in front of the marker
    starts = set(int(s) for s in b.starts)
    assert b.empties[len(D.RAW_HEADER)] == 1 and b.empties[b.total] == 1 and 2 in b.empties.values()
    assert any(o in starts and o != len(D.RAW_HEADER) for o in b.empties) and any(o not in starts and o != b.total for o in b.empties)
    assert len(blocks) > 100


def test_the_short_sequences_cover_every_length_at_both_parities():
    b = D.short_sequences()
    assert {(ln, p) for ln in range(25) for p in (0, 1)} <= b.parities
    lens = np.diff(b.seq_off.astype(np.int64))
    assert set(range(25)) <= set(lens.tolist()) and lens.max() <= 24
    for ln in range(25):
        assert {int(o) % 2 for o in b.seq_off[:-1][lens == ln]} == {0, 1}
    assert set(range(16)) <= set(b.nib.tolist())
    q = b.qual
    assert {D.SHORT_THRESHOLD - 1, D.SHORT_THRESHOLD, D.SHORT_THRESHOLD + 1, 0xFF} <= set(q.tolist())
    # the records of the general builder: every length from 0 to 24 too, names of 1 to 255 bytes, every aux type
    p = D.plain("htslib")
    assert set(range(25)) <= set(np.diff(p.seq_off.astype(np.int64)).tolist())
    assert {len(n) + 1 for n in p.names} >= {1, 2, 255}
    assert any(g is None for g in p.rg) and (p.qual == 0xFF).any() and ((p.flag & 0xF04) == 0).mean() > 0.5
