"""The yardstick of --write-index, from the SAM specification (sections 4.2, 5.2, 5.3) and nothing of the product's: a BAI
parser, a builder that derives the index from a written BAM file alone — its BGZF members with their file offsets, its records
with their places in the inflated data, and the rule the issue states (what hts_idx_push records, before any compaction) —, and
a region query through an index: reg2bins, the chunks that end above the linear index's offset, a BGZF reader positioned at a
virtual offset, records filtered by overlap.

The rule, once more:
  extent      [pos, end), end = pos + max(1, reference bases of the CIGAR: M D N = X)
  bin         reg2bin(pos, end)
  chunk       a maximal run of consecutive records with the same (tid, bin): first record's start offset, last one's end offset
  linear      ioffset[w] = the start offset of the first record that touches window w (16 KiB); n_intv = highest touched + 1;
              an untouched window below takes the next touched one above
  pseudo-bin  37450: (first start, last end), (records, 0)
  offsets     coffset << 16 | uoffset; the end of a member is the start of the next one
  file        magic, n_ref, per reference the bins ascending with 37450 last, then the intervals; n_no_coor = 0 at the end"""

import bisect
import struct
import zlib

PSEUDO_BIN = 37450
CONSUMES_REFERENCE = (0, 2, 3, 7, 8)        # M D N = X


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, offset in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += range(offset + (beg >> shift), offset + (end >> shift) + 1)
    return bins


def cigar_span(cigar):
    """Reference bases of a list of BAM CIGAR words."""
    return sum(c >> 4 for c in cigar if c & 15 in CONSUMES_REFERENCE)


def extent_end(pos, cigar):
    return pos + max(1, cigar_span(cigar))


# ---------------------------------------------------------------------- the file
class Bam:
    """A BAM file taken apart: ``members`` [(file offset, compressed size, start in the inflated data, inflated size)], the
    header's ``names`` and ``lengths``, and ``records``: dicts with tid, pos, end, flag, name, ``start`` / ``stop`` (places in the
    inflated data), ``bytes``."""

    def __init__(self, path):
        self.data = open(path, "rb").read()
        self.members, chunks, at, u = [], [], 0, 0
        while at < len(self.data):
            assert self.data[at:at + 4] == b"\x1f\x8b\x08\x04" and self.data[at + 12:at + 16] == b"BC\x02\x00", at
            size = struct.unpack_from("<H", self.data, at + 16)[0] + 1
            raw = zlib.decompress(self.data[at:at + size], 31)
            self.members.append((at, size, u, len(raw)))
            chunks.append(raw)
            at += size
            u += len(raw)
        assert at == len(self.data) and self.members and self.members[-1][3] == 0, "no end-of-file marker"
        self.stream = s = b"".join(chunks)
        self.ustarts = [m[2] for m in self.members]
        assert s[:4] == b"BAM\x01"
        at = 8 + struct.unpack_from("<i", s, 4)[0]
        n_ref = struct.unpack_from("<i", s, at)[0]
        at += 4
        self.names, self.lengths = [], []
        for _ in range(n_ref):
            l_name = struct.unpack_from("<i", s, at)[0]
            self.names.append(s[at + 4:at + 3 + l_name].decode())
            self.lengths.append(struct.unpack_from("<i", s, at + 4 + l_name)[0])
            at += 8 + l_name
        self.header_bytes = at
        self.records = []
        while at < len(s):
            self.records.append(self.record_at(at))
            at = self.records[-1]["stop"]
        assert at == len(s)

    def record_at(self, at):
        s = self.stream
        size, tid, pos, l_name, _mapq, _bin, n_cigar, flag = struct.unpack_from("<iiiBBHHH", s, at)
        assert size >= 32 and at + 4 + size <= len(s)
        cigar = struct.unpack_from("<%dI" % n_cigar, s, at + 36 + l_name)
        return dict(tid=tid, pos=pos, end=extent_end(pos, cigar), flag=flag, name=s[at + 36:at + 35 + l_name].decode("latin-1"),
                    start=at, stop=at + 4 + size, bytes=s[at:at + 4 + size])

    def virtual(self, u):
        """The virtual offset of place ``u`` of the inflated data: in the member whose data holds that byte — at the end of a
        member's data, the next member (the end-of-file marker after the last)."""
        m = bisect.bisect_right(self.ustarts, u) - 1
        # (members without data other than the marker would make this ambiguous: the writers under test make none)
        assert all(size > 0 for _, _, _, size in self.members[:-1])
        return self.members[m][0] << 16 | (u - self.members[m][2])


def build_index(bam):
    """The expected BAI bytes of a ``Bam``."""
    refs = [dict(bins={}, order=[], linear={}, first=None, last=None, n=0) for _ in bam.lengths]
    prev = None
    for r in bam.records:
        tid, pos, end = r["tid"], r["pos"], r["end"]
        assert 0 <= tid < len(refs) and 0 <= pos and end <= bam.lengths[tid] and end <= 1 << 29, "a record the rule cannot place"
        assert prev is None or (prev[0], prev[1]) <= (tid, pos), "records out of order"
        b = reg2bin(pos, end)
        beg_v, end_v = bam.virtual(r["start"]), bam.virtual(r["stop"])
        ref = refs[tid]
        if prev is not None and prev[0] == tid and prev[2] == b:
            chunks = ref["bins"][b]
            chunks[-1] = (chunks[-1][0], end_v)             # the run goes on
        else:
            ref["bins"].setdefault(b, []).append((beg_v, end_v))
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            ref["linear"].setdefault(w, beg_v)
        if ref["first"] is None:
            ref["first"] = beg_v
        ref["last"] = end_v
        ref["n"] += 1
        prev = (tid, pos, b)
    out = [b"BAI\x01", struct.pack("<i", len(refs))]
    for ref in refs:
        if ref["n"] == 0:
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", len(ref["bins"]) + 1))
        for b in sorted(ref["bins"]):
            out.append(struct.pack("<Ii", b, len(ref["bins"][b])))
            out += [struct.pack("<QQ", *c) for c in ref["bins"][b]]
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, ref["first"], ref["last"], ref["n"], 0))
        n_intv = max(ref["linear"]) + 1
        offsets, above = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            above = ref["linear"].get(w, above)
            offsets[w] = above
        out.append(struct.pack("<i%dQ" % n_intv, n_intv, *offsets))
    out.append(struct.pack("<Q", 0))
    return b"".join(out)


def parse_index(data):
    """[(bins {bin: [(beg, end)]} in file order, [ioffset])] per reference; every byte accounted for."""
    assert data[:4] == b"BAI\x01"
    n_ref = struct.unpack_from("<i", data, 4)[0]
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, at)[0]
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at)
            at += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
        n_intv = struct.unpack_from("<i", data, at)[0]
        at += 4
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, data, at))))
        at += 8 * n_intv
    assert struct.unpack_from("<Q", data, at)[0] == 0 and at + 8 == len(data)
    return refs


# ---------------------------------------------------------------------- a reader through the index
class BgzfReader:
    def __init__(self, data):
        self.data = data
        self.block_at, self.block, self.within, self.next_at = 0, b"", 0, 0

    def seek(self, voffset):
        self._load(voffset >> 16)
        self.within = voffset & 0xFFFF
        assert self.within <= len(self.block)

    def _load(self, at):
        size = struct.unpack_from("<H", self.data, at + 16)[0] + 1
        self.block_at, self.block, self.within, self.next_at = at, zlib.decompress(self.data[at:at + size], 31), 0, at + size

    def tell(self):
        """bgzf_tell: at the end of a block's data, the next block."""
        if self.within == len(self.block):
            return self.next_at << 16
        return self.block_at << 16 | self.within

    def read(self, n):
        out = b""
        while len(out) < n:
            if self.within == len(self.block):
                assert self.next_at < len(self.data), "read past the end of the file"
                self._load(self.next_at)
                continue
            piece = self.block[self.within:self.within + n - len(out)]
            self.within += len(piece)
            out += piece
        return out


def query(bam, index, tid, beg, end):
    """The records (their bytes, in file order) of ``bam`` that overlap [beg, end) of reference ``tid``, found through the parsed
    ``index`` alone."""
    bins, linear = index[tid]
    w = beg >> 14
    min_offset = linear[w] if w < len(linear) else 0
    chunks = sorted(c for b in reg2bins(beg, end) for c in bins.get(b, []) if c[1] > min_offset)
    reader, out = BgzfReader(bam.data), []
    for c_beg, c_end in chunks:
        reader.seek(c_beg)
        while reader.tell() < c_end:
            head = reader.read(4)
            body = reader.read(struct.unpack("<i", head)[0])
            r_tid, pos, l_name, _mapq, _bin, n_cigar = struct.unpack_from("<iiBBHH", body, 0)
            cigar = struct.unpack_from("<%dI" % n_cigar, body, 32 + l_name)
            if r_tid == tid and pos < end and extent_end(pos, cigar) > beg:
                out.append(head + body)
        assert reader.tell() == c_end, "a chunk does not end where a record does"
    return out


def brute(bam, tid, beg, end):
    return [r["bytes"] for r in bam.records if r["tid"] == tid and r["pos"] < end and r["end"] > beg]
