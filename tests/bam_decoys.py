"""BAM files that mislead the device decoder's record scan (csrc/mdx_gbam.hip gbam_scan_kernel), assembled byte by byte from
the SAM/BAM specification with numpy, struct and zlib, deterministic from a seed, together with the truth they were built
from.  A builder: it collects no tests (tests/test_bam_decoys.py checks the fixtures on the host, tests/test_gpu_bam_scan.py
runs them through the device path).

True records carry POS = their index in the file, so any slab of records is located in the truth by its first POS.

A DECOY IMAGE is a byte string that passes every test of the scan's plausibility rule for this header — a block_size that
holds the sizes behind it, reference ids of the dictionary, POS >= DECOY_POS (no true record has one), a read name that ends
in NUL — and whose block_size leads to the next image.  Images travel inside true records as the payload of a ZD:B:C array:
the file stays a valid BAM file that every decoder reads as one record with one long tag.  The carriers:

  a   six images at the very end of the carrier: the decoy chain lands exactly on the next true record
  b   images followed by bytes that are no record: the decoy chain ends in "cannot be a record"
  c   the last image's block_size reaches 20 bytes into the next true record: the chain lands inside a true record
  d   an image whose CIGAR field is the CG placeholder <l_seq>S<n>N
  e   two images only, bytes that are no record behind them: never three records in a row

``plausible_mask`` / ``triple_starts`` restate the scan's rule in Python, from the comment above gbam_plausible and the BAM
specification: they are there to check the FIXTURES (which block's first "three records in a row" is a decoy), never the
decoder."""
import functools
import struct
import zlib

import numpy as np

EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
DECOY_POS = 1_000_000
REFS = (("chrA", 60_000), ("chrB", 30_000), ("chrC", 9_000))
READ_GROUPS = (("rg1", "s", "libA"), ("rg.2", "s", "libB"), ("r3", "s", "libA"))
LIBRARIES = [("s", "libA"), ("s", "libB")]
LIB_OF_RG = {"rg1": 0, "rg.2": 1, "r3": 0}
HEADER_TEXT = ("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
               + "".join("@RG\tID:%s\tSM:%s\tLB:%s\n" % g for g in READ_GROUPS))
RAW_HEADER = (b"BAM\x01" + struct.pack("<i", len(HEADER_TEXT)) + HEADER_TEXT.encode() + struct.pack("<i", len(REFS))
              + b"".join(struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln) for n, ln in REFS))
SEQ_LETTERS = np.frombuffer(b"=ACMGRSVTWYHKDBN", np.uint8)
DROP_BITS = (0x4, 0x100, 0x200, 0x400, 0x800)
BLOCK = 3001                                     # the uniform cut of the decoy files
IMAGE_BASES = 20
JUNK = b"\xff" * 48                              # no record: a block_size of 0xFFFFFFFF wherever one is read in it
FILLER = b"\xff" * 64


def genome(seed=3):
    """The sequences of REFS: random ACGT (what the reads hold does not have to agree with them)."""
    rng = np.random.default_rng(seed)
    return [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)]) for _, ln in REFS]


# ------------------------------------------------------------------------------------------------ records
def _aux_others(i, rng, every=False):
    """Aux fields of every type (SAMv1 4.2.4), three of them in turn or all."""
    small = int(rng.integers(0, 5))
    fields = [b"XAA" + bytes([33 + i % 90]), b"Xcc" + struct.pack("<b", -(i % 100)), b"XCC" + struct.pack("<B", i % 256),
              b"Xss" + struct.pack("<h", -(i % 30000)), b"XSS" + struct.pack("<H", (i * 7) % 65536),
              b"Xii" + struct.pack("<i", -70000 - i), b"XII" + struct.pack("<I", 3_000_000_000 + i), b"Xff" + struct.pack("<f", i / 8.0),
              b"XZZ" + bytes(33 + int(v) for v in rng.integers(0, 90, i % 23)) + b"\0", b"XHH" + b"1AE3" * (i % 3) + b"\0",
              b"YcBc" + struct.pack("<i", small) + bytes(rng.integers(0, 256, small, dtype=np.uint8)),
              b"YCBC" + struct.pack("<i", small) + bytes(rng.integers(0, 256, small, dtype=np.uint8)),
              b"YsBs" + struct.pack("<i", small) + bytes(rng.integers(0, 256, 2 * small, dtype=np.uint8)),
              b"YSBS" + struct.pack("<i", small) + bytes(rng.integers(0, 256, 2 * small, dtype=np.uint8)),
              b"YiBi" + struct.pack("<i", small) + bytes(rng.integers(0, 256, 4 * small, dtype=np.uint8)),
              b"YIBI" + struct.pack("<i", small) + bytes(rng.integers(0, 256, 4 * small, dtype=np.uint8)),
              b"YfBf" + struct.pack("<i", small) + struct.pack("<%df" % small, *[k / 4.0 for k in range(small)])]
    if every:
        return fields
    return [fields[(i + k * 5) % len(fields)] for k in range(3)]


def _cigar_for(i, l_seq):
    """0 to four operations that consume exactly l_seq bases of the read; (operations, reference bases)."""
    M, I, D, N, S = 0, 1, 2, 3, 4
    shape = i % 6
    if l_seq == 0 or shape == 0:
        return [], 0
    if l_seq < 12 or shape == 1:
        return [l_seq << 4 | M], l_seq
    a = 3 + i % 5
    if shape == 2:
        return [a << 4 | S, (l_seq - a) << 4 | M], l_seq - a
    if shape == 3:
        return [a << 4 | M, 1 << 4 | I, (l_seq - a - 1) << 4 | M], l_seq - 1
    if shape == 4:
        return [a << 4 | M, 2 << 4 | D, (l_seq - a) << 4 | M], l_seq + 2
    return [a << 4 | M, 3 << 4 | N, (l_seq - a - 2) << 4 | M, 2 << 4 | S], l_seq + 1


def make_record(i, rng, l_seq=None, min_seq=0, payload=None, rg_front=None, nib=None, qual=None, flag=None):
    """True record ``i`` (POS = i) with its block_size, and what it was built from.  ``payload``: the bytes of a ZD:B:C array
    (a carrier); ``rg_front``: the RG tag in front of (True) or behind (False) the other fields."""
    if l_seq is None:
        l_seq = i // 4 % 25 if i % 4 == 0 else 25 + (i * 13) % 120
        l_seq = max(l_seq, min_seq)
    tid = i % 3 if i + 400 < REFS[i % 3][1] else 0
    l_name = (i * 37) % 255 + 1
    name = bytes(33 + int(v) for v in rng.integers(0, 94, l_name - 1))
    cigar, _ = _cigar_for(i, l_seq)
    if nib is None:
        nib = np.where(rng.random(l_seq) < 0.85, np.asarray([1, 2, 4, 8])[rng.integers(0, 4, l_seq)], rng.integers(0, 16, l_seq)).astype(np.uint8)
    if qual is None:
        qual = np.full(l_seq, 0xFF, np.uint8) if i % 7 == 3 else rng.integers(0, 46, l_seq).astype(np.uint8)
    aux_kind = i % 5 if payload is None else (1 if rg_front else 2)
    rg = None if aux_kind == 0 else READ_GROUPS[i % 3][0]
    others = _aux_others(i, rng, every=aux_kind == 4)
    if payload is not None:
        others = others[:1] + [b"ZDBC" + struct.pack("<i", len(payload)) + payload]
    rg_tag = b"" if rg is None else b"RGZ" + rg.encode() + b"\0"
    aux = {0: b"".join(others), 1: rg_tag + b"".join(others), 2: b"".join(others) + rg_tag, 3: rg_tag,
           4: b"".join(others[:9]) + rg_tag + b"".join(others[9:])}[aux_kind]
    if flag is None:
        flag = 0x10 * (i % 2)
        # what a run cannot count is not kept: no operations, no bases, no read group; and every eleventh record
        if not cigar or rg is None or i % 11 == 5:
            flag |= DROP_BITS[i % 5] | (0x1 if i % 3 == 0 else 0)
    # (no mate on the first sequence: the last three bytes of a record, the block_size behind them and a record of refID 0,
    # next_refID 0 look like one record of 2^24 bytes and more, whose chain leaves the data — nothing speaks against it)
    mtid, mpos, tlen = (-1, -1, 0) if i % 4 else (tid or 1, i + 7, 150 - i % 300)
    pad = np.append(nib, 0).astype(np.uint8) if l_seq % 2 else np.asarray(nib, np.uint8)
    packed = (pad[0::2] << 4 | pad[1::2]).astype(np.uint8)          # (the high nibble of a byte is the earlier base)
    fixed = struct.pack("<iiBBHHHiiii", tid, i, l_name, i % 61, 4680, len(cigar), flag, l_seq, mtid, mpos, tlen)
    parts, body = {}, b""
    for key, piece in (("fixed", fixed), ("name", name + b"\0"), ("cigar", struct.pack("<%dI" % len(cigar), *cigar)),
                       ("nibbles", bytes(packed)), ("qual", bytes(qual)), ("tags", aux)):
        parts[key] = (4 + len(body), 4 + len(body) + len(piece))
        body += piece
    truth = dict(flag=flag, tid=tid, pos=i, tlen=tlen, mtid=mtid, mpos=mpos, cigar=cigar, nib=nib, qual=np.asarray(qual, np.uint8),
                 name=name.decode(), rg=rg, parts=parts)
    if payload is not None:
        truth["payload_at"] = 4 + len(body) - len(aux) + aux.index(b"ZDBC") + 8
    return struct.pack("<i", len(body)) + body, truth


def image(k, reach=0, cg=False):
    """Decoy image ``k``; ``reach``: bytes behind the image that its block_size takes in as well."""
    name = b"decoy%04d\0" % (k % 10000)
    cigar = [IMAGE_BASES << 4 | 4, 77 << 4 | 3] if cg else [IMAGE_BASES << 4]
    body = (struct.pack("<iiBBHHHiiii", 0, DECOY_POS + k, len(name), 30, 4680, len(cigar), 0, IMAGE_BASES, -1, -1, 0) + name
            + struct.pack("<%dI" % len(cigar), *cigar) + b"\x12\x48" * (IMAGE_BASES // 4) + bytes([30]) * IMAGE_BASES + b"RGZrg1\0")
    return struct.pack("<i", len(body) + reach) + body


def payload_of(kind, n_images, behind=0):
    """(payload, offsets of its images in it).  ``behind``: the bytes of the carrier behind the payload (kind c: the last image
    reaches over them and 20 bytes into the next record)."""
    if kind == "e":
        n_images = 2
    images = [image(k, cg=(kind == "d" and k % 3 == 1)) for k in range(n_images)]
    tail = b"" if kind == "a" else JUNK
    if kind == "c":
        images[-1] = image(n_images - 1, reach=len(tail) + behind + 20)
    offs, at = [], len(FILLER)
    for im in images:
        offs.append(at)
        at += len(im)
    return FILLER + b"".join(images) + tail, offs


# ------------------------------------------------------------------------------------------------ files
class Built:
    """One file: its inflated bytes, where they are cut, and the truth."""

    def __init__(self, name, bodies, truths, cuts=None, empties=None, decoys=()):
        self.name, self.records, self.truths = name, bodies, truths
        self.stream = RAW_HEADER + b"".join(bodies)
        self.total = len(self.stream)
        self.starts = np.cumsum([len(RAW_HEADER)] + [len(b) for b in bodies])[:-1].astype(np.int64)
        self.cuts = sorted(set(int(c) for c in (cuts or []) if 0 < c < self.total))
        self.empties = dict(empties or {})          # offset in the inflated stream -> empty members in front of it
        self.decoys = list(decoys)                  # (kind, record, offset of the first image behind the planted cut)
        t = truths
        self.n = len(t)
        self.flag = np.asarray([r["flag"] for r in t], np.uint16)
        for key in ("tid", "pos", "tlen", "mtid", "mpos"):
            setattr(self, key, np.asarray([r[key] for r in t], np.int32))
        self.cigar_off = np.concatenate([[0], np.cumsum([len(r["cigar"]) for r in t])]).astype(np.uint32)
        self.cigar = np.asarray([c for r in t for c in r["cigar"]], np.uint32)
        self.seq_off = np.concatenate([[0], np.cumsum([len(r["nib"]) for r in t])]).astype(np.uint32)
        self.nib = np.concatenate([r["nib"] for r in t] + [np.zeros(0, np.uint8)]).astype(np.uint8)
        self.seq = SEQ_LETTERS[self.nib]
        self.qual = np.concatenate([r["qual"] for r in t] + [np.zeros(0, np.uint8)]).astype(np.uint8)
        self.names = [r["name"] for r in t]
        self.rg = [r["rg"] for r in t]
        self.lib = np.asarray([0xFFFF if g is None else LIB_OF_RG[g] for g in self.rg], np.uint16)
        self.ends = self.starts + np.asarray([len(b) for b in bodies], np.int64)

    def blocks(self):
        """[lo, hi) of the BGZF members that hold data, in the inflated stream."""
        edges = [0] + self.cuts + [self.total]
        return list(zip(edges[:-1], edges[1:]))

    def write(self, path):
        """The BGZF file: a member per piece between two cuts, empty members where ``empties`` says, the end-of-file marker."""
        def member(chunk):
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            body = c.compress(chunk) + c.flush()
            assert len(chunk) <= 65536 and len(body) + 26 <= 65536
            return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body
                    + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
        with open(path, "wb") as out:
            for lo, hi in self.blocks():
                out.write(member(b"") * self.empties.get(lo, 0))
                out.write(member(self.stream[lo:hi]))
            out.write(member(b"") * self.empties.get(self.total, 0))
            out.write(EOF_MARKER)
        return path

    # ---- the scan's rule over this file's bytes
    @functools.cached_property
    def triples(self):
        return triple_starts(self.stream, len(REFS))

    def guess(self, lo, hi):
        """The first offset of [lo, hi) at which three plausible records follow one another, or None."""
        t = self.triples
        k = int(np.searchsorted(t, lo))
        return int(t[k]) if k < len(t) and t[k] < hi else None

    def false_starts(self):
        """The members that hold the start of a true record and whose guess is another offset: (lo, hi, guess, true start)."""
        out = []
        for lo, hi in self.blocks():
            k = int(np.searchsorted(self.starts, lo))
            if lo >= len(RAW_HEADER) and k < self.n and self.starts[k] < hi and self.guess(lo, hi) != int(self.starts[k]):
                out.append((lo, hi, self.guess(lo, hi), int(self.starts[k])))
        return out


def _uniform(total, step, keep_out=()):
    return [c for c in range(step, total, step) if not any(a <= c < b for a, b in keep_out)]


def htslib_cuts(built_starts, header_len, total, limit=0xFF00):
    """htslib's layout: the header in members of its own, every other member starts at a record."""
    cuts, lo = [header_len], header_len
    starts = list(built_starts) + [total]
    for a, b in zip(starts[:-1], starts[1:]):
        if b - lo > limit:
            cuts.append(int(a))
            lo = a
    return cuts


@functools.lru_cache(maxsize=None)
def plain(layout="htslib", n=1500, seed=1):
    """Decoy-free records: htslib's layout, or the stream cut every ``layout`` bytes."""
    rng = np.random.default_rng(seed)
    made = [make_record(i, rng) for i in range(n)]
    b = Built("plain_%s" % layout, [m[0] for m in made], [m[1] for m in made])
    if layout == "htslib":
        b.cuts = htslib_cuts(b.starts, len(RAW_HEADER), b.total, limit=20_000)
    else:
        b.cuts = _uniform(b.total, int(layout))
    return b


@functools.lru_cache(maxsize=None)
def decoys(kind, where, n=1500, seed=2):
    """Carriers of one kind among plain records.  ``where``: "front" — a cut inside the carrier, in front of the first image;
    "mid" — the cut inside the third of six images, three behind it; "long" — carriers of ten members of BLOCK bytes, cut
    uniformly: whole members inside them hold decoy chains."""
    rng = np.random.default_rng(seed + 17 * "abcde".index(kind) + 101 * ("front", "mid", "long").index(where))
    every, n_images = (400, 10 * BLOCK // len(image(0))) if where == "long" else (150, 6 if where == "mid" or kind == "a" else 3)
    bodies, truths, planted = [], [], []
    for i in range(n):
        if i % every != every // 2:
            body, t = make_record(i, rng)
        else:
            rg_front = kind == "a"
            behind = 0 if rg_front else len(b"RGZ" + READ_GROUPS[i % 3][0].encode() + b"\0")
            payload, offs = payload_of(kind, n_images, behind)
            body, t = make_record(i, rng, payload=payload, rg_front=rg_front)
            planted.append((i, [t["payload_at"] + o for o in offs]))
        bodies.append(body)
        truths.append(t)
    b = Built("%s_%s" % (kind, where), bodies, truths)
    if where == "long":
        b.cuts = _uniform(b.total, BLOCK)
        # (the first image a member inside the carrier can guess: the first one that starts in it)
        for i, offs in planted:
            first = [int(b.starts[i]) + o for o in offs]
            lo = next(c for c in b.cuts if c > first[0])
            b.decoys.append((kind, i, next(o for o in first if o >= lo)))
    else:
        spans = [(int(b.starts[i]), int(b.starts[i]) + len(bodies[i]) + 400) for i, _ in planted]
        cuts = _uniform(b.total, BLOCK, keep_out=spans)
        for i, offs in planted:
            s = int(b.starts[i])
            if where == "front" or kind == "e":
                cuts.append(s + offs[0] - 17)
                b.decoys.append((kind, i, s + offs[0]))
            else:
                cuts.append(s + offs[2] + 11)
                b.decoys.append((kind, i, s + offs[3]))
        b.cuts = sorted(cuts)
    return b


@functools.lru_cache(maxsize=None)
def mixed(n=1500, seed=5):
    """Every record a carrier of kind a (bases for a tabulation: 25 and more), cut uniformly: most members begin with a false
    start."""
    rng = np.random.default_rng(seed)
    payload, offs = payload_of("a", 6)
    made = [make_record(i, rng, min_seq=25, payload=payload, rg_front=True) for i in range(n)]
    b = Built("mixed", [m[0] for m in made], [m[1] for m in made])
    b.cuts = _uniform(b.total, BLOCK)
    b.decoys = [("a", i, int(b.starts[i]) + made[i][1]["payload_at"] + offs[0]) for i in range(n)]
    return b


@functools.lru_cache(maxsize=None)
def phases(n=420, seed=7):
    """Decoy-free records cut at every phase of a record — 0 to 3 bytes into a block_size field, inside the fixed 32 bytes, the
    name, the CIGAR, the nibbles, the qualities, the tags; the last cut fewer than 36 bytes before the end of the data — with
    empty members in front of the first record, between two records, inside a record, twice in a row and in front of the
    end-of-file marker."""
    rng = np.random.default_rng(seed)
    made = [make_record(i, rng) for i in range(n)]
    b = Built("phases", [m[0] for m in made], [m[1] for m in made])
    cuts, where = [len(RAW_HEADER)], []
    for k, i in enumerate(range(2, n - 2, 3)):
        parts, s = made[i][1]["parts"], int(b.starts[i])
        if k % 12 < 4:
            at = k % 12
        else:
            key = ("fixed", "fixed", "fixed", "name", "cigar", "nibbles", "qual", "tags")[k % 12 - 4]
            lo, hi = parts[key]
            at = lo if hi == lo else lo + (k * 5 + (9, 16, 31, 0, 1, 0, 2, 3)[k % 12 - 4]) % (hi - lo)
        cuts.append(s + at)
        where.append((i, at))
    cuts.append(b.total - 20)
    b.cuts = sorted(set(c for c in cuts if 0 < c < b.total))
    b.cut_phases = where
    inside = int(b.starts[201]) + made[201][1]["parts"]["qual"][0] + 5
    b.cuts = sorted(set(b.cuts) | {inside, int(b.starts[5]), int(b.starts[8])})
    b.empties = {len(RAW_HEADER): 1, int(b.starts[5]): 1, inside: 1, int(b.starts[8]): 2, b.total: 1}
    assert all(o in b.cuts or o == b.total for o in b.empties)
    return b


SHORT_THRESHOLD = 20


@functools.lru_cache(maxsize=None)
def short_sequences(seed=9):
    """Records of every l_seq from 0 to 24, each length at both nibble parities of seq_off (a record of one base in front of it
    where the parity has to flip), all sixteen nibble codes among the bases; qualities one below, at and above SHORT_THRESHOLD
    in three rotations, or 0xFF."""
    rng = np.random.default_rng(seed)
    made, bases = [], 0
    for mode in range(4):
        for parity in (0, 1):
            for l_seq in range(25):
                want = [l_seq] if bases % 2 == parity else [1, l_seq]
                for ln in want:
                    i = len(made)
                    t = np.arange(ln)
                    nib = ((t * 7 + l_seq + mode) % 16).astype(np.uint8)
                    qual = np.full(ln, 0xFF, np.uint8) if mode == 3 else (SHORT_THRESHOLD - 1 + (t + mode) % 3).astype(np.uint8)
                    made.append(make_record(i, rng, l_seq=ln, nib=nib, qual=qual, rg_front=True) + (bases % 2,))
                    bases += ln
    b = Built("short", [m[0] for m in made], [m[1] for m in made])
    b.cuts = htslib_cuts(b.starts, len(RAW_HEADER), b.total)
    b.parities = {(len(m[1]["nib"]), m[2]) for m in made}
    return b


# ------------------------------------------------------------------------------------------------ the scan's rule, restated
def _u32_at(d, offs):
    o = np.asarray(offs, np.int64)
    return d[o].astype(np.int64) | d[o + 1].astype(np.int64) << 8 | d[o + 2].astype(np.int64) << 16 | d[o + 3].astype(np.int64) << 24


def plausible_mask(stream, n_ref):
    """For every offset o with o + 36 <= len(stream): do the bytes look like the start of a BAM record?  The fields a writer
    cannot choose freely (SAMv1 4.2): block_size between the 32 fixed bytes and 2^28 and no smaller than what the record must
    hold — 32 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq —, refID and next_refID in [-1, n_ref), pos and next_pos
    >= -1, l_read_name >= 1 and the name's last byte NUL (where the data holds that byte), l_seq no negative number."""
    d = np.frombuffer(stream, np.uint8)
    total = len(d)
    o = np.arange(max(0, total - 35), dtype=np.int64)

    def s32(at):
        v = _u32_at(d, o + at)
        return np.where(v >= 1 << 31, v - (1 << 32), v)
    bs, tid, pos, l_seq, mtid, mpos = s32(0), s32(4), s32(8), s32(20), s32(24), s32(28)
    l_name = d[o + 12].astype(np.int64)
    n_cigar = d[o + 16].astype(np.int64) | d[o + 17].astype(np.int64) << 8
    ok = (bs >= 32) & (bs <= 1 << 28) & (tid >= -1) & (tid < n_ref) & (mtid >= -1) & (mtid < n_ref) & (pos >= -1) & (mpos >= -1)
    ok &= (l_name >= 1) & (l_seq >= 0) & (32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq <= bs)
    nul = o + 36 + l_name - 1
    ok &= (nul >= total) | (d[np.minimum(nul, total - 1)] == 0)
    return ok, bs


def triple_starts(stream, n_ref):
    """The sorted offsets at which three plausible records follow one another — block_size leading from each to the next — as
    far as the data can say: where fewer than 36 bytes are left nothing speaks against a record."""
    ok, bs = plausible_mask(stream, n_ref)
    total, visible = len(stream), len(ok)
    out = []
    for o in np.flatnonzero(ok):
        at, good = int(o), True
        for _ in range(3):
            if at >= visible:           # (the fixed part does not lie inside the data)
                break
            if not ok[at]:
                good = False
                break
            at += 4 + int(bs[at])
            if at > total:
                break
        if good:
            out.append(int(o))
    return np.asarray(out + list(range(visible, total)), np.int64)
