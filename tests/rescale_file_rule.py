"""What --rescale / --rescale-only writes back, in plain Python: the yardstick of tests/test_rescale_file_rule.py (CPU) and
tests/test_gpu_rescale_file.py (the route that never brings a record to the host).  Collects no tests.

The rule (mapdamage/rescale.py:266-281, :344): a record the pass rescales — routing status "single end" or "inward pair" — is
written with its QUAL field replaced, ``MR:f`` appended behind its last tag and block_size seven larger; every other record is
written byte for byte.  A rescaled record that carries a tag named MR already, of any type, stops the pass (:277-278).

Records here are what ``sam.read_bam(path, keep_raw=True).raw`` holds: the encoded record without its block_size field, which
is the length of the rest — seven bytes more *are* the block_size raised by seven (``stream_of`` writes the field).

The generator (``make_mix``) shares nothing with ``mapdamage_amd.synth``: records are encoded byte by byte here."""

import struct

import numpy as np

from mapdamage_amd.batch import Reference
from mapdamage_amd.rescale import RescaleModel

UNMAPPED, NO_QUAL, SINGLE_END, INWARD_PAIR, IMPROPER = range(5)         # rescale.py:300-342, the oracle's status
STATUS_NAMES = ("unmapped", "without_qualities", "single_end", "inward_pairs", "improper_pairs")
AUX_FIXED = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
B_ITEM = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}
L5 = L3 = 12


# ---------------------------------------------------------------------- the record's fields
def fields(body):
    tid, pos, l_name, mapq, _bin, n_cigar, flag, l_seq, mtid, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", body, 0)
    return dict(tid=tid, pos=pos, l_name=l_name, mapq=mapq, n_cigar=n_cigar, flag=flag, l_seq=l_seq, mtid=mtid, mpos=mpos, tlen=tlen)


def qual_at(body):
    """Offset of the QUAL field, and its length."""
    f = fields(body)
    return 32 + f["l_name"] + 4 * f["n_cigar"] + (f["l_seq"] + 1) // 2, f["l_seq"]


def tags_at(body):
    at, l_seq = qual_at(body)
    return at + l_seq


def walk_tags(body):
    """(name, type, first value byte, one past the last) of every aux field, over all BAM aux types.  ValueError where the
    fields do not end with the record or a type is unknown."""
    at, out = tags_at(body), []
    while at < len(body):
        if at + 3 > len(body):
            raise ValueError("a tag cut short at byte %d" % at)
        name, typ = bytes(body[at:at + 2]), bytes(body[at + 2:at + 3])
        val = at + 3
        if typ in AUX_FIXED:
            end = val + AUX_FIXED[typ]
        elif typ in (b"Z", b"H"):
            end = bytes(body).index(b"\0", val) + 1
        elif typ == b"B":
            sub = bytes(body[val:val + 1])
            count, = struct.unpack_from("<i", body, val + 1)
            end = val + 5 + count * B_ITEM[sub]
        else:
            raise ValueError("aux type %r at byte %d" % (typ, at + 2))
        if end > len(body):
            raise ValueError("tag %r runs past the record" % name)
        out.append((name, typ, val, end))
        at = end
    return out


def has_tag(body, name=b"MR"):
    return any(n == name for n, _t, _v, _e in walk_tags(body))


def mr_tag(mr_raw):
    """rescale.py:275-276: the sum printed with five decimals, read back, stored as the float32 of an ``f`` field."""
    return b"MRf" + struct.pack("<f", float("%.5f" % mr_raw))


# ---------------------------------------------------------------------- the rule
def rule(records, seq_off, qual_out, mr, status, rounded=False):
    """The expected records of the rescaled file — or, where a rescaled record has an MR tag already, the index of the first
    such record in file order (an int).  ``seq_off`` / ``qual_out``: the quality column the oracle returns and where each record's
    bytes lie in it; ``mr``: its sums (``rounded``: the float32 values as they are to be stored); ``status``: its routing."""
    assert len(records) == len(mr) == len(status) == len(seq_off) - 1
    out = []
    for i, body in enumerate(records):
        body = bytes(body)
        if int(status[i]) not in (SINGLE_END, INWARD_PAIR):
            out.append(body)
            continue
        if has_tag(body, b"MR"):
            return i
        at, l_seq = qual_at(body)
        new = bytes(bytearray(qual_out[int(seq_off[i]):int(seq_off[i + 1])]))
        assert len(new) == l_seq
        tag = b"MRf" + struct.pack("<f", mr[i]) if rounded else mr_tag(float(mr[i]))
        out.append(body[:at] + new + body[at + l_seq:] + tag)
    return out


def stream_of(records):
    """The records as they lie in a BAM stream: each behind its block_size."""
    return b"".join(struct.pack("<i", len(r)) + bytes(r) for r in records)


def counts_of(status):
    got = np.bincount(np.asarray(status, np.int64), minlength=5)
    return {name: int(got[code]) for code, name in enumerate(STATUS_NAMES)}


# ---------------------------------------------------------------------- a model, and its table in the oracle's layout
def make_model(seed=5, l5=L5, l3=L3, value=None):
    """(RescaleModel, corr[2][1 + l5 + l3] for ``oracle.rescale``, the dictionary): seeded probabilities for every position of
    both windows, or ``value`` for all of them."""
    rng = np.random.default_rng(seed)
    corr_prob = {}
    for p in list(range(1, l5 + 1)) + list(range(-l3, 0)):
        for r, s in (("C", "T"), ("G", "A")):
            corr_prob[(r, s, p)] = float(rng.random() * 0.8) if value is None else float(value)
    model = RescaleModel(corr_prob, l5, l3)
    corr = np.zeros((2, model.npos))
    for (r, _s, p), v in corr_prob.items():
        corr[0 if r == "C" else 1, p if p > 0 else l5 - p] = v
    return model, corr, corr_prob


def write_corr_csv(path, corr_prob, l5=L5, l3=L3):
    """``Stats_out_MCMC_correct_prob.csv`` as the command line reads it (rescale.py:23-46); ``repr`` keeps every bit."""
    with open(path, "w") as out:
        out.write('"","Position","C.T","G.A"\n')
        for k, p in enumerate(list(range(1, l5 + 1)) + list(range(-l3, 0))):
            out.write('"%d",%d,%r,%r\n' % (k + 1, p, corr_prob[("C", "T", p)], corr_prob[("G", "A", p)]))


# ---------------------------------------------------------------------- the encoder
SEQ_CODE = {c: i for i, c in enumerate(b"=ACMGRSVTWYHKDBN")}
OPS = {c: i for i, c in enumerate("MIDNSHP=X")}


def encode(name, flag, tid, pos, cigar, seq, qual, mtid=-1, mpos=-1, tlen=0, mapq=30, tags=b""):
    """One record without its block_size.  ``name``: bytes without the NUL; ``cigar``: [(operation letter, length)]; ``seq``:
    ASCII bytes; ``qual``: as many raw Phred bytes."""
    assert len(seq) == len(qual) and len(name) <= 254
    codes = [SEQ_CODE[c] for c in seq] + [0]
    packed = bytes((codes[k] << 4) | codes[k + 1] for k in range(0, len(seq), 2))
    ops = b"".join(struct.pack("<I", (ln << 4) | OPS[op]) for op, ln in cigar)
    return (struct.pack("<iiBBHHHiiii", tid, pos, len(name) + 1, mapq, 4680, len(cigar), flag, len(seq), mtid, mpos, tlen)
            + name + b"\0" + ops + packed + bytes(qual) + tags)


def raw_header(ref):
    text = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, ln) for n, ln in zip(ref.names, ref.lengths))
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(ref.names))
    for n, ln in zip(ref.names, ref.lengths):
        out += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    return out


def every_type_tags(rng):
    """A field of every aux type: A c C s S i I f Z H, and B over each of its seven item types."""
    out = b"XAAq" + b"Xcc" + struct.pack("<b", -5) + b"XCC" + struct.pack("<B", 200) + b"Xss" + struct.pack("<h", -300)
    out += b"XSS" + struct.pack("<H", 60000) + b"Xii" + struct.pack("<i", -70000) + b"XII" + struct.pack("<I", 4000000000)
    out += b"Xff" + struct.pack("<f", 1.5) + b"XZZ" + bytes(rng.integers(33, 127, int(rng.integers(0, 30)), dtype=np.uint8)) + b"\0"
    out += b"XHH" + b"1AE301" + b"\0"
    for sub, fmt in ((b"c", "b"), (b"C", "B"), (b"s", "h"), (b"S", "H"), (b"i", "i"), (b"I", "I"), (b"f", "f")):
        k = int(rng.integers(0, 5))
        out += b"Y" + sub + b"B" + sub + struct.pack("<i", k) + struct.pack("<%d%s" % (k, fmt), *([1] * k))
    return out


LOOKALIKE_Z = b"XLZabMRfxyzMRf!\0"                                                              # "MRf" inside a string
LOOKALIKE_B = b"XMBC" + struct.pack("<i", 9) + b"..MRf\x00\x00\x80\x3f"                           # ... inside a B:C array


def make_reference(seed=17):
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return Reference(["chrR", "chrS"], [rng.choice(acgt, 30_000).tobytes(), rng.choice(acgt, 8_000).tobytes()])


KINDS = ("forward", "reverse", "soft clips", "hard clips", "indels", "skip = X", "unmapped", "no bases", "no qualities", "mate A",
         "mate B", "improper", "short", "pristine")


def make_mix(n=1400, seed=23, ref=None, interleave_empty=False):
    """``n`` records over ``ref`` (``make_reference()``), the kinds of ``KINDS`` in turn: (reference, header bytes, record
    bodies, kind of each).  Bases are copied from the reference; C>T and G>A mismatches are planted in the first and last
    dozen bases of most records (``pristine`` ones get none: rescaled, nothing changes, MR 0).  ``interleave_empty``: a record
    without bases behind every other one."""
    ref = make_reference() if ref is None else ref
    rng = np.random.default_rng(seed)
    contigs = [np.frombuffer(s, np.uint8) for s in ref.seqs]
    bodies, kinds = [], []
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        tid = int(rng.integers(0, 2))
        length = int(rng.integers(1, 11)) if kind == "short" else int(rng.integers(25, 120))
        # the operations between the clips, and the reference bases they span
        if kind == "indels":
            a, b, c = (int(rng.integers(5, 40)) for _ in range(3))
            core = [("M", a), ("I", int(rng.integers(1, 5))), ("M", b), ("D", int(rng.integers(1, 6))), ("M", c)]
        elif kind == "skip = X":
            a, b, c = (int(rng.integers(5, 40)) for _ in range(3))
            core = [("=", a), ("N", int(rng.integers(1, 200))), ("X", b), ("M", c)]
        else:
            core = [("M", length)]
        span = sum(ln for op, ln in core if op in "MDN=X")
        pos = int(rng.integers(0, len(contigs[tid]) - span))
        seq, r = [], pos
        for op, ln in core:
            if op == "I":
                seq.append(rng.choice(np.frombuffer(b"ACGT", np.uint8), ln))
            elif op in "DN":
                r += ln
            else:
                seq.append(contigs[tid][r:r + ln].copy())
                r += ln
        seq = np.concatenate(seq)
        if kind != "pristine":
            m = seq.shape[0]
            ends = (np.arange(m) < 12) | (np.arange(m) >= m - 12)
            hit = ends & (rng.random(m) < 0.6)
            seq = np.where(hit & (seq == ord("C")), ord("T"), np.where(hit & (seq == ord("G")), ord("A"), seq)).astype(np.uint8)
        cigar = list(core)
        if kind == "soft clips":
            sl, sr = int(rng.integers(1, 15)), int(rng.integers(0, 15))
            seq = np.concatenate([rng.choice(np.frombuffer(b"ACGT", np.uint8), sl), seq, rng.choice(np.frombuffer(b"ACGT", np.uint8), sr)])
            cigar = [("S", sl)] + cigar + ([("S", sr)] if sr else [])
        elif kind == "hard clips":
            # (a hard clip outside a soft one is a record rescale.py:266-271 cannot write: none here)
            form = i // len(KINDS) % 3
            if form == 0:
                cigar = [("H", 5)] + cigar
            elif form == 1:
                cigar = cigar + [("H", 7)]
            else:
                seq = np.concatenate([rng.choice(np.frombuffer(b"ACGT", np.uint8), 4), seq])
                cigar = [("S", 4)] + cigar + [("H", 3)]
        qual = np.where(rng.random(seq.shape[0]) < 0.05, rng.choice([0, 1, 92, 93], seq.shape[0]), rng.integers(2, 42, seq.shape[0])).astype(np.uint8)
        flag, mtid, mpos, tlen = (16 if kind == "reverse" or (kind not in ("forward", "mate A", "mate B") and rng.random() < 0.5) else 0), -1, -1, 0
        if kind == "unmapped":
            flag, cigar = flag | 4, []
            if i // len(KINDS) % 2:
                tid, pos = -1, -1
        elif kind == "no bases":
            seq, qual, cigar = seq[:0], qual[:0], []
        elif kind == "no qualities":
            qual[:] = 0xFF
        elif kind == "mate A":                   # forward, its mate reverse and to the right
            flag, mtid, mpos, tlen = 0x1 | 0x2 | 0x40 | 0x20, tid, pos + int(rng.integers(1, 300)), 300
        elif kind == "mate B":                   # reverse, its mate forward and to the left
            flag, mtid, mpos, tlen = 0x1 | 0x2 | 0x80 | 0x10, tid, max(0, pos - int(rng.integers(1, 300))), -300
        elif kind == "improper":
            form = i // len(KINDS) % 3
            if form == 0:                        # outward
                flag, mtid, mpos = 0x1 | 0x40 | 0x20, tid, pos - int(rng.integers(1, 300))
            elif form == 1:                      # the mate on the other sequence
                flag, mtid, mpos = 0x1 | 0x80 | 0x10, 1 - tid, max(0, pos - 50)
            else:                                # both on one strand
                flag, mtid, mpos = 0x1 | 0x40, tid, pos + 100
        # names: one character, 254 characters, "MRf" inside; tags: none, every type, look-alikes, a real MR where nothing is rescaled
        which = i // len(KINDS) % 7
        if which == 0:
            name = bytes([65 + i % 26])
        elif which == 1:
            name = (b"MRf%d_" % i + bytes(rng.integers(97, 123, 254, dtype=np.uint8)))[:254]
        else:
            name = b"r%d" % i
        rescaled = kind not in ("unmapped", "no bases", "no qualities", "improper")
        pick = int(rng.integers(0, 5))
        if pick == 0:
            tags = b""
        elif pick == 1:
            tags = every_type_tags(rng)
        elif pick == 2:
            tags = LOOKALIKE_Z + LOOKALIKE_B
        elif pick == 3:
            tags = b"RGZlane1\0" + every_type_tags(rng) + b"NMC\x02"
        else:
            tags = b"NMC\x01"
        if not rescaled and which in (2, 3, 4):
            mr = (b"MRf" + struct.pack("<f", 0.25), b"MRi" + struct.pack("<i", 7), b"MRZold\0")[which - 2]
            tags = every_type_tags(rng) + mr + LOOKALIKE_B + b"XQi" + struct.pack("<i", i)
        bodies.append(encode(name, flag, tid, pos, cigar, seq.tobytes(), qual, mtid, mpos, tlen, mapq=int(rng.integers(0, 61)), tags=tags))
        kinds.append(kind)
        if interleave_empty and i % 2:
            bodies.append(encode(b"e%d" % i, 0, tid, pos, [], b"", b"", tags=b"XEi" + struct.pack("<i", i)))
            kinds.append("no bases")
    return ref, raw_header(ref), bodies, kinds
