"""--mask-ends restated for the tests (the rule: mapdamage_amd/csrc/mdx_kept_mask.h; the issue's paragraph "the rule"), the slow
obvious way: a record is decoded into lists of bases, qualities and CIGAR operations, its alignment is expanded column by
column, the windows are sets of SEQ indices taken from the query in the molecule's orientation, and the record is encoded
again.  Nothing here is shared with the product.

A record is its bytes behind the block_size field (``body``; ``len(body)`` is its block_size).  The reference is a list of
strings, one per sequence in the header's order: 'A' 'C' 'G' 'T', anything else for what is no base."""

import struct

ALL, TRANSITIONS, MISMATCHES = "all", "transitions", "mismatches"
MODES = (ALL, TRANSITIONS, MISMATCHES)
NIBBLES = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"


def parse_cigar(text):
    """'3S10M2D5M' -> [('S', 3), ('M', 10), ...]"""
    out, number = [], ""
    for ch in text:
        if ch.isdigit():
            number += ch
        else:
            out.append((ch, int(number)))
            number = ""
    assert not number
    return out


def make_record(cigar, seq, qual=None, flag=0, tid=0, pos=0, name=b"r", tags=b"", l_seq=None, pad=0):
    """A record's body: ``cigar`` as text or a list of (op, length), ``seq`` as letters of ``NIBBLES``, ``qual`` a list of
    bytes (None: 30 everywhere), ``pad`` the unused low nibble of an odd SEQ's last byte."""
    ops = parse_cigar(cigar) if isinstance(cigar, str) else list(cigar)
    nibbles = [NIBBLES.index(c) for c in seq]
    n = len(nibbles)
    if n % 2:
        nibbles.append(pad)
    packed = bytes(nibbles[i] << 4 | nibbles[i + 1] for i in range(0, len(nibbles), 2))
    qual = [30] * n if qual is None else list(qual)
    assert len(qual) == n
    name = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), 37, 4680, len(ops), flag, n if l_seq is None else l_seq, -1, -1, 0)
    body += name + b"".join(struct.pack("<I", length << 4 | OPS.index(op)) for op, length in ops) + packed + bytes(qual) + tags
    return body


def decode(body):
    """The record as a dict of lists, or None where its SEQ and QUAL do not lie inside its bytes (or it has no bases)."""
    if len(body) < 32:
        return None
    tid, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", body, 0)
    seq_at = 32 + l_name + 4 * n_cig
    qual_at = seq_at + (l_seq + 1) // 2
    if l_seq == 0 or qual_at + l_seq > len(body):
        return None
    ops = []
    for k in range(n_cig):
        word = struct.unpack_from("<I", body, 32 + l_name + 4 * k)[0]
        ops.append((word & 15, word >> 4))
    nibbles = []
    for byte in body[seq_at:qual_at]:
        nibbles += [byte >> 4, byte & 15]
    return dict(tid=tid, pos=pos, flag=flag, l_seq=l_seq, ops=ops, nibbles=nibbles, qual=list(body[qual_at:qual_at + l_seq]),
                seq_at=seq_at, qual_at=qual_at)


def encode(body, rec):
    """``body`` with the SEQ and QUAL of ``rec``."""
    nib = rec["nibbles"]
    packed = bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))
    return body[:rec["seq_at"]] + packed + bytes(rec["qual"]) + body[rec["qual_at"] + rec["l_seq"]:]


def query_range(rec):
    """[qs, qe) of SEQ: without the terminal soft clips (leading S behind optional H, trailing S in front of optional H, the
    first operation never taken for a trailing one); None where the CIGAR's M I S = X do not add up to l_seq."""
    ops = rec["ops"]
    if not ops:
        return 0, rec["l_seq"]
    if sum(length for op, length in ops if op < len(OPS) and OPS[op] in "MIS=X") != rec["l_seq"]:
        return None
    qs, qe = 0, rec["l_seq"]
    i = 0
    while i < len(ops) and ops[i][0] in (4, 5):
        qs += ops[i][1] if ops[i][0] == 4 else 0
        i += 1
    j = len(ops)
    while j > 1 and ops[j - 1][0] in (4, 5):
        qe -= ops[j - 1][1] if ops[j - 1][0] == 4 else 0
        j -= 1
    return qs, qe


def columns(rec):
    """The alignment, column by column: (SEQ index or None, reference offset from pos or None); a soft-clipped base is a
    column without a reference base of its own kind ('S')."""
    out, q, r = [], 0, 0
    for op, length in rec["ops"]:
        letter = OPS[op] if op < len(OPS) else "?"
        for _ in range(length):
            if letter in "M=X":
                out.append((q, r, "M"))
                q, r = q + 1, r + 1
            elif letter == "I":
                out.append((q, None, "I"))
                q += 1
            elif letter == "S":
                out.append((q, None, "S"))
                q += 1
            elif letter in "DN":
                out.append((None, r, letter))
                r += 1
    return out, r


def apply(body, k5, k3, what, single_stranded=False, ref=None):
    """(the record masked, its selected bases)"""
    assert what in MODES and 0 <= k5 <= 255 and 0 <= k3 <= 255 and (k5 or k3)
    rec = decode(body)
    if rec is None:
        return body, 0
    if not rec["ops"] and what == MISMATCHES:
        return body, 0
    span = query_range(rec)
    if span is None:
        return body, 0
    qs, qe = span
    if qe - qs <= 0:
        return body, 0
    reverse = bool(rec["flag"] & 0x10)
    query = list(range(qs, qe))
    molecule = query[::-1] if reverse else query                 # 5' to 3'
    window5 = set(molecule[:min(k5, len(molecule))])
    window3 = set(molecule[len(molecule) - min(k3, len(molecule)):])
    want5 = "A" if reverse else "T"
    want3 = want5 if single_stranded else ("T" if reverse else "A")
    under = {}
    if what == MISMATCHES:
        cols, ref_span = columns(rec)
        tid, pos = rec["tid"], rec["pos"]
        if ref is None or not 0 <= tid < len(ref) or pos < 0 or pos + ref_span > len(ref[tid]):
            return body, 0
        for q, r, kind in cols:
            if kind == "M":
                under[q] = ref[tid][pos + r]
    selected = []
    for b in query:
        base = NIBBLES[rec["nibbles"][b]]
        in5, in3 = b in window5, b in window3
        if what == ALL:
            hit = in5 or in3
        else:
            hit = (in5 and base == want5) or (in3 and base == want3)
            if hit and what == MISMATCHES:
                hit = under.get(b) == {"T": "C", "A": "G"}[base]
        if hit:
            selected.append(b)
    has_qual = rec["qual"][0] != 0xFF
    for b in selected:
        rec["nibbles"][b] = 15
        if has_qual:
            rec["qual"][b] = 0
    return encode(body, rec), len(selected)
