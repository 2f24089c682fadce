"""--calmd restated for the tests, from the text of the rule (the issue's paragraph "the rule"; the product's form of it is
mapdamage_amd/csrc/mdx_kept_md.h), the slow obvious way: a record is taken apart into its fields and a list of its tags, the
alignment is walked a column at a time into a list of MD tokens, and the record is put together again.  Nothing here is
shared with the product.

``rebuild`` goes the other way: from an MD string, the CIGAR and SEQ it says which reference base lies under every M = X
and D column, without looking at a reference — the tests compare that with the reference.  It shares no line with the emitter.

A record is its bytes behind the block_size field (``body``).  The reference is a list of strings, one per sequence in the
header's order: 'A' 'C' 'G' 'T' in upper case, anything else is read as 'N'."""

import struct

NIBBLES = "=ACMGRSVTWYHKDBN"
OPS = "MIDNSHP=X"
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def fields(body):
    """The record's fixed fields and where its parts begin, or None for less than 32 bytes."""
    if len(body) < 32:
        return None
    tid, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", body, 0)
    cig_at = 32 + l_name
    seq_at = cig_at + 4 * n_cig
    qual_at = seq_at + (l_seq + 1) // 2
    return dict(tid=tid, pos=pos, flag=flag, n_cig=n_cig, l_seq=l_seq, cig_at=cig_at, seq_at=seq_at, qual_at=qual_at, tags_at=qual_at + l_seq)


def tags(body, at):
    """[(name, type, first byte, byte behind)] of the tag region body[at:], or None where it cannot be followed to exactly the
    record's end: a field cut off, a Z or H without its NUL, a B array past the end, an unknown type."""
    out, end = [], len(body)
    while at < end:
        if at + 3 > end:
            return None
        name, ty = body[at:at + 2], chr(body[at + 2])
        q = at + 3
        if ty in FIXED:
            q += FIXED[ty]
        elif ty in "ZH":
            nul = body.find(b"\0", q)
            if nul < 0:
                return None
            q = nul + 1
        elif ty == "B":
            if q + 5 > end:
                return None
            sub, count = chr(body[q]), struct.unpack_from("<I", body, q + 1)[0]
            q += 5 + count * (1 if sub in "cC" else 2 if sub in "sS" else 4)
        else:
            return None
        if q > end:
            return None
        out.append((name, ty, at, q))
        at = q
    return out


def operations(body, f):
    ops = []
    for k in range(f["n_cig"]):
        word = struct.unpack_from("<I", body, f["cig_at"] + 4 * k)[0]
        ops.append((OPS[word & 15] if (word & 15) < len(OPS) else "?", word >> 4))
    return ops


def nibbles(body, f):
    out = []
    for byte in body[f["seq_at"]:f["qual_at"]]:
        out += [byte >> 4, byte & 15]
    return out[:f["l_seq"]]


def ref_letter(ch):
    return ch if ch in "ACGT" else "N"


def outcome(body, ref):
    """(the new body, recomputed?, had NM or MD?) — the same body where the record is skipped."""
    f = fields(body)
    if f is None:
        return body, False, False
    listed = tags(body, f["tags_at"]) if f["tags_at"] <= len(body) else None
    had = listed is not None and any(t[0] in (b"NM", b"MD") for t in listed)
    skipped = (body, False, had)
    if f["l_seq"] == 0 or f["n_cig"] == 0 or f["tags_at"] > len(body):
        return skipped
    ops = operations(body, f)
    if sum(n for op, n in ops if op in "MIS=X") != f["l_seq"]:
        return skipped
    span = sum(n for op, n in ops if op in "MDN=X")
    if not 0 <= f["tid"] < len(ref) or f["pos"] < 0 or f["pos"] + span > len(ref[f["tid"]]):
        return skipped
    if listed is None or any(t[0] == b"CG" and t[1] == "B" for t in listed):
        return skipped
    under = ref[f["tid"]][f["pos"]:f["pos"] + span]
    read = nibbles(body, f)
    tokens, x, y, u, nm = [], 0, 0, 0, 0
    for op, n in ops:
        if op in "M=X":
            for _ in range(n):
                base, nib = under[x], read[y]
                if nib == 0 or (nib in (1, 2, 4, 8) and base in "ACGT" and NIBBLES[nib] == base):
                    u += 1
                else:
                    tokens += [str(u), ref_letter(base)]
                    u, nm = 0, nm + 1
                x, y = x + 1, y + 1
        elif op == "D":
            tokens += [str(u), "^" + "".join(ref_letter(c) for c in under[x:x + n])]
            u, nm, x = 0, nm + n, x + n
        elif op == "I":
            y, nm = y + n, nm + n
        elif op == "S":
            y += n
        elif op == "N":
            x += n
    md = "".join(tokens) + str(u)
    if len(md) > 2 * f["l_seq"] + 64:
        return skipped
    kept = b"".join(body[a:b] for name, _ty, a, b in listed if name not in (b"NM", b"MD"))
    if nm < 256:
        field = b"NMC" + struct.pack("<B", nm)
    elif nm < 65536:
        field = b"NMS" + struct.pack("<H", nm)
    else:
        field = b"NMI" + struct.pack("<I", nm)
    return body[:f["tags_at"]] + kept + field + b"MDZ" + md.encode() + b"\0", True, had


def calmd(body, ref):
    """The record with NM and MD recomputed — the same body where the rule skips it."""
    return outcome(body, ref)[0]


def nm_md(body):
    """(NM, MD) as the record's tags have them (None where it has none; the first one of each)."""
    f = fields(body)
    nm = md = None
    for name, ty, a, b in tags(body, f["tags_at"]) or []:
        if name == b"NM" and nm is None and ty in "cCsSiI":
            nm = struct.unpack_from("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty], body, a + 3)[0]
        if name == b"MD" and md is None and ty == "Z":
            md = body[a + 3:b - 1].decode()
    return nm, md


def rebuild(md, ops, read):
    """The reference under every M = X and D column, in order, as MD, the operations and the read's nibbles tell it: a letter
    of MD, or — inside a run of matches — the read's own base (None under a '=' nibble, which names no base).  Returns (the
    list, the mismatches and deleted bases MD names); AssertionError where MD does not fit the alignment."""
    at, out, edits, y = 0, [], 0, 0

    def number():
        nonlocal at
        start = at
        while at < len(md) and md[at].isdigit():
            at += 1
        assert at > start, "MD has no number at %d: %r" % (start, md)
        return int(md[start:at])

    run = number()
    for op, n in ops:
        if op in "M=X":
            for _ in range(n):
                if run > 0:
                    run -= 1
                    nib = read[y]
                    assert nib in (0, 1, 2, 4, 8), "MD calls a match what is no single base: %r" % md
                    out.append(None if nib == 0 else NIBBLES[nib])
                else:
                    assert at < len(md) and md[at].isalpha(), "MD has no letter at %d: %r" % (at, md)
                    out.append(md[at])
                    at += 1
                    edits += 1
                    run = number()
                y += 1
        elif op == "D":
            assert run == 0 and at < len(md) and md[at] == "^", "MD has no deletion at %d: %r" % (at, md)
            at += 1
            assert md[at:at + n].isalpha() and len(md[at:at + n]) == n
            out += list(md[at:at + n])
            at += n
            edits += n
            run = number()
        elif op in "IS":
            y += n
    assert run == 0 and at == len(md), "MD goes on behind the alignment: %r" % md
    return out, edits


def check_inverse(new_body, ref):
    """A recomputed record's MD and NM against the reference, by ``rebuild``."""
    f = fields(new_body)
    ops = operations(new_body, f)
    nm, md = nm_md(new_body)
    assert nm is not None and md is not None
    got, edits = rebuild(md, ops, nibbles(new_body, f))
    span = sum(n for op, n in ops if op in "MDN=X")
    under = ref[f["tid"]][f["pos"]:f["pos"] + span]
    want, x = [], 0
    for op, n in ops:
        if op in "M=XD":
            want += [ref_letter(c) for c in under[x:x + n]]
        if op in "MDN=X":
            x += n
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g is None or g == w, (md, got, want)
    assert nm == edits + sum(n for op, n in ops if op == "I")
