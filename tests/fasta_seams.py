"""Cases for the tests of the resident reference at its seams: small FASTA files (and their BGZF twins) built so that
something ends inside a lane's sixteen bytes or at a piece, slab or file boundary of the library's loader
(mdx_fasta.hip fasta_strip_kernel), of the 4-bit form (ref_finish) and of the composition kernel (genome_comp_kernel) — and
a model of what must come out: faidx restated.  Deterministic from a seed; numpy only (the BGZF twins are written by
tests/test_fasta_bgzf.py's ``_write_blocks``, where the tests need them).  Collects no tests:
tests/test_fasta_seams_cases.py checks the cases themselves (no GPU), tests/test_gpu_fasta_seams.py runs them on the device.

The model shares nothing with mapdamage_amd.fasta: ``fai_rows`` restates the index build (the name ends at the first white
space, linebases and linewidth are the first line's), ``fetch`` the faidx arithmetic (base i lies at
offset + i // linebases * linewidth + i % linebases), ``fold`` the classes of the resident reference (.upper(), then ACGT,
'-', and 'N' for everything else), ``composition`` a count of the four bases.  ``pieces`` and ``slabs`` restate which parts
of a file the loader has to touch: the pieces of an uncompressed file from the first wanted byte in steps of the piece size,
the BGZF blocks a wanted sequence reaches into joined to slabs of at most a piece."""
import functools

import numpy as np

# the smallest piece the loader accepts (mdx_fasta.hip fasta_piece_bytes: max(4096, MDX_FASTA_PIECE_BYTES) & ~15)
PIECE = 4096
CLASSES = ("phase", "crowded", "geometry", "alphabet", "tail", "gaps", "overlap")
# inflated bytes per BGZF block of a twin: slab boundaries at arbitrary text offsets; PIECE + 1 is a slab of its own
BLOCK_SIZES = (16, 17, 997, 1000, 1024, PIECE, PIECE + 1)
PHASE_WIDTHS = (1, 7, 16, 60, 61)
# what the byte at a piece (slab) boundary can be
PHASE_KINDS = ("line_first", "line_last", "lf", "cr", "gt", "header", "seq_first", "raw_end")


class Case:
    """One FASTA file.  ``cls``: its class; ``label``: what is particular about it; ``text``: the (inflated) file's bytes;
    ``fai``: rows (name, length, offset, linebases, linewidth), ``fai_rows(text)`` unless ``own_fai``; ``order``: the names
    asked for, in header order (absent ones among them); ``piece``: MDX_FASTA_PIECE_BYTES or None; ``kind``: for ``phase``
    the byte kind meant to lie at the boundary; ``block`` / ``gzi``: None for the plain file, for a BGZF twin the inflated
    bytes per block and whether the .gzi is built."""

    def __init__(self, cls, label, text, order, piece, fai=None, kind=None, block=None, gzi=None):
        self.cls, self.label, self.text, self.order, self.piece = cls, label, bytes(text), list(order), piece
        self.own_fai = fai is not None
        self.fai = list(fai) if fai is not None else fai_rows(self.text)
        self.kind, self.block, self.gzi = kind, block, gzi

    def twin(self, block, gzi):
        assert not self.own_fai
        return Case(self.cls, "%s [BGZF blocks of %d, %s .gzi]" % (self.label, block, "with" if gzi else "no"), self.text,
                    self.order, self.piece, None, self.kind, block, gzi)

    def __repr__(self):
        return "Case(%s, %s)" % (self.cls, self.label)


# ---------------------------------------------------------------------------------------------------------------- the model

def fai_rows(text):
    """The index of ``text`` as faidx builds it: (name, length, offset, linebases, linewidth) per sequence."""
    rows, at, n = [], 0, len(text)
    while at < n:
        assert text[at:at + 1] == b">", at
        end = text.find(b"\n", at)
        head = text[at + 1:end if end >= 0 else n]
        name = b""
        for i in range(len(head) + 1):
            if i == len(head) or head[i:i + 1] in b" \t\r\v\f":
                name = head[:i]
                break
        at = end + 1 if end >= 0 else n
        off, length, lb, lw, first = at, 0, 0, 0, True
        while at < n and text[at:at + 1] != b">":
            end = text.find(b"\n", at)
            line = text[at:end if end >= 0 else n]
            width = len(line) + (1 if end >= 0 else 0)
            bases = len(line.rstrip(b"\r"))
            if first:
                lb, lw, first = bases, width, False
            length += bases
            at = end + 1 if end >= 0 else n
        rows.append((name.decode("ascii"), length, off, lb, lw))
    return rows


def fai_text(rows):
    return "".join("%s\t%d\t%d\t%d\t%d\n" % row for row in rows).encode()


def raw_span(row):
    """Bytes of the file from a sequence's first base to behind its last."""
    _, length, _, lb, lw = row
    return 0 if length == 0 else (length - 1) // lb * lw + (length - 1) % lb + 1


def offsets(row):
    """The file offset of every base of a sequence."""
    _, length, off, lb, lw = row
    i = np.arange(length, dtype=np.int64)
    return off + i // max(lb, 1) * lw + i % max(lb, 1)


def fold(seq):
    """.upper(), then the classes the resident reference tells apart: ACGT, '-', 'N' for everything else."""
    up = np.frombuffer(bytes(seq).upper(), np.uint8)
    out = np.full(up.shape, ord("N"), np.uint8)
    for ch in b"ACGT-":
        out[up == ch] = ch
    return out.tobytes()


def fetch_raw(file_bytes, row):
    return np.frombuffer(file_bytes, np.uint8)[offsets(row)].tobytes()


def fetch(file_bytes, row):
    """faidx restated: the whole sequence of one index row, folded."""
    return fold(fetch_raw(file_bytes, row))


def sequences(case):
    """What ``case.order`` must load to: one folded sequence per name, b"" for a name the index lacks (the first row of a
    name counts, as faidx)."""
    rows = {}
    for row in case.fai:
        rows.setdefault(row[0], row)
    return [fetch(case.text, rows[name]) if name in rows else b"" for name in case.order]


def wanted_rows(case):
    """The rows of the non-empty wanted sequences, by file offset."""
    rows = {}
    for row in case.fai:
        rows.setdefault(row[0], row)
    return sorted((rows[n] for n in case.order if n in rows and rows[n][1] > 0), key=lambda r: r[2])


def composition(seqs):
    """A, C, G, T per (folded) sequence."""
    out = np.zeros((len(seqs), 4), np.uint64)
    for i, s in enumerate(seqs):
        a = np.frombuffer(s, np.uint8)
        out[i] = [int((a == c).sum()) for c in b"ACGT"]
    return out


def pieces(case):
    """The pieces of the uncompressed file: [(first byte, bytes, holds a wanted byte)] from the first wanted byte to the
    last in steps of the piece size."""
    spans = [(r[2], r[2] + raw_span(r)) for r in wanted_rows(case)]
    if not spans:
        return []
    step = case.piece or (256 << 20)
    lo, hi = spans[0][0], max(e for _, e in spans)
    return [(f0, min(step, hi - f0), any(a < f0 + min(step, hi - f0) and e > f0 for a, e in spans)) for f0 in range(lo, hi, step)]


def block_bounds(case):
    """[inflated offset of block b, ... , text length] of a twin's data blocks."""
    n = len(case.text)
    return list(range(0, n, case.block)) + [n]


def slabs(case):
    """The slabs of a BGZF twin: lists of block numbers — the blocks a wanted sequence reaches into, consecutive ones joined
    while their inflated bytes come to at most a piece."""
    spans = [(r[2], r[2] + raw_span(r)) for r in wanted_rows(case)]
    step = case.piece or (256 << 20)
    at = block_bounds(case)
    out, size = [], 0
    for b in range(len(at) - 1):
        if not any(a < at[b + 1] and e > at[b] for a, e in spans):
            continue
        if not out or out[-1][-1] != b - 1 or size + at[b + 1] - at[b] > step:
            out.append([])
            size = 0
        out[-1].append(b)
        size += at[b + 1] - at[b]
    return out


def boundary(case):
    """The first place where the loader's view of the file ends and another begins: the end of the first piece of a plain
    file, of the first slab of a twin (the file's end where there is no second)."""
    if case.block is None:
        f0, n, _ = pieces(case)[0]
        return f0 + n
    return block_bounds(case)[slabs(case)[0][-1] + 1]


def byte_kinds(case, at):
    """What the byte at offset ``at`` of the text is, in the words of PHASE_KINDS (a set: the only base of a line is its
    first and its last)."""
    text = case.text
    if at == len(text):
        return {"raw_end"} if any(r[2] + raw_span(r) == at and r[1] > 0 for r in case.fai) else {"end_of_file"}
    start = text.rfind(b"\n", 0, at) + 1
    if text[start:start + 1] == b">":
        return {"gt"} if at == start else {"header"}
    ch = text[at:at + 1]
    if ch == b"\n":
        return {"lf"}
    if ch == b"\r":
        return {"cr"}
    kinds = set()
    if any(r[2] == at and r[1] > 0 for r in case.fai):
        kinds.add("seq_first")
    elif at == start:
        kinds.add("line_first")
    if text[at + 1:at + 2] in (b"\n", b"\r"):
        kinds.add("line_last")
    return kinds or {"base"}


# ---------------------------------------------------------------------------------------------------------------- builders

_PLAIN = np.frombuffer(b"ACGT", np.uint8)
_ODD = np.frombuffer(b"acgtNnRYKM-*", np.uint8)


def _bases(rng, n, odd=0.06):
    out = rng.choice(_PLAIN, n)
    if n and odd:
        hit = rng.random(n) < odd
        out[hit] = rng.choice(_ODD, int(hit.sum()))
    return out.tobytes()


def _lines(seq, width, eol, last_eol=True):
    """``seq`` in lines of ``width`` bases."""
    parts = [seq[i:i + width] for i in range(0, len(seq), width)]
    out = eol.join(parts)
    return out + eol if parts and last_eol else out


def _phase_text(rng, width, eol, kind, at_of):
    """A file ``p``, ``s``, ``q``[, ``z``] (all wanted; ``p`` starts the pieces) in which the byte of ``kind`` lies on the
    boundary: ``p`` and ``q`` in lines of ``width``, ``s`` one line whose length is tuned.  ``at_of(raw_off of p)``: where
    the boundary is."""
    lw = width + len(eol)
    head_p = b">p" + eol
    goal = at_of(len(head_p))
    n_q = 6 * width + (width + 1) // 2              # a short last line (width 1: full)
    if kind == "raw_end":
        n_q = 3 * width + (width // 2 or 1)
    q = _lines(_bases(rng, n_q), width, eol, last_eol=kind != "raw_end")
    head_q = b">q" + (b" piece boundary" if kind == "header" else b"") + eol
    # where the byte lies, counted from the first byte of q's header
    rel = {"line_first": len(head_q) + 2 * lw, "line_last": len(head_q) + 2 * lw + width - 1, "cr": len(head_q) + 2 * lw + width,
           "lf": len(head_q) + 3 * lw - 1, "gt": 0, "header": 4, "seq_first": len(head_q), "raw_end": len(head_q) + len(q)}[kind]
    head_s = b">s" + eol
    fixed = len(head_p) + len(head_s) + len(eol) + rel          # all but p's lines and s's bases
    n_lines = (goal - fixed - 1) // lw
    assert n_lines >= 1
    n_s = goal - fixed - n_lines * lw
    assert 1 <= n_s <= lw
    text = head_p + _lines(_bases(rng, n_lines * width), width, eol) + head_s + _bases(rng, n_s) + eol + head_q + q
    if kind != "raw_end":
        # (enough behind the boundary that a twin's next block does not fit into the first slab)
        text += b">z tail" + eol + _lines(_bases(rng, max(150, width + 3)), width, eol)
    return text


def _phase(seed):
    out = []
    for wi, width in enumerate(PHASE_WIDTHS):
        for ei, eol in enumerate((b"\n", b"\r\n")):
            kinds = [k for k in PHASE_KINDS if k != "cr" or eol == b"\r\n"]
            for ki, kind in enumerate(kinds):
                rng = np.random.default_rng([seed, 1, wi, ei, ki])
                name = "width %d, %s, boundary on %s" % (width, "CRLF" if ei else "LF", kind)
                order = ["p", "absent", "q", "s"] + (["z"] if kind != "raw_end" else [])
                out.append(Case("phase", name, _phase_text(rng, width, eol, kind, lambda r: r + PIECE), order, PIECE, kind=kind))
    return out


def _phase_twins(seed):
    """Texts of their own: the slab boundary of a twin lies elsewhere than the piece boundary of the plain file (whole
    blocks from the block of the first wanted byte, which is the file's first here)."""
    out = []
    for wi, width in enumerate(PHASE_WIDTHS):
        for ei, eol in enumerate((b"\n", b"\r\n")):
            kinds = [k for k in PHASE_KINDS if k != "cr" or eol == b"\r\n"]
            for ki, kind in enumerate(kinds):
                block = BLOCK_SIZES[(2 * wi + ei + ki) % len(BLOCK_SIZES)]
                goal = PIECE // block * block if block <= PIECE else block
                rng = np.random.default_rng([seed, 2, wi, ei, ki])
                name = "width %d, %s, boundary on %s" % (width, "CRLF" if ei else "LF", kind)
                order = ["p", "absent", "q", "s"] + (["z"] if kind != "raw_end" else [])
                plain = Case("phase", name, _phase_text(rng, width, eol, kind, lambda r: goal), order, PIECE, kind=kind)
                out += [plain.twin(block, True), plain.twin(block, False)]
    return out


def _names(rng, n):
    """``n`` different names of two or three characters (the names of one are _crowded's to place)."""
    alphabet = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_."
    seen, out = set(), []
    while len(out) < n:
        name = "".join(alphabet[i] for i in rng.integers(0, len(alphabet), int(rng.integers(2, 4))))
        if name not in seen:
            seen.add(name)
            out.append(name)
    return out


def _crowded(seed):
    out = []
    for si, (n, eol, last_eol) in enumerate(((200, b"\n", True), (317, b"\n", False), (400, b"\r\n", True))):
        rng = np.random.default_rng([seed, 3, si])
        names = _names(rng, n)
        lens = rng.integers(0, 4, n)
        # (chance alone rarely puts three sequences with bases and an empty one into sixteen bytes: runs of one-letter names
        # with 1, 1, 0 and 1 bases — fourteen bytes from the first base to the last — at a dozen places, each aligned otherwise)
        for k in range(12):
            at = 5 + k * ((n - 12) // 12)
            names[at:at + 4] = list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"[4 * k:4 * k + 4])
            lens[at:at + 4] = (1, 1, 0, 1)
        lens[-1] = 2 + si % 2                         # (the last one holds bases, and where the file has no line end a last line)
        text = b""
        for i, (name, ln) in enumerate(zip(names, lens)):
            seq = _bases(rng, int(ln), odd=0.15)
            text += b">" + name.encode() + eol + (seq + (eol if last_eol or i < n - 1 else b"") if seq else b"")
        for subset, picked in (("all", names), ("every other one", names[::2]), ("only the last", names[-1:])):
            order = [picked[i] for i in rng.permutation(len(picked))]
            for k in range(0, len(order) + 1, 7):       # absent names in between
                order.insert(int(rng.integers(0, len(order) + 1)), "no-%d" % k)
            out.append(Case("crowded", "%d sequences of 0 to 3 bases, %s, %s wanted" % (n, "CRLF" if eol != b"\n" else "LF", subset),
                            text, order, PIECE))
    return out


def _geometry(seed):
    out = []
    lbs = (1, 2, 15, 16, 17, 60, PIECE - 1, PIECE, PIECE + 1)
    count = 0
    for li, lb in enumerate(lbs):
        for end in (0, 1, 2):
            eol = (b"", b"\n", b"\r\n")[end]
            many = 3 if lb < 1000 else 2
            lengths = (lb,) if end == 0 else (many * lb, many * lb - 1, lb)
            for ni, n in enumerate(lengths):
                for at_eof in ((True,) if end == 0 else (False, True)):
                    if n == 0:
                        continue
                    rng = np.random.default_rng([seed, 4, li, end, ni, int(at_eof)])
                    front = b">u0 not wanted\n" + _lines(_bases(rng, 23), 10, b"\n")
                    main = b">g the line shape under test" + (eol or b"\n") + _lines(_bases(rng, n), lb, eol, last_eol=not at_eof)
                    rear = b"" if at_eof else b">t\tbehind\n" + _bases(rng, 5) + b"\n"
                    order = ["g", "absent"] if at_eof else ["t", "absent", "g"]
                    name = "%d bases in lines of %d + %d%s" % (n, lb, end, ", the file ends without a line end" if at_eof else "")
                    out.append(Case("geometry", name, front + main + rear, order, PIECE if count % 5 else None))
                    count += 1
    return out


def alphabet_values():
    """Every byte a sequence line can hold: all but LF and CR."""
    return [v for v in range(256) if v not in (10, 13)]


def _alphabet(seed):
    """Lines of 'A', the 254 values in an order of the case's own, 'C': 257 bytes with the line end — a line starts one
    place further in its sixteen-byte unit than the line above, so sixteen lines and more put each value into each place of a
    unit, wherever the units start.  ('A' and 'C' at the lines' ends: no '>' at a line's start and no white space at a line's
    end, where another reader would strip it.)"""
    out = []
    for si, n_lines in enumerate((16, 33, 21)):
        rng = np.random.default_rng([seed, 5, si])
        lines = [b"A" + bytes(rng.permutation(np.asarray(alphabet_values(), np.uint8))) + b"C"] * n_lines
        text = b">u\nACGT\n>sym every byte value\n" + b"\n".join(lines) + (b"\n>w\nGATTACA\n" if si != 2 else b"")
        out.append(Case("alphabet", "%d lines of all byte values%s" % (n_lines, ", to the file's end" if si == 2 else ""), text,
                        ["sym", "w"] if si != 2 else ["absent", "sym"], PIECE if si != 1 else None))
    return out


def _tail(seed):
    """Two wanted sequences ``a`` and ``b`` (something unwanted between them in the second half of the cases, more than a
    piece of it): ``total`` = wanted bases mod 16, ``last`` = bytes in the last unit of the last piece, (last wanted byte -
    first wanted byte) mod 16 — set by the length of ``b`` and by a description behind its name."""
    out = []
    for far in (False, True):
        for total in range(16):
            last = (total * 3 + 5 + far) % 16
            rng = np.random.default_rng([seed, 6, int(far), total])
            n_a = 37
            n_b = 16 + (total - n_a) % 16
            head_a = b">a\n"
            body_a = _lines(_bases(rng, n_a), 10, b"\n")
            middle = b">u filler\n" + _lines(_bases(rng, PIECE + 500), 60, b"\n") if far else b""
            at_eof = total % 2 == 1
            body_b = _lines(_bases(rng, n_b), 10, b"\n", last_eol=not at_eof)
            span_b = len(body_b.rstrip(b"\n"))
            fixed = len(body_a) + len(middle) + len(b">b\n") + span_b
            pad = (last - fixed) % 16
            head_b = b">b" + (b" " + b"x" * (pad - 1) if pad else b"") + b"\n"
            text = head_a + body_a + middle + head_b + body_b + (b"" if at_eof else b">c\nAC\n")
            out.append(Case("tail", "%d wanted bases mod 16, %d bytes in the last unit%s" % (total, last, ", two pieces apart" if far else ""),
                            text, ["b", "a"] if total % 4 < 2 else ["a", "none", "b"], PIECE))
    return out


def _gaps(seed):
    out = []
    rng = np.random.default_rng([seed, 7])
    parts = [("w0", 200), ("u1", 3500), ("u2", 3600), ("u3", 3700), ("w1", 300), ("u4", 9100), ("w2", 100), ("u5", 2500), ("w3", 61)]
    text = b"".join(b">" + n.encode() + b"\n" + _lines(_bases(rng, ln), 60, b"\n") for n, ln in parts)
    for order in (["w0", "w1", "w2", "w3"], ["w3", "absent", "w0"], ["w2", "w0"], ["w1", "w3"]):
        out.append(Case("gaps", "wanted: %s" % " ".join(order), text, order, PIECE))
    return out


def _overlap(seed):
    """Hand-written indexes over one line of 250 bases: rows that share bytes of the file (faidx serves each of them), and
    rows that merely touch."""
    rng = np.random.default_rng([seed, 8])
    text = b">a\n" + _bases(rng, 250, odd=0) + b"\n"
    return [Case("overlap", "overlapping", text, ["a", "b"], PIECE, fai=[("a", 100, 3, 100, 101), ("b", 100, 53, 100, 101)]),
            Case("overlap", "nested", text, ["b", "a"], PIECE, fai=[("a", 200, 3, 200, 201), ("b", 50, 53, 50, 51)]),
            Case("overlap", "nested, three", text, ["a", "b", "c"], PIECE,
                 fai=[("a", 200, 3, 200, 201), ("b", 10, 13, 10, 11), ("c", 50, 103, 50, 51)]),
            Case("overlap", "touching", text, ["b", "a"], PIECE, fai=[("a", 100, 3, 100, 100), ("b", 100, 103, 100, 100)])]


_BUILDERS = {"phase": _phase, "crowded": _crowded, "geometry": _geometry, "alphabet": _alphabet, "tail": _tail, "gaps": _gaps,
             "overlap": _overlap}


def generate(cls, seed=0):
    return _BUILDERS[cls](seed)


@functools.lru_cache(maxsize=None)
def cases(cls, seed=0):
    """The plain files of a class."""
    return tuple(generate(cls, seed))


@functools.lru_cache(maxsize=None)
def twins(cls, seed=0):
    """The BGZF twins of a class: every text with and without a built .gzi, the block sizes in turn (``gaps``: all of them;
    ``phase``: texts of their own, so that the slab boundary visits the byte kinds); none for ``overlap``."""
    if cls == "overlap":
        return ()
    if cls == "phase":
        return tuple(_phase_twins(seed))
    out = []
    for i, case in enumerate(cases(cls, seed)):
        # (``gaps``, few cases and the class whose slabs the loader's account is held against: every block size)
        for block in (BLOCK_SIZES if cls == "gaps" else (BLOCK_SIZES[i % len(BLOCK_SIZES)],)):
            out += [case.twin(block, True), case.twin(block, False)]
    return tuple(out)
