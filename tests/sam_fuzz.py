"""Cases for the differential test of the device SAM parser (include/mdx.h mdx_gsam_*) against sam.read_sam: small SAM
files, each a header, four good record lines, the case's own line or lines and four more good lines, grouped into classes
by what they probe.  Deterministic from a seed; numpy and the standard library only.  Collects no tests:
tests/test_sam_fuzz_cases.py checks the cases themselves (no GPU), tests/test_gpu_sam_fuzz.py runs them on the device.

The hash of the library's name tables (mdx_samio.cpp upload_names, mdx_gsam.hip hash_find) is restated here (``fnv1a``,
``table_size``, ``home_slots``) so that names can be searched that share one slot of a table."""
import functools
import pathlib
import tempfile

import numpy as np

from mapdamage_amd import sam, synth

CLASSES = ("valid", "numeric", "rname", "header", "mutated", "geometry")
# (the file of tests/test_gpu_sam_decode.py: its genome, its two read groups)
RGS = [{"ID": "rgA", "SM": "s1", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s2", "LB": "lib2"}]
READGROUPS = (("rgA", 0), ("rg_b2", 1))
SEPARATORS = (b"\x0b", b"\x0c", b"\x1c", b"\x1d", b"\x1e")        # where str.splitlines() cuts and C's '\n' does not


class Case:
    """One SAM file.  ``cls``: its class; ``label``: repr of the odd line (or what else is odd); ``line_no``: the 1-based
    number of the odd line among the body lines, None where there is not exactly one; ``data``: the file's bytes;
    ``n_records``: how many records read_sam returns (stated for the classes that must parse, None otherwise);
    ``readgroups``: (id, library) pairs for GpuSamStream."""

    def __init__(self, cls, label, line_no, data, n_records, readgroups):
        self.cls, self.label, self.line_no, self.data, self.n_records = cls, label, line_no, data, n_records
        self.readgroups = tuple(readgroups)

    def __repr__(self):
        return "Case(%s, %s)" % (self.cls, self.label)


# ---- the library's name table, restated
def fnv1a(name):
    h = 2166136261
    for c in name:
        h = ((h ^ c) * 16777619) & 0xFFFFFFFF
    return h


def table_size(n):
    size = 16
    while size < 2 * n:
        size <<= 1
    return size


def home_slots(names):
    """The slot each name hashes to in the table of these names (before probing)."""
    mask = table_size(len(names)) - 1
    return [fnv1a(n) & mask for n in names]


def colliding_names(prefix, slot, size, count, skip=0):
    """``count`` names prefix + digits whose home slot in a table of ``size`` slots is ``slot`` (the first ``skip`` left out)."""
    out, i = [], 0
    while len(out) < count + skip:
        name = prefix + b"%d" % i
        if fnv1a(name) & (size - 1) == slot:
            out.append(name)
        i += 1
    return out[skip:]


# ---- good lines
def genome():
    return synth.make_genome(seed=11, sizes=(("chr1", 300_000), ("chr2", 100_000), ("chrS", 500)), n_run=500, lower_run=3000)


@functools.lru_cache(maxsize=4)
def _good(seed):
    """(header bytes, record lines) of a file sam.write_sam wrote: reads with qualities and the two read groups."""
    ref = genome()
    b = synth.make_reads(ref, 256, seed + 4, len_range=(25, 160), paired=True, frac_softclip=0.2, frac_ins=0.08, frac_del=0.08,
                         frac_skip=0.01, with_qual=True, frac_filtered=0.05)
    rng = np.random.default_rng(seed + 4)
    rg = [RGS[i]["ID"] for i in rng.integers(0, 2, size=b.n)]
    with tempfile.TemporaryDirectory() as tmp:
        path = pathlib.Path(tmp) / "good.sam"
        sam.write_sam(str(path), b, ref.names, ref.lengths, RGS, rg)
        lines = path.read_bytes().split(b"\n")[:-1]
    head = b"".join(x + b"\n" for x in lines if x.startswith(b"@"))
    return head, tuple(x for x in lines if not x.startswith(b"@"))


def qual_of(n):
    """n quality bytes, values 0 to 40 mixed (some below 20: the -Q fold has something to fold)."""
    return bytes(33 + (7 * i) % 41 for i in range(n))


def line(qname=b"q", flag=b"0", rname=b"chr1", pos=b"100", mapq=b"30", cigar=b"10M", rnext=b"*", pnext=b"0", tlen=b"0",
         seq=b"ACGTACGTAC", qual=None, tags=(b"RG:Z:rgA",)):
    if qual is None:
        qual = qual_of(len(seq))
    return b"\t".join((qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual) + tuple(tags))


def header(names=(b"chr1", b"chr2", b"chrS"), rgs=(b"rgA", b"rg_b2"), extra_front=(), extra_back=()):
    out = [b"@HD\tVN:1.6\tSO:unsorted"] + list(extra_front) + [b"@SQ\tSN:%s\tLN:%d" % (n, 1000 + i) for i, n in enumerate(names)]
    out += [b"@RG\tID:%s\tSM:s%d\tLB:lib%d" % (r, i, i) for i, r in enumerate(rgs)] + list(extra_back)
    return b"".join(x + b"\n" for x in out)


class _Builder:
    def __init__(self, cls, seed):
        self.cls, self.rng, self.cases, self.at = cls, np.random.default_rng([seed, CLASSES.index(cls)]), [], 0
        self.head, self.good = _good(seed)

    def take(self, n):
        out = [self.good[(self.at + i) % len(self.good)] for i in range(n)]
        self.at += n
        return out

    def add(self, odd, records=None, head=None, label=None, readgroups=READGROUPS, before=4, after=4, one_line=True, end=b"\n"):
        """A case around the lines ``odd`` (bytes: one line).  ``records``: how many of them are records (None: not stated)."""
        odd = [odd] if isinstance(odd, bytes) else list(odd)
        body = self.take(before) + odd + self.take(after)
        data = (self.head if head is None else head) + b"\n".join(body) + (end if body else b"")
        line_no = before + 1 if one_line and len(odd) == 1 and b"\n" not in odd[0] else None
        label = label or (repr(odd[0]) if len(odd) == 1 else repr(odd))
        if len(label) > 300:
            label = label[:140] + " ... " + label[-140:] + " (%d bytes)" % len(odd[0])
        self.cases.append(Case(self.cls, label, line_no, data, None if records is None else before + after + records, readgroups))


def _cigar_of(n_ops, rng):
    """A CIGAR of n_ops operations (M and I or D in turns, random lengths) and the SEQ length it asks for."""
    out, bases = [], 0
    for i in range(n_ops):
        k = int(rng.integers(1, 4))
        op = b"M" if i % 2 == 0 else (b"I", b"D")[int(rng.integers(0, 2))]
        out.append(b"%d%s" % (k, op))
        bases += k if op != b"D" else 0
    return b"".join(out), bases


def _bases(n, rng, alphabet=b"ACGTacgtNn"):
    return bytes(np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)])


def _valid(b):
    rng = b.rng
    for flag in (b"0", b"00000", b"16383", b"16384", b"65535"):
        b.add(line(flag=flag), 1)
    for pos in (b"0", b"1", b"-0", b"-1", b"2147483647", b"-2147483647"):
        b.add(line(pos=pos), 1)
    for tlen in (b"-2147483648", b"2147483647"):
        b.add(line(tlen=tlen), 1)
    for cigar in (b"", b"*", b"M", b"0M", b"00005M", b"268435455M", b"0268435455M", b"00000000000000000012M", b"1M268435455N1M"):
        b.add(line(cigar=cigar), 1)
    for op in b"MIDNSHP=X":
        b.add(line(cigar=b"3" + bytes([op]) + b"7M"), 1)
    for n_ops in [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 127, 255, 256, 257, 399, 400] + [int(x) for x in rng.integers(1, 401, size=8)]:
        cigar, n = _cigar_of(n_ops, rng)
        b.add(line(cigar=cigar, seq=_bases(n, rng)), 1)
    # SEQ: every ASCII byte but tab, newline and carriage return, at changing places of an odd-length SEQ
    every = np.asarray([c for c in range(128) if c not in (9, 10, 13)], np.uint8)
    for _ in range(5):
        seq = bytes(rng.permutation(every))
        b.add(line(seq=seq, cigar=b"%dM" % len(seq)), 1)
    for c in (0, ord("="), ord("."), ord("a"), ord("*"), ord("@"), 0x0b, 0x0c, 0x1c, 0x7f):
        b.add(line(seq=b"AC" + bytes([c]) + b"GT", cigar=b"5M"), 1)
    for n in [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 129, 255, 256, 257, 299, 300] + [int(x) for x in rng.integers(0, 301, size=7)]:
        b.add(line(seq=_bases(n, rng), cigar=b"%dM" % n), 1)
    b.add(line(qual=b"*"), 1)
    b.add(line(seq=b"A", qual=b"*", cigar=b"1M"), 1)
    b.add(line(seq=b"*", qual=b"*"), 1)
    b.add(line(seq=b"", qual=b""), 1)
    b.add(line(seq=b"AC", qual=b"*I", cigar=b"2M"), 1)
    b.add(line(qual=b"!" * 10), 1)
    b.add(line(qual=b"~" * 10), 1)
    b.add(line(qual=b"!" * 9 + b"~"), 1)
    # field count and tags
    b.add(line(tags=()), 1)
    b.add(line(tags=(b"",)), 1)
    b.add(line(tags=(b"RG:Z:rg_b2", b"")), 1)
    b.add(line(seq=b"", qual=b"", tags=()), 1)
    for n_tags in [0, 1, 2, 5, 13, 27, 40] + [int(x) for x in rng.integers(0, 41, size=13)]:
        tags = [b"X" + bytes(rng.integers(33, 127, size=int(rng.integers(0, 70)), dtype=np.uint8)) for _ in range(n_tags)]
        b.add(line(tags=tuple(tags) + (b"RG:Z:" + (b"rgA", b"rg_b2")[n_tags % 2],)), 1)
    b.add(line(tags=(b"RG:Z:rgA", b"RG:Z:rg_b2")), 1)
    b.add(line(tags=(b"RG:Z:rg_b2", b"XX:i:1", b"RG:Z:rgA", b"YY:Z:x")), 1)
    b.add(line(tags=(b"RG:Z:",)), 1)
    b.add(line(tags=(b"RG:Z:rgA", b"RG:Z:")), 1)
    b.add(line(tags=(b"RG:Z:", b"XX:i:1")), 1)
    b.add(line(tags=(b"XX:i:1", b"RG:Z:rg_b2")), 1)
    b.add(line(tags=(b"RG:Z:nope",)), 1)
    b.add(line(tags=(b"RG:Z:rg",)), 1)
    b.add(line(tags=(b"RG:Z:rgAA",)), 1)
    # look-alikes of the read-group tag
    for tag in (b"RG:Z", b"RG:i:5", b"XRG:Z:rgA", b"RG:Z;rgA", b"rg:z:rgA", b"RG:", b"R", b"RG:Z:rgA RG:Z:rg_b2"):
        b.add(line(tags=(tag,)), 1)
        b.add(line(tags=(b"RG:Z:rg_b2", tag)), 1)
    b.add(line(qname=b"RG:Z:rgA", tags=()), 1)
    b.add(line(qname=b"RG:Z:rgA", tags=(b"RG:Z:rg_b2",)), 1)
    b.add(line(seq=b"ACGTACGT", qual=b"RG:Z:rgA", cigar=b"8M", tags=(b"XX:i:1",)), 1)
    b.add(line(seq=b"RG:Z:rgA", cigar=b"8M", tags=()), 1)
    # lines that are no records
    for odd in (b"short\tline\tonly", b"", b"\t", b"\t" * 9, b"a\tb\tc\td\te\tf\tg\th\ti\tj", b"q\tx\tchr1\t-\t30\t5Q\t*\t0\t1e3\t*",
                b"RG:Z:rgA", b"q\t0\tchr1\t100\t30\t10M\t*\t0\t0\tACGTACGTAC"):
        b.add(odd, 0)
    b.add([b"", b""], 0)
    # random combinations of the above
    flags, poss, tlens = (b"0", b"00016", b"16383", b"65535", b"4"), (b"0", b"1", b"-1", b"2147483647", b"77"), (b"0", b"-2147483648", b"2147483647", b"-5")
    while len(b.cases) < 170:
        n = int(rng.integers(0, 120))
        cigar = (b"*", b"", b"%dM" % n, b"0%dM" % n)[int(rng.integers(0, 4))]
        qual = b"*" if rng.integers(0, 3) == 0 else None
        tags = ((), (b"RG:Z:rgA",), (b"XX:Z:" + _bases(int(rng.integers(0, 60)), rng), b"RG:Z:rg_b2"), (b"RG:Z:rgA", b""))[int(rng.integers(0, 4))]
        b.add(line(qname=b"c" * int(rng.integers(1, 40)), flag=flags[int(rng.integers(0, 5))], rname=(b"chr1", b"chr2", b"chrS", b"*")[int(rng.integers(0, 4))],
                   pos=poss[int(rng.integers(0, 5))], tlen=tlens[int(rng.integers(0, 4))], cigar=cigar, seq=_bases(n, rng, b"ACGTacgtNn=.RYKM"),
                   qual=qual, tags=tags), 1)


def _numeric(b):
    common = [b"65536", b"99999", b"100000", b"", b"-", b"--1", b"+4", b" 4", b"4 ", b"1_6", b"0x10", b"4.0", b"1e3", b"\x004", b"4\x00",
              b"4294967296", b"4294967297", b"12345678901234567890", b"7" * 5000, b"\x0b4", b"4\x0c", b"\x1c4", b"4\x1f", b"+", b"-+4", b"_4", b"4_",
              b"000000004", b"-4", b"\xe0\xa5\xaa", b"4,0", b"0b1", b"4 4"]
    for value in common:
        b.add(line(flag=value))
        b.add(line(pos=value))
        b.add(line(tlen=value))
    for value in (b"2147483648", b"2147483649", b"-2147483648", b"-2147483649", b"4294967295", b"-4294967296", b"-4294967297"):
        b.add(line(pos=value))
    for value in (b"2147483648", b"-2147483649", b"2147483649", b"-2147483650", b"4294967295", b"-4294967296", b"-4294967297", b"-12345678901234567890"):
        b.add(line(tlen=value))
    for value in (b"**", b"*M", b"5", b"5M5", b"5m", b"5M ", b"268435456M", b"1000000000M", b"4294967297M", b"5Q", b" 5M", b"5M*", b"M5", b"-5M", b"+5M",
                  b"5\x00M", b"5M\x00", b"4294967296M", b"4294967301M", b"99999999999999999999M", b"5M1000000000I", b"10000000000M", b"5MM5", b"0", b"=", b"5B"):
        b.add(line(cigar=value))
    for seq, qual in ((b"AC", b"*I"), (b"ACGTACGTAC", qual_of(9)), (b"ACGTACGTAC", qual_of(11)), (b"*", b"IIII"), (b"*", b"I"), (b"A", b""), (b"", b"I"),
                      (b"ACGT", b"II I"), (b"ACGT", b"II\x1fI"), (b"ACGT", b"II\x00I"), (b"ACGT", b" III"), (b"ACGT", b"III "), (b"ACGT", b"\x00\x00\x00\x00"),
                      (b"ACGT", b"**"), (b"ACGT", b"*"), (b"*", b"*"), (b"A", b" "), (b"ACGTACGTA", b"IIIIIIII\x20"), (b"ACGT", b"II\x7fI")):
        b.add(line(seq=seq, qual=qual, cigar=b"%dM" % max(1, len(seq))))


def _rname(b):
    rng = b.rng
    long_name = b"L" * 300
    for rname in (b"*", b"", b"CHR1", b"Chr1", b"chr", b"chr1x", b"chr3", b"chr1 ", b" chr1", b"chr1\x00", b"chr2", b"chrS", b"chrs", long_name, b"=", b"c"):
        b.add(line(rname=rname))
    head = header(names=(b"chr1", long_name, b"chr2", long_name[:-1] + b"M", b""))
    for rname in (long_name, long_name[:-1], long_name + b"L", long_name[:-1] + b"M", long_name[:-1] + b"N", b"", b"*", b"chr2"):
        b.add(line(rname=rname), head=head)
    head = header(names=(b"*", b"chr1"))
    for rname in (b"*", b"chr1", b"**"):
        b.add(line(rname=rname), head=head)
    # the sizes at which the table of names doubles
    for n in (1, 8, 9, 16, 17, 1000):
        names = ([b"chr1", b"chr2", b"chrS"] + [b"n%d" % i for i in range(n)])[:n]
        head = header(names=names)
        picks = {0, n - 1, n // 2, n // 3, int(rng.integers(0, n)), int(rng.integers(0, n))}
        for i in sorted(picks):
            b.add(line(rname=names[i]), head=head)
        for rname in (names[-1] + b"0", names[-1][:-1], b"n%d" % n, b"N0"):
            b.add(line(rname=rname), head=head)
    # names that share a slot of the table, and absent names that hash into their chain; the chain at slot 14 of 16 wraps
    for slot in (5, 14):
        chain = colliding_names(b"ctg", slot, 16, 5)
        absent = colliding_names(b"ctg", slot, 16, 8, skip=5) + colliding_names(b"ctg", (slot + 2) & 15, 16, 3)
        names = chain + [b"chr1"]
        head = header(names=names)
        for rname in chain + absent + [chain[0][:-1], chain[-1] + b"0"]:
            b.add(line(rname=rname), head=head)
        # ... and the same for read-group ids
        rg_chain = colliding_names(b"grp", slot, 16, 5)
        rg_absent = colliding_names(b"grp", slot, 16, 8, skip=5) + colliding_names(b"grp", (slot + 2) & 15, 16, 3)
        ids = rg_chain + [b"rgA", b"rg_b2"]
        head = header(rgs=ids)
        groups = tuple((r.decode(), i) for i, r in enumerate(ids))
        for rg in rg_chain + rg_absent + [rg_chain[0][:-1], b""]:
            b.add(line(tags=(b"XX:i:1", b"RG:Z:" + rg)), head=head, readgroups=groups)


def chains():
    """The name sets of the ``rname`` class that are built to collide: (names of the table, the colliding ones)."""
    out = []
    for slot in (5, 14):
        chain = colliding_names(b"ctg", slot, 16, 5)
        out.append((chain + [b"chr1"], chain))
        chain = colliding_names(b"grp", slot, 16, 5)
        out.append((chain + [b"rgA", b"rg_b2"], chain))
    return out


def _header(b):
    rec_x = line(rname=b"x")
    b.add(line(), head=b"", one_line=False)
    b.add([], head=b.head, before=0, after=0, label="a header and no records")
    b.add([], head=b.head[:-1], before=0, after=0, label="a header without its last newline and no records")
    b.add([], head=b"", before=0, after=0, label="an empty file")
    b.add(line(), head=header(extra_front=(b"@",)), one_line=False)
    b.add(line(), head=b"@\n", one_line=False)
    b.add(line(), head=header(extra_back=(b"@SQ\tSN:x",)), one_line=False)
    b.add(line(), head=header(extra_back=(b"@SQ\tLN:5",)), one_line=False)
    b.add(line(), head=header(extra_back=(b"@SQ",)), one_line=False)
    b.add(line(), head=header(extra_back=(b"@SQ\t",)), one_line=False)
    b.add(line(rname=b"chr1"), head=header(extra_back=(b"@SQ\tSN:chr1\tLN:5",)), one_line=False)
    b.add(line(rname=b"chr1"), head=header(extra_front=(b"@SQ\tSN:chr1\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ\tSN:x\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ\tLN:5\tSN:x",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ\tSN:y\tSN:x\tLN:5",)), one_line=False)
    b.add(line(rname=b"y"), head=header(extra_back=(b"@SQ\tSN:y\tSN:x\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ\tXSN:x\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ\tXSN:y\tSN:x\tLN:5",)), one_line=False)
    b.add(line(rname=b"x:y"), head=header(extra_back=(b"@SQ\tSN:x:y\tLN:5",)), one_line=False)
    b.add(line(rname=b""), head=header(extra_back=(b"@SQ\tSN:\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@sq\tSN:x\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQX\tSN:x\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ SN:x\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ\tSN:x\tLN:5\t",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ\t\tSN:x\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ\tSN:x\tLN:5\tLN:x",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@CO\tfoo\x00bar", b"@SQ\tSN:x\tLN:5")), one_line=False)
    b.add(line(rname=b"x\x00y"), head=header(extra_back=(b"@SQ\tSN:x\x00y\tLN:5",)), one_line=False)
    b.add(rec_x, head=header(extra_back=(b"@SQ\tSN:x\x00y\tLN:5",)), one_line=False)
    for ln in (b"+5", b" 5", b"5 ", b"5_0", b"00", b"-5", b"", b"abc", b"1.5", b"5\x00", b"1" * 25, b"0x5", b"1e3"):
        b.add(rec_x, head=header(extra_back=(b"@SQ\tSN:x\tLN:" + ln,)), one_line=False)
    # @SQ behind @RG (header() writes the extra lines behind the read groups), and a header of read groups alone
    b.add(rec_x, head=header(names=(), extra_back=(b"@SQ\tSN:chr1\tLN:9", b"@SQ\tSN:x\tLN:5")), one_line=False)
    b.add(rec_x, head=header(names=()), one_line=False)
    # lines that start with '@' behind the first record are the header's to read_sam
    b.add(line(qname=b"@q"))
    b.add(line(qname=b"@SQ", rname=b"chr2"))
    b.add(b"@CO\ta comment behind the first record")
    b.add(b"@SQ\tSN:late\tLN:5")
    b.add(b"@SQ\tSN:late")
    b.add(b"@")
    b.add([b"@SQ\tSN:late\tLN:5", line(rname=b"late")], one_line=False)
    # a separator of str.splitlines() in a header line, in front of text shaped like an @SQ line
    for sep in SEPARATORS + (b"\x1f", b" ", b"\x00"):
        for kind in (b"@CO\tfoo", b"@PG\tID:bwa\tPN:bwa", b"@RG\tID:zz\tSM:s"):
            for shaped in (b"@SQ\tSN:x\tLN:5", b"@SQ\tSN:chr2\tLN:5", b"@SQ\tSN:x", b"@SQ\tLN:5"):
                for front in (True, False):
                    extra = (kind + sep + shaped,)
                    b.add(rec_x, head=header(extra_front=extra) if front else header(extra_back=extra), one_line=False,
                          label=repr(extra[0]) + (" in front of the @SQ lines" if front else " behind the @RG lines"))


_EDIT_BYTES = (b"0123456789", b"+-_ *=.@:", b"\t\n\x00\x1f\x7f", b"MIDNSHPXRGZmid", b"\r", bytes(range(0x80, 0x100)))
_EDIT_WEIGHTS = (0.30, 0.20, 0.15, 0.30, 0.025, 0.025)


def _mutated(b, n=180):
    rng = b.rng
    for _ in range(n):
        good = bytearray(b.take(1)[0])
        for _ in range(int(rng.integers(1, 4))):
            tabs = [i for i, c in enumerate(good) if c == 9]
            front = tabs[8] if len(tabs) > 8 else len(good)
            span = front if rng.random() < 0.7 and front > 0 else len(good)
            at = int(rng.integers(0, max(1, span)))
            group = _EDIT_BYTES[int(rng.choice(len(_EDIT_BYTES), p=_EDIT_WEIGHTS))]
            byte = group[int(rng.integers(0, len(group)))]
            kind = int(rng.integers(0, 3))
            if kind == 0 and good:
                good[at] = byte
            elif kind == 1:
                good.insert(at, byte)
            elif good:
                del good[at]
        b.add(bytes(good))


def _geometry(b):
    """Multi-slab files of valid lines: QNAMEs of 1 to 320 bytes, so that lines start and end at every offset mod 32 (the first
    QNAME ``shift`` bytes longer moves them all), a line of more than 65 536 bytes and one of more than 131 072, with and
    without the last newline, and with a line padded to end exactly on byte 65 536 behind the header."""
    rng = b.rng
    long_a, long_b = _bases(33_001, rng), _bases(66_003, rng)
    for shift in range(32):
        for variant in ("newline", "no newline") + (("boundary",) if shift % 4 == 0 else ()):
            lines = []
            for k in range(1, 321):
                n = int(rng.integers(0, 40))
                tags = ((b"RG:Z:rgA",), (b"RG:Z:rg_b2",), (), (b"XX:i:%d" % k, b"RG:Z:rgA"))[k % 4]
                lines.append(line(qname=b"g" * (k + (shift if k == 1 else 0)), rname=(b"chr1", b"chr2")[k % 2], pos=b"%d" % (k * 7), cigar=b"%dM" % n if n else b"*",
                                  seq=_bases(n, rng), tags=tags))
                if k == 100:
                    lines.append(line(qname=b"longA", cigar=b"%dM" % len(long_a), seq=long_a, tags=(b"RG:Z:rg_b2",)))
                if k == 300:
                    lines.append(line(qname=b"longB", cigar=b"%dM" % len(long_b), seq=long_b, tags=(b"XX:Z:" + b"x" * 100, b"RG:Z:rgA")))
            if variant == "boundary":
                end = 0
                for i, x in enumerate(lines):
                    if end + len(x) + 1 > 65536:
                        break
                    end += len(x) + 1
                # (the lines in front of line i take `end` bytes: the last of them made longer until they take 65 536)
                lines[i - 1] = b"g" * (65536 - end) + lines[i - 1]
            body = b"\n".join(lines) + (b"" if variant == "no newline" else b"\n")
            b.cases.append(Case(b.cls, "geometry: first QNAME %d bytes longer, %s" % (shift, variant), None, b.head + body, len(lines), READGROUPS))


_MAKERS = {"valid": _valid, "numeric": _numeric, "rname": _rname, "header": _header, "mutated": _mutated, "geometry": _geometry}


def generate(cls, seed=0):
    """The cases of a class, made afresh."""
    b = _Builder(cls, seed)
    _MAKERS[cls](b)
    return b.cases


@functools.lru_cache(maxsize=None)
def cases(cls, seed=0):
    """... and kept: both GPU runs and the CPU tests read the same objects."""
    return tuple(generate(cls, seed))


def host_verdict(case, path=None):
    """What read_sam makes of the case: (Alignments, None), or (None, the exception).  ``path``: the file, where the caller
    has written one; text is decoded and cut into lines as open(path, 'rt') does either way."""
    import io
    try:
        if path is not None:
            return sam.read_sam(str(path)), None
        return sam.read_sam(io.TextIOWrapper(io.BytesIO(case.data))), None
    except Exception as exc:          # noqa: BLE001 (any type: that is the contract)
        return None, exc
