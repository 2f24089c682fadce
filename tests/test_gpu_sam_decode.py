"""SAM text parsed on the GPU (include/mdx.h mdx_gsam_*): the columns equal sam.read_sam's, the command line writes the
reference's tables from a file, a pipe, a FIFO, /dev/fd/N and `< x.sam` with no fallback, and where Python's parser could read
a line otherwise the device path gives up and the host parser has the last word."""
import pathlib

import numpy as np
import pytest

from mapdamage_amd import fasta, sam, synth
from tests.test_gpu_decode import _d2h
from tests.test_gpu_pipe_input import FILES, GOLDENS, ROOT, _cli, _main_on_pipe, _tables

pytestmark = pytest.mark.gpu

RGS = [{"ID": "rgA", "SM": "s1", "LB": "lib1"}, {"ID": "rg_b2", "SM": "s2", "LB": "lib2"}]
LIB_OF = {"rgA": 0, "rg_b2": 1}
CODE = {ord("A"): 1, ord("C"): 2, ord("T"): 4, ord("G"): 8}


def _genome():
    return synth.make_genome(seed=11, sizes=(("chr1", 300_000), ("chr2", 100_000), ("chrS", 500)), n_run=500, lower_run=3000)


def _reads(ref, n, seed=4, with_qual=True):
    b = synth.make_reads(ref, n, seed, len_range=(25, 160), paired=True, frac_softclip=0.2, frac_ins=0.08, frac_del=0.08,
                         frac_skip=0.01, with_qual=with_qual, frac_filtered=0.05)
    rng = np.random.default_rng(seed)
    return b, [RGS[i]["ID"] for i in rng.integers(0, 2, size=b.n)]


def _edge_lines():
    """Lines for every rule of read_sam's table: '*' fields, POS 0, unknown RNAME, negative TLEN, the nine CIGAR operations,
    a CIGAR of 320 operations, lower-case / IUPAC / '=' bases, several RG:Z tags, short and empty lines."""
    q = lambda n: "".join(chr(33 + (7 * i) % 41) for i in range(n))
    return [
        "u1\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*",
        "u2\t0\tchrZ\t17\t0\t5M\t*\t0\t-150\tACGTN\t%s\tRG:Z:rgA" % q(5),
        "u3\t16\tchr1\t1000\t30\t2S3M1I2M1D2N1P2=1X1H\t*\t0\t-42\tacgtRYKM=n.\t%s\tRG:Z:rgA\tXX:i:1\tRG:Z:rg_b2" % q(11),
        "u4\t0\tchr2\t5000\t30\t%s\t*\t0\t99\t%s\t*\tRG:Z:rg_b2" % ("1M1I" * 160, "ACGTacgtNN" * 32),
        "short\tline\tonly",
        "",
        "u5\t65535\tchrS\t1\t0\t10M\t*\t0\t2147483647\tGGGGGCCCCC\t%s\tRG:Z:nope" % q(10),
        "u6\t1\tchr1\t2147483647\t0\t*\t*\t0\t-2147483648\tAC\t!!",
        "u7\t0\tchr1\t5\t0\t0M\t*\t0\t0\t\t",
    ]


def _write_sam(path, ref, b, rg, extra=(), at=None, newline_at_end=True):
    sam.write_sam(str(path), b, ref.names, ref.lengths, RGS, rg)
    lines = path.read_text().split("\n")[:-1]
    head = [x for x in lines if x.startswith("@")]
    body = [x for x in lines if not x.startswith("@")]
    at = len(body) // 2 if at is None else at
    body[at:at] = list(extra)
    path.write_text("\n".join(head + body) + ("\n" if newline_at_end else ""))


def _pack(seq, qual, seq_off, minqual):
    """read_sam's SEQ column in the MDX_SEQ_4BIT form (low nibble first), under -Q the masked nibbles complemented."""
    codes = np.zeros(seq.shape[0], np.uint8)
    for ch, c in CODE.items():
        codes[seq == ch] = c
    if minqual:
        low = (qual != 0xFF) & (qual < minqual)
        codes[low] ^= 15
    if codes.shape[0] % 2:
        codes = np.concatenate([codes, np.zeros(1, np.uint8)])
    return codes[0::2] | (codes[1::2] << 4)


def _device_columns(eng, path, chunk, minqual, packed):
    cols = {k: [] for k in ("flag", "lib", "tid", "pos", "tlen", "cigar", "seq", "qual", "clen", "slen")}
    with sam.GpuSamStream(eng, str(path), readgroups=list(LIB_OF.items()), chunk_bytes=chunk, want_qual=True,
                          min_basequal=minqual, packed=packed) as g:
        while True:
            v = g.next_view()
            if v is None:
                break
            eng.sync()
            k, nb = int(v.n_reads), int(v.n_bases)
            cols["flag"].append(_d2h(v.flag, k, np.uint16)); cols["lib"].append(_d2h(v.lib, k, np.uint16))
            for name in ("tid", "pos", "tlen"):
                cols[name].append(_d2h(getattr(v, name), k, np.int32))
            co, so = _d2h(v.cigar_off, k + 1, np.uint32), _d2h(v.seq_off, k + 1, np.uint32)
            assert co[0] == 0 and so[0] == 0 and co[-1] == v.n_cigar and so[-1] == nb
            cols["clen"].append(np.diff(co)); cols["slen"].append(np.diff(so))
            cols["cigar"].append(_d2h(v.cigar, int(v.n_cigar), np.uint32))
            if packed:
                # (the slab's own nibbles, unpacked: a slab's column starts at nibble 0)
                raw = _d2h(v.seq, (nb + 1) // 2, np.uint8)
                cols["seq"].append(np.stack([raw & 15, raw >> 4], 1).reshape(-1)[:nb])
            else:
                cols["seq"].append(_d2h(v.seq, nb, np.uint8))
            cols["qual"].append(_d2h(v.qual, nb, np.uint8) if v.qual else None)
        missing = g.missing_qualities()
    return cols, missing


@pytest.mark.parametrize("chunk", [1 << 28, 4096])
def test_columns_equal_read_sam(tmp_path, chunk):
    from mapdamage_amd.engine import DamageEngine
    ref = _genome()
    b, rg = _reads(ref, 3000)
    path = tmp_path / "x.sam"
    _write_sam(path, ref, b, rg, extra=_edge_lines(), newline_at_end=False)
    host = sam.read_sam(str(path))
    hb = host.batch
    want_lib = np.asarray([LIB_OF.get(r, 0xFFFF) if r is not None else 0xFFFF for r in host.rg], np.uint16)
    seq_lens = np.diff(hb.seq_off.astype(np.int64))
    for minqual, packed in ((0, False), (0, True), (20, True)):
        with DamageEngine([("s1", "lib1"), ("s2", "lib2")], 70, 10, minqual) as eng:
            eng.set_reference(ref)
            cols, missing = _device_columns(eng, path, chunk, minqual, packed)
        got = {k: np.concatenate(v) for k, v in cols.items() if k not in ("qual", "seq")}
        assert got["flag"].shape[0] == hb.n
        np.testing.assert_array_equal(got["flag"] & 0x3FFF, hb.flag)
        for name in ("tid", "pos", "tlen", "cigar"):
            np.testing.assert_array_equal(got[name], getattr(hb, name), err_msg=name)
        np.testing.assert_array_equal(got["clen"], np.diff(hb.cigar_off)); np.testing.assert_array_equal(got["slen"], seq_lens)
        np.testing.assert_array_equal(got["lib"], want_lib)
        first = hb.qual[np.minimum(hb.seq_off[:-1].astype(np.int64), hb.qual.shape[0] - 1)]
        has_qual = (seq_lens > 0) & (first != 0xFF)
        np.testing.assert_array_equal((got["flag"] & 0x4000) != 0, has_qual)
        if packed:
            codes = np.concatenate(cols["seq"])
            want = _pack(hb.seq, hb.qual, hb.seq_off, minqual)
            want = np.stack([want & 15, want >> 4], 1).reshape(-1)[:hb.seq.shape[0]]
            np.testing.assert_array_equal(codes, want)
        else:
            np.testing.assert_array_equal(np.concatenate(cols["seq"]), hb.seq)
        if minqual == 0:
            np.testing.assert_array_equal(np.concatenate(cols["qual"]), hb.qual)
        else:
            qmin = np.asarray([hb.qual[a:z].min() if z > a else 0xFF for a, z in zip(hb.seq_off[:-1], hb.seq_off[1:])])
            np.testing.assert_array_equal((got["flag"] & 0x8000) != 0, qmin >= minqual)
            counted = (hb.flag & 0xF04) == 0
            assert missing == bool((counted & ~has_qual).any())
    # the hint bits equal those the BAM decoder sets on the same records
    bam = tmp_path / "x.bam"
    sam.write_bam(str(bam), hb, ref.names, ref.lengths, RGS, [r if r in LIB_OF else None for r in host.rg])
    with DamageEngine([("s1", "lib1"), ("s2", "lib2")], 70, 10, 20) as eng:
        eng.set_reference(ref)
        flags = []
        with sam.GpuBamStream(eng, str(bam), readgroups=list(LIB_OF.items()), want_qual=True, min_basequal=20) as g:
            while (v := g.next_view()) is not None:
                eng.sync()
                flags.append(_d2h(v.flag, int(v.n_reads), np.uint16))
        cols, _ = _device_columns(eng, path, chunk, 20, True)
    np.testing.assert_array_equal(np.concatenate(cols["flag"]), np.concatenate(flags))


def _golden_sam(tmp_path, golden, extra):
    from tests.util import Golden
    g = Golden(golden)
    rgs = [{"ID": "rg%d" % i, "SM": s, "LB": l} for i, (s, l) in enumerate(g.meta["libraries"])]
    raw_lib = np.load(str(ROOT / "tests" / "golden" / (golden + ".npz")))["lib"]
    if "--merge-libraries" in extra:
        rgs = [{"ID": "rg0", "SM": "a", "LB": "b"}, {"ID": "rg1", "SM": "c", "LB": "d"}]
        rg_of = ["rg%d" % (i % 2) for i in range(g.batch.n)]
    else:
        rg_of = ["rg%d" % int(x) for x in raw_lib]
    path = tmp_path / "in.sam"
    sam.write_sam(str(path), g.batch, g.ref.names, g.ref.lengths, rgs, rg_of)
    fasta.write_fasta(tmp_path / "ref.fa", g.ref)
    return g, path


@pytest.mark.parametrize("golden,extra", GOLDENS)
def test_goldens_from_sam_on_the_device(tmp_path, golden, extra):
    """The reference's three tables, byte for byte, from SAM text as a file, through a pipe, a FIFO, /dev/fd/N and `< x.sam`
    — parsed on the device (this fails where SAM text always took the host parser)."""
    from mapdamage_amd.main import main
    g, path = _golden_sam(tmp_path, golden, extra)
    want = [g.txt[f] for f in FILES]
    base = ["-r", tmp_path / "ref.fa", "--no-stats", "--log-level", "DEBUG"] + extra
    runs = []
    out = tmp_path / "file"
    assert main(["-i", str(path), "-d", str(out)] + [str(a) for a in base]) == 0
    runs.append(out)
    for kind in ("fifo", "devfd"):
        out = tmp_path / kind
        assert _main_on_pipe(tmp_path, path.read_bytes(), ["-d", out] + base, kind) == 0
        runs.append(out)
    out = tmp_path / "pipe"
    _, err, rc = _cli(["-i", "-", "-d", out] + base, data=path.read_bytes())
    assert rc == 0, err.decode()[-2000:]
    runs.append(out)
    out = tmp_path / "redirect"
    _, err, rc = _cli(["-i", "-", "-d", out] + base, stdin_file=path)
    assert rc == 0, err.decode()[-2000:]
    runs.append(out)
    for out in runs:
        assert _tables(out) == want, out.name
        assert "Decode path: device; fallbacks from the device path: 0" in (out / "Runtime_log.txt").read_text(), out.name


@pytest.mark.parametrize("opts", [["-Q", "20"], ["--downsample", "0.3", "--downsample-seed", "7"]])
def test_many_slabs_equal_the_host_parser(tmp_path, opts, monkeypatch):
    from mapdamage_amd.main import main
    ref = _genome()
    fasta.write_fasta(tmp_path / "ref.fa", ref)
    b, rg = _reads(ref, 20_000)
    path = tmp_path / "x.sam"
    _write_sam(path, ref, b, rg)
    monkeypatch.setenv("MDX_GBAM_SLAB_BYTES", "65536")
    base = ["-r", tmp_path / "ref.fa", "--no-stats", "--log-level", "DEBUG"] + opts
    assert main(["-i", str(path), "-d", str(tmp_path / "host"), "--host-decode"] + [str(a) for a in base]) == 0
    assert main(["-i", str(path), "-d", str(tmp_path / "file")] + [str(a) for a in base]) == 0
    assert _main_on_pipe(tmp_path, path.read_bytes(), ["-d", tmp_path / "pipe"] + base, "devfd") == 0
    for name in ("file", "pipe"):
        assert _tables(tmp_path / name) == _tables(tmp_path / "host"), name
        assert "Decode path: device; fallbacks from the device path: 0" in (tmp_path / name / "Runtime_log.txt").read_text()


def _last_line(err):
    lines = [x for x in err.decode(errors="replace").strip().splitlines() if x.strip()]
    return lines[-1] if lines else ""


def _odd(kind, i):
    q = "I" * 10
    return {
        "high_byte": "ré%d\t0\tchr1\t100\t30\t10M\t*\t0\t0\tACGTACGTAC\t%s\tRG:Z:rgA" % (i, q),
        "carriage_return": "rcr%d\t0\tchr1\t100\t30\t10M\t*\t0\t0\tACGTACGTAC\t%s\tRG:Z:rgA\r" % (i, q),
        "late_header": "@CO\ta comment behind the first record",
        "flag": "rf%d\t+16\tchr1\t100\t30\t10M\t*\t0\t0\tACGTACGTAC\t%s\tRG:Z:rgA" % (i, q),
        "flag_big": "rf%d\t65536\tchr1\t100\t30\t10M\t*\t0\t0\tACGTACGTAC\t%s\tRG:Z:rgA" % (i, q),
        "pos": "rp%d\t0\tchr1\t1_00\t30\t10M\t*\t0\t0\tACGTACGTAC\t%s\tRG:Z:rgA" % (i, q),
        "tlen": "rt%d\t0\tchr1\t100\t30\t10M\t*\t0\t99999999999\tACGTACGTAC\t%s\tRG:Z:rgA" % (i, q),
        "cigar_op": "rc%d\t0\tchr1\t100\t30\t10Q\t*\t0\t0\tACGTACGTAC\t%s\tRG:Z:rgA" % (i, q),
        "cigar_long": "rc%d\t4\tchr1\t100\t30\t268435456M\t*\t0\t0\tACGTACGTAC\t%s\tRG:Z:rgA" % (i, q),
        "cigar_digits": "rc%d\t0\tchr1\t100\t30\t10M5\t*\t0\t0\tACGTACGTAC\t%s\tRG:Z:rgA" % (i, q),
        "qual_len": "rq%d\t0\tchr1\t100\t30\t10M\t*\t0\t0\tACGTACGTAC\tIIII\tRG:Z:rgA" % i,
        "qual_low": "rq%d\t0\tchr1\t100\t30\t10M\t*\t0\t0\tACGTACGTAC\tIIII IIIII\tRG:Z:rgA" % i,
        "seq_star": "rs%d\t4\tchr1\t100\t30\t*\t*\t0\t0\t*\tIIII\tRG:Z:rgA" % i,
    }[kind]


@pytest.mark.parametrize("kind", ["high_byte", "carriage_return", "late_header", "flag", "flag_big", "pos", "tlen", "cigar_op",
                                  "cigar_long", "cigar_digits", "qual_len", "qual_low", "seq_star"])
def test_give_ups_leave_the_host_parser_the_last_word(tmp_path, kind):
    """One line read_sam could read otherwise than the device parser, in the third slab: the device path gives up once, and
    the exit status, tables or error text are --host-decode's; on a pipe the host parser takes over at that slab's first
    line and the outcome is the file's."""
    ref = _genome()
    fasta.write_fasta(tmp_path / "ref.fa", ref)
    b, rg = _reads(ref, 1500)
    path = tmp_path / "x.sam"
    _write_sam(path, ref, b, rg, extra=[_odd(kind, 0)], at=1000)
    env = {"MDX_GBAM_SLAB_BYTES": "65536"}
    base = ["-r", tmp_path / "ref.fa", "--no-stats", "--log-level", "DEBUG"]
    res = {}
    for name, args, data in (("host", ["-i", path, "--host-decode"], None), ("file", ["-i", path], None),
                             ("pipe", ["-i", "-"], path.read_bytes())):
        out = tmp_path / name
        _, err, rc = _cli(args + ["-d", out] + base, data=data if data is not None else b"", env=env)
        res[name] = (rc, _tables(out) if rc == 0 else _last_line(err).replace(repr(str(path)), "X").replace("'-'", "X"), out)
    assert res["file"][:2] == res["host"][:2], (res["file"][1], res["host"][1])
    assert res["pipe"][:2] == res["file"][:2], (res["pipe"][1], res["file"][1])
    for name in ("file", "pipe"):
        log = (res[name][2] / "Runtime_log.txt").read_text()
        assert log.count("GPU decode path gave up") == 1, (name, log[-3000:])
        if res[name][0] == 0:
            assert "fallbacks from the device path: 1" in log
    assert "from byte offset" in (res["pipe"][2] / "Runtime_log.txt").read_text()


@pytest.mark.parametrize("case", ["missing", "unlisted", "filtered"])
def test_read_group_errors_are_the_host_paths(tmp_path, case):
    ref = _genome()
    fasta.write_fasta(tmp_path / "ref.fa", ref)
    b, rg = _reads(ref, 1500)
    keep = np.nonzero((b.flag & 0xF04) == 0)[0]
    drop = np.nonzero((b.flag & 0xF04) != 0)[0]
    i = int(keep[len(keep) * 2 // 3]) if case != "filtered" else int(drop[len(drop) * 2 // 3])
    rg = list(rg)
    rg[i] = None if case in ("missing", "filtered") else "zz"
    path = tmp_path / "x.sam"
    _write_sam(path, ref, b, rg, at=0)
    base = ["-r", tmp_path / "ref.fa", "--no-stats"]
    res = {}
    for name, args, data in (("host", ["-i", path, "--host-decode"], b""), ("file", ["-i", path], b""),
                             ("pipe", ["-i", "-"], path.read_bytes())):
        out = tmp_path / name
        _, err, rc = _cli(args + ["-d", out] + base, data=data, env={"MDX_GBAM_SLAB_BYTES": "65536"})
        res[name] = (rc, _tables(out) if rc == 0 else _last_line(err).replace(repr(str(path)), "X").replace("'-'", "X"))
    assert res["file"] == res["host"] and res["pipe"] == res["host"], res
    assert (res["host"][0] == 0) == (case == "filtered")
    if case != "filtered":
        assert "read-group" in res["host"][1]


def test_min_basequal_without_qualities_warns_once(tmp_path):
    from mapdamage_amd.main import main
    ref = _genome()
    fasta.write_fasta(tmp_path / "ref.fa", ref)
    b, rg = _reads(ref, 3000, with_qual=False)
    path = tmp_path / "x.sam"
    _write_sam(path, ref, b, rg)
    for name, extra in (("host", ["--host-decode"]), ("dev", [])):
        assert main(["-i", str(path), "-d", str(tmp_path / name), "-r", str(tmp_path / "ref.fa"), "--no-stats", "-Q", "20",
                     "--log-level", "DEBUG"] + extra) == 0
    log = (tmp_path / "dev" / "Runtime_log.txt").read_text()
    assert log.count("Reads without PHRED scores found; cannot filter by --min-basequal") == 1
    assert "Decode path: device; fallbacks from the device path: 0" in log
    assert _tables(tmp_path / "dev") == _tables(tmp_path / "host")
