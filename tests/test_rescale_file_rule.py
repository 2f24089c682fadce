"""tests/rescale_file_rule.py held against what the project already trusts, without a GPU: the generator's mix is what the GPU
tests need it to be, the rule writes the records the host write-back (``mdx_bam_patch_rescaled``) writes from the oracle's
outputs, it reproduces the reference's own golden, and its tag walk tells an MR tag from bytes that only look like one."""

import struct

import numpy as np
import pytest

from mapdamage_amd import sam
from tests import rescale_file_rule as F


@pytest.fixture(scope="module")
def mix(tmp_path_factory):
    """The default mix as a file, read back, with the oracle's qualities, sums and routing."""
    from oracle import oracle
    ref, header, bodies, kinds = F.make_mix()
    path = tmp_path_factory.mktemp("rule") / "mix.bam"
    sam.write_bam_raw(str(path), header, bodies)
    al = sam.read_bam(path, keep_raw=True)
    model, corr, _ = F.make_model()
    qual_out, mr, status = oracle.rescale(ref, al.batch, corr, F.L5, F.L3)         # raises on no record: nothing is left out
    return dict(ref=ref, path=path, bodies=bodies, kinds=kinds, al=al, model=model, qual_out=qual_out, mr=mr, status=status)


def test_the_file_holds_the_generated_records(mix):
    assert [bytes(r) for r in mix["al"].raw] == mix["bodies"] and mix["al"].raw_header == F.raw_header(mix["ref"])


def test_conditions_on_the_default_mix(mix):
    al, status, qual_out, mr = mix["al"], mix["status"], mix["qual_out"], mix["mr"]
    got = np.bincount(status, minlength=5)
    assert got.shape[0] == 5 and (got >= 20).all(), got
    off = al.batch.seq_off.astype(np.int64)
    changed = np.add.reduceat(np.concatenate([(qual_out != al.batch.qual).astype(np.int64), [0]]), off[:-1])
    changed[off[:-1] == off[1:]] = 0
    rescaled = (status == F.SINGLE_END) | (status == F.INWARD_PAIR)
    assert not changed[~rescaled].any() and np.isnan(mr[~rescaled]).all() and not np.isnan(mr[rescaled]).any()
    untouched = rescaled & (changed == 0) & (mr == 0.0)
    assert untouched.sum() >= 20 and (rescaled & (changed > 1)).sum() >= 20
    # ... and the kinds the GPU tests lean on are all there
    kinds, f = mix["kinds"], [F.fields(b) for b in mix["bodies"]]
    assert set(kinds) == set(F.KINDS)
    assert {x["l_name"] for x in f} >= {2, 255}
    assert any(x["l_seq"] == 0 for x in f) and any(x["tid"] == -1 for x in f)
    assert any(x["flag"] & 16 for x, r in zip(f, rescaled) if r) and any(not x["flag"] & 16 for x, r in zip(f, rescaled) if r)
    assert any(status[i] == F.INWARD_PAIR and f[i]["flag"] & 0x40 for i in range(len(f)))
    assert any(status[i] == F.INWARD_PAIR and f[i]["flag"] & 0x80 for i in range(len(f)))
    assert any(0 < x["l_seq"] < 12 for x, r in zip(f, rescaled) if r)
    ops = set()
    for b, x in zip(mix["bodies"], f):
        at = 32 + x["l_name"]
        ops |= {struct.unpack_from("<I", b, at + 4 * k)[0] & 15 for k in range(x["n_cigar"])}
    assert ops >= {F.OPS[c] for c in "MIDNSH=X"}
    types = set()
    for b, r in zip(mix["bodies"], rescaled):
        tags = F.walk_tags(b)
        types |= {t for _n, t, _v, _e in tags}
        names = [n for n, _t, _v, _e in tags]
        assert not (r and b"MR" in names)                       # the default mix stops no route
    assert types == {b"A", b"c", b"C", b"s", b"S", b"i", b"I", b"f", b"Z", b"H", b"B"}
    carried = [[n for n, _t, _v, _e in F.walk_tags(b)] for b in mix["bodies"]]
    assert sum(1 for names in carried if b"MR" in names and 0 < names.index(b"MR") < len(names) - 1) >= 20
    assert sum(1 for b in mix["bodies"] if not F.walk_tags(b)) >= 20


def test_rule_against_the_host_write_back(mix):
    """``BamStream(keep_raw=True)`` + ``patch_rescaled`` — mdx_bam_patch_rescaled — fed with the oracle's outputs, in chunks of a
    few kilobytes: the bytes of every record."""
    from mapdamage_amd.rescale import round_mr
    want = F.rule(mix["al"].raw, mix["al"].batch.seq_off, mix["qual_out"], mix["mr"], mix["status"])
    assert isinstance(want, list)
    rescaled = ((mix["status"] == F.SINGLE_END) | (mix["status"] == F.INWARD_PAIR)).astype(np.uint8)
    off = mix["al"].batch.seq_off.astype(np.int64)
    got, lo, chunks = [], 0, 0
    with sam.BamStream(str(mix["path"]), chunk_bytes=20_000, keep_raw=True) as stream:
        for chunk in stream:
            n = chunk.batch.n
            patched = stream.patch_rescaled(chunk, mix["qual_out"][off[lo]:off[lo + n]], round_mr(mix["mr"][lo:lo + n]), rescaled[lo:lo + n])
            got.append(bytes(patched))
            lo += n
            chunks += 1
    assert lo == len(want) and chunks > 5
    assert b"".join(got) == F.stream_of(want)
    assert sum(len(w) for w in want) == sum(len(b) for b in mix["bodies"]) + 7 * int(rescaled.sum())


def test_rule_against_the_reference_golden(tmp_path):
    """The records of tests/golden/genome_rescale.npz as a file: the rule over the oracle's outputs holds the qualities the
    reference wrote, and its MR as float32."""
    from oracle import oracle
    from tests.test_rescale import corr_table, load
    ref, batch, model, corr_prob, want_qual, want_mr = load(tmp_path)
    sam.write_bam(tmp_path / "in.bam", batch, ref.names, ref.lengths, [], None)
    al = sam.read_bam(tmp_path / "in.bam", keep_raw=True)
    qual_out, mr, status = oracle.rescale(ref, al.batch, corr_table(corr_prob, model), model.len5p, model.len3p)
    out = F.rule(al.raw, al.batch.seq_off, qual_out, mr, status)
    assert isinstance(out, list) and len(out) == batch.n
    off = batch.seq_off.astype(np.int64)
    for i, (body, new) in enumerate(zip(al.raw, out)):
        at, l_seq = F.qual_at(new)
        assert new[at:at + l_seq] == bytes(want_qual[off[i]:off[i + 1]])
        if np.isnan(want_mr[i]):
            assert new == bytes(body)
        else:
            assert len(new) == len(body) + 7 and new[:at] == bytes(body[:at]) and new[at + l_seq:-7] == bytes(body[at + l_seq:])
            assert new[-7:-4] == b"MRf" and struct.unpack("<f", new[-4:])[0] == np.float32(want_mr[i])


def record(tags, name=b"q"):
    return F.encode(name, 0, 0, 10, [("M", 4)], b"ACGT", bytes([30, 31, 32, 33]), tags=tags)


@pytest.mark.parametrize("what,tags,name,has", [
    ("none", b"", b"q", False),
    ("inside a Z string", b"XZZabMRfMRfab\0", b"q", False),
    ("inside a B:C array", F.LOOKALIKE_B, b"q", False),
    ("inside a B:C array, behind other fields", b"NMC\x01" + F.LOOKALIKE_B + b"XQi\x01\x00\x00\x00", b"q", False),
    ("inside the read name", b"NMC\x01", b"MRfMRf", False),
    ("inside an H string", b"XHHMRf0\0", b"q", False),
    ("the value of an i field", b"XIi" + b"MRf\0", b"q", False),
    ("MR:f", b"MRf" + struct.pack("<f", 0.5), b"q", True),
    ("MR:i", b"NMC\x01" + b"MRi" + struct.pack("<i", 3), b"q", True),
    ("MR:Z", b"MRZabc\0" + b"NMC\x01", b"q", True),
    ("MR:B behind a look-alike", F.LOOKALIKE_Z + b"MRBs" + struct.pack("<ihh", 2, 1, 2), b"q", True),
], ids=lambda v: v if isinstance(v, str) else None)
def test_tag_walk(what, tags, name, has):
    body = record(tags, name)
    assert F.walk_tags(body)[-1][3] == len(body) if tags else F.walk_tags(body) == []
    assert F.has_tag(body) is has
    # as the rule sees it: a clash where the record is rescaled, nothing where it is not
    qual = np.frombuffer(bytes([1, 2, 3, 4]), np.uint8)
    for status, want in ((F.SINGLE_END, 0 if has else [body[:F.qual_at(body)[0]] + bytes(qual) + tags + F.mr_tag(0.123456)]),
                         (F.IMPROPER, [body])):
        assert F.rule([body], [0, 4], qual, [0.123456], [status]) == want


def test_tag_walk_refuses_what_it_cannot_follow():
    with pytest.raises(ValueError):
        F.walk_tags(record(b"XQ?abc"))
    with pytest.raises(ValueError):
        F.walk_tags(record(b"XBBC" + struct.pack("<i", 50) + b"abc"))
    with pytest.raises(ValueError):
        F.walk_tags(record(b"XQ"))


def test_mr_tag_is_the_references_expression():
    for x in (0.0, 0.000005, 0.000015, 0.123455, 2.5e-6, 1e-300, 11.999995):
        assert F.mr_tag(x) == b"MRf" + struct.pack("<f", float("%.5f" % x))
        assert struct.unpack("<f", F.mr_tag(x)[3:])[0] == np.float32(float("%.5f" % x))
    assert F.mr_tag(0.0)[3:] == b"\0\0\0\0" and F.mr_tag(1.0)[3:] == b"\x00\x00\x80\x3f"
