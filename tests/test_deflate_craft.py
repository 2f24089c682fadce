"""The hand-built DEFLATE streams of tests/deflate_craft.py, without a GPU: the builder is right (zlib inflates every
valid stream to the bytes the builder says and refuses every stream built to be refused), the corpus holds what it is
meant to hold (asserted on the builder's own counts), and the host build of mapdamage_amd/csrc/mdx_inflate.h decodes
all of it exactly as zlib does — accept / refuse included — once more under AddressSanitizer and UBSan, as the stand-alone
program tests/native/inflate_check.cpp.  The device build: tests/test_gpu_inflate_craft.py."""
import pathlib
import struct
import subprocess
import zlib

import pytest

from tests import deflate_craft as dc

ROOT = pathlib.Path(__file__).resolve().parent.parent
CORPORA = list(dc.THEMES) + ["random-%d" % s for s in dc.RANDOM_SEEDS]


def corpus(name):
    return dc.THEMES[name]() if name in dc.THEMES else dc.random_corpus(int(name.split("-")[1]))


def zlib_says(comp):
    """the bytes of a complete raw stream of at most 65536 bytes out, None for anything else"""
    try:
        z = zlib.decompressobj(-15)
        out = z.decompress(comp, dc.CAP + 1)
        if z.eof and len(out) <= dc.CAP:
            return out
    except zlib.error:
        pass
    return None


@pytest.mark.parametrize("name", CORPORA)
def test_zlib_reads_what_the_builder_says(name):
    n_valid = n_refused = 0
    for c in corpus(name):
        z = zlib_says(c.stream)
        if c.expected is not None:
            assert z == c.expected, c
            n_valid += 1
        elif c.theme != "random":
            assert z is None, c                          # built to be refused
            n_refused += 1
    assert n_valid and (n_refused > 200 if name == "invalid" else True)


def test_directed_cases_hold_what_they_are_for():
    directed = [c for name in dc.THEMES for c in dc.THEMES[name]()]
    st, pairs = dc.totals(directed)
    valid_st, _ = dc.totals([c for c in directed if c.expected is not None])
    labels = {c.label for c in directed}
    need = ["blk_lit_le2", "blk_lit_all11", "blk_lit_15", "blk_lit_both_sides_of_fast_table", "eob_code_1", "eob_code_15",
            "no_distance_code", "single_distance_code_len1", "dist_code_15", "alt258",
            "m_straddles_seg", "far_behind_stored", "far_behind_far", "far_source_of_same_block",
            "hlit_286", "hdist_30", "hclen_5", "hclen_19", "hlit_above_min", "hdist_above_min", "hclen_above_min",
            "rep16_crosses_into_distances", "rep18_138", "rep16_after_1718", "header_no_repeat",
            "empty_dynamic_between", "empty_fixed_between", "empty_stored_between", "pad_all_ones", "ends_on_byte",
            "blocks_1", "blocks_2", "blocks_3", "blocks_6", "mixed_kinds", "stored_len_words_straddle_512"]
    need += ["run%d_%s" % (n, f) for n in range(1, 10) for f in ("longlit", "eob", "shortlen", "longlen")]
    need += ["run%d_longlit" % p for p in range(7)]                      # a slow literal at every position of a fast run
    need += ["run%d_longest_pair_behind_code_%d" % (n, ln) for n in range(10) for ln in (9, 10, 11, 13)]
    need += ["L%d_%s" % (i, e) for i in range(29) for e in ("min", "max")] + ["D%d_%s" % (i, e) for i in range(30) for e in ("min", "max")]
    need += ["x%d_%s" % (at, w) for at in (512, 1024) for w in ("hdr_fields", "cl_lens", "code_lens", "tokens")]
    missing = [k for k in need if not valid_st[k]]
    assert not missing, missing
    # (HCLEN 4 codes 16, 17, 18 and 0 alone — every length zero, no end-of-block code: no valid block has it, a refused one does)
    assert st["hclen_4"] and not valid_st["hclen_4"]
    want = {(ln, d) for ln in dc.MATCH_LENS for d in dc.directed_distances(ln) + list(dc.FAR)}
    assert not want - pairs, sorted(want - pairs)[:10]
    assert {4095, 4096, 4097} <= set(dc.BAND) and min(dc.BAND) == 4096 - 258 and max(dc.BAND) == 4096 + 258
    for k in range(490, 531):
        assert "dynamic block behind %d stored bytes" % k in labels and "dynamic block behind %d stored bytes" % (512 + k) in labels
    # the 11 / 12-bit block really is one: both lengths, nothing else, in one block
    (c,) = [c for c in directed if c.label == "literals of 11 and 12 bits in turn"]
    assert c.stats["blk_lit_both_sides_of_fast_table"] == 2 and c.stats["blk_lit_ge12"] == 2 and not c.stats["blk_lit_15"]
    # the output bound: 65536 bytes, and one more
    full = [c for c in directed if c.expected is not None and len(c.expected) == dc.CAP]
    over = [c for c in directed if c.label.endswith("and one literal")]
    assert len(full) == 1 and len(over) == 1 and (258, 4500) in full[0].pairs
    z = zlib.decompressobj(-15)
    assert len(z.decompress(over[0].stream)) == dc.CAP + 1 and z.eof
    # the prefixes: every proper one of a three-block stream of about 200 bytes
    (whole,) = [c for c in directed if c.label == "the stream the prefixes are of"]
    assert whole.stats["blocks_3"] and 150 <= len(whole.stream) <= 250
    assert {c.stream for c in directed if c.label.startswith("prefix of")} == {whole.stream[:n] for n in range(len(whole.stream))}


@pytest.mark.parametrize("seed", dc.RANDOM_SEEDS)
def test_random_corpus_holds_what_it_is_for(seed):
    cases = dc.random_corpus(seed)
    st, _ = dc.totals(cases)
    assert st["blk_lit_ge12"] >= 50 and st["blk_lit_le2"] >= 50, st
    assert st["m_far"] >= 200 and st["m_band"] >= 200 and st["m_short_period_long"] >= 200 and st["m_overlap_64"] >= 100, st
    twins = [zlib_says(c.stream) is not None for c in cases if c.expected is None]
    assert len(twins) == len(cases) // 2
    assert 6 * sum(twins) >= len(twins) and 6 * (len(twins) - sum(twins)) >= len(twins), (sum(twins), len(twins))
    out = sum(len(c.expected) for c in cases if c.expected is not None)
    assert out < 3_000_000 and sum(1 for c in cases if c.expected is not None and 5000 <= len(c.expected) <= 9300) > len(twins) * 0.8


def _records():
    blob, n = bytearray(), 0
    for name in CORPORA:
        for c in corpus(name):
            if c.expected is not None:
                blob += struct.pack("<II", len(c.stream), len(c.expected)) + c.stream + c.expected
            else:
                blob += struct.pack("<II", len(c.stream), 0xFFFFFFFF) + c.stream       # zlib's verdict, zlib's bytes
            n += 1
    return bytes(blob), n


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "asan-ubsan"])
def test_host_build_decodes_the_corpus_as_zlib_does(tmp_path, flags):
    exe = tmp_path / "inflate_check"
    subprocess.check_call(["g++", *flags, "-I", str(ROOT / "mapdamage_amd" / "csrc"), str(ROOT / "tests" / "native" / "inflate_check.cpp"),
                           "-lz", "-o", str(exe)])
    blob, n = _records()
    out = subprocess.run([str(exe)], input=blob, capture_output=True, timeout=120)
    assert out.returncode == 0, (out.stdout.decode()[-2000:], out.stderr.decode()[-3000:])
    assert out.stdout.decode().strip().endswith("%d streams, 0 bad" % n)
    assert b"Sanitizer" not in out.stderr and b"runtime error" not in out.stderr, out.stderr.decode()[-3000:]
