"""--tag-group / --tag-pmd-score on the GPU (include/mdx.h ``mdx_gbam_write_kept_tagged``, ``mdx_strata_pmd_keep_scores``,
``mdx_strata_pmd_scores``; csrc/mdx_kept_tags.h): the written records carry their group and their PMD score as tags.

The yardstick is that of tests/test_gpu_write_kept.py — its reader of BGZF members and its split of a stream into records — and a
small tag parser below.  The expected record is built here: the input record with its block_size raised and the tag bytes
appended, the group from the host restatement of the key (the record's reference sequence, or ``P.groups_of`` of its score), the
score from ``P.scores`` narrowed as numpy narrows an int64 to a float32."""

import functools
import struct
import types

import numpy as np
import pytest

from mapdamage_amd import fasta, sam, synth
from tests import pmd_util as P
from tests.test_gpu_strata import genome5
from tests.test_gpu_write_kept import (DEVICE, FILES, KEPT_WAVE_BYTES, LIBS, THRESHOLDS, encode, flags_of, group_rows,
                                       lib_data, lib_stream, members_stream, minimal, open_stream, patterns, plain_bodies,  # noqa: F401
                                       read_bam_file, run, split_stream, strata_engine, tables, with_flag, write_input)

pytestmark = pytest.mark.gpu

PMD_THS = (0.0, 3.0)
NIBBLES = "=ACMGRSVTWYHKDBN"
TAG_SETS = {"group": ("XG", None), "score": (None, "DS"), "both": ("XG", "DS")}
SCALAR_BYTES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


# ---------------------------------------------------------------------- the yardstick's other half: tags, and the expectation
def tags_at(record):
    """Where the tags of a record (with its block_size field) begin."""
    l_name, n_cig, l_seq = record[12], struct.unpack_from("<H", record, 16)[0], struct.unpack_from("<i", record, 20)[0]
    return 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq


def parse_tags(record):
    """[(name, type, value or raw bytes)] of a record's tags; every tag complete, nothing left over."""
    out, at = [], tags_at(record)
    while at < len(record):
        name, ty = record[at:at + 2].decode(), chr(record[at + 2])
        at += 3
        if ty in "ZH":
            end = record.index(b"\0", at)
            out.append((name, ty, record[at:end]))
            at = end + 1
        elif ty == "B":
            size = 5 + SCALAR_BYTES[chr(record[at])] * struct.unpack_from("<I", record, at + 1)[0]
            out.append((name, ty, record[at:at + size]))
            at += size
        else:
            out.append((name, ty, record[at:at + SCALAR_BYTES[ty]]))
            at += SCALAR_BYTES[ty]
    assert at == len(record)
    return out


def score_bits(S):
    """The 32 bits of the score tag: the float32 nearest to the integer S (numpy rounds to nearest, ties to even) times 2^-24."""
    return (np.asarray(S, np.int64).astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)


def tagged(record, group, bits, group_tag, score_tag):
    """The expected record: block_size raised, TAG 'S' u16 and TAG 'f' f32 appended, nothing else touched."""
    extra = b""
    if group_tag is not None:
        extra += group_tag.encode() + b"S" + struct.pack("<H", int(group))
    if score_tag is not None:
        extra += score_tag.encode() + b"f" + struct.pack("<I", int(bits))
    return struct.pack("<i", len(record) - 4 + len(extra)) + record[4:] + extra


def batch_of(bodies):
    """The columns ``P.scores`` reads, from the bytes of BAM records (without block_size)."""
    flag, tid, pos, cigar_off, cigar, seq_off, seq, qual = [], [], [], [0], [], [0], [], []
    for b in bodies:
        t, p, l_name, _, _, n_cig, fl, l_seq = struct.unpack_from("<iiBBHHHi", b, 0)
        at = 32 + l_name
        cigar += [(w >> 4) << 4 | (w & 15) for w in struct.unpack_from("<%dI" % n_cig, b, at)]
        at += 4 * n_cig
        nib = np.frombuffer(b, np.uint8, (l_seq + 1) // 2, at)
        codes = np.stack([nib >> 4, nib & 15], axis=1).reshape(-1)[:l_seq]
        seq.append(np.frombuffer(NIBBLES.encode(), np.uint8)[codes])
        qual.append(np.frombuffer(b, np.uint8, l_seq, at + (l_seq + 1) // 2))
        flag.append(fl), tid.append(t), pos.append(p), cigar_off.append(len(cigar)), seq_off.append(seq_off[-1] + l_seq)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint8)       # noqa: E731
    return types.SimpleNamespace(n=len(bodies), flag=np.asarray(flag, np.uint16), tid=np.asarray(tid, np.int32), pos=np.asarray(pos, np.int32),
                                 cigar_off=np.asarray(cigar_off, np.uint32), cigar=np.asarray(cigar, np.uint32),
                                 seq_off=np.asarray(seq_off, np.uint32), seq=cat(seq), qual=cat(qual))


@functools.lru_cache(maxsize=None)
def big_genome():
    """The two sequences RAW_HEADER names, at their lengths."""
    return synth.make_genome(seed=5, sizes=(("chr1", 1_000_000), ("chr2", 500_000)))


def scores_of(bodies):
    """int64 S of every record: the restatement over the test's own decode of the records."""
    return P.scores(big_genome(), batch_of(bodies))


@functools.lru_cache(maxsize=None)
def plain_scores():
    """S of ``plain_bodies(False)`` under the strand bits ``flags_of`` gives them (the drop bits say nothing to the score)."""
    plain = plain_bodies(False)
    flag = flags_of(np.ones(len(plain), bool))
    return scores_of([with_flag(b, int(f)) for b, f in zip(plain, flag)])


@pytest.fixture(scope="module")
def engines():
    """name -> (engine over ``big_genome()``, its groups): two groups of reference sequences; PMD strata that keep their scores."""
    from mapdamage_amd import pmd
    from mapdamage_amd.engine import DamageEngine
    ref = DamageEngine([("s", "l")], groups=["one", "two"])
    ref.set_strata([0, 1])
    ref.set_reference(big_genome())
    scored = DamageEngine([("s", "l")], groups=pmd.group_names(PMD_THS))
    scored.set_strata_pmd(PMD_THS, keep_scores=True)
    scored.set_reference(big_genome())
    try:
        yield {"group": (ref, 2), "score": (scored, 3), "both": (scored, 3)}
    finally:
        scored.close()
        ref.close()


def groups_for(which, bodies, S):
    """The group of every record as the engine of ``engines()[which]`` keys it."""
    if which == "group":
        return np.asarray([struct.unpack_from("<i", b, 0)[0] for b in bodies], np.int64)
    return P.groups_of(np.asarray(S, np.int64), PMD_THS)


def tagged_file(engines, which, path, chunk_bytes=256 << 20, groups=None, uncountable=False):
    """Every slab's tagged ``write_kept`` through the engine of ``which``: (inflated streams per slab, records, raw bytes).
    ``uncountable``: the file holds the encoder's records without a base, which the tabulation reports when they are kept (at
    ``sync``: MDX_ERR_BAD_READ) — its own report, made behind the key kernel the writer reads from; it says nothing about
    the written records, which are compared all the same."""
    from mapdamage_amd.engine import BadReadError
    eng, n_groups = engines[which]
    group_tag, score_tag = TAG_SETS[which]
    kw = dict(want_qual=True, packed=True) if which != "group" else {}
    streams, n_written, raw = [], 0, 0
    with open_stream(eng, path, chunk_bytes, **kw) as stream:
        while True:
            view = stream.next_view()
            if view is None:
                break
            eng.tabulate_view(view)
            bound = stream.kept_bound(group_tag, score_tag)
            members, n, r = stream.write_kept(view, groups, n_groups, group_tag, score_tag)
            assert len(members) <= bound
            streams.append(members_stream(members))
            assert len(streams[-1]) == r and (n == 0) == (len(members) == 0)
            assert len(split_stream(streams[-1])) == n
            n_written += n
            raw += r
        try:
            eng.sync()
        except BadReadError:
            if not uncountable:
                raise
        finally:
            eng.reset()
    return streams, n_written, raw


def check_tagged(engines, which, path, bodies, keep, S, chunk_bytes=256 << 20, uncountable=False):
    group_tag, score_tag = TAG_SETS[which]
    group, bits = groups_for(which, bodies, S), score_bits(S)
    want = [tagged(struct.pack("<i", len(b)) + b, g, f, group_tag, score_tag) for b, k, g, f in zip(bodies, keep, group, bits) if k]
    streams, n_written, raw = tagged_file(engines, which, path, chunk_bytes, uncountable=uncountable)
    got = b"".join(streams)
    assert n_written == len(want) and raw == sum(len(w) for w in want)
    assert split_stream(got) == want
    assert got == b"".join(want)
    return streams, want


# ---------------------------------------------------------------------- 1. the score column
def check_scores(eng, b, S):
    got = eng.pmd_scores()
    assert got.dtype == np.float32 and got.shape == (b.n,)
    np.testing.assert_array_equal(got.view(np.uint32), score_bits(S))


@pytest.mark.parametrize("no_lds", [False, True])
def test_score_column(monkeypatch, no_lds):
    from tests.test_gpu_pmd import pmd_engine
    from tests.test_gpu_strata import libraries
    if no_lds:
        monkeypatch.setenv("MDX_PMD_NO_LDS", "1")
    ref = genome5()
    hand, many = P.hand_batch(ref, "dropped"), P.synthetic_batch(ref, 4099, 61, 3)
    assert many.n == 16 * 256 + 3
    S_hand, S_many = P.scores(ref, hand), P.scores(ref, many)
    assert (S_hand == 0).any() and (S_hand > 0).any() and (S_many < 0).any() and len(set(score_bits(S_many).tolist())) > 2000
    with pmd_engine(libraries(3), PMD_THS) as eng:
        eng.set_reference(ref)
        eng.keep_pmd_scores(True)
        for packed in (True, False):
            eng.tabulate(hand, packed=packed)
            check_scores(eng, hand, S_hand)
            eng.tabulate(many, packed=packed)
            check_scores(eng, many, S_many)
        with_switch = (eng.strata_kept(), eng.pmd_histogram(), eng.finish())
    with pmd_engine(libraries(3), PMD_THS) as eng:
        eng.set_reference(ref)
        for packed in (True, False):
            eng.tabulate(hand, packed=packed)
            eng.tabulate(many, packed=packed)
        plain = (eng.strata_kept(), eng.pmd_histogram(), eng.finish())
    # the switch changes nothing that was there: kept reads per stratum, the histogram, the tables
    np.testing.assert_array_equal(with_switch[0], plain[0])
    np.testing.assert_array_equal(with_switch[1], plain[1])
    for name in ("mis", "comp", "lgd"):
        np.testing.assert_array_equal(getattr(with_switch[2].merged, name), getattr(plain[2].merged, name))
        for g in range(len(PMD_THS) + 1):
            np.testing.assert_array_equal(getattr(with_switch[2].group(g), name), getattr(plain[2].group(g), name))


def test_score_column_state_errors():
    from mapdamage_amd.engine import DamageEngine, MdxError
    from tests.test_gpu_pmd import pmd_engine
    from tests.test_gpu_strata import libraries
    ref = genome5()
    b = P.synthetic_batch(ref, 300, 62, 3)
    with pmd_engine(libraries(3), PMD_THS) as eng:
        eng.set_reference(ref)
        eng.tabulate(b, packed=True)
        with pytest.raises(MdxError, match="not kept") as err:                    # without the switch
            eng.pmd_scores()
        assert err.value.code == -3
        eng.keep_pmd_scores(True)
        with pytest.raises(MdxError, match="not keyed") as err:                   # nothing keyed since the switch
            eng.pmd_scores()
        assert err.value.code == -3
        eng.tabulate(b, packed=True)
        check_scores(eng, b, P.scores(ref, b))
        with pytest.raises(MdxError) as err:                                      # another number of records
            eng.pmd_scores(b.n - 1)
        assert err.value.code == -1
        db = eng.upload(b, packed=True)                                           # a resident batch brings its buckets
        eng.tabulate(db)
        eng.sync()
        with pytest.raises(MdxError, match="not keyed") as err:
            eng.pmd_scores()
        assert err.value.code == -3
        eng.tabulate(b, packed=True)
        check_scores(eng, b, P.scores(ref, b))
        eng.keep_pmd_scores(False)
        with pytest.raises(MdxError, match="not kept"):
            eng.pmd_scores()
        db.free()
    with DamageEngine(libraries(3), groups=["x", "y"]) as eng:                        # no PMD strata
        eng.set_strata([0, 1, 0, 1, 0])
        with pytest.raises(MdxError, match="no PMD strata") as err:
            eng.keep_pmd_scores(True)
        assert err.value.code == -3
        with pytest.raises(MdxError, match="no PMD strata") as err:
            eng.pmd_scores(0)
        assert err.value.code == -3


# ---------------------------------------------------------------------- 2. alignments and size classes
@pytest.mark.parametrize("which", sorted(TAG_SETS))
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 4097])
def test_alignments_and_size_classes(engines, tmp_path, n, which):
    plain = plain_bodies(False)[:n]
    assert n < 1024 or {(len(b) + 4) % 16 for b in plain} == set(range(16))
    S = plain_scores()[:n]
    for name, keep in patterns(n).items():
        bodies = [with_flag(b, int(f)) for b, f in zip(plain, flags_of(keep))]
        path = tmp_path / ("%s.bam" % name.replace(" ", "_"))
        write_input(path, bodies, "raw")
        _, want = check_tagged(engines, which, path, bodies, keep, S, uncountable=True)
        if which == "both" and name == "all" and n >= 1024:
            # 12 more bytes per record shift every destination: each of them lands on every residue
            starts = np.cumsum([0] + [len(w) for w in want[:-1]])
            assert set((starts % 16).tolist()) == set(range(16)) and {len(w) % 16 for w in want} == set(range(16))


# ---------------------------------------------------------------------- 3. the threshold between eight lanes and a wavefront
def sized(k, size):
    """Record ``k`` of ``size`` bytes with its block_size field: a few bases, the rest a Z tag."""
    base = len(encode(k, n_bases=30, tag=0, name_len=2)) + 4 + 4
    body = encode(k, n_bases=30, tag=0, name_len=2, z_bytes=size - base)
    assert len(body) + 4 == size
    return body


@pytest.mark.parametrize("which", sorted(TAG_SETS))
def test_records_around_the_wavefront_threshold(engines, tmp_path, which):
    extra = {"group": 5, "score": 7, "both": 12}[which]
    # output sizes below, at and above the threshold; input sizes at and below it whose output lies above it
    sizes = [KEPT_WAVE_BYTES - 1 - extra, KEPT_WAVE_BYTES - extra, KEPT_WAVE_BYTES + 1 - extra, KEPT_WAVE_BYTES, KEPT_WAVE_BYTES - 1,
             KEPT_WAVE_BYTES + 1, 3 * KEPT_WAVE_BYTES + 5]
    plain = []
    for k, size in enumerate(sizes * 3):
        plain += [sized(k, size), minimal(k)]
    assert {37, 38, 39, 40} == {len(b) + 4 for b in plain[1::2]}
    S = scores_of(plain)
    for keep in (np.random.default_rng(9).random(len(plain)) < 0.7, np.ones(len(plain), bool), np.arange(len(plain)) % 2 == 0):
        bodies = [with_flag(b, int(f)) for b, f in zip(plain, flags_of(keep, np.zeros(len(plain))))]
        write_input(tmp_path / "in.bam", bodies, "raw")
        _, want = check_tagged(engines, which, tmp_path / "in.bam", bodies, keep, S, uncountable=True)
    assert {KEPT_WAVE_BYTES - 1, KEPT_WAVE_BYTES, KEPT_WAVE_BYTES + 1, KEPT_WAVE_BYTES + extra} <= {len(w) for w in want}


@pytest.mark.parametrize("where", ["start", "middle", "last"])
def test_a_long_record(engines, tmp_path, where):
    long_body = encode(6, n_bases=50, tag=2, z_bytes=300_000)
    short = [minimal(i) for i in range(41)]
    at = {"start": 0, "middle": 20, "last": 41}[where]
    plain = short[:at] + [long_body] + short[at:]
    S = scores_of(plain)
    for long_kept in (True, False):
        keep = np.arange(len(plain)) % 2 == (at % 2 if long_kept else 1 - at % 2)
        bodies = [with_flag(b, int(f)) for b, f in zip(plain, flags_of(keep, np.zeros(len(plain))))]
        for layout in ("raw", "3001"):
            write_input(tmp_path / (layout + ".bam"), bodies, layout)
            check_tagged(engines, "both", tmp_path / (layout + ".bam"), bodies, keep, S, uncountable=True)


# ---------------------------------------------------------------------- 4. several slabs
@functools.lru_cache(maxsize=None)
def slab_bodies():
    n = 7000
    keep = np.random.default_rng(3).random(n) < 0.6
    keep[1200:3400] = False                 # a stretch of dropped records longer than two slabs
    keep[3400:3500] = True
    bodies = [encode(i, int(f)) for i, f in enumerate(flags_of(keep))]
    return bodies, keep, scores_of(bodies)


@pytest.mark.parametrize("layout", ["raw", "3001"])
def test_several_slabs(engines, tmp_path, layout):
    bodies, keep, S = slab_bodies()
    write_input(tmp_path / "in.bam", bodies, layout)
    streams, _ = check_tagged(engines, "both", tmp_path / "in.bam", bodies, keep, S, chunk_bytes=65536, uncountable=True)
    assert len(streams) >= 12
    assert sum(1 for s in streams if not s) >= 2 and streams[0] and streams[-1]


# ---------------------------------------------------------------------- 5. a selection with tags, every kind of groups
@pytest.fixture(scope="module")
def lib_scores(lib_data):
    return P.scores(lib_data["ref"], lib_data["batch"])


@pytest.mark.parametrize("kind", ["pmd", "regions", "damage", "reference"])
def test_selection_with_tags(lib_data, lib_scores, kind):
    eng, n_groups = strata_engine(kind, lib_data["ref"])
    tag_sets = [("XG", None)] + ([("g1", "s1"), (None, "DS")] if kind == "pmd" else [])
    selections = [(1,), (0, n_groups - 1), None]
    plain = {s: [] for s in selections}
    got = {(s, t): [] for s in selections for t in tag_sets}
    with eng:
        if kind == "pmd":
            eng.keep_pmd_scores(True)
        with lib_stream(eng, lib_data["dir"] / "in.bam", kind) as stream:
            while True:
                view = stream.next_view()
                if view is None:
                    break
                eng.tabulate_view(view)
                for s in selections:
                    ng = n_groups if s is not None else 0
                    plain[s].append(members_stream(stream.write_kept(view, s, ng)[0]))
                    for t in tag_sets:
                        members, n, raw = stream.write_kept(view, s, n_groups, *t)
                        got[s, t].append(members_stream(members))
                        assert raw == len(got[s, t][-1]) and len(members) <= stream.kept_bound(*t)
            eng.sync()
    group, bits = lib_data["groups"][kind], score_bits(lib_scores)
    assert kind != "pmd" or (group == P.groups_of(lib_scores, THRESHOLDS)).all()
    index = {r: i for i, r in enumerate(lib_data["records"])}
    assert len(index) == len(lib_data["records"])
    for s in selections:
        written = split_stream(b"".join(plain[s]))
        keep = lib_data["kept"] & (np.isin(group, s) if s is not None else True)
        assert written == [r for r, k in zip(lib_data["records"], keep) if k] and len(written) > 50
        for t in tag_sets:
            # the written set is the untagged call's, each record the same record and its tags
            assert split_stream(b"".join(got[s, t])) == [tagged(r, group[index[r]], bits[index[r]], *t) for r in written], (s, t)


# ---------------------------------------------------------------------- 6. a record that has the tag already
def with_tag(i, name, flag=0):
    """Record ``i`` with an RG:Z tag and a five-byte tag of that name: every record of the clash files is as long as its twin."""
    return encode(i, flag, n_bases=20 + i % 60, tag=1) + name + b"S" + struct.pack("<H", i % 7)


def slab_sizes(engines, path, chunk_bytes):
    eng = engines["group"][0]
    sizes = []
    with open_stream(eng, path, chunk_bytes) as stream:
        while True:
            view = stream.next_view()
            if view is None:
                return sizes
            sizes.append(int(view.n_reads))


def test_clash(engines, tmp_path):
    n = 3000
    bodies = [with_tag(i, b"XH") for i in range(n)]
    write_input(tmp_path / "clean.bam", bodies, "raw")
    sizes = slab_sizes(engines, tmp_path / "clean.bam", 65536)
    assert len(sizes) >= 4 and sum(sizes) == n and min(sizes[:3]) > 8
    keep = np.ones(n, bool)
    S = scores_of(bodies)
    check_tagged(engines, "both", tmp_path / "clean.bam", bodies, keep, S, chunk_bytes=65536)
    # the second record of the first slab, the last record of a slab, a record of a later slab
    places = {"second": (0, 1), "last of a slab": (1, sizes[1] - 1), "a later slab": (2, 5)}
    for what, (slab, at) in places.items():
        i = sum(sizes[:slab]) + at
        for which, name in (("group", b"XG"), ("score", b"DS"), ("both", b"DS")):
            clashing = list(bodies)
            clashing[i] = with_tag(i, name)
            # (a later record with the name too: the lowest index of the slab is the one reported)
            later = min(i + 3, sum(sizes[:slab + 1]) - 1)
            clashing[later] = with_tag(later, name)
            assert len(clashing[i]) == len(bodies[i])
            write_input(tmp_path / "clash.bam", clashing, "raw")
            assert slab_sizes(engines, tmp_path / "clash.bam", 65536) == sizes
            with pytest.raises(sam.KeptTagClash) as err:
                tagged_file(engines, which, tmp_path / "clash.bam", 65536)
            assert err.value.code == -6 and err.value.index == at, (what, which)
            name_len = clashing[i][8]
            assert err.value.name == clashing[i][32:32 + name_len - 1].decode() and err.value.name in str(err.value), (what, which)
        # the same records with those two dropped by a flag: written without error, the other records tagged
        dropped = list(clashing)
        for j in (i, later):
            dropped[j] = with_flag(clashing[j], 0x400)
        keep_but = keep.copy()
        keep_but[[i, later]] = False
        write_input(tmp_path / "dropped.bam", dropped, "raw")
        check_tagged(engines, "both", tmp_path / "dropped.bam", dropped, keep_but, S, chunk_bytes=65536)
    # the other tag's name is no clash for a call that adds one tag only
    check_tagged(engines, "group", tmp_path / "clash.bam", clashing, keep, S, chunk_bytes=65536)


def test_a_tag_region_the_walk_cannot_follow(engines, tmp_path):
    """An unknown type, and a B array that runs past the record's end, in front of the sought name: no clash, the record is
    written with its bytes as they are and the new tags behind them."""
    bodies = [with_tag(i, b"XH") for i in range(40)]
    bodies[3] = encode(3, n_bases=25, tag=1) + b"QQq\1\2\3\4" + b"XGS\0\0"
    bodies[17] = encode(17, n_bases=25, tag=1) + b"ZBBi" + struct.pack("<I", 1000) + b"XGS\0\0DSf\0\0\0\0"
    bodies[39] = encode(39, n_bases=25, tag=0) + b"XA"
    write_input(tmp_path / "in.bam", bodies, "raw")
    check_tagged(engines, "both", tmp_path / "in.bam", bodies, np.ones(40, bool), scores_of(bodies))


# ---------------------------------------------------------------------- 7. state errors
def test_state_errors(lib_data):
    from mapdamage_amd.engine import MdxError
    eng, n_groups = strata_engine("pmd", lib_data["ref"])
    with eng:
        with lib_stream(eng, lib_data["dir"] / "in.bam", "pmd") as stream:
            view = stream.next_view()
            with pytest.raises(MdxError, match="tabulate the view first") as err:          # before the view is tabulated
                stream.write_kept(view, None, n_groups, "XG")
            assert err.value.code == -3
            eng.tabulate_view(view)
            with pytest.raises(MdxError, match="n_groups 5, the context has 4") as err:     # a wrong n_groups
                stream.write_kept(view, None, n_groups + 1, "XG")
            assert err.value.code == -1
            with pytest.raises(MdxError, match="no score column") as err:                  # a score tag without the switch
                stream.write_kept(view, None, n_groups, "XG", "DS")
            assert err.value.code == -3
            with pytest.raises(MdxError, match="same name") as err:
                stream.write_kept(view, None, n_groups, "XG", "XG")
            assert err.value.code == -1
            with pytest.raises(MdxError, match="two characters") as err:
                stream.write_kept(view, None, n_groups, "X_")
            assert err.value.code == -1
            assert stream.write_kept(view, None, n_groups, "XG")[1] > 0
            eng.keep_pmd_scores(True)
            with pytest.raises(MdxError, match="no score column") as err:                  # the switch came behind the view's launch
                stream.write_kept(view, None, n_groups, None, "DS")
            assert err.value.code == -3
            view = stream.next_view()
            eng.tabulate_view(view)
            first = stream.write_kept(view, None, n_groups, "XG", "DS")
            assert first[1] > 0
            eng.tabulate(lib_data["batch"].slice(0, 100))                                  # another batch tabulated in between
            eng.sync()
            for tags in (("XG", None), (None, "DS")):
                with pytest.raises(MdxError, match="not that of this view") as err:
                    stream.write_kept(view, None, n_groups, *tags)
                assert err.value.code == -3
            view = stream.next_view()                                                      # the next view, not tabulated yet
            with pytest.raises(MdxError) as err:
                stream.write_kept(view, None, n_groups, "XG")
            assert err.value.code == -3
            assert stream.write_kept(view)[1] > 0                                          # (no tag, no selection: no key needed)
            eng.tabulate_view(view)
            assert stream.write_kept(view, (0,), n_groups, "XG", "DS")[1] > 0
            eng.sync()
    from mapdamage_amd.engine import DamageEngine
    with DamageEngine(LIBS) as plain:                                                     # tags on an unstratified context
        plain.set_reference(lib_data["ref"])
        with lib_stream(plain, lib_data["dir"] / "in.bam", "reference") as stream:
            view = stream.next_view()
            plain.tabulate_view(view)
            with pytest.raises(MdxError, match="without strata") as err:
                stream.write_kept(view, None, 3, "XG")
            assert err.value.code == -1
            plain.sync()


# ---------------------------------------------------------------------- 8. the command line
CLI = {
    "pmd": (["--by-pmd-score", "--pmd-thresholds", "0,3"], ["--tag-group", "XG", "--tag-pmd-score", "DS"], "XG:S group, DS:f PMD score"),
    "regions": (["--regions", "panels.bed", "--write-groups", "0"], ["--tag-group", "XG"], "XG:S group"),
    "damage": (["--by-terminal-damage", "--min-mapq", "25", "-n", "0.5", "--downsample-seed", "7"], ["--tag-group", "DG"], "DG:S group"),
}


def tree(folder):
    """Every file of the by_* directories, by its path below the folder."""
    return {str(p.relative_to(folder)): p.read_bytes() for d in sorted(folder.glob("by_*")) for p in sorted(d.rglob("*")) if p.is_file()}


@pytest.fixture(scope="module")
def untagged_runs(lib_data, tmp_path_factory):
    """The same commands with --write-kept and without the tag options, once each: (folder, the records written)."""
    done = {}

    def get(case):
        if case not in done:
            d = tmp_path_factory.mktemp("untagged_" + case)
            opts = [lib_data["dir"] / a if a == "panels.bed" else a for a in CLI[case][0]]
            out = run(lib_data, d / "out", "in.bam", *opts, "--write-kept", d / "kept.bam")
            done[case] = (out, read_bam_file(d / "kept.bam")[1])
        return done[case]
    return get


@pytest.mark.parametrize("route", ["file", "pipe"])
@pytest.mark.parametrize("case", sorted(CLI))
def test_command_line(lib_data, lib_scores, untagged_runs, tmp_path, case, route):
    opts = [lib_data["dir"] / a if a == "panels.bed" else a for a in CLI[case][0]]
    kept_path = tmp_path / "kept.bam"
    out = run(lib_data, tmp_path / "out", "in.bam", *opts, "--write-kept", kept_path, *CLI[case][1], route=route)
    log = (out / "Runtime_log.txt").read_text()
    assert DEVICE in log and "gave up" not in log
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == ["kept.bam"]
    plain_out, plain_records = untagged_runs(case)
    # the tables, the by_* tree and the filters' report are those of the run without the tag options
    assert tables(out) == tables(plain_out) and tree(out) == tree(plain_out) and len(tree(out)) > 4
    for name in ("record_filters.tsv",):
        assert (out / name).exists() == (plain_out / name).exists() and (not (out / name).exists() or (out / name).read_bytes() == (plain_out / name).read_bytes())
    header, records = read_bam_file(kept_path)
    assert header == lib_data["header"] and len(records) == len(plain_records) > 50
    group_tag = CLI[case][1][1]
    score_tag = "DS" if case == "pmd" else None
    extra = 5 + (7 if score_tag else 0)
    groups = []
    for got, plain in zip(records, plain_records):
        # the plain run's record, block_size raised, the tags behind its own
        assert got[4:len(plain)] == plain[4:] and struct.unpack_from("<i", got)[0] == len(plain) - 4 + extra and len(got) == len(plain) + extra
        new = parse_tags(got)[len(parse_tags(plain)):]
        assert [(t[0], t[1]) for t in new] == [(group_tag, "S")] + ([(score_tag, "f")] if score_tag else [])
        groups.append(struct.unpack("<H", new[0][2])[0])
    # per group, the records that carry its index are those groups.tsv counts
    by_dir = next(out.glob("by_*"))
    rows = group_rows(by_dir / "groups.tsv")
    counts = np.bincount(groups, minlength=len(rows))
    which = opts[opts.index("--write-groups") + 1] if "--write-groups" in opts else "all"
    for name, (index, reads) in rows.items():
        assert counts[index] == (reads if which == "all" or int(which) == index else 0), name
    if case == "pmd":
        # ... and exactly the records, from the restatement of the score
        keep = lib_data["kept"]
        want = [tagged(r, g, f, "XG", "DS") for r, k, g, f in zip(lib_data["records"], keep, P.groups_of(lib_scores, PMD_THS), score_bits(lib_scores)) if k]
        assert records == want
    assert "Wrote %d records to %s (groups: %s); tags: %s" % (len(records), kept_path, which, CLI[case][2]) in log
    assert (out / "write_kept.tsv").read_text() == "path\tgroups\trecords\tuncompressed_bytes\n%s\t%s\t%d\t%d\n" % (
        kept_path, which, len(records), sum(len(r) for r in records))
    plain_log = (plain_out / "Runtime_log.txt").read_text()
    assert "; tags:" not in plain_log and "Wrote %d records to" % len(records) in plain_log


@pytest.mark.parametrize("route", ["file", "pipe"])
def test_command_line_clash(lib_data, tmp_path, route):
    """A record of the input has an XG tag already: exit code 1, the record's name, neither the file nor its temporary twin."""
    bodies = [with_tag(i, b"XH") for i in range(600)]
    bodies[333] = with_tag(333, b"XG")
    d = tmp_path / "in"
    d.mkdir()
    write_input(d / "clash.bam", bodies, "raw")
    fasta.write_fasta(d / "big.fa", big_genome())
    args = ["-r", str(d / "big.fa"), "--by-reference", "--write-kept", tmp_path / "kept.bam", "--tag-group", "XG"]
    out = run(lib_data, tmp_path / "out", d / "clash.bam", *args, route=route, rc=1)
    log = (out / "Runtime_log.txt").read_text()
    name = bodies[333][32:32 + bodies[333][8] - 1].decode()
    assert "Read: %s already has a tag named XG" % name in log and "gave up" not in log
    assert sorted(p.name for p in tmp_path.iterdir() if p.is_file()) == []
    assert not any((out / f).exists() for f in FILES + ("write_kept.tsv",))
    # with another name the same file is written
    args[-1] = "XI"
    out = run(lib_data, tmp_path / "fine", d / "clash.bam", *args, route=route)
    assert len(read_bam_file(tmp_path / "kept.bam")[1]) == 600
