"""The tabulation kernels' many-tiles-per-wavefront machinery at small batches: MDX_TEST_CUS (include/mdx.h,
mdx_last_launch_geometry) sizes a context's launches as on a device of 2-8 compute units, so that every wavefront of a batch of
~100 000 records takes dozens of tiles — several rounds of MDX_ROUND_TILES tiles, rings (MDX_LIST_RING entries, MDX_DRING records
handed over) that wrap, more than 255 steps between two folds of the packed kernels' bit-sliced planes, tiles of other pools,
fewer pools than libraries.  On the whole device a wavefront gets its second tile only beyond 258 000 records.

Every case asserts, from the launch's geometry and the constants of csrc/mdx_internal.h alone, the condition it exists for, then
compares the whole table set bit for bit with the C oracle."""

import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from mapdamage_amd import synth
from mapdamage_amd.batch import concat_batches
from tests.util import assert_tables_equal, oracle_tableset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# csrc/mdx_internal.h
LIST_RING, ROUND_TILES, DRING, POOL_CHUNK, TILE_MAX = 1024, 14, 128, 24, 64
# wavefronts per compute unit of a full grid at --length 70 --around 10 (csrc/mdx_kernels.hip): the packed and the fused kernels one
# block of 1024 threads, the ASCII kernels two of 768
WAVES_PK, WAVES_ASCII = 16, 24
L, A = 70, 10


def records_for(tiles_per_wave, cus, waves_per_cu):
    """The smallest batch that gives every wavefront of a full grid ``tiles_per_wave`` tiles on average, a tile taken at its
    largest (64 records; 63 where the columns are prefetched)."""
    n = tiles_per_wave * cus * waves_per_cu * TILE_MAX
    assert n <= 150_000, n
    return n


@functools.lru_cache(maxsize=None)
def genome():
    return synth.make_genome(seed=11, sizes=(("chr1", 300_000), ("chr2", 100_000), ("chrS", 500)), n_run=500, lower_run=3000)


def libraries(nlib):
    return [("S%d" % i, "L%d" % i) for i in range(nlib)]


def few_low_qualities(batch, seed, frac=0.05):
    rng = np.random.default_rng(seed)
    nb = batch.seq.shape[0]
    batch.qual = np.where(rng.random(nb) < frac, rng.integers(2, 20, nb), rng.integers(20, 42, nb)).astype(np.uint8)
    return batch


MIXED = dict(len_range=(20, 130), frac_softclip=0.15, frac_ins=0.08, frac_del=0.08, frac_skip=0.02, frac_hardclip=0.005,
             frac_filtered=0.02, frac_n_base=0.02)


@functools.lru_cache(maxsize=None)
def mixed_batch(n, nlib, seed=51):
    """Soft clips, single indels, N operations, partial reads of 20-69 bases, complete ones, both strands; 5 % of the qualities
    below Phred 20.  Several libraries: 90 % of the records in library 0 (a launch over several libraries hands a library's tiles
    to its own pools only: the large one is the one whose wavefronts take many)."""
    batch = few_low_qualities(synth.make_reads(genome(), n, seed + nlib, nlib=nlib, with_qual=True, **MIXED), seed)
    if nlib > 1:
        batch.lib[np.random.default_rng(seed + 7).random(n) < 0.9] = 0
    return batch


@functools.lru_cache(maxsize=None)
def mixed_want(n, nlib, Q, length=L):
    return oracle_tableset(genome(), mixed_batch(n, nlib), libraries(nlib), length, A, Q)


def make_engine(monkeypatch, cus, libs, length=L, Q=0, **kw):
    from mapdamage_amd.engine import DamageEngine
    monkeypatch.setenv("MDX_TEST_CUS", str(cus))
    eng = DamageEngine(libs, length, A, Q, **kw)
    eng.set_reference(genome())
    return eng


def tiles_per_wave(geom):
    return geom["tiles"] / (geom["grid"] * geom["waves_per_block"])


FILTERED = 0xF04        # unmapped, secondary, QC fail, duplicate, supplementary: the records no table counts
TILE_ML = 63            # records of a tile of the packed kernels at --length 70 (the columns are prefetched)


def ml_pools(tiles, n_pools):
    """The pools of a launch over several libraries dealt to its libraries (csrc/mdx_kernels.hip, ml_plan_kernel): the share of
    the pools by tiles rounded down, one at least for a library that has a tile; what is left over one at a time to the library
    with the most tiles per pool (the lowest library on a tie), what is too many back from the one with the fewest."""
    tiles = [int(t) for t in tiles]
    total = sum(tiles)
    m = [max(1, t * n_pools // total) if t else 0 for t in tiles]
    if total == 0:
        m[0] = n_pools
    while sum(m) != n_pools:
        if sum(m) < n_pools:
            load = [np.float32(t) / np.float32(k) if k else np.float32(-1) for t, k in zip(tiles, m)]
            m[int(np.argmax(load))] += 1
        else:
            load = [-np.float32(t) / np.float32(k - 1) if k > 1 else np.float32(-3.0e38) for t, k in zip(tiles, m)]
            m[int(np.argmax(load))] -= 1
    return m


def ml_tiles_per_wave(batch, nlib, geom):
    """Tiles per wavefront, library by library, of a call of the packed kernels over several libraries.  The call is one launch
    per ``pools`` libraries; a launch works on the batch bucketed by library, the filtered records dropped, and a library's tiles go
    to the wavefronts of its own pools.  ``mdx_last_launch_geometry`` reports the tiles of the whole batch: the per-library
    figures are worked out here, from the batch (every launch of these calls has a full grid: the last one's geometry)."""
    kept = np.bincount(batch.lib[(batch.flag & FILTERED) == 0], minlength=nlib)
    tiles = -(-kept // TILE_ML)
    pools = geom["pools"]
    waves_per_pool = geom["grid"] // pools * geom["waves_per_block"]
    out = []
    for lo in range(0, nlib, min(nlib, pools)):
        t = tiles[lo:lo + min(nlib, pools)]
        out += [ti / (mi * waves_per_pool) if mi else 0.0 for ti, mi in zip(t, ml_pools(t, pools))]
    return out


def tabulate(eng, batch, packed, resident):
    if resident:
        dev = eng.upload(batch, packed=packed)
        eng.tabulate(dev)
        eng.sync()
        dev.free()
    else:
        eng.tabulate(batch, packed=packed)
    return eng.last_launch_geometry()


def test_the_knob_only_shrinks_the_grid(monkeypatch):
    """Without MDX_TEST_CUS, or with more compute units than the device has, a launch is the device's own."""
    from mapdamage_amd.engine import DamageEngine
    batch = mixed_batch(records_for(43, 2, WAVES_PK), 1)
    geoms = {}
    for cus in (None, 1 << 20, 2):
        if cus is None:
            monkeypatch.delenv("MDX_TEST_CUS", raising=False)
        else:
            monkeypatch.setenv("MDX_TEST_CUS", str(cus))
        with DamageEngine(libraries(1), L, A, 0) as eng:
            assert eng.last_launch_geometry() == dict(grid=0, waves_per_block=0, tiles=0, pools=0)
            eng.set_reference(genome())
            geoms[cus] = tabulate(eng, batch, True, True)
    assert geoms[None] == geoms[1 << 20]
    assert geoms[2]["grid"] == 2 and geoms[2]["pools"] == 1 and geoms[2]["waves_per_block"] == WAVES_PK
    assert geoms[None]["grid"] > 2 and geoms[None]["tiles"] == geoms[2]["tiles"]


# ---------------------------------------------------------------------------------------------------------------- rounds

@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
@pytest.mark.parametrize("nlib", [1, 3])
@pytest.mark.parametrize("Q", [0, 20])
@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "4bit"])
def test_three_rounds_in_every_kernel(monkeypatch, packed, Q, nlib, resident):
    """Every wavefront takes 42 tiles and more — three rounds — of the mixed batch, on 2 compute units (on 8, three rounds are
    338 000 records): the ASCII kernels (plain, masked; three libraries in one image), the packed kernel, its masked form (one
    library: rings sized by the tile quota), the kernel over several libraries with and without the mask — one launch per library
    on the one pool of 2 compute units, three rounds in the launch of library 0, which holds 90 % of the records."""
    n = records_for(43, 2, WAVES_ASCII)
    batch, want = mixed_batch(n, nlib), mixed_want(n, nlib, Q)
    with make_engine(monkeypatch, 2, libraries(nlib), Q=Q) as eng:
        geom = tabulate(eng, batch, packed, resident)
        # (2 compute units are one pool, and a pool counts one library: three libraries are three launches of the kernel over
        # several libraries, each over its library's stretch of the bucketed batch)
        assert eng.packed_launches() == (-(-nlib // geom["pools"]) if packed else 0)
        if packed and nlib > 1:     # (library 0's launch: 90 % of the records on the one pool's 32 wavefronts)
            assert max(ml_tiles_per_wave(batch, nlib, geom)) >= 3 * ROUND_TILES, (geom, ml_tiles_per_wave(batch, nlib, geom))
        else:                       # (the ASCII kernels count the libraries of one image over all records of the batch)
            assert tiles_per_wave(geom) >= 3 * ROUND_TILES, geom
        got = eng.finish()
    assert_tables_equal(got, want)


@pytest.mark.parametrize("out_form", ["column", "patches"])
@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "4bit"])
def test_fused_launch_with_many_tiles_per_wavefront(monkeypatch, packed, out_form):
    """The fused tabulate + rescale kernels (a block of 1024 threads per compute unit, no rounds: rings and the lists of records left
    to the rescale kernels sized by the tile quota) with 42 tiles and more per wavefront: tables, rescaled qualities, MR sums,
    routing and the summary words against the oracle."""
    from mapdamage_amd.rescale import RescaleModel
    from oracle import oracle
    from tests.test_rescale import corr_table, one_pass, summary_ints_from_oracle
    l5, l3 = 12, 12
    rng = np.random.default_rng(170)
    corr_prob = {}
    for p in list(range(1, l5 + 1)) + list(range(-l3, 0)):
        corr_prob[("C", "T", p)] = float(rng.random() * 0.7)
        corr_prob[("G", "A", p)] = float(rng.random() * 0.7)
    model = RescaleModel(corr_prob, l5, l3)
    n = records_for(43, 2, WAVES_PK)
    b = synth.make_reads(genome(), n, 41, len_range=(25, 160), paired=True, frac_softclip=0.2, frac_ins=0.05, frac_del=0.05,
                         frac_skip=0.01, with_qual=True, frac_filtered=0.03)
    b.mtid = np.where(rng.random(b.n) < 0.9, b.tid, (b.tid + 1) % 2).astype(np.int32)
    b.mpos = (b.pos + rng.integers(-300, 300, size=b.n)).astype(np.int32)
    b.flag = np.where(rng.random(b.n) < 0.4, b.flag & 0xF14, b.flag).astype(np.uint16)      # unpaired: rescaled from both ends
    b.flag = np.where(rng.random(b.n) < 0.05, b.flag | 0x400, b.flag).astype(np.uint16)     # duplicates: rescaled, not counted
    want_tables = oracle_tableset(genome(), b, libraries(1), L, A, 0)
    want_q, want_mr, want_st, want_counts, _ = oracle.rescale_with_subs(genome(), b, corr_table(corr_prob, model), l5, l3)
    patches = out_form == "patches"
    with make_engine(monkeypatch, 2, libraries(1)) as eng:
        eng.set_rescale_model(model)
        q, mr, st = one_pass(eng, b, packed, patches)
        assert eng.fused_launches() == (2 if patches else 1)
        geom = eng.last_launch_geometry()
        assert geom["grid"] == 2 and tiles_per_wave(geom) >= 3 * ROUND_TILES, geom
        words = eng.rescale_summary()
        if patches:         # (the pass ran twice, behind a reset of the tables)
            assert (words % 2 == 0).all()
            words = words // 2
        tables = eng.finish()
    assert_tables_equal(tables, want_tables)
    np.testing.assert_array_equal(q, want_q)
    np.testing.assert_array_equal(st, want_st)
    assert np.array_equal(np.isnan(mr), np.isnan(want_mr))
    np.testing.assert_array_equal(mr[~np.isnan(mr)], want_mr[~np.isnan(want_mr)])
    np.testing.assert_array_equal(words[:756], summary_ints_from_oracle(want_counts))


def test_counters_double_when_a_batch_is_tabulated_twice(monkeypatch):
    """Two multi-round launches into one context: the second finds the tile counters and the rings as the first left them."""
    n = records_for(43, 2, WAVES_PK)
    batch, want = mixed_batch(n, 1), mixed_want(n, 1, 0)
    with make_engine(monkeypatch, 2, libraries(1)) as eng:
        dev = eng.upload(batch, packed=True)
        for _ in range(2):
            eng.tabulate(dev)
            eng.sync()
            assert tiles_per_wave(eng.last_launch_geometry()) >= 3 * ROUND_TILES
        got = eng.finish()
        dev.free()
    np.testing.assert_array_equal(got.mis, 2 * want.mis)
    np.testing.assert_array_equal(got.comp, 2 * want.comp)
    np.testing.assert_array_equal(got.lgd, 2 * want.lgd)
    assert got.n_kept == 2 * want.n_kept


# ------------------------------------------------------------------------------------------------------------- ring wrap

# batches none of whose records is a plain one: every record of a tile is an entry of one of the wavefront's rings, or is handed
# to the general pass.  (make_reads arguments, the share of the records that the fullest list ring takes, how often that ring is
# filled at least, whether every record goes through the hand-over ring.)  The first three are those of
# test_gpu_parity.test_hip_lists_full_in_every_round — their records are split over two or three rings, the fullest wraps once —;
# the next three fill ONE ring each, three times over; the last hands every record to the general pass (a hard clip in front of
# a single indel), which makes entries of both indel rings.
WRAP = {
    "ins+del": (dict(read_len=100, frac_ins=0.5, frac_del=0.5), 0.5, 1, False),
    "clipped": (dict(read_len=100, frac_softclip=1.0, frac_ins=0.3, frac_del=0.3, frac_skip=0.2), 0.0, 0, True),
    "partial+indel": (dict(len_range=(20, 69), frac_ins=0.2, frac_del=0.2), 0.6, 1, False),
    "insertions": (dict(read_len=100, frac_ins=1.0), 1.0, 3, False),
    "deletions": (dict(read_len=100, frac_del=1.0), 1.0, 3, False),
    "partial": (dict(len_range=(20, 69)), 1.0, 3, False),
    "general": (dict(read_len=100, frac_hardclip=1.0, frac_ins=0.5, frac_del=0.5), 0.5, 1, True),
}


@pytest.mark.parametrize("Q", [0, 20])
@pytest.mark.parametrize("kind", sorted(WRAP))
def test_rings_wrap(monkeypatch, kind, Q):
    """A wavefront takes 3 200 records, none of them plain.  The kinds of one ring ("insertions", "deletions", "partial") append
    three times MDX_LIST_RING entries and more to it (63 per tile: 49 tiles); those whose records are split over several rings fill
    the fullest at least once over (WRAP); "general" and "clipped" hand 25 times MDX_DRING records to the general pass.
    -Q 20: the masked kernel, whose rings are sized by its tile quota instead."""
    kw, share, times, handed_over = WRAP[kind]
    n = records_for(50, 2, WAVES_PK)
    batch = few_low_qualities(synth.make_reads(genome(), n, 31, with_qual=True, **kw), 32)
    want = oracle_tableset(genome(), batch, libraries(1), L, A, Q)
    with make_engine(monkeypatch, 2, libraries(1), Q=Q) as eng:
        geom = tabulate(eng, batch, True, True)
        assert eng.packed_launches() == 1
        per_wave = tiles_per_wave(geom) * (batch.n / geom["tiles"])       # records of a wavefront, every one an entry
        assert per_wave * share >= times * LIST_RING, geom
        assert per_wave >= 3 * DRING or not handed_over, geom
        got = eng.finish()
    assert_tables_equal(got, want)


@pytest.mark.parametrize("variant", ["masked", "fused-ascii", "fused-4bit"])
def test_quota_kernels_on_a_batch_of_uneven_cost(monkeypatch, variant):
    """The kernels held to a tile quota — twice a wavefront's even share of its pool's tiles plus two; their rings are sized from
    it, not MDX_LIST_RING — with 40 tiles and more per wavefront on average (a quota of 82 and more: rings of 8192 entries).  Chunks of
    MDX_POOL_CHUNK tiles alternate between all-gapped 150-base reads and records the flag filter drops, so the wavefronts do not
    take the tiles evenly; how far ahead any of them runs is settled while the launch runs and is not asserted."""
    n = records_for(46, 2, WAVES_PK)
    b = few_low_qualities(synth.make_reads(genome(), n, 61, read_len=150, frac_ins=0.5, frac_del=0.5, with_qual=True), 62)
    cheap = (np.arange(n) // (POOL_CHUNK * 63)) % 2 == 1
    b.flag = np.where(cheap, b.flag | 0x400, b.flag).astype(np.uint16)
    Q = 20 if variant == "masked" else 0
    want = oracle_tableset(genome(), b, libraries(1), L, A, Q)
    with make_engine(monkeypatch, 2, libraries(1), Q=Q) as eng:
        if variant == "masked":
            geom = tabulate(eng, b, True, True)
        else:
            from mapdamage_amd.rescale import RescaleModel
            from tests.test_rescale import one_pass
            corr_prob = {(r, s, p): 0.3 for r, s in (("C", "T"), ("G", "A")) for p in list(range(1, 13)) + list(range(-12, 0))}
            eng.set_rescale_model(RescaleModel(corr_prob, 12, 12))
            b.mtid, b.mpos = b.tid.copy(), b.pos.copy()
            one_pass(eng, b, variant == "fused-4bit", False)
            assert eng.fused_launches() == 1
            geom = eng.last_launch_geometry()
        # (a pool of 32 wavefronts; a wavefront's even share is 40 tiles and more, its quota twice that: more than three rounds' worth)
        # (tiles of 63 records in all three kernels at --length 70: the chunks above are chunks of tiles)
        assert geom["pools"] == 1 and geom["tiles"] == -(-n // 63) and tiles_per_wave(geom) >= 40, geom
        got = eng.finish()
    assert_tables_equal(got, want)
    assert got.n_kept == int((~cheap).sum())


# -------------------------------------------------------------------------------------- the early fold of the bit-sliced planes

def steps_per_tile_one_strand(length):
    """Steps of the packed kernel for a tile of 63 complete records of one strand (csrc/mdx_internal.h: mdx_make_dims H4)."""
    h4 = min(3, 32 // (2 * ((length + A + 15) // 16)))
    return -(-63 // h4)


@pytest.mark.parametrize("Q", [0, 20])
@pytest.mark.parametrize("length", [70, 100])
@pytest.mark.parametrize("shape", ["forward", "reverse", "identical"])
def test_planes_are_folded_before_they_overflow(monkeypatch, shape, length, Q):
    """Complete plain 100-base reads of ONE strand: a wavefront runs more than 255 steps — 21 a tile at --length 70, 32 at
    --length 100 — without anything else folding the eight planes of its counters (a ninth bit would be lost).  "identical": one
    record over and over — single counters carry every step, and with -Q 20 the second set of planes (the masked columns) too."""
    n = 4 * records_for(-(-256 // steps_per_tile_one_strand(length)), 2, WAVES_PK)
    if shape == "identical":
        one = few_low_qualities(synth.make_reads(genome(), 1, 71, read_len=100, frac_reverse=0.0, with_qual=True), 72, frac=0.3)
        batch = concat_batches([one] * 64)
        batch = concat_batches([batch] * (n // 64))
    else:
        batch = few_low_qualities(synth.make_reads(genome(), n, 73, read_len=100, frac_reverse=0.0 if shape == "forward" else 1.0,
                                                   with_qual=True), 74)
    want = oracle_tableset(genome(), batch, libraries(1), length, A, Q)
    with make_engine(monkeypatch, 2, libraries(1), length=length, Q=Q) as eng:
        geom = tabulate(eng, batch, True, True)
        assert eng.packed_launches() == 1
        # (tiles are handed out on demand: four times the tiles of 256 steps per wavefront on average, so that no wavefront of a pool
        # whose others take at most twice their share — see the quota kernels — stays below them)
        assert tiles_per_wave(geom) * steps_per_tile_one_strand(length) >= 4 * 255, geom
        got = eng.finish()
    assert_tables_equal(got, want)


# ---------------------------------------------------------------------------------------------------- tiles of other pools

def skewed(n, expensive, seed):
    """Records [i] from a batch of gapped 150-base reads where ``expensive[i]``, else from one of plain 30-base reads."""
    e = synth.make_reads(genome(), n, seed, read_len=150, frac_ins=0.5, frac_del=0.5)
    c = synth.make_reads(genome(), n, seed + 1, read_len=30)
    return concat_batches([e, c]).take(np.where(expensive, np.arange(n), n + np.arange(n)))


def test_idle_pools_take_the_tiles_of_the_busy_one(monkeypatch):
    """8 compute units: four pools of two blocks.  Chunk c of MDX_POOL_CHUNK tiles belongs to pool c mod 4; the chunks of pool 0 are
    gapped 150-base reads, every other record is dropped by the flag filter: the wavefronts of pools 1-3 run out of their own
    tiles at once and go on with pool 0's."""
    cus, pools = 8, 4
    n = records_for(18, cus, WAVES_PK)
    b = synth.make_reads(genome(), n, 81, read_len=150, frac_ins=0.5, frac_del=0.5)
    busy = (np.arange(n) // (POOL_CHUNK * 63)) % pools == 0
    b.flag = np.where(busy, b.flag, b.flag | 0x200).astype(np.uint16)
    want = oracle_tableset(genome(), b, libraries(1), L, A, 0)
    with make_engine(monkeypatch, cus, libraries(1)) as eng:
        geom = tabulate(eng, b, True, True)
        assert geom["pools"] == pools >= 3 and geom["tiles"] >= 3 * pools * POOL_CHUNK, geom
        got = eng.finish()
    assert_tables_equal(got, want)
    assert got.n_kept == int(busy.sum())


def test_pools_of_one_library_share_its_tiles_only(monkeypatch):
    """Three libraries on four pools: library 0 (70 % of the records) gets two of them, and of its chunks — c mod 2 by pool — the
    even ones are gapped 150-base reads, the odd ones plain 30-base reads; the pool that is done first takes the other's tiles,
    never those of another library (its counts would land in the wrong tables)."""
    cus, pools, nlib = 8, 4, 3
    n = records_for(18, cus, WAVES_PK)
    rng = np.random.default_rng(83)
    lib = np.where(rng.random(n) < 0.7, 0, rng.integers(1, nlib, n)).astype(np.uint16)
    rank = np.cumsum(lib == 0) - 1                    # place of a record of library 0 among its library's
    expensive = np.where(lib == 0, (rank // (POOL_CHUNK * 63)) % 2 == 0, rng.random(n) < 0.5)
    b = skewed(n, expensive, 84)
    b.lib = lib
    want = oracle_tableset(genome(), b, libraries(nlib), L, A, 0)
    with make_engine(monkeypatch, cus, libraries(nlib)) as eng:
        geom = tabulate(eng, b, True, True)
        assert eng.packed_launches() == 1
        # (the plan: two pools for library 0 — its chunks alternate between them —, one for each of the others)
        assert geom["pools"] == pools >= 3 and ml_pools(-(-np.bincount(lib, minlength=nlib) // TILE_ML), pools) == [2, 1, 1], geom
        assert int((lib == 0).sum()) >= 3 * 2 * POOL_CHUNK * TILE_ML
        got = eng.finish()
    assert_tables_equal(got, want)
    assert got.n_kept == n


# ------------------------------------------------------------------------------------------- several libraries on few pools

@functools.lru_cache(maxsize=None)
def skewed_libraries(nlib):
    # (library 1: 90 % of the records, 5 % of them filtered — 43 tiles and more for each of the 32 wavefronts of one pool)
    n = int(records_for(43, 2, WAVES_PK) / 0.9 / 0.95 * 1.02)
    batch = synth.make_reads(genome(), n, 90 + nlib, len_range=(30, 120), nlib=nlib - 1, frac_softclip=0.1, frac_ins=0.05,
                             frac_del=0.05, paired=True, frac_filtered=0.05, with_qual=True)
    batch.lib[np.random.default_rng(nlib).random(n) < 0.9] = 1
    assert not (batch.lib == nlib - 1).any()
    return batch


@functools.lru_cache(maxsize=None)
def skewed_libraries_want(nlib, Q):
    return oracle_tableset(genome(), skewed_libraries(nlib), libraries(nlib), L, A, Q, lgd_max=300)


@pytest.mark.parametrize("own_sort", [True, False], ids=["libsort", "sorted-in-launch"])
@pytest.mark.parametrize("Q", [0, 15])
@pytest.mark.parametrize("cus", [2, 4])
@pytest.mark.parametrize("nlib", [8, 40])
def test_more_libraries_than_pools(monkeypatch, nlib, cus, Q, own_sort):
    """One or two pools for 8 and 40 libraries: a launch counts as many libraries as it has pools, a call is several launches.
    Library 1 holds 90 % of the records — the one pool it gets takes three rounds of them —, the last one none."""
    batch, want = skewed_libraries(nlib), skewed_libraries_want(nlib, Q)
    with make_engine(monkeypatch, cus, libraries(nlib), Q=Q, lgd_max=300) as eng:
        if own_sort:
            dev = eng.upload(batch, packed=True)
            assert dev.dev.libsort
            eng.tabulate(dev)
            eng.sync()
            dev.free()
        else:
            eng.tabulate(batch, packed=True)
        geom = eng.last_launch_geometry()
        assert geom["pools"] == cus // 2 < nlib, geom
        per_library = ml_tiles_per_wave(batch, nlib, geom)
        assert per_library[1] >= 3 * ROUND_TILES and per_library[nlib - 1] == 0, per_library
        assert eng.packed_launches() == -(-nlib // geom["pools"])
        assert eng.libsorts() == (0 if own_sort else 1)
        got = eng.finish()
    assert_tables_equal(got, want)


# ------------------------------------------------------------------------------------------------- errors from a late round

@pytest.mark.parametrize("variant", ["plain", "masked", "libraries", "fused"])
def test_lowest_bad_record_of_a_late_round(monkeypatch, variant):
    """Two records that run past their contig's end: one in the last tile of the batch, one in a tile of a third round (tiles are
    handed out in order: tile t is some wavefront's floor(t / wavefronts)-th).  With three libraries both are records of library 0,
    whose launch works on its kept records in batch order: the tiles are those of that stretch.  The lower index is reported, and
    the context counts a clean batch afterwards as if nothing had happened."""
    from mapdamage_amd.engine import BadReadError
    nlib = 3 if variant == "libraries" else 1
    Q = 20 if variant == "masked" else 0
    n = records_for(43, 2, WAVES_ASCII if variant == "libraries" else WAVES_PK)
    if variant == "fused":      # (the batch of the fused rounds case: records the rescaling takes too)
        clean = synth.make_reads(genome(), n, 41, len_range=(25, 160), paired=True, frac_softclip=0.2, frac_ins=0.05, frac_del=0.05,
                                 frac_skip=0.01, with_qual=True, frac_filtered=0.03)
        want = oracle_tableset(genome(), clean, libraries(1), L, A, 0)
    else:
        clean, want = mixed_batch(n, nlib), mixed_want(n, nlib, Q)
    bad = clean.slice(0, n)
    plain = np.flatnonzero((np.diff(bad.cigar_off.astype(np.int64)) == 1) & ((bad.flag & 0xF04) == 0))
    if variant == "libraries":
        # (place of a record among the kept records of library 0, the order its launch takes them in)
        mine = (bad.lib == 0) & ((bad.flag & FILTERED) == 0)
        place = np.cumsum(mine) - 1
        plain = plain[mine[plain]]
        first, last = int(plain[place[plain] // TILE_ML >= 30 * 2 * WAVES_PK][0]), int(plain[-1])
        assert place[last] // TILE_ML == (int(mine.sum()) - 1) // TILE_ML and place[first] // TILE_ML >= 2 * ROUND_TILES * 2 * WAVES_PK
    else:
        first, last = int(plain[plain > 35 * 2 * WAVES_PK * TILE_MAX][0]), int(plain[-1])
        assert last >= n - 63 and first // 63 >= 2 * ROUND_TILES * 2 * WAVES_PK
    for i in (first, last):
        bad.pos[i] = genome().lengths[int(bad.tid[i])] - 5
    with make_engine(monkeypatch, 2, libraries(nlib), Q=Q) as eng:
        if variant == "fused":
            import torch
            from mapdamage_amd.rescale import RescaleModel
            corr_prob = {(r, s, p): 0.3 for r, s in (("C", "T"), ("G", "A")) for p in list(range(1, 13)) + list(range(-12, 0))}
            eng.set_rescale_model(RescaleModel(corr_prob, 12, 12))
            dev = eng.upload(bad, packed=True)
            t = [torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
                 torch.zeros(bad.seq.shape[0] + 64, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"),
                 torch.zeros(n, dtype=torch.uint8, device="cuda")]
            torch.cuda.synchronize()
            eng.rescale_device(dev, *[x.data_ptr() for x in t], with_tables=True)
            assert eng.fused_launches() == 1
        else:
            dev = eng.upload(bad, packed=True)
            eng.tabulate(dev)
        with pytest.raises(BadReadError) as err:
            eng.sync()
        assert err.value.read_index == first
        geom = eng.last_launch_geometry()
        assert (ml_tiles_per_wave(bad, nlib, geom)[0] if nlib > 1 else tiles_per_wave(geom)) >= 3 * ROUND_TILES, geom
        dev.free()
        eng.reset()
        tabulate(eng, clean, True, True)
        got = eng.finish()
    assert_tables_equal(got, want)


# ----------------------------------------------------------------------------------------------------------- smaller blocks

CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %r)
    from tests import test_gpu_few_cus as t
    from mapdamage_amd.engine import DamageEngine
    length, threads = int(sys.argv[1]), int(sys.argv[2])
    n = t.records_for(43, 2, t.WAVES_PK)
    batch, want = t.mixed_batch(n, 1), t.mixed_want(n, 1, 0, length)
    with DamageEngine(t.libraries(1), length, t.A, 0) as eng:
        eng.set_reference(t.genome())
        geom = t.tabulate(eng, batch, True, True)
        assert eng.packed_launches() == 1
        assert geom["waves_per_block"] == threads // 64 and geom["grid"] * geom["waves_per_block"] <= 2 * t.WAVES_PK, geom
        assert t.tiles_per_wave(geom) >= 3 * t.ROUND_TILES, geom
        t.assert_tables_equal(eng.finish(), want)
    print("few cus ok", geom)
""" % ROOT)


@pytest.mark.parametrize("length,env,threads", [(70, {"MDX_PK_THREADS": "256"}, 256), (170, {}, 512)], ids=["forced-256", "length-170"])
def test_three_rounds_in_smaller_blocks(length, env, threads):
    """The packed kernel's smaller images — blocks of 256 threads, forced, and the blocks of 512 that the tables of --length 170
    leave room for — over three rounds; in a process of its own: the library reads MDX_PK_THREADS once."""
    out = subprocess.run([sys.executable, "-c", CHILD, str(length), str(threads)], cwd=ROOT, env=dict(os.environ, MDX_TEST_CUS="2", **env),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "few cus ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
