"""The packed kernel compiled for the default geometry (csrc/mdx_kernels.hip: tabulate_kernel<.., GEO = 1>, MdxGeo — --length 70
--around 10, one library, no --min-basequal, a block of 1024 threads with the prefetch areas): it runs where, and only where, a
launch passes what it has folded (``geo_spec_launches``), and counts what the kernel that takes its geometry from its arguments
counts (MDX_NO_GEO_SPEC=1, read once per process: the comparisons run in child processes) — the reference's goldens and the C
oracle decide."""

import functools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from mapdamage_amd import synth
from mapdamage_amd.batch import concat_batches
from mapdamage_amd.tables import TableSet
from tests.test_gpu_few_cus import WAVES_PK, genome, libraries, records_for
from tests.util import Golden, assert_tables_equal, oracle_tableset

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, A = 70, 10
TILE = 63                       # records of a tile of the packed kernels at --length 70 (csrc/mdx_internal.h: mdx_tile_records)
PK_QCAP = 112                   # ... events a wavefront's queue holds (a lane with a column that is no plain match is one)
N_MIX = records_for(3, 2, WAVES_PK)     # 6 144: three tiles per wavefront of two compute units


def engine(libs=1, length=L, around=A, **kw):
    from mapdamage_amd.engine import DamageEngine
    eng = DamageEngine(libraries(libs), length, around, 0, **kw)
    eng.set_reference(genome())
    return eng


def tabulate_resident(eng, batch):
    dev = eng.upload(batch, packed=True)
    eng.tabulate(dev)
    eng.sync()
    return dev


def one_indel(batch, g, deletion):
    """Plain 100-base records -> M a, {I | D} g, M b, the read's bases as they are (a + b [+ g] = 100)."""
    n = batch.n
    assert (np.diff(batch.cigar_off.astype(np.int64)) == 1).all() and (batch.cigar == (100 << 4)).all()
    a = 20 + (np.arange(n) * 7) % 50
    b = 100 - a - (0 if deletion else g)
    cig = np.empty((n, 3), np.uint32)
    cig[:, 0], cig[:, 1], cig[:, 2] = a << 4, (g << 4) | (2 if deletion else 1), b << 4
    batch.cigar = cig.reshape(-1)
    batch.cigar_off = (3 * np.arange(n + 1)).astype(np.uint32)
    # (a deletion lengthens the stretch of the reference: keep the record and its flank inside the contig)
    lens = np.asarray(genome().lengths)[batch.tid]
    batch.pos = np.minimum(batch.pos, lens - 100 - g - A - 1).astype(np.int32)
    return batch.validate()


@functools.lru_cache(maxsize=None)
def mix_batch():
    """N_MIX records, one library: the config-3 mix (pairs, soft clips, indels, N operations, hard clips), reads of 35-69 bases,
    single insertions and deletions of 7 bases (phase 1 of the tile loop makes their entries) and of 8 (the general pass does),
    plain records 0, 3, 9 and 10 bases from either end of a contig (flanks cut short, and just complete), 252 records in a row
    whose every base is a mismatch (4 tiles of 63 records x 12 lanes of events: a step's events do not fit what is left of a queue
    of PK_QCAP), and 252 records in a row of the reverse strand (two whole tiles of them at least)."""
    ref = genome()
    plain = lambda n, seed, **kw: synth.make_reads(ref, n, seed, read_len=100, **kw)
    parts = [synth.config3_batch(ref, 3000, seed=3), synth.make_reads(ref, 1200, 5, len_range=(35, 69))]
    for k, (g, deletion) in enumerate(((7, False), (7, True), (8, False), (8, True))):
        parts.append(one_indel(plain(150, 20 + k), g, deletion))
    edges = plain(16, 30, contigs=[0, 1])
    lens = np.asarray(ref.lengths)[edges.tid]
    k = np.tile(np.array([0, 3, 9, 10]), 4)
    edges.pos = np.where(np.arange(16) < 8, k, lens - 100 - k).astype(np.int32)
    parts.append(edges)
    wrong = plain(4 * TILE, 31)
    swap = np.arange(256, dtype=np.uint8)
    for x, y in zip(b"ACGT", b"CGTA"):
        swap[x] = y
    wrong.seq = swap[wrong.seq]
    assert 4 * TILE * 12 > 4 * PK_QCAP
    parts.append(wrong)
    rev = plain(4 * TILE, 32)
    rev.flag = (rev.flag | 0x10).astype(np.uint16)
    parts.append(rev)
    n_so_far = sum(p.n for p in parts)
    parts.append(synth.config3_batch(ref, N_MIX - n_so_far, seed=33))
    batch = concat_batches(parts)
    assert batch.n == N_MIX and (batch.lib == 0).all()
    # (the reverse stretch covers two whole tiles wherever it starts)
    lo = n_so_far - 4 * TILE
    t0 = -(-lo // TILE)
    assert (batch.flag[t0 * TILE:(t0 + 2) * TILE] & 0x10).all() and (t0 + 2) * TILE <= n_so_far
    return batch


@functools.lru_cache(maxsize=None)
def mix_want():
    return oracle_tableset(genome(), mix_batch(), libraries(1), L, A, 0)


# ------------------------------------------------------------------------------------------------------------------ goldens

@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
@pytest.mark.parametrize("name", ["indelshapes_L70_A10_Q0", "edge_L70_A10_Q0"])
def test_goldens_library_by_library(name, resident):
    """The golden's two libraries, each tabulated by a context of ONE library from a 4-bit SEQ column — every launch the compiled-in
    geometry's —, put side by side: tables and texts are the reference's (the edge records include fragment lengths beyond lgd_max:
    the list of those names the library, 0 in a context of one)."""
    from mapdamage_amd.engine import DamageEngine
    g = Golden(name)
    assert (g.length, g.around, g.minqual) == (L, A, 0) and len(g.libraries) == 2
    got = []
    for k, lib in enumerate(g.libraries):
        b = g.batch.take(np.flatnonzero(g.batch.lib == k))
        b.lib = np.zeros(b.n, np.uint16)
        with DamageEngine([lib], L, A, 0) as eng:
            eng.set_reference(g.ref)
            if resident:
                tabulate_resident(eng, b).free()
            else:
                eng.tabulate(b, packed=True)
            assert eng.geo_spec_launches() == eng.packed_launches() == 1
            t = eng.finish()
        assert (t.lgd_over[:, 0] == 0).all()
        t.lgd_over[:, 0] = k
        got.append(t)
    both = TableSet(list(g.libraries), L, A, np.concatenate([t.mis for t in got]), np.concatenate([t.comp for t in got]),
                    np.concatenate([t.lgd for t in got]), np.concatenate([t.lgd_over for t in got]), sum(t.n_kept for t in got))
    g.check(both)


# ------------------------------------------------------------------------------------------- specialised against generic

CHILD = textwrap.dedent("""
    import sys
    import numpy as np
    sys.path.insert(0, %r)
    from tests import test_gpu_geo_spec as t
    out, want_spec, min_tiles = sys.argv[1], int(sys.argv[2]), float(sys.argv[3])
    batch = t.mix_batch()
    with t.engine() as eng:
        dev = t.tabulate_resident(eng, batch)
        geom = eng.last_launch_geometry()
        assert eng.packed_launches() == 1 and eng.geo_spec_launches() == want_spec, (eng.packed_launches(), eng.geo_spec_launches())
        assert geom["tiles"] / (geom["grid"] * geom["waves_per_block"]) >= min_tiles, geom
        got = eng.finish()
        dev.free()
    np.savez(out, mis=got.mis, comp=got.comp, lgd=got.lgd, lgd_over=got.lgd_over, n_kept=np.int64(got.n_kept))
    print("geo spec ok", geom)
""" % ROOT)


def child(out, want_spec, min_tiles=0.0, **env):
    r = subprocess.run([sys.executable, "-c", CHILD, str(out), str(want_spec), str(min_tiles)], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "geo spec ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("cus", [None, 2], ids=["whole-device", "2-cus"])
def test_specialised_kernel_counts_what_the_generic_one_counts(tmp_path, cus):
    """The mixed batch, resident, in two processes — the compiled-in geometry, and MDX_NO_GEO_SPEC=1 —: every word of the tables the
    same, and the oracle's.  "2-cus": every wavefront takes three tiles on average and more (tiles are handed out on demand), its
    prefetch area, staging area and queue in use tile after tile."""
    env = {} if cus is None else {"MDX_TEST_CUS": str(cus)}
    min_tiles = 0.0 if cus is None else 3.0
    spec = child(tmp_path / "spec.npz", 1, min_tiles, MDX_NO_GEO_SPEC="", **env)
    generic = child(tmp_path / "generic.npz", 0, min_tiles, MDX_NO_GEO_SPEC="1", **env)
    want = mix_want()
    for key in ("mis", "comp", "lgd", "lgd_over", "n_kept"):
        np.testing.assert_array_equal(spec[key], generic[key], err_msg=key)
    np.testing.assert_array_equal(spec["mis"], want.mis)
    np.testing.assert_array_equal(spec["comp"], want.comp)
    np.testing.assert_array_equal(spec["lgd"], want.lgd)
    assert spec["lgd_over"].shape[0] == want.lgd_over.shape[0] == 0
    assert int(spec["n_kept"]) == want.n_kept > 0


# ------------------------------------------------------------------------------------------------------ the predicate is exact

@functools.lru_cache(maxsize=None)
def small_batch(nlib):
    return synth.make_reads(genome(), 3000, 41 + nlib, len_range=(35, 130), paired=True, frac_softclip=0.1, frac_ins=0.05, frac_del=0.05,
                            frac_skip=0.002, nlib=nlib)


@pytest.mark.parametrize("length,around,nlib,lgd_max", [(69, 10, 1, 65536), (71, 10, 1, 65536), (70, 9, 1, 65536), (70, 11, 1, 65536),
                                                        (70, 10, 1, 100), (70, 10, 2, 65536)],
                         ids=["L69", "L71", "A9", "A11", "lgd_max-100", "two-libraries"])
def test_any_other_geometry_takes_the_generic_kernel(length, around, nlib, lgd_max):
    """One step off the default in --length or --around, a fragment-length histogram so short (lgd_max 100 against 65 536) that its
    part in the LDS is another size, two libraries: the packed kernel runs, the compiled-in geometry does not, the oracle's tables."""
    batch = small_batch(nlib)
    want = oracle_tableset(genome(), batch, libraries(nlib), length, around, 0, lgd_max=lgd_max)
    with engine(nlib, length, around, lgd_max=lgd_max) as eng:
        tabulate_resident(eng, batch).free()
        assert eng.packed_launches() > 0 and eng.geo_spec_launches() == 0
        got = eng.finish()
    assert_tables_equal(got, want)


def test_default_geometry_in_blocks_of_512_takes_the_generic_kernel(tmp_path):
    """--length 70 --around 10 in blocks of 512 threads (MDX_PK_THREADS, read once per process): another block, another image."""
    got = child(tmp_path / "b512.npz", 0, 3.0, MDX_PK_THREADS="512", MDX_TEST_CUS="2")
    want = mix_want()
    np.testing.assert_array_equal(got["mis"], want.mis)
    np.testing.assert_array_equal(got["comp"], want.comp)
    np.testing.assert_array_equal(got["lgd"], want.lgd)
    assert int(got["n_kept"]) == want.n_kept


# ------------------------------------------------------------------------------------------------------------------- twice

def test_counters_double_when_the_batch_is_tabulated_twice():
    batch, want = mix_batch(), mix_want()
    with engine() as eng:
        dev = eng.upload(batch, packed=True)
        for _ in range(2):
            eng.tabulate(dev)
            eng.sync()
        assert eng.geo_spec_launches() == eng.packed_launches() == 2
        got = eng.finish()
        dev.free()
    np.testing.assert_array_equal(got.mis, 2 * want.mis)
    np.testing.assert_array_equal(got.comp, 2 * want.comp)
    np.testing.assert_array_equal(got.lgd, 2 * want.lgd)
    assert got.n_kept == 2 * want.n_kept
