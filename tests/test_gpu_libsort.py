"""The by-library sort on the device (csrc/mdx_libsort.hip) against a stable sort, place by place.

Every run with several libraries goes through the sort in front of the packed kernel, and the tests of the tables cannot
tell a sort that moves records within a library, names a wrong index in ``perm`` or hands a record its neighbour's template
length: the tables are sums.  Here the blob a resident batch brings (``mdx_batch::libsort``) is read back and compared with
``tests/libsort_model.model`` over the device batch's own columns — the columns as ``mdx_batch_upload`` left them are what
the sort read.  The packed column holds random nibbles 1..15, so a nibble that is misplaced or left zero shows; the shapes
are the smallest at which each path of the kernels exists (the table of CASES).

The blob of a sort inside a launch is the context's own: those cases (short reads, a caller's column at an odd address)
compare the tables with the oracle's."""

import ctypes
import functools
import time

import numpy as np
import pytest

from mapdamage_amd import synth
from tests.libsort_model import d2h, model, read_blob
from tests.util import assert_tables_equal, oracle_tableset

pytestmark = pytest.mark.gpu

FILTER_BITS = np.array([0x4, 0x100, 0x200, 0x400, 0x800], np.uint16)      # reader.py:121-132


def libraries(n):
    return [("S%d" % i, "L%d" % i) for i in range(n)]


# ---------------------------------------------------------------------- the batches
def make_batch(n, nlib, seed, lens=(0, 20), zeros=0.0, filtered=0.05, lib="uniform", empty_run=0, unknown=False,
               distinct=False, qual=False, n_tid=50):
    """Host columns of a batch of ``n`` records over ``nlib`` libraries (a dict of the names of ``MdxBatch``).

    lens: SEQ lengths drawn uniformly from [lo, hi]; zeros: that share of the records emptied; filtered: the share that
    carries a bit of the flag filter, or "one" for exactly one record; lib: "uniform", "skew" (half of the records in
    library 1) or a number (every record there); empty_run: that many consecutive places of library 1 emptied; unknown:
    three records with a library the context does not have, the first of them filtered; distinct: tid, pos and tlen
    differ from record to record."""
    rng = np.random.default_rng([seed, n, nlib])
    flag = (rng.integers(0, 0x100, n) & 0xFB).astype(np.uint16)
    if filtered == "one":
        flag[n // 2] |= 0x400
    elif filtered:
        f = rng.random(n) < filtered
        flag[f] |= rng.choice(FILTER_BITS, int(f.sum()))
    if lib == "uniform":
        libcol = rng.integers(0, nlib, n).astype(np.uint16)
    elif lib == "skew":
        libcol = rng.integers(0, nlib, n).astype(np.uint16)
        libcol[rng.random(n) < 0.5] = 1
    else:
        libcol = np.full(n, lib, np.uint16)
    slen = rng.integers(lens[0], lens[1] + 1, n)
    slen[rng.random(n) < zeros] = 0
    if empty_run:
        mine = np.flatnonzero(((flag & 0xF04) == 0) & (libcol == 1))
        assert mine.shape[0] > 300 + empty_run
        slen[mine[300:300 + empty_run]] = 0
    if unknown:
        at = np.array([n // 5, n // 3, n // 2])
        libcol[at] = [nlib, nlib + 9, 0xFFFF]
        flag[at[0]] |= 0x100
        flag[at[1:]] &= 0xFB
    if distinct:
        tid, pos, tlen = rng.permutation(n), rng.permutation(n) + 7, rng.permutation(n) - n // 2
    else:
        tid, pos, tlen = rng.integers(-1, n_tid, n), rng.integers(0, 1 << 30, n), rng.integers(-2000, 2000, n)
    seq_off = np.zeros(n + 1, np.uint32)
    seq_off[1:] = np.cumsum(slen)
    cigar_off = np.zeros(n + 1, np.uint32)
    cigar_off[1:] = np.cumsum(rng.integers(0, 4, n))
    nb = int(seq_off[-1])
    nibbles = rng.integers(1, 16, nb + (nb & 1)).astype(np.uint8)
    cols = dict(flag=flag, lib=libcol, tid=tid.astype(np.int32), pos=pos.astype(np.int32), tlen=tlen.astype(np.int32),
                cigar_off=cigar_off, cigar=rng.integers(0, 1 << 32, int(cigar_off[-1]), dtype=np.uint64).astype(np.uint32),
                seq_off=seq_off, seq=(nibbles[0::2] | (nibbles[1::2] << 4)).astype(np.uint8))
    if qual:
        cols["qual"] = rng.integers(2, 42, nb).astype(np.uint8)
    return cols


def upload(eng, cols):
    """The host columns as an ``MdxBatch`` with a 4-bit SEQ column, through ``mdx_batch_upload`` -> a ``DeviceBatch``."""
    from mapdamage_amd.engine import SEQ_4BIT, DeviceBatch, MdxBatch
    hb = MdxBatch()
    hb.n_reads, hb.n_cigar, hb.n_bases = cols["flag"].shape[0], cols["cigar"].shape[0], int(cols["seq_off"][-1])
    keep = {k: np.ascontiguousarray(v) for k, v in cols.items()}
    for name, arr in keep.items():
        setattr(hb, name, arr.ctypes.data)
    hb.seq_format = SEQ_4BIT
    dev = MdxBatch()
    eng._check(eng._lib.mdx_batch_upload(eng._ctx, ctypes.byref(hb), ctypes.byref(dev)))
    return DeviceBatch(eng, dev, hb.n_reads, hb.n_bases, hb.n_cigar)


def device_columns(db):
    """The device batch's own columns, as the sort read them."""
    d, n = db.dev, db.n
    return dict(flag=d2h(d.flag, n, np.uint16), lib=d2h(d.lib, n, np.uint16), tid=d2h(d.tid, n, np.int32),
                pos=d2h(d.pos, n, np.int32), tlen=d2h(d.tlen, n, np.int32), cigar_off=d2h(d.cigar_off, n + 1, np.uint32),
                cigar=d2h(d.cigar, db.n_cigar, np.uint32), seq_off=d2h(d.seq_off, n + 1, np.uint32),
                seq_packed=d2h(d.seq, (db.n_bases + 1) // 2, np.uint8))


def check_blob(db, nlib, key=None):
    """The blob of the resident batch ``db`` equals the model over its columns, up to the kept records; -> the model.
    key: a function of the columns that gives the column the context sorted by (default: the lib column)."""
    assert db.dev.libsort
    cols = device_columns(db)
    if key is not None:
        cols["lib"] = key(cols)
    want = model(nlib=nlib, **cols)
    got = read_blob(db.dev.libsort, db.n, db.n_cigar, db.n_bases, nlib)
    kept = want["kept"]
    assert got["bad"] == want["bad"]
    np.testing.assert_array_equal(got["lib_start"], want["lib_start"])
    for name in ("perm", "flag", "tid", "pos", "tlen"):
        np.testing.assert_array_equal(got[name][:kept], want[name], err_msg=name)
    for name in ("cigar_off", "seq_off"):
        np.testing.assert_array_equal(got[name][:kept + 1], want[name], err_msg=name)
    np.testing.assert_array_equal(got["cigar"][:want["cigar"].shape[0]], want["cigar"])
    assert got["seq_bytes"] == want["seq_bytes"]
    np.testing.assert_array_equal(got["seq"], want["seq"])
    return want


def small_engine(nlib, minqual=0, groups=None):
    """The sort depends on the number of libraries alone: small tables, so that thousands of libraries are cheap."""
    from mapdamage_amd.engine import DamageEngine
    return DamageEngine(libraries(nlib), 20, 4, minqual, lgd_max=256, groups=groups)


# ---------------------------------------------------------------------- 1. the blob, place by place
CASES = {
    # wavefront (64 places), copy tile (256) and block edges
    **{"n%d" % n: dict(n=n, nlib=2) for n in (1, 63, 64, 65, 255, 256, 257)},
    # sort blocks and scan blocks of 4096: no record filtered, so that `kept` lands on and next to the boundary, where entry
    # `kept` of the offset columns is the first of the next scan block
    **{"kept%d" % n: dict(n=n, nlib=3, filtered=0.0) for n in (4095, 4096, 4097, 8193)},
    "kept4096_of_4097": dict(n=4097, nlib=3, filtered="one"),
    # three to eight records per dword of the new column; a stretch border with places beyond the 72 kept in the LDS
    "many_per_dword": dict(n=5000, nlib=2, lens=(0, 2), zeros=0.7),
    # wavefronts all of whose 64 places are empty
    "empty_wavefronts": dict(n=5000, nlib=2, lens=(0, 3), empty_run=200),
    "no_bases": dict(n=700, nlib=3, lens=(0, 0)),
    "nothing_kept": dict(n=700, nlib=3, filtered=1.0),
    "one_library_owns_all": dict(n=1000, nlib=5, lib=3),
    "skew_stability": dict(n=5000, nlib=40, lib="skew", distinct=True),
    # the scan of the counts: m = blocks x libraries entries over 1024 threads
    "counts_m2": dict(n=100, nlib=2),
    "counts_m1500": dict(n=20_000, nlib=300),
    # more libraries than LS_LDS_LIBS = 4096: counts and places in global memory
    "global_places": dict(n=20_000, nlib=5000, lens=(0, 5)),
    "unknown_libraries": dict(n=3000, nlib=4, unknown=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_blob_equals_a_stable_sort(name):
    case = dict(CASES[name])
    n, nlib = case.pop("n"), case.pop("nlib")
    cols = make_batch(n, nlib, 1, **case)
    with small_engine(nlib) as eng:
        db = upload(eng, cols)
        try:
            want = check_blob(db, nlib)
        finally:
            db.free()
    # the case is the one its name says
    if name.startswith("kept"):
        assert want["kept"] == int(name[4:8])
    elif name == "many_per_dword":
        off, kept = want["seq_off"].astype(np.int64), want["kept"]
        assert np.diff(off).max() <= 2 and np.bincount(off[:-1][np.diff(off) > 0] // 8).max() >= 6
        # a wavefront's last dword (it begins inside the wavefront's 64 places) that ends behind place 72's first nibble
        d1 = off[64:kept:64]
        d0, o72 = off[0:kept - 64:64][:d1.shape[0]], off[np.minimum(np.arange(72, kept + 8, 64), kept)][:d1.shape[0]]
        assert ((d1 % 8 != 0) & (d1 // 8 * 8 >= d0) & (o72 < d1 // 8 * 8 + 8)).sum() > 10
    elif name == "empty_wavefronts":
        ln = np.diff(want["seq_off"].astype(np.int64))
        assert any(not ln[r0:r0 + 64].any() for r0 in range(0, want["kept"] - 63, 64))
    elif name == "no_bases":
        assert int(cols["seq_off"][-1]) == 0 and want["kept"] > 0
    elif name == "nothing_kept":
        assert want["kept"] == 0 and not want["lib_start"].any()
    elif name == "one_library_owns_all":
        assert want["lib_start"].tolist() == [0, 0, 0, 0, want["kept"], want["kept"]] and want["kept"] > 900
    elif name == "skew_stability":
        assert np.diff(want["lib_start"].astype(np.int64))[1] > want["kept"] // 2
    elif name == "unknown_libraries":
        assert want["bad"] == ((n // 3) << 8 | 6) and want["kept"] < n - 2


def test_blob_at_the_cap_on_blocks():
    """5 000 libraries allow 2^20 / 5000 = 209 blocks (csrc/mdx_libsort.hip ``geometry``): 900 000 records are more than
    209 x 4096, so a block takes more than 4096 of them.  Reads of 0 to 2 bases keep the batch small."""
    n, nlib = 900_000, 5000
    assert n > (2 ** 20 // nlib) * 4096
    cols = make_batch(n, nlib, 2, lens=(0, 2))
    with small_engine(nlib) as eng:
        t0 = time.perf_counter()
        db = upload(eng, cols)
        print("upload and sort of %d records over %d libraries: %.3f s" % (n, nlib, time.perf_counter() - t0))
        try:
            check_blob(db, nlib)
        finally:
            db.free()


def test_blob_with_the_mask_in_the_nibbles():
    """--min-basequal: ``mdx_batch_upload`` folds the mask into the column (MDX_SEQ_4BITQ) in front of the sort; the masked
    nibbles travel with their records."""
    cols = make_batch(3000, 3, 3, qual=True)
    with small_engine(3, minqual=20) as eng:
        db = upload(eng, cols)
        try:
            assert db.dev.seq_format == 2
            folded = d2h(db.dev.seq, (db.n_bases + 1) // 2, np.uint8)
            assert (folded != cols["seq"]).mean() > 0.3
            check_blob(db, 3)
        finally:
            db.free()


def test_blob_ordered_by_stratum():
    """A stratified context sorts by library x groups + group of the record's sequence (csrc/mdx_internal.h: 0xFFFF for a
    library the context does not have, group 0 for a sequence outside the header)."""
    group_of_tid = np.array([0, 1, 0, 2, 1], np.int64)
    n_lib, n_groups = 3, 3
    cols = make_batch(6000, n_lib, 4, n_tid=7, unknown=True)
    assert (cols["tid"] < 0).any() and (cols["tid"] >= 5).any()

    def key(c):
        tid = c["tid"].astype(np.int64)
        group = np.where((tid >= 0) & (tid < 5), group_of_tid[np.clip(tid, 0, 4)], 0)
        return np.where(c["lib"] < n_lib, c["lib"].astype(np.int64) * n_groups + group, 0xFFFF)

    with small_engine(n_lib, groups=["g0", "g1", "g2"]) as eng:
        eng.set_strata(group_of_tid)
        db = upload(eng, cols)
        try:
            want = check_blob(db, n_lib * n_groups, key)
        finally:
            db.free()
    assert (np.diff(want["lib_start"].astype(np.int64)) > 0).all() and want["bad"] == ((6000 // 3) << 8 | 6)


# ---------------------------------------------------------------------- 2. the sort inside the launch
INDELS = dict(frac_softclip=0.1, frac_ins=0.05, frac_del=0.05)
LIBS3 = libraries(3)


@functools.lru_cache(maxsize=None)
def mid_genome():
    return synth.make_genome(seed=11, sizes=(("chr1", 300_000), ("chr2", 100_000), ("chrS", 500)), n_run=500, lower_run=3000)


@functools.lru_cache(maxsize=None)
def reads(lo, hi, indels):
    """(batch, the oracle's tables): 20 000 paired records of lo to hi bases over three libraries, one in twenty filtered
    (indels: every tenth with an insertion or a deletion, fewer records — see below)."""
    b = synth.make_reads(mid_genome(), 20_000, 100 + lo, len_range=(lo, hi), nlib=3, paired=True, frac_filtered=0.05,
                         **(INDELS if indels else {}))
    if indels:
        # The generator keeps five aligned bases on either side of an insertion or deletion; around a read with fewer than
        # five it writes a CIGAR that asks for more bases than the record has (3I5M over five bases) — no record of a BAM
        # file, and one the kernel rightly reports (CIGAR / SEQ mismatch).  Those few per cent are left out.
        op, ln = (b.cigar & 15).astype(np.int64), (b.cigar >> 4).astype(np.int64)
        n_ops = np.diff(b.cigar_off.astype(np.int64))
        query = np.bincount(np.repeat(np.arange(b.n), n_ops), weights=ln * np.isin(op, (0, 1, 4, 7, 8)), minlength=b.n)
        formed = query == np.diff(b.seq_off.astype(np.int64))
        assert 0.9 < formed.mean() < 1 and (n_ops[formed] > 1).sum() > 1000
        b = b.take(np.flatnonzero(formed))
    return b, oracle_tableset(mid_genome(), b, LIBS3, 70, 10, 0, lgd_max=300)


def view_without_sort(dev):
    view = type(dev.dev)()
    ctypes.memmove(ctypes.byref(view), ctypes.byref(dev.dev), ctypes.sizeof(view))
    view.libsort = None
    return view


@pytest.mark.parametrize("way", ["resident", "in-launch"])
@pytest.mark.parametrize("indels", [False, True], ids=["plain", "indels"])
def test_short_reads_through_the_sort(indels, way):
    """Reads of 1 to 12 bases: a dword of the sorted column holds up to eight records.  Through the blob of the resident
    batch and through the sort inside the launch; a base that moves moves a count."""
    from mapdamage_amd.engine import DamageEngine
    batch, want = reads(1, 12, indels)
    with DamageEngine(LIBS3, 70, 10, 0, lgd_max=300) as eng:
        eng.set_reference(mid_genome())
        dev = eng.upload(batch, packed=True)
        try:
            assert dev.dev.libsort
            if way == "resident":
                eng.tabulate(dev)
            else:
                eng.tabulate_view(view_without_sort(dev))
            eng.sync()
            assert eng.packed_launches() == 1 and eng.libsorts() == (0 if way == "resident" else 1)
            got = eng.finish()
        finally:
            dev.free()
    assert_tables_equal(got, want)


@pytest.mark.parametrize("lens,phase", [((1, 12), 1), ((1, 12), 2), ((1, 12), 3), ((30, 120), 3)],
                         ids=["short-1", "short-2", "short-3", "long-3"])
def test_sort_of_a_column_at_an_odd_address(lens, phase):
    """A caller's own 4-bit column that begins 1, 2 or 3 bytes behind a dword boundary, several libraries: the sort inside
    the launch reads it from the boundary in front and shifts by the phase.  0xFF in front of and behind the column:
    a nibble read from outside it is a base the oracle does not have.  (The case with reads of 30 to 120 bases tells a fault
    of the phase from one of short reads.)"""
    import torch
    from mapdamage_amd.engine import DamageEngine, pack_seq
    batch, want = reads(lens[0], lens[1], False)
    pk = pack_seq(batch.seq)
    with DamageEngine(LIBS3, 70, 10, 0, lgd_max=300) as eng:
        eng.set_reference(mid_genome())
        dev = eng.upload(batch, packed=True)
        try:
            tseq = torch.full((pk.shape[0] + 128,), 0xFF, dtype=torch.uint8, device="cuda")
            at = 64 + phase
            tseq[at:at + pk.shape[0]] = torch.from_numpy(pk).cuda()
            torch.cuda.synchronize()
            assert (tseq.data_ptr() + at) % 4 == phase
            view = view_without_sort(dev)
            view.seq = tseq.data_ptr() + at
            eng.tabulate_view(view)
            eng.sync()
            assert eng.packed_launches() == 1 and eng.libsorts() == 1
            got = eng.finish()
        finally:
            dev.free()
    assert_tables_equal(got, want)
