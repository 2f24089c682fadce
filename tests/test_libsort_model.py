"""The yardstick of tests/test_gpu_libsort.py checked on the CPU: ``libsort_model.model`` against a loop over the records
with Python lists, a nibble at a time, and ``libsort_model.layout`` against an example worked by hand."""

import numpy as np

from tests.libsort_model import NO_BAD, layout, model


def random_batch(rng, n, nlib, max_len, frac_zero, frac_filtered, frac_unknown):
    flag = (rng.integers(0, 0x100, n) & 0xFB).astype(np.uint16)
    filt = rng.random(n) < frac_filtered
    flag[filt] |= rng.choice(np.array([0x4, 0x100, 0x200, 0x400, 0x800], np.uint16), int(filt.sum()))
    lib = rng.integers(0, nlib, n).astype(np.uint16)
    unk = rng.random(n) < frac_unknown
    lib[unk] = rng.choice(np.array([nlib, nlib + 3, 0xFFFF], np.uint16), int(unk.sum()))
    slen = rng.integers(0, max_len + 1, n)
    slen[rng.random(n) < frac_zero] = 0
    clen = rng.integers(0, 4, n)
    seq_off = np.zeros(n + 1, np.uint32)
    seq_off[1:] = np.cumsum(slen)
    cigar_off = np.zeros(n + 1, np.uint32)
    cigar_off[1:] = np.cumsum(clen)
    nb = int(seq_off[-1])
    nibbles = rng.integers(1, 16, nb + (nb & 1)).astype(np.uint8)
    packed = (nibbles[0::2] | (nibbles[1::2] << 4)).astype(np.uint8)
    return dict(flag=flag, lib=lib, tid=rng.integers(-1, 50, n).astype(np.int32),
                pos=rng.integers(0, 1 << 30, n).astype(np.int32), tlen=rng.integers(-1000, 1000, n).astype(np.int32),
                cigar_off=cigar_off, cigar=rng.integers(0, 1 << 32, int(cigar_off[-1]), dtype=np.uint64).astype(np.uint32),
                seq_off=seq_off, seq_packed=packed)


def by_hand(b, nlib):
    """The same record by record: a list per library, appended to in batch order."""
    n = len(b["flag"])
    buckets = [[] for _ in range(nlib)]
    bad = NO_BAD
    for i in range(n):
        if int(b["flag"][i]) & 0xF04:
            continue
        if int(b["lib"][i]) >= nlib:
            bad = min(bad, (i << 8) | 6)
            continue
        buckets[int(b["lib"][i])].append(i)
    perm, lib_start = [], [0]
    for bucket in buckets:
        perm += bucket
        lib_start.append(len(perm))
    cigar_off, seq_off, cigar, nibbles = [0], [0], [], []
    for i in perm:
        for c in range(int(b["cigar_off"][i]), int(b["cigar_off"][i + 1])):
            cigar.append(int(b["cigar"][c]))
        for s in range(int(b["seq_off"][i]), int(b["seq_off"][i + 1])):
            byte = int(b["seq_packed"][s // 2])
            nibbles.append((byte >> 4) if s % 2 else (byte & 15))
        cigar_off.append(len(cigar))
        seq_off.append(len(nibbles))
    seq = [0] * ((int(b["seq_off"][n]) + 1) // 2 + 64)
    for k, v in enumerate(nibbles):
        seq[k // 2] |= v << (4 * (k % 2))
    return dict(bad=bad, kept=len(perm), lib_start=lib_start, perm=perm, flag=[int(b["flag"][i]) for i in perm],
                tid=[int(b["tid"][i]) for i in perm], pos=[int(b["pos"][i]) for i in perm],
                tlen=[int(b["tlen"][i]) for i in perm], cigar_off=cigar_off, seq_off=seq_off, cigar=cigar, seq=seq,
                seq_bytes=len(seq))


def test_model_equals_a_loop_over_the_records():
    rng = np.random.default_rng(20)
    seen_bad = seen_empty = 0
    for case in range(300):
        n = int(rng.integers(1, 90))
        nlib = int(rng.integers(1, 7))
        b = random_batch(rng, n, nlib, max_len=int(rng.choice([2, 5, 20])), frac_zero=float(rng.choice([0.0, 0.7])),
                         frac_filtered=float(rng.choice([0.0, 0.05, 1.0], p=[0.3, 0.6, 0.1])),
                         frac_unknown=float(rng.choice([0.0, 0.05])))
        got, want = model(nlib=nlib, **b), by_hand(b, nlib)
        assert set(got) == set(want)
        for name, w in want.items():
            g = got[name]
            assert (g.tolist() if isinstance(g, np.ndarray) else g) == w, (case, name)
        seen_bad += want["bad"] != NO_BAD
        seen_empty += want["kept"] == 0
    assert seen_bad > 20 and seen_empty > 5


def test_model_is_stable_and_names_the_lowest_unknown_library():
    """Five records by hand: libraries 1 0 1 (filtered) 0 1, the nibbles of each its own digit."""
    flag = np.array([0, 0x10, 0x400, 0, 0x1], np.uint16)
    lib = np.array([1, 0, 1, 0, 1], np.uint16)
    seq_off = np.array([0, 3, 4, 6, 6, 8], np.uint32)           # lengths 3 1 2 0 2
    nib = np.array([1, 1, 1, 2, 3, 3, 5, 5], np.uint8)
    packed = nib[0::2] | (nib[1::2] << 4)
    cigar_off = np.array([0, 1, 1, 2, 4, 5], np.uint32)
    cigar = np.array([10, 30, 40, 41, 50], np.uint32)
    m = model(flag, lib, np.arange(5), np.arange(5) * 10, -np.arange(5), cigar_off, cigar, seq_off, packed, 2)
    assert m["perm"].tolist() == [1, 3, 0, 4] and m["lib_start"].tolist() == [0, 2, 4] and m["bad"] == NO_BAD
    assert m["tlen"].tolist() == [-1, -3, 0, -4] and m["flag"].tolist() == [0x10, 0, 0, 1]
    assert m["seq_off"].tolist() == [0, 1, 1, 4, 6] and m["cigar_off"].tolist() == [0, 0, 2, 3, 4]
    assert m["cigar"].tolist() == [40, 41, 10, 50]
    assert m["seq"][:4].tolist() == [0x12, 0x11, 0x55, 0] and not m["seq"][3:].any() and m["seq_bytes"] == 4 + 64
    lib[[1, 2, 4]] = [7, 9, 2]            # record 2 is filtered: record 1 is the one to be named
    m = model(flag, lib, np.arange(5), np.arange(5), np.arange(5), cigar_off, cigar, seq_off, packed, 2)
    assert m["bad"] == (1 << 8 | 6) and m["perm"].tolist() == [3, 0]


def test_layout_of_a_small_blob():
    """n = 5, 7 operations, 21 bases, 3 libraries: 21 entries per column (84 bytes -> 96; the 16-bit flags 42 -> 48),
    23 CIGAR words (92 -> 96), 11 + 64 SEQ bytes (75 -> 80)."""
    lay = layout(5, 7, 21, 3)
    assert lay == dict(bad=0, lib_start=16, perm=32, tid=128, pos=224, tlen=320, cigar_off=416, seq_off=512, flag=608,
                       cigar=656, seq=752, seq_bytes=75, total=1088)
    a16 = lambda v: (v + 15) // 16 * 16
    for n, n_cigar, n_bases, nlib in ((5, 7, 21, 3), (1, 0, 0, 2), (4096, 9000, 123_457, 300), (900_000, 1_350_000, 901_234, 5000)):
        lay = layout(n, n_cigar, n_bases, nlib)
        n1 = n + 16
        sizes = dict(bad=16, lib_start=(nlib + 1) * 4, perm=n1 * 4, tid=n1 * 4, pos=n1 * 4, tlen=n1 * 4, cigar_off=n1 * 4,
                     seq_off=n1 * 4, flag=n1 * 2, cigar=(n_cigar + 16) * 4, seq=lay["seq_bytes"])
        order = sorted(sizes, key=lambda k: lay[k])
        assert order == ["bad", "lib_start", "perm", "tid", "pos", "tlen", "cigar_off", "seq_off", "flag", "cigar", "seq"]
        for name, nxt in zip(order, order[1:] + ["total"]):
            assert lay[name] % 16 == 0 and lay[name] + sizes[name] <= lay[nxt]
        # mdx_k_libsort_bytes
        assert lay["total"] == 16 + a16((nlib + 1) * 4) + a16(n1 * 4) * 6 + a16(n1 * 2) + a16((n_cigar + 16) * 4) + \
            a16((n_bases + 1) // 2 + 64) + 256
