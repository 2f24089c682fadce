"""The by-library sort (csrc/mdx_libsort.hip) in plain numpy, and a reader for the blob the device writes.

``model`` is what ``MdxLibSort`` documents (csrc/mdx_internal.h): the kept records of a batch in a stable order by
library, the fixed columns gathered, new CIGAR and SEQ offset columns, the CIGAR words and the SEQ nibbles concatenated in
the new order.  ``layout`` and ``read_blob`` take the device's blob apart so that a test can compare it place by place."""

import ctypes

import numpy as np

NO_BAD = 2 ** 64 - 1
ERR_BAD_READ = 6          # csrc/mdx_libsort.hip LS_ERR_BAD_READ


def _ragged_gather(start, length):
    """Indices start[r], start[r] + 1, ... start[r] + length[r] - 1 for every r, concatenated; and the exclusive sums of
    ``length`` with the total behind them."""
    off = np.zeros(length.shape[0] + 1, np.int64)
    np.cumsum(length, out=off[1:])
    idx = np.repeat(start - off[:-1], length) + np.arange(int(off[-1]), dtype=np.int64)
    return idx, off


def model(flag, lib, tid, pos, tlen, cigar_off, cigar, seq_off, seq_packed, nlib):
    """The sorted batch as a dict of arrays: bad, kept, lib_start [nlib + 1], perm, flag, tid, pos, tlen [kept],
    cigar_off, seq_off [kept + 1], cigar [total operations], seq [seq_bytes], seq_bytes.

    ``lib`` is the key the device sorts by (the library, or the stratum of a stratified context); ``seq_packed`` the
    MDX_SEQ_4BIT column (include/mdx.h: base i in bits [4 (i & 1), 4 (i & 1) + 4) of byte i / 2)."""
    flag = np.asarray(flag)
    key = np.asarray(lib).astype(np.int64)
    cigar_off = np.asarray(cigar_off).astype(np.int64)
    seq_off = np.asarray(seq_off).astype(np.int64)
    seq_packed = np.asarray(seq_packed, np.uint8)
    n = flag.shape[0]
    passes = (flag.astype(np.int64) & 0xF04) == 0
    kept_mask = passes & (key < nlib)
    idx = np.flatnonzero(kept_mask)
    perm = idx[np.argsort(key[idx], kind="stable")]
    kept = int(perm.shape[0])
    lib_start = np.zeros(nlib + 1, np.int64)
    np.cumsum(np.bincount(key[idx], minlength=nlib), out=lib_start[1:])
    unknown = np.flatnonzero(passes & (key >= nlib))
    bad = ((int(unknown[0]) << 8) | ERR_BAD_READ) if unknown.shape[0] else NO_BAD

    c_idx, new_co = _ragged_gather(cigar_off[perm], cigar_off[perm + 1] - cigar_off[perm])
    s_idx, new_so = _ragged_gather(seq_off[perm], seq_off[perm + 1] - seq_off[perm])
    n_bases = int(seq_off[n]) if n else 0
    seq_bytes = (n_bases + 1) // 2 + 64
    nib = (seq_packed[s_idx >> 1] >> (4 * (s_idx & 1)).astype(np.uint8)) & np.uint8(15)
    seq = np.zeros(seq_bytes, np.uint8)
    total = int(new_so[-1])
    seq[:(total + 1) // 2] = nib[0::2]
    seq[:total // 2] |= nib[1::2] << np.uint8(4)
    return dict(bad=bad, kept=kept, lib_start=lib_start.astype(np.uint32), perm=perm.astype(np.uint32),
                flag=flag[perm].astype(np.uint16), tid=np.asarray(tid)[perm].astype(np.int32),
                pos=np.asarray(pos)[perm].astype(np.int32), tlen=np.asarray(tlen)[perm].astype(np.int32),
                cigar_off=new_co.astype(np.uint32), seq_off=new_so.astype(np.uint32),
                cigar=np.asarray(cigar, np.uint32)[c_idx], seq=seq, seq_bytes=seq_bytes)


def _align16(v):
    return (v + 15) & ~15


# the parts of the blob behind its header, in the order they lie: (name, dtype)
_PARTS = (("perm", np.uint32), ("tid", np.int32), ("pos", np.int32), ("tlen", np.int32), ("cigar_off", np.uint32),
          ("seq_off", np.uint32), ("flag", np.uint16))


def layout(n, n_cigar, n_bases, nlib):
    """Byte offsets of the blob's parts, ``seq_bytes`` and the blob's size ``total``.  Mirrors ``mdx_k_libsort_layout``
    and ``mdx_k_libsort_bytes`` (csrc/mdx_libsort.hip): a 16-byte header (``bad`` and a spare word), ``lib_start``, the
    per-record columns with room for n + 16 entries each, ``cigar`` with room for n_cigar + 16 words, ``seq``; every part
    begins on a multiple of 16 bytes, and 256 spare bytes follow the last."""
    n1 = max(n, 0) + 16
    out = {"bad": 0, "lib_start": 16}
    p = 16 + _align16((nlib + 1) * 4)
    for name, dtype in _PARTS:
        out[name] = p
        p += _align16(n1 * np.dtype(dtype).itemsize)
    out["cigar"] = p
    p += _align16((n_cigar + 16) * 4)
    out["seq"] = p
    out["seq_bytes"] = (n_bases + 1) // 2 + 64
    out["total"] = p + _align16(out["seq_bytes"]) + 256
    return out


def d2h(ptr, n, dtype):
    """n elements at device address ``ptr`` (hipMemcpy through the HIP runtime the library itself is linked to)."""
    out = np.empty(n, dtype)
    if n:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0        # hipMemcpyDeviceToHost
    return out


def read_blob(ptr, n, n_cigar, n_bases, nlib):
    """The blob at device address ``ptr`` in one copy, split by ``layout``: bad (int), lib_start [nlib + 1], the
    per-record columns [n + 16], cigar [n_cigar + 16], seq [seq_bytes]."""
    lay = layout(n, n_cigar, n_bases, nlib)
    raw = d2h(ptr, lay["total"], np.uint8)

    def part(name, dtype, count):
        return raw[lay[name]:lay[name] + count * np.dtype(dtype).itemsize].view(dtype)

    out = dict(bad=int(part("bad", np.uint64, 1)[0]), lib_start=part("lib_start", np.uint32, nlib + 1),
               cigar=part("cigar", np.uint32, n_cigar + 16), seq=part("seq", np.uint8, lay["seq_bytes"]),
               seq_bytes=lay["seq_bytes"])
    for name, dtype in _PARTS:
        out[name] = part(name, dtype, n + 16)
    return out
