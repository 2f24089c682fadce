"""SAM / BAM decoding and encoding without pysam (pysam is absent from this image).

Produces the SoA ``ReadBatch`` columns of the boundary directly.  Text SAM and BGZF-compressed
BAM (through the standard library's zlib) are supported for reading and writing; this is the
host-side "N1" row of SURVEY §8f in its first, pure-Python form.
"""

import ctypes
import dataclasses
import gzip
import io
import re
import struct
import zlib

import numpy as np

from . import layout as L
from .batch import ReadBatch

_SEQ_DECODE = np.frombuffer(b"=ACMGRSVTWYHKDBN", dtype=np.uint8)
_SEQ_ENCODE = np.full(256, 15, np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    _SEQ_ENCODE[_c] = _i
    _SEQ_ENCODE[ord(chr(_c).lower())] = _i


def usable_cpus():
    """CPUs this process may keep busy: its affinity mask, cut down to what the control group grants (``cpu.max``: a pod
    with 256 hardware threads and 16 CPUs' worth of quota stalls for most of every period under 64 busy threads;
    ``MDX_CPU_MAX_FILE`` names a stand-in for the tests) and divided by the ranks of this node (``LOCAL_WORLD_SIZE``, as
    torchrun sets it: one process per GPU, SURVEY 8e, and all of them decode at the same time).  The same rule as the
    library's own pool (include/mdx.h ``mdx_host_threads``)."""
    import os
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open(os.environ.get("MDX_CPU_MAX_FILE") or "/sys/fs/cgroup/cpu.max") as fh:
            quota, period = fh.read().split()[:2]
        if quota != "max" and int(period) > 0:
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    try:
        ranks = int(os.environ.get("LOCAL_WORLD_SIZE", "1"))
    except ValueError:
        ranks = 1
    if ranks > 1:
        n //= ranks
    return max(1, n)


class BAMError(RuntimeError):
    """Read-group problems (mapdamage/reader.py:16-17)."""


FILTER_REASONS = ("require-flags", "exclude-flags", "min-mapq", "min-read-length", "max-read-length")


@dataclasses.dataclass(frozen=True)
class RecordFilter:
    """The record filters of the command line (--min-mapq, --require-flags, --exclude-flags, --min-read-length,
    --max-read-length; include/mdx.h ``mdx_record_filter``).  A record is dropped when ``(FLAG & require_flags) !=
    require_flags``, ``(FLAG & exclude_flags) != 0``, ``MAPQ < min_mapq`` (numeric, as ``samtools view -q``: 255 passes),
    ``l_seq < min_length`` or — ``max_length`` not 0 — ``l_seq > max_length``; FLAG is the 16 bits of the file, ``l_seq`` the
    length of the SEQ field (0 for a SAM ``*``), not the CIGAR's query length.  Every decoder marks a dropped record with
    0x200 in its flag column, which the flag filter (0xF04) drops: nothing downstream knows about filters."""
    min_mapq: int = 0
    require_flags: int = 0
    exclude_flags: int = 0
    min_length: int = 0
    max_length: int = 0

    def __post_init__(self):
        if not 0 <= self.min_mapq <= 255:
            raise ValueError("min_mapq must lie in 0..255")
        if not (0 <= self.require_flags <= 0xFFFF and 0 <= self.exclude_flags <= 0xFFFF):
            raise ValueError("flag masks must lie in 0..65535")
        if self.min_length < 0 or self.max_length < 0 or self.min_length >= 1 << 31 or self.max_length >= 1 << 31:
            raise ValueError("read lengths must lie in 0..2^31-1")
        if self.max_length and self.min_length > self.max_length:
            raise ValueError("min_length is greater than max_length")

    @property
    def active(self):
        return bool(self.min_mapq or self.require_flags or self.exclude_flags or self.min_length or self.max_length)

    def drops(self, flag, mapq, l_seq):
        """The reason index (``FILTER_REASONS``) of each record that leaves — the first in the order require, exclude, MAPQ,
        shortest, longest — or -1, over numpy arrays of the file's FLAG (16 bits), MAPQ and SEQ length."""
        flag = np.asarray(flag).astype(np.int64) & 0xFFFF
        mapq = np.asarray(mapq).astype(np.int64)
        l_seq = np.asarray(l_seq).astype(np.int64)
        out = np.full(flag.shape, -1, np.int64)
        tests = ((flag & self.require_flags) != self.require_flags, (flag & self.exclude_flags) != 0, mapq < self.min_mapq,
                 l_seq < self.min_length, (l_seq > self.max_length) if self.max_length else np.zeros(flag.shape, bool))
        for reason in range(4, -1, -1):
            out[tests[reason]] = reason
        return out

    def as_struct(self):
        """The ctypes mirror of ``mdx_record_filter``."""
        return MdxRecordFilter(self.min_mapq, self.require_flags, self.exclude_flags, self.min_length, self.max_length)

    @staticmethod
    def counts_of(why):
        """(records, dropped by each reason) of the reason indices ``drops`` returned, as the decoders count: uint64[6]."""
        return np.concatenate([[why.shape[0]], np.bincount(why[why >= 0], minlength=5)]).astype(np.uint64)

    def counts(self, flag, mapq, l_seq):
        return self.counts_of(self.drops(flag, mapq, l_seq))


class MdxRecordFilter(ctypes.Structure):
    _fields_ = [("min_mapq", ctypes.c_int32), ("require_flags", ctypes.c_uint32), ("exclude_flags", ctypes.c_uint32),
                ("min_length", ctypes.c_int32), ("max_length", ctypes.c_int32)]


_MAPQ = re.compile(r"-?[0-9]+", re.ASCII)


def _mark_dropped(al, record_filter, flags16, mapqs):
    """The Python parsers' share of ``RecordFilter``: 0x200 into the flag column, and ``al.filter_counts``."""
    lens = np.diff(al.batch.seq_off.astype(np.int64))
    why = record_filter.drops(flags16, mapqs, lens)
    al.batch.flag[why >= 0] |= 0x200
    al.filter_counts = record_filter.counts_of(why)
    return al


class Header:
    def __init__(self, text=""):
        self.text = text
        self.references, self.lengths, self.read_groups = [], [], []
        for line in text.splitlines():
            fields = line.split("\t")
            tags = dict(f.split(":", 1) for f in fields[1:] if ":" in f)
            if fields[0] == "@SQ":
                self.references.append(tags["SN"])
                self.lengths.append(int(tags["LN"]))
            elif fields[0] == "@RG":
                self.read_groups.append(tags)

    def get(self, key, default=()):
        return self.read_groups if key == "RG" else default


class Alignments:
    """All records of a SAM/BAM file: header + SoA batch + per-record RG id and query name.
    ``raw`` (BAM only, ``keep_raw=True``): the record bodies as stored, and ``raw_header`` the bytes
    in front of the first record, so that a rewritten file keeps every field it does not touch."""

    def __init__(self, header, batch, rg, qname):
        self.header, self.batch, self._rg, self._qname = header, batch, rg, qname
        self.raw, self.raw_header, self.has_mr = None, None, None
        # native decoder: per-record read-group index (-1 = no RG tag) into rg_names, and the query names as one
        # blob + offsets; the Python lists are only built when somebody asks for them
        self.rg_index, self.rg_names, self._qblob, self._qoff = None, None, None, None

    @property
    def rg(self):
        if self._rg is None:
            names = self.rg_names
            self._rg = [names[i] if i >= 0 else None for i in self.rg_index.tolist()]
        return self._rg

    @rg.setter
    def rg(self, value):
        self._rg = value

    @property
    def qname(self):
        if self._qname is None:
            blob, off = bytes(self._qblob), self._qoff.tolist()
            self._qname = [blob[off[i]:off[i + 1]].decode() for i in range(len(off) - 1)]
        return self._qname

    @qname.setter
    def qname(self, value):
        self._qname = value

    def qname_at(self, i):
        if self._qname is not None:
            return self._qname[i]
        return bytes(self._qblob[int(self._qoff[i]):int(self._qoff[i + 1])]).decode()


def _finish(header, flags, tids, poss, tlens, cigs, cig_counts, seqs, quals, rgs, qnames):
    n = len(flags)
    cigar_off = np.zeros(n + 1, np.uint32)
    np.cumsum(np.asarray(cig_counts, dtype=np.int64), out=cigar_off[1:])
    seq_off = np.zeros(n + 1, np.uint32)
    np.cumsum(np.asarray([len(s) for s in seqs], dtype=np.int64), out=seq_off[1:])
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    qual = np.frombuffer(b"".join(quals), dtype=np.uint8).copy()
    batch = ReadBatch(np.asarray(flags, np.uint16), np.zeros(n, np.uint16), np.asarray(tids, np.int32),
                      np.asarray(poss, np.int32), np.asarray(tlens, np.int32), cigar_off,
                      np.asarray(cigs, np.uint32), seq_off, seq, qual).validate()
    return Alignments(header, batch, rgs, qnames)


def read_sam(path_or_handle, header=None, record_filter=None):
    """SAM text -> ``Alignments``.  ``header``: a ``Header`` read already (a host parser that takes a stream up behind the
    device decoder, ``GpuSamStream.tell``): every line is then a record line, and a line that starts with '@' is skipped.
    ``record_filter`` (a ``RecordFilter``): the records it drops get 0x200 in the flag column, ``filter_counts`` on the
    result; MAPQ is read only under a MAPQ threshold, and one that is not ``-?[0-9]+`` is then a ``BAMError``."""
    handle = open(path_or_handle, "rt") if isinstance(path_or_handle, (str, bytes)) or hasattr(path_or_handle, "__fspath__") else path_or_handle
    head, lines = [], []
    for line in handle:
        (head if line.startswith("@") else lines).append(line)
    if header is None:
        header = Header("".join(head))
    tid_of = {name: i for i, name in enumerate(header.references)}
    flags, tids, poss, tlens, cigs, cig_counts, seqs, quals, rgs, qnames = [], [], [], [], [], [], [], [], [], []
    filtering = record_filter is not None and record_filter.active
    want_mapq = filtering and record_filter.min_mapq > 0
    flags16, mapqs = [], []
    for line in lines:
        f = line.rstrip("\n").split("\t")
        if len(f) < 11:
            continue
        qnames.append(f[0])
        if filtering:
            flags16.append(int(f[1]))
            if want_mapq:
                # (-?[0-9]+, compared as a number whatever its size; anything else — int() would take "+5", " 7", "1_0" — is a
                # line htslib, behind the reference's pysam, refuses)
                if not _MAPQ.fullmatch(f[4]):
                    raise BAMError("Read %r: MAPQ %r is not a number" % (f[0], f[4]))
                mapqs.append(int(f[4]))
        flags.append(int(f[1]) & 0x3FFF)       # bits 14 and 15 are the kernels' hint bits (mdx.h MDX_FLAG_HAS_QUAL / _QUAL_ABOVE_MIN), never the file's
        tids.append(tid_of.get(f[2], -1))
        poss.append(int(f[3]) - 1)
        tlens.append(int(f[8]))
        n_ops, num = 0, 0
        if f[5] != "*":
            for ch in f[5]:
                if ch.isdigit():
                    num = num * 10 + ord(ch) - 48
                else:
                    cigs.append((num << 4) | L.CIGAR_CHARS.index(ch))
                    n_ops += 1
                    num = 0
        cig_counts.append(n_ops)
        s = b"" if f[9] == "*" else f[9].upper().encode()
        # htslib stores SEQ through the 4-bit alphabet: anything else becomes N
        s = bytes(_SEQ_DECODE[_SEQ_ENCODE[np.frombuffer(s, dtype=np.uint8)]])
        seqs.append(s)
        if f[10] == "*":
            quals.append(b"\xff" * len(s))
        else:
            quals.append(bytes((np.frombuffer(f[10].encode(), dtype=np.uint8) - 33).astype(np.uint8)))
        rg = None
        for tag in f[11:]:
            if tag.startswith("RG:Z:"):
                rg = tag[5:]
        rgs.append(rg)
    al = _finish(header, flags, tids, poss, tlens, cigs, cig_counts, seqs, quals, rgs, qnames)
    if filtering:
        _mark_dropped(al, record_filter, flags16, mapqs if want_mapq else np.zeros(len(flags16), np.int64))
    return al


def read_bam(path, keep_raw=False, record_filter=None):
    with gzip.open(path, "rb") as handle:   # BGZF is a series of gzip members
        data = handle.read()
    if data[:4] != b"BAM\x01":
        raise ValueError("%r is not a BAM file" % (path,))
    l_text, = struct.unpack_from("<i", data, 4)
    text = data[8:8 + l_text].split(b"\x00")[0].decode()
    off = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, off)
    off += 4
    names, lengths = [], []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, off)
        names.append(data[off + 4:off + 4 + l_name - 1].decode())
        l_ref, = struct.unpack_from("<i", data, off + 4 + l_name)
        lengths.append(l_ref)
        off += 8 + l_name
    header = Header(text)
    if not header.references:
        header.references, header.lengths = names, lengths
    flags, tids, poss, tlens, cigs, cig_counts, seqs, quals, rgs, qnames = [], [], [], [], [], [], [], [], [], []
    mtids, mposs, raws, has_mr = [], [], [], []
    flags16, mapqs = [], []
    raw_header = data[:off]
    n = len(data)
    while off + 4 <= n:
        block_size, = struct.unpack_from("<i", data, off)
        rec = memoryview(data)[off + 4:off + 4 + block_size]
        off += 4 + block_size
        tid, pos, l_read_name, mapq, _bin, n_cigar, flag, l_seq, ntid, npos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 0)
        flags16.append(flag)
        mapqs.append(mapq)
        mtids.append(ntid)
        mposs.append(npos)
        if keep_raw:
            raws.append(bytes(rec))
        p = 32
        qnames.append(bytes(rec[p:p + l_read_name - 1]).decode())
        p += l_read_name
        cig = np.frombuffer(rec[p:p + 4 * n_cigar], dtype="<u4")
        p += 4 * n_cigar
        packed = np.frombuffer(rec[p:p + (l_seq + 1) // 2], dtype=np.uint8)
        p += (l_seq + 1) // 2
        nib = np.empty(packed.shape[0] * 2, np.uint8)
        nib[0::2] = packed >> 4
        nib[1::2] = packed & 15
        seqs.append(bytes(_SEQ_DECODE[nib[:l_seq]]))
        quals.append(bytes(rec[p:p + l_seq]))
        p += l_seq
        rg = None
        aux = bytes(rec[p:])
        has_mr.append(False)
        q = 0
        while q + 3 <= len(aux):
            tag, typ = aux[q:q + 2], aux[q + 2:q + 3]
            q += 3
            if tag == b"MR":
                has_mr[-1:] = [True]
            if typ == b"Z" or typ == b"H":
                end = aux.index(b"\x00", q)
                if tag == b"RG":
                    rg = aux[q:end].decode()
                q = end + 1
            elif typ in b"AcC":
                q += 1
            elif typ in b"sS":
                q += 2
            elif typ in b"iIf":
                q += 4
            elif typ == b"B":
                sub = aux[q:q + 1]
                cnt, = struct.unpack_from("<i", aux, q + 1)
                if (tag == b"CG" and sub == b"I" and n_cigar == 2 and int(cig[0]) == ((l_seq << 4) | 4) and (int(cig[1]) & 15) == 3):
                    # SAMv1 4.2.2: a CIGAR of more than 65 535 operations lives here, the field holds <l_seq>S<n>N (htslib
                    # puts it back behind the reference's pysam)
                    cig = np.frombuffer(aux[q + 5:q + 5 + 4 * cnt], dtype="<u4")
                    n_cigar = cnt
                q += 5 + cnt * {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}[sub]
            else:
                break
        flags.append(flag & 0x3FFF); tids.append(tid); poss.append(pos); tlens.append(tlen)
        cigs.extend(int(c) for c in cig)
        cig_counts.append(n_cigar)
        rgs.append(rg)
    al = _finish(header, flags, tids, poss, tlens, cigs, cig_counts, seqs, quals, rgs, qnames)
    al.batch.mtid = np.asarray(mtids, np.int32)
    al.batch.mpos = np.asarray(mposs, np.int32)
    al.has_mr = has_mr
    if keep_raw:
        al.raw, al.raw_header = raws, raw_header
    if record_filter is not None and record_filter.active:
        _mark_dropped(al, record_filter, flags16, mapqs)
    return al


def apply_record_filter(al, record_filter, counts=None):
    """``RecordFilter`` over the ``Alignments`` of the native host decoder (include/mdx.h ``mdx_bam_apply_record_filter``): 0x200
    into the flag column of the records it drops; ``counts`` (uint64[6]) += records, dropped by each reason."""
    import ctypes

    from .engine import load_library
    if counts is None:
        counts = np.zeros(6, np.uint64)
    flt = record_filter.as_struct() if record_filter is not None else None
    rc = load_library().mdx_bam_apply_record_filter(al.native, ctypes.byref(flt) if flt is not None else None,
                                                    ctypes.c_void_p(counts.ctypes.data))
    if rc != 0:
        raise ValueError("mdx_bam_apply_record_filter failed (%d)" % rc)
    return counts


def write_bam_raw(path, raw_header, records):
    """BGZF-compress an already encoded BAM stream (header bytes + record bodies)."""
    data = bytearray(raw_header)
    for body in records:
        data += struct.pack("<i", len(body)) + body
    data = bytes(data)
    with open(path, "wb") as out:
        for lo in range(0, len(data), 0xFF00):
            out.write(_bgzf_block(data[lo:lo + 0xFF00]))
        out.write(_bgzf_block(b""))


class BgzfWriter:
    """BGZF output stream: 0xFF00-byte blocks deflated on a pool of threads (zlib drops the GIL), written in order.  ``write``
    hands its blocks to the pool and returns: they are deflated while the caller prepares the next piece (the rescaling pass:
    the next chunk's decode, kernels and patching run under the deflate of this one's output, which is what bounds it), at most
    ``max_pending`` blocks — 256 MiB of input — wait at a time."""

    def __init__(self, path, threads=None, max_pending=4096, engine=None):
        """``engine`` (a ``DamageEngine``): the members are made on its device instead (include/mdx.h ``mdx_bgzf_deflate``: a lane
        per quarter of a member, 2.9 GB/s against 0.6 on sixteen threads; 3 % larger than zlib's level 6) — every ``write`` is
        then compressed on its own, its last member as short as it comes."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        self._out = open(path, "wb")
        self._engine = engine
        # (engine: one thread writes the finished members to the file, in order, while the next piece is compressed)
        self._pool = ThreadPoolExecutor(1) if engine is not None else ThreadPoolExecutor(threads or min(32, usable_cpus()))
        self._tail = b""
        self._pending = deque()
        self._max_pending = max_pending
        # (engine: the members' bytes handed to the file so far, whether its thread has written them or not — where the
        # next ``write_members`` will lie in the file)
        self.bytes_handed = 0

    def _drain(self, keep):
        """Write the finished blocks at the head of the queue; wait for the oldest ones while more than ``keep`` are queued."""
        if self._engine is not None:
            while len(self._pending) > keep:
                self._pending.popleft().result()
            return
        while self._pending and (len(self._pending) > keep or self._pending[0].done()):
            self._out.write(self._pending.popleft().result())

    def write(self, data):
        """Append bytes (anything with the buffer protocol; the object must not change until the stream is closed or flushed)."""
        view = memoryview(data).cast("B")
        if self._engine is not None:
            if len(view):
                members = self._engine.bgzf_deflate(view)
                self.bytes_handed += len(memoryview(members.data).cast("B"))
                self._pending.append(self._pool.submit(self._out.write, members.data))
                while len(self._pending) > 2:           # (two pieces' members waiting for the disk at most)
                    self._pending.popleft().result()
            return
        if self._tail:
            view = memoryview(self._tail + view.tobytes())
        whole = len(view) // 0xFF00 * 0xFF00
        self._tail = view[whole:].tobytes()
        for lo in range(0, whole, 0xFF00):
            self._pending.append(self._pool.submit(_bgzf_block, view[lo:lo + 0xFF00]))
            if len(self._pending) > self._max_pending:
                self._drain(self._max_pending // 2)
        self._drain(self._max_pending)

    def write_members(self, members):
        """Append finished BGZF members (the device's: ``GpuBamStream.rescale_slab``) as they are."""
        assert not self._tail
        self.bytes_handed += len(memoryview(members).cast("B"))
        self._pending.append(self._pool.submit(self._out.write, memoryview(members)))
        while len(self._pending) > 2:
            self._pending.popleft().result()

    def flush(self):
        self._drain(0)

    def close(self):
        if self._out is None:
            return
        self._drain(0)
        if self._tail:
            self._out.write(_bgzf_block(self._tail))
        self._out.write(_bgzf_block(b""))
        self._out.close()
        self._out = None
        self._pool.shutdown()

    def abandon(self):
        """Close the file as it stands — no tail, no end-of-file marker, whatever the writes still queued come to: the
        caller removes it (--write-kept on an error path)."""
        if self._out is None:
            return
        self._pool.shutdown(wait=True)
        self._pending.clear()
        try:
            self._out.close()
        finally:
            self._out = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def bam_header_bytes(header):
    """The uncompressed BAM header block (magic, text, reference dictionary) of a parsed ``Header``."""
    text = header.text.encode()
    out = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(header.references)))
    for name, length in zip(header.references, header.lengths):
        raw = name.encode() + b"\0"
        out += struct.pack("<i", len(raw)) + raw + struct.pack("<i", int(length))
    return bytes(out)


class _NativeBam:
    """Owner of a decoded BAM inside libmdx.so (``mdx_bam_free`` when the last array viewing it is gone)."""

    def __init__(self, lib, handle):
        self._lib, self._handle = lib, handle

    def __del__(self):
        if self._handle:
            self._lib.mdx_bam_free(self._handle)
            self._handle = None


def _native_header(lib, handle):
    header = Header(lib.mdx_bam_header_text(handle).decode())
    n_ref = lib.mdx_bam_n_ref(handle)
    if not header.references:
        header.references = [lib.mdx_bam_ref_name(handle, i).decode() for i in range(n_ref)]
        header.lengths = [int(lib.mdx_bam_ref_length(handle, i)) for i in range(n_ref)]
    return header


def _native_alignments(lib, handle, owner, header=None):
    """``Alignments`` over the columns of a decoded ``mdx_bam`` (numpy views, no copy; every view keeps
    ``owner`` and with it the decoder's buffers alive)."""
    import ctypes

    from .engine import MdxBatch
    if header is None:
        header = _native_header(lib, handle)
    view = MdxBatch()
    mtid, mpos, rgi, hmr = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    lib.mdx_bam_batch(handle, ctypes.byref(view), ctypes.byref(mtid), ctypes.byref(mpos), ctypes.byref(rgi),
                      ctypes.byref(hmr))
    n, nb, nc = view.n_reads, view.n_bases, view.n_cigar

    def col(ptr, count, dtype):
        if count == 0 or not ptr:
            return np.zeros(0, dtype)
        raw = (ctypes.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr)
        raw._owner = owner          # the view (and every view of it) keeps the decoder's buffers alive
        return np.frombuffer(raw, dtype=dtype)

    batch = ReadBatch(col(view.flag, n, np.uint16), col(view.lib, n, np.uint16), col(view.tid, n, np.int32),
                      col(view.pos, n, np.int32), col(view.tlen, n, np.int32),
                      col(view.cigar_off, n + 1, np.uint32) if n else np.zeros(1, np.uint32),
                      col(view.cigar, nc, np.uint32),
                      col(view.seq_off, n + 1, np.uint32) if n else np.zeros(1, np.uint32),
                      col(view.seq, nb, np.uint8), col(view.qual, nb, np.uint8),
                      col(mtid.value, n, np.int32), col(mpos.value, n, np.int32)).validate()
    al = Alignments(header, batch, None, None)
    al.rg_names = [lib.mdx_bam_rg_name(handle, i).decode() for i in range(lib.mdx_bam_n_rg(handle))]
    al.rg_index = col(rgi.value, n, np.int32)
    offs = ctypes.c_void_p()
    blob_ptr = lib.mdx_bam_qnames(handle, ctypes.byref(offs))
    al._qoff = col(offs.value, n + 1, np.uint32) if n else np.zeros(1, np.uint32)
    al._qblob = col(blob_ptr, int(al._qoff[-1]), np.uint8) if n else np.zeros(0, np.uint8)
    al.has_mr = col(hmr.value, n, np.uint8).view(bool)
    al.qmin = col(lib.mdx_bam_qmin(handle), n, np.uint8)     # lowest quality of each record
    al.native, al._native_owner = handle, owner              # (apply_record_filter, patch_rescaled)
    return al


def read_bam_native(path, threads=None):
    """BAM -> ``Alignments`` through the C++ decoder of libmdx.so (multi-threaded BGZF inflate,
    records unpacked straight into the SoA columns; include/mdx.h ``mdx_bam_*``).  The columns are numpy
    views of the decoder's buffers (no copy); every view keeps the decoder alive."""
    import ctypes
    import os

    from .engine import MdxBatch, load_library
    lib = load_library()
    handle = ctypes.c_void_p()
    if isinstance(path, Source):
        # (a stream is read to its end: memory in proportion to it — what reservoir sampling, -n N, needs anyway)
        rc = lib.mdx_bam_read_source(path.handle, ctypes.c_int(threads or min(64, usable_cpus())), ctypes.byref(handle))
    else:
        rc = lib.mdx_bam_read(str(path).encode(), ctypes.c_int(threads or min(64, usable_cpus())),
                              ctypes.byref(handle))
    owner = _NativeBam(lib, handle)
    if rc != 0:
        raise ValueError("%r: %s" % (str(path), lib.mdx_bam_error(handle).decode() if handle else "BAM decode failed"))
    return _native_alignments(lib, handle, owner)


class GpuBamStream:
    """GPU-side decode of a BAM file (include/mdx.h ``mdx_gbam_*``): the compressed file goes to HBM a slab of BGZF
    blocks at a time and is inflated and unpacked there; ``next_view`` returns an ``MdxBatch`` of DEVICE pointers for
    ``DamageEngine.tabulate_view`` (valid until the next call), or None at the end of the file.  ``readgroups``: the
    header's read-group ids with the library index of each; ``lib_default``: library of a record without RG tag
    (None: such a record is an error when it is counted).  Any BGZF layout: records may straddle blocks and slabs, the
    header may share a block with records.  Raises ``GpuDecodeUnsupported`` for what is left (a record longer than a
    gigabyte; in a sharded run a slab whose first record cannot be told without the slab in front) — the caller then
    decodes on the host (``BamStream``), from ``tell()`` on if it likes.  ``path``: a file's, or a ``Source``."""

    def __init__(self, engine, path, readgroups=(), lib_default=None, chunk_bytes=256 << 20, want_qual=False,
                 want_mate=False, min_basequal=0, packed=None, record_filter=None):
        import ctypes
        self._lib = engine._lib
        self._engine = engine
        self._g = ctypes.c_void_p()
        self.path, self.chunk_bytes = path, int(chunk_bytes)
        if not engine._ctx:
            raise ValueError("the engine is closed")
        if isinstance(path, Source):
            rc = self._lib.mdx_gbam_open_source(engine._ctx, path.handle, ctypes.byref(self._g))
        else:
            rc = self._lib.mdx_gbam_open(engine._ctx, str(path).encode(), ctypes.byref(self._g))
        # (the engine closes the streams still open on it before it destroys its context: DamageEngine.close)
        if not hasattr(engine, "_streams"):
            import weakref
            engine._streams = weakref.WeakSet()
        engine._streams.add(self)
        if rc != 0:
            message = self._error()
            self.close()
            if rc == -8:
                raise GpuDecodeUnsupported("%r: %s" % (str(path), message))
            raise ValueError("%r: %s" % (str(path), message))
        self.header = _native_header(self._lib, self._lib.mdx_gbam_header(self._g))
        ids = [str(rg).encode() for rg, _ in readgroups]
        arr = (ctypes.c_char_p * max(1, len(ids)))(*ids)
        libs = (ctypes.c_int32 * max(1, len(ids)))(*[int(lib) for _, lib in readgroups])
        rc = self._lib.mdx_gbam_configure(self._g, len(ids), arr, libs, -1 if lib_default is None else int(lib_default),
                                          int(bool(want_qual)), int(bool(want_mate)))
        if rc != 0:
            raise ValueError("%r: %s" % (str(path), self._error()))
        if min_basequal:
            # --min-basequal: unmaskable records are flagged on the device, see ``missing_qualities``
            if self._lib.mdx_gbam_set_min_basequal(self._g, int(min_basequal)) != 0:
                raise ValueError("%r: %s" % (str(path), self._error()))
        # the SEQ column of the views: BAM's nibbles kept as nibbles (MDX_SEQ_4BIT: the packed kernel — with --min-basequal
        # its masked form — reads them) unless the launches behind it read ASCII anyway (the rescale kernels of
        # --rescale-only want the qualities without a threshold); ``packed`` overrides the choice
        if packed is None:
            packed = bool(min_basequal) or not want_qual
        self.packed = bool(packed)
        if self.packed:
            self._lib.mdx_gbam_set_seq_format(self._g, 1)
        if record_filter is not None and record_filter.active:
            flt = record_filter.as_struct()
            if self._lib.mdx_gbam_set_record_filter(self._g, ctypes.byref(flt)) != 0:
                raise ValueError("%r: %s" % (str(path), self._error()))

    def filter_counts(self):
        """uint64[6]: the records decoded so far, and those among them the record filter dropped, by reason."""
        import ctypes
        out = np.zeros(6, np.uint64)
        if self._lib.mdx_gbam_filter_counts(self._g, ctypes.c_void_p(out.ctypes.data)) != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        return out

    def missing_qualities(self):
        """A record the kernel counts has come by without qualities (main.py:185-192 warns once)."""
        return bool(self._lib.mdx_gbam_missing_qualities(self._g))

    def _error(self):
        return self._lib.mdx_gbam_error(self._g).decode() if self._g else "GPU BAM decode failed"

    def next_view(self):
        import ctypes
        from .engine import MdxBatch
        view = MdxBatch()
        mtid, mpos = ctypes.c_void_p(), ctypes.c_void_p()
        rc = self._lib.mdx_gbam_next(self._g, self.chunk_bytes, ctypes.byref(view), ctypes.byref(mtid), ctypes.byref(mpos))
        if rc == -8:
            raise GpuDecodeUnsupported("%r: %s" % (str(self.path), self._error()))
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        if view.n_reads == 0 and self._lib.mdx_gbam_at_end(self._g):
            return None
        view.mtid, view.mpos = mtid.value, mpos.value       # (python attributes: not fields of the C struct)
        return view

    def tell(self):
        """(compressed offset of the next slab's first BGZF block, inflated bytes in front of its first record) — where
        ``BamStream.seek`` takes up the file — or None when the device path does not know (behind ``skip``)."""
        import ctypes
        coff, phase = ctypes.c_int64(), ctypes.c_int64()
        if self._lib.mdx_gbam_tell(self._g, ctypes.byref(coff), ctypes.byref(phase)) != 0:
            return None
        return coff.value, phase.value

    def view_flags(self, view):
        """The flag column of the view ``next_view`` handed out last, on the host (--downsample on the device path:
        reader.py:134-146 draws once per record the flag filter keeps, in file order)."""
        import ctypes
        import numpy as np
        n = int(view.n_reads)
        out = np.empty(n, np.uint16)
        self._lib.mdx_gbam_view_flags.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        rc = self._lib.mdx_gbam_view_flags(self._g, ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(n))
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        return out

    def set_view_flags(self, view, flags):
        """... and back: the caller has marked the records that leave (a bit the flag filter drops)."""
        import ctypes
        import numpy as np
        flags = np.ascontiguousarray(flags, dtype=np.uint16)
        assert flags.shape[0] == int(view.n_reads)
        self._lib.mdx_gbam_view_set_flags.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
        rc = self._lib.mdx_gbam_view_set_flags(self._g, ctypes.c_void_p(flags.ctypes.data), ctypes.c_int64(flags.shape[0]))
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))

    def rescale_slab(self, view, counts):
        """The slab ``next_view`` handed out last (a stream opened with ``want_qual``, ``want_mate``, ``packed=False``) rescaled
        through the engine's model and written back on the device (include/mdx.h ``mdx_gbam_rescale_slab``): returns the slab's
        records — new qualities, ``MR:f`` tags — as BGZF members (a uint8 array); ``counts`` (int64[5]) += records by routing
        status.  Raises SystemExit with the reference's message when a record to be rescaled has an MR tag already
        (rescale.py:277-278), BadReadError for a record the kernels cannot process."""
        import ctypes
        import numpy as np
        # (the bound include/mdx.h states for ``out``: the inflated bytes of the view's records, from the chain of their offsets,
        # seven more for every record of the view, 64 per member — ``mdx_gbam_kept_bound_tagged``, never a guess)
        bound = ctypes.c_int64(0)
        fn = self._lib.mdx_gbam_kept_bound_tagged
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p], ctypes.c_int
        if fn(self._g, ctypes.c_int32(7), ctypes.byref(bound)) != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        cap = int(bound.value)
        out = np.empty(cap, np.uint8)
        out_len, clash = ctypes.c_int64(0), ctypes.c_int64(-1)
        fn = self._lib.mdx_gbam_rescale_slab
        fn.restype = ctypes.c_int
        rc = fn(self._g, ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(cap), ctypes.byref(out_len),
                ctypes.c_void_p(counts.ctypes.data), ctypes.byref(clash))
        if rc == -6 and clash.value >= 0:
            name = ctypes.create_string_buffer(256)
            self._lib.mdx_gbam_record_name(self._g, ctypes.c_int64(clash.value), name, 256)
            raise SystemExit("Read: %s already has a MR tag, can't rescale" % name.value.decode(errors="replace"))
        if rc == -6:
            from .engine import BadReadError
            raise BadReadError(-2 - clash.value, self._error())
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        return out[:out_len.value]

    def kept_bound(self, group_tag=None, score_tag=None, calmd=None):
        """Bytes that always suffice for the members ``write_kept`` makes of the view handed out last (include/mdx.h
        ``mdx_gbam_kept_bound``: from the view's record offsets, never a guess) — with the tags' 5 and 7 bytes for every record
        of the view where they are asked for (``mdx_gbam_kept_bound_tagged``), and with what recomputing NM and MD can add
        (``mdx_gbam_kept_bound_md``) where ``calmd`` is true; ``None``: as ``set_kept_md`` left the stream."""
        import ctypes
        tag_bytes = (5 if group_tag is not None else 0) + (7 if score_tag is not None else 0)
        bound = ctypes.c_int64(0)
        if getattr(self, "_kept_md", False) if calmd is None else calmd:
            fn = self._lib.mdx_gbam_kept_bound_md
            fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p], ctypes.c_int
            rc = fn(self._g, ctypes.c_int32(tag_bytes), ctypes.c_int32(1), ctypes.byref(bound))
        elif tag_bytes:
            fn = self._lib.mdx_gbam_kept_bound_tagged
            fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p], ctypes.c_int
            rc = fn(self._g, ctypes.c_int32(tag_bytes), ctypes.byref(bound))
        else:
            fn = self._lib.mdx_gbam_kept_bound
            fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
            rc = fn(self._g, ctypes.byref(bound))
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        return int(bound.value)

    def write_kept(self, view, groups=None, n_groups=0, group_tag=None, score_tag=None):
        """The records of the view ``next_view`` handed out last that the run counts — ``(flag & 0xF04) == 0`` in the flag column
        as it stands, so behind ``set_view_flags`` — selected, compacted and compressed on the device (include/mdx.h
        ``mdx_gbam_write_kept``): returns ``(members, n_written, raw_bytes)``, the records byte for byte as BGZF members (a uint8
        array, valid until the next call: one output array, grown when ``kept_bound`` says so), their number and their bytes
        before compression.  ``groups``: indices of the groups of a stratified engine (``n_groups`` of them in all) whose records
        alone are written — behind ``DamageEngine.tabulate_view`` of this very view (MdxError -3 otherwise).
        ``group_tag`` / ``score_tag`` (two characters, ``[A-Za-z][A-Za-z0-9]``): every written record gets ``TAG:S``, its group
        among the engine's ``n_groups``, and ``TAG:f``, its PMD score (an engine with ``keep_pmd_scores``), appended
        (``mdx_gbam_write_kept_tagged``; behind ``tabulate_view`` of this very view as well).  A written record that has such
        a tag already: ``KeptTagClash`` with the record's index in the slab and its name; nothing of the slab is written."""
        import ctypes
        import numpy as np
        tags = []
        for tag in (group_tag, score_tag):
            if tag is not None and (len(tag) != 2 or not tag.isascii()):
                raise ValueError("a tag is two ASCII characters, not %r" % (tag,))
            tags.append(None if tag is None else tag.encode("ascii"))
        bound = self.kept_bound(group_tag, score_tag)
        out = getattr(self, "_kept_out", None)
        if out is None or out.shape[0] < bound:
            out = self._kept_out = np.empty(bound + bound // 8, np.uint8)
        selected = None
        if groups is not None:
            selected = np.zeros(max(1, int(n_groups)), np.uint8)
            for g in groups:
                if not 0 <= int(g) < int(n_groups):
                    raise ValueError("group %d is outside 0..%d" % (int(g), int(n_groups) - 1))
                selected[int(g)] = 1
        out_len, n_written, raw_bytes, clash = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(-1)
        sel = None if selected is None else ctypes.c_void_p(selected.ctypes.data)
        if tags[0] is None and tags[1] is None:
            fn = self._lib.mdx_gbam_write_kept
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                           ctypes.c_void_p, ctypes.c_void_p]
            fn.restype = ctypes.c_int
            rc = fn(self._g, sel, ctypes.c_int32(int(n_groups)), ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(out.shape[0]),
                    ctypes.byref(out_len), ctypes.byref(n_written), ctypes.byref(raw_bytes))
        else:
            fn = self._lib.mdx_gbam_write_kept_tagged
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p,
                           ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
            fn.restype = ctypes.c_int
            rc = fn(self._g, sel, ctypes.c_int32(int(n_groups)), tags[0], tags[1], ctypes.c_void_p(out.ctypes.data),
                    ctypes.c_int64(out.shape[0]), ctypes.byref(out_len), ctypes.byref(n_written), ctypes.byref(raw_bytes),
                    ctypes.byref(clash))
        if rc == -6 and clash.value >= 0:
            name = ctypes.create_string_buffer(256)
            self._lib.mdx_gbam_record_name(self._g, ctypes.c_int64(clash.value), name, 256)
            raise KeptTagClash(clash.value, name.value.decode(errors="replace"), [t for t in (group_tag, score_tag) if t is not None])
        if rc != 0:
            from .engine import MdxError
            raise MdxError(rc, "%r: %s" % (str(self.path), self._error()))
        return out[:out_len.value], int(n_written.value), int(raw_bytes.value)

    def set_kept_mask(self, k5, k3, what="all", single_stranded=False):
        """The mask of every later ``write_kept`` of this stream (include/mdx.h ``mdx_gbam_set_kept_mask``; the rule:
        csrc/mdx_kept_mask.h): the written records' bases inside the first ``k5`` query bases of the molecule's 5' end and the
        last ``k3`` of its 3' end (0..255 each) become N with quality 0 — ``what``: ``all`` of them, the ``transitions`` (T at
        the 5' end, A at the 3' end as the forward strand stores them; with ``single_stranded`` T at both), or those of them
        that are ``mismatches`` against the engine's reference (C under T, G under A).  ``k5 == k3 == 0`` clears the mask.
        Either way the counts start again at 0.  ValueError for an unknown ``what``, ``MdxError`` -1 for a value out of range."""
        import ctypes
        if what not in MASK_WHAT:
            raise ValueError("what is one of %s, not %r" % (", ".join(MASK_WHAT), what))
        fn = self._lib.mdx_gbam_set_kept_mask
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32], ctypes.c_int
        rc = fn(self._g, ctypes.c_int32(int(k5)), ctypes.c_int32(int(k3)), ctypes.c_int32(MASK_WHAT.index(what)),
                ctypes.c_int32(1 if single_stranded else 0))
        if rc != 0:
            from .engine import MdxError
            raise MdxError(rc, "%r: %s" % (str(self.path), self._error()))

    def kept_mask_counts(self):
        """``(records, bases)``: the written records with a masked base and the masked bases, summed over the ``write_kept``
        calls since ``set_kept_mask`` (``mdx_gbam_kept_mask_counts``)."""
        import ctypes
        fn = self._lib.mdx_gbam_kept_mask_counts
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
        records, bases = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = fn(self._g, ctypes.byref(records), ctypes.byref(bases))
        if rc != 0:
            from .engine import MdxError
            raise MdxError(rc, "%r: %s" % (str(self.path), self._error()))
        return int(records.value), int(bases.value)

    def set_kept_md(self, on=True):
        """Every later ``write_kept`` of this stream hands its records on with ``NM`` and ``MD`` recomputed against the
        engine's reference (include/mdx.h ``mdx_gbam_set_kept_md``; the rule: csrc/mdx_kept_md.h) — from the bytes the file will
        hold, so behind ``set_kept_mask`` and with the tags of ``write_kept`` in place; ``raw_bytes`` and ``kept_index`` are
        those of the new records.  ``on=False`` switches it off.  Either way the counts start again at 0.  A write on an
        engine without a reference is ``MdxError`` -3."""
        import ctypes
        fn = self._lib.mdx_gbam_set_kept_md
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int32], ctypes.c_int
        rc = fn(self._g, ctypes.c_int32(1 if on else 0))
        if rc != 0:
            from .engine import MdxError
            raise MdxError(rc, "%r: %s" % (str(self.path), self._error()))
        self._kept_md = bool(on)

    def kept_md_counts(self):
        """``(recomputed, skipped, had_tags)``: the written records whose ``NM`` and ``MD`` were recomputed, those left as they
        are, and those that had either tag, summed over the ``write_kept`` calls since ``set_kept_md``
        (``mdx_gbam_kept_md_counts``)."""
        import ctypes
        fn = self._lib.mdx_gbam_kept_md_counts
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
        out = (ctypes.c_uint64 * 3)()
        rc = fn(self._g, out)
        if rc != 0:
            from .engine import MdxError
            raise MdxError(rc, "%r: %s" % (str(self.path), self._error()))
        return int(out[0]), int(out[1]), int(out[2])

    def kept_index(self, stream_base, prev, n_written):
        """The index entries of the records the last ``write_kept`` of this view wrote (include/mdx.h ``mdx_gbam_kept_index``;
        the rule: csrc/mdx_kept_index.h): ``(runs, prev)`` — ``runs`` a ``bai.RUN_DTYPE`` array, the maximal runs of written
        records with the same (tid, bin) in file order, their bytes as offsets of the uncompressed stream, ``stream_base`` (the
        raw bytes of all earlier slabs) + the offset in this slab's; ``prev`` = ``(tid, pos)`` of the last written record in
        front of the slab (``(-1, -1)``: none), returned as this slab's last.  ``n_written``: what ``write_kept`` returned.  A
        written record out of coordinate order or outside its reference sequence: ``KeptIndexError`` with its index in the
        slab and its name.  ``MdxError`` -3 unless the call comes right behind ``write_kept`` of the view handed out last."""
        import ctypes
        from .bai import RUN_DTYPE
        runs = np.zeros(max(1, int(n_written)), RUN_DTYPE)
        tid, pos = ctypes.c_int32(int(prev[0])), ctypes.c_int32(int(prev[1]))
        n_runs, bad, reason = ctypes.c_int64(0), ctypes.c_int64(-1), ctypes.c_int32(0)
        fn = self._lib.mdx_gbam_kept_index
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        fn.restype = ctypes.c_int
        rc = fn(self._g, ctypes.c_int64(int(stream_base)), ctypes.byref(tid), ctypes.byref(pos), ctypes.c_void_p(runs.ctypes.data),
                ctypes.c_int64(int(n_written)), ctypes.byref(n_runs), ctypes.byref(bad), ctypes.byref(reason))
        if rc == -6 and bad.value >= 0:
            name = ctypes.create_string_buffer(256)
            self._lib.mdx_gbam_record_name(self._g, ctypes.c_int64(bad.value), name, 256)
            raise KeptIndexError(bad.value, name.value.decode(errors="replace"), reason.value)
        if rc != 0:
            from .engine import MdxError
            raise MdxError(rc, "%r: %s" % (str(self.path), self._error()))
        return runs[:n_runs.value], (int(tid.value), int(pos.value))

    def kept_index_linear(self):
        """The linear index all ``kept_index`` calls of this stream left on the device (``mdx_gbam_kept_index_linear``): one
        uint64 per 16 KiB window of every header sequence in turn, the lowest stream offset of a written record that touches
        it, all ones for an untouched window."""
        import ctypes
        fn = self._lib.mdx_gbam_kept_index_linear
        fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p], ctypes.c_int
        words = ctypes.c_int64(0)
        rc = fn(self._g, None, ctypes.c_int64(0), ctypes.byref(words))
        out = np.zeros(max(1, words.value), np.uint64)
        if rc == 0:
            rc = fn(self._g, ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(words.value), None)
        if rc != 0:
            from .engine import MdxError
            raise MdxError(rc, "%r: %s" % (str(self.path), self._error()))
        return out[:words.value]

    def fixups(self):
        """BGZF blocks whose guessed first record was not where the chain of the records in front of it ended (rescanned
        from the right offset: the result is exact either way)."""
        return int(self._lib.mdx_gbam_fixups(self._g))

    def skip(self):
        """Step over the slab ``next_view`` would decode (a run over several GPUs: the slabs of the other ranks).
        False at the end of the file."""
        if self._lib.mdx_gbam_at_end(self._g):
            return False
        rc = self._lib.mdx_gbam_skip(self._g, self.chunk_bytes)
        if rc == -8:
            raise GpuDecodeUnsupported("%r: %s" % (str(self.path), self._error()))
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        return True

    def close(self):
        if self._g:
            # (mdx_gbam_close gives the arena back to the context: never reached with the context gone — the engine closes
            # its streams first)
            self._lib.mdx_gbam_close(self._g)
            self._g = None
            streams = getattr(self._engine, "_streams", None)
            if streams is not None:
                streams.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuSamStream:
    """GPU-side parse of SAM text (include/mdx.h ``mdx_gsam_*``): a slab of whole lines at a time goes to HBM and is parsed
    there into the columns ``read_sam`` makes; ``GpuBamStream``'s interface (``next_view`` returns an ``MdxBatch`` of DEVICE
    pointers, None at the end).  Raises ``GpuDecodeUnsupported`` for a slab where Python's parser could read a line otherwise
    (see the header) — the caller then parses on the host, a stream from ``tell()`` on (``Source.seek``).  ``path``: a
    file's, or a ``Source``."""

    def __init__(self, engine, path, readgroups=(), lib_default=None, chunk_bytes=256 << 20, want_qual=False,
                 min_basequal=0, packed=None, record_filter=None):
        import ctypes
        self._lib = engine._lib
        self._engine = engine
        self._g = ctypes.c_void_p()
        self.path, self.chunk_bytes = path, int(chunk_bytes)
        if not engine._ctx:
            raise ValueError("the engine is closed")
        lib = self._lib
        lib.mdx_gsam_error.restype = ctypes.c_char_p
        lib.mdx_gsam_header.restype = ctypes.c_void_p
        for name in ("mdx_gsam_error", "mdx_gsam_header", "mdx_gsam_at_end", "mdx_gsam_missing_qualities", "mdx_gsam_close",
                     "mdx_gsam_is_bgzf"):
            getattr(lib, name).argtypes = [ctypes.c_void_p]
        if isinstance(path, Source):
            rc = lib.mdx_gsam_open_source(engine._ctx, path.handle, ctypes.byref(self._g))
        else:
            rc = lib.mdx_gsam_open(engine._ctx, str(path).encode(), ctypes.byref(self._g))
        if not hasattr(engine, "_streams"):
            import weakref
            engine._streams = weakref.WeakSet()
        engine._streams.add(self)
        if rc != 0:
            message = self._error()
            self.close()
            if rc == -8:
                raise GpuDecodeUnsupported("%r: %s" % (str(path), message))
            raise ValueError("%r: %s" % (str(path), message))
        self.header = _native_header(lib, lib.mdx_gsam_header(self._g))
        ids = [str(rg).encode() for rg, _ in readgroups]
        arr = (ctypes.c_char_p * max(1, len(ids)))(*ids)
        libs = (ctypes.c_int32 * max(1, len(ids)))(*[int(x) for _, x in readgroups])
        rc = lib.mdx_gsam_configure(self._g, len(ids), arr, libs, -1 if lib_default is None else int(lib_default), int(bool(want_qual)))
        if rc != 0:
            raise ValueError("%r: %s" % (str(path), self._error()))
        if min_basequal and lib.mdx_gsam_set_min_basequal(self._g, int(min_basequal)) != 0:
            raise ValueError("%r: %s" % (str(path), self._error()))
        if packed is None:
            packed = bool(min_basequal) or not want_qual
        self.packed = bool(packed)
        if self.packed:
            lib.mdx_gsam_set_seq_format(self._g, 1)
        if record_filter is not None and record_filter.active:
            flt = record_filter.as_struct()
            if lib.mdx_gsam_set_record_filter(self._g, ctypes.byref(flt)) != 0:
                raise ValueError("%r: %s" % (str(path), self._error()))

    def filter_counts(self):
        """uint64[6]: the records parsed so far (of slabs handed out), and those the record filter dropped, by reason."""
        import ctypes
        out = np.zeros(6, np.uint64)
        if self._lib.mdx_gsam_filter_counts(self._g, ctypes.c_void_p(out.ctypes.data)) != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        return out

    def _error(self):
        return self._lib.mdx_gsam_error(self._g).decode(errors="replace") if self._g else "GPU SAM decode failed"

    def missing_qualities(self):
        """A record the kernel counts has come by without qualities (main.py:185-192 warns once)."""
        return bool(self._lib.mdx_gsam_missing_qualities(self._g))

    def next_view(self):
        import ctypes
        from .engine import MdxBatch
        view = MdxBatch()
        rc = self._lib.mdx_gsam_next(self._g, ctypes.c_int64(self.chunk_bytes), ctypes.byref(view))
        if rc == -8:
            raise GpuDecodeUnsupported("%r: %s" % (str(self.path), self._error()))
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        if view.n_reads == 0 and self._lib.mdx_gsam_at_end(self._g):
            return None
        view.mtid, view.mpos = None, None
        return view

    def tell(self):
        """Where the first line of the slab ``next_view`` would parse starts (a failed call: of the slab that failed): a byte
        offset for plain text; for bgzip-compressed text the pair (compressed offset of a BGZF block, inflated bytes in
        front of the line within it) — what ``compressed_text`` and ``BAMReader.iter_batches(resume=...)`` take."""
        import ctypes
        if self._lib.mdx_gsam_is_bgzf(self._g):
            coff, phase = ctypes.c_int64(), ctypes.c_int64()
            if self._lib.mdx_gsam_tell_bgzf(self._g, ctypes.byref(coff), ctypes.byref(phase)) != 0:
                return None
            return coff.value, phase.value
        off = ctypes.c_int64()
        if self._lib.mdx_gsam_tell(self._g, ctypes.byref(off)) != 0:
            return None
        return off.value

    def view_flags(self, view):
        import ctypes
        n = int(view.n_reads)
        out = np.empty(n, np.uint16)
        rc = self._lib.mdx_gsam_view_flags(self._g, ctypes.c_void_p(out.ctypes.data), ctypes.c_int64(n))
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        return out

    def set_view_flags(self, view, flags):
        import ctypes
        flags = np.ascontiguousarray(flags, dtype=np.uint16)
        assert flags.shape[0] == int(view.n_reads)
        rc = self._lib.mdx_gsam_view_set_flags(self._g, ctypes.c_void_p(flags.ctypes.data), ctypes.c_int64(flags.shape[0]))
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))

    def fixups(self):
        return 0

    def skip(self):
        raise GpuDecodeUnsupported("%r: SAM text is parsed by one rank" % str(self.path))

    def close(self):
        if self._g:
            self._lib.mdx_gsam_close(self._g)
            self._g = None
            streams = getattr(self._engine, "_streams", None)
            if streams is not None:
                streams.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _header_run(data, complete):
    """The leading run of '@' lines of ``data``: (its length, True if it is known to end there)."""
    off = 0
    while True:
        if off >= len(data):
            return off, complete
        if data[off:off + 1] != b"@":
            return off, True
        e = data.find(b"\n", off)
        if e < 0:
            return (len(data), True) if complete else (off, False)
        off = e + 1


def sam_header(src):
    """The header of SAM text — its leading run of lines that start with '@', as ``read_sam`` reads it — and the byte
    offset of the first line behind it, without reading further: a ``Source`` is peeked (a stream keeps every byte for
    whoever parses the body), a path is read line by line.  Compressed text (``input_format``): the offset counts inflated
    bytes, and only as many compressed bytes are read (a ``Source``: peeked) as the header takes."""
    compressed = input_format(src) in (SAM_BGZF, SAM_GZIP)
    if isinstance(src, Source) or compressed:
        handle = None if isinstance(src, Source) else open(src, "rb")
        try:
            n = 1 << 16
            while True:
                if handle is None:
                    data = src.peek(n)
                else:
                    handle.seek(0)
                    data = handle.read(n)
                complete = len(data) < n            # (the whole input)
                if compressed:
                    data = _inflate_prefix(data)[0]
                off, done = _header_run(data, complete)
                if done:
                    break
                n *= 2
        finally:
            if handle is not None:
                handle.close()
        raw = data[:off]
    else:
        raw = b""
        with open(src, "rb") as handle:
            for line in handle:
                if not line.startswith(b"@"):
                    break
                raw += line
    import sys
    encoding = getattr(sys.__stdin__, "encoding", None) or "utf-8" if isinstance(src, Source) else None
    text = raw.decode(encoding) if encoding else io.TextIOWrapper(io.BytesIO(raw)).read()
    return Header(text), len(raw)


class GpuDecodeUnsupported(ValueError):
    """The file's layout is not one the GPU decode path takes (MDX_ERR_UNSUPPORTED)."""


MASK_WHAT = ("all", "transitions", "mismatches")      # include/mdx.h MDX_MASK_*, by value (--mask-what)


class KeptTagClash(Exception):
    """``GpuBamStream.write_kept`` with tags: a record to be written has a tag of one of the names already (MDX_ERR_BAD_READ,
    ``code`` -6).  ``index``: the record's index in its slab, ``name``: its read name, ``tags``: the names asked for."""
    code = -6

    def __init__(self, index, name, tags):
        super().__init__("Read: %s already has a tag named %s; the run appends such a tag to every record it writes "
                         "(choose another name)" % (name, " or ".join(tags)))
        self.index, self.name, self.tags = int(index), name, list(tags)


class KeptIndexError(Exception):
    """``GpuBamStream.kept_index``: a record that is written cannot be indexed (MDX_ERR_BAD_READ, ``code`` -6) — ``reason``
    1: it lies in front of the written record before it, 2: it does not lie inside the first 2^29 bases of a header sequence.
    ``index``: the record's index in its slab, ``name``: its read name."""
    code = -6
    UNSORTED, UNPLACEABLE = 1, 2

    def __init__(self, index, name, reason):
        why = ("lies in front of the written record before it; an index needs the written records in coordinate order (sort the "
               "input first)" if int(reason) == self.UNSORTED else
               "does not lie inside its reference sequence, or ends behind base 2^29, which BAI cannot address")
        super().__init__("Read: %s is to be written and %s" % (name, why))
        self.index, self.name, self.reason = int(index), name, int(reason)


class BamStream:
    """Chunked form of ``read_bam_native`` (include/mdx.h ``mdx_bam_open`` / ``mdx_bam_next``): iterating yields
    ``Alignments`` of consecutive records, at most ``chunk_bytes`` of uncompressed BAM data each, so host memory stays
    bounded and the caller can tabulate one chunk while the next is decoded (the ctypes call drops the GIL).  ``path``: a
    file's, or a ``Source`` (a stream is taken up where a ``GpuBamStream`` on the same source gave up: ``seek``)."""

    def __init__(self, path, threads=None, chunk_bytes=256 << 20, keep_raw=False):
        import ctypes
        import os

        from .engine import load_library
        self._lib = load_library()
        self._stream = ctypes.c_void_p()
        self.path, self.chunk_bytes, self.keep_raw = path, int(chunk_bytes), bool(keep_raw)
        if isinstance(path, Source):
            rc = self._lib.mdx_bam_open_source(path.handle, ctypes.c_int(threads or min(64, usable_cpus())),
                                               ctypes.byref(self._stream))
        else:
            rc = self._lib.mdx_bam_open(str(path).encode(), ctypes.c_int(threads or min(64, usable_cpus())),
                                        ctypes.byref(self._stream))
        if rc != 0:
            message = self._error()
            self.close()
            raise ValueError("%r: %s" % (str(path), message))
        self.header = _native_header(self._lib, self._lib.mdx_bam_stream_header(self._stream))
        if self.keep_raw:
            self._lib.mdx_bam_stream_keep_raw(self._stream, 1)

    def _error(self):
        if not self._stream:
            return "BAM decode failed"
        return self._lib.mdx_bam_error(self._lib.mdx_bam_stream_header(self._stream)).decode()

    def seek(self, comp_off, phase=0):
        """Go on from the BGZF block at compressed offset ``comp_off``, the first record ``phase`` inflated bytes into it
        (``GpuBamStream.tell``)."""
        import ctypes
        if self._lib.mdx_bam_seek(self._stream, ctypes.c_int64(int(comp_off)), ctypes.c_int64(int(phase))) != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))

    def next_chunk(self):
        """The next ``Alignments`` or None at the end of the file."""
        import ctypes
        handle = ctypes.c_void_p()
        rc = self._lib.mdx_bam_next(self._stream, self.chunk_bytes, ctypes.byref(handle))
        if rc != 0:
            raise ValueError("%r: %s" % (str(self.path), self._error()))
        if not handle:
            return None
        chunk = _native_alignments(self._lib, handle, _NativeBam(self._lib, handle), self.header)
        chunk.native = handle          # (kept alive by the chunk's owner object) for patch_rescaled()
        return chunk

    def raw_bodies(self, chunk, count=None):
        """The encoded bodies (without their block_size field) of the first ``count`` records of ``chunk`` (decoded with
        ``keep_raw``), as bytes objects."""
        import ctypes
        n = chunk.batch.n if count is None else min(int(count), chunk.batch.n)
        data, rec_off = ctypes.c_void_p(), ctypes.c_void_p()
        if self._lib.mdx_bam_raw(chunk.native, ctypes.byref(data), ctypes.byref(rec_off)) != 0:
            raise ValueError("the stream was not opened with keep_raw")
        off = np.ctypeslib.as_array(ctypes.cast(rec_off, ctypes.POINTER(ctypes.c_uint64)), (chunk.batch.n + 1,))
        blob = ctypes.string_at(data.value, int(off[n]))
        return [blob[int(off[i]) + 4:int(off[i + 1])] for i in range(n)]

    def patch_rescaled(self, chunk, qual_out, mr, rescaled):
        """The encoded records of ``chunk`` (decoded with ``keep_raw``) with the QUAL of the records flagged in
        ``rescaled`` replaced from ``qual_out`` and an ``MR:f`` tag appended; every other byte as in the file."""
        import ctypes
        n = chunk.batch.n
        qual_out = np.ascontiguousarray(qual_out, np.uint8)
        mr = np.ascontiguousarray(mr, np.float32)
        rescaled = np.ascontiguousarray(rescaled, np.uint8)
        data, rec_off = ctypes.c_void_p(), ctypes.c_void_p()
        if self._lib.mdx_bam_raw(chunk.native, ctypes.byref(data), ctypes.byref(rec_off)) != 0:
            raise ValueError("the stream was not opened with keep_raw")
        end = int(np.ctypeslib.as_array(ctypes.cast(rec_off, ctypes.POINTER(ctypes.c_uint64)), (n + 1,))[n])
        out = np.empty(end + 7 * int(rescaled.sum()) + 8, np.uint8)
        out_len = ctypes.c_int64(0)
        rc = self._lib.mdx_bam_patch_rescaled(chunk.native, qual_out.ctypes.data_as(ctypes.c_void_p),
                                              mr.ctypes.data_as(ctypes.c_void_p), rescaled.ctypes.data_as(ctypes.c_void_p),
                                              out.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(out.shape[0]),
                                              ctypes.byref(out_len))
        if rc != 0:
            raise ValueError("mdx_bam_patch_rescaled failed (%d)" % rc)
        return out[:out_len.value]

    def __iter__(self):
        while True:
            chunk = self.next_chunk()
            if chunk is None:
                return
            yield chunk

    def close(self):
        if self._stream:
            self._lib.mdx_bam_close(self._stream)
            self._stream = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def input_is_stream(path):
    """The reference's rule for an input read as a stream (mapdamage/reader.py:32-38): ``-``, a FIFO (a named pipe,
    ``/dev/fd/N`` of a process substitution) or a character device.  Such a path is opened once per run (``Source``)."""
    import os
    import stat
    if str(path) == "-":
        return True
    try:
        mode = os.stat(path).st_mode
    except OSError:
        return False
    return stat.S_ISFIFO(mode) or stat.S_ISCHR(mode)


class Source:
    """The input opened once (include/mdx.h ``mdx_source_*``): a regular file is mapped, anything else — stdin (``-``), a
    pipe, a FIFO, a character device — is read front to back by a thread of the library into a bounded window.  The header
    read, the device decode and the host decoder all attach to it (``BamStream``, ``GpuBamStream``, ``read_bam_native``
    take one in place of a path); ``peek`` tells SAM from BAM without losing a byte, ``text`` reads SAM through it.
    ``str()`` is the path, so messages name the input as for a file."""

    def __init__(self, path):
        import ctypes

        from .engine import load_library
        self._lib = load_library()
        self.path = path
        self.handle = ctypes.c_void_p()
        self._peeked = (0, b"")
        rc = self._lib.mdx_source_open(str(path).encode(), ctypes.byref(self.handle))
        if rc != 0:
            message = self._lib.mdx_source_error(self.handle).decode() if self.handle else "cannot open"
            self.close()
            raise ValueError("%r: %s" % (str(path), message))
        self.is_stream = bool(self._lib.mdx_source_is_stream(self.handle))

    def __str__(self):
        return str(self.path)

    def error(self):
        return self._lib.mdx_source_error(self.handle).decode() if self.handle else "closed"

    def peek(self, n):
        """The first ``n`` bytes (fewer: the input is shorter); a stream waits for them.  (They are kept here too: a stream
        lets go of its first bytes once a decoder has read past them, and the format is asked about after that.)"""
        import ctypes
        if n <= self._peeked[0]:
            return self._peeked[1][:n]
        buf = ctypes.create_string_buffer(max(1, int(n)))
        got = ctypes.c_int32(0)
        if self._lib.mdx_source_peek(self.handle, buf, int(n), ctypes.byref(got)) != 0:
            raise ValueError("%r: %s" % (str(self.path), self.error()))
        self._peeked = (int(n), buf.raw[:got.value])
        return self._peeked[1]

    def readinto(self, view):
        """The next bytes in order into ``view`` (a writable buffer): how many, 0 at the end."""
        import ctypes
        n = len(view)
        if n == 0:
            return 0
        buf = (ctypes.c_char * n).from_buffer(view)
        got = self._lib.mdx_source_read(self.handle, buf, n)
        if got < 0:
            raise ValueError("%r: %s" % (str(self.path), self.error()))
        return int(got)

    def text(self):
        """The input as text, from its first byte — the peeked ones included — decoded as ``sys.stdin`` decodes."""
        import sys
        source = self

        class _Raw(io.RawIOBase):
            def readable(self):
                return True

            def readinto(self, view):
                return source.readinto(memoryview(view).cast("B"))

        stdin = sys.__stdin__
        return io.TextIOWrapper(io.BufferedReader(_Raw(), 1 << 20), encoding=getattr(stdin, "encoding", None) or "utf-8",
                                errors=getattr(stdin, "errors", None) or "strict")

    def seek(self, offset):
        """The next ``readinto`` (and ``text``) starts at byte ``offset`` of the input (a stream: not in front of what it has
        let go of)."""
        import ctypes
        fn = self._lib.mdx_source_seek
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int64]
        if fn(self.handle, int(offset)) != 0:
            raise ValueError("%r: %s" % (str(self.path), self.error()))

    def close(self):
        if getattr(self, "handle", None):
            self._lib.mdx_source_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BAM, SAM_TEXT, SAM_BGZF, SAM_GZIP = "BAM", "SAM text", "bgzip-compressed SAM text", "plain gzip SAM text"


def _inflate_prefix(data, want=None):
    """(what the gzip members at the front of ``data`` — the first bytes of an input, cut anywhere — inflate to: all of it, or
    ``want`` bytes at least where there are as many; True where bytes that do not inflate ended it).  Empty members are stepped
    over."""
    import zlib
    out, rest = [], data
    got = 0
    while rest and (want is None or got < want):
        z = zlib.decompressobj(31)
        try:
            piece = z.decompress(rest) if want is None else z.decompress(rest, max(1, want - got))
        except zlib.error:
            return b"".join(out), True
        out.append(piece)
        got += len(piece)
        if not z.eof:
            break
        rest = z.unused_data
    return b"".join(out), False


def _bgzf_member(head):
    """Do the bytes start a gzip member with the 'BC' extra subfield of BGZF (``fasta.is_bgzf``'s test)?"""
    if len(head) < 12 or head[:4] != b"\x1f\x8b\x08\x04":
        return False
    extra = head[12:12 + int.from_bytes(head[10:12], "little")]
    at = 0
    while at + 4 <= len(extra):
        size = int.from_bytes(extra[at + 2:at + 4], "little")
        if extra[at:at + 2] == b"BC" and size == 2 and at + 6 <= len(extra):
            return True
        at += 4 + size
    return False


def input_format(path):
    """``BAM``, ``SAM_TEXT``, ``SAM_BGZF`` or ``SAM_GZIP``, by content, as htslib sniffs through compression
    (mapdamage/reader.py:38).  Two bytes tell uncompressed SAM text; an input that starts with 1f 8b is inflated until four
    bytes of content have come or the input ends (empty members in front stepped over) — ``BAM\\1`` is BAM, anything else SAM
    text, an input that inflates to nothing too; it is bgzip-compressed when the first member carries the 'BC' extra subfield
    and plain gzip otherwise.  The one exception: first bytes that do not inflate at all are left to the BAM decoders, which
    word what is wrong with such a file.  A ``Source`` is peeked; a path that is a stream (``input_is_stream``) is never
    opened here — its bytes would be lost to the run — and must come as a ``Source``."""
    if not isinstance(path, Source) and input_is_stream(path):
        raise ValueError("%r is a stream: it is read once, through a Source" % str(path))

    def first(n):
        if isinstance(path, Source):
            return path.peek(n)
        with open(path, "rb") as handle:
            return handle.read(n)

    if first(2) != b"\x1f\x8b":
        return SAM_TEXT
    n = 1 << 16
    while True:
        data = first(n)
        content, failed = _inflate_prefix(data, 4)
        if len(content) >= 4 or failed or len(data) < n:
            break
        n *= 4
    if content[:4] == b"BAM\x01" or (failed and not content):
        return BAM
    return SAM_BGZF if _bgzf_member(data) else SAM_GZIP


def is_bam(path):
    """BAM or not (SAM text, compressed or plain), by content (``input_format``)."""
    return input_format(path) == BAM


class _Inflated(io.RawIOBase):
    """The gzip members of a compressed input — BGZF blocks or plain gzip, any number of them — inflated as they are read
    (zlib checks every member's CRC32 and ISIZE), without the first ``drop`` inflated bytes.  ``readinto`` brings the
    compressed bytes, from compressed offset ``base`` on; ``handle``: what to close with this.  zlib is fed a few KiB at a time
    and rewound to where a member ended, so that small members cost no copy of everything behind them."""

    PIECE = 4096

    def __init__(self, name, readinto, drop=0, base=0, handle=None):
        import zlib
        self._name, self._readinto, self._drop, self._handle = name, readinto, int(drop), handle
        self._z = zlib.decompressobj(31)
        self._buf = bytearray(1 << 20)
        self._data, self._pos, self._base = b"", 0, int(base)      # the bytes read last, how many zlib has, where they start
        self._out = b""
        self._member = int(base)                                    # where the current member starts
        self._fresh, self._eof = True, False

    def readable(self):
        return True

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None
        super().close()

    def _more(self):
        import zlib
        if self._z.eof:
            self._member = self._base + self._pos
            self._z = zlib.decompressobj(31)
            self._fresh = True
        if self._pos >= len(self._data):
            got = self._readinto(memoryview(self._buf))
            if not got:
                if not self._fresh:
                    raise BAMError("%r: the gzip member at compressed offset %d is cut short" % (self._name, self._member))
                self._eof = True
                return b""
            self._base += len(self._data)
            self._data, self._pos = bytes(self._buf[:got]), 0
        piece = self._data[self._pos:self._pos + self.PIECE]
        self._pos += len(piece)
        self._fresh = False
        try:
            out = self._z.decompress(piece)
        except zlib.error as error:
            raise BAMError("%r: the gzip member at compressed offset %d does not inflate or fails its CRC32 / ISIZE check (%s)"
                           % (self._name, self._member, error)) from None
        if self._z.eof:
            self._pos -= len(self._z.unused_data)
        return out

    def readinto(self, view):
        view = memoryview(view).cast("B")
        while not self._out and not self._eof:
            piece = self._more()
            if self._drop:
                cut = min(self._drop, len(piece))
                self._drop -= cut
                piece = piece[cut:]
            self._out = piece
        n = min(len(view), len(self._out))
        view[:n] = self._out[:n]
        self._out = self._out[n:]
        return n


def compressed_text(path, resume=(0, 0)):
    """Compressed SAM text (``SAM_BGZF`` or ``SAM_GZIP``) as a text handle for ``read_sam``, inflated by zlib as it is read.
    ``resume``: (compressed offset of a gzip member — a BGZF block —, inflated bytes to drop behind it): the text from there
    on (``GpuSamStream.tell``; a ``Source`` that is a stream must still hold that block).  A ``Source`` is decoded as
    ``sys.stdin`` decodes, a path as ``open(path, "rt")`` does."""
    import sys
    coff, drop = int(resume[0]), int(resume[1])
    if isinstance(path, Source):
        path.seek(coff)
        stdin = sys.__stdin__
        raw = _Inflated(str(path), path.readinto, drop, coff)
        return io.TextIOWrapper(io.BufferedReader(raw, 1 << 20), encoding=getattr(stdin, "encoding", None) or "utf-8",
                                errors=getattr(stdin, "errors", None) or "strict")
    handle = open(path, "rb")
    handle.seek(coff)
    raw = _Inflated(str(path), handle.readinto, drop, coff, handle)
    return io.TextIOWrapper(io.BufferedReader(raw, 1 << 20))


def read_alignments(path, record_filter=None):
    """SAM or BAM by content (mapdamage/reader.py:38 lets htslib sniff the format, through compression too).  BAM goes through
    the native decoder of libmdx.so; the pure-Python ``read_bam`` remains as its cross-check.  Compressed SAM text — BGZF or
    plain gzip, any number of members — is inflated by zlib on the way into ``read_sam``.  ``path``: a file's, or a
    ``Source`` (stdin and pipes: SAM text is read through it, the sniffed bytes included).  ``record_filter``: a
    ``RecordFilter`` — the result then has its dropped records marked and carries ``filter_counts``."""
    if not isinstance(path, Source) and str(path) == "-":
        import sys
        return read_sam(sys.stdin, record_filter=record_filter)
    kind = input_format(path)
    if kind == BAM:
        al = read_bam_native(path)
        if record_filter is not None and record_filter.active:
            al.filter_counts = apply_record_filter(al, record_filter)
        return al
    if kind != SAM_TEXT:
        with compressed_text(path) as handle:
            return read_sam(handle, record_filter=record_filter)
    if isinstance(path, Source):
        return read_sam(path.text(), record_filter=record_filter)
    return read_sam(str(path), record_filter=record_filter)


def header_text(ref_names, ref_lengths, read_groups):
    lines = ["@HD\tVN:1.6\tSO:unsorted"]
    lines += ["@SQ\tSN:%s\tLN:%d" % (n, ln) for n, ln in zip(ref_names, ref_lengths)]
    for rg in read_groups:
        lines.append("@RG\t" + "\t".join("%s:%s" % kv for kv in rg.items()))
    return "\n".join(lines) + "\n"


def _cigar_string(ops):
    return "".join("%d%s" % (int(c) >> 4, L.CIGAR_CHARS[int(c) & 15]) for c in ops) or "*"


def write_sam(path, batch: ReadBatch, ref_names, ref_lengths, read_groups, rg_of_record=None, mapq=None):
    """``read_groups``: list of dicts (ID, SM, LB ...); ``rg_of_record``: RG id per record or None; ``mapq``: MAPQ per record
    (30 everywhere without)."""
    with open(path, "wt") as out:
        out.write(header_text(ref_names, ref_lengths, read_groups))
        for i in range(batch.n):
            c0, c1 = int(batch.cigar_off[i]), int(batch.cigar_off[i + 1])
            s0, s1 = int(batch.seq_off[i]), int(batch.seq_off[i + 1])
            seq = batch.seq[s0:s1].tobytes().decode() or "*"
            qual = "*"
            if batch.qual is not None and s1 > s0 and int(batch.qual[s0]) != 0xFF:
                qual = (batch.qual[s0:s1] + 33).astype(np.uint8).tobytes().decode()
            tid = int(batch.tid[i])
            fields = ["r%d" % i, str(int(batch.flag[i])), ref_names[tid] if tid >= 0 else "*",
                      str(int(batch.pos[i]) + 1), "30" if mapq is None else str(int(mapq[i])), _cigar_string(batch.cigar[c0:c1]), "*", "0",
                      str(int(batch.tlen[i])), seq, qual]
            rg = None if rg_of_record is None else rg_of_record[i]
            if rg is not None:
                fields.append("RG:Z:%s" % rg)
            out.write("\t".join(fields) + "\n")


_WB_JOB = None


def _wb_slice(span):
    """Worker of write_bam(workers=N): records [lo, hi) of batch k as finished BGZF blocks, each starting at a record."""
    k, lo, hi = span
    batches, rg_of_record, mapq = _WB_JOB
    batch = batches[k]
    mapq = None if mapq is None else mapq[k]                          # (per batch: write_bam has seen to it)
    out = io.BytesIO()
    room = 0xFF00
    piece = bytearray()
    for i in range(lo, hi):
        record = _bam_record(batch, i, rg_of_record if rg_of_record is None or isinstance(rg_of_record, str) else rg_of_record[i],
                             mapq=None if mapq is None else (mapq if np.isscalar(mapq) else mapq[i]))
        if piece and len(piece) + len(record) > room:
            out.write(_bgzf_block(bytes(piece)))
            piece = bytearray()
        piece += record
        while len(piece) > room:                 # a record larger than a block spills over
            out.write(_bgzf_block(bytes(piece[:room])))
            del piece[:room]
    if piece:
        out.write(_bgzf_block(bytes(piece)))
    return out.getvalue()


def _bam_record(batch, i, rg, mapq=None):
    c0, c1 = int(batch.cigar_off[i]), int(batch.cigar_off[i + 1])
    s0, s1 = int(batch.seq_off[i]), int(batch.seq_off[i + 1])
    name = ("r%d" % i).encode() + b"\x00"
    l_seq = s1 - s0
    codes = _SEQ_ENCODE[batch.seq[s0:s1]]
    if l_seq % 2:
        codes = np.concatenate([codes, np.zeros(1, np.uint8)])
    packed = ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8).tobytes()
    qual = batch.qual[s0:s1].tobytes() if batch.qual is not None else b"\xff" * l_seq
    aux = b"" if rg is None else b"RGZ" + rg.encode() + b"\x00"
    ntid = -1 if batch.mtid is None else int(batch.mtid[i])
    npos = -1 if batch.mpos is None else int(batch.mpos[i])
    body = struct.pack("<iiBBHHHiiii", int(batch.tid[i]), int(batch.pos[i]), len(name), 30 if mapq is None else int(mapq), 4680,
                       c1 - c0, int(batch.flag[i]), l_seq, ntid, npos, int(batch.tlen[i]))
    body += name + batch.cigar[c0:c1].astype("<u4").tobytes() + packed + qual + aux
    return struct.pack("<i", len(body)) + body


def write_bam(path, batch, ref_names, ref_lengths, read_groups, rg_of_record=None, htslib_blocks=True,
              workers=1, block_bytes=0xFF00, mapq=None):
    """``htslib_blocks``: lay the BGZF blocks out as htslib does (the header flushed on its own, and a block closed
    early when the next record would not fit, ``bgzf_flush_try`` in ``bam_write1``), so that every block starts
    at a record — what the files mapDamage sees in practice look like, and what the native decoder's parallel
    record scan speculates on.  False: header and records as one stream cut into blocks of ``block_bytes`` anywhere — the
    header shares a block with records, records straddle blocks (htsjdk / Picard fill 65 498 bytes per block).
    ``workers`` > 1 (htslib layout only): the records are encoded and deflated by forked worker processes, a slice
    each (call it before the process touches the GPU); a slice starts a block of its own, otherwise the same file.
    With workers, ``batch`` may be a list of batches (written one behind the other: a file of more than 4 G bases) and
    ``rg_of_record`` one read-group id for every record.  ``mapq``: one MAPQ for every record, or — ``batch`` a single batch — one per record,
    or — ``batch`` a list of batches, of whatever length — a list of one array (or value) per batch; 30 everywhere without."""
    text = header_text(ref_names, ref_lengths, read_groups).encode()
    batches = list(batch) if isinstance(batch, (list, tuple)) else [batch]
    # MAPQ per batch from here on: one value, or an array per record
    if mapq is not None:
        if np.isscalar(mapq):
            mapq = [mapq] * len(batches)
        elif isinstance(batch, (list, tuple)):
            mapq = list(mapq)
            if len(mapq) != len(batches) or any(not np.isscalar(m) and len(m) != b.n for m, b in zip(mapq, batches)):
                raise ValueError("with a list of batches, mapq is a list of one array (or value) per batch")
        else:
            if len(mapq) != batches[0].n:
                raise ValueError("mapq holds one value per record")
            mapq = [mapq]
    if htslib_blocks and workers > 1 and sum(b.n for b in batches) > 4 * workers:
        import multiprocessing as mp
        global _WB_JOB
        head = io.BytesIO()
        head.write(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(ref_names)))
        for name, ln in zip(ref_names, ref_lengths):
            nb = name.encode() + b"\x00"
            head.write(struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln))
        hv = head.getvalue()
        n_jobs = workers * 4
        spans = [(k, b.n * j // n_jobs, b.n * (j + 1) // n_jobs) for k, b in enumerate(batches) for j in range(n_jobs)]
        _WB_JOB = (batches, rg_of_record, mapq)
        try:
            with mp.get_context("fork").Pool(workers) as pool, open(path, "wb") as out:
                for lo in range(0, len(hv), 0xFF00):
                    out.write(_bgzf_block(hv[lo:lo + 0xFF00]))
                for blob in pool.imap(_wb_slice, spans, chunksize=1):
                    out.write(blob)
                out.write(_bgzf_block(b""))
        finally:
            _WB_JOB = None
        return
    if len(batches) != 1:
        raise ValueError("several batches are written by forked workers only (workers > 1, htslib layout)")
    batch = batches[0]
    mapq = None if mapq is None else mapq[0]
    if isinstance(rg_of_record, str):
        rg_of_record = [rg_of_record] * batch.n
    raw = io.BytesIO()
    pieces = []                      # htslib layout: uncompressed payload of each block
    room = 0xFF00
    raw.write(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(ref_names)))
    for name, ln in zip(ref_names, ref_lengths):
        nb = name.encode() + b"\x00"
        raw.write(struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln))
    if htslib_blocks:
        head = raw.getvalue()
        pieces = [bytearray(head[lo:lo + room]) for lo in range(0, len(head), room)] + [bytearray()]
    for i in range(batch.n):
        record = _bam_record(batch, i, None if rg_of_record is None else rg_of_record[i],
                             mapq=None if mapq is None else (mapq if np.isscalar(mapq) else mapq[i]))
        if not htslib_blocks:
            raw.write(record)
            continue
        if pieces[-1] and len(pieces[-1]) + len(record) > room:
            pieces.append(bytearray())
        pieces[-1] += record
        while len(pieces[-1]) > room:            # a record larger than a block spills over
            pieces.append(pieces[-1][room:])
            del pieces[-2][room:]
    if not htslib_blocks:
        data = raw.getvalue()
        pieces = [data[lo:lo + block_bytes] for lo in range(0, len(data), block_bytes)]
    with open(path, "wb") as out:
        for piece in pieces:
            if len(piece):
                out.write(_bgzf_block(bytes(piece)))
        out.write(_bgzf_block(b""))


def _bgzf_block(chunk):
    comp = zlib.compressobj(6, zlib.DEFLATED, -15)
    deflated = comp.compress(chunk) + comp.flush()
    bsize = len(deflated) + 25
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize)
            + deflated + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk)))
