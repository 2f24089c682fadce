"""--write-index: the BAI file (SAM specification 5.2) of the BAM ``--write-kept`` writes, put together from what the device
hands back per slab (include/mdx.h ``mdx_gbam_kept_index``; the rule: csrc/mdx_kept_index.h) — the runs of written records
with the same (tid, bin) and, at the end, the linear index's minima, all in offsets of the uncompressed record stream — and
from the compressed sizes of the BGZF members the same slab became, which turn a stream offset into a virtual file offset.
Nothing here reads the written file."""

import struct

import numpy as np

MEMBER_BYTES = 0xFF00           # the device's BGZF writer cuts a slab's stream into members of exactly this many bytes
PSEUDO_BIN = 37450
UNTOUCHED = np.uint64(0xFFFFFFFFFFFFFFFF)
RUN_DTYPE = np.dtype([("tid", "<i4"), ("bin", "<u4"), ("ustart", "<u8"), ("uend", "<u8"), ("first", "<u4"), ("last", "<u4")])
assert RUN_DTYPE.itemsize == 32


def member_sizes(members):
    """The compressed sizes of back-to-back BGZF members (a uint8 array or bytes), from their BSIZE fields."""
    data = memoryview(members).cast("B")
    sizes, at = [], 0
    while at < len(data):
        if at + 18 > len(data) or bytes(data[at:at + 4]) != b"\x1f\x8b\x08\x04" or bytes(data[at + 12:at + 16]) != b"BC\x02\x00":
            raise ValueError("not a BGZF member at byte %d" % at)
        size = (data[at + 16] | data[at + 17] << 8) + 1
        sizes.append(size)
        at += size
    if at != len(data):
        raise ValueError("the last BGZF member is cut short")
    return np.asarray(sizes, np.int64)


def linear_windows(lengths):
    """Words of the device's linear index: ceil(LN / 16384) per header sequence, in turn."""
    return [max(0, (int(n) + 16383) >> 14) for n in lengths]


class BaiAssembler:
    """``add_slab`` once per slab that wrote records, in file order; ``finish(linear)`` gives the file's bytes."""

    def __init__(self, lengths):
        self.lengths = [int(n) for n in lengths]
        self.bases, self.raws, self.first_member, self.file_offsets = [], [], [], []     # per slab with records
        self.cum = [np.zeros(1, np.int64)]          # per slab: the members' offsets from the slab's first, one more than members
        self.runs = []
        self.n_chunks = self.n_references = 0

    def add_slab(self, stream_base, file_offset, sizes, raw_bytes, runs):
        """``stream_base``: uncompressed bytes of the slabs in front; ``file_offset``: where the slab's first member lies in
        the file; ``sizes``: its members' compressed sizes; ``raw_bytes``: its bytes before compression; ``runs``: RUN_DTYPE."""
        raw_bytes, sizes = int(raw_bytes), np.asarray(sizes, np.int64)
        if raw_bytes == 0:
            if len(runs) or len(sizes):
                raise ValueError("a slab without bytes has neither members nor runs")
            return
        if len(sizes) != (raw_bytes + MEMBER_BYTES - 1) // MEMBER_BYTES:
            raise ValueError("%d bytes in members of %d make %d members, not %d"
                             % (raw_bytes, MEMBER_BYTES, (raw_bytes + MEMBER_BYTES - 1) // MEMBER_BYTES, len(sizes)))
        if self.bases and int(stream_base) != self.bases[-1] + self.raws[-1]:
            raise ValueError("the slab's stream does not begin where the one in front ended")
        self.first_member.append(sum(len(c) for c in self.cum[1:]))
        self.bases.append(int(stream_base))
        self.raws.append(raw_bytes)
        self.file_offsets.append(int(file_offset))
        self.cum.append(np.concatenate([[0], np.cumsum(sizes)]))
        runs = np.array(runs, RUN_DTYPE)
        if len(runs) == 0:
            raise ValueError("a slab with bytes has runs")
        if self.runs and self.runs[-1]["tid"][-1] == runs["tid"][0] and self.runs[-1]["bin"][-1] == runs["bin"][0]:
            # the run goes on across the slab border: one chunk
            last = self.runs[-1]
            last["uend"][-1] = runs["uend"][0]
            last["last"][-1] += runs["last"][0] - runs["first"][0]
            runs = runs[1:]
        # (first / last are ranks within a slab: from here on only their difference, the run's records, counts)
        if len(runs):
            self.runs.append(runs)

    def virtual(self, offsets, end=False):
        """Stream offsets to virtual file offsets; ``end``: offsets of the byte behind a record's last one, which at the end
        of a member are the next member's first byte (also the next slab's, or the end-of-file marker's)."""
        u = np.asarray(offsets, np.uint64).astype(np.int64)
        if len(u) == 0:
            return np.zeros(0, np.uint64)
        bases = np.asarray(self.bases, np.int64)
        k = np.searchsorted(bases, u, side="left" if end else "right") - 1
        if (k < 0).any():
            raise ValueError("an offset in front of the first slab")
        x = u - bases[k]
        raws = np.asarray(self.raws, np.int64)[k]
        if (x > raws).any() or (not end and (x >= raws).any()):
            raise ValueError("an offset behind its slab's last byte")
        member, within = x // MEMBER_BYTES, x % MEMBER_BYTES
        if end:
            at_end = x == raws
            member = np.where(at_end, (raws + MEMBER_BYTES - 1) // MEMBER_BYTES, member)
            within = np.where(at_end, 0, within)
        cum = np.concatenate(self.cum[1:])
        coffset = np.asarray(self.file_offsets, np.int64)[k] + cum[np.asarray(self.first_member, np.int64)[k] + member]
        return (coffset.astype(np.uint64) << np.uint64(16)) | within.astype(np.uint64)

    def finish(self, linear):
        """The BAI file: ``linear`` = the device's linear index (``linear_windows`` words per sequence, UNTOUCHED for none)."""
        windows = linear_windows(self.lengths)
        linear = np.asarray(linear, np.uint64)
        if len(linear) != sum(windows):
            raise ValueError("the linear index has %d words, the header's sequences %d windows" % (len(linear), sum(windows)))
        runs = np.concatenate(self.runs) if self.runs else np.zeros(0, RUN_DTYPE)
        beg, end = self.virtual(runs["ustart"]), self.virtual(runs["uend"], end=True)
        count = runs["last"].astype(np.int64) - runs["first"].astype(np.int64)
        if len(runs) and ((np.diff(runs["tid"]) < 0).any() or runs["tid"][0] < 0 or runs["tid"][-1] >= len(self.lengths)):
            raise ValueError("the runs are not in the order of the header's sequences")
        edges = np.searchsorted(runs["tid"], np.arange(len(self.lengths) + 1))
        out = [b"BAI\x01", struct.pack("<i", len(self.lengths))]
        self.n_chunks, self.n_references = len(runs), 0
        w0 = 0
        for tid, n_win in enumerate(windows):
            lo, hi = int(edges[tid]), int(edges[tid + 1])
            if hi > lo:
                self.n_references += 1
                out.append(_bins(runs["bin"][lo:hi], beg[lo:hi], end[lo:hi], int(count[lo:hi].sum())))
            else:
                out.append(struct.pack("<i", 0))
            seg = linear[w0:w0 + n_win]
            w0 += n_win
            touched = np.flatnonzero(seg != UNTOUCHED)
            if (hi > lo) != bool(len(touched)):
                raise ValueError("sequence %d has %s" % (tid, "runs and no window" if hi > lo else "windows and no run"))
            if len(touched) == 0:
                out.append(struct.pack("<i", 0))
                continue
            n_intv = int(touched[-1]) + 1
            values = self.virtual(seg[touched])
            # (an untouched window takes the next touched one above it)
            filled = values[np.searchsorted(touched, np.arange(n_intv), side="left")]
            out.append(struct.pack("<i", n_intv) + filled.astype("<u8").tobytes())
        out.append(struct.pack("<Q", 0))
        return b"".join(out)


def _bins(bins, beg, end, n_mapped):
    """One sequence's bins: ascending, each with its chunks in file order, the pseudo-bin last."""
    order = np.argsort(bins, kind="stable")
    b, s, e = bins[order], beg[order], end[order]
    unique, first, counts = np.unique(b, return_index=True, return_counts=True)
    rank = np.repeat(np.arange(len(unique)), counts)
    words = np.zeros(2 * len(unique) + 4 * len(b), "<u4")
    head = 2 * np.arange(len(unique)) + 4 * first
    words[head], words[head + 1] = unique, counts
    at = 2 * (rank + 1) + 4 * np.arange(len(b))
    words[at], words[at + 1] = s & np.uint64(0xFFFFFFFF), s >> np.uint64(32)
    words[at + 2], words[at + 3] = e & np.uint64(0xFFFFFFFF), e >> np.uint64(32)
    pseudo = struct.pack("<IiQQQQ", PSEUDO_BIN, 2, int(beg[0]), int(end[-1]), n_mapped, 0)
    return struct.pack("<i", len(unique) + 1) + words.tobytes() + pseudo
