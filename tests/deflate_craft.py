"""Raw DEFLATE streams (RFC 1951) written bit by bit, for the decoder of the GPU decode path (mapdamage_amd/csrc/mdx_inflate.h).
A compressor chooses its blocks, codes and matches from the data; here the caller chooses them, so that the streams are the
ones zlib never writes and the format allows: any complete prefix code over the symbols a block uses (deep, flat, random,
1-bit and 15-bit codes), HLIT / HDIST / HCLEN above their minimum, code lengths written plainly or with 16 / 17 / 18 in any
legal way, matches of chosen (length, distance), length 258 as symbol 284 with extra bits 31, empty blocks, any padding.
Deterministic from a seed; numpy and the standard library only.  Collects no tests: tests/test_deflate_craft.py checks the
streams themselves against zlib and runs the decoder's host build over them (no GPU), tests/test_gpu_inflate_craft.py runs
them through the device build.

Every stream comes with the bytes it must inflate to (None: built to be refused) and with counts of what it contains
(``Case.stats``, ``Case.pairs``), taken while it is written: the tests assert their coverage on those.

The directed cases are placed by the constants of mdx_inflate.h, restated below."""
import collections
import functools
import random

import numpy as np

RING, SEG, FAST_LL, FAST_D, STRETCH = 4096, 2048, 11, 8, 512
CAP = 65536                                         # a BGZF block's output

ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LBASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEXT = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DBASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577)
DEXT = (0, 0, 0, 0) + tuple(i // 2 for i in range(2, 28))
LSYM = [0] * 259
for _s in range(28):
    for _v in range(LBASE[_s], LBASE[_s] + (1 << LEXT[_s])):
        if _v <= 258:
            LSYM[_v] = _s
LSYM[258] = 28
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32

MATCH_LENS = (3, 63, 64, 65, 128, 129, 257, 258)
BAND = tuple(sorted(set(range(RING - 258, RING + 259, 47)) | {RING - 1, RING, RING + 1, RING + 258}))
FAR = (8192, 8193, 32767, 32768)


def dsym_of(dist):
    s = 29
    while DBASE[s] > dist:
        s -= 1
    return s


def directed_distances(length):
    """The distances the matches theme crosses a length with (the far ones apart: they need 32 KiB of history)."""
    near = {1, 2, 3, 63, 64, 65, length - 1, length, length + 1, 2047, 2048, 2049} | set(BAND)
    return sorted(d for d in near if d >= 1)


# ------------------------------------------------------------------------------------------------ prefix codes
def complete_lengths(n, maxlen, shape, rng):
    """The code lengths, ascending, of a complete prefix code of n symbols no longer than maxlen bits: a tree grown by
    splitting its deepest ('deep'), shallowest ('flat') or a random leaf.  One symbol: a single 1-bit code."""
    if n == 1:
        return [1]
    assert 2 <= n <= (1 << maxlen)
    cnt = [0] * (maxlen + 2)
    cnt[1] = 2
    for _ in range(n - 2):
        cand = [ln for ln in range(1, maxlen) if cnt[ln]]
        ln = max(cand) if shape == "deep" else (min(cand) if shape == "flat" else rng.choice(cand))
        cnt[ln] -= 1
        cnt[ln + 1] += 2
    return [ln for ln in range(1, maxlen + 1) for _ in range(cnt[ln])]


def complete_with(fixed, fillers, deep=True, size=None):
    """{symbol: length} for the symbols of `fixed` as given plus every symbol of `fillers`, which share what the fixed
    ones leave of the code space: the first filler gets the shortest code.  The set is complete."""
    left = (1 << 15) - sum(1 << (15 - ln) for ln in fixed.values())
    assert left > 0 and fillers
    terms = [15 - b for b in range(15, -1, -1) if (left >> b) & 1]
    assert len(terms) <= len(fillers), (terms, fillers)
    while len(terms) < len(fillers):
        cand = [ln for ln in terms if ln < 15]
        ln = max(cand) if deep else min(cand)
        terms.remove(ln)
        terms += [ln + 1, ln + 1]
    out = dict(fixed)
    out.update(zip(fillers, sorted(terms)))
    return as_lens(out, size)


def as_lens(by_symbol, size=None):
    lens = [0] * (size if size is not None else max(by_symbol) + 1)
    for s, ln in by_symbol.items():
        lens[s] = ln
    return lens


def kraft(lens):
    """the code space the lengths take, in units of 2**-15 (complete: 32768)"""
    return sum(1 << (15 - ln) for ln in lens if ln)


def canonical(lens):
    """(code, written LSB first) per symbol, RFC 1951 3.2.2; an over-subscribed set gets codes all the same (nobody reads them)"""
    count = [0] * 17
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for ln in range(1, 16):
        code = (code + count[ln - 1]) << 1
        nxt[ln] = code
    out = [0] * len(lens)
    for s, ln in enumerate(lens):
        if ln:
            c = nxt[ln] & ((1 << ln) - 1)
            nxt[ln] += 1
            out[s] = int(format(c, "0%db" % ln)[::-1], 2)
    return out


# ------------------------------------------------------------------------------------------------ the writer
class Case:
    """One stream.  ``theme`` / ``label``: what it is for; ``stream``: the raw DEFLATE bytes; ``expected``: the bytes it
    inflates to, None for a stream built to be refused; ``size``: the ISIZE to declare for it on the device (the bytes
    of `expected`, or of the valid stream it was derived from); ``stats`` / ``pairs``: what the writer counted."""

    def __init__(self, theme, label, stream, expected, stats=None, pairs=(), size=None):
        self.theme, self.label, self.stream, self.expected = theme, label, bytes(stream), expected
        self.stats = stats if stats is not None else collections.Counter()
        self.pairs = frozenset(pairs)
        self.size = size if size is not None else (len(expected) if expected is not None else 1)

    def __repr__(self):
        return "Case(%s, %s)" % (self.theme, self.label)


class Stream:
    """A DEFLATE stream under construction: blocks are appended with stored() / fixed() / dynamic(), finish() pads the last
    byte.  Tokens: an int is a literal, (length, distance) a match — (258, distance, True) writes the length as symbol 284
    with extra bits 31 —, and, for streams that are to be refused, ("ll", symbol) / ("d", symbol) write that symbol's code
    and ("bits", value, n) n raw bits; those three leave `out` alone."""

    def __init__(self, rng=None):
        self.rng = rng or random.Random(0)
        self.buf, self.acc, self.n = bytearray(), 0, 0
        self.out = bytearray()
        self.stats = collections.Counter()
        self.pairs = set()
        self.blocks = []                         # (kind, bytes it carries)
        self.prev = None                         # the token before: "far", "stored", None (anything else)

    # -- bits
    def put(self, v, k):
        self.acc |= v << self.n
        self.n += k
        if self.n >= 32:
            self.buf += (self.acc & 0xFFFFFFFF).to_bytes(4, "little")
            self.acc >>= 32
            self.n -= 32

    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def _to_byte(self, fill):
        k = -self.n % 8
        self.put(fill & ((1 << k) - 1), k)
        while self.n:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return k

    def _crossings(self, what, a, b):
        for at in (STRETCH, 2 * STRETCH):
            if a < 8 * at < b:
                self.stats["x%d_%s" % (at, what)] += 1

    # -- blocks
    def stored(self, data, last=False, pad=0, len_field=None, nlen_field=None):
        self.put(int(last), 1)
        self.put(0, 2)
        self._to_byte(pad)
        at = len(self.buf)
        if at < STRETCH < at + 4:
            self.stats["stored_len_words_straddle_512"] += 1
        ln = len(data) if len_field is None else len_field
        self.buf += ln.to_bytes(2, "little") + ((ln ^ 0xFFFF) if nlen_field is None else nlen_field).to_bytes(2, "little")
        self.buf += data
        self.out += data
        self.blocks.append(("stored", len(data)))
        self.stats["stored_blocks"] += 1
        if data:
            self.prev = "stored"
        return self

    def fixed(self, tokens, last=False):
        self.put(int(last), 1)
        self.put(1, 2)
        before = len(self.out)
        self._tokens(tokens, FIXED_LL, FIXED_D)
        self.blocks.append(("fixed", len(self.out) - before))
        self.stats["fixed_blocks"] += 1
        return self

    def dynamic(self, tokens, ll_lens, d_lens, last=False, hlit=None, hdist=None, hclen=None, cl_mode="greedy", cl_shape="random",
                cl_lens=None, cl_syms=None, hlit_field=None, hdist_field=None, eob=True):
        """ll_lens / d_lens: code lengths by symbol (trailing zeros may be left out); hlit / hdist / hclen: how many
        lengths the header carries (default: as few as the format allows); cl_mode: 'plain', 'greedy', 'zero16' or
        'random' (rle()); cl_lens: the code-length code (default: a complete code over the symbols rle() used, of shape
        cl_shape); cl_syms: the (symbol, extra bits) sequence itself in place of rle()'s."""
        st, rng = self.stats, self.rng
        start = self.bitpos()
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        min_hlit = max(257, max((s + 1 for s, ln in enumerate(ll_lens) if ln), default=257))
        min_hdist = max(1, max((s + 1 for s, ln in enumerate(d_lens) if ln), default=1))
        hlit = min_hlit if hlit is None else hlit
        hdist = min_hdist if hdist is None else hdist
        assert hlit >= min_hlit and hdist >= min_hdist
        ll = (ll_lens + [0] * hlit)[:hlit]
        dd = (d_lens + [0] * hdist)[:hdist]
        if cl_syms is None:
            cl_syms = rle(ll + dd, cl_mode, rng)
        used = sorted({s for s, _ in cl_syms})
        if cl_lens is None:
            # (a lone symbol takes a partner: zlib wants the code-length code complete)
            alphabet = used if len(used) > 1 else used + [s for s in (0, 18) if s not in used][:1]
            lens = complete_lengths(len(alphabet), 7, cl_shape, rng)
            rng.shuffle(lens)
            cl_lens = as_lens(dict(zip(alphabet, lens)), 19)
        min_hclen = max(4, max(i + 1 for i, s in enumerate(ORDER) if cl_lens[s]))
        hclen = min_hclen if hclen is None else hclen
        assert min_hclen <= hclen <= 19
        self.put(int(last), 1)
        self.put(2, 2)
        self.put((hlit - 257) if hlit_field is None else hlit_field, 5)
        self.put((hdist - 1) if hdist_field is None else hdist_field, 5)
        self.put(hclen - 4, 4)
        a = self.bitpos()
        self._crossings("hdr_fields", start, a)
        for i in range(hclen):
            self.put(cl_lens[ORDER[i]], 3)
        b = self.bitpos()
        self._crossings("cl_lens", a, b)
        codes = canonical(cl_lens)
        at, before16 = 0, None
        for s, extra in cl_syms:
            self.put(codes[s], cl_lens[s])
            if s < 16:
                at += 1
            else:
                rep = extra + (3 if s < 18 else 11)
                self.put(extra, (2, 3, 7)[s - 16])
                if s == 16:
                    st["rep16"] += 1
                    if at < hlit < at + rep:
                        st["rep16_crosses_into_distances"] += 1
                    if before16 in (17, 18):
                        st["rep16_after_1718"] += 1
                elif at < hlit < at + rep:
                    st["rep1718_crosses_into_distances"] += 1
                if s == 18 and rep == 138:
                    st["rep18_138"] += 1
                at += rep
            before16 = s
        c = self.bitpos()
        self._crossings("code_lens", b, c)
        st["dynamic_blocks"] += 1
        st["hlit_%d" % hlit] += 1
        st["hdist_%d" % hdist] += 1
        st["hclen_%d" % hclen] += 1
        st["hlit_above_min"] += hlit > min_hlit
        st["hdist_above_min"] += hdist > min_hdist
        st["hclen_above_min"] += hclen > min_hclen
        st["header_no_repeat"] += all(s < 16 for s, _ in cl_syms)
        nd = sum(1 for ln in dd if ln)
        st["no_distance_code"] += nd == 0 and hdist == 1
        st["single_distance_code_len1"] += nd == 1 and max(dd) == 1
        before = len(self.out)
        self._tokens(tokens, ll, dd, eob)
        self._crossings("tokens", c, self.bitpos())
        self.blocks.append(("dynamic", len(self.out) - before))
        return self

    def _tokens(self, tokens, ll_lens, d_lens, eob=True):
        st, out, put = self.stats, self.out, self.put
        llc, dc = canonical(ll_lens), canonical(d_lens)
        block_start = len(out)
        lit_lo, lit_hi, run = 99, 0, 0           # shortest and longest literal code used; literals with a code in the fast table in a row
        prev = self.prev

        def follower(kind):
            if run <= 9:
                st["run%d_%s" % (run, kind)] += 1

        for i, t in enumerate(tokens):
            if type(t) is int:
                ln = ll_lens[t]
                assert ln, ("literal without a code", t)
                put(llc[t], ln)
                out.append(t)
                lit_lo, lit_hi = min(lit_lo, ln), max(lit_hi, ln)
                if ln <= FAST_LL:
                    run += 1
                else:
                    follower("longlit")
                    run = 0
                prev = None
                continue
            if t[0] == "ll":
                put(llc[t[1]], ll_lens[t[1]])
                continue
            if t[0] == "d":
                put(dc[t[1]], d_lens[t[1]])
                continue
            if t[0] == "bits":
                put(t[1], t[2])
                continue
            length, dist = t[0], t[1]
            alt = len(t) > 2 and t[2]
            ls = 27 if alt else LSYM[length]
            assert 3 <= length <= 258 and 1 <= dist <= 32768 and (not alt or length == 258)
            ln = ll_lens[257 + ls]
            assert ln, ("length symbol without a code", 257 + ls)
            put(llc[257 + ls], ln)
            ex = length - LBASE[ls]
            put(ex, LEXT[ls])
            ds = dsym_of(dist)
            assert d_lens[ds], ("distance symbol without a code", ds)
            put(dc[ds], d_lens[ds])
            dx = dist - DBASE[ds]
            put(dx, DEXT[ds])
            follower("shortlen" if ln <= FAST_LL else "longlen")
            ran, run = run, 0
            st["alt258"] += bool(alt)
            if LEXT[ls] + d_lens[ds] + DEXT[ds] == 33:       # the longest a pair gets behind its length code: 5 + 15 + 13 bits
                st["run%d_longest_pair_behind_code_%d" % (min(ran, 9), ln)] += 1
            st["len_code_%d" % ln] += 1
            st["dist_code_%d" % d_lens[ds]] += 1
            if ex == 0:
                st["L%d_min" % ls] += 1
            if ex == (1 << LEXT[ls]) - 1:
                st["L%d_max" % ls] += 1
            if dx == 0:
                st["D%d_min" % ds] += 1
            if dx == (1 << DEXT[ds]) - 1:
                st["D%d_max" % ds] += 1
            o = len(out)
            far = dist > RING
            st["matches"] += 1
            st["m_far"] += far
            st["m_band"] += RING - 258 < dist <= RING
            st["m_short_period_long"] += dist < 64 and length > 64
            st["m_overlap_64"] += 64 <= dist < length
            st["m_one_per_lane"] += length <= 64 and dist >= length
            st["m_straddles_seg"] += o // SEG != (o + length - 1) // SEG
            if far:
                st["far_behind_stored"] += prev == "stored" and i == 0
                st["far_behind_far"] += prev == "far"
                st["far_source_of_same_block"] += o - dist >= block_start and o // SEG > block_start // SEG
            self.pairs.add((length, dist))
            if dist <= o:
                if dist >= length:
                    out += out[o - dist:o - dist + length]
                else:
                    out += (out[o - dist:] * (length // dist + 1))[:length]
            else:
                st["distance_too_far"] += 1      # (a stream to be refused)
            prev = "far" if far else None
        if eob:
            ln = ll_lens[256]
            put(llc[256], ln)
            follower("eob")
            st["eob_code_%d" % ln] += 1
        if lit_hi:
            st["blk_lit_ge12"] += lit_hi >= 12
            st["blk_lit_le2"] += lit_hi <= 2
            st["blk_lit_all11"] += lit_lo == lit_hi == 11
            st["blk_lit_15"] += lit_hi == 15
            st["blk_lit_both_sides_of_fast_table"] += lit_lo <= FAST_LL < lit_hi
        self.prev = prev

    def finish(self, pad=0):
        k = self._to_byte(pad)
        st = self.stats
        st["ends_on_byte"] += k == 0
        st["pad_all_ones"] += k > 0 and (pad & ((1 << k) - 1)) == (1 << k) - 1
        st["blocks_%d" % len(self.blocks)] += 1
        st["mixed_kinds"] += len({k for k, _ in self.blocks}) > 1
        for i, (kind, n) in enumerate(self.blocks):
            if n == 0 and any(m for _, m in self.blocks[:i]) and any(m for _, m in self.blocks[i + 1:]):
                st["empty_%s_between" % kind] += 1
        return bytes(self.buf), bytes(self.out)

    def case(self, theme, label, pad=0, valid=True, size=None):
        stream, out = self.finish(pad)
        return Case(theme, label, stream, out if valid else None, self.stats, self.pairs, size if size is not None else max(1, len(out)))


def rle(lens, mode, rng):
    """The (code-length symbol, extra bits) sequence for `lens`: 'plain' writes every length itself, 'greedy' repeats as
    long as it can, 'zero16' continues a run of zeros begun by 17 / 18 with 16s, 'random' picks any legal way."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, r = lens[i], 1
        while i + r < n and lens[i + r] == v:
            r += 1
        i += r
        fresh = True                             # nothing of this run written yet: 16 would repeat the run in front
        while r:
            opts = {"p": 1}
            if v == 0 and r >= 3:
                opts[17] = min(r, 10)
            if v == 0 and r >= 11:
                opts[18] = min(r, 138)
            if not fresh and r >= 3:
                opts[16] = min(r, 6)
            if mode == "plain":
                how = "p"
            elif mode == "greedy":
                how = 18 if 18 in opts else (17 if 17 in opts else (16 if 16 in opts else "p"))
            elif mode == "zero16":
                how = 16 if 16 in opts else (18 if 18 in opts else (17 if 17 in opts else "p"))
                if how in (17, 18) and r - 3 >= {17: 3, 18: 11}[how]:
                    opts[how] = min(opts[how], r - 3)     # (leave three for a 16)
            else:
                how = rng.choice(sorted(opts, key=str))
                if how != "p":
                    opts[how] = rng.randint({16: 3, 17: 3, 18: 11}[how], opts[how])
            k = opts[how]
            out.append((v, 0) if how == "p" else (how, k - (11 if how == 18 else 3)))
            r -= k
            fresh = False
    return out


# ------------------------------------------------------------------------------------------------ helpers of the cases
def _bytes(rng, n):
    return bytes(np.random.default_rng(rng.getrandbits(32)).integers(0, 256, n, dtype=np.uint8))


def _code_for(tokens, rng, shape="random", maxlen=15, extra_ll=0, extra_d=0, long_literals=False, fixed_ll=None):
    """(ll_lens, d_lens): complete codes over the symbols the tokens use (and the end-of-block code, and `extra_*` symbols
    nobody uses).  long_literals: the longest codes go to literals."""
    lits = sorted({t for t in tokens if type(t) is int})
    lsyms = sorted({257 + (27 if len(t) > 2 and t[2] else LSYM[t[0]]) for t in tokens if type(t) is tuple and type(t[0]) is int})
    dsyms = sorted({dsym_of(t[1]) for t in tokens if type(t) is tuple and type(t[0]) is int})
    syms = lits + [256] + lsyms
    free = [s for s in range(286) if s not in set(syms)]
    rng.shuffle(free)
    syms += free[:extra_ll]
    if fixed_ll is not None:
        ll = complete_with(fixed_ll, [s for s in syms if s not in fixed_ll], deep=shape == "deep", size=286)
    else:
        lens = complete_lengths(len(syms), max(maxlen, (len(syms) - 1).bit_length()), shape, rng)
        if long_literals:
            unused, others = free[:extra_ll], [256] + lsyms
            rng.shuffle(others)
            rng.shuffle(lits)
            order = others + unused + lits                                  # ascending lengths
        else:
            order = list(syms)
            rng.shuffle(order)
        ll = as_lens(dict(zip(order, lens)), 286)
    dfree = [s for s in range(30) if s not in set(dsyms)]
    rng.shuffle(dfree)
    dsyms = dsyms + dfree[:extra_d]
    if dsyms:
        lens = complete_lengths(len(dsyms), max(min(maxlen, 15), (len(dsyms) - 1).bit_length()), shape, rng)
        rng.shuffle(lens)
        dl = as_lens(dict(zip(dsyms, lens)), 30)
    else:
        dl = [0]
    return ll, dl


def _dyn(s, tokens, rng, last=False, **kw):
    hdr = {k: kw.pop(k) for k in ("hlit", "hdist", "hclen", "cl_mode", "cl_shape") if k in kw}
    ll, dl = _code_for(tokens, rng, **kw)
    return s.dynamic(tokens, ll, dl, last=last, **hdr)


# ------------------------------------------------------------------------------------------------ directed: literal runs
@functools.lru_cache(maxsize=None)
def literal_runs():
    rng = random.Random(101)
    cases = []
    A, B, C, D = 65, 67, 71, 84

    def runs_code(short):
        # two literals with `short`-bit codes (1 and 2, or 2 and 2), a length symbol and end-of-block with short codes, and a
        # chain down to 15 bits that holds a literal and length symbols with 12- to 15-bit codes
        fixed = {A: short[0], B: short[1]}
        fillers = [257, 256, 259, 260, 261, 262, 263, 264, 265, 266, 267, 258, 270, C, 284]      # ascending lengths
        return complete_with(fixed, fillers, deep=True, size=286)

    for short in ((1, 2), (2, 2)):
        ll = runs_code(short)
        assert ll[C] >= 12 and ll[258] >= 12 and ll[270] >= 12 and ll[284] >= 12 and ll[257] <= 4
        dl = as_lens({0: 1, 3: 2, 9: 2}, 30)
        for phase in range(3):
            s = Stream(rng)
            s.stored(_bytes(rng, 300))
            for n in range(1, 10):
                toks = [C] * phase
                for kind in ("longlit", "shortlen", "longlen", "longlen258", "eob"):
                    toks += [rng.choice((A, B)) for _ in range(n)]
                    if kind == "longlit":
                        toks.append(C)
                    elif kind == "shortlen":
                        toks.append((3, rng.choice((1, 4, 30))))
                    elif kind == "longlen":
                        toks.append((rng.choice((4, 23, 26)), rng.choice((1, 4, 25, 32))))
                    elif kind == "longlen258":
                        toks.append((258, 4, True))
                s.dynamic(toks, ll, dl, last=n == 9)
            cases.append(s.case("literal_runs", "runs 1..9 of %s-bit literals, phase %d" % ("/".join(map(str, short)), phase), pad=phase))
    # the longest symbol pair — a length with five extra bits, a 15-bit distance code, thirteen extra bits: 33 bits behind
    # the length code — behind runs of 0 .. 9 literals of 2 and 3 bits, its length code 9, 10, 11 (fast table) or 13 bits
    fixed = {A: 2, B: 2, C: 2, 282: 9, 283: 10, 284: 11}
    ll = complete_with(fixed, [D, 256, 257, 258, 259, 260, 261, 281, 285], deep=True, size=286)
    assert ll[D] == 3 and ll[281] == 13
    dl = as_lens(dict(zip([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 28, 29], complete_lengths(16, 15, "deep", rng))), 30)
    for phase in range(4):
        s = Stream(rng)
        s.stored(_bytes(rng, 32768))
        toks = [D] * phase
        for n in range(10):
            for sym, base in ((282, 163), (283, 195), (284, 227), (281, 131)):
                toks += [rng.choice((A, B, C, D)) for _ in range(n)]
                toks.append((base + rng.choice((0, 15, 30)), rng.choice((16385, 24576, 24577, 32768))))
        s.dynamic(toks, ll, dl, last=True)
        cases.append(s.case("literal_runs", "the longest symbol pair behind runs of 0..9 literals, phase %d" % phase, pad=phase * 37))
    # all literals on 1- and 2-bit codes: seven of them in 7 .. 14 bits
    for fixed in ({A: 1, B: 2}, {A: 2, B: 2, C: 2}, {A: 1}, {A: 2, B: 2}):
        s = Stream(rng)
        lits = list(fixed)
        toks = []
        for _ in range(40):
            toks += [rng.choice(lits) for _ in range(rng.randint(1, 30))]
            toks.append((rng.choice((3, 4, 10, 70)), rng.choice((1, 2, 5))))
        _dyn(s, toks, rng, fixed_ll=fixed, shape="deep")
        s.dynamic([lits[0]] * 64 + [(258, 1)] * 30, complete_with(fixed, [285, 256], size=286), [1], last=True)
        cases.append(s.case("literal_runs", "literals of %s bits only" % sorted(fixed.values())))
    # all literals exactly 11 bits; literals alternating 11 and 12 bits, the 12-bit one at every position of the run
    ll11 = complete_with({b: 11 for b in range(256)}, [256, 257, 258], size=286)
    s = Stream(rng)
    data = list(_bytes(rng, 1500))
    s.dynamic(data[:700] + [(3, 2)] + data[700:], ll11, [1, 1], last=True)
    cases.append(s.case("literal_runs", "every literal 11 bits"))
    fixed = {b: 11 for b in range(128)}
    fixed.update({b: 12 for b in range(128, 256)})
    ll1112 = complete_with(fixed, [256, 257, 258, 259], size=286)
    s = Stream(rng)
    toks = []
    for rep in range(6):
        for p in range(8):
            toks += [rng.randrange(128) for _ in range(p)] + [128 + rng.randrange(128)]
            if rep % 2:
                toks.append((rng.choice((3, 4, 5)), rng.choice((1, 2))))
    s.dynamic(toks, ll1112, [1, 1], last=False)
    s.dynamic([rng.randrange(256) for _ in range(900)], ll1112, [0], last=True)
    cases.append(s.case("literal_runs", "literals of 11 and 12 bits in turn"))
    # 15-bit literals; end-of-block on 1 bit and on 15 bits
    chain = list(range(1, 15)) + [15, 15]
    for eob_len in (1, 15):
        syms = [257, 258, 259, 260, 261, 262, 263, 264, 265, 266, 267, 268, 269, 270]       # 1 .. 14 bits
        by = dict(zip(syms, chain[:14]))
        by[A], by[B] = 15, 15
        if eob_len == 1:
            by[256], by[257] = 1, 15
            del by[B]
        else:
            by[256] = 15
            del by[B]
            by[257] = 1
        ll = as_lens(by, 286)
        assert kraft(ll) == 1 << 15
        s = Stream(rng)
        s.dynamic([A] * 9 + [(3, 1), A, (4, 2), A, A, (10, 3)], ll, [2, 2, 2, 2], last=False)
        s.dynamic([A, A, A], ll, [0], last=False)
        s.dynamic([A] * 40 + [(258, 1)] * 20, complete_with({A: 15}, [256, 285] + list(range(14)), size=286), [1], last=True)
        cases.append(s.case("literal_runs", "15-bit literals, end-of-block on %d bit%s" % (eob_len, "s" * (eob_len > 1)), pad=0x7F))
    # an alphabet of all 256 literals, deep: literals on both sides of the fast table in one block
    for shape in ("deep", "random", "flat"):
        s = Stream(rng)
        toks = list(_bytes(rng, 2500))
        for at in range(100, 2400, 97):
            toks.insert(at, (rng.choice((3, 9, 40)), rng.choice((1, 7, 90))))
        _dyn(s, toks, rng, last=True, shape=shape, long_literals=shape == "deep")
        cases.append(s.case("literal_runs", "256 literals, %s code" % shape))
    return tuple(cases)


# ------------------------------------------------------------------------------------------------ directed: matches and the ring
def _match_block(s, matches, rng, kind, last=True, shape="random"):
    toks = []
    for m in matches:
        toks += [rng.randrange(256) for _ in range(rng.choice((0, 1, 1, 2, 5)))]
        toks.append(m)
    toks += [rng.randrange(256) for _ in range(3)]
    if kind == "fixed":
        s.fixed(toks, last=last)
    else:
        _dyn(s, toks, rng, last=last, shape=shape, maxlen=rng.choice((9, 12, 15)))
    return s


@functools.lru_cache(maxsize=None)
def matches():
    rng = random.Random(202)
    cases = []
    for li, length in enumerate(MATCH_LENS):
        for rep, kind in enumerate(("fixed", "dynamic")):
            s = Stream(rng)
            s.stored(_bytes(rng, RING + 300 + 517 * rep + 129 * li))
            ms = [(length, d) for d in directed_distances(length)]
            rng.shuffle(ms)
            if length == 258:
                ms = [m + (True,) if i % 3 == 0 else m for i, m in enumerate(ms)]
            _match_block(s, ms, rng, kind)
            cases.append(s.case("matches", "length %d at every near distance, %s block" % (length, kind), pad=rng.getrandbits(7)))
    # the far ones: 32 KiB of history first
    for kind in ("fixed", "dynamic"):
        s = Stream(rng)
        s.stored(_bytes(rng, 32768))
        ms = [(ln, d) for ln in MATCH_LENS for d in FAR]
        rng.shuffle(ms)
        _match_block(s, ms, rng, kind, shape="deep")
        cases.append(s.case("matches", "every length at 8192 .. 32768, %s block" % kind))
    # every length and distance symbol at both ends of its extra bits (distance 32768 = symbol 29, thirteen one-bits)
    for kind in ("fixed", "dynamic"):
        s = Stream(rng)
        s.stored(_bytes(rng, 32768))
        ms = [(LBASE[i], 300 + i) for i in range(29)] + [(min(258, LBASE[i] + (1 << LEXT[i]) - 1), 700 + i) for i in range(28)]
        ms += [(258, 5, True)] + [(3, DBASE[i]) for i in range(30)] + [(4, DBASE[i] + (1 << DEXT[i]) - 1) for i in range(30)]
        rng.shuffle(ms)
        _match_block(s, ms, rng, kind, shape="deep")
        cases.append(s.case("matches", "every length and distance symbol, least and most extra bits, %s block" % kind))
    # 15-bit distance codes: all thirty in a deep code
    s = Stream(rng)
    s.stored(_bytes(rng, 5000))
    toks = [(3 + i, DBASE[i] if DBASE[i] <= 5000 else 1 + i) for i in range(30)]
    dl = complete_lengths(30, 15, "deep", rng)
    ll, _ = _code_for(toks, rng)
    s.dynamic(toks, ll, dl[::-1], last=True)
    assert s.stats["dist_code_15"]
    cases.append(s.case("matches", "distance codes of 15 bits"))
    # destinations across a multiple of SEG
    for j in (1, 2, 15, 16, 63, 64, 65, 257):
        s = Stream(rng)
        s.stored(_bytes(rng, 3 * SEG - j - 2))
        s.fixed([7, 8, (258, 1), (258, 100), (200, SEG), (258, SEG - 1), (258, RING), (258, RING + 1), (64, 64), (65, 64)], last=True)
        cases.append(s.case("matches", "match written across a multiple of %d, %d bytes in front of it" % (SEG, j)))
    # far matches right behind a stored block, behind one another, and into what the same block produced
    for dist in (RING + 1, 5000, 9000):
        s = Stream(rng)
        s.stored(_bytes(rng, dist + 40))
        toks = [(100, dist), (258, dist + 7), (3, dist), 9, (70, dist - 800)]
        toks += [rng.randrange(256) for _ in range(300)] + [(258, 1)] * 20 + [(258, 5300), (258, 5300), (40, RING + 1), (258, RING + 258)]
        _dyn(s, toks, rng, last=False, shape="flat")
        s.stored(_bytes(rng, 100))
        s.fixed([(258, RING + 2), (258, RING + 3)], last=True)
        cases.append(s.case("matches", "far matches behind a stored block and behind one another, distance %d" % dist))
    # the output bound: 65536 bytes that end in a 258-byte match; one literal more is a block too long
    for more in (0, 1):
        s = Stream(rng)
        s.stored(_bytes(rng, 40000))
        s.stored(_bytes(rng, 20000))
        n = CAP - 60000 - 258 - 3 * 258
        s.fixed([rng.randrange(256) for _ in range(n)] + [(258, 30000), (258, 1), (258, 70), (258, 4500)] + [5] * more, last=True)
        c = s.case("matches", "65536 bytes ending in a match" + ", and one literal" * more, valid=not more, size=CAP)
        assert len(s.out) == CAP + more
        cases.append(c)
    return tuple(cases)


# ------------------------------------------------------------------------------------------------ directed: headers and block structure
@functools.lru_cache(maxsize=None)
def headers():
    rng = random.Random(303)
    cases = []
    text = [rng.choice(b"ACGTN#I") for _ in range(400)]
    for at in range(30, 380, 41):
        text.insert(at, (rng.choice((3, 7, 20)), rng.choice((1, 6, 25))))

    def one(label, **kw):
        s = Stream(rng)
        s.stored(_bytes(rng, 40))
        _dyn(s, text, rng, last=True, **kw)
        cases.append(s.case("headers", label, pad=rng.getrandbits(7)))
        return s

    for hclen in (None, 19):
        for mode in ("plain", "greedy", "zero16", "random"):
            one("HCLEN %s, lengths written %s" % (hclen or "least", mode), hclen=hclen, cl_mode=mode, cl_shape=rng.choice(("deep", "flat", "random")))
    one("HLIT 286, HDIST 30", hlit=286, hdist=30)
    one("HLIT 286, HDIST 30, HCLEN 19, plain", hlit=286, hdist=30, hclen=19, cl_mode="plain")
    one("unused symbols carry codes", extra_ll=150, extra_d=20, cl_mode="random")
    # (HCLEN 4 gives codes to 16, 17, 18 and 0 alone: every length is then zero, the end-of-block code's too, and no such
    # block is valid — it stands among the streams of invalid().  The least HCLEN of a valid block is 5: lengths 8 and 0.)
    ll8 = [0] * 286
    for sym in list(range(255)) + [256]:
        ll8[sym] = 8
    s = Stream(rng)
    s.dynamic(list(_bytes(rng, 300).replace(b"\xff", b"\x00")), ll8, [0], last=True, cl_mode="greedy",
              cl_lens=as_lens({16: 2, 17: 2, 18: 2, 8: 3, 0: 3}, 19))
    assert s.stats["hclen_5"]
    cases.append(s.case("headers", "HCLEN 5: lengths 8 and 0 only"))
    # a 16 that runs from the literal/length lengths into the distance lengths: the last literal/length codes and the first
    # distance codes share a length
    toks = [65, 66, (3, 1), (4, 2), (258, 3, True), (258, 4), 66, (258, 1)]
    by = {65: 2, 66: 2, 256: 2, 257: 3, 258: 4, 284: 5, 285: 5}
    ll = as_lens(by, 286)
    assert kraft(ll) == 1 << 15
    s = Stream(rng)
    s.dynamic(toks, ll, [5] * 28 + [4, 4], last=False, cl_mode="greedy")
    s.dynamic(toks, ll, [2, 2, 2, 2], last=True, hlit=286, cl_mode="random")
    assert s.stats["rep16_crosses_into_distances"]
    cases.append(s.case("headers", "a 16 runs from the literal/length lengths into the distance lengths"))
    # an 18 of 138, a 16 right behind a 17 / 18
    ll = as_lens({0: 1, 256: 2, 257: 2}, 257 + 1)
    s = Stream(rng)
    s.dynamic([0, 0, (3, 1), 0], ll, [1], last=False, cl_mode="greedy")
    s.dynamic([0, 0, (3, 1), 0], ll, [1], last=False, cl_mode="zero16")
    s.dynamic([0, 0, (258, 1), 0], as_lens({0: 1, 256: 2, 285: 2}, 286), [1], last=False, cl_mode="zero16", hdist=30)
    s.dynamic([0] * 5 + [(258, 2)] * 3, as_lens({0: 1, 256: 2, 285: 2}, 286), [0, 1], last=True, cl_mode="random", hdist=30)
    assert s.stats["rep18_138"] and s.stats["rep16_after_1718"]
    cases.append(s.case("headers", "an 18 of 138; a 16 right behind a 17 / 18"))
    # no distance code at all; a single one of 1 bit
    s = Stream(rng)
    s.dynamic([1, 2, 3, 2, 1], as_lens({1: 2, 2: 2, 3: 2, 256: 2}, 257), [0], last=False)
    s.dynamic([1, 2, (7, 2), 2, 1, (258, 2)], as_lens({1: 2, 2: 2, 261: 3, 285: 3, 256: 2}, 286), as_lens({1: 1}, 2), last=False)
    s.dynamic([1, 2, (5, 1), 2, 1, (258, 1)], as_lens({1: 2, 2: 2, 259: 3, 285: 3, 256: 2}, 286), [1], last=True, hdist=30, hlit=286)
    assert s.stats["no_distance_code"] and s.stats["single_distance_code_len1"] == 2
    cases.append(s.case("headers", "no distance code; a single distance code of 1 bit"))
    # empty blocks of every kind, non-final, between blocks that carry data
    lone_eob = as_lens({256: 1}, 257)
    for first in ("stored", "fixed", "dynamic"):
        s = Stream(rng)
        if first == "stored":
            s.stored(_bytes(rng, 700))
        elif first == "fixed":
            s.fixed(list(_bytes(rng, 700)))
        else:
            _dyn(s, text, rng)
        s.dynamic([], lone_eob, [0])
        s.fixed([])
        s.stored(b"", pad=0x55)
        s.dynamic([], as_lens({256: 1, 0: 1}, 257), [1], cl_mode="plain")
        s.stored(b"")
        s.fixed([])
        s.fixed([(200, 350), (258, 1)] + text, last=True)
        cases.append(s.case("headers", "empty blocks of every kind behind a %s block" % first, pad=0x7F))
        assert s.stats["empty_dynamic_between"] == 2 and s.stats["empty_fixed_between"] == 2 and s.stats["empty_stored_between"] == 2
    # 1, 2, 3 and 6 blocks of mixed kinds; final padding all ones; a stream that ends on a byte
    for nb in (1, 2, 3, 6):
        for variant in range(3):
            s = Stream(rng)
            for b in range(nb):
                kind = ("dynamic", "stored", "fixed")[(b + variant) % 3]
                if kind == "stored":
                    s.stored(_bytes(rng, rng.randint(1, 900)), last=b == nb - 1, pad=rng.getrandbits(7))
                elif kind == "fixed":
                    s.fixed(text[:rng.randint(5, 400)], last=b == nb - 1)
                else:
                    _dyn(s, text[:rng.randint(5, 400)], rng, last=b == nb - 1, shape=rng.choice(("deep", "flat", "random")),
                         cl_mode=rng.choice(("plain", "greedy", "zero16", "random")))
            cases.append(s.case("headers", "%d blocks, variant %d" % (nb, variant), pad=0x7F))
    for k in range(16):
        s = Stream(rng)
        s.fixed([65] * k + text, last=True)
        c = s.case("headers", "ends on a byte boundary", pad=0)
        if c.stats["ends_on_byte"]:
            cases.append(c)
            break
    return tuple(cases)


# ------------------------------------------------------------------------------------------------ directed: the phase of the input
@functools.lru_cache(maxsize=None)
def input_phase():
    rng = random.Random(404)
    cases = []
    text = [rng.choice(b"ACGTN#I") for _ in range(260)]
    for at in range(20, 250, 31):
        text.insert(at, (rng.choice((3, 7, 20)), rng.choice((1, 6, 25))))
    ll, dl = _code_for(text, rng, shape="deep", extra_ll=12)
    cl = as_lens(dict(zip((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18),
                          (4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 5, 5, 5, 5))), 19)
    assert kraft(cl) == 1 << 15
    for base in (0, STRETCH):
        for k in range(490, 531):
            s = Stream(rng)
            s.stored(_bytes(rng, base + k))
            # (the same block each time: a header of ~45 bytes — HCLEN 19 — and its first symbols)
            s.dynamic(text, ll, dl, last=False, hclen=19, cl_lens=cl, cl_mode="greedy")
            s.fixed(text[:40], last=True)
            cases.append(s.case("input_phase", "dynamic block behind %d stored bytes" % (base + k), pad=k))
    # LEN / NLEN across byte 512 (and 1024), behind a stored and behind a compressed block
    for base in (0, STRETCH):
        for k in (502, 503, 504, 505, 506):
            s = Stream(rng)
            s.stored(_bytes(rng, base + k))
            s.stored(_bytes(rng, 600), pad=0x2A)
            s.fixed(text[:30] + [(258, 600), (100, 1100)], last=True)
            cases.append(s.case("input_phase", "LEN/NLEN behind %d stored bytes" % (base + k)))
    for n in range(430, 520):                      # (8 or 9 bits a literal: those of the sizes that put LEN / NLEN across byte 512)
        s = Stream(rng)
        s.dynamic(list(_bytes(rng, n)), [8] * 255 + [9, 9], [0], last=False, cl_mode="greedy")
        s.stored(_bytes(rng, 300), last=True)
        if s.stats["stored_len_words_straddle_512"]:
            cases.append(s.case("input_phase", "LEN/NLEN behind a compressed block of %d literals" % n))
    # a long run of compressed input: many stretches, matches decoded across each hand-over
    for variant in range(4):
        s = Stream(rng)
        toks = []
        for i in range(1800):
            toks.append(rng.randrange(256))
            if i % 5 == variant:
                toks.append((rng.choice((3, 4, 5, 40)), rng.randint(1, 1 + i)))
        _dyn(s, toks, rng, last=True, shape=("deep", "flat", "random", "deep")[variant], long_literals=variant == 3)
        cases.append(s.case("input_phase", "2 KiB of compressed input, variant %d" % variant))
    return tuple(cases)


# ------------------------------------------------------------------------------------------------ invalid on purpose
@functools.lru_cache(maxsize=None)
def invalid():
    """Streams a decoder must refuse.  Each is a valid opening — data that inflates — followed by what is wrong, and
    enough bytes behind it that "needs more input" is not the reason."""
    rng = random.Random(505)
    cases = []
    tail = _bytes(rng, 24)
    text = [rng.choice(b"ACGT") for _ in range(50)] + [(5, 3), (9, 20)]

    def opening():
        s = Stream(rng)
        s.stored(_bytes(rng, 100))
        s.fixed(text)
        return s

    def add(label, s):
        stream, out = s.finish(0)
        cases.append(Case("invalid", label, stream + tail, None, s.stats, s.pairs, size=max(1, len(out) + 40)))

    for sym in (286, 287):
        s = opening()
        s.fixed([1, 2, ("ll", sym), 3, 4], last=True)
        add("fixed block, literal/length symbol %d" % sym, s)
    for sym in (30, 31):
        s = opening()
        s.fixed([1, 2, ("ll", 260), ("d", sym), 3, 4], last=True)
        add("fixed block, distance symbol %d" % sym, s)
    good_ll = as_lens({65: 1, 256: 2, 257: 2}, 257 + 1)
    for field in (30, 31):
        s = opening()
        s.dynamic([65, 65], good_ll, [1], last=True, hlit_field=field)
        add("HLIT field %d: %d codes" % (field, 257 + field), s)
        s = opening()
        s.dynamic([65, 65], good_ll, [1], last=True, hdist_field=field)
        add("HDIST field %d: %d codes" % (field, 1 + field), s)
    # over-subscribed and incomplete sets, for each of the three codes
    s = opening()
    s.dynamic([65], good_ll, [1], last=True, cl_lens=as_lens({0: 1, 1: 1, 2: 2}, 19))
    add("code-length code over-subscribed", s)
    s = opening()
    s.dynamic([65], good_ll, [1], last=True, cl_lens=as_lens({0: 2, 1: 2, 2: 2}, 19))
    add("code-length code incomplete", s)
    s = opening()
    s.dynamic([65], good_ll, [1], last=True, cl_lens=as_lens({1: 1}, 19), cl_syms=[(1, 0)] * 259)
    add("code-length code of a single code", s)
    s = opening()
    s.dynamic([65], as_lens({65: 1, 66: 1, 256: 2, 257: 2}, 258), [1], last=True)
    add("literal/length code over-subscribed", s)
    s = opening()
    s.dynamic([65], as_lens({65: 2, 256: 2, 257: 2}, 258), [1], last=True)
    add("literal/length code incomplete", s)
    s = opening()
    s.dynamic([65, (3, 1)], good_ll, [1, 1, 1], last=True)
    add("distance code over-subscribed", s)
    s = opening()
    s.dynamic([65, (3, 1)], good_ll, [2, 2, 2], last=True)
    add("distance code incomplete", s)
    s = opening()
    s.dynamic([65, (3, 1)], good_ll, [2], last=True)
    add("a single distance code of 2 bits", s)
    s = opening()
    s.dynamic([65, 65], as_lens({65: 1, 255: 2, 257: 2}, 258), [1], last=True, eob=False)
    add("no end-of-block code", s)
    # HCLEN 4 (16, 17, 18 and 0 alone): a header that reads well and can carry no code at all
    s = opening()
    s.dynamic([], [0] * 257, [0], last=True, cl_lens=as_lens({18: 1, 0: 1}, 19), hclen=4, eob=False)
    assert s.stats["hclen_4"]
    add("HCLEN 4: every length zero", s)
    s = opening()
    s.dynamic([65], good_ll, [1], last=True, cl_syms=[(16, 0)] + [(0, 0)] * 62 + [(1, 0), (18, 127), (18, 41), (2, 0), (2, 0), (1, 0)])
    add("16 as the first length", s)
    s = opening()
    s.dynamic([65], good_ll, [1], last=True, cl_syms=[(18, 54), (1, 0), (18, 127), (18, 41), (2, 0), (2, 0), (17, 0)])
    add("a 17 that runs past HLIT + HDIST", s)
    s = opening()
    s.dynamic([65], good_ll, [1], last=True, cl_syms=[(18, 54), (1, 0), (18, 127), (18, 41), (2, 0), (2, 0), (16, 3)])
    add("a 16 that runs past HLIT + HDIST", s)
    s = opening()
    s.dynamic([65, 65, ("ll", 257), ("bits", 1, 1), 65], good_ll, [1], last=True)
    add("the unused sibling of a single 1-bit distance code", s)
    s = Stream(rng)
    s.fixed([(3, 1), 65], last=True)
    add("distance beyond the bytes produced, at output 0", s)
    s = Stream(rng)
    s.dynamic([(3, 1), 65], as_lens({65: 1, 256: 2, 257: 2}, 258), [1], last=True)
    add("distance beyond the bytes produced, at output 0, dynamic block", s)
    for dist in (1, 4097 - 164, 32768 - 164):
        s = opening()
        dist += len(s.out)
        s.fixed([(3, dist), 65], last=True)
        add("distance %d beyond the %d bytes produced" % (dist, len(s.out) - 1), s)
    s = Stream(rng)
    s.stored(_bytes(rng, 5000))
    s.fixed([(258, 5001), 65], last=True)
    add("distance 5001 beyond the 5000 bytes produced", s)
    s = opening()
    s.stored(_bytes(rng, 30), last=True, nlen_field=30)
    add("stored block, NLEN is not the complement of LEN", s)
    s = opening()
    s.stored(_bytes(rng, 30), last=True, len_field=31, nlen_field=31 ^ 0xFFFF ^ 0x8000)
    add("stored block, one bit of NLEN wrong", s)
    s = opening()
    s.stored(_bytes(rng, 30), last=True, len_field=30 + len(tail) + 1)
    add("stored block longer than the input", s)
    s = opening()
    s.stored(_bytes(rng, 10), last=True, len_field=65535)
    add("stored block of 65535 bytes, 10 present", s)
    s = opening()
    s.put(1, 1)
    s.put(3, 2)
    add("block type 3", s)
    s = Stream(rng)
    s.put(0, 1)
    s.put(3, 2)
    add("block type 3 first", s)
    # every proper prefix of one three-block stream
    s = Stream(rng)
    s.stored(_bytes(rng, 90))
    _dyn(s, text, rng, shape="deep")
    s.fixed(text[:30] + [(258, 100)], last=True)
    stream, out = s.finish(0)
    assert 150 <= len(stream) <= 250, len(stream)
    for n in range(len(stream)):
        cases.append(Case("invalid", "prefix of %d of %d bytes" % (n, len(stream)), stream[:n], None, size=len(out)))
    cases.append(Case("invalid", "the stream the prefixes are of", stream, out, s.stats, s.pairs))
    return tuple(cases)


# ------------------------------------------------------------------------------------------------ random streams and their damaged twins
def _random_tokens(rng, have, want, lits):
    """tokens for `want` more bytes behind `have` bytes of output: literal runs from the alphabet `lits`, matches drawn from
    the kinds of the matches theme as far as the output so far allows them"""
    toks, n = [], 0
    while n < want:
        if rng.random() < 0.45 or have + n == 0:
            k = rng.choice((1, 1, 2, 3, 5, 7, 8, 12))
            toks += [rng.choice(lits) for _ in range(k)]
            n += k
            continue
        o = have + n
        kind = rng.randrange(7)
        length = rng.choice(MATCH_LENS) if rng.random() < 0.3 else rng.randint(3, 258)
        if kind == 0 and o > RING:
            dist = rng.randint(RING + 1, min(o, 32768))
        elif kind == 1 and o >= RING:
            dist = rng.randint(RING - 257, RING)
        elif kind == 2:
            dist, length = rng.randint(1, min(o, 63)), rng.randint(65, 258)
        elif kind == 3 and o >= 64:
            dist = rng.randint(64, min(o, 257))
            length = rng.randint(dist + 1, 258)
        elif kind == 4:
            dist = rng.choice([d for d in directed_distances(length) + list(FAR) if d <= o])
        else:
            dist = rng.randint(1, min(o, 32768))
            length = rng.choice((3, 4, 5, 6, 8, 11, 15, 20, 40))
        toks.append((length, dist, True) if length == 258 and rng.random() < 0.3 else (length, dist))
        n += length
    return toks, n


def random_stream(rng):
    s = Stream(rng)
    total = rng.randint(5000, 9000)
    nblocks = rng.choice((1, 2, 2, 3, 3, 4, 6))
    for b in range(nblocks):
        last = b == nblocks - 1
        have = len(s.out)
        want = max(0, (total - have) if last else rng.randint(0, 2 * total // nblocks))
        if rng.random() < 0.08:
            want = 0
        kind = rng.choice(("stored", "fixed", "dynamic", "dynamic", "dynamic"))
        if b == 0 and rng.random() < 0.5:
            kind, want = "stored", rng.randint(RING, RING + 1500)           # history for the far matches
        if kind == "stored":
            s.stored(_bytes(rng, want), last=last, pad=rng.getrandbits(7))
            continue
        style = rng.choice(("le2", "le2", "le2", "deep", "deep", "deep", "flat", "random"))
        if kind == "fixed":
            lits = list(range(256))
        elif style == "le2":
            lits = rng.sample(range(256), rng.choice((1, 2, 2, 3)))
        else:
            lits = rng.sample(range(256), rng.choice((1, 2, 4, 20, 100, 256, 256)))
        toks, _ = _random_tokens(rng, have, want, lits)
        if kind == "fixed":
            s.fixed(toks, last=last)
            continue
        hdr = dict(cl_mode=rng.choice(("plain", "greedy", "zero16", "random")), cl_shape=rng.choice(("deep", "flat", "random")))
        if rng.random() < 0.3:
            hdr.update(hlit=286 if rng.random() < 0.5 else None, hdist=30 if rng.random() < 0.5 else None,
                       hclen=19 if rng.random() < 0.5 else None)
        used = sorted({t for t in toks if type(t) is int})
        if style == "le2" and used:
            fixed = dict(zip(used, {1: (1,), 2: rng.choice(((1, 2), (2, 2))), 3: (2, 2, 2)}[len(used)]))
            ll, dl = _code_for(toks, rng, shape=rng.choice(("deep", "flat")), fixed_ll=fixed, extra_d=rng.choice((0, 0, 3)))
        elif style == "deep":
            ll, dl = _code_for(toks, rng, shape="deep", long_literals=True, extra_ll=rng.choice((0, 16, 30)), extra_d=rng.choice((0, 5)))
        else:
            ll, dl = _code_for(toks, rng, shape=style, maxlen=rng.choice((9, 11, 12, 15)), extra_ll=rng.choice((0, 0, 9)))
        s.dynamic(toks, ll, dl, last=last, **hdr)
    return s


def damage(rng, stream):
    """1 or 2 flipped bits, more often than not among the first 40 bytes; one in five truncated"""
    b = bytearray(stream)
    for _ in range(rng.randint(1, 2)):
        at = rng.randrange(min(40, len(b))) if rng.random() < 0.6 else rng.randrange(len(b))
        b[at] ^= 1 << rng.randrange(8)
    if rng.random() < 0.2:
        del b[rng.randrange(1, len(b) + 1):]
    return bytes(b)


@functools.lru_cache(maxsize=None)
def random_corpus(seed, n=160):
    """n valid streams and, behind each, its damaged twin (expected None: whatever zlib says)."""
    rng = random.Random(seed)
    cases = []
    for i in range(n):
        s = random_stream(rng)
        c = s.case("random", "seed %d stream %d" % (seed, i), pad=rng.getrandbits(7))
        cases.append(c)
        cases.append(Case("random", "seed %d stream %d damaged" % (seed, i), damage(rng, c.stream), None, size=c.size))
    return tuple(cases)


THEMES = {"literal_runs": literal_runs, "matches": matches, "headers": headers, "input_phase": input_phase, "invalid": invalid}
RANDOM_SEEDS = (11, 12, 13)


def totals(cases):
    st, pairs = collections.Counter(), set()
    for c in cases:
        st.update(c.stats)
        pairs |= c.pairs
    return st, pairs
