"""The inputs the DEFLATE encoder of the device BGZF writer (mapdamage_amd/csrc/mdx_deflate.h) is tested on: a list of
(label, bytes), the same list in every run — every draw is seeded.  A member is at most MAX_IN bytes and is encoded in PIECES
pieces of PIECE bytes, a lane each on the device; a piece's matches reach back into the piece in front of it.

tests/native/deflate_check.cpp holds the host build of the encoder against zlib on these and counts the encoder's paths they
reach (tests/test_deflate_paths.py asserts that each is reached); tests/test_gpu_bgzf_writer.py holds the device against the
host build's bytes."""
import functools
import pathlib
import random
import re
import struct

_HEADER = (pathlib.Path(__file__).resolve().parent.parent / "mapdamage_amd" / "csrc" / "mdx_deflate.h").read_text()


def _enum(name):
    return int(re.search(r"\b%s = (0x[0-9A-Fa-f]+|\d+)" % name, _HEADER).group(1), 0)


MAX_IN = _enum("MAX_IN")
PIECES = int(re.search(r"#define MDX_DEFLATE_PIECES (\d+)", _HEADER).group(1))
PIECE = MAX_IN // PIECES
MIN_MATCH, MAX_MATCH, WINDOW = _enum("MIN_MATCH"), _enum("MAX_MATCH"), _enum("WINDOW")
assert PIECE * PIECES == MAX_IN


def noise(n, seed):
    """Incompressible: a piece of it is written as a stored block."""
    return random.Random("noise %d" % seed).randbytes(n)


def text(n, seed, alphabet=b"ACGT"):
    """Compressible: four letters, with matches at every distance."""
    return bytes(random.Random("text %d" % seed).choices(alphabet, k=n))


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _legacy():
    """The cases test_deflate_core_is_read_by_zlib had before this list, its unseeded draws as seeded ones of the same kinds."""
    rnd = random.Random(1)
    full = MAX_IN
    datas = [b"", b"a", b"ab", b"abc", b"abcd", b"aaaa", b"abc" * 1000, bytes(rnd.getrandbits(8) for _ in range(60000)),
             bytes(rnd.choice(b"ACGT") for _ in range(full)), b"\x00" * full, rnd.randbytes(100), rnd.randbytes(full),
             bytes(rnd.choice(b"ACGTN!#$%&'()*+,-./0123456789") for _ in range(30000)),
             b"ACGT" * 3000 + rnd.randbytes(30000) + b"TTTTGGGG" * 2000, bytes([i % 251 for i in range(65000)]),
             bytes(rnd.choice(b"ab") for _ in range(full)), b"x" * 258 + b"y" + b"x" * 259 + b"z" + b"x" * 40000]
    skew = bytearray()
    for i, f in enumerate(_fib(24)):
        skew += bytes([i]) * min(f, 20000)
    skew = list(skew)
    rnd.shuffle(skew)
    datas.append(bytes(skew[:full]))
    for _ in range(120):
        n = rnd.randint(0, full)
        kind = rnd.randint(0, 3)
        if kind == 0:
            d = rnd.randbytes(n)
        elif kind == 1:
            d = bytes(rnd.choices(b"ACGT", k=n))
        elif kind == 2:
            w = rnd.randbytes(rnd.randint(1, 300))
            d = (w * (n // len(w) + 1))[:n]
        else:
            d = bytearray()
            while len(d) < n:
                if d and rnd.random() < 0.5:
                    st = rnd.randint(0, len(d) - 1)
                    d += d[st:st + rnd.randint(1, 400)]
                else:
                    d += rnd.randbytes(rnd.randint(1, 50))
            d = bytes(d[:n])
        datas.append(d)
    return [("legacy %d" % i, d) for i, d in enumerate(datas)]


def edge_lengths():
    """Around a piece's ends (a last piece of fewer than MIN_MATCH bytes cannot hash), a member's end, and the 1 KiB a lane of
    the kernel that assembles a member takes of its CRC-32."""
    p = PIECE
    return sorted({0, 1, 3, 4, 5, p - 1, p, p + 1, p + 3, p + 4, 2 * p - 1, 2 * p + 1, 3 * p + 1, 3 * p + 2, 3 * p + 3, MAX_IN - 1, MAX_IN,
                   1023, 1024, 1025, 64 * 1024 - 257})


def every_match_length():
    """Runs of one byte, a byte value per run: a literal and then one match of distance 1 and of each length MIN_MATCH to
    MAX_MATCH, the longest first (in front of the first piece's end); a zero between two runs."""
    assert MAX_MATCH - MIN_MATCH + 1 <= 255
    return b"".join(bytes([length - MIN_MATCH + 1]) * (length + 1) + b"\0" for length in range(MAX_MATCH, MIN_MATCH - 1, -1))


def far_match(distance, at_end_of=None):
    """Eight bytes, zeros (which hash to one bucket and leave the eight's alone), the eight again ``distance`` later."""
    word = bytes([0xA7, 0x3C, 0x59, 0xE1, 0x1D, 0x82, 0x6B, 0xF4])
    if at_end_of is None:
        return word + b"\0" * (distance - 8) + word + b"\x55"
    # ... the second time as the last MIN_MATCH bytes of the piece behind the one it starts
    word = word[:MIN_MATCH]
    assert distance == at_end_of - MIN_MATCH
    return word + b"\0" * (distance - MIN_MATCH) + word


def match_in_the_piece_in_front():
    """300 bytes of noise that end where the second piece starts, and again as that piece's first bytes: the only copy lies
    entirely in front of the piece."""
    again = noise(300, 77)
    return text(PIECE - 300, 70) + again + again + text(2000, 71, b"TGCA")


def fibonacci_literals(symbols=19):
    """Byte i occurs fib(i) times, shuffled, in less than a piece: the minimum-redundancy code of such counts is as deep as
    it has symbols — of the bytes' counts, that is; the encoder finds matches among the frequent ones, and the code of what
    is left of them is not that deep (tests/test_deflate_paths.py)."""
    data = bytearray()
    for i, f in enumerate(_fib(symbols)):
        data += bytes([i]) * f
    assert len(data) <= PIECE
    data = list(data)
    random.Random(19).shuffle(data)
    return bytes(data)


def dyadic(n, seed):
    """``n`` (a power of two) bytes whose histogram is dyadic: a complete prefix code's lengths drawn at random, the symbol of
    length l occurring n >> l times, shuffled.  The literal code then has those lengths, many different ones, and the code of
    the code lengths has counts of its own that can need more than its 7 bits — whether they do depends on the draw:
    DYADIC is a size and a seed at which they do (tests/test_deflate_paths.py runs the checker on that input alone)."""
    rnd = random.Random("dyadic %d" % seed)
    depth = n.bit_length() - 1
    lengths = [0]
    while len(lengths) < 200:
        can = [i for i, length in enumerate(lengths) if length < depth]
        if not can or rnd.random() < 0.02:
            break
        i = rnd.choice(can)
        lengths[i] += 1
        lengths.append(lengths[i])
    symbols = rnd.sample(range(256), len(lengths))
    data = bytearray()
    for s, length in zip(symbols, lengths):
        data += bytes([s]) * (n >> length)
    assert len(data) == n
    data = list(data)
    rnd.shuffle(data)
    return bytes(data)


# (size, seed) of the corpus's dyadic input: of the seeds 0 to 29 none binds the code-length code at 1024 bytes; at 2048 bytes
# seed 2 is the first that does, in a piece written as a dynamic block
DYADIC = (2048, 2)

HASH_BITS = _enum("HASH_BITS")
_HASH_MULTIPLIER = int(re.search(r"\* (\d+)u\) >> \(32 - HASH_BITS\)", _HEADER).group(1))


def _bucket(window):
    """The encoder's hash of four bytes (deflate_piece: load32 times the multiplier, the top HASH_BITS bits)."""
    return ((struct.unpack("<I", window)[0] * _HASH_MULTIPLIER) & 0xFFFFFFFF) >> (32 - HASH_BITS)


# skewed_distances and skewed_lengths below mirror deflate_piece's table updates — a head per bucket, set at every place the
# greedy parse looks at and at every other place inside a match, one candidate looked up per place — to plan every token.  If
# the encoder's hash, its insertions or its parse change, they stop reaching the limits and tests/test_deflate_paths.py says
# so (ll_bound, d_bound of these two inputs alone); they then have to follow the encoder again.


# The counts of 17 symbols whose minimum-redundancy code, built with a leaf taken first where a leaf and an inner node weigh
# the same (build_lengths), is a chain 16 deep: every count one more than the sum of all counts two and more places below it.
# Nothing smaller is that deep, and its 3570 matches of four bytes fit into a piece only just.
CHAIN = (1, 1, 1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1364)
# distances in words of four bytes, one distance code (5 to 21) per class: the nearest the most frequent
_WORD_DISTANCES = ((2, 2), (3, 3), (4, 4), (5, 6), (7, 8), (9, 12), (13, 16), (17, 24), (25, 32), (33, 48), (49, 64), (65, 96), (97, 128),
                   (129, 192), (193, 256), (257, 384), (385, 512))


def skewed_distances(seed=0, vocabulary=120):
    """Less than a piece whose distance codes occur CHAIN times: words of four bytes, 120 of them once as literals, then 3570
    words that each repeat the word a chosen number of words back — a match of exactly four bytes, since no two words start
    with the same byte and the word behind it is not the one behind its source.  The encoder keeps one candidate per hash
    bucket, so the heads of its table are followed here, window by window as it fills them, and a word is only repeated where
    the table still leads to its last place; where no class with matches left has such a word, a new word goes in."""
    rnd = random.Random("distances %d" % seed)
    quota = list(reversed(CHAIN))
    full = list(quota)
    firsts = rnd.sample(range(256), vocabulary)
    words = [bytes([f]) + rnd.randbytes(3) for f in firsts]
    spare = [bytes([f]) + rnd.randbytes(2) + bytes([f]) for f in range(256) if f not in firsts]
    seq = list(range(vocabulary))
    last = {w: i for i, w in enumerate(seq)}
    data = bytearray(b"".join(words))
    head = {}
    for p in range(len(data) - 3):
        head[_bucket(bytes(data[p:p + 4]))] = p + 1
    pending = [len(data) - 3, len(data) - 2, len(data) - 1]         # places whose windows end in the next word
    forbidden = None
    while sum(quota):
        i = len(seq)
        tail_at = pending[0]
        options = []
        for c, (lo, hi) in enumerate(_WORD_DISTANCES):
            for k in range(lo, hi + 1) if quota[c] else ():
                w = seq[i - k] if i >= k else None
                if w is None or last[w] != i - k or w == forbidden:
                    continue
                tail = bytes(data[tail_at:]) + words[w]
                mine = _bucket(words[w])
                if head.get(mine) == 4 * (i - k) + 1 and all(_bucket(tail[q - tail_at:q - tail_at + 4]) != mine for q in pending):
                    options.append((c, k, w))
        if options:
            c = max({c for c, _, _ in options}, key=lambda c: (quota[c] / full[c], rnd.random()))
            _, k, w = rnd.choice([o for o in options if o[0] == c])
            quota[c] -= 1
        else:
            words.append(spare.pop())
            w, k = len(words) - 1, None
        tail = bytes(data[tail_at:]) + words[w]
        for q in pending:
            head[_bucket(tail[q - tail_at:q - tail_at + 4])] = q + 1
        p = len(data)
        data += words[w]
        head[_bucket(words[w])] = p + 1
        pending = [p + 2] if k else [p + 1, p + 2, p + 3]
        forbidden = seq[i - k + 1] if k else None
        seq.append(w)
        last[w] = i
    assert len(data) + 2 <= PIECE
    return bytes(data) + b"\xfe\xfd"


def skewed_lengths(seed=0, text_bytes=220):
    """Less than a piece whose literal/length symbols occur CHAIN times.  A literal cannot be frequent unless the three bytes
    behind it differ every time, and the encoder turns the repeats of a skewed alphabet into matches (fibonacci_literals), so
    the four frequent symbols are the match lengths 4 to 7 and the others twelve byte values and the end of the block: a text
    of those bytes with no window of four twice, then 3050 matches of planned lengths that copy any place the hash table
    still leads to — each ends where planned because the byte behind it is not the byte behind its source — some with one
    literal in front whose window is new.  The table's heads are followed as in skewed_distances."""
    rnd = random.Random("lengths %d" % seed)
    literals = dict(zip(rnd.sample(range(256), 12), reversed(CHAIN[1:13])))
    matches = dict(zip((4, 5, 6, 7), reversed(CHAIN[13:])))
    all_literals, all_matches = dict(literals), dict(matches)
    data = bytearray()
    head = {}
    queue = []                  # (place, looked up there?) of the windows that still lack bytes, in order

    def settle(extra, commit):
        """The waiting windows that ``extra`` behind the data completes -> the buckets they fill; None if one that the
        encoder looks up is found."""
        base = queue[0][0] if queue else len(data)
        tail = bytes(data[base:]) + extra
        filled, done = {}, 0
        for place, looked in queue:
            window = tail[place - base:place - base + 4]
            if len(window) < 4:
                break
            b = _bucket(window)
            c = filled.get(b, head.get(b, 0))
            if looked and c and (data[c - 1:c + 3] if c + 3 <= len(data) else (bytes(data[c - 1:]) + extra)[:4]) == window:
                return None
            filled[b] = place + 1
            done += 1
        if commit:
            head.update(filled)
            del queue[:done]
        return filled

    def literal(v):
        settle(bytes([v]), True)
        queue.append((len(data), True))
        data.append(v)
        literals[v] -= 1

    while len(data) < text_bytes:
        by_need = sorted((v for v in literals if literals[v]), key=lambda v: -literals[v] / all_literals[v] * rnd.uniform(0.3, 1.0))
        v = next((v for v in by_need if settle(bytes([v]), False) is not None), None)
        if v is None:
            break
        literal(v)
    forbidden = None            # the byte behind the last match's source: the next byte must differ
    while sum(matches.values()):
        x = None
        if rnd.random() < 1.3 * sum(literals.values()) / sum(matches.values()):
            can = [v for v in literals if literals[v] and v != forbidden]
            x = max(can, key=lambda v: literals[v] / all_literals[v] * rnd.uniform(0.6, 1.0)) if can else None
        front = bytes([x]) if x is not None else b""
        places = list(head.values())
        chosen = None
        for length in sorted((n for n in matches if matches[n]), key=lambda n: -matches[n] / all_matches[n] * rnd.uniform(0.8, 1.0)):
            for _ in range(60):
                q = rnd.choice(places) - 1
                word = bytes(data[q:q + length])
                if q + length >= len(data) or (x is None and word[0] == forbidden) or head.get(_bucket(word[:4])) != q + 1:
                    continue
                if x is not None:
                    queue.append((len(data), True))
                filled = settle(front + word, False)
                if x is not None:
                    queue.pop()
                if filled is not None and _bucket(word[:4]) not in filled:
                    chosen = (length, q, word)
                    break
            if chosen:
                break
        if chosen is None:
            assert x is not None, "no place to copy from"
            continue
        length, q, word = chosen
        if x is not None:
            literal(x)
        settle(word, True)
        p = len(data)
        data += word
        head[_bucket(word[:4])] = p + 1
        queue.extend((p + k, False) for k in range(2, length, 2))
        settle(b"", True)
        forbidden = data[q + length]
        matches[length] -= 1
    while sum(literals.values()):
        literal(next(v for v in sorted(literals) if literals[v] and v != forbidden and settle(bytes([v]), False) is not None))
        forbidden = None
    assert len(data) <= PIECE
    return bytes(data)


@functools.lru_cache(maxsize=None)
def corpus():
    cases = _legacy()
    for n in edge_lengths():
        cases.append(("text of %d" % n, text(n, n)))
        cases.append(("noise of %d" % n, noise(n, n)))
    cases += [
        # a stored block that is not the member's last, and one that is, beside pieces that compress
        ("noise then text", noise(PIECE, 1) + text(MAX_IN - PIECE, 2)),
        ("text then noise", text(MAX_IN - PIECE, 3) + noise(PIECE, 4)),
        ("text, noise, text, noise", text(PIECE, 5) + noise(PIECE, 6) + text(PIECE, 7) + noise(PIECE - 7, 8)),
        ("match in the piece in front", match_in_the_piece_in_front()),
        ("match a window back", far_match(WINDOW)),
        ("match two pieces back", b"\0" * PIECE + far_match(2 * PIECE - MIN_MATCH, at_end_of=2 * PIECE)),
        ("runs: distance 1", b"\0" * 700 + b"\xff" * 5000 + b"q" * 259),
        ("every match length", every_match_length()),
        ("fibonacci literals", fibonacci_literals()),
        ("skewed distances", skewed_distances()),
        ("skewed lengths", skewed_lengths()),
        ("dyadic histogram", dyadic(*DYADIC)),
        # one literal and no match: the distance code is empty
        ("one literal", b"k"), ("three of one literal", b"kkk"),
        # one literal, then matches of distance 1 only: one distance code
        ("one distance", b"z" * 3000),
    ]
    labels = [label for label, _ in cases]
    assert len(set(labels)) == len(labels)
    assert all(len(d) <= MAX_IN for _, d in cases)
    return tuple(cases)



def cases_file(path, cases):
    """The cases as tests/native/deflate_check.cpp reads them: {u32 n, n bytes}."""
    with open(path, "wb") as out:
        for _, d in cases:
            out.write(struct.pack("<I", len(d)) + d)


def read_members(path):
    """What ``deflate_check --emit`` wrote: {u32 size, bytes}, a member per case."""
    blob = pathlib.Path(path).read_bytes()
    members, at = [], 0
    while at < len(blob):
        size = struct.unpack_from("<I", blob, at)[0]
        members.append(blob[at + 4:at + 4 + size])
        at += 4 + size
    assert at == len(blob)
    return members
