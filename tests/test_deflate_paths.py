"""The DEFLATE encoder of the device BGZF writer (mapdamage_amd/csrc/mdx_deflate.h), compiled for the host: that the corpus of
tests/deflate_corpus.py reaches every path of it the round trip through zlib does not tell apart — the length limits of its
three codes, stored blocks that are and are not a member's last, pieces too short to hash, matches into the piece in front and
at the largest distance and length — and its small functions against their definitions: the code lengths of build_lengths
against a plain Huffman construction, length_code and dist_code against the tables of RFC 1951 for every value.

Every comparison is exact: bytes, counts, integer costs."""
import heapq
import pathlib
import random
import struct
import subprocess

import pytest

from tests import deflate_corpus as C

ROOT = pathlib.Path(__file__).resolve().parent.parent


def compile_native(folder, name):
    exe = folder / name
    subprocess.check_call(["g++", "-O2", "-I", str(ROOT / "mapdamage_amd" / "csrc"), str(ROOT / "tests" / "native" / (name + ".cpp")), "-lz", "-o", str(exe)])
    return exe


def run_checker(exe, folder, cases, emit=None):
    """deflate_check over the cases -> (its "ok" line, the counters of its "paths" line); zlib has inflated every member, as
    one block and in pieces, to the bytes that went in."""
    path = folder / "cases.bin"
    C.cases_file(path, cases)
    out = subprocess.run([str(exe), str(path)] + (["--emit", str(emit)] if emit else []), capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok %d cases" % len(cases)), out.stdout + out.stderr
    ok, paths = out.stdout.splitlines()
    assert paths.startswith("paths ")
    return ok, {k: int(v) for k, v in (item.split("=") for item in paths.split()[1:])}


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    folder = tmp_path_factory.mktemp("deflate_paths")
    return folder, compile_native(folder, "deflate_check"), compile_native(folder, "deflate_tables")


# ---------------------------------------------------------------------- (a) every path runs
@pytest.fixture(scope="module")
def paths(native):
    folder, check, _ = native
    ok, found = run_checker(check, folder, C.corpus())
    print(ok)
    print(found)
    return found


def test_the_corpus_reaches_every_path(paths):
    """Conditions on the corpus, not on the encoder: a counter at 0 is an input missing from tests/deflate_corpus.py.

    The distance of a whole window, 32768, is met in the member written as one block only: a piece's matches start at most
    PIECE - MIN_MATCH behind its first byte and reach no further back than the first byte of the piece in front, so the
    largest distance a piece can see is 2 * PIECE - MIN_MATCH, and that one is met too."""
    cases = C.corpus()
    assert sum(len(d) for _, d in cases) < 6 << 20
    for name in ("ll_bound", "d_bound", "cl_bound", "stored_final", "stored_inner", "short_pieces", "no_dist", "one_dist", "back_match"):
        assert paths[name] > 0, (name, paths)
    assert paths["max_dist"] == C.WINDOW == 32768 and paths["max_len"] == C.MAX_MATCH == 258
    assert paths["max_dist_pieces"] == 2 * C.PIECE - C.MIN_MATCH
    assert paths["lengths_seen"] == C.MAX_MATCH - C.MIN_MATCH + 1
    assert paths["pieces"] == sum(max(1, -(-len(d) // C.PIECE)) for _, d in cases)


@pytest.mark.parametrize("label,counter", [("skewed lengths", "ll_bound"), ("skewed distances", "d_bound"), ("dyadic histogram", "cl_bound")])
def test_an_input_built_for_a_limit_binds_it(native, label, counter):
    """The three inputs built for the length limits of the three codes, each alone: one piece, written as a dynamic block, whose
    code of that kind would be deeper than its limit — so that none of them loses its effect behind the others' counts."""
    folder, check, _ = native
    data = dict(C.corpus())[label]
    assert 0 < len(data) <= C.PIECE
    _, found = run_checker(check, folder, [(label, data)])
    assert found["pieces"] == 1 and found[counter] == 1 and found["stored_final"] == found["stored_inner"] == 0, found


def test_the_corpus_is_the_same_every_time():
    first = C.corpus()
    C.corpus.cache_clear()
    again = C.corpus()
    assert first == again and first is not again
    lengths = {len(d) for _, d in first}
    assert set(C.edge_lengths()) <= lengths
    for n in C.edge_lengths():
        assert {"text of %d" % n, "noise of %d" % n} <= {label for label, _ in first}


# ---------------------------------------------------------------------- (b) build_lengths
def huffman(freq):
    """(cost, depth) of a minimum-redundancy code of the counts that occur — among the codes of that cost one of the least
    depth (ties between weights go to the shallower subtree)."""
    heap = [(f, 0) for f in freq if f]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


def frequency_vectors(n, rnd):
    """Seeded counts of five kinds over n symbols, some of them absent; every vector's sum stays below 2^31."""
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    out = []
    for trial in range(60):
        m = rnd.choice([1, 2, 3, n // 2, n - 1, n]) if trial % 3 == 0 else rnd.randint(1, n)
        used = rnd.sample(range(n), max(1, m))
        top = rnd.choice([2, 10, 1000, 65280])
        kinds = {
            "uniform": [rnd.randint(1, top) for _ in used],
            "fibonacci": [fib[i % 40] for i in range(len(used))],
            "powers of two": [1 << (i % 22) for i in range(len(used))],
            "spikes": [rnd.choice([1, 1, 1, 2, 60000]) for _ in used],
            "geometric": [max(1, int(65280 * rnd.uniform(0.3, 0.95) ** i)) for i in range(len(used))],
        }
        for kind, values in kinds.items():
            rnd.shuffle(values)
            freq = [0] * n
            for s, v in zip(used, values):
                freq[s] = v
            assert sum(freq) < 1 << 31
            out.append((kind, freq))
    return out


@pytest.mark.parametrize("n,max_len", [(19, 7), (30, 15), (286, 15)])
def test_build_lengths(native, n, max_len):
    folder, _, tables = native
    vectors = frequency_vectors(n, random.Random(n * 100 + max_len))
    src, dst = folder / ("freq_%d.bin" % n), folder / ("len_%d.bin" % n)
    src.write_bytes(b"".join(struct.pack("<II%dI" % n, n, max_len, *freq) for _, freq in vectors))
    subprocess.check_call([str(tables), "lengths", str(src), str(dst)])
    got = dst.read_bytes()
    assert len(got) == n * len(vectors)
    bound = exact = 0
    for k, (kind, freq) in enumerate(vectors):
        lens = list(got[k * n:(k + 1) * n])
        where = (kind, freq, lens)
        m = sum(1 for f in freq if f)
        assert all((f == 0 and length == 0) or (f > 0 and 1 <= length <= max_len) for f, length in zip(freq, lens)), where
        if m == 1:
            assert sum(lens) == 1, where
        else:
            assert sum(1 << (max_len - length) for length in lens if length) == 1 << max_len, where            # Kraft: complete
        # a strictly more frequent symbol never has the longer code: from the highest count down, no code is shorter than
        # the longest code of the strictly higher counts
        longest_above, longest_here, count_here = 0, 0, None
        for f, length in sorted(((f, length) for f, length in zip(freq, lens) if f), reverse=True):
            if f != count_here:
                longest_above, count_here = max(longest_above, longest_here), f
            assert length >= longest_above, where
            longest_here = max(longest_here, length)
        cost, depth = huffman(freq)
        assert sum(f * length for f, length in zip(freq, lens)) >= cost, where
        if depth <= max_len:
            assert sum(f * length for f, length in zip(freq, lens)) == cost, where
            exact += 1
        else:
            bound += 1
    assert bound >= 20 and exact >= 20, (bound, exact)


# ---------------------------------------------------------------------- (c) length_code, dist_code
# RFC 1951 section 3.2.5: the codes 257 to 285 of the match lengths and 0 to 29 of the distances, their extra bits and the
# smallest value each stands for
LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def by_the_table(value, base, extra):
    code = max(i for i, b in enumerate(base) if b <= value)
    assert value - base[code] < 1 << extra[code]
    return code, extra[code], value - base[code]


def test_length_and_distance_codes_are_the_rfcs(native):
    _, _, tables = native
    assert len(LENGTH_BASE) == len(LENGTH_EXTRA) == 29 and len(DIST_BASE) == len(DIST_EXTRA) == 30
    lines = subprocess.run([str(tables), "codes"], capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(line.split()) for line in lines if line]
    want = []
    for length in range(3, 259):
        code, bits, value = by_the_table(length, LENGTH_BASE, LENGTH_EXTRA)
        want.append(("L", str(length), str(257 + code), str(bits), str(value)))
    for dist in range(1, 32769):
        code, bits, value = by_the_table(dist, DIST_BASE, DIST_EXTRA)
        want.append(("D", str(dist), str(code), str(bits), str(value)))
    assert len(got) == len(want) == 256 + 32768
    assert got == want, next((g, w) for g, w in zip(got, want) if g != w)
