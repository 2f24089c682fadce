"""The cases of tests/sam_fuzz.py are what tests/test_gpu_sam_fuzz.py needs them to be (no GPU here): the same bytes from the
same seed, read_sam's verdict as the generator states it, and both verdicts in every class that may get both — so that the
GPU test is not about one side only."""
import numpy as np
import pytest

from tests import sam_fuzz as F


@pytest.fixture(scope="module")
def verdicts():
    """read_sam's verdict on every case, computed once."""
    return {cls: [(case,) + F.host_verdict(case) for case in F.cases(cls)] for cls in F.CLASSES}


@pytest.mark.parametrize("cls", F.CLASSES)
def test_same_seed_same_bytes(cls):
    a, b = F.generate(cls, 0), F.generate(cls, 0)
    assert [(x.label, x.line_no, x.data, x.n_records, x.readgroups) for x in a] == \
           [(x.label, x.line_no, x.data, x.n_records, x.readgroups) for x in b]
    assert [x.data for x in a] == [x.data for x in F.cases(cls, 0)]
    if cls == "mutated":
        assert [x.data for x in a] != [x.data for x in F.generate(cls, 1)]


@pytest.mark.parametrize("cls", F.CLASSES)
def test_cases_have_the_shape_the_issue_states(cls):
    cases = F.cases(cls)
    assert len(cases) >= 60
    assert all(x.cls == cls and isinstance(x.label, str) and x.label for x in cases)
    if cls != "geometry":
        # one slab each, and the odd line where the case says it is
        assert max(len(x.data) for x in cases) < 65536
        for x in cases:
            if x.line_no is not None:
                lines, head_lines = x.data.split(b"\n"), 0
                while lines[head_lines].startswith(b"@"):
                    head_lines += 1
                odd = lines[head_lines + x.line_no - 1]
                assert repr(odd) == x.label or len(repr(odd)) > 300, (x, odd)
    else:
        assert min(len(x.data) for x in cases) > 3 * 65536


@pytest.mark.parametrize("cls", ["valid", "geometry"])
def test_read_sam_reads_what_must_parse(cls, verdicts):
    for case, al, exc in verdicts[cls]:
        assert exc is None, (case, exc)
        assert case.n_records is not None and al.batch.n == case.n_records, (case, al.batch.n, case.n_records)


@pytest.mark.parametrize("cls", ["numeric", "header", "mutated"])
def test_both_verdicts_occur(cls, verdicts):
    read = sum(1 for _, _, exc in verdicts[cls] if exc is None)
    refused = len(verdicts[cls]) - read
    assert read >= 30 and refused >= 30, (cls, read, refused)


def test_rname_hits_and_misses(verdicts):
    hit = miss = 0
    for case, al, exc in verdicts["rname"]:
        assert exc is None, (case, exc)
        tid = int(al.batch.tid[case.line_no - 1])
        hit, miss = hit + (tid >= 0), miss + (tid < 0)
    assert hit >= 30 and miss >= 30, (hit, miss)
    # ... and for the read groups: ids of the table and ids that are not
    known = sum(1 for case, al, _ in verdicts["rname"] if al.rg[case.line_no - 1] in dict(case.readgroups))
    assert known >= 10 and len(verdicts["rname"]) - known >= 10


def test_geometry_lines_start_and_end_on_every_offset():
    starts, ends, long_lines, exact = set(), set(), 0, 0
    for case in F.cases("geometry"):
        body = case.data[case.data.index(b"\ng") + 1:]          # (behind the header: the first QNAME starts with 'g')
        at = np.flatnonzero(np.frombuffer(body, np.uint8) == 10)
        starts.update(int(x) % 32 for x in at + 1)
        ends.update(int(x) % 32 for x in at)
        lens = np.diff(np.concatenate([[-1], at]))
        long_lines += int((lens > 65536).sum() >= 2 and (lens > 131072).sum() >= 1)
        exact += int(body[65535:65536] == b"\n")
    assert starts == set(range(32)) and ends == set(range(32))
    assert long_lines == len(F.cases("geometry")) and exact >= 8
    assert sum(1 for case in F.cases("geometry") if not case.data.endswith(b"\n")) >= 8


def test_the_collision_search_yields_chains():
    tables = F.chains()
    assert len(tables) == 4
    for names, chain in tables:
        size = F.table_size(len(names))
        assert size == 16 and len(set(names)) == len(names)
        homes = F.home_slots(names)
        slot = homes[names.index(chain[0])]
        assert sum(1 for h in homes if h == slot) >= 4, (names, homes)
        assert all(homes[names.index(c)] == slot for c in chain)
    # the restated hash is FNV-1a (32 bit): its published test vectors
    assert F.fnv1a(b"") == 0x811C9DC5 and F.fnv1a(b"a") == 0xE40C292C and F.fnv1a(b"foobar") == 0xBF9CF968
    assert [F.table_size(n) for n in (1, 8, 9, 16, 17, 1000)] == [16, 16, 32, 32, 64, 2048]
    # the chain names and the absent names of their slot are in the cases
    labels = " ".join(case.label for case in F.cases("rname"))
    for _, chain in tables:
        assert all(c.decode() in labels for c in chain)
