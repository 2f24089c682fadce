"""Strata by terminal damage, the parts that need no GPU (``--by-terminal-damage``, ``--terminal-positions``): the command
line's argument errors, ``by_damage/conditional.tsv`` and ``groups.tsv`` from hand-filled tables, and the rule itself — the
lines the key kernel runs per lane (mapdamage_amd/csrc/mdx_damage_key.h), compiled for the host and compared with the
oracle run on every record alone, in the three forms of the SEQ column."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from mapdamage_amd import layout as L
from mapdamage_amd.tables import StratifiedTables, TableSet
from tests import damage_util as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------- the command line
def _argv(tmp_path, *extra):
    return ["-i", "x.bam", "-r", "x.fa", "-d", str(tmp_path / "out")] + list(extra)


@pytest.mark.parametrize("extra,word", [
    (["--by-terminal-damage", "--by-reference"], "exclude each other"),
    (["--by-terminal-damage", "--reference-groups", "g.tsv"], "exclude each other"),
    (["--by-terminal-damage", "--regions", "p.bed"], "exclude each other"),
    (["--by-terminal-damage", "--region-groups", "p.bed"], "exclude each other"),
    (["--by-terminal-damage", "--rescale-only"], "--rescale-only counts nothing"),
    (["--terminal-positions", "2"], "needs --by-terminal-damage"),
    (["--by-terminal-damage", "--terminal-positions", "71"], "--length"),
    (["--by-terminal-damage", "--terminal-positions", "6", "-l", "5", "-m", "5"], "--length"),
    (["--by-terminal-damage", "--terminal-positions", "0"], "--terminal-positions"),
])
def test_argument_errors(tmp_path, capsys, extra, word):
    from mapdamage_amd.main import main
    assert main(_argv(tmp_path, *extra)) == 1
    assert word in capsys.readouterr().err
    assert not (tmp_path / "out" / "by_damage").exists()


def test_the_positions_default_to_one_and_land_in_the_options(tmp_path):
    from mapdamage_amd.engine import DamageEngine
    from mapdamage_amd.main import TerminalDamage, parse_args, reference_strata
    o = parse_args(_argv(tmp_path))
    assert o.by_terminal_damage is False and o.terminal_positions is None and reference_strata(o, ["chr1"], [10]) is None
    o = parse_args(_argv(tmp_path, "--by-terminal-damage"))
    assert o.by_terminal_damage is True and o.terminal_positions == 1
    assert reference_strata(o, ["chr1"], [10]) == (["none", "5p", "3p", "both"], TerminalDamage(1, False))
    o = parse_args(_argv(tmp_path, "--by-terminal-damage", "--terminal-positions", "70", "--single-stranded"))
    assert o.terminal_positions == 70
    assert reference_strata(o, ["chr1"], [10]) == (DamageEngine.DAMAGE_GROUPS, TerminalDamage(70, True))
    from mapdamage_amd.main import build_parser
    helps = {a.option_strings[0]: " ".join((a.help or "").split()) for a in build_parser()._actions if a.option_strings}
    assert "Not a reference option" in helps["--by-terminal-damage"] and "Not a reference option" in helps["--terminal-positions"]


# ---------------------------------------------------------------------- conditional.tsv, groups.tsv
LENGTH = 5
LIBS = [("Zed", "b"), ("Alpha", "a")]           # (the emitters sort: Alpha first)


def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % p for p in out):
            out.append(k)
        k += 1
    return out


def hand_tables():
    """2 libraries x 4 groups at --length 5: distinct primes in the C, C>T, G and G>A columns of every cell, one C cell and one
    G cell zero."""
    cols = [L.MIS_COLS.index(c) for c in ("C", "C>T", "G", "G>A")]
    mis = np.zeros((8, 2, 2, LENGTH, L.N_MIS_COLS), np.uint64)
    primes = iter(_primes(8 * 2 * 2 * LENGTH * 4))
    for s in range(8):
        for e in range(2):
            for st in range(2):
                for p in range(LENGTH):
                    for c in cols:
                        mis[s, e, st, p, c] = next(primes)
    # library 1 (Alpha), 5p end, position 3: no C among the reads whose 3p end is damaged (groups 3p, both)
    mis[[4 + 2, 4 + 3], L.ENDS.index("5p"), :, 2, L.MIS_COLS.index("C")] = 0
    # library 0, 3p end, position 5: no G among the reads whose 5p end is undamaged (groups none, 3p)
    mis[[0, 2], L.ENDS.index("3p"), :, 4, L.MIS_COLS.index("G")] = 0
    strata = TableSet([lib for lib in LIBS for _ in range(4)], LENGTH, 2, mis, np.zeros((8, 2, 2, LENGTH + 2, 4), np.uint64),
                      np.zeros((8, 2, 2, 16), np.uint64), np.zeros((0, 4), np.int64), 0)
    return StratifiedTables.from_block(strata, LIBS, D.GROUPS, np.arange(8, dtype=np.uint64) * 3 + 1), mis


@pytest.mark.parametrize("single_stranded", [False, True])
def test_conditional_tsv(single_stranded):
    tables, mis = hand_tables()
    lines = tables.conditional_text(single_stranded).split("\n")
    assert lines[0] == "Sample\tLibrary\tEnd\tPos\tGiven\tSubstitutions\tBases\tFrequency" and lines[-1] == ""
    rows = [x.split("\t") for x in lines[1:-1]]
    assert len(rows) == 2 * 2 * 3 * LENGTH
    by_lib = mis.reshape(2, 4, 2, 2, LENGTH, L.N_MIS_COLS)
    want = []
    n_nan = 0
    for sample, library, li in (("Alpha", "a", 1), ("Zed", "b", 0)):
        for end, num, den, given in (("5p", "C>T", "C", (("all", [0, 1, 2, 3]), ("3p-damaged", [2, 3]), ("3p-undamaged", [0, 1]))),
                                     ("3p",) + (("C>T", "C") if single_stranded else ("G>A", "G")) +
                                     ((("all", [0, 1, 2, 3]), ("5p-damaged", [1, 3]), ("5p-undamaged", [0, 2])),)):
            for name, groups in given:
                for p in range(LENGTH):
                    cell = by_lib[li, groups, L.ENDS.index(end), :, p]
                    s, b = int(cell[..., L.MIS_COLS.index(num)].sum()), int(cell[..., L.MIS_COLS.index(den)].sum())
                    n_nan += b == 0
                    want.append([sample, library, end, str(p + 1), name, str(s), str(b), "%.15g" % (s / b) if b else "NaN"])
    assert rows == want
    # (the zero G cell is a 3p cell of the double-stranded rows only)
    assert n_nan == (1 if single_stranded else 2)
    assert ["Alpha", "a", "5p", "3", "3p-damaged"] in [r[:5] for r in rows if r[7] == "NaN"]
    # (%.15g: no more than 15 significant digits, as damage_frequency_text writes them)
    assert all(len(r[7].split("e")[0].replace(".", "").lstrip("0")) <= 15 for r in rows if r[7] != "NaN")
    assert any(len(r[7].split("e")[0].replace(".", "").lstrip("0")) == 15 for r in rows)


def test_groups_tsv():
    tables, _ = hand_tables()
    # kept[library * 4 + group] = 3 (library * 4 + group) + 1
    assert tables.damage_groups_text() == "Index\tGroup\tReads\n0\tnone\t14\n1\t5p\t20\n2\t3p\t26\n3\tboth\t32\n"


def test_conditional_tsv_needs_the_damage_groups():
    tables, _ = hand_tables()
    tables.groups = ["a", "b", "c", "d"]
    with pytest.raises(ValueError):
        tables.conditional_text()


# ---------------------------------------------------------------------- the rule, compiled for the host
@pytest.fixture(scope="module")
def host_rule(tmp_path_factory):
    so = tmp_path_factory.mktemp("damage_key") / "damage_key_host.so"
    subprocess.check_call(["c++", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mapdamage_amd", "csrc"),
                           os.path.join(ROOT, "tests", "damage_key_host.cpp"), "-o", str(so)])
    lib = ctypes.CDLL(str(so))

    def ptr(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def groups(ref, b, form, minqual, positions, single_stranded=False):
        resident, offs = D.resident_reference(ref)
        qual, lowq = (b.qual if minqual else None), None
        if form == "ascii":
            seq, packed, folded = b.seq, 0, 0
        elif form == "4bit":
            seq, packed, folded = D.pack4(b.seq), 1, 0
        elif form == "4bit+lowq":
            seq, packed, folded = D.pack4(b.seq), 1, 0
            lowq = np.concatenate([np.packbits(b.qual < minqual, bitorder="little"), np.zeros(4, np.uint8)])
        else:
            seq, packed, folded, qual = D.pack4(b.seq, b.qual, minqual), 1, int(minqual > 0), None
        seq = np.ascontiguousarray(seq)
        out = np.zeros(b.n, np.uint8)
        lib.damage_groups_host(ctypes.c_int64(b.n), ctypes.c_int64(b.cigar.shape[0]), ctypes.c_int64(b.seq.shape[0]), ptr(b.flag), ptr(b.tid),
                               ptr(b.pos), ptr(b.cigar_off), ptr(b.cigar), ptr(b.seq_off), ptr(seq), ptr(qual), ptr(lowq), packed, folded,
                               minqual, ptr(resident), ptr(offs), len(ref.names), positions, int(single_stranded), ptr(out))
        return out.astype(np.int64)
    return groups


@pytest.mark.parametrize("minqual", [0, 20])
def test_the_rule_agrees_with_the_oracle_record_by_record(host_rule, minqual):
    from tests.test_gpu_strata import genome5
    b, first = D.grid_batch(), D.grid_first(minqual)
    kept = (b.flag & 0xF04) == 0
    assert int(kept.sum()) == 3875
    for positions in (1, 3, 70):
        for single_stranded in (False, True):
            want = D.groups_of(first, positions, single_stranded)
            assert single_stranded or len(set(want[kept])) == 4
            for form in ("ascii", "4bit", "4bitq") + (("4bit+lowq",) if minqual else ()):
                got = host_rule(genome5(), b, form, minqual, positions, single_stranded)
                np.testing.assert_array_equal(got[kept], want[kept], err_msg="%s K=%d ss=%s" % (form, positions, single_stranded))
