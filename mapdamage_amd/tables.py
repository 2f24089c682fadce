"""Dense count tables and their byte-exact text emitters.

``TableSet`` is what ``DamageEngine.finish()`` returns: the canonical dense uint64 tables of
``layout.py`` indexed by library *id*, plus the emitters that reproduce the reference's
``misincorporation.txt`` / ``dnacomp.txt`` / ``lgdistribution.txt`` byte for byte
(mapdamage/statistics.py:53-55,95-98,128-137,187-203; format in SURVEY.md Appendix B).
"""

import io
from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

from . import layout as L


@dataclass
class TableSet:
    libraries: list            # [(sample, library)] indexed by library id
    length: int
    around: int
    mis: np.ndarray            # u64 [nlib][2][2][L][25]
    comp: np.ndarray           # u64 [nlib][2][2][L+A][4]
    lgd: np.ndarray            # u64 [nlib][2][2][lgd_max]
    lgd_over: np.ndarray = field(default_factory=lambda: np.zeros((0, 4), np.int64))
    n_kept: int = 0

    # ------------------------------------------------------------------ helpers
    def _sorted_libs(self):
        """(lib tuple, id) in the order of ``sorted(table.items())`` (statistics.py:190)."""
        return sorted((tuple(lib), i) for i, lib in enumerate(self.libraries))

    def lgd_sparse(self):
        """Sorted rows (lib id, kind, strand, length, count) of the length histogram."""
        idx = np.argwhere(self.lgd > 0)
        rows = {}
        for li, k, s, ln in idx:
            rows[(int(li), int(k), int(s), int(ln))] = int(self.lgd[li, k, s, ln])
        for li, k, s, ln in self.lgd_over:
            key = (int(li), int(k), int(s), int(ln))
            rows[key] = rows.get(key, 0) + 1
        return sorted(key + (cnt,) for key, cnt in rows.items())

    def add(self, other):
        assert self.mis.shape == other.mis.shape and self.comp.shape == other.comp.shape
        self.mis += other.mis
        self.comp += other.comp
        self.lgd += other.lgd
        self.lgd_over = np.concatenate([self.lgd_over, other.lgd_over])
        self.n_kept += other.n_kept
        return self

    # ------------------------------------------------------------------ emitters
    def misincorporation_text(self):
        out = io.StringIO()
        out.write("Sample\tLibrary\tEnd\tStd\tPos\t%s\n" % "\t".join(L.MIS_HEADER))
        for (sample, library), li in self._sorted_libs():
            for ei, end in enumerate(L.ENDS):
                for si, strand in enumerate(L.STRANDS):
                    block = self.mis[li, ei, si]
                    totals = block[:, :4].sum(axis=1)
                    for p in range(self.length):
                        row = block[p]
                        cells = [str(int(x)) for x in row[:4]]
                        cells.append(str(int(totals[p])))
                        cells.extend(str(int(x)) for x in row[4:])
                        out.write("%s\t%s\t%s\t%s\t%d\t%s\n"
                                  % (sample, library, end, strand, p + 1, "\t".join(cells)))
        return out.getvalue()

    def dnacomp_text(self):
        out = io.StringIO()
        out.write("Sample\tLibrary\tEnd\tStd\tPos\t%s\n" % "\t".join(L.COMP_HEADER))
        for (sample, library), li in self._sorted_libs():
            for ei, end in enumerate(L.ENDS):
                keys = L.comp_positions(ei, self.length, self.around)
                for si, strand in enumerate(L.STRANDS):
                    block = self.comp[li, ei, si]
                    totals = block.sum(axis=1)
                    for ri, key in enumerate(keys):
                        row = block[ri]
                        out.write("%s\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\n"
                                  % (sample, library, end, strand, key, int(row[0]), int(row[1]),
                                     int(row[2]), int(row[3]), int(totals[ri])))
        return out.getvalue()

    def lgdistribution_text(self):
        out = io.StringIO()
        out.write("Sample\tLibrary\tStd\tKind\tLength\tOccurences\n")
        sparse = self.lgd_sparse()
        by_lib = {}
        for li, k, s, ln, cnt in sparse:
            by_lib.setdefault(li, []).append((k, s, ln, cnt))
        for (sample, library), li in self._sorted_libs():
            for k, s, ln, cnt in sorted(by_lib.get(li, [])):
                out.write("%s\t%s\t%s\t%s\t%d\t%d\n"
                          % (sample, library, L.STRANDS[s], L.KINDS[k], ln, cnt))
        return out.getvalue()

    def damage_frequency_text(self, end, readplot):
        """EXPERIMENTAL, parity unpinned: ``5pCtoT_freq.txt`` (end "5p") or
        ``3pGtoA_freq.txt`` (end "3p") as mapDamage 2.0-2.2 wrote them from R; the reference snapshot
        no longer produces these files, so the format is recalled, not checked.  Per position 1..readplot:
        sum over libraries and strands of C>T / C at the 5' end (G>A / G at the 3' end), the aggregation of
        ``calculate.mutation.table`` (mapdamage/r/mapDamage.r:81-92)."""
        ei = L.ENDS.index(end)
        num_col, den_col, name = ("C>T", "C", "5pC>T") if end == "5p" else ("G>A", "G", "3pG>A")
        num = self.mis[:, ei, :, :, L.MIS_COLS.index(num_col)].sum(axis=(0, 1))
        den = self.mis[:, ei, :, :, L.MIS_COLS.index(den_col)].sum(axis=(0, 1))
        out = io.StringIO()
        out.write("pos\t%s\n" % name)
        for p in range(min(readplot, self.length)):
            freq = float(num[p]) / float(den[p]) if den[p] else float("nan")
            out.write("%d\t%s\n" % (p + 1, "NaN" if freq != freq else "%.15g" % freq))
        return out.getvalue()

    def write(self, folder):
        """Write the three tables into ``folder`` (mapdamage/main.py:229-231)."""
        import pathlib
        folder = pathlib.Path(folder)
        (folder / "misincorporation.txt").write_text(self.misincorporation_text())
        (folder / "dnacomp.txt").write_text(self.dnacomp_text())
        (folder / "lgdistribution.txt").write_text(self.lgdistribution_text())


def table_words(nlib, length, around, lgd_max):
    """uint64 words of the packed table block (include/mdx.h: mdx_table_words)."""
    return nlib * 4 * length * L.N_MIS_COLS + nlib * 4 * (length + around) * 4 + nlib * 4 * lgd_max + 2


def pack_words(ts: "TableSet") -> np.ndarray:
    """TableSet -> packed block [mis | comp | lgd | n_kept | n_lgd_over] (the all-reduce message)."""
    tail = np.asarray([ts.n_kept, ts.lgd_over.shape[0]], dtype=np.uint64)
    return np.concatenate([ts.mis.reshape(-1), ts.comp.reshape(-1), ts.lgd.reshape(-1), tail]).astype(np.uint64)


def unpack_words(words, libraries, length, around, lgd_max, lgd_over=None) -> "TableSet":
    """Packed block (host copy of mdx_finish_device output, possibly all-reduced) -> TableSet."""
    nlib = len(libraries)
    nm = nlib * 4 * length * L.N_MIS_COLS
    nc = nlib * 4 * (length + around) * 4
    nl = nlib * 4 * lgd_max
    words = np.ascontiguousarray(words).view(np.uint64)
    assert words.shape[0] == nm + nc + nl + 2, (words.shape, nm + nc + nl + 2)
    mis = words[:nm].reshape(nlib, 2, 2, length, L.N_MIS_COLS).copy()
    comp = words[nm:nm + nc].reshape(nlib, 2, 2, length + around, 4).copy()
    lgd = words[nm + nc:nm + nc + nl].reshape(nlib, 2, 2, lgd_max).copy()
    over = np.zeros((0, 4), np.int64) if lgd_over is None else np.asarray(lgd_over, np.int64).reshape(-1, 4)
    return TableSet([tuple(x) for x in libraries], length, around, mis, comp, lgd, over, int(words[-2]))


def merge_library_ids(libraries):
    """Map read-group order to unique library ids (reader.py:47-50: several read groups may
    name the same (SM, LB)).  Returns (unique list, remap array old id -> new id)."""
    uniq, remap = [], []
    index = {}
    for lib in libraries:
        lib = tuple(lib)
        if lib not in index:
            index[lib] = len(uniq)
            uniq.append(lib)
        remap.append(index[lib])
    return uniq, np.asarray(remap, dtype=np.uint16)


# ---------------------------------------------------------------------- strata: tables per (library, reference group)
CATCH_ALL_GROUP = "*"


def parse_reference_groups(text, references):
    """``--reference-groups FILE``: lines ``sequence name<TAB>group name``.  Returns (group names, group_of_tid): groups
    numbered in order of first appearance in the file; the sequences of ``references`` (the header's, tid order) that the
    file does not list go to a last group named ``*``.  A listed name the header lacks, a sequence listed twice, a line
    without two columns: ValueError naming it.  Empty lines and lines starting with ``#`` are skipped."""
    index = {name: tid for tid, name in enumerate(references)}
    names, number, group_of_tid = [], {}, [-1] * len(references)
    for lineno, line in enumerate(text.splitlines(), 1):
        line = line.rstrip("\r")
        if not line.strip() or line.startswith("#"):
            continue
        cols = line.split("\t")
        if len(cols) != 2 or not cols[0] or not cols[1]:
            raise ValueError("reference groups, line %d: expected 'sequence name<TAB>group name', found %r" % (lineno, line))
        seq, group = cols
        if seq not in index:
            raise ValueError("reference groups, line %d: the header has no sequence named %r" % (lineno, seq))
        if group == CATCH_ALL_GROUP:
            raise ValueError("reference groups, line %d: the group name %r is taken by the sequences the file does not list"
                             % (lineno, CATCH_ALL_GROUP))
        if group_of_tid[index[seq]] >= 0:
            raise ValueError("reference groups, line %d: sequence %r is listed twice" % (lineno, seq))
        if group not in number:
            number[group] = len(names)
            names.append(group)
        group_of_tid[index[seq]] = number[group]
    if any(g < 0 for g in group_of_tid):
        names.append(CATCH_ALL_GROUP)
        group_of_tid = [len(names) - 1 if g < 0 else g for g in group_of_tid]
    return names, np.asarray(group_of_tid, dtype=np.int32)


def groups_by_reference(references):
    """``--by-reference``: every sequence of the header its own group."""
    return [str(r) for r in references], np.arange(len(references), dtype=np.int32)


def parse_regions(text, references, lengths, named):
    """``--regions BED`` (``named=False``) / ``--region-groups BED`` (``named=True``): lines
    ``sequence<TAB>start<TAB>end[<TAB>name...]``, 0-based and half-open.  Returns (group names, iv_off, iv_start, iv_end,
    iv_group): the intervals of sequence ``t`` of ``references`` (the header's, tid order) are ``iv_off[t]:iv_off[t + 1]`` of
    the three parallel int32 columns, sorted and disjoint — overlapping or abutting regions of the same group are merged.
    ``named=False``: one group ``regions``; ``named=True``: column 4 names the group, numbered in order of first appearance.
    A last group named ``*`` always follows: the records that overlap no region.  ValueError naming the line for fewer than
    three columns, coordinates that are no integers, ``start >= end`` or ``start < 0``, an end beyond the sequence's length,
    a sequence the header lacks, a group named ``*``, a missing name with ``named=True``; naming both lines for overlapping
    regions of different groups.  Empty lines and lines starting with ``#``, ``track`` or ``browser`` are skipped."""
    index = {name: tid for tid, name in enumerate(references)}
    names, number = ([], {}) if named else (["regions"], {})
    per_seq = [[] for _ in references]          # (start, end, group, line number)
    for lineno, line in enumerate(text.splitlines(), 1):
        line = line.rstrip("\r")
        if not line.strip() or line.startswith("#") or line.split(None, 1)[0] in ("track", "browser"):
            continue
        cols = line.split("\t")
        if len(cols) < 3:
            raise ValueError("regions, line %d: expected 'sequence<TAB>start<TAB>end', found %r" % (lineno, line))
        seq = cols[0]
        try:
            start, end = int(cols[1]), int(cols[2])
        except ValueError:
            raise ValueError("regions, line %d: the coordinates %r and %r are no integers" % (lineno, cols[1], cols[2])) from None
        if seq not in index:
            raise ValueError("regions, line %d: the header has no sequence named %r" % (lineno, seq))
        if start < 0 or start >= end:
            raise ValueError("regions, line %d: [%d, %d) is not 0 <= start < end" % (lineno, start, end))
        if end > int(lengths[index[seq]]):
            raise ValueError("regions, line %d: the end %d lies beyond the %d bases of sequence %r"
                             % (lineno, end, int(lengths[index[seq]]), seq))
        group = 0
        if named:
            if len(cols) < 4 or not cols[3]:
                raise ValueError("regions, line %d: no group name in column 4" % lineno)
            if cols[3] == CATCH_ALL_GROUP:
                raise ValueError("regions, line %d: the group name %r is taken by the records outside every region"
                                 % (lineno, CATCH_ALL_GROUP))
            if cols[3] not in number:
                number[cols[3]] = len(names)
                names.append(cols[3])
            group = number[cols[3]]
        per_seq[index[seq]].append((start, end, group, lineno))
    iv_off, iv_start, iv_end, iv_group = [0], [], [], []
    for ivs in per_seq:
        ivs.sort()
        first = len(iv_start)
        members = []                            # the lines merged into the last interval
        for start, end, group, lineno in ivs:
            if len(iv_start) > first and start <= iv_end[-1] and group == iv_group[-1]:
                iv_end[-1] = max(iv_end[-1], end)
                members.append((start, end, lineno))
                continue
            if len(iv_start) > first and start < iv_end[-1]:
                other = next(n for s, e, n in members if s < end and e > start)
                raise ValueError("regions, lines %d and %d: regions of the groups %r and %r overlap"
                                 % (min(other, lineno), max(other, lineno), names[iv_group[-1]], names[group]))
            iv_start.append(start); iv_end.append(end); iv_group.append(group)
            members = [(start, end, lineno)]
        iv_off.append(len(iv_start))
    names.append(CATCH_ALL_GROUP)
    return (names, np.asarray(iv_off, dtype=np.int64), np.asarray(iv_start, dtype=np.int32), np.asarray(iv_end, dtype=np.int32),
            np.asarray(iv_group, dtype=np.int32))


class Regions(NamedTuple):
    """The intervals of ``parse_regions`` and the lengths of the header's sequences: what a region run hands to
    ``DamageEngine.set_strata_regions`` and to ``region_groups_text``."""
    iv_off: np.ndarray
    iv_start: np.ndarray
    iv_end: np.ndarray
    iv_group: np.ndarray
    lengths: list


def region_groups_text(groups, iv_start, iv_end, iv_group, lengths, kept):
    """``by_region/groups.tsv``: index, group name, regions and bases after merging, kept reads (``kept[g]``); the last
    group — ``*`` — has no regions and the bases of the genome that no region covers."""
    ng = len(groups)
    span = np.asarray(iv_end, np.int64) - np.asarray(iv_start, np.int64)
    n_regions = np.bincount(np.asarray(iv_group, np.int64), minlength=ng)
    n_bases = np.bincount(np.asarray(iv_group, np.int64), weights=span, minlength=ng).astype(np.int64)
    n_bases[ng - 1] = int(np.sum(np.asarray(lengths, np.int64))) - int(span.sum())
    out = io.StringIO()
    out.write("Index\tGroup\tRegions\tBases\tReads\n")
    for g, name in enumerate(groups):
        out.write("%d\t%s\t%d\t%d\t%d\n" % (g, name, int(n_regions[g]), int(n_bases[g]), int(kept[g])))
    return out.getvalue()


@dataclass
class StratifiedTables:
    """What a stratified ``DamageEngine.finish()`` returns: ``strata`` — the block as the device holds it, one table per
    (library, group), library-major —, ``group(g)`` — the ``TableSet`` of group ``g`` over the libraries —, and ``merged`` —
    the groups of each library summed: the tables of the run without strata.  ``kept``: records the flag filter kept, per
    stratum (``DamageEngine.strata_kept``; the block itself counts them once for the whole run)."""
    libraries: list
    groups: list
    strata: TableSet
    kept: np.ndarray = None
    merged: TableSet = None
    pmd_hist: np.ndarray = None      # --by-pmd-score: kept records per library and bin of the score (``pmd.scores_text``)
    pmd_unqualified: int = 0         # ... and those of them scored without qualities

    @classmethod
    def from_block(cls, strata, libraries, groups, kept=None):
        libraries = [tuple(x) for x in libraries]
        nl, ng = len(libraries), len(groups)
        assert strata.mis.shape[0] == nl * ng, (strata.mis.shape, nl, ng)
        kept = np.zeros(nl * ng, np.uint64) if kept is None else np.asarray(kept, np.uint64).reshape(nl * ng)
        out = cls(libraries, [str(g) for g in groups], strata, kept)
        over = strata.lgd_over.copy()
        if over.shape[0]:
            over[:, 0] //= ng
        out.merged = TableSet(libraries, strata.length, strata.around, out._split(strata.mis).sum(axis=1, dtype=np.uint64),
                              out._split(strata.comp).sum(axis=1, dtype=np.uint64), out._split(strata.lgd).sum(axis=1, dtype=np.uint64),
                              over, strata.n_kept)
        return out

    @property
    def n_kept(self):
        return self.strata.n_kept

    def _split(self, a):
        return a.reshape((len(self.libraries), len(self.groups)) + a.shape[1:])

    def group_kept(self, g):
        return int(self._split(self.kept)[:, g].sum())

    def group(self, g):
        """The tables of group ``g`` (index or name), indexed by library."""
        if not isinstance(g, (int, np.integer)):
            g = self.groups.index(g)
        ng = len(self.groups)
        s = self.strata
        over = s.lgd_over[s.lgd_over[:, 0] % ng == g].copy() if s.lgd_over.shape[0] else s.lgd_over.copy()
        if over.shape[0]:
            over[:, 0] //= ng
        return TableSet(self.libraries, s.length, s.around, self._split(s.mis)[:, g].copy(), self._split(s.comp)[:, g].copy(),
                        self._split(s.lgd)[:, g].copy(), over, self.group_kept(g))

    def groups_text(self, group_of_tid):
        """``groups.tsv``: index, group name, number of sequences, kept reads."""
        n_seq = np.bincount(np.asarray(group_of_tid, dtype=np.int64), minlength=len(self.groups))
        out = io.StringIO()
        out.write("Index\tGroup\tSequences\tReads\n")
        for g, name in enumerate(self.groups):
            out.write("%d\t%s\t%d\t%d\n" % (g, name, int(n_seq[g]), self.group_kept(g)))
        return out.getvalue()

    def kept_groups_text(self):
        """``by_damage/groups.tsv``, ``by_pmd/groups.tsv``: index, group name, kept reads."""
        from .pmd import groups_text
        return groups_text(self.groups, [self.group_kept(g) for g in range(len(self.groups))])
    damage_groups_text = kept_groups_text

    def conditional_text(self, single_stranded=False):
        """``by_damage/conditional.tsv`` of a run stratified by terminal damage (groups ``none, 5p, 3p, both``): the
        substitution frequency at one end given the damage state of the OTHER end — the conditional substitution analysis
        that tells a damaged library from a contaminated one (a row conditioned on its own end would be 1 by construction
        within the positions the groups were told by).  Per library (the emitters' order), end (5p, then 3p), condition
        (``all``, other end damaged, other end undamaged) and position 1..length, strands summed: 5p rows C>T over C; 3p
        rows G>A over G (``single_stranded``: C>T over C).  ``Frequency`` as ``damage_frequency_text`` writes it."""
        if self.groups != ["none", "5p", "3p", "both"]:
            raise ValueError("conditional_text: the groups are not those of terminal damage")
        mis = self._split(self.strata.mis)                  # [library][group][end][strand][pos][col]
        rows = (("5p", "C>T", "C", (("all", (0, 1, 2, 3)), ("3p-damaged", (2, 3)), ("3p-undamaged", (0, 1)))),
                ("3p",) + (("C>T", "C") if single_stranded else ("G>A", "G")) +
                ((("all", (0, 1, 2, 3)), ("5p-damaged", (1, 3)), ("5p-undamaged", (0, 2))),))
        out = io.StringIO()
        out.write("Sample\tLibrary\tEnd\tPos\tGiven\tSubstitutions\tBases\tFrequency\n")
        for (sample, library), li in sorted((tuple(lib), i) for i, lib in enumerate(self.libraries)):
            for end, num_col, den_col, conditions in rows:
                ei = L.ENDS.index(end)
                for given, groups in conditions:
                    block = mis[li, list(groups), ei].sum(axis=(0, 1), dtype=np.uint64)         # [pos][col]
                    for p in range(self.strata.length):
                        num, den = int(block[p, L.MIS_COLS.index(num_col)]), int(block[p, L.MIS_COLS.index(den_col)])
                        out.write("%s\t%s\t%s\t%d\t%s\t%d\t%d\t%s\n"
                                  % (sample, library, end, p + 1, given, num, den, "%.15g" % (num / den) if den else "NaN"))
        return out.getvalue()

    def write(self, folder, group_of_tid=None, subdir="by_reference", groups_text=None, usual=None):
        """The run's three files into ``folder`` from the merged block (``usual``: from that ``TableSet`` instead), and
        ``folder/subdir``: ``groups.tsv`` (``groups_text``; default: that of the sequence groups ``group_of_tid``) and one
        directory per group, named by its index (sequence names hold ``*``, ``:`` and ``/``), with the three files of that
        group written by the same emitters."""
        import pathlib
        folder = pathlib.Path(folder)
        (self.merged if usual is None else usual).write(folder)
        sub = folder / subdir
        sub.mkdir(parents=True, exist_ok=True)
        (sub / "groups.tsv").write_text(self.groups_text(group_of_tid) if groups_text is None else groups_text)
        for g in range(len(self.groups)):
            (sub / str(g)).mkdir(exist_ok=True)
            self.group(g).write(sub / str(g))

    def sum_of_groups(self, groups):
        """The ``TableSet`` of the libraries summed over the groups ``groups`` (indices) — ``TableSet.add`` on the host."""
        total = None
        for g in groups:
            total = self.group(g) if total is None else total.add(self.group(g))
        return total
