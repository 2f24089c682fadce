"""Helpers of the terminal-damage tests (``--by-terminal-damage``, include/mdx.h ``mdx_set_strata_damage``): a record's group
read from the reference-pinned CPU oracle run on that record alone — it shares nothing with the product, which assigns on the
device only."""

import functools

import numpy as np

from mapdamage_amd import layout as L
from tests.util import oracle_tableset

GROUPS = ["none", "5p", "3p", "both"]
_CT, _GA = L.MIS_COLS.index("C>T"), L.MIS_COLS.index("G>A")
_E3, _E5 = L.ENDS.index("3p"), L.ENDS.index("5p")
NEVER = 1 << 30


def first_damage(ref, batch, libs, minqual, length=70, around=10):
    """Per record the lowest index at which the oracle's tables of that record alone count C>T at the 5p end, G>A at the 3p
    end and C>T at the 3p end (``NEVER`` where none; a record the flag filter drops, or one the oracle refuses, counts
    nothing): int64 [n][3]."""
    from oracle.oracle import OracleError
    out = np.full((batch.n, 3), NEVER, np.int64)
    for i in range(batch.n):
        try:
            mis = oracle_tableset(ref, batch.slice(i, i + 1), libs, length, around, minqual).mis
        except OracleError:
            continue
        for k, (end, col) in enumerate(((_E5, _CT), (_E3, _GA), (_E3, _CT))):
            hit = np.flatnonzero(mis[:, end, :, :, col].any(axis=(0, 1)))
            if hit.size:
                out[i, k] = hit[0]
    return out


def groups_of(first, positions, single_stranded=False):
    """The group (index into ``GROUPS``) of every record for ``positions`` terminal positions."""
    p5 = first[:, 0] < positions
    p3 = first[:, 2 if single_stranded else 1] < positions
    return p5.astype(np.int64) + 2 * p3.astype(np.int64)


def pack4(seq, qual=None, minqual=0):
    """An ASCII SEQ column as MDX_SEQ_4BIT bytes (include/mdx.h: low nibble first, A C T G = 1 2 4 8, else 0); with
    ``qual`` and ``minqual`` as MDX_SEQ_4BITQ (a base below the threshold is the complement of its code)."""
    code = np.zeros(256, np.uint8)
    for ch, c in zip(b"ACTG", (1, 2, 4, 8)):
        code[ch] = c
    nib = code[seq]
    if qual is not None and minqual:
        nib = np.where(qual < minqual, nib ^ 15, nib).astype(np.uint8)
    if nib.shape[0] & 1:
        nib = np.concatenate([nib, np.zeros(1, np.uint8)])
    return (nib[0::2] | (nib[1::2] << 4)).astype(np.uint8)


def resident_reference(ref):
    """The reference as the device holds it (MdxTabArgs::ref): upper-case ASCII for A C G T, 0x84 for '-', 0x85 for the rest."""
    bases, offs = ref.concat()
    up = np.where((bases >= ord("a")) & (bases <= ord("z")), bases - 32, bases).astype(np.uint8)
    out = np.full(up.shape, 0x85, np.uint8)
    keep = np.isin(up, np.frombuffer(b"ACGT", np.uint8))
    out[keep] = up[keep]
    out[up == ord("-")] = 0x84
    return out, np.ascontiguousarray(offs, np.int64)


@functools.lru_cache(maxsize=None)
def grid_batch():
    """The grid's batch (tests/test_gpu_terminal_damage.py): 4 000 mixed records of three libraries over ``genome5()``, 5 % of
    the qualities in 2..19."""
    from mapdamage_amd import synth
    from tests.test_gpu_strata import MIXED, genome5
    b = synth.make_reads(genome5(), 4000, 91, nlib=3, with_qual=True, **MIXED)
    rng = np.random.default_rng(92)
    nb = b.seq.shape[0]
    b.qual = np.where(rng.random(nb) < 0.05, rng.integers(2, 20, nb), rng.integers(20, 42, nb)).astype(np.uint8)
    return b


@functools.lru_cache(maxsize=None)
def grid_first(minqual):
    from tests.test_gpu_strata import genome5, libraries
    return first_damage(genome5(), grid_batch(), libraries(3), minqual)
