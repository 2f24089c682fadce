"""A fresh process for tests/test_gpu_remove_duplicates.py: the table of --remove-duplicates reads MDX_TEST_DUP_SLOTS when the
set begins, so a run from a table of 8 slots starts cold.  argv: BAM path, slab bytes, ends, output prefix -> PREFIX.npy (the
flag column behind ``dedup_mark``, all slabs) and PREFIX.json (``dedup_info`` and the slabs)."""
import json
import sys

import numpy as np


def main(path, chunk_bytes, ends, prefix):
    from mapdamage_amd.engine import DamageEngine
    from tests.test_gpu_remove_duplicates import LIBS3, mark_file
    with DamageEngine(LIBS3) as eng:
        got = mark_file(eng, path, int(chunk_bytes), ends)
    np.save(prefix + ".npy", got["flags"])
    json.dump(dict(got["info"], slabs=len(got["slabs"])), open(prefix + ".json", "w"))


if __name__ == "__main__":
    main(*sys.argv[1:])
