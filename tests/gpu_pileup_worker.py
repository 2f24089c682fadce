"""A fresh process for tests/test_gpu_pileup.py: the add kernel's list takes its capacity from MDX_TEST_PILEUP_LIST where
``pileup_begin`` reads it, so a list of a few dozen pairs needs an environment of its own.  argv: a directory, then NAME per case
-> for DIR/NAME.bam over the test module's dense sites, DIR/NAME.npz with what ``pileup_finish`` gives and ``pileup_info``."""
import os
import sys

import numpy as np


def main(directory, *cases):
    from mapdamage_amd.engine import DamageEngine
    from tests.test_gpu_pileup import DENSE_LENGTHS, DENSE_SITES, LIBS3, add_file, begin
    with DamageEngine(LIBS3) as eng:
        for name in cases:
            begin(eng, DENSE_LENGTHS, DENSE_SITES, min_basequal=20, mask_ends=(2, 1), call="majority", seed=3)
            add_file(eng, os.path.join(directory, name + ".bam"))
            counters, refbase, call, depth, counts = eng.pileup_finish()
            info = eng.pileup_info()
            np.savez(os.path.join(directory, name + ".npz"), counters=counters, refbase=refbase, call=call, depth=depth,
                     counts=np.array([counts[k] for k in ("counted", "outside", "over_a_site", "pairs")], np.uint64),
                     info=np.array([info[k] for k in ("list_pairs", "block_records", "bytes", "sites")], np.uint64))


if __name__ == "__main__":
    main(*sys.argv[1:])
