"""A fresh process for tests/test_gpu_pileup_damage_likelihoods.py, as tests/gpu_pileup_gl_worker.py is one for
tests/test_gpu_pileup_likelihoods.py: the add kernel's list takes its capacity from MDX_TEST_PILEUP_LIST where ``pileup_begin``
reads it.  argv: a directory, then NAME per case -> for DIR/NAME.bam over the dense sites under the damage profile, DIR/NAME.npz
with what ``pileup_likelihoods_finish`` and ``pileup_finish`` give and ``pileup_info``."""
import os
import sys

import numpy as np


def main(directory, *cases):
    from mapdamage_amd.engine import DamageEngine
    from tests.test_gpu_pileup import DENSE_LENGTHS, DENSE_SITES, LIBS3, add_file, begin
    from tests.test_gpu_pileup_damage_likelihoods import DENSE_NOQUAL, table_of
    with DamageEngine(LIBS3) as eng:
        for name in cases:
            begin(eng, DENSE_LENGTHS, DENSE_SITES, min_basequal=20, mask_ends=(1, 0), call="majority", seed=3)
            eng.pileup_likelihoods_damage_begin(table_of(5), noqual_quality=DENSE_NOQUAL)
            add_file(eng, os.path.join(directory, name + ".bam"))
            sums, gl, best, bases, added = eng.pileup_likelihoods_finish()
            counters, refbase, call, depth, counts = eng.pileup_finish()
            info = eng.pileup_info()
            np.savez(os.path.join(directory, name + ".npz"), sums=sums, gl=gl, best=best, bases=bases,
                     added=np.array([added[k] for k in ("added", "without_qualities")], np.uint64), counters=counters, refbase=refbase, call=call, depth=depth,
                     counts=np.array([counts[k] for k in ("counted", "outside", "over_a_site", "pairs")], np.uint64),
                     info=np.array([info[k] for k in ("list_pairs", "block_records", "bytes", "sites")], np.uint64))


if __name__ == "__main__":
    main(*sys.argv[1:])
