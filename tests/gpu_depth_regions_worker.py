"""A fresh process for tests/test_gpu_depth_regions.py: MDX_TEST_DEPTH_ROUND is read where the accumulator is allocated, so a scan
of four tiles a round starts cold.  argv: a directory and the bases of the one sequence -> for DIR/in.bam and the intervals of
DIR/regions.npz (iv_off, iv_start, iv_end, iv_group), DIR/out.npz with what ``depth_regions`` and ``depth_finish`` give and
``depth_info``."""
import os
import sys

import numpy as np


def main(directory, bases):
    from mapdamage_amd.engine import DamageEngine
    from tests.test_gpu_depth import LIBS3, add_file, reference
    r = np.load(os.path.join(directory, "regions.npz"))
    with DamageEngine(LIBS3, groups=["a", "b", "*"]) as eng:
        eng.set_reference(reference([int(bases)]))
        eng.set_strata_regions(r["iv_off"], r["iv_start"], r["iv_end"], r["iv_group"])
        eng.depth_begin()
        add_file(eng, os.path.join(directory, "in.bam"))
        per_interval, per_group, group_hist = eng.depth_regions()
        per_contig, hist, _ = eng.depth_finish()
        info = eng.depth_info()
        np.savez(os.path.join(directory, "out.npz"), per_interval=per_interval, per_group=per_group, group_hist=group_hist,
                 per_contig=per_contig, hist=hist, info=np.array([info[k] for k in ("block_records", "tile", "round_tiles", "bytes")], np.uint64))


if __name__ == "__main__":
    main(*sys.argv[1:])
