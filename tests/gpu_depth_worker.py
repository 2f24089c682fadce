"""A fresh process for tests/test_gpu_depth.py: the finish of --depth reads MDX_TEST_DEPTH_ROUND where the accumulator is
allocated, so a scan of four tiles a round starts cold.  argv: a directory, then NAME:BASES per case -> for DIR/NAME.bam over a
reference of one sequence of BASES bases, DIR/NAME.npz with what ``collect`` of the test module gives and ``depth_info``."""
import os
import sys

import numpy as np


def main(directory, *cases):
    from mapdamage_amd.engine import DamageEngine
    from tests.test_gpu_depth import LIBS3, add_file, begin, collect
    with DamageEngine(LIBS3) as eng:
        for case in cases:
            name, bases = case.split(":")
            lengths = [int(bases)]
            begin(eng, lengths)
            add_file(eng, os.path.join(directory, name + ".bam"))
            got = collect(eng, lengths)
            info = eng.depth_info()
            np.savez(os.path.join(directory, name + ".npz"), fetch=got["fetch"][0], per_contig=got["per_contig"], hist=got["hist"],
                     counts=np.array([got["counts"][k] for k in ("counted", "outside", "intervals", "runs")], np.uint64),
                     run_tid=got["runs"][0], run_start=got["runs"][1], run_end=got["runs"][2], run_depth=got["runs"][3],
                     info=np.array([info[k] for k in ("block_records", "tile", "round_tiles", "bytes")], np.uint64))


if __name__ == "__main__":
    main(*sys.argv[1:])
