"""Worker for the gloo runs of tests/test_movie_piv.py: movie.process_movie(use_piv=True) over _movie_worker's numpy
stand-in for the device step.  An IndexError is written to argv[1].rank<r>.err, not raised out of the process."""
import os
import sys

import numpy as np

from _movie_worker import PivOracleBackend, golden_frames, save_ids
from gloo_launch import gloo_group


def main():
    from tissue_image_processing_amd import movie
    out_path, mode = sys.argv[1], sys.argv[2]
    block = int(sys.argv[3]) if len(sys.argv) > 3 and int(sys.argv[3]) > 0 else None
    frames = golden_frames(crop=(mode == "crop"))
    try:
        with gloo_group() as (rank, world, dist):
            tabs, ids = movie.process_movie(len(frames), lambda t: frames[t], PivOracleBackend(), rank, world, dist, "cpu",
                                            block_frames=block, use_piv=True)
            if rank == 0:
                save_ids(out_path, ids, drifts=np.array([tb["drift"] for tb in tabs]))
    except IndexError as e:      # (the group is gone by now, without a barrier)
        with open("%s.rank%s.err" % (out_path, os.environ["RANK"]), "w") as f:
            f.write(str(e))


if __name__ == "__main__":
    main()
