"""Worker for the gloo tests of tests/test_exchanges_host.py, argv = (out path, mode):
"seg<frames>"  movie.save_seg of the first frames of overlays_small, every rank holding only its own frames' parts: rank 0 writes
               <out>.seg, every rank pickles what save_seg returned to <out>.rank<r>.pkl;
"dup"          movie.find_events with an id twice among the valid rows of frame 1: every rank writes the exception it got, type
               name and message on two lines, to <out>.rank<r>.err and exits 0."""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seg_inputs(frames):
    """(movie, tables, ids) of the archive tests: the first `frames` frames of overlays_small, every row's id its label"""
    import events_cases as ec
    from _movie_events_worker import driver_inputs
    movie = ec.first_frames(ec.load_movie("overlays_small"), frames)
    return movie, driver_inputs(movie)[0], [np.arange(1, int(lab.max()) + 1) for lab in movie["labels"]]


def duplicated_ids(movie, ids, t):
    """ids with frame t's second valid row carrying the id of its first"""
    import events_cases as ec
    rows = np.flatnonzero(ec.frame_rows(movie, t)["sel"])
    twice = [i.copy() for i in ids]
    twice[t][rows[1]] = twice[t][rows[0]]
    return twice


def main():
    import events_cases as ec
    from _movie_events_worker import EventsBackend, driver_inputs
    from gloo_launch import gloo_group
    from tissue_image_processing_amd import movie as mv
    from tissue_image_processing_amd.pipeline import frames_for_rank
    out_path, mode = sys.argv[1], sys.argv[2]
    rank = int(os.environ["RANK"])
    if mode.startswith("seg"):
        from test_events_host import _ArchivedBackend
        frames = int(mode[3:])
        movie, tables, ids = seg_inputs(frames)
        with gloo_group() as (rank, world, dist):
            backend = _ArchivedBackend(movie)
            backend.archive_frames = {t: backend.archive_frames[t] for t in frames_for_rank(frames, rank, world)}
            got = mv.save_seg(out_path, frames, backend, *((tables, ids) if rank == 0 else (None, None)), rank, world, dist, "cpu")
            with open("%s.rank%d.pkl" % (out_path, rank), "wb") as fh:
                pickle.dump(got, fh)
        return
    movie = ec.first_frames(ec.load_movie("overlays_small"), 3)
    tables, ids = driver_inputs(movie)
    try:
        with gloo_group() as (rank, world, dist):
            assert 1 in frames_for_rank(3, 1, world)
            given = (tables, duplicated_ids(movie, ids, 1)) if rank == 0 else (None, None)
            mv.find_events(3, EventsBackend(movie, rank, world), *given, rank, world, dist, "cpu")
    except Exception as e:      # (the group is gone by now, without a barrier)
        with open("%s.rank%d.err" % (out_path, rank), "w") as fh:
            fh.write("%s\n%s" % (type(e).__name__, e))


if __name__ == "__main__":
    main()
