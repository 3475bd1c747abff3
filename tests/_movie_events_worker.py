"""The CPU stand-in for GpuFrameBackend's event methods (the numpy restatement behind the same interface, in the style of
_movie_worker.OracleBackend) and the worker for the gloo tests of movie.find_events in tests/test_events_host.py: both golden
movies at 5 and at 2 frames in one process group; rank 0 pickles the four tables to argv[1]."""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_COUNTS = (5, 2)


class EventsBackend(object):
    """Holds this rank's frames of a movie of events_cases (label maps and tables) as a backend that archived them."""

    def __init__(self, movie, rank, world):
        from tissue_image_processing_amd.pipeline import frames_for_rank
        self.movie = movie
        self.archive = dict(type_name="HC")
        self.archive_frames = {t: movie["tables"][t] for t in frames_for_rank(len(movie["labels"]), rank, world)}

    def event_rows(self, t):
        import events_cases as ec
        assert t in self.archive_frames
        rows = ec.frame_rows(self.movie, t)
        del rows["id"]
        return rows

    def border_rows(self, t):
        import events_restate as er
        assert t in self.archive_frames
        return er.border_rows(self.movie["labels"][t], self.movie["tables"][t]["label"].size)

    def lookup_exact(self, t, qy, qx):
        import events_restate as er
        assert t in self.archive_frames
        return er.lookup_exact(self.movie["labels"][t], qy, qx)

    def classify_pair(self, t, prev, cur, first_edge_ids):
        import events_restate as er
        from tissue_image_processing_amd import events as ev
        assert t in self.archive_frames
        return ev.found_rows(er.event_flags(prev, cur, first_edge_ids), prev, cur, self.movie["tables"][t]["neighbors"])


def driver_inputs(movie):
    """(tables, ids) as process_movie leaves them on rank 0"""
    tables = [dict(area=tab["area"], cy=tab["cy"], cx=tab["cx"], type=tab["type"], drift=movie["drifts"][t].copy())
              for t, tab in enumerate(movie["tables"])]
    return tables, [tab["label"].astype(np.int64) for tab in movie["tables"]]


def main():
    import events_cases as ec
    from gloo_launch import gloo_group
    from tissue_image_processing_amd import movie as mv
    out = {}
    with gloo_group() as (rank, world, dist):
        for name in ec.MOVIES:
            for frames in FRAME_COUNTS:
                movie = ec.first_frames(ec.load_movie(name), frames)
                tables, ids = driver_inputs(movie) if rank == 0 else (None, None)
                table = mv.find_events(frames, EventsBackend(movie, rank, world), tables, ids, rank, world, dist, "cpu")
                assert (table is None) == (rank != 0)
                out[(name, frames)] = table
        if rank == 0:
            with open(sys.argv[1], "wb") as fh:
                pickle.dump(out, fh)


if __name__ == "__main__":
    main()
