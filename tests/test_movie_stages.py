"""CPU: the pure pieces of the sharded movie driver -- the round plan and the stages of a round -- without a process group."""
import numpy as np
import pytest


@pytest.mark.parametrize("n_frames,world,block", [(7, 4, 1), (7, 4, 2), (1, 4, 1), (3, 4, None), (6, 2, None)])
def test_round_plan(n_frames, world, block):
    from tissue_image_processing_amd import movie
    plans = [movie.plan_rounds(n_frames, r, world, block) for r in range(world)]
    assert len(set(len(p) for p in plans)) == 1 and len(plans[0]) >= 1          # every rank runs the same rounds
    assert sorted(t for p in plans for frames in p for t in frames) == list(range(n_frames))
    per_round = (block if block else -(-n_frames // world)) * world
    for p in plans:
        for k, frames in enumerate(p):
            assert all(t // per_round == k for t in frames)


def _recording(base):
    """`base` with every drift-related backend call of frame t noted in self.calls[t], in order."""
    class Recording(base):
        def __init__(self):
            base.__init__(self)
            self.calls = {}

    def noting(name):
        def method(self, t, *args):
            self.calls.setdefault(t, []).append(name)
            return getattr(base, name)(self, t, *args)
        return method

    for name in ("lookup", "drift", "piv_lookup", "local_drift_lookup"):
        if hasattr(base, name):
            setattr(Recording, name, noting(name))
    return Recording()


@pytest.mark.parametrize("source,per_frame", [("given", ["lookup"]), ("estimate", ["drift", "lookup"]), ("piv", ["piv_lookup"])])
def test_backend_calls_per_drift_source(golden, source, per_frame):
    """One process, the three-frame tracking golden (rows padded with background to a square 120 x 120, which upstream's
    transposed PIV sampling needs) next to a smooth plane: each drift source asks the backend for exactly its own steps, once
    per frame t >= 1 and in this order, and the first frame for none."""
    from _movie_worker import OracleBackend, PivOracleBackend
    from tissue_image_processing_amd import movie
    labs = [np.pad(lab, ((0, 24), (0, 0))) for lab in golden("tracking")["labels"]]
    ramp = np.add.outer(np.arange(120.0), 2.0 * np.arange(120.0))
    frames = [(lab, 100.0 + 50.0 * np.sin((ramp + t) / 9.0)) for t, lab in enumerate(labs)]
    backend = _recording(PivOracleBackend if source == "piv" else OracleBackend)
    kw = {"given": dict(drifts=np.array([(0.0, 0.0), (0.5, -0.3), (0.5, -0.3)])), "estimate": dict(estimate_drift=True),
          "piv": dict(use_piv=True)}[source]
    tables, ids = movie.process_movie(3, lambda t: frames[t], backend, 0, 1, None, "cpu", **kw)
    assert len(tables) == len(ids) == 3
    assert backend.calls == {1: per_frame, 2: per_frame}
