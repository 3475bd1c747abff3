"""CPU: the pure pieces of the sharded movie driver -- the two wire formats and the round plan -- without a process group."""
import numpy as np
import pytest

from tissue_image_processing_amd.movie import GpuFrameBackend

TYPE_COLUMNS = GpuFrameBackend.CELL_TYPE_COLUMNS


def _table(n, seed, typed):
    rng = np.random.default_rng(seed)
    tb = dict(area=rng.integers(0, 500, n).astype(np.int64), cy=rng.uniform(0, 99, n), cx=rng.uniform(0, 99, n),
              drift=rng.normal(0, 2, 2))
    if typed:
        tb.update(type=rng.integers(0, 2, n).astype(np.uint8), valid=rng.integers(0, 2, n).astype(np.uint8),
                  mean_intensity=rng.normal(10, 3, n))
        tb["mean_intensity"][:1] = np.nan                    # an absent row
    return tb


@pytest.mark.parametrize("typed", [False, True])
def test_table_payload_round_trip(typed):
    from tissue_image_processing_amd import movie
    extra = TYPE_COLUMNS if typed else ()
    sent = {3: _table(5, 0, typed), 7: _table(0, 1, typed), 11: _table(2, 2, typed)}
    flat = movie.pack_tables(sent, extra)
    assert flat.dtype == np.float64 and flat.size == sum(4 + (3 + len(extra)) * tb["area"].size for tb in sent.values())
    got = movie.unpack_tables(flat, extra)
    assert list(got) == [3, 7, 11]
    for t, tb in sent.items():
        assert sorted(got[t]) == sorted(tb)
        for k, v in tb.items():
            assert got[t][k].dtype == v.dtype, (t, k)
            np.testing.assert_array_equal(got[t][k], v)      # (NaN == NaN here)
        assert got[t]["drift"].base is None                  # a pair of its own, not a view of the payload
    if typed:
        assert np.isnan(got[3]["mean_intensity"][0])
    assert movie.pack_tables({}, extra).shape == (0,) and movie.unpack_tables(np.zeros(0), extra) == {}


def test_lookup_payload_round_trip():
    from tissue_image_processing_amd import movie
    sent = {4: np.array([7, -1, 0, 12], np.int32), 5: np.zeros(0, np.int32), 9: np.array([-1], np.int64)}
    flat = movie.pack_lookups(sent)
    assert flat.dtype == np.int64 and flat.size == 2 * 3 + 5
    got = movie.unpack_lookups(flat)
    assert list(got) == [4, 5, 9]
    for t, hits in sent.items():
        assert got[t].dtype == np.int64
        np.testing.assert_array_equal(got[t], hits)
    empty = movie.pack_lookups({})
    assert empty.dtype == np.int64 and empty.shape == (0,) and movie.unpack_lookups(empty) == {}


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
