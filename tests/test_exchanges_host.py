"""CPU: what the sharded drivers send between ranks.  The one record format (_collectives.pack_records / unpack_records) round-trips
every exchange's own field tuple, and the exchanges that only a GPU machine ran before run under gloo -- save_seg's member gather
at worlds 2 and 3, find_events' failure path at world 2."""
import pickle

import numpy as np
import pytest

from gloo_launch import run_ranks

NAN_WITH_PAYLOAD = np.array([0x7FF8DEADBEEF0001], np.uint64).view(np.float64)[0]
MEMBERS = [("a.npy", b"\x01\x02\x03", 0xFFFFFFFF, 3), ("frame_10_data.pkl", b"", 0, 0), ("b", bytes(range(17)), 5, 1 << 33)]


def _table(n, seed, typed):
    rng = np.random.default_rng(seed)
    tb = dict(area=rng.integers(0, 500, n).astype(np.int64), cy=rng.uniform(0, 99, n), cx=rng.uniform(0, 99, n),
              drift=rng.normal(0, 2, 2))
    if typed:
        tb.update(type=rng.integers(0, 2, n).astype(np.uint8), valid=rng.integers(0, 2, n).astype(np.uint8),
                  mean_intensity=rng.normal(10, 3, n))
        tb["mean_intensity"][:1] = np.nan                    # an absent row
    return tb


def _exchanges():
    """{name: (the exchange's field tuple, as its module declares it, {key: record})}"""
    from tissue_image_processing_amd import events, movie, seg_archive, tiling
    i32 = lambda *v: np.array(v, np.int32)
    u8 = lambda *v: np.array(v, np.uint8)
    return {
        "tables": (movie.TABLE_FIELDS, {3: _table(5, 0, False), 7: _table(0, 1, False), 11: _table(2, 2, False)}),
        "typed tables": (movie.TABLE_FIELDS + tuple(movie.GpuFrameBackend.CELL_TYPE_COLUMNS),      # keys descending
                         {11: _table(5, 0, True), 7: _table(0, 1, True), 3: _table(2, 2, True)}),
        "lookups": (movie.LOOKUP_FIELDS, {4: dict(hits=i32(7, -1, 0, 12)), 5: dict(hits=np.zeros(0, np.int32)),
                                          9: dict(hits=np.array([-1], np.int64))}),
        "ids": (seg_archive.ID_FIELDS, {1: dict(ids=np.array([2 ** 53 + 1, 2 ** 62, -2 ** 31], np.int64)), 0: dict(ids=np.zeros(0, np.int64))}),
        "members": (seg_archive.MEMBER_FIELDS, seg_archive.members_as_records(MEMBERS)),
        "hand-out": (events.MOVIE_FIELDS, {0: dict(drift=np.array([-0.0, NAN_WITH_PAYLOAD]), id=np.array([5, 2 ** 53 + 1, 9], np.int64),
                                                   cy=np.array([1.5, np.nan, NAN_WITH_PAYLOAD]), cx=np.array([0.25, -0.0, 7.0])),
                                           1: dict(drift=np.zeros(2), id=np.zeros(0, np.int64), cy=np.zeros(0), cx=np.zeros(3))}),
        "rows": (events.ROW_FIELDS, {2: dict(sel=u8(1, 0, 1), pos=u8(0, 0, 1), edge=u8(1, 1, 0), offsets=i32(0, 2, 2, 3), adj=i32(1, 2, 0),
                                             under_next=np.zeros(0, np.int32)),      # the last frame: nothing under a next one
                                     0: dict(sel=u8(*range(9)), pos=u8(*[1] * 9), edge=u8(*[0] * 9), offsets=np.zeros(10, np.int32),
                                             adj=np.zeros(0, np.int32), under_next=i32(-1, -2 ** 31, 2 ** 31 - 1))}),
        "found": (events.FOUND_FIELDS, {1: dict(delam=np.array([4, 0]), diff=np.zeros(0, np.int64), division=np.array([2]), mother=np.array([-1])),
                                        2: {name: np.zeros(0, np.int64) for name, _ in events.FOUND_FIELDS}}),
        "tiles": (tiling.TILE_FIELDS, {3: dict(proj=np.arange(24.0).reshape(2, 3, 4) / 7, zmap=np.array([[2 ** 53 + 1, -1, 0]] * 4).T),
                                       0: dict(proj=np.zeros((2, 0, 4)), zmap=np.zeros((0, 4), np.int64))}),
    }


@pytest.mark.parametrize("name", ["tables", "typed tables", "lookups", "ids", "members", "hand-out", "rows", "found", "tiles"])
def test_record_round_trip(name):
    """Every exchange's payload comes back as sent: the keys in their order, every field in its declared dtype and byte for byte,
    each array owning its data; the payload is as long as the format says, and the empty one works in both directions."""
    from tissue_image_processing_amd._collectives import pack_records, unpack_records
    fields, sent = _exchanges()[name]
    flat = pack_records(sent, fields)
    words = lambda a, dtype: -(-np.asarray(a).size * np.dtype(dtype).itemsize // 8)
    assert flat.dtype == np.int64 and flat.ndim == 1
    assert flat.size == sum(1 + len(fields) + sum(words(r[f], dtype) for f, dtype in fields) for r in sent.values())
    got = unpack_records(flat, fields)
    assert list(got) == list(sent)
    for key, record in sent.items():
        assert sorted(got[key]) == sorted(f for f, _ in fields)
        for f, dtype in fields:
            want = np.asarray(record[f]).astype(dtype).ravel()
            assert got[key][f].dtype == np.dtype(dtype) and got[key][f].shape == want.shape, (key, f)
            np.testing.assert_array_equal(got[key][f], want)      # (NaN == NaN here)
            assert got[key][f].tobytes() == want.tobytes(), (key, f)
            assert got[key][f].base is None and got[key][f].flags.owndata, (key, f)      # no view of the payload
    empty = pack_records({}, fields)
    assert empty.dtype == np.int64 and empty.shape == (0,) and unpack_records(empty, fields) == {}


def test_members_come_back_equal():
    from tissue_image_processing_amd import seg_archive as sa
    from tissue_image_processing_amd._collectives import pack_records, unpack_records
    for members in (MEMBERS, []):
        assert sa.records_as_members(unpack_records(pack_records(sa.members_as_records(members), sa.MEMBER_FIELDS), sa.MEMBER_FIELDS)) == members


def test_what_the_old_formats_could_not_hold():
    """the cases above hold them; this says so: an int64 above 2^53, a NaN with payload bits, uint8 fields of 3, 9 and 17 bytes, an
    empty field next to a full one, a negative int32 and keys that do not ascend"""
    ex = _exchanges()
    assert float(np.int64(2 ** 53 + 1)) != 2 ** 53 + 1 and ex["ids"][1][1]["ids"][0] == 2 ** 53 + 1
    assert np.isnan(NAN_WITH_PAYLOAD) and NAN_WITH_PAYLOAD.tobytes() != np.float64(np.nan).tobytes()
    assert sorted(r["stream"].size for r in ex["members"][1].values()) == [0, 3, 17] and ex["rows"][1][0]["sel"].size == 9
    assert ex["rows"][1][2]["under_next"].size == 0 < ex["rows"][1][2]["adj"].size and ex["rows"][1][0]["under_next"].min() == -2 ** 31
    assert list(ex["typed tables"][1]) == [11, 7, 3] and list(ex["ids"][1]) == [1, 0]


# ---- save_seg's member gather ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world1_archives(tmp_path_factory):
    """{frames: the bytes of the archive one process writes}"""
    from _exchange_worker import seg_inputs
    from test_events_host import _ArchivedBackend
    from tissue_image_processing_amd import movie as mv
    out = {}
    for frames in (3, 2):
        movie, tables, ids = seg_inputs(frames)
        path = mv.save_seg(str(tmp_path_factory.mktemp("seg") / "world1"), frames, _ArchivedBackend(movie), tables, ids)
        with open(path, "rb") as fh:
            out[frames] = fh.read()
    return out


@pytest.mark.parametrize("world,frames", [(2, 3), (3, 3), (3, 2)])
def test_save_seg_gathers_the_archive_one_process_writes(tmp_path, world1_archives, world, frames):
    """every rank holds only its own frames' parts; (3, 3): one frame per rank; (3, 2): rank 2 owns nothing"""
    out = tmp_path / "movie"
    run_ranks("_exchange_worker.py", world, (out, "seg%d" % frames), timeout=120)
    returned = []
    for r in range(world):
        with open("%s.rank%d.pkl" % (out, r), "rb") as fh:
            returned.append(pickle.load(fh))
    assert returned == [str(out) + ".seg"] + [None] * (world - 1)
    with open(returned[0], "rb") as fh:
        assert fh.read() == world1_archives[frames]


# ---- find_events' failure path ------------------------------------------------------------------------------------------------------
def test_find_events_owner_failure_reaches_both_ranks(tmp_path):
    """frame 1, rank 1's, has an id twice among its valid rows: the owner raises its own error, rank 0 one that names the owner,
    and both processes exit (run_ranks waits for them) -- neither is left in a collective"""
    out = tmp_path / "dup"
    run_ranks("_exchange_worker.py", 2, (out, "dup"), timeout=120)
    kinds, texts = zip(*(open("%s.rank%d.err" % (out, r)).read().split("\n", 1) for r in range(2)))
    assert kinds == ("RuntimeError", "ValueError")
    assert "failed on rank 1" in texts[0] and "two valid" in texts[1]
