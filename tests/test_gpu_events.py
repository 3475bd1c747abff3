"""GPU: the event kernels (csrc/tip_events.hip) -- border rows, the exact look-up and the pair classification, host forms and _dev
forms -- against the reference's goldens and the numpy restatement (tests/events_restate.py), and movie.find_events end to end:
the table the driver writes into the `.seg` archive equals what find_events_iterator builds on that same archive, loaded."""
import warnings

import numpy as np
import pytest

import events_cases as ec
import events_restate as er
from gloo_launch import run_ranks

pytestmark = pytest.mark.gpu


class HostForms(object):
    """the three entries through their host-array wrappers (the look-up's map is a device buffer, as the entry takes it)"""

    @staticmethod
    def border_rows(labels, n):
        from tissue_image_processing_amd import _segmentation as seg
        return seg.border_rows(labels, n)

    @staticmethod
    def lookup_exact(labels, qy, qx):
        from tissue_image_processing_amd import _lib, _segmentation as seg
        labels = np.ascontiguousarray(labels, np.int32)
        d_lab = _lib.DeviceBuffer(labels.nbytes).upload(labels)
        try:
            return seg.lookup_exact_dev(d_lab.ptr, labels.shape[0], labels.shape[1], qy, qx)
        finally:
            d_lab.free()

    @staticmethod
    def event_flags(prev, cur, first_edge_ids):
        from tissue_image_processing_amd import _segmentation as seg
        return seg.event_flags(prev, cur, first_edge_ids)


class DevForms(HostForms):
    """border rows and the classification on DEVICE arrays (the _dev entries), results downloaded"""

    @staticmethod
    def border_rows(labels, n):
        from tissue_image_processing_amd import _lib, _segmentation as seg
        labels = np.ascontiguousarray(labels, np.int32)
        d_lab, d_flags = _lib.DeviceBuffer(labels.nbytes).upload(labels), _lib.DeviceBuffer(max(n, 1))
        try:
            seg.border_rows_dev(d_lab.ptr, labels.shape[0], labels.shape[1], n, d_flags.ptr)
            return d_flags.download((n,), np.uint8)
        finally:
            d_lab.free()
            d_flags.free()

    @staticmethod
    def event_flags(prev, cur, first_edge_ids):
        from tissue_image_processing_amd import _lib, _segmentation as seg
        held = []

        def up(a, dtype):
            a = np.ascontiguousarray(a, dtype).reshape(-1)
            held.append(_lib.DeviceBuffer(max(a.nbytes, 16)).upload(a))
            return held[-1].ptr

        def frame(f):
            return [up(f["id"], np.int64), up(f["sel"], np.uint8), up(f["pos"], np.uint8), up(f["offsets"], np.int32), up(f["adj"], np.int32)]

        n_prev, n_cur = len(prev["id"]), len(cur["id"])
        first = np.ascontiguousarray(first_edge_ids, np.int64)
        outs = [_lib.DeviceBuffer(max(16, (n_prev if name in ("delam", "diff") else n_cur) * np.dtype(dt).itemsize)) for name, dt in seg.EVENT_OUTPUTS]
        try:
            seg.event_flags_dev(frame(prev), n_prev, len(prev["adj"]), frame(cur), n_cur, len(cur["adj"]), up(cur["edge"], np.uint8),
                                up(cur["under"], np.int32), up(first, np.int64), first.size, [o.ptr for o in outs])
            return {name: o.download((n_prev if name in ("delam", "diff") else n_cur,), dt) for (name, dt), o in zip(seg.EVENT_OUTPUTS, outs)}
        finally:
            for b in held + outs:
                b.free()


def assert_same_flags(got, want, tag=""):
    for name, _ in er.EVENT_OUTPUTS:
        np.testing.assert_array_equal(got[name], want[name], err_msg="%s %s" % (tag, name))


@pytest.mark.parametrize("impl", (HostForms, DevForms), ids=("host", "dev"))
@pytest.mark.parametrize("name", ec.MOVIES)
def test_entries_give_the_goldens_events(name, impl):
    g = ec.golden(name)
    calls = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, _ = ec.row_form(ec.load_movie(name), impl, calls)
    assert [c[0] for c in calls] == [str(v) for v in g["found_type"]]
    assert [list(c[1:]) for c in calls] == g["found_rows"].tolist()
    assert len(calls) >= 1
    for k in ec.TABLE_COLUMNS:
        np.testing.assert_array_equal(np.asarray(got[k].to_numpy(), np.float64), g["table_" + k], err_msg=k)


@pytest.mark.parametrize("impl", (HostForms, DevForms), ids=("host", "dev"))
def test_entries_equal_the_restatement_on_every_mutated_case(impl):
    ran = 0
    for tag, movie in ec.all_cases():
        for t in range(1, ec.n_frames(movie)):
            prev, cur, first = ec.pair_inputs(movie, t, impl)
            want_prev, want_cur, want_first = ec.pair_inputs(movie, t, er)
            np.testing.assert_array_equal(cur["edge"], want_cur["edge"], err_msg=tag)
            np.testing.assert_array_equal(cur["under"], want_cur["under"], err_msg=tag)
            np.testing.assert_array_equal(first, want_first, err_msg=tag)
            assert_same_flags(impl.event_flags(prev, cur, first), er.event_flags(want_prev, want_cur, want_first), "%s pair %d" % (tag, t))
            ran += 1
    assert ran >= 4 * 22


def synthetic_pair(seed=5, n_prev=5003, n_cur=4871):
    """Tables only: about 5 000 rows per frame (twenty workgroups, the last one partly filled), n_prev != n_cur, ids up to 10^6 --
    most of them shared by the two frames --, random sel / pos / edge / under, rows of 0..9 neighbours whose labels reach the
    row count, and one row with 150 neighbours in either frame."""
    rng = np.random.default_rng(seed)
    pool = rng.choice(np.arange(1, 10 ** 6 + 1), n_prev + 600, replace=False)

    def frame(n, ids):
        deg = rng.integers(0, 10, n)
        deg[n // 2] = min(150, n)
        offsets = np.zeros(n + 1, np.int32)
        offsets[1:] = np.cumsum(deg)
        adj = np.concatenate([np.sort(rng.choice(np.arange(1, n + 1), d, replace=False)) for d in deg]).astype(np.int32)
        return dict(id=ids.astype(np.int64), sel=(rng.random(n) < 0.9).astype(np.uint8), pos=(rng.random(n) < 0.3).astype(np.uint8),
                    offsets=offsets, adj=adj)

    prev = frame(n_prev, pool[:n_prev])
    cur = frame(n_cur, rng.permutation(pool[300:300 + n_cur]))
    cur["edge"] = (rng.random(n_cur) < 0.05).astype(np.uint8)
    cur["under"] = rng.integers(-1, 12, n_cur).astype(np.int32)          # few labels: neighbours often share one; -1 and 0 occur
    return prev, cur, rng.choice(pool, 200, replace=False).astype(np.int64)


@pytest.mark.parametrize("impl", (HostForms, DevForms), ids=("host", "dev"))
def test_entries_equal_the_restatement_on_large_tables(impl):
    prev, cur, first = synthetic_pair()
    want = er.event_flags(prev, cur, first)
    assert np.diff(cur["offsets"]).max() > 64 and len(prev["id"]) != len(cur["id"])
    # the case is no empty one: every output is used, several matches occur
    assert want["delam"].sum() >= 3 and want["diff"].sum() >= 3 and want["division"].sum() >= 3 and want["n_match"].max() >= 2
    assert_same_flags(impl.event_flags(prev, cur, first), want)


@pytest.mark.parametrize("impl", (HostForms, DevForms), ids=("host", "dev"))
def test_border_rows_at_the_corners_and_on_one_row(impl):
    lab = np.zeros((6, 9), np.int32)
    lab[5, 8] = 3                      # a corner pixel is the cell's only border pixel (and its only pixel)
    lab[1:5, 1:8] = 2                  # an interior cell
    lab[0, 3] = 1
    np.testing.assert_array_equal(impl.border_rows(lab, 4), [1, 0, 1, 0])
    np.testing.assert_array_equal(impl.border_rows(lab, 2), [1, 0])          # label 3 is above n: no part
    for corner in ((0, 0), (0, 8), (5, 0)):
        one = np.zeros((6, 9), np.int32)
        one[corner] = 1
        np.testing.assert_array_equal(impl.border_rows(one, 1), [1])
    row = np.array([[0, 2, 2, 0, 5, 0, 1]], np.int32)                        # a 1-row map: every pixel is border
    np.testing.assert_array_equal(impl.border_rows(row, 5), [1, 1, 0, 0, 1])
    np.testing.assert_array_equal(impl.border_rows(row.T.copy(), 5), [1, 1, 0, 0, 1])
    rng = np.random.default_rng(2)
    big = rng.integers(0, 400, (301, 517)).astype(np.int32)                  # the border spans several workgroups
    np.testing.assert_array_equal(impl.border_rows(big, 399), er.border_rows(big, 399))


def test_exact_lookup_at_the_corners_and_just_outside():
    rng = np.random.default_rng(4)
    Y, X = 37, 53
    lab = rng.integers(0, 1000, (Y, X)).astype(np.int32)
    qy = np.array([0, 0, Y - 1, Y - 1, -1, Y, 0, Y - 1, 5, 5, -1, Y], np.int64)
    qx = np.array([0, X - 1, 0, X - 1, 0, X - 1, -1, X, -1, X, -1, X], np.int64)
    got = HostForms.lookup_exact(lab, qy, qx)
    np.testing.assert_array_equal(got, er.lookup_exact(lab, qy, qx))
    assert got[:4].tolist() == [lab[0, 0], lab[0, X - 1], lab[Y - 1, 0], lab[Y - 1, X - 1]] and (got[4:] == -1).all()
    qy, qx = rng.integers(-3, Y + 3, 700), rng.integers(-3, X + 3, 700)      # three workgroups
    np.testing.assert_array_equal(HostForms.lookup_exact(lab, qy, qx), er.lookup_exact(lab, qy, qx))


def test_bad_arguments_are_refused():
    prev, cur, first = synthetic_pair(n_prev=40, n_cur=30)
    twice = dict(cur, id=cur["id"].copy(), sel=np.ones(30, np.uint8))
    twice["id"][3] = twice["id"][7]
    with pytest.raises(ValueError, match="twice"):
        HostForms.event_flags(prev, twice, first)
    with pytest.raises(ValueError):
        HostForms.event_flags(dict(prev, offsets=prev["offsets"][::-1].copy()), cur, first)
    with pytest.raises(ValueError):
        HostForms.border_rows(np.zeros((3, 3, 3), np.int32), 2)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _loaded(path):
    import _gpu_movie_seg_worker as w
    from tissue_image_processing_amd.tissue_info import Tissue
    tissue = Tissue(w.T)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in tissue.load(path):
            pass
    return tissue


def _same_table(got, want):
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    for k in want.columns:          # every column, floats exactly: both tables hold the archive's own values
        assert np.array_equal(got[k].to_numpy(), want[k].to_numpy()), k


@pytest.fixture(scope="module")
def one_process(tmp_path_factory):
    import _gpu_movie_events_worker as ew
    events, path = ew.run_movie(str(tmp_path_factory.mktemp("events") / "one"), 0, 1, None)
    return events, path


def test_movie_events_equal_the_reference_on_the_archive(one_process):
    """The movie's sites are edited (_gpu_movie_events_worker.EDITS): site 9 removed from frame 2 on, a site added at (64, 80) from
    frame 3 on, site 4's is_hc switched on from frame 3 on."""
    import _gpu_movie_seg_worker as w
    from tissue_image_processing_amd import tissue_info as ti
    events, path = one_process
    tissue = _loaded(path)
    in_archive = tissue.events
    tissue.events = ti.make_df(0, ti.EVENTS_INFO_SPEC)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in tissue.find_events_iterator(1, w.T, differentiation_type_name="HC"):
            pass
    want = tissue.events
    print("the reference finds", [(str(r.type), int(r.start_frame), int(r.end_frame), int(r.cell_id), int(r.daughter_id)) for r in want.itertuples()])
    assert len(want) >= 3 and len(set(str(v) for v in want["type"])) >= 2
    _same_table(in_archive, want)
    _same_table(events, want)
    assert [str(v) for v in in_archive["source"]] == ["automatic"] * len(want)


def test_two_ranks_find_the_same_events(tmp_path, one_process):
    out = str(tmp_path / "world2")
    run_ranks("_gpu_movie_events_worker.py", 2, (out,), timeout=600, local_rank="0")
    _same_table(_loaded(out + ".seg").events, _loaded(one_process[1]).events)
