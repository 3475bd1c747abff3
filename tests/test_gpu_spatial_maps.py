"""GPU: the spatial feature maps and window statistics (csrc/tip_spatial.hip) through the Tissue methods against the goldens of the
reference's own calculate_spatial_data / calculate_data_around_a_given_cell / get_frame_data (tools/make_goldens_spatial.py), and
through tip_window_stats_f64 against the numpy restatement (tests/spatial_restate.py) on seeded random tables.

Bounds: counts, the integer area sum, density and type_fraction (one division of two integers) are exact.  A sum of n_sel same-sign
doubles taken in another order differs by at most n_sel 2^-52 relative (worst-case reordering error); that is the bound of sum_sel and of
every mean, per centre / grid point with its own n_sel.  The kernel tile is 128 centres and the LDS chunk 512 table rows."""
import builtins
import ctypes
import threading

import numpy as np
import pytest

import spatial_restate as sr

CASES = sr.golden_cases(sr.load_golden())
IDS = ["%02d-%s-r%g-s%d-%s-%s-%d" % c[:7] for c in CASES]

pytestmark = pytest.mark.gpu

TILE, CHUNK = 128, 512


@pytest.fixture(scope="module")
def g(golden):
    return golden("spatial_maps")


def assert_sum_bound(got, ref, n_sel, what):
    bound = np.asarray(n_sel) * 2.0 ** -52 * np.abs(ref)
    err = np.abs(np.asarray(got) - ref)
    ok = bound > 0
    print("%s: worst error / bound = %.3g" % (what, np.max(err[ok] / bound[ok]) if ok.any() else 0.0))
    assert (err <= bound).all(), what


# ---- through the Tissue methods, against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_map_equals_reference(g, case):
    k, tag, radius, step, feature, cells_type, positive, status, msg = case
    t = sr.build_tissue(g, tag)
    if status == 2:                                     # the reference raises (a name that is no type): the same exception type
        with pytest.raises(getattr(builtins, msg)):
            t.calculate_spatial_data(1, radius, step, feature, cells_type=cells_type, positive_for_type=positive)
        return
    got, got_msg = t.calculate_spatial_data(1, radius, step, feature, cells_type=cells_type, positive_for_type=positive)
    assert got_msg == msg
    if status == 1:
        assert got is None and msg == "No matching cells"
        return
    ref = g["case%02d_map" % k]
    assert got.shape == ref.shape and got.dtype == np.float64
    if feature.split(" ")[-1] in ("density", "type_fraction"):
        np.testing.assert_array_equal(got, ref)         # bit for bit
    else:
        n_sel = sr.restate_case(g, case)[2]
        assert_sum_bound(got, ref, sr.fill(ref.shape, step, n_sel), "case %d" % k)
        assert (got[ref == 0] == 0).all()               # seams and unfilled borders


@pytest.mark.parametrize("tag", ["A", "B"])
def test_cell_windows_equal_reference(g, tag):
    t = sr.build_tissue(g, tag)
    valid = t.get_valid_non_edge_cells(1, t.get_cells_info(1))
    kw = dict(special_features=t.SPECIAL_FEATURES, global_features=t.GLOBAL_FEATURES, spatial_features=t.SPATIAL_FEATURES)
    status = g["gfd_%s_spatial_status" % tag].reshape(len(t.SPATIAL_FEATURES), 2)
    for i, feature in enumerate(t.SPATIAL_FEATURES):
        for hist in (False, True):
            if status[i, int(hist)] == 2:
                with pytest.raises(KeyError):
                    t.get_frame_data(1, feature, valid, for_histogram=hist, window_radius=25.5, **kw)
                continue
            assert status[i, int(hist)] == 0
            data, msg = t.get_frame_data(1, feature, valid, for_histogram=hist, window_radius=25.5, **kw)
            assert msg == "" and data.dtype == np.float64
            np.testing.assert_array_equal(data, g["gfd_%s_%s_%d" % (tag, feature, hist)], err_msg=feature)
    assert status[0, 0] == 0 and status[2, 0] == 0      # the HC features are maps of values, not raises
    empty, msg = t.get_frame_data(1, "HC density", valid.iloc[:0], window_radius=25.5, **kw)
    assert empty.shape == (0,) and msg == ""
    info = t.get_cells_info(1)
    for j, row in enumerate(g["around_rows_" + tag]):
        cell = info.loc[row]
        for feature, cells_type, positive in (("HC density", "all", True), ("type_fraction", "HC", False), ("area", "HC", True),
                                              ("roundness", "all", True)):
            data, msg = t.calculate_data_around_a_given_cell(1, cell, valid, 25.5, feature, cells_type, positive_for_type=positive)
            assert msg == ""
            np.testing.assert_array_equal(np.asarray(data, dtype=np.float64),
                                          g["around_%s_%d_%s_%s_%d" % (tag, j, feature, cells_type, positive)], err_msg=feature)
    assert t.calculate_data_around_a_given_point(1, 0.25, 0.75, valid, 0.5, "area", "all") == (None, "No matching cells")
    assert t.calculate_data_around_a_given_point(1, 0.25, 0.75, valid, 0.5, "HC density", "all") == (0, "")
    # rows chosen by the caller: density over their own area, and the error return when the selector leaves none
    hc = info.loc[g["hc_rows_" + tag]]
    value, msg = t.calculate_spatial_data_for_given_cells(1, hc, "density", "HC")
    assert msg == "" and value == hc.shape[0] / int(hc.area.sum())
    assert t.calculate_spatial_data_for_given_cells(1, hc, "HC type_fraction", "all") == (1.0, "")
    assert t.calculate_spatial_data_for_given_cells(1, hc, "area", "HC", positive_for_type=False) == (None, "No matching cells")
    areas, msg = t.calculate_spatial_data_for_given_cells(1, hc, "area", "all")
    np.testing.assert_array_equal(areas, hc.area.to_numpy())


# ---- through tip_window_stats_f64, against the restatement ----------------------------------------------------------------------------
def random_table(rng, n, integer):
    if integer:
        cy, cx = rng.integers(0, 40, n).astype(np.float64), rng.integers(0, 40, n).astype(np.float64)
    else:
        cy, cx = rng.uniform(0, 40, n), rng.uniform(0, 40, n)
    area = rng.integers(1, 2 ** 50, n)                  # window sums pass 2^53: the area sum is int64, not a double
    typ = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), n)
    feat = rng.uniform(0.5, 2.0, n) * 10.0 ** rng.integers(-3, 4, n)
    return cy, cx, area, typ, feat


# (centres, rows): one partial tile / chunk, exact multiples, one past, several chunks with a partial last one, and the empty table
SIZES = [(1, 0), (1, 1), (TILE, CHUNK), (TILE + 1, CHUNK + 1), (2 * TILE + 3, 2 * CHUNK + 276), (37, 3 * CHUNK), (300, 77)]


@pytest.mark.parametrize("integer", [False, True], ids=["float", "integer"])
@pytest.mark.parametrize("m,n", SIZES)
def test_window_stats_equal_restatement(m, n, integer):
    from tissue_image_processing_amd import _segmentation as seg
    rng = np.random.default_rng(1000 * m + n + int(integer))
    cy, cx, area, typ, feat = random_table(rng, n, integer)
    if integer:                                          # whole coordinates and r2 = 25: 3-4-5 rows sit exactly on the circle
        qy, qx, r2 = rng.integers(0, 40, m).astype(np.float64), rng.integers(0, 40, m).astype(np.float64), 25.0
        if n:
            on_circle = ((cx[None, :] - qx[:, None]) ** 2 + (cy[None, :] - qy[:, None]) ** 2 == r2).sum()
            assert on_circle > 0 or m * n < 1000, "the integer case is meant to hold rows on the circle"
    else:
        qy, qx, r2 = rng.uniform(0, 40, m), rng.uniform(0, 40, m), sr.fmt6(9.7 ** 2)
    for sel_bit, sel_positive in ((-1, True), (0, True), (1, False)):
        ref = sr.window_stats(qy, qx, r2, cy, cx, area, typ, feat, sel_bit, sel_positive)
        got = seg.window_stats(qy, qx, r2, cy, cx, area, typ, feat, sel_bit, sel_positive)
        for name, a, b in zip(("n_in", "area_in", "n_sel"), got, ref):
            assert a.dtype == np.int64
            np.testing.assert_array_equal(a, b, err_msg="%s sel %d %d" % (name, sel_bit, sel_positive))
        assert_sum_bound(got[3], ref[3], ref[2], "sum_sel (%d, %d) sel %d" % (m, n, sel_bit))
    if n >= CHUNK:
        assert ref[0].max() > 0 and (ref[0] != ref[2]).any()


def test_window_stats_edge_cases():
    from tissue_image_processing_amd import _segmentation as seg
    # a row exactly on the circle is outside, one ulp inside is inside; r2 = 25 is met with equality by (3, 4)
    cy, cx = np.array([3.0, 3.0, 0.0]), np.array([4.0, np.nextafter(4.0, 0.0), 0.0])
    area, typ, feat = np.array([10, 20, 40]), np.array([1, 1, 255], np.uint8), np.array([1.5, 2.5, 4.0])
    n_in, area_in, n_sel, sum_sel = seg.window_stats([0.0], [0.0], 25.0, cy, cx, area, typ, feat, 0, True)
    assert (n_in[0], area_in[0], n_sel[0], sum_sel[0]) == (2, 60, 1, 2.5)
    n_in, area_in, n_sel, sum_sel = seg.window_stats([0.0], [0.0], 25.0, cy, cx, area, typ, feat, 0, False)
    assert (n_in[0], area_in[0], n_sel[0], sum_sel[0]) == (2, 60, 1, 4.0)           # the invalid byte counts as not positive
    # a pair for which contraction would flip the answer: with separately rounded squares the sum EQUALS r2 (outside), while
    # fma(dx, dx, dy * dy) -- the exact dx^2 added to the rounded dy^2, rounded once -- falls below it (inside)
    from fractions import Fraction
    rng = np.random.default_rng(77)
    for _ in range(10000):
        dx, dy = float(rng.uniform(1, 2)), float(rng.uniform(1, 2))
        r2 = dx * dx + dy * dy
        if float(Fraction(dx) * Fraction(dx) + Fraction(dy * dy)) < r2:
            break
    else:
        raise AssertionError("no contraction-sensitive pair found")
    n_in = seg.window_stats([0.0], [0.0], r2, [dy], [dx], [1], [0])[0]
    assert n_in[0] == 0
    assert seg.window_stats([0.0], [0.0], np.nextafter(r2, np.inf), [dy], [dx], [1], [0])[0][0] == 1
    # an infinite radius takes every row; no centres and no rows are valid calls
    assert seg.window_stats([1e9], [-1e9], np.inf, cy, cx, area, typ)[0][0] == 3
    assert all(a.shape == (0,) for a in seg.window_stats([], [], 1.0, cy, cx, area, typ))
    assert [int(a[0]) for a in seg.window_stats([0.0], [0.0], 1.0, [], [], [], [])[:3]] == [0, 0, 0]
    with pytest.raises(ValueError):
        seg.window_stats([0.0], [0.0], 1.0, cy, cx, area, typ, sel_bit=8)
    with pytest.raises(ValueError):
        seg.window_stats([0.0], [0.0], float("nan"), cy, cx, area, typ)
    with pytest.raises(ValueError):
        seg.spatial_map((8, 8), 0, 1.0, cy, cx, area, typ)


def test_fill_rule_on_the_device():
    """odd step seams, step 1, a step wider than the frame, the clipped last block: the restatement's fill, which is upstream's slices"""
    from tissue_image_processing_amd import _segmentation as seg
    rng = np.random.default_rng(5)
    cy, cx, area, typ, feat = random_table(rng, 60, False)
    for shape, step in (((13, 12), 5), ((6, 7), 1), ((5, 300), 3), ((41, 37), 7), ((3, 3), 8), ((40, 40), 16), ((9, 9), 2)):
        got, n_sel = seg.spatial_map(shape, step, 81.0, cy, cx, area, typ, feat, 0, True, "density")
        ref, _, ref_n = sr.spatial_map(shape, step, 9.0, cy, cx, area, typ, feat, 0, True, "density")
        np.testing.assert_array_equal(got, ref, err_msg=str((shape, step)))
        np.testing.assert_array_equal(n_sel, ref_n)
    got, n_sel = seg.spatial_map((13, 12), 5, 1e4, cy, cx, area, typ, feat, -1, True, "mean")
    ref = sr.spatial_map((13, 12), 5, 100.0, cy, cx, area, typ, feat, -1, True, "mean")[0]
    assert_sum_bound(got, ref, np.full(ref.shape, 60), "mean fill")
    assert not got[4].any() and not got[:, 9:].any() and got[12, 8] != 0


def test_dev_and_host_entries_give_the_same_map(g):
    from tissue_image_processing_amd import _lib, _segmentation as seg
    cols, labels = sr.golden_columns(g, "B"), sr.golden_labels(g, "B")
    keep = sr.valid_non_edge(labels, cols["valid"], cols["empty_cell"])
    cy, cx = np.ascontiguousarray(cols["cy"][keep]), np.ascontiguousarray(cols["cx"][keep])
    area, typ = cols["area"][keep].astype(np.int64), cols["type"][keep].astype(np.uint8)
    feat = sr.roundness(cols["area"][keep], cols["perimeter"][keep])
    n = int(cy.size)
    bufs = [_lib.DeviceBuffer(max(a.nbytes, 16)).upload(a) for a in (cy, cx, area, typ, feat)]
    for step, mode, sel in ((7, "density", 0), (5, "mean", -1), (16, "type_fraction", 1)):
        host_map, host_n = seg.spatial_map(labels.shape, step, 650.25, cy, cx, area, typ, feat, sel, True, mode)
        d_map = _lib.DeviceBuffer(host_map.nbytes)
        d_n = _lib.DeviceBuffer(max(host_n.nbytes, 16))
        seg.spatial_map_dev(labels.shape, step, 650.25, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, n, sel, True,
                            mode, d_map.ptr, d_n.ptr)
        _lib.check(_lib.lib().tip_sync())
        np.testing.assert_array_equal(d_map.download(host_map.shape, np.float64), host_map)
        np.testing.assert_array_equal(d_n.download(host_n.shape, np.int64), host_n)
    # ... a NULL n_sel_grid is skipped: the host entry gives the same map without it
    host_map, _ = seg.spatial_map(labels.shape, 7, 650.25, cy, cx, area, typ, feat, 0, True, "density")
    alone = np.full(host_map.shape, -7.0)
    _lib.check(_lib.lib().tip_spatial_map_f64(
        labels.shape[0], labels.shape[1], 7, ctypes.c_double(650.25), _lib.ptr(cy), _lib.ptr(cx), _lib.ptr(area), _lib.ptr(typ), _lib.ptr(feat),
        ctypes.c_int64(n), 0, 1, seg.SPATIAL_MODES["density"], _lib.ptr(alone), None))
    np.testing.assert_array_equal(alone, host_map)
    # ... and the statistics' device entry
    qy, qx = np.ascontiguousarray(cy[:50]), np.ascontiguousarray(cx[:50])
    host = seg.window_stats(qy, qx, 650.25, cy, cx, area, typ, feat, 0, False)
    dq = [_lib.DeviceBuffer(qy.nbytes).upload(qy), _lib.DeviceBuffer(qx.nbytes).upload(qx)]
    outs = [_lib.DeviceBuffer(50 * 8) for _ in range(4)]
    seg.window_stats_dev(dq[0].ptr, dq[1].ptr, 50, 650.25, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, n, 0, False,
                         *[o.ptr for o in outs])
    _lib.check(_lib.lib().tip_sync())
    for o, h in zip(outs, host):
        np.testing.assert_array_equal(o.download(h.shape, h.dtype), h)


def test_two_threads_give_the_serial_results():
    """the library is re-entrant per thread: each thread has its own stream and workspaces"""
    from tissue_image_processing_amd import _segmentation as seg
    jobs = []
    for seed in (11, 12):
        rng = np.random.default_rng(seed)
        table = random_table(rng, 2 * CHUNK + 100, False)
        jobs.append((rng.uniform(0, 40, 3 * TILE + 5), rng.uniform(0, 40, 3 * TILE + 5), 50.0 + seed) + table + (seed % 2, True))
    serial = [seg.window_stats(*job) for job in jobs]
    serial_maps = [seg.spatial_map((90, 70), 3, job[2], *job[3:8], job[8], job[9], "mean")[0] for job in jobs]
    results, errors = [None, None], []

    def work(i):
        try:
            rounds = []
            for _ in range(5):
                rounds.append((seg.window_stats(*jobs[i]), seg.spatial_map((90, 70), 3, jobs[i][2], *jobs[i][3:8], jobs[i][8], jobs[i][9],
                                                                           "mean")[0]))
            results[i] = rounds
        except Exception as e:       # noqa: BLE001  (reported by the main thread)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for i in range(2):
        for stats, out in results[i]:
            for a, b in zip(stats, serial[i]):
                np.testing.assert_array_equal(a, b)
            np.testing.assert_array_equal(out, serial_maps[i])


# ---- the "%f" trip of radius**2 and of the centres, through the device-backed Tissue methods -------------------------------------------
def small_tissue(cy, cx, area, typ, shape=(8, 8)):
    """a frame without labels (no cell touches the border) whose table holds the given valid cells; type name "HC" = bit 0"""
    import pandas as pd
    from tissue_image_processing_amd import tissue_info as ti
    t = ti.Tissue(1, None, ["zo", "atoh"])
    t.type_names = ["HC"]
    t.set_labels(1, np.zeros(shape, np.int32))
    n = len(cy)
    t.set_cells_info(1, pd.DataFrame({"cy": np.asarray(cy, np.float64), "cx": np.asarray(cx, np.float64), "area": np.asarray(area, np.int64),
                                      "perimeter": np.full(n, 30.0), "type": np.asarray(typ, np.int64), "valid": 1, "empty_cell": 0,
                                      "n_neighbors": 6, "label": np.arange(1, n + 1)}))
    return t


def test_radius_takes_the_percent_f_trip_in_the_map():
    """radius 10.0001: radius**2 = 100.00200001 reaches the comparison as 100.002; a cell at squared distance 100.002000005 from the one
    grid point (4, 4) is inside the exact circle and outside upstream's.  Radius 10.0002 takes it."""
    cx = 4.0 + np.sqrt(100.002000005)
    dist2 = (cx - 4.0) ** 2 + (4.0 - 4.0) ** 2
    assert sr.fmt6(10.0001 ** 2) == 100.002 and 100.002 <= dist2 < 10.0001 ** 2
    t = small_tissue([4.0], [cx], [50], [1])
    out, msg = t.calculate_spatial_data(1, 10.0001, 8, "HC density")
    assert msg == "" and out.shape == (8, 8) and not out.any()
    assert t.calculate_spatial_data(1, 10.0001, 8, "area") == (None, "No matching cells")
    out, msg = t.calculate_spatial_data(1, 10.0002, 8, "HC density")
    assert msg == "" and (out == 1 / 50).all()
    valid = t.get_cells_info(1)
    assert t.calculate_data_around_a_given_point(1, 4, 4, valid, 10.0001, "density", "all") == (0, "")
    assert t.calculate_data_around_a_given_point(1, 4, 4, valid, 10.0002, "density", "all") == (1 / 50, "")


def test_centres_take_the_percent_f_trip_in_the_windows():
    """a centre at x = 4.0000004 reads 4.000000 and one at 4.0000006 reads 4.000001: with radius 10.0000003 (squared: 100.000006) the
    cell at x = 14.0000005 is 10.0000005 from the first (outside) and 9.9999995 from the second (inside); unrounded, the first centre
    would be 10.0000001 away (inside)."""
    radius = 10.0000003
    t = small_tissue([4.0, 4.0, 4.0], [4.0000004, 14.0000005, 4.0000006], [30, 50, 70], [1, 1, 1], shape=(8, 24))
    info = t.get_cells_info(1)
    far = info.iloc[[1]]                                   # the windows look at the far cell only
    assert t.calculate_data_around_a_given_point(1, 4.0000004, 4.0, far, radius, "HC density", "all") == (0, "")
    assert t.calculate_data_around_a_given_point(1, 4.0000006, 4.0, far, radius, "HC density", "all") == (1 / 50, "")
    assert t.calculate_data_around_a_given_cell(1, info.iloc[0], far, radius, "type_fraction", "HC") == (0, "")
    assert t.calculate_data_around_a_given_cell(1, info.iloc[2], far, radius, "type_fraction", "HC") == (1.0, "")
    # get_frame_data's per-cell windows over the whole table: the restatement with rounded centres, which differs from the unrounded one
    data, msg = t.get_frame_data(1, "HC density", info, spatial_features=t.SPATIAL_FEATURES, window_radius=radius)
    cols = [info[k].to_numpy() for k in ("cy", "cx", "area", "type")]
    rounded = sr.window_stats([sr.fmt6(v) for v in cols[0]], [sr.fmt6(v) for v in cols[1]], sr.fmt6(radius ** 2), *cols, None, 0, True)
    exact = sr.window_stats(cols[0], cols[1], radius ** 2, *cols, None, 0, True)
    assert rounded[0].tolist() != exact[0].tolist()
    np.testing.assert_array_equal(data, sr.point_values("density", *rounded))
    assert msg == "" and data[0] == 2 / 100 and data[2] == 3 / 150
