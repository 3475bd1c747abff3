"""GPU: the order kernels (csrc/tip_order.hip), the mixin methods on top of them, FramePipeline.order_features and the movie
driver's order columns.  Neighbour sets: equality with the reference's goldens (tests/golden/order_features.npz), with the numpy
restatement (tests/order_restate.py) and with scipy's Voronoi, no tolerance.  psi: |difference| <= 1e-13 (order_cases.PSI_TOL:
the two libms' atan2 / sincos differ by a few ulp, so psi is not bit-equal to numpy's).  Correlations: order_cases.corr_tol."""
import builtins
import ctypes

import numpy as np
import pandas as pd
import pytest

import order_cases as oc
import order_restate as orr
from gloo_launch import run_ranks

pytestmark = pytest.mark.gpu


def _seg():
    from tissue_image_processing_amd import _segmentation as seg
    return seg


def device_rows(py, px):
    """delaunay_neighbors as a list of rows; the sizes-only call and the CSR agree"""
    sizes, moff, mem = _seg().delaunay_neighbors(py, px)
    np.testing.assert_array_equal(sizes, _seg().delaunay_neighbors(py, px, members=False))
    np.testing.assert_array_equal(np.diff(moff), sizes)
    return [mem[moff[q]:moff[q + 1]] for q in range(sizes.size)]


def assert_rows_equal(got, want):
    assert len(got) == len(want)
    for q, (a, b) in enumerate(zip(got, want)):
        assert np.asarray(a).tolist() == np.asarray(b).tolist(), "row %d: %r != %r" % (q, a, b)      # (ascending on both sides)


@pytest.mark.parametrize("tag", oc.FRAMES)
def test_neighbours_equal_the_goldens_and_the_restatement(tag):
    f = oc.frame(tag)
    py, px = f["cy"][f["cells"]], f["cx"][f["cells"]]
    rows = device_rows(py, px)
    assert oc.label_sets(f, rows) == oc.sets_of(*f["vor"])
    assert_rows_equal(rows, orr.delaunay_neighbors(py, px))
    if tag == "H":
        assert max(len(r) for r in rows) > 64


def test_collinear_points_give_the_chain():
    px = np.asarray([3.0, 0.0, 7.0, 1.0, 12.5, -4.0])
    for py in (np.zeros(6), 0.5 * px + 1.0):
        rows = device_rows(py, px)
        assert_rows_equal(rows, orr.delaunay_neighbors(py, px))
        assert [r.tolist() for r in rows] == [[2, 3], [3, 5], [0, 4], [0, 1], [2], [1]]


def _order_grid(py, px):
    """The grid kernel's cell side and shape for these points (its own formula, on the CPU): (first h, doublings, gx, gy)."""
    n = len(px)
    W, H, target = float(np.ptp(px)), float(np.ptp(py)), float(max(n // 2, 1))
    h0 = np.sqrt(W / target * H) if W > 0 and H > 0 else (max(W, H) / target if W > 0 or H > 0 else 1.0)
    h, doublings = h0, 0
    while (np.floor(W / h) + 1.0) * (np.floor(H / h) + 1.0) > n + 4:
        h, doublings = 2.0 * h, doublings + 1
    return h0, doublings, int(np.floor(W / h)) + 1, int(np.floor(H / h)) + 1


def test_thin_box_doubles_the_grid_cell():
    """1000 x 1 with 40 points: square cells of two points each would outnumber the points, so h doubles (twice, to a 35 x 1
    grid); every other case's box is near-square or exactly degenerate."""
    rng = np.random.default_rng(11)
    px = rng.uniform(0, 1000, 40)
    py = rng.uniform(0, 1, 40)
    h0, doublings, gx, gy = _order_grid(py, px)
    assert abs(h0 - 6.83) < 0.01 and (doublings, gx, gy) == (2, 35, 1)
    want = orr.delaunay_neighbors(py, px)
    assert max(len(r) for r in want) == 11
    rows = device_rows(py, px)
    assert_rows_equal(rows, want)
    assert orr.edges_of(rows) == orr.voronoi_edges(py, px)


def test_points_on_an_axis_parallel_line():
    """W = 0 with distinct py, and its transpose (H = 0): one row or one column of cells of side max(W, H) / (n // 2)."""
    line, const = np.asarray([0.0, 5.0, 1.0, 9.0, 2.5, 7.0, 4.0]), np.full(7, 3.0)
    for py, px in ((line, const), (const, line)):
        rows = device_rows(py, px)
        assert_rows_equal(rows, orr.delaunay_neighbors(py, px))
        assert [r.tolist() for r in rows] == [[2], [5, 6], [0, 4], [5], [2, 6], [1, 3], [1, 4]]


def test_neighbours_equal_scipy_on_2000_points():
    rng = np.random.default_rng(72)
    py, px = rng.uniform(0, 512, 2000), rng.uniform(0, 512, 2000)
    assert orr.edges_of(device_rows(py, px)) == orr.voronoi_edges(py, px)


def test_small_inputs_and_argument_errors():
    seg = _seg()
    for n in (0, 1):
        sizes, moff, mem = seg.delaunay_neighbors(np.arange(n, dtype=float), np.zeros(n))
        assert sizes.tolist() == [0] * n and mem.size == 0
    assert [r.tolist() for r in device_rows([0.0, 0.0, 1.0], [0.0, 1.0, 0.0])] == [[1, 2], [0, 2], [0, 1]]
    py, px = np.asarray([0.0, 0.0, 1.0, 1.1]), np.asarray([0.0, 1.0, 0.0, 1.3])
    assert orr.edges_of(device_rows(py, px)) == orr.voronoi_edges(py, px)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError):
            seg.delaunay_neighbors([0.0, 1.0, bad], [0.0, 0.0, 1.0])
    with pytest.raises(ValueError):                                            # two points with the same coordinates
        seg.delaunay_neighbors([0.0, 1.0, 0.0, 5.0], [2.0, 0.0, 2.0, 5.0])
    with pytest.raises(ValueError):
        seg.psin([0.0, 1.0], [0.0, 1.0], [0, 1, 1], [3])                       # a label outside the table
    with pytest.raises(ValueError):
        seg.psin([0.0, 1.0], [0.0, 1.0], [0, 1, 1], [2], order=0)
    with pytest.raises(ValueError):
        seg.graph_neighbor_state([0, 1, 2], [2, 1], [1, 1], [0.0, 1.0], [2])   # a query row outside the table
    assert seg.psin([0.0, 1.0], [0.0, 1.0], [0, 0, 0], []).tolist() == [0.0, 0.0]      # empty rows: 0


@pytest.mark.parametrize("tag", oc.FRAMES)
def test_psi_equals_the_goldens_and_the_restatement(tag):
    f = oc.frame(tag)
    worst = 0.0
    for (order, kind), want in f["psi"].items():
        got = _seg().psin(f["cy"], f["cx"], *f[kind], f["cells"], order)
        restated = orr.psin(f["cy"], f["cx"], *f[kind], f["cells"], order)
        worst = max(worst, np.max(np.abs(got - want), initial=0.0), np.max(np.abs(got - restated), initial=0.0))
        np.testing.assert_allclose(got, want, rtol=0, atol=oc.PSI_TOL)
        np.testing.assert_allclose(got, restated, rtol=0, atol=oc.PSI_TOL)
    print(tag, "max |psi - golden or restatement| = %.3g" % worst)


@pytest.mark.parametrize("tag", oc.FRAMES)
def test_neighbour_state_equals_the_restatement_bit_for_bit(tag):
    f = oc.frame(tag)
    for state_by, type_name in (("type", "HC"), ("intensity", "HC")):
        member, full = oc.state_columns(f, oc.state_of(f, state_by, type_name))
        for query in (f["cells"], None):
            nb_sum, nb_cnt = _seg().graph_neighbor_state(f["offsets"], f["adj"], member, full, query)
            want_sum, want_cnt = orr.graph_neighbor_state(f["offsets"], f["adj"], member, full, query)
            np.testing.assert_array_equal(nb_cnt, want_cnt)
            assert nb_sum.tobytes() == want_sum.tobytes()


@pytest.mark.parametrize("tag", ["C", "H"])
def test_dev_forms_equal_the_host_forms(tag):
    """H: 73 points around a hub of 71 Delaunay neighbours, so the chained entry's row sort (int32 offsets, labels = positions
    + 1) meets a row of two 64-lane chunks"""
    from tissue_image_processing_amd import _lib
    seg = _seg()
    f = oc.frame(tag)
    if tag == "H":
        assert f["cells"].size == 73 and int(np.diff(f["vor"][0]).max()) == 71      # (from the golden, on the CPU)
    py, px = np.ascontiguousarray(f["cy"][f["cells"]]), np.ascontiguousarray(f["cx"][f["cells"]])
    n = py.size
    sizes, moff, mem = seg.delaunay_neighbors(py, px)
    d_y, d_x = _lib.DeviceBuffer(8 * n).upload(py), _lib.DeviceBuffer(8 * n).upload(px)
    d_sizes, d_moff, d_mem = _lib.DeviceBuffer(8 * n), _lib.DeviceBuffer(8 * (n + 1)).upload(moff), _lib.DeviceBuffer(4 * mem.size)
    seg.delaunay_neighbors_dev(d_y.ptr, d_x.ptr, n, d_sizes.ptr)
    seg.delaunay_neighbors_dev(d_y.ptr, d_x.ptr, n, None, d_moff.ptr, d_mem.ptr, mem.size)
    np.testing.assert_array_equal(d_sizes.download((n,), np.int64), sizes)
    np.testing.assert_array_equal(d_mem.download((mem.size,), np.int32), mem)
    labels = (mem + 1).astype(np.int32)
    want = seg.psin(py, px, moff, labels)
    d_lab, d_psi = _lib.DeviceBuffer(4 * mem.size).upload(labels), _lib.DeviceBuffer(8 * n)
    seg.psin_dev(d_y.ptr, d_x.ptr, n, None, n, d_moff.ptr, d_lab.ptr, mem.size, 6, d_psi.ptr)
    assert d_psi.download((n,), np.float64).tobytes() == want.tobytes()
    d_deg = _lib.DeviceBuffer(8 * n)
    seg.order_features_dev(d_y.ptr, d_x.ptr, n, 6, d_psi.ptr, d_deg.ptr)      # the chained entry
    assert d_psi.download((n,), np.float64).tobytes() == want.tobytes()
    np.testing.assert_array_equal(d_deg.download((n,), np.int64), sizes)
    state = oc.state_of(f, "intensity", "HC")
    member, full = oc.state_columns(f, state)
    want_sum, want_cnt = seg.graph_neighbor_state(f["offsets"], f["adj"], member, full)
    N = f["n"]
    d_off, d_adj = _lib.DeviceBuffer(4 * (N + 1)).upload(f["offsets"]), _lib.DeviceBuffer(4 * f["adj"].size).upload(f["adj"])
    d_member, d_state = _lib.DeviceBuffer(N).upload(member), _lib.DeviceBuffer(8 * N).upload(full)
    d_sum, d_cnt = _lib.DeviceBuffer(8 * N), _lib.DeviceBuffer(8 * N)
    seg.graph_neighbor_state_dev(d_off.ptr, d_adj.ptr, N, f["adj"].size, d_member.ptr, d_state.ptr, None, N, d_sum.ptr, d_cnt.ptr)
    assert d_sum.download((N,), np.float64).tobytes() == want_sum.tobytes()
    np.testing.assert_array_equal(d_cnt.download((N,), np.int64), want_cnt)


def test_neighbour_state_sums_in_row_order_and_takes_a_row_that_does_not_ascend():
    """(-1e16 + 1e16) + 1.0 = 1.0 in the row's order 4, 2, 3; the ascending order 2, 3, 4 would give (1e16 + 1.0) - 1e16 = 0.0"""
    from tissue_image_processing_amd import _lib
    seg = _seg()
    offsets, adj = np.asarray([0, 3, 3, 3, 3], np.int32), np.asarray([4, 2, 3], np.int32)
    member, state, query = np.ones(4, np.uint8), np.asarray([0.0, 1e16, 1.0, -1e16]), np.asarray([0], np.int32)
    nb_sum, nb_cnt = seg.graph_neighbor_state(offsets, adj, member, state, query)
    assert nb_sum.tolist() == [1.0] and nb_cnt.tolist() == [3]
    bufs = [_lib.DeviceBuffer(a.nbytes).upload(a) for a in (offsets, adj, member, state, query)]
    d_sum, d_cnt = _lib.DeviceBuffer(8), _lib.DeviceBuffer(8)
    seg.graph_neighbor_state_dev(bufs[0].ptr, bufs[1].ptr, 4, 3, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, 1, d_sum.ptr, d_cnt.ptr)
    assert d_sum.download((1,), np.float64).tolist() == [1.0] and d_cnt.download((1,), np.int64).tolist() == [3]
    with pytest.raises(ValueError):                                            # the entries that search a row ask for ascending rows
        seg.graph_counts(offsets, adj, member, 0 * member, 0 * member, query, "valid")


def golden_tissue(tag):
    """the stand-alone Tissue holding the golden table"""
    from tissue_image_processing_amd import tissue_info as ti
    f = oc.frame(tag)
    t = ti.Tissue(1)
    t.type_names = ["HC", "X"]
    table = pd.DataFrame({"cx": f["cx"], "cy": f["cy"], "mean_intensity_HC": f["intensity"]})
    for name, key in (("valid", "valid"), ("type", "type"), ("empty_cell", "empty")):
        table[name] = f[key].astype(np.int64)
    table["label"] = np.arange(1, f["n"] + 1)
    table["neighbors"] = oc.sets_of(f["offsets"], f["adj"])
    t.set_cells_info(1, table)
    return t, table


@pytest.mark.parametrize("tag", oc.FRAMES)
def test_mixin_methods_equal_the_goldens(tag):
    f = oc.frame(tag)
    t, table = golden_tissue(tag)
    cells = table.iloc[f["cells"]]
    sets = t.find_nearest_neighbors_using_voroni_tesselation(cells)
    assert sets == oc.sets_of(*f["vor"])
    assert type(t).find_nearest_neighbors_using_voroni_tesselation(cells.iloc[:3]) == [set(), set(), set()]
    for order in (6, 4):
        for hist in (False, True):                                             # upstream's call shape
            got = t.calc_psin(1, cells, t.find_nearest_neighbors_using_voroni_tesselation(cells), n=order, for_histogram=hist)
            np.testing.assert_allclose(got, f["psi"][(order, "vor")], rtol=0, atol=oc.PSI_TOL)
        got = t.calc_psin(1, cells, t.find_second_order_neighbors(1, cells), n=order)
        np.testing.assert_allclose(got, f["psi"][(order, "son")], rtol=0, atol=oc.PSI_TOL)
    for a, b, state_by, type_name, method in oc.corr_cases():
        got = t.calculate_neighbors_correlation_function(1, cells, set_state_by=state_by, method=method, type_name=type_name)
        state = oc.state_of(f, state_by, type_name)
        contacts = int(orr.graph_neighbor_state(f["offsets"], f["adj"], *oc.state_columns(f, state), f["cells"])[1].sum())
        tol = oc.corr_tol(state, state_by, contacts)
        print(tag, state_by, type_name, method, "|got - golden| = %.3g, bound %.3g" % (abs(got - f["corr"][a, b]), tol))
        assert abs(got - f["corr"][a, b]) <= tol
    for state_by, method, type_name, exc in oc.raising_cases(tag):
        with pytest.raises(getattr(builtins, exc)):
            t.calculate_neighbors_correlation_function(1, cells, set_state_by=state_by, method=method, type_name=type_name)
    flat = cells.assign(type=0)                                                # zero variance: NaN, as upstream
    assert np.isnan(t.calculate_neighbors_correlation_function(1, flat, type_name="HC"))
    t.set_cells_info(1, None)
    assert t.calc_psin(1, cells, sets) is None
    t.set_cells_info(1, table)
    for feature in ("psi6", "HC neighbors correlation"):                       # the routing stays as it was
        with pytest.raises(NotImplementedError):
            t.get_frame_data(1, feature, cells, special_features=[feature])


def expected_order_columns(valid, cy, cx):
    """psi6 and the Delaunay degree of the valid rows from scipy's Voronoi and the restated psi"""
    n = valid.size
    psi, deg = np.zeros(n), np.zeros(n, np.int64)
    rows = np.flatnonzero(valid == 1)
    if rows.size < 4:
        return psi, deg
    edges = orr.voronoi_edges(cy[rows], cx[rows])
    nb = [[] for _ in rows]
    for a, b in edges:
        nb[a].append(b)
        nb[b].append(a)
    off, mem = orr.csr([sorted(r) for r in nb], add=1)
    psi[rows] = orr.psin(cy[rows], cx[rows], off, mem)
    deg[rows] = np.diff(off)
    return psi, deg


def test_pipeline_order_features_equal_scipy_and_the_restated_psi():
    from tissue_image_processing_amd import synthetic
    from tissue_image_processing_amd.pipeline import FramePipeline
    Z, Y, X = 6, 128, 128
    pipe = FramePipeline(2, Z, Y, X)
    pipe.project(pipe.upload_stack(synthetic.make_stack(Z, Y, X, seed=31)))
    pipe.segment(0)
    tab = pipe.cell_tables()
    n = tab["area"].size
    area = tab["area"].astype(np.float64)
    cy, cx = tab["sumy"] / area, tab["sumx"] / area
    valid = ((area > 0.1 * area.mean()) & (area < 10 * area.mean())).astype(np.uint8)
    valid[::7] = 0
    assert valid.sum() > 20
    got = pipe.order_features(n, valid, cy, cx)
    psi, deg = expected_order_columns(valid, cy, cx)
    assert got["psi6"].dtype == np.float64 and got["voronoi_neighbors"].dtype == np.int64
    np.testing.assert_array_equal(got["voronoi_neighbors"], deg)
    np.testing.assert_allclose(got["psi6"], psi, rtol=0, atol=oc.PSI_TOL)
    assert (got["psi6"][valid == 0] == 0).all() and got["psi6"].max() > 0.1
    few = np.zeros(n, np.uint8)
    few[:3] = 1
    none = pipe.order_features(n, few, cy, cx)
    assert not none["psi6"].any() and not none["voronoi_neighbors"].any()


def test_movie_rows_carry_the_order_columns(tmp_path):
    out = str(tmp_path / "w1.npz")
    run_ranks("_gpu_movie_order_worker.py", 1, (out,), timeout=600, local_rank="0")
    a = np.load(out)
    assert list(a["columns"]) == ["psi6", "voronoi_neighbors"]
    for t in range(int(a["n"])):
        area = a["area_%d" % t]
        valid = ((area > 0.1 * area.mean()) & (area < 10 * area.mean())).astype(np.uint8)
        psi, deg = expected_order_columns(valid, a["cy_%d" % t], a["cx_%d" % t])
        assert a["psi6_%d" % t].dtype == np.float64 and a["voronoi_neighbors_%d" % t].dtype == np.int64
        np.testing.assert_array_equal(a["voronoi_neighbors_%d" % t], deg, err_msg="frame %d" % t)
        np.testing.assert_allclose(a["psi6_%d" % t], psi, rtol=0, atol=oc.PSI_TOL, err_msg="frame %d" % t)
        assert deg.max() >= 5
