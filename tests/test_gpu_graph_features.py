"""GPU: the neighbour-graph kernels (csrc/tip_graph.hip), the mixin methods on top of them, FramePipeline.neighbor_features and the
movie driver's neighbour columns.  Every output is an integer or a set of integers: equality with the reference's goldens
(tests/golden/graph_features.npz), no tolerance."""
import builtins
import ctypes
import types

import numpy as np
import pandas as pd
import pytest

import graph_cases as gc
import graph_restate as gr
from gloo_launch import run_ranks

pytestmark = pytest.mark.gpu


def _seg():
    from tissue_image_processing_amd import _segmentation as seg
    return seg


def _device_ops():
    """the device entries behind graph_restate's signatures"""
    seg = _seg()

    def graph_counts(offsets, adj, valid, empty, type, query, mode, bit=-1, positive=True):
        return seg.graph_counts(offsets, adj, valid, empty, type, query, mode, bit, positive)

    def graph_second(offsets, adj, valid, type, query, bit=-1, positive=True):
        sizes, moff, members = seg.graph_second(offsets, adj, valid, type, query, bit, positive)
        sets = [set(members[moff[q]:moff[q + 1]].tolist()) for q in range(sizes.size)]
        assert [len(s) for s in sets] == sizes.tolist()              # no label twice in a set
        return sets

    def contact_sums(pairs, counts, offsets, adj, valid, type, query, mode, bit=-1, positive=True):
        sums, voff, labels, values = seg.contact_sums(pairs, counts, offsets, adj, valid, type, query, mode, bit, positive, values=True)
        np.testing.assert_array_equal(sums, seg.contact_sums(pairs, counts, offsets, adj, valid, type, query, mode, bit, positive))
        m = sums.size
        return sums, [labels[voff[q]:voff[q + 1]] for q in range(m)], [values[voff[q]:voff[q + 1]] for q in range(m)]

    return types.SimpleNamespace(graph_counts=graph_counts, graph_second=graph_second, contact_sums=contact_sums)


@pytest.mark.parametrize("tag", gc.FRAMES)
def test_kernels_equal_the_goldens(tag):
    ops = _device_ops()
    ran = 0
    for c in gc.cases(tag):
        got = gc.on_kernels(ops, c)
        if got is not None:
            gc.assert_same(got, gc.expected(c))
            ran += 1
    assert ran >= 22


def test_device_contact_triples_equal_the_restatement():
    for tag in gc.FRAMES:
        f = gc.frame(tag)
        pairs, counts = _seg().contact_triples(f["labels"])
        keep = pairs[:, 0] > pairs[:, 1]                                # (a zero-filled minimum gives lo = max + 1: never asked for)
        got = {(int(h), int(l)): int(c) for (h, l), c in zip(pairs[keep], counts[keep])}
        want = {(int(h), int(l)): int(c) for (h, l), c in zip(*f["triples"])}
        assert got == want


def _csr_from_device_pairs(labels, n, working):
    """labels uploaded, pairs left on the device by tip_neighbor_pairs_i32_dev, CSR by tip_neighbor_csr_i32_dev"""
    from tissue_image_processing_amd import _lib
    seg = _seg()
    lab = np.ascontiguousarray(labels, np.int32)
    cap = 16 * (n + 1)
    d_lab = _lib.DeviceBuffer(lab.nbytes).upload(lab)
    d_pairs, d_off, d_adj = _lib.DeviceBuffer(8 * cap), _lib.DeviceBuffer(4 * (n + 1)), _lib.DeviceBuffer(8 * cap)
    d_work = None if working is None else _lib.DeviceBuffer(max(n, 1)).upload(np.ascontiguousarray(working, np.uint8))
    npairs = ctypes.c_int64(0)
    _lib.check(_lib.lib().tip_neighbor_pairs_i32_dev(_lib.dptr(d_lab.ptr), lab.shape[0], lab.shape[1], _lib.dptr(d_pairs.ptr),
                                                     ctypes.c_int64(cap), ctypes.byref(npairs)))
    n_adj = seg.neighbor_csr_dev(d_pairs.ptr, npairs.value, n, None if d_work is None else d_work.ptr, d_off.ptr, d_adj.ptr, 2 * cap,
                                 want_count=True)
    return d_off.download((n + 1,), np.int32), d_adj.download((2 * cap,), np.int32)[:n_adj]


@pytest.mark.parametrize("tag", gc.FRAMES)
def test_csr_from_device_pairs_equals_the_reference_tables(tag):
    f = gc.frame(tag)
    off, adj = _csr_from_device_pairs(f["labels"], f["n"], f["working"])      # what calculate_frame_cellinfo builds
    np.testing.assert_array_equal(off, f["offsets"])
    np.testing.assert_array_equal(adj, f["adj"])
    off, adj = _csr_from_device_pairs(f["labels"], f["n"], None)              # find_neighbors(only_for_labels=None)
    np.testing.assert_array_equal(off, f["all_offsets"])
    np.testing.assert_array_equal(adj, f["all_adj"])
    off, adj = _seg().neighbor_csr(_seg().neighbor_pairs(f["labels"]), f["n"], f["working"])      # the host form
    np.testing.assert_array_equal(off, f["offsets"])
    np.testing.assert_array_equal(adj, f["adj"])


def test_empty_inputs_and_a_single_label():
    seg = _seg()
    none8, none32 = np.zeros(0, np.uint8), np.zeros(0, np.int32)
    off, adj = seg.neighbor_csr(np.zeros((0, 2), np.int32), 0)                # n = 0
    assert off.tolist() == [0] and adj.size == 0
    assert seg.graph_counts(off, adj, none8, none8, none8, none32, "valid").size == 0
    assert seg.graph_second(off, adj, none8, none8, none32)[0].size == 0
    assert seg.contact_sums(np.zeros((0, 2), np.int32), np.zeros(0, np.int64), off, adj, none8, none8, none32).size == 0
    f = gc.frame("A")                                                          # m = 0 on a real graph
    assert seg.graph_counts(f["offsets"], f["adj"], f["valid"], f["empty"], f["type"], none32, "type", 0, True).size == 0
    assert seg.graph_second(f["offsets"], f["adj"], f["valid"], f["type"], none32, 0, True)[2].size == 0
    assert seg.contact_sums(*f["triples"], f["offsets"], f["adj"], f["valid"], f["type"], none32, "all", values=True)[3].size == 0
    one = np.ones((9, 7), np.int32)                                            # one label: no pair, one row of degree 0
    pairs = seg.neighbor_pairs(one)
    assert pairs.shape[0] == 0
    off, adj = seg.neighbor_csr(pairs, 1)
    assert off.tolist() == [0, 0] and adj.size == 0
    ones = np.ones(1, np.uint8)
    assert seg.graph_counts(off, adj, ones, 0 * ones, 0 * ones, None, "all").tolist() == [0]
    assert seg.graph_second(off, adj, ones, 0 * ones, None)[0].tolist() == [0]
    assert seg.contact_sums(*seg.contact_triples(one), off, adj, ones, 0 * ones, None).tolist() == [0]


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_chain_graph_offsets_at_the_scan_chunk_edges(n):
    """A chain 1 - 2 - ... - n: the single-workgroup scan of the degrees walks n in chunks of 1024, and the total lands behind
    the last one."""
    i = np.arange(1, n, dtype=np.int32)
    off, adj = _seg().neighbor_csr(np.stack([i + 1, i], axis=1), n)
    deg = np.full(n, 2, np.int64)
    deg[0] -= 1
    deg[-1] -= 1
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(deg)]))
    assert off.tolist()[:2] == ([0, 0] if n == 1 else [0, 1])
    labels = np.arange(1, n + 1)
    want = np.stack([labels - 1, labels + 1], axis=1).ravel()
    np.testing.assert_array_equal(adj, want[(want >= 1) & (want <= n)])          # every row: its one or two neighbours, ascending


def test_adj_capacity_one_short_is_an_overflow():
    from tissue_image_processing_amd import _lib
    f = gc.frame("H")
    pairs = np.ascontiguousarray(gr.neighbor_pairs(f["labels"]), np.int32)
    need = int(f["all_adj"].size)
    offsets, adj = np.zeros(f["n"] + 1, np.int32), np.full(need, -7, np.int32)
    n_adj = ctypes.c_int64(0)
    rc = _lib.lib().tip_neighbor_csr_i32(_lib.ptr(pairs), ctypes.c_int64(pairs.shape[0]), ctypes.c_int64(f["n"]), None, _lib.ptr(offsets),
                                         _lib.ptr(adj), ctypes.c_int64(need - 1), ctypes.byref(n_adj))
    assert rc == _lib.TIP_ERR_OVERFLOW and n_adj.value == need
    assert (adj == -7).all()                                                   # nothing was written
    assert str(need) in _lib.last_error()
    rc = _lib.lib().tip_neighbor_csr_i32(_lib.ptr(pairs), ctypes.c_int64(pairs.shape[0]), ctypes.c_int64(f["n"]), None, _lib.ptr(offsets),
                                         _lib.ptr(adj), ctypes.c_int64(need), ctypes.byref(n_adj))
    assert rc == 0 and n_adj.value == need
    np.testing.assert_array_equal(adj, f["all_adj"])


def test_a_null_optional_output_of_contact_sums_is_skipped():
    from tissue_image_processing_amd import _lib
    f = gc.frame("B")
    pairs, counts = np.ascontiguousarray(f["triples"][0], np.int32).reshape(-1, 2), np.ascontiguousarray(f["triples"][1], np.int64)
    n, i64 = f["n"], ctypes.c_int64
    head = (_lib.ptr(pairs), _lib.ptr(counts), i64(counts.size), _lib.ptr(f["offsets"]), _lib.ptr(f["adj"]), i64(n), i64(f["adj"].size),
            _lib.ptr(f["valid"]), _lib.ptr(f["type"]), None, i64(n), 1, -1, 1)
    got = {}
    for name, skip in (("both", ()), ("no_n_sel", ("n_sel",)), ("no_sums", ("sums",))):
        out = {k: None if k in skip else np.full(n, -7, np.int64) for k in ("sums", "n_sel")}
        _lib.check(_lib.lib().tip_contact_sums_i32(*head, _lib.ptr(out["sums"]), _lib.ptr(out["n_sel"]), None, None, None, i64(0)))
        got[name] = out
    assert got["both"]["sums"].max() > 0 and got["both"]["n_sel"].max() > 0
    np.testing.assert_array_equal(got["no_n_sel"]["sums"], got["both"]["sums"])
    np.testing.assert_array_equal(got["no_sums"]["n_sel"], got["both"]["n_sel"])


def test_argument_errors():
    seg = _seg()
    from tissue_image_processing_amd import _lib
    lib = _lib.lib()
    f = gc.frame("B")
    n, q = f["n"], np.zeros(1, np.int32)
    out = np.zeros(1, np.int64)
    i64 = ctypes.c_int64
    graph = (_lib.ptr(f["offsets"]), _lib.ptr(f["adj"]), i64(n), i64(f["adj"].size))
    rows = (_lib.ptr(f["valid"]), _lib.ptr(f["empty"]), _lib.ptr(f["type"]))
    assert lib.tip_graph_counts_i32(None, _lib.ptr(f["adj"]), i64(n), i64(f["adj"].size), *rows, _lib.ptr(q), i64(1), 0, -1, 1, _lib.ptr(out)) == _lib.TIP_ERR_ARG
    assert lib.tip_graph_counts_i32(*graph, *rows, _lib.ptr(q), i64(1), 0, -1, 1, None) == _lib.TIP_ERR_ARG
    assert lib.tip_graph_counts_i32(*graph, None, None, None, _lib.ptr(q), i64(1), 1, -1, 1, _lib.ptr(out)) == _lib.TIP_ERR_ARG
    assert lib.tip_graph_counts_i32(_lib.ptr(f["offsets"]), _lib.ptr(f["adj"]), i64(-1), i64(0), *rows, _lib.ptr(q), i64(1), 0, -1, 1, _lib.ptr(out)) == _lib.TIP_ERR_ARG
    assert lib.tip_graph_counts_i32(*graph, *rows, _lib.ptr(q), i64(1), 3, 8, 1, _lib.ptr(out)) == _lib.TIP_ERR_ARG      # type bit 8
    assert lib.tip_graph_second_i32(*graph, None, _lib.ptr(f["type"]), _lib.ptr(q), i64(1), -1, 1, _lib.ptr(out), None, None, i64(0)) == _lib.TIP_ERR_ARG
    assert lib.tip_contact_sums_i32(None, None, i64(3), *graph, rows[0], rows[2], _lib.ptr(q), i64(1), 0, -1, 1, _lib.ptr(out), None, None, None,
                                    None, i64(0)) == _lib.TIP_ERR_ARG
    assert lib.tip_neighbor_csr_i32(None, i64(0), i64(-1), None, _lib.ptr(f["offsets"]), None, i64(0), ctypes.byref(i64(0))) == _lib.TIP_ERR_ARG
    for bad in (n, n + 5, -1):                                                 # a query row outside the table
        with pytest.raises(ValueError):
            seg.graph_counts(f["offsets"], f["adj"], f["valid"], f["empty"], f["type"], [0, bad], "all")
        with pytest.raises(ValueError):
            seg.graph_second(f["offsets"], f["adj"], f["valid"], f["type"], [bad])
        with pytest.raises(ValueError):
            seg.contact_sums(*f["triples"], f["offsets"], f["adj"], f["valid"], f["type"], [bad])
    unsorted = f["adj"].copy()
    r = int(np.argmax(np.diff(f["offsets"])))
    unsorted[f["offsets"][r]:f["offsets"][r] + 2] = unsorted[f["offsets"][r]:f["offsets"][r] + 2][::-1]
    with pytest.raises(ValueError):                                            # a host CSR whose row is not ascending
        seg.graph_second(f["offsets"], unsorted, f["valid"], f["type"], [r])
    beyond = f["adj"].copy()
    beyond[0] = n + 1
    with pytest.raises(ValueError):                                            # a label outside the table
        seg.graph_counts(f["offsets"], beyond, f["valid"], f["empty"], f["type"], [0], "valid")


def golden_tissue(tag):
    """the stand-alone Tissue holding the golden frame's labels and table"""
    from tissue_image_processing_amd import tissue_info as ti
    g, f = gc.golden(), gc.frame(tag)
    t = ti.Tissue(1)
    t.type_names = ["HC", "X"]
    t.set_labels(1, f["labels"].copy(), reset_data=True)
    table = pd.DataFrame({name: g["ci_%s_%s" % (tag, name)] for name in
                          ("area", "perimeter", "cx", "cy", "bounding_box_min_row", "bounding_box_min_col", "bounding_box_max_row",
                           "bounding_box_max_col")})
    for name in ("label", "n_neighbors", "valid", "type", "empty_cell"):
        table[name] = g["ci_%s_%s" % (tag, name)].astype(np.int64)
    table["neighbors"] = gr.sets_from_csr(f["offsets"], f["adj"])
    t.set_cells_info(1, table)
    return t, table


FEATURES = {"contact length": ("all", True), "HC contact length": ("HC", True), "SC contact length": ("HC", False)}


def through_mixin(t, table, c):
    cells = table.iloc[gc.query_rows(c)]
    if c["method"] == "nnt":
        return t.calculate_n_neighbors_from_type(1, cells, cell_type=c["cell_type"], positive_for_type=c["positive"],
                                                 second_neighbors=c["second"])
    if c["method"] == "nbt":
        df = t.calculate_n_neighbors_by_type(1, cells, type_list=c["cell_type"].split(",") if c["cell_type"] else None)
        assert list(df.columns) == c["cell_type"].split(",")
        return df.to_numpy()
    if c["method"] in ("son", "son0"):
        return t.find_second_order_neighbors(1, cells=None if c["method"] == "son0" else cells, cell_type=c["cell_type"],
                                             positive_for_type=c["positive"])
    if c["method"] == "gfd":
        cell_type, positive = FEATURES[c["cell_type"]]
        sums = t.calculate_contact_lengths(1, cells, cell_type=cell_type, positive_for_type=positive)
        flat = t.calculate_contact_lengths(1, cells, cell_type=cell_type, positive_for_type=positive, for_histogram=True)
        assert sums.dtype == np.float64 and flat.sum() == sums.sum()
        return sums
    rows = []
    for _, cell in cells.iterrows():
        labels, lengths = t.calculate_contact_length(1, cell, None, None, cell_type=c["cell_type"], positive_for_type=c["positive"])
        rows.append((labels.tolist(), [int(v) for v in lengths]))
    if c["cell_type"] == "all":                                                # the batch method's histogram: the same values, row after row
        flat = t.calculate_contact_lengths(1, cells, for_histogram=True)
        assert flat.tolist() == [v for _, vals in rows for v in vals]
    return rows


@pytest.mark.parametrize("tag", gc.FRAMES)
def test_mixin_methods_equal_the_goldens(tag):
    t, table = golden_tissue(tag)
    for c in gc.cases(tag):
        if c["method"] == "nbt" and not c["cell_type"]:
            with pytest.raises(NotImplementedError):                          # recorded deviation: pos / neg type lists
                through_mixin(t, table, c)
        elif c["status"] != 0:
            with pytest.raises(getattr(builtins, c["exc"])):
                through_mixin(t, table, c)
        else:
            gc.assert_same(through_mixin(t, table, c), gc.expected(c))
    empty = table.iloc[:0]
    assert t.calculate_n_neighbors_from_type(1, empty, cell_type="same").size == 0      # upstream's loop never runs
    assert t.find_second_order_neighbors(1, empty) == [] and t.calculate_contact_lengths(1, empty).size == 0
    with pytest.raises(NotImplementedError):
        t.get_frame_data(1, "HC neighbors", table, special_features=t.SPECIAL_FEATURES)      # the routing stays as it was


def mixin_columns(labels, type=None, valid=None):
    """the ten columns of FramePipeline.neighbor_features through the stand-alone Tissue on downloaded labels"""
    from tissue_image_processing_amd import tissue_info as ti
    t = ti.Tissue(1)
    t.type_names = ["HC"]
    t.set_labels(1, np.asarray(labels).copy(), reset_data=True)
    t.calculate_frame_cellinfo(1)
    table = t.get_cells_info(1)
    if valid is not None:
        np.testing.assert_array_equal(table["valid"].to_numpy(), valid)
    out = dict(n_neighbors=t.calculate_n_neighbors_from_type(1, table, "all"),
               valid_neighbors=t.calculate_n_neighbors_from_type(1, table, "valid"),
               second_neighbors=t.calculate_n_neighbors_from_type(1, table, "all", second_neighbors=True),
               contact_length=t.calculate_contact_lengths(1, table))
    np.testing.assert_array_equal(out["n_neighbors"], table["n_neighbors"].to_numpy())
    if type is not None:
        table["type"] = np.asarray(type).astype(np.int64)
        for prefix, positive in (("hc", True), ("sc", False)):
            out[prefix + "_neighbors"] = t.calculate_n_neighbors_from_type(1, table, "HC", positive)
            out[prefix + "_second_neighbors"] = [len(s) for s in t.find_second_order_neighbors(1, table, "HC", positive)]
            out[prefix + "_contact_length"] = t.calculate_contact_lengths(1, table, "HC", positive)
    return out


def test_pipeline_neighbor_features_equal_the_mixin():
    from tissue_image_processing_amd import synthetic
    from tissue_image_processing_amd.pipeline import FramePipeline
    Z, Y, X = 6, 128, 128
    stack = synthetic.make_stack(Z, Y, X, seed=31)
    pipe = FramePipeline(2, Z, Y, X)
    pipe.project(pipe.upload_stack(stack))
    pipe.segment(0)
    tab = pipe.cell_tables()
    n = tab["area"].size
    assert n > 20
    typed = pipe.cell_types(atoh_channel=1, threshold=0.03, percentage_above_threshold=3, peak_window_size=3, n=n)
    got = pipe.neighbor_features(n, typed["valid"], typed["type"])
    plain = pipe.neighbor_features(n, typed["valid"])
    want = mixin_columns(pipe.fetch_labels(), typed["type"], typed["valid"])
    assert sorted(got) == sorted(want) and len(got) == 10 and sorted(plain) == sorted(FramePipeline.NEIGHBOR_COLUMNS)
    for name in want:
        assert got[name].dtype == np.int64
        np.testing.assert_array_equal(got[name], np.asarray(want[name]).astype(np.int64), err_msg=name)
        if name in plain:
            np.testing.assert_array_equal(plain[name], got[name])
    assert got["n_neighbors"].max() >= 3 and got["contact_length"].max() > 0 and got["second_neighbors"].max() > got["n_neighbors"].max()


def test_movie_rows_carry_the_neighbour_columns(tmp_path):
    from tissue_image_processing_amd.pipeline import FramePipeline
    out = str(tmp_path / "w1.npz")
    run_ranks("_gpu_movie_graph_worker.py", 1, (out,), timeout=600, local_rank="0")
    a, labels = np.load(out), np.load(out + ".labels.npz")
    names = FramePipeline.NEIGHBOR_COLUMNS + FramePipeline.TYPED_NEIGHBOR_COLUMNS
    assert list(a["columns"]) == ["type", "valid", "mean_intensity"] + list(names)
    for t in range(int(a["n"])):
        want = mixin_columns(labels["labels_%d" % t], a["type_%d" % t], a["valid_%d" % t])
        for name in names:
            assert a["%s_%d" % (name, t)].dtype == np.int64
            np.testing.assert_array_equal(a["%s_%d" % (name, t)], np.asarray(want[name]).astype(np.int64), err_msg="%s frame %d" % (name, t))
