"""CPU: the sensory-region filter without a device -- the numpy + Fraction restatement (tests/hull_restate.py) against the goldens
the reference's own methods wrote (tests/golden/sensory_region.npz, tools/make_goldens_sensory.py), and tip_sensory_region_host,
the kernels' checker, against the restatement on the goldens and on the point sets where an inexact predicate goes wrong."""
import ctypes
import os
import re

import numpy as np
import pytest

import hull_cases as hc
import hull_restate as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("tip_convex_hull_f64", "tip_convex_hull_f64_dev", "tip_points_outside_hull_f64", "tip_points_outside_hull_f64_dev",
               "tip_invalidate_cells_u8_dev", "tip_sensory_region_i32_dev", "tip_sensory_region_host")


@pytest.mark.parametrize("tag", hc.GOLDEN_CASES)
def test_restatement_equals_the_reference(tag):
    g = hc.golden()
    outside, hull = hc.exact("golden_" + tag)
    np.testing.assert_array_equal(outside, g["outside_" + tag])
    np.testing.assert_array_equal(hull, g["hull_" + tag])
    assert outside.size == g["cx_" + tag].size                      # every row is tested, invalid and empty ones included
    if "labels_" + tag in g.files:
        types_in = g["types_in_" + tag] if "types_in_" + tag in g.files else None
        valid, types = hr.remove_cells(g["labels_" + tag], types_in, g["valid_" + tag], outside)
        np.testing.assert_array_equal(valid, g["valid_out_" + tag])
        if types_in is not None:
            np.testing.assert_array_equal(types, g["types_out_" + tag])
        else:
            assert types is None


def test_golden_cases_are_what_they_claim():
    g = hc.golden()
    b = hc.golden_case("B")
    hair = hr.hair_rows(b["type"], b["valid"], b["empty"])
    assert (b["type"] == 3).sum() == 3 and ((b["type"] == 1) & (b["valid"] == 0)).sum() >= 3 and (b["empty"] == 1).sum() == 3
    assert hair.size == 12 and g["outside_B"].sum() > 0 and (g["types_in_B"] != g["types_out_B"]).any()
    assert g["boundary_rows_D"].size == 36 and not g["outside_D"].any() and g["hull_D"].size == 4
    assert g["cx_E"].size == 11500 and (g["type_E"] == 1).sum() == 3000
    for tag in hc.GOLDEN_CASES:                                     # the band: no fixture rests on Qhull's rounding
        vertex = np.isin(np.arange(g["cx_" + tag].size), g["hull_" + tag])
        near = ~vertex & (g["margin_" + tag] <= float(g["band"]) * float(g["diameter_" + tag]))
        assert not near.any() if tag != "D" else np.array_equal(np.flatnonzero(near | vertex), g["boundary_rows_D"])


def test_restatement_raises_where_the_reference_does():
    g = hc.golden()
    assert str(g["raises_C"]) == "QhullError"
    with pytest.raises(hr.NoHull):
        hr.sensory_region(g["cx_C"], g["cy_C"], g["type_C"], g["valid_C"], g["empty_cell_C"])


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_host_entry_equals_the_restatement(name):
    outside, hull = hc.host(name)
    want_outside, want_hull = hc.exact(name)
    np.testing.assert_array_equal(hull, want_hull)
    np.testing.assert_array_equal(outside, want_outside)


def test_the_cases_exercise_what_they_are_for():
    assert hc.exact("circle200")[1].size > 150
    d = hc.case("duplicates")
    hull = hc.exact("duplicates")[1]
    for v in hull:                                                  # the lowest position stands for coincident points
        assert v == np.flatnonzero((d["cx"] == d["cx"][v]) & (d["cy"] == d["cy"][v])).min()
    n = len(hc.POLY[0]) + 1
    assert not hc.exact("query_vertices")[0].any() and not hc.exact("query_edges")[0].any()
    near = hc.exact("query_nextafter")[0][n:]
    assert near.any() and not near.all()                            # one ulp decides: some outside, some inside


@pytest.mark.parametrize("name", sorted(hc.DEGENERATE))
def test_host_entry_reports_no_hull(name):
    from tissue_image_processing_amd import _lib, _segmentation as seg
    c = hc.DEGENERATE[name]
    n_hull = ctypes.c_int64(-1)
    hull, outside = np.zeros(8, np.int32), np.zeros(8, np.uint8)
    rc = _lib.load().tip_sensory_region_host(_lib.ptr(c["cx"]), _lib.ptr(c["cy"]), None, None, None, c["cx"].size, _lib.ptr(outside),
                                             _lib.ptr(hull), 8, ctypes.byref(n_hull))
    assert rc == _lib.TIP_ERR_DEGENERATE == -7 and n_hull.value == min(2, len(set(zip(c["cx"], c["cy"]))))
    with pytest.raises(seg.NoHullError):
        seg.sensory_region_host(c["cx"], c["cy"], None, None)
    assert issubclass(seg.NoHullError, ValueError)
    with pytest.raises(hr.NoHull):
        hr.sensory_region(c["cx"], c["cy"])


def test_host_entry_edges_of_its_contract():
    from tissue_image_processing_amd import _lib, _segmentation as seg
    lib = _lib.load()
    n_hull = ctypes.c_int64(-1)
    hull = np.zeros(8, np.int32)
    # no rows at all: no hull
    assert lib.tip_sensory_region_host(None, None, None, None, None, 0, None, _lib.ptr(hull), 8, ctypes.byref(n_hull)) == -7
    # no outside array (no queries wanted): the hull alone
    c = hc.case("query_vertices")
    assert lib.tip_sensory_region_host(_lib.ptr(c["cx"]), _lib.ptr(c["cy"]), _lib.ptr(c["type"]), _lib.ptr(c["valid"]), _lib.ptr(c["empty"]),
                                       c["cx"].size, None, _lib.ptr(hull), 8, ctypes.byref(n_hull)) == 0
    np.testing.assert_array_equal(hull[:n_hull.value], hc.exact("query_vertices")[1])
    # a capacity one too small: the overflow report names the size needed and writes nothing
    hull[:] = -1
    assert lib.tip_sensory_region_host(_lib.ptr(c["cx"]), _lib.ptr(c["cy"]), _lib.ptr(c["type"]), _lib.ptr(c["valid"]), _lib.ptr(c["empty"]),
                                       c["cx"].size, None, _lib.ptr(hull), n_hull.value - 1, ctypes.byref(n_hull)) == _lib.TIP_ERR_OVERFLOW
    assert n_hull.value == len(hc.POLY[0]) and (hull == -1).all()
    with pytest.raises(ValueError):
        seg.sensory_region_host([0.0, 1.0, np.nan, 5.0], [0.0, 4.0, 1.0, 2.0], None, None)
    # the selection is an equality: type 3 and valid 2 span nothing
    cx, cy = np.array([0.0, 10.0, 0.0, 10.0, 5.0]), np.array([0.0, 0.0, 10.0, 10.0, 30.0])
    outside, h = seg.sensory_region_host(cx, cy, np.array([1, 1, 1, 1, 3], np.uint8), np.ones(5, np.uint8), np.zeros(5, np.uint8))
    assert list(h) == [0, 1, 3, 2] and list(outside) == [0, 0, 0, 0, 1]
    outside, h = seg.sensory_region_host(cx, cy, np.ones(5, np.uint8), np.array([1, 1, 1, 1, 2], np.uint8), None)
    assert list(h) == [0, 1, 3, 2] and list(outside) == [0, 0, 0, 0, 1]


def test_new_entries_are_declared_and_exported():
    from tissue_image_processing_amd import _abi, _lib
    text = open(os.path.join(ROOT, "include", "tissue_hip.h")).read()
    declared = re.findall(r"TIP_API\s+int\s+(tip_\w+)\s*\(", text)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in declared and name in _abi.SIGNATURES and hasattr(lib, name), name
    assert "TIP_ERR_DEGENERATE = -7" in text


def test_tissue_has_the_two_methods():
    from tissue_image_processing_amd.tissue_info import Tissue, TissueHipMixin
    assert isinstance(TissueHipMixin.__dict__["detect_non_sensory_region_cells"], staticmethod)
    assert callable(Tissue.remove_cells_outside_of_sensory_region)
    tissue = Tissue(1)
    assert tissue.remove_cells_outside_of_sensory_region(1) == 0       # no labels: returns 0, touches no device
