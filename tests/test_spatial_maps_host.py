"""CPU: the numpy restatement of the window statistics and spatial maps (tests/spatial_restate.py) against the goldens made by the
reference's own `calculate_spatial_data` / `get_frame_data` (tools/make_goldens_spatial.py), and the host-side helpers of the drop-in
(`get_valid_non_edge_cells`, `get_cells_inside_a_circle`, the element-wise features, the global features of `get_frame_data`).

Bounds.  density / type_fraction are integer counts, an exact integer sum and one division: bit for bit.  A mean is a sum of n_sel
same-sign doubles and a division: summed in another order than upstream's np.average it differs by at most n_sel 2^-52 relative (the
worst-case reordering error), asserted per grid point with that point's n_sel.  "shape index" holds a pow(area, 0.5) whose last bit
differs between numpy builds (both results are neighbours of the true value): per cell at most 2^-52 from the power, plus two
roundings of the quotient, 2^-51 relative."""
import numpy as np
import pandas as pd
import pytest

import spatial_restate as sr
from tissue_image_processing_amd import tissue_info as ti

@pytest.fixture(scope="module")
def g(golden):
    return golden("spatial_maps")


CASES = sr.golden_cases(sr.load_golden())
IDS = ["%02d-%s-r%g-s%d-%s-%s-%d" % c[:7] for c in CASES]


def assert_mean_bound(got, ref, n_sel_map):
    bound = n_sel_map * 2.0 ** -52 * np.abs(ref)
    err = np.abs(got - ref)
    worst = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))
    print("mean map: worst error / bound = %.3g" % worst)
    assert (err <= bound).all()


@pytest.mark.parametrize("case", [c for c in CASES if c[7] != 2], ids=[i for i, c in zip(IDS, CASES) if c[7] != 2])
def test_restatement_equals_golden(g, case):
    k, tag, radius, step, feature, cells_type, positive, status, msg = case
    got, got_msg, n_sel = sr.restate_case(g, case)
    if status == 1:
        assert got is None and got_msg == msg == "No matching cells"
        return
    ref = g["case%02d_map" % k]
    assert got_msg == "" and got.shape == ref.shape and got.dtype == np.float64
    split = feature.split(" ")[-1]
    if split in ("density", "type_fraction"):
        np.testing.assert_array_equal(got, ref)                     # bit for bit
        return
    assert_mean_bound(got, ref, sr.fill(ref.shape, step, n_sel))
    if feature in ("area", "n_neighbors", "roundness"):             # summed as upstream sums (np.average per window): the same bits
        np.testing.assert_array_equal(sr.restate_case(g, case, upstream_mean=True)[0], ref)


def test_golden_covers_the_issue(g):
    """the cases the goldens were asked to hold are there, with the outcomes that make them cases"""
    by = {(c[1], c[2], c[3], c[4], c[5], c[6]): c for c in CASES}
    assert {c[3] for c in CASES} == {1, 2, 5, 7, 16} and {c[2] for c in CASES} == {10.0, 25.5, 60.0}
    assert by[("A", 10.0, 2, "area", "all", True)][7] == 1                                  # empty windows: the error return
    empty = g["case%02d_map" % by[("A", 10.0, 2, "HC density", "all", True)][0]]
    assert (sr.restate_case(g, by[("A", 10.0, 2, "HC density", "all", True)])[2] == 0).any() and (empty == 0).any()
    assert not g["case%02d_map" % by[("A", 25.5, 1, "HC density", "all", True)][0]].any()   # step 1: nothing is filled
    assert not g["case%02d_map" % by[("E", 25.5, 5, "HC density", "all", True)][0]].any()   # no valid non-edge cell
    assert by[("E", 25.5, 5, "area", "all", True)][7] == 1
    assert by[("A", 25.5, 5, "SC density", "all", True)][7:] == (2, "KeyError")
    assert any(not c[6] for c in CASES)


def test_percent_f_rounding_of_the_radius_decides():
    """radius 10.0001: radius**2 = 100.00200001, "%f" makes it 100.002; a cell at squared distance 100.002000005 is inside the
    exact circle and outside upstream's"""
    radius = 10.0001
    d = np.sqrt(100.002000005)
    cy, cx = np.array([4.0]), np.array([4.0 + d])
    dist2 = (cx[0] - 4.0) ** 2 + (cy[0] - 4.0) ** 2
    assert sr.fmt6(radius ** 2) == 100.002 and sr.fmt6(radius ** 2) <= dist2 < radius ** 2
    out, msg, n_sel = sr.spatial_map((8, 8), 8, radius, cy, cx, np.array([50]), np.array([1]), mode="density")
    assert n_sel.tolist() == [[0]] and not out.any()
    out, msg, n_sel = sr.spatial_map((8, 8), 8, 10.0002, cy, cx, np.array([50]), np.array([1]), mode="density")
    assert n_sel.tolist() == [[1]] and out[0, 0] == 1 / 50
    # the drop-in's host helper rounds the same way, the centre included: 4.0000004 reads 4.000000, 4.0000006 reads 4.000001
    cells = pd.DataFrame({"cx": cx, "cy": cy})
    assert ti.Tissue.get_cells_inside_a_circle(cells, (4.0, 4.0), radius).shape[0] == 0
    assert ti.Tissue.get_cells_inside_a_circle(cells, (4.0, 4.0), 10.0002).shape[0] == 1
    edge = pd.DataFrame({"cx": [14.0000005], "cy": [4.0]})          # 10.0000005 from x = 4, 10.0000001 from x = 4.0000004
    assert ti.Tissue.get_cells_inside_a_circle(edge, (4.0, 4.0000004), 10.0000003).shape[0] == 0
    assert ti.Tissue.get_cells_inside_a_circle(edge, (4.0, 4.0000006), 10.0000003).shape[0] == 1


def test_cell_on_the_circle_is_outside():
    """strict <: integer coordinates 3-4-5 from the centre, radius 5"""
    out, msg, n_sel = sr.spatial_map((8, 8), 8, 5, np.array([7.0, 7.0]), np.array([8.0, 7.5]), np.array([10, 30]), np.array([0, 0]),
                                     mode="density")
    assert n_sel.tolist() == [[1]] and out[0, 0] == 1 / 30


def test_seam_rule():
    """step 5 on 13 x 12: grid rows 2, 7, 12 and columns 2, 7 (12 is no column): row blocks [0, 4), [5, 9), [10, 13) -- the last one
    clipped by the frame --, column blocks [0, 4), [5, 9); rows / columns 4 and 9 are seams and columns 10, 11 belong to no grid point.
    Step 1 fills nothing; an even step tiles without seams."""
    assert sr.grid(13, 5).tolist() == [2, 7, 12] and sr.grid(12, 5).tolist() == [2, 7]
    vals = np.arange(1, 7, dtype=np.float64).reshape(3, 2)
    out = sr.fill((13, 12), 5, vals)
    expect = np.zeros((13, 12))
    for i, (r0, r1) in enumerate(((0, 4), (5, 9), (10, 13))):
        for j, (c0, c1) in enumerate(((0, 4), (5, 9))):
            expect[r0:r1, c0:c1] = vals[i, j]
    np.testing.assert_array_equal(out, expect)
    assert not out[4].any() and not out[9].any() and not out[:, 4].any() and not out[:, 9:].any() and out[12, 8] == 6
    assert not sr.fill((6, 6), 1, np.ones((6, 6))).any()
    assert sr.fill((8, 8), 4, np.ones((2, 2))).all()


def test_error_returns():
    cy, cx, area, typ = np.array([4.0]), np.array([4.0]), np.array([20]), np.array([0])
    out, msg, _ = sr.spatial_map((16, 8), 8, 3, cy, cx, area, typ, feat=area.astype(float), mode="mean")
    assert out is None and msg == "No matching cells"              # the second grid point (12, 4) sees no cell
    out, msg, _ = sr.spatial_map((16, 8), 8, 3, cy, cx, area, typ, mode="density")
    assert msg == "" and out[0, 0] == 1 / 20 and not out[8:].any()
    out, msg, _ = sr.spatial_map((16, 8), 8, 3, cy, cx, area, typ, sel_bit=0, mode="type_fraction")
    assert msg == "" and not out.any()                             # cells, but none of the type: 0, not an error
    out, msg, _ = sr.spatial_map((16, 8), 8, 3, cy[:0], cx[:0], area[:0], typ[:0], mode="density")
    assert msg == "" and not out.any()                             # an empty table


def test_selector_treats_invalid_bytes_as_upstream():
    typ = np.array([0, 1, 2, 3, 255])
    assert sr.selected(typ, 0, True).tolist() == [False, True, False, True, False]
    assert sr.selected(typ, 0, False).tolist() == [True, False, True, False, True]      # the negation takes the invalid byte
    assert sr.selected(typ, 1, True).tolist() == [False, False, True, True, False]
    np.testing.assert_array_equal(sr.selected(typ, 1, True), ti.is_positive_for_type(typ, 1))


# ---- the drop-in's host-side helpers (no device involved) -----------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["A", "B"])
def test_helpers_equal_reference(g, tag):
    t = sr.build_tissue(g, tag)
    info = t.get_cells_info(1)
    valid = t.get_valid_non_edge_cells(1, info)
    np.testing.assert_array_equal(valid.index.to_numpy(), g["valid_rows_" + tag])
    np.testing.assert_array_equal(np.flatnonzero(sr.valid_non_edge(t.get_labels(1), info.valid, info.empty_cell)), g["valid_rows_" + tag])
    kw = dict(special_features=t.SPECIAL_FEATURES, global_features=t.GLOBAL_FEATURES, spatial_features=t.SPATIAL_FEATURES)
    for feature in ("roundness", "area", "perimeter", "n_neighbors", "density", "type_fraction", "total_area", "number_of_cells"):
        data, msg = t.get_frame_data(1, feature, valid, **kw)
        assert msg == ""
        np.testing.assert_array_equal(np.asarray(data, dtype=np.float64), g["gfd_%s_%s" % (tag, feature)], err_msg=feature)
    shape_index, _ = t.get_frame_data(1, "shape index", valid, **kw)
    ref = g["gfd_%s_shape index" % tag]
    assert (np.abs(shape_index - ref) <= 2.0 ** -51 * ref).all()
    hc = info.loc[g["hc_rows_" + tag]]
    for feature in ("density", "type_fraction", "total_area", "number_of_cells"):
        data, _ = t.get_frame_data(1, feature, hc, **kw)
        np.testing.assert_array_equal(np.asarray(data, dtype=np.float64), g["gfd_hc_%s_%s" % (tag, feature)], err_msg=feature)
    assert t.calculate_density(1, valid, reference_area=0) == 0 and t.calculate_type_fraction(1, valid, reference_cell_num=0) == 0
    assert ti.Tissue.calculate_total_area(valid) == valid.area.sum()


def test_features_that_are_not_built_say_so(g):
    t = sr.build_tissue(g, "A")
    valid = t.get_valid_non_edge_cells(1, t.get_cells_info(1))
    kw = dict(special_features=t.SPECIAL_FEATURES + t.SPECIAL_X_ONLY_FEATURES, global_features=t.GLOBAL_FEATURES,
              spatial_features=t.SPATIAL_FEATURES)
    for feature in ("psi6", "HC neighbors", "contact length", "Distance from ablation", "neighbors correlation"):
        with pytest.raises(NotImplementedError, match=feature):
            t.get_frame_data(1, feature, valid, **kw)
    with pytest.raises(KeyError):                      # not listed as special by the caller: a plain column lookup, as upstream
        t.get_frame_data(1, "roundness", valid)
    with pytest.raises(KeyError):                      # a name that is no type (upstream indexes the table with a scalar False)
        t._window_selector("SC", True)
    assert t._window_selector("X", False) == (1, False) and t._window_selector("all", False) == (-1, True)
    with pytest.raises(NotImplementedError, match="total_area"):
        t._window_feature(1, "total_area", valid)


# ---- the mixin in front of a class that has its own get_frame_data (INTEGRATION.md option B) ---------------------------------------
class HostStub(object):
    """stands for the reference's Tissue behind the mixin: records what reaches it"""

    def get_frame_data(self, frame, feature, valid_cells, special_features=[], global_features=[], spatial_features=[],
                       for_histogram=False, reference=None, intensity_img=None, window_radius=0, types=None):
        self.calls.append(("get_frame_data", frame, feature, valid_cells.shape[0], for_histogram, reference, intensity_img, window_radius,
                           types, tuple(special_features), tuple(global_features), tuple(spatial_features)))
        if feature == "contact length" and for_histogram:
            return np.arange(3.0), ""                  # one value per contact, not per cell
        return np.full(valid_cells.shape[0], 2.0), ""

    def calculate_spatial_data(self, frame, window_radius, step_size, feature, cells_type='all', positive_for_type=True):
        self.calls.append(("calculate_spatial_data", frame, window_radius, step_size, feature, cells_type, positive_for_type))
        return "the host's map", ""


def test_unbuilt_features_go_to_the_class_behind_the_mixin(g):
    class Mixed(ti.Tissue, HostStub):                  # MRO: Mixed, Tissue, TissueHipMixin, HostStub
        pass

    t = sr.build_tissue(g, "A")
    t.__class__ = Mixed
    t.calls = []
    valid = t.get_valid_non_edge_cells(1, t.get_cells_info(1))
    kw = dict(special_features=t.SPECIAL_FEATURES + t.SPECIAL_X_ONLY_FEATURES, global_features=t.GLOBAL_FEATURES,
              spatial_features=t.SPATIAL_FEATURES)
    for feature in ("psi6", "HC neighbors", "SC second neighbors", "contact length", "Distance from ablation", "neighbors by type",
                    "neighbors correlation", "neighbors correlation average"):
        data, msg = t.get_frame_data(1, feature, valid, for_histogram=False, reference=7, intensity_img="img", window_radius=3,
                                     types=["HC"], **kw)
        assert msg == "" and (data == 2.0).all()
        assert t.calls[-1] == ("get_frame_data", 1, feature, valid.shape[0], False, 7, "img", 3, ["HC"], tuple(kw["special_features"]),
                               tuple(kw["global_features"]), tuple(kw["spatial_features"]))
    seen = len(t.calls)
    for feature in ("roundness", "shape index", "density", "type_fraction", "total_area", "number_of_cells", "area"):
        t.get_frame_data(1, feature, valid, **kw)      # built here: the class behind is not asked
    assert len(t.calls) == seen
    # a map of a feature that is no device mode is the host class's own loop, asked with the caller's names
    assert t.calculate_spatial_data(1, 25.5, 5, "total_area", cells_type="HC", positive_for_type=False) == ("the host's map", "")
    assert t.calls[-1] == ("calculate_spatial_data", 1, 25.5, 5, "total_area", "HC", False)
    assert t.calculate_spatial_data(1, 25.5, 5, "contact length") == ("the host's map", "")      # not one value per cell
    assert t.calls[-1] == ("calculate_spatial_data", 1, 25.5, 5, "contact length", "all", True)


def test_mean_atoh_intensity_is_the_mixins_own(g):
    """the mixin has calculate_mean_intensity: a table that holds the column answers without the device or a host class"""
    t = sr.build_tissue(g, "A")
    info = t.get_cells_info(1)
    info["mean_intensity_HC"] = np.arange(info.shape[0], dtype=np.float64)
    valid = t.get_valid_non_edge_cells(1, info)
    data, msg = t.get_frame_data(1, "Mean atoh intensity", valid, special_features=t.SPECIAL_FEATURES)
    np.testing.assert_array_equal(data, valid["mean_intensity_HC"].to_numpy())
