"""Plain-numpy restatement of the window statistics and spatial feature maps (csrc/tip_spatial.hip, Tissue.calculate_spatial_data),
written from the behaviour of upstream's pandas code (ti.py:1194-1266, 1610-1644), for the tests and tools/spatial_map_time.py.

Upstream asks, per grid point, `cells.query("(cx - %f)**2 + (cy - %f)**2 < %f" % (x, y, radius**2))`: the centre and the squared
radius reach the comparison with six decimals, and the comparison itself is float64 arithmetic rounded step by step."""
import numpy as np

INVALID_TYPE = 255
MODES = ("density", "type_fraction", "mean")


def fmt6(v):
    """a number after its trip through "%f" """
    return float("%f" % v)


def selected(type, sel_bit, sel_positive=True):
    """the type selector over a uint8 column: sel_bit -1 takes every row; else the bit is set on a valid byte, or the negation of that"""
    type = np.asarray(type).astype(np.uint8)
    if sel_bit < 0:
        return np.ones(type.shape, bool)
    positive = (((type >> sel_bit) & 1) == 1) & (type != INVALID_TYPE)
    return positive if sel_positive else ~positive


def inside(qy, qx, r2, cy, cx):
    """(M, N) bool: row j strictly inside the circle of squared radius r2 around centre i"""
    qy, qx = np.asarray(qy, np.float64).reshape(-1, 1), np.asarray(qx, np.float64).reshape(-1, 1)
    cy, cx = np.asarray(cy, np.float64).reshape(1, -1), np.asarray(cx, np.float64).reshape(1, -1)
    return (cx - qx) ** 2 + (cy - qy) ** 2 < r2


def window_stats(qy, qx, r2, cy, cx, area, type, feat=None, sel_bit=-1, sel_positive=True, rows_per_pass=2048):
    """(n_in, area_in, n_sel, sum_sel) per centre, vectorised over passes of rows_per_pass centres.  sum_sel adds the selected rows'
    feature in table order (np.cumsum's running sum): the order one device thread uses."""
    qy, qx = np.asarray(qy, np.float64).reshape(-1), np.asarray(qx, np.float64).reshape(-1)
    area = np.asarray(area).astype(np.int64)
    feat = np.zeros(area.shape) if feat is None else np.asarray(feat, np.float64)
    sel = selected(type, sel_bit, sel_positive)
    m = qy.size
    n_in, area_in, n_sel, sum_sel = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m)
    for a in range(0, m, rows_per_pass):
        b = min(m, a + rows_per_pass)
        hit = inside(qy[a:b], qx[a:b], r2, cy, cx)
        n_in[a:b] = hit.sum(axis=1)
        area_in[a:b] = (hit * area[None, :]).sum(axis=1)
        both = hit & sel[None, :]
        n_sel[a:b] = both.sum(axis=1)
        if area.size:
            sum_sel[a:b] = np.cumsum(np.where(both, feat[None, :], 0.0), axis=1)[:, -1]
    return n_in, area_in, n_sel, sum_sel


def grid(extent, step):
    return np.arange(step // 2, extent, step)


def point_values(mode, n_in, area_in, n_sel, sum_sel):
    """the per-centre value; the mean of an empty selection is NaN"""
    n_in, area_in, n_sel = (np.asarray(v, np.float64) for v in (n_in, area_in, n_sel))
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "density":
            return np.where((n_sel == 0) | (area_in <= 0), 0.0, n_sel / area_in)
        if mode == "type_fraction":
            return np.where(n_sel == 0, 0.0, n_sel / n_in)
        return np.asarray(sum_sel, np.float64) / n_sel


def fill(shape, step, values):
    """zeros, with the block [y - s//2, y + s//2) x [x - s//2, x + s//2) of every grid point set to its value"""
    out = np.zeros(shape)
    h = step // 2
    for i, y in enumerate(grid(shape[0], step)):
        for j, x in enumerate(grid(shape[1], step)):
            out[y - h:y + h, x - h:x + h] = values[i, j]
    return out


def spatial_map(shape, step, radius, cy, cx, area, type, feat=None, sel_bit=-1, sel_positive=True, mode="density", upstream_mean=False):
    """-> (map or None, message, n_sel per grid point).  Centres are whole pixels ("%f" leaves them alone); radius**2 takes the "%f"
    trip.  upstream_mean: the mean as upstream forms it, np.average over the selected rows (numpy's pairwise sum), per grid point."""
    gy, gx = grid(shape[0], step), grid(shape[1], step)
    qy, qx = np.repeat(gy, gx.size).astype(np.float64), np.tile(gx, gy.size).astype(np.float64)
    r2 = fmt6(radius ** 2)
    n_in, area_in, n_sel, sum_sel = window_stats(qy, qx, r2, cy, cx, area, type, feat, sel_bit, sel_positive)
    counts = n_sel.reshape(gy.size, gx.size)
    if mode == "mean" and (n_sel == 0).any():
        return None, "No matching cells", counts
    values = point_values(mode, n_in, area_in, n_sel, sum_sel)
    if mode == "mean" and upstream_mean and qy.size:
        both = inside(qy, qx, r2, cy, cx) & selected(type, sel_bit, sel_positive)[None, :]
        feat = np.asarray(feat, np.float64)
        values = np.array([np.average(feat[row]) for row in both])
    return fill(shape, step, values.reshape(gy.size, gx.size)), "", counts


def roundness(area, perimeter):
    """4 pi area / perimeter**2 with upstream's six-decimal pi"""
    return 4 * fmt6(np.pi) * np.asarray(area) / (np.asarray(perimeter) ** 2)


def shape_index(area, perimeter):
    """perimeter / area**(1/2), the power as upstream writes it"""
    return np.asarray(perimeter) / (np.asarray(area) ** (1 / 2))


def edge_rows(labels):
    border = np.hstack([labels[0, :], labels[:, 0], labels[-1, :], labels[:, -1]])
    return np.unique(border[border > 0]) - 1


def valid_non_edge(labels, valid, empty_cell):
    """bool over the table's rows: valid, not empty, not touching the frame's border"""
    keep = (np.asarray(valid) == 1) & (np.asarray(empty_cell) == 0)
    keep[edge_rows(labels)[edge_rows(labels) < keep.size]] = False
    return keep


# ---- access to tests/golden/spatial_maps.npz (tools/make_goldens_spatial.py) ------------------------------------------------------
COLUMNS = ("area", "perimeter", "label", "cx", "cy", "n_neighbors", "valid", "type", "empty_cell")


def golden_columns(g, tag):
    """the table of frame `tag` as {column: array}; frame E is frame A with every row invalid"""
    cols = {k: g["ci_%s_%s" % ("A" if tag == "E" else tag, k)] for k in COLUMNS}
    if tag == "E":
        cols["valid"] = np.zeros_like(cols["valid"])
    return cols


def golden_labels(g, tag):
    return g["labels_" + ("A" if tag == "E" else tag)]


def golden_cases(g):
    """[(k, frame, radius, step, feature, cells_type, positive, status, message)]; status 0 map, 1 error return, 2 raises"""
    return [(k, str(g["case_frame"][k]), float(g["case_radius"][k]), int(g["case_step"][k]), str(g["case_feature"][k]),
             str(g["case_cells_type"][k]), bool(g["case_positive"][k]), int(g["case_status"][k]), str(g["case_msg"][k]))
            for k in range(g["case_frame"].shape[0])]


TYPE_NAMES = ["HC", "X"]      # the goldens' type names: bit 0 and bit 1


def feature_column(cols, keep, feature):
    """the averaged feature over the kept rows (None for the two ratio features)"""
    if feature in ("density", "type_fraction"):
        return None
    if feature == "roundness":
        return roundness(cols["area"][keep], cols["perimeter"][keep])
    if feature == "shape index":
        return shape_index(cols["area"][keep], cols["perimeter"][keep])
    return cols[feature][keep]


def restate_case(g, case, upstream_mean=False):
    """a golden case through the restatement -> (map or None, message, n_sel per grid point)"""
    k, tag, radius, step, feature, cells_type, positive, status, msg = case
    cols, labels = golden_columns(g, tag), golden_labels(g, tag)
    keep = valid_non_edge(labels, cols["valid"], cols["empty_cell"])
    if feature in ("HC density", "SC density", "HC type_fraction", "SC type_fraction"):
        cells_type, feature = feature.split(" ")
    sel_bit = -1 if cells_type == "all" else TYPE_NAMES.index(cells_type)
    mode = feature if feature in ("density", "type_fraction") else "mean"
    return spatial_map(labels.shape, step, radius, cols["cy"][keep], cols["cx"][keep], cols["area"][keep], cols["type"][keep],
                       feature_column(cols, keep, feature), sel_bit, positive, mode, upstream_mean=upstream_mean)


def load_golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spatial_maps.npz"), allow_pickle=False)


def build_tissue(g, tag):
    """the golden frame in the drop-in's in-memory Tissue"""
    import pandas as pd
    from tissue_image_processing_amd import tissue_info as ti
    cols = golden_columns(g, tag)
    t = ti.Tissue(1, None, ["zo", "atoh"])
    t.type_names = list(TYPE_NAMES)
    t.set_labels(1, golden_labels(g, tag).copy())
    tab = pd.DataFrame({k: cols[k] for k in ("perimeter", "cx", "cy")})
    for k in ("area", "label", "n_neighbors", "valid", "type", "empty_cell"):
        tab[k] = cols[k].astype(np.int64)
    t.set_cells_info(1, tab)
    return t
