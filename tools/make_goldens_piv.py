#!/opt/conda/bin/python3.9
"""Golden vectors for the TV-L1 optical flow (skimage.registration.optical_flow_tvl1, scikit-image 0.18.3) and for the
reference's track_cells_iterator(use_piv=True) (ti.py:2061-2070).

Run in the build container only, like tools/make_goldens.py (same interpreter, same stubs):
    /opt/conda/bin/python3.9 tools/make_goldens_piv.py

Writes tests/golden/optflow_<case>.npz (one file per case: inputs as given, flows as float32, warps per pyramid level counted by wrapping
skimage.registration._optical_flow.warp) and tests/golden/piv_tracking.npz (ids per frame of the reference tracker on a
drifting synthetic tessellation, once with the real flow and once with a fixed analytic field).  Only DATA is written.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402  (stubs, reference import path, save())

np, ndi, ti, synthetic = mg.np, mg.ndi, mg.ti, mg.synthetic
import skimage.segmentation  # noqa: E402
import skimage.registration._optical_flow as OF  # noqa: E402
from skimage.registration import optical_flow_tvl1  # noqa: E402

_counts = []
_orig_warp, _orig_tvl1 = OF.warp, OF._tvl1


def _count_warp(*a, **k):
    _counts[-1] += 1
    return _orig_warp(*a, **k)


def _count_level(*a, **k):
    _counts.append(0)
    return _orig_tvl1(*a, **k)


OF.warp, OF._tvl1 = _count_warp, _count_level


def scene(H, W, seed, n=60):
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W))
    for _ in range(n):
        cy, cx, s = r.random() * H, r.random() * W, 2 + 6 * r.random()
        img += r.random() * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return img / img.max()


def gold_flows():
    base = scene(256, 256, 1)
    shifted = ndi.shift(base, (1.3, -0.7), order=3, mode="nearest")
    a16, b16 = (base * 60000).astype(np.uint16), (shifted * 60000).astype(np.uint16)
    yy, xx = np.mgrid[0:181, 0:243].astype(np.float64)
    odd = scene(181, 243, 2)
    odd_moved = ndi.map_coordinates(odd, [yy - 0.8 - 0.6 * np.sin(xx / 40.0), xx + 0.5 + 0.7 * np.cos(yy / 30.0)], order=3,
                                    mode="nearest")
    small = scene(24, 40, 3, 8)
    cases = {
        "shift": (a16, b16, {}),
        "shift_tol3e-3": (a16, b16, {"tol": 3e-3}),
        "identical": (a16, a16.copy(), {}),
        "odd_f64": (odd, odd_moved, {}),
        "single_level": (small, ndi.shift(small, (0.4, 0.6), order=3, mode="nearest"), {}),
        "constant": (np.full((48, 40), 1234, np.uint16), np.full((48, 40), 1234, np.uint16), {}),
    }
    for name, (a, b, kw) in cases.items():
        _counts.clear()
        flow = optical_flow_tvl1(a, b, **kw)
        assert flow.dtype == np.float32
        mg.save("optflow_" + name, ref=a, mov=b, flow=flow, warps=np.array(_counts, np.int32),
                tol=np.array(kw.get("tol", 1e-4)))


def _movie(n=128, frames=4):
    sites_t, _ = synthetic.make_movie_sites(n, n, frames, seed=21)
    labs, imgs = [], []
    for f in range(frames):
        d1, d2, _ = synthetic._two_nearest(sites_t[f], n, n)
        membrane = np.exp(-((d2 - d1) ** 2) / 4.0)
        lab = skimage.segmentation.watershed(ndi.gaussian_filter(membrane, 1.5), watershed_line=True)
        labs.append(lab.astype(np.int32))
        imgs.append((membrane * 50000 + 1000).astype(np.uint16))
    return np.stack(labs), np.stack(imgs)


def _track(labs, imgs):
    frames = labs.shape[0]
    t = ti.Tissue(frames, os.path.join(mg.tempfile.mkdtemp(prefix="tipgold_"), "movie_p"), ["zo"], load_to_memory=True)
    for f in range(frames):
        t.labels_list[f] = labs[f]
        t.set_labels(f + 1, labs[f].copy(), reset_data=False)
        t.calculate_frame_cellinfo(f + 1)
        t.cell_info_list[f] = t.cells_info.copy()
    before = [t.get_cells_info(f + 1)[["cx", "cy"]].to_numpy().astype(np.float64).copy() for f in range(frames)]
    for _ in t.track_cells_iterator(1, frames, images=imgs, image_in_memory=True, use_piv=True):
        pass
    ids = [t.get_cells_info(f + 1).label.to_numpy().astype(np.int64) for f in range(frames)]
    return ids, before, t.drifts.copy()


def gold_piv_tracking():
    labs, imgs = _movie()
    flows = []
    orig = ti.optical_flow_tvl1

    def recording(a, b):
        flows.append(orig(a, b))
        return flows[-1]

    def analytic(a, b):
        yy, xx = np.mgrid[0:a.shape[0], 0:a.shape[1]].astype(np.float32)
        return np.stack([0.6 + 0.01 * yy - 0.004 * xx, -0.9 + 0.007 * xx]).astype(np.float32)

    out = {"labels": labs, "images": imgs}
    for tag, fn in (("flow", recording), ("analytic", analytic)):
        ti.optical_flow_tvl1 = fn
        flows.clear()
        ids, before, drifts = _track(labs, imgs)
        for f, v in enumerate(ids):
            out["%s_ids_%d" % (tag, f)] = v
        out[tag + "_drifts"] = drifts
        if tag == "flow":
            # the lookups round cx - flow, cy - flow: how close any of them came to a .5 boundary
            margin = np.inf
            for f, fl in enumerate(flows):
                cx, cy = before[f][:, 0], before[f][:, 1]
                r, c = np.round(cx).astype(int), np.round(cy).astype(int)
                for v in (cx - fl[0][r, c], cy - fl[1][r, c]):
                    margin = min(margin, float(np.min(np.abs(np.abs(v - np.floor(v)) - 0.5))))
            out["flow_margin"] = np.array(margin)
            print("piv tracking: lookup margin from .5 = %.3g" % margin)
    ti.optical_flow_tvl1 = orig
    mg.save("piv_tracking", **out)


if __name__ == "__main__":
    gold_flows()
    gold_piv_tracking()
