"""A plain-numpy restatement of skimage.registration.optical_flow_tvl1 (scikit-image 0.18.3, 2-D, float32, no prefilter),
kept with the tests as the yardstick for the device flow at sizes the goldens do not cover.  It is not part of the product
(the product has no CPU path).

Every step keeps scikit-image's float32 operation order; the interpolations run in double and round to float32 where
scipy's map_coordinates / skimage's _warp_fast do.  tvl1() returns (flow, warps_per_level) with the levels coarse to fine.
"""
import math

import numpy as np

F32 = np.float32


def convert(img):
    """skimage.util.dtype._convert(img, float32)."""
    img = np.asarray(img)
    if img.dtype in (np.uint8, np.uint16):
        return np.multiply(img, 1.0 / np.iinfo(img.dtype).max, dtype=F32)
    return img.astype(F32)


def _gauss_taps():
    sigma = 2 * 2 / 6.0
    radius = int(4.0 * sigma + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def _correlate_reflect(a, w, axis):
    """ndi.correlate1d(mode='reflect') into a float32 array: double accumulation, scipy's symmetric-kernel order."""
    r = len(w) // 2
    a = np.moveaxis(a, axis, 0).astype(np.float64)
    n = a.shape[0]
    idx = np.arange(-r, n + r)
    idx = np.where(idx < 0, -idx - 1, idx)
    idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    p = a[idx]
    acc = p[r:r + n] * w[r]
    for j in range(r, 0, -1):
        acc = acc + (p[r - j:r - j + n] + p[r + j:r + j + n]) * w[r + j]
    return np.moveaxis(acc.astype(F32), 0, axis)


def _bilinear_f32(img, r, c):
    """skimage's bilinear_interpolation on float32 coordinates inside the image, in double, rounded once."""
    r = r.astype(np.float64)
    c = c.astype(np.float64)
    r0, c0 = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
    r1, c1 = np.ceil(r).astype(np.int64), np.ceil(c).astype(np.int64)
    dr, dc = r - r0, c - c0
    top = (1 - dc) * img[r0, c0] + dc * img[r0, c1]
    bot = (1 - dc) * img[r1, c0] + dc * img[r1, c1]
    return ((1 - dr) * top + dr * bot).astype(F32)


def reduce(img):
    """pyramid_reduce(img, 2): 7-tap reflect Gaussian (sigma 2/3), then resize(order=1, mode='reflect') to ceil(shape/2)."""
    w = _gauss_taps()
    s = _correlate_reflect(_correlate_reflect(img, w, 0), w, 1)
    H, W = s.shape
    h, wd = math.ceil(H / 2.0), math.ceil(W / 2.0)
    ar, ac = H / h, W / wd
    # _warp_fast's metric transform in float32: coordinate = a * index + (a/2 - 1/2)
    rr = F32(ar) * np.arange(h, dtype=F32) + F32(0.5 * ar - 0.5)
    cc = F32(ac) * np.arange(wd, dtype=F32) + F32(0.5 * ac - 0.5)
    R, C = np.meshgrid(rr, cc, indexing="ij")
    return _bilinear_f32(s, R, C)


def pyramid(img):
    levels = [img]
    while min(levels[-1].shape) > 32 and len(levels) < 10:
        levels.append(reduce(levels[-1]))
    return levels[::-1]


def warp_nearest(img, coords):
    """ndi.map_coordinates(img, coords, order=1, mode='nearest') into float32."""
    H, W = img.shape
    r = np.clip(coords[0].astype(np.float64), 0, H - 1)
    c = np.clip(coords[1].astype(np.float64), 0, W - 1)
    r0, c0 = np.floor(r).astype(np.int64), np.floor(c).astype(np.int64)
    tr, tc = r - r0, c - c0
    r1, c1 = np.minimum(r0 + 1, H - 1), np.minimum(c0 + 1, W - 1)
    t = img[r0, c0] * (1 - tr) * (1 - tc)
    t = t + img[r0, c1] * (1 - tr) * tc
    t = t + img[r1, c0] * tr * (1 - tc)
    t = t + img[r1, c1] * tr * tc
    return t.astype(F32)


def resize_flow(flow, shape):
    """skimage's resize_flow: ndi.zoom(order=0, mode='nearest') to `shape`, then each component times new/old."""
    out = np.empty((2,) + tuple(shape), F32)
    idx = []
    for n, o in zip(shape, flow.shape[1:]):
        z = (o - 1) / (n - 1) if n > 1 else 1.0
        idx.append(np.minimum(np.floor(np.arange(n) * z + 0.5).astype(np.int64), o - 1))
    for k in range(2):
        out[k] = F32(shape[k] / flow.shape[1 + k]) * flow[k][np.ix_(idx[0], idx[1])]
    return out


def tvl1_level(I0, I1, flow, attachment=15, tightness=0.3, num_warp=5, num_iter=10, tol=1e-4):
    """skimage's _tvl1 for 2-D; returns (flow, warps run)."""
    H, W = I0.shape
    dt = 0.25
    f0 = attachment * tightness
    f1 = dt / tightness
    tol = tol * I0.size
    gr = np.arange(H, dtype=F32)[:, None]
    gc = np.arange(W, dtype=F32)[None, :]
    u = flow.copy()
    proj = np.zeros((2, 2, H, W), F32)
    g = np.zeros((2, H, W), F32)
    warps = 0
    for _ in range(num_warp):
        warps += 1
        w = warp_nearest(I1, np.stack([u[0] + gr, u[1] + gc]))
        grad = np.array(np.gradient(w))
        NI = (grad * grad).sum(0)
        NI[NI == 0] = 1
        rho_0 = w - I0 - (grad * u).sum(0)
        snap = None
        for it in range(num_iter):
            rho = rho_0 + (grad * u).sum(0)
            idx = abs(rho) <= f0 * NI
            ua = u.copy()
            ua[:, idx] -= rho[idx] * grad[:, idx] / NI[idx]
            nidx = ~idx
            ua[:, nidx] -= (f0 * np.sign(rho[nidx])) * grad[:, nidx]
            if it == 0:
                snap = ua.copy()          # flow_previous aliases flow_auxiliary in the first data step
            u = ua.copy()
            for k in range(2):
                for _ in range(2):
                    g[0, :-1] = np.diff(u[k], axis=0)
                    g[1, :, :-1] = np.diff(u[k], axis=1)
                    norm = np.sqrt((g ** 2).sum(0))[np.newaxis]
                    norm *= f1
                    norm += 1.
                    proj[k] -= dt * g
                    proj[k] /= norm
                    d = -proj[k].sum(0)
                    d[1:] += proj[k, 0, :-1]
                    d[:, 1:] += proj[k, 1, :, :-1]
                    u[k] = ua[k] + d
        if snap is None:
            break
        diff = snap - u
        if (diff * diff).sum() < tol:
            break
    return u, warps


def tvl1(ref, mov, attachment=15, tightness=0.3, num_warp=5, num_iter=10, tol=1e-4):
    p0 = pyramid(convert(ref))
    p1 = pyramid(convert(mov))
    flow = np.zeros((2,) + p0[0].shape, F32)
    counts = []
    for lvl, (a, b) in enumerate(zip(p0, p1)):
        if lvl:
            flow = resize_flow(flow, a.shape)
        flow, n = tvl1_level(a, b, flow, attachment, tightness, num_warp, num_iter, tol)
        counts.append(n)
    return flow, counts
