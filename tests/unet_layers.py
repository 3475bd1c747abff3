"""Shared by the layer-level U-Net tests (test_gpu_unet_conv.py, test_gpu_unet_compose.py, test_gpu_unet_flavours.py,
test_gpu_unet_six_taps.py, test_gpu_unet_mfma16.py, test_unet_plan_host.py): the piece formats on the host, the per-layer error
bounds, one launcher for tip_unet_conv_dev that names the kernel flavour it means to run and fences every output with sentinels, the
float64 evaluation of the same stencil on the unsplit values, and the EXACT and RANDOM cases of the one-launch tests (exact_case,
random_case: cached, so every test file of a process draws a case once; run_case, bits)."""
import ctypes
import functools
import math

MODES = {"f16x3": (2, 1), "bf16x3": (2, 0), "bf16x6": (3, 0)}     # mode -> (planes, piece format)
TOL = {"f16x3": 2e-6, "bf16x3": 4e-5, "bf16x6": 2e-6}             # one layer: max error / max |reference|
HEAD_TOL = {"f16x3": 4e-6, "bf16x3": 3e-5, "bf16x6": 4e-6}        # class probabilities, absolute (the network tests' bounds)
ACT = 16.0                                                        # _unet_hip._F16_ACT_SCALE

# tip_unet_conv_flavour's codes (include/tissue_hip.h) -> <pieces, tile rows, D, DA, SPB>
FLAVOURS = {0: (2, 8, 2, 1, 1), 1: (2, 16, 2, 1, 1), 2: (2, 16, 4, 1, 1), 3: (3, 8, 2, 1, 1), 4: (2, 16, 2, 2, 1), 6: (2, 16, 4, 1, 3)}

# tap offsets (dy, dx) in a fixed order no reflection, rotation or transposition maps onto itself: a stencil of n < 9 taps takes the
# first n, nine taps are the 3x3 stencil in kernel order
_TAP_ORDER = [(-1, 0), (0, 1), (1, 1), (0, 0), (1, -1), (-1, -1), (0, -1), (-1, 1), (1, 0)]

GUARD = 4096                 # sentinel elements in front of and behind every output tensor (a multiple of the kernels' 16-byte stores)
PIECE_SENTINEL = 0x5A5A      # the 16-bit planes' sentinel, compared as int16 (as bf16 / fp16 a finite value no test computes)


def _split(t, planes, fmt=0):
    """float32 tensor -> pieces; fp16 pieces (fmt 1) of the values times ACT, as the kernels store activations"""
    import torch
    pieces, rest = [], (t.float() * ACT if fmt else t.float())
    for _ in range(planes):
        h = rest.to(torch.float16 if fmt else torch.bfloat16)
        pieces.append(h)
        rest = rest - h.float()
    return torch.stack(pieces, 0).contiguous()


def _join(planes_t, fmt=0):
    v = planes_t.float().sum(0)
    return v / ACT if fmt else v


def _regions(H, W):
    """name -> index of the output (H, W, C): the whole tensor, the four edges, the four corners, the interior"""
    r = {"all": (slice(None), slice(None)), "first row": (0, slice(None)), "last row": (H - 1, slice(None)),
         "first column": (slice(None), 0), "last column": (slice(None), W - 1), "interior": (slice(1, H - 1), slice(1, W - 1))}
    for ny, y in (("top", 0), ("bottom", H - 1)):
        for nx, x in (("left", 0), ("right", W - 1)):
            r["%s-%s corner" % (ny, nx)] = (y, x)
    return r


def _assert_regions(mode, what, got, ref, names):
    H, W = ref.shape[:2]
    top = float(ref.abs().max())
    regions = _regions(H, W)
    for name in names:
        idx = regions[name]
        err = float((got[idx] - ref[idx]).abs().max()) / top
        print("%s %s, %s: max error / max |value| = %.2e" % (mode, what, name, err))
        assert err < TOL[mode], (what, name)


def seams(H, W, th):
    """name -> index of the rows / columns on either side of every seam between two th-row x 32-column tiles"""
    r = {}
    for y in range(th, H, th):
        r["rows %d, %d" % (y - 1, y)] = (slice(y - 1, y + 1), slice(None))
    for x in range(32, W, 32):
        r["columns %d, %d" % (x - 1, x)] = (slice(None), slice(x - 1, x + 1))
    return r


def assert_seams(mode, what, got, ref, th):
    """the bound of _assert_regions on the pixels either side of every tile seam"""
    H, W = ref.shape[:2]
    top = float(ref.abs().max())
    for name, idx in seams(H, W, th).items():
        err = float((got[idx] - ref[idx]).abs().max()) / top
        print("%s %s, %s: max error / max |value| = %.2e" % (mode, what, name, err))
        assert err < TOL[mode], (what, name)


def tap_offsets(ntaps):
    """(dy list, dx list) of an ntaps-tap stencil"""
    offs = [(k // 3 - 1, k % 3 - 1) for k in range(9)] if ntaps == 9 else _TAP_ORDER[:ntaps]
    return [o[0] for o in offs], [o[1] for o in offs]


class Fenced:
    """A device tensor of `shape` inside a larger buffer filled with a sentinel: NaN (float32) or PIECE_SENTINEL (16-bit planes)."""

    def __init__(self, shape, dtype, dev):
        import torch
        n = int(math.prod(shape))
        self.n = n
        if dtype == torch.float32:
            self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
            self.bits, self.sentinel = torch.int32, int(self.buf[:1].view(torch.int32).cpu()[0])
        else:
            self.buf = torch.full((n + 2 * GUARD,), PIECE_SENTINEL, dtype=torch.int16, device=dev).view(dtype)
            self.bits, self.sentinel = torch.int16, PIECE_SENTINEL
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def untouched(self, t):
        return bool((t.view(self.bits) == self.sentinel).all())

    def check(self, what, written=None):
        """the guard bands hold the sentinel; written = (oy, ox, stride): of a (..., H, W, C) tensor only the pixels (oy::stride,
        ox::stride) were written -- every other parity class holds the sentinel too"""
        assert self.untouched(self.buf[:GUARD]), "%s: written in front of the tensor" % what
        assert self.untouched(self.buf[GUARD + self.n:]), "%s: written behind the tensor" % what
        if written is not None:
            oy, ox, s = written
            for py in range(s):
                for px in range(s):
                    if (py, px) != (oy, ox):
                        assert self.untouched(self.t[..., py::s, px::s, :]), "%s: parity class (%d, %d) was written" % (what, py, px)


def describe(mode, a0, a1, taps, dy, dx, cout=None, **kw):
    """The descriptor of run_layer's launch over DUMMY (non-null, never dereferenced) pointers: for tip_unet_conv_flavour alone.
    a0 / a1: (H, W, C) shapes; taps: the number of taps; cout: output channels; keywords: descriptor fields to override."""
    from tissue_image_processing_amd import _unet_hip as uh
    planes, fmt = MODES[mode]
    d = uh._ConvDesc()
    H, W, c0 = a0
    d.in0, d.c0, d.h, d.w, d.planes, d.format, d.acc_scale = 64, c0, H, W, planes, fmt, 1.0
    d.in1, d.c1 = (64, a1[2]) if a1 is not None else (None, 0)
    d.weights, d.ntaps, d.cout = 64, taps, cout
    for i in range(min(taps, len(dy), 9)):
        d.dy[i], d.dx[i] = dy[i], dx[i]
    d.bias, d.scale, d.shift, d.out = 64, 64, 64, 64
    d.out_h, d.out_w, d.sy, d.sx, d.oy, d.ox = H, W, 1, 1, 0, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def run_layer(mode, a0, a1, taps, dy, dx, flavour, bias=None, scale=None, shift=None, raw=False, seed=None, pool=False, head=None,
              stride=1, oy=0, ox=0):
    """One tip_unet_conv_dev launch on cuda:0.  a0 (H, W, C0), a1 (H, W, C1) or None, taps (T, Cin, Cout), bias / scale / shift (Cout)
    and seed (H, W, Cout): float32 host tensors in the layer's own units; scale None: a bias-only layer; raw: the float32 sum instead
    of everything else; head = (weights (2, Cout), bias (2,)): the fused head instead of the stored output.  `flavour` is the code
    tip_unet_conv_flavour must return for the descriptor -- asserted BEFORE the launch.  Every output lives in a Fenced buffer whose
    guard bands (and, with stride 2, unwritten parity classes) are checked.  Returns host tensors: "out" (planes, sH, sW, Cout) in
    the pieces' dtype, "pool" (planes, H/2, W/2, Cout), "raw" (sH, sW, Cout), "head" (2, H, W); "status": the fp16 range word."""
    import torch
    from tissue_image_processing_amd import _unet_hip as uh, _lib
    planes, fmt = MODES[mode]
    A = ACT if fmt else 1.0
    store = torch.float16 if fmt else torch.bfloat16
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    H, W = a0.shape[:2]
    cout = taps.shape[2]
    oH, oW = H * stride, W * stride
    bias_only = scale is None and not raw
    wp, inv = uh._pack(taps.float().to(dev), planes, fmt, bias_only)
    p0 = _split(a0, planes, fmt).to(dev)
    p1 = _split(a1, planes, fmt).to(dev) if a1 is not None else None
    keep = [wp, p0, p1]
    fb = fs = ft = None
    if not raw:
        fb = (bias.float() * (A if bias_only else 1.0)).to(dev)
        if scale is not None:
            fs, ft = (scale.float() * A).to(dev), (shift.float() * A).to(dev)
    fenced = {}
    if raw:
        fenced["raw"] = Fenced((oH, oW, cout), torch.float32, dev)
    elif head is not None:
        fenced["head"] = Fenced((2, H, W), torch.float32, dev)
        keep += [(head[0].float() / A).contiguous().to(dev), head[1].float().to(dev)]
    else:
        fenced["out"] = Fenced((planes, oH, oW, cout), store, dev)
        if pool:
            fenced["pool"] = Fenced((planes, H // 2, W // 2, cout), store, dev)
    sd = seed.float().contiguous().to(dev) if seed is not None else None
    d = uh._conv_desc((wp, dy, dx, inv), planes, fmt, p0, p1, H, W, fb, fs, ft, out=fenced["out"].t if "out" in fenced else None,
                      out_h=oH, out_w=oW, stride=stride, oy=oy, ox=ox, pooled=fenced["pool"].t if "pool" in fenced else None,
                      head=(keep[-2], keep[-1], fenced["head"].t) if head is not None else None,
                      raw=fenced["raw"].t if raw else None, seed=sd)
    got = lib.tip_unet_conv_flavour(ctypes.byref(d))
    assert got == flavour, "the dispatcher picks flavour %d %s, the test means %d %s" % (got, FLAVOURS.get(got), flavour, FLAVOURS[flavour])
    if fmt:
        _lib.check(lib.tip_unet_range_reset(stream))
    _lib.check(lib.tip_unet_conv_dev(ctypes.byref(d), stream))
    res = {}
    if fmt:
        flags = ctypes.c_int(-1)
        _lib.check(lib.tip_unet_range_read(stream, ctypes.byref(flags)))
        res["status"] = flags.value
    torch.cuda.synchronize()
    what = "%s flavour %d, %d taps, %d+%d->%d" % (mode, flavour, len(dy), a0.shape[2], a1.shape[2] if a1 is not None else 0, cout)
    for name, f in fenced.items():
        f.check("%s, %s" % (what, name), (oy, ox, stride) if stride > 1 and name in ("out", "raw") else None)
        res[name] = f.t.cpu()
    return res


def head_dev(mode, stored, hw, hb, logits):
    """tip_unet_head_dev on stored planes (planes, H, W, 128) (host) -> float32 (2, H, W) on the host, fenced like run_layer's outputs"""
    import torch
    from tissue_image_processing_amd import _lib
    planes, fmt = MODES[mode]
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    H, W = stored.shape[1:3]
    src = stored.contiguous().to(dev)
    w, b = (hw.float() / (ACT if fmt else 1.0)).contiguous().to(dev), hb.float().to(dev)
    out = Fenced((2, H, W), torch.float32, dev)
    _lib.check(lib.tip_unet_head_dev(src.data_ptr(), H * W, w.data_ptr(), b.data_ptr(), out.t.data_ptr(), planes, fmt, logits, stream))
    torch.cuda.synchronize()
    out.check("%s tip_unet_head_dev" % mode)
    return out.t.cpu()


def reference(a0, a1, taps, dy, dx, bias=None, scale=None, shift=None, seed=None, head=None):
    """The same stencil in float64 on the unsplit values, on the input grid: "sum" = seed + sum over taps of the shifted, zero-padded
    input times the tap's (Cin, Cout) matrix; "out" = sum + bias [-> ReLU -> scale, shift]; "pool" = MaxPool2D(2) of out; with head =
    (weights (2, Cout), bias (2,)): "logits" and "head" (softmax), both (2, H, W)."""
    import torch
    x = (a0 if a1 is None else torch.cat([a0, a1], 2)).double()
    H, W, cin = x.shape
    xp = torch.zeros((H + 2, W + 2, cin), dtype=torch.float64)
    xp[1:-1, 1:-1] = x
    s = torch.zeros((H, W, taps.shape[2]), dtype=torch.float64) if seed is None else seed.double().clone()
    for t in range(taps.shape[0]):
        win = xp[1 + dy[t]:1 + dy[t] + H, 1 + dx[t]:1 + dx[t] + W]
        s += (win.reshape(H * W, cin) @ taps[t].double()).view(H, W, -1)
    r = {"sum": s}
    if bias is not None:
        o = s + bias.double()
        if scale is not None:
            o = torch.relu(o) * scale.double() + shift.double()
        r["out"] = o
        r["pool"] = torch.nn.functional.max_pool2d(o.permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0)
        if head is not None:
            z = (o @ head[0].double().t() + head[1].double()).permute(2, 0, 1)
            r["logits"], r["head"] = z, torch.softmax(z, 0)
    return r


# ---- the cases of the one-launch tests (test_gpu_unet_flavours.py has the argument for the two kinds of data) -----------------------

REGIONS = ["all", "interior", "first row", "last row", "first column", "last column", "top-left corner", "top-right corner",
           "bottom-left corner", "bottom-right corner"]


@functools.lru_cache(maxsize=None)
def exact_case(ntaps, c0, c1, cout=256, h=32, w=64):
    """exact data of one case and its float64 results (shared by the tests; never modified)"""
    import torch
    g = torch.Generator().manual_seed(1000 * ntaps + c0 + 7 * c1 + cout + h * w)
    dy, dx = tap_offsets(ntaps)
    a0 = torch.randint(0, 64, (h, w, c0), generator=g).float() / 16
    a1 = torch.randint(0, 64, (h, w, c1), generator=g).float() / 16 if c1 else None
    taps = 2.0 ** -torch.randint(0, 4, (ntaps, c0 + c1, cout), generator=g).float() * (torch.randint(0, 2, (ntaps, c0 + c1, cout), generator=g).float() * 2 - 1)
    bias = torch.randint(-64, 64, (cout,), generator=g).float() / 16
    scale = 2.0 ** torch.randint(-1, 2, (cout,), generator=g).float()
    shift = torch.randint(-64, 64, (cout,), generator=g).float() / 16
    seed = torch.randint(-1024, 1024, (h, w, cout), generator=g).float() / 128
    ref = reference(a0, a1, taps, dy, dx, bias, scale, shift)
    seeded = reference(a0, a1, taps, dy, dx, seed=seed)["sum"]
    # the construction: every sum, seeded or not, is a float32 (a multiple of 2^-7 below 2^9 + 8), and so is the BatchNorm output
    for t in (ref["sum"], seeded, ref["out"]):
        assert torch.equal(t.float().double(), t)
    assert float(ref["sum"].abs().max()) < 512 and float(ref["out"].abs().max()) < 2048
    return dict(a0=a0, a1=a1, taps=taps, dy=dy, dx=dx, bias=bias, scale=scale, shift=shift, seed=seed, ref=ref, seeded=seeded)


@functools.lru_cache(maxsize=None)
def random_case(ntaps, c0, c1, cout=256, h=32, w=64):
    """randn data of one case, as test_gpu_unet_conv.py::test_single_layers_against_float64 draws it, and its float64 results"""
    import torch
    g = torch.Generator().manual_seed(2000 * ntaps + c0 + 7 * c1 + cout + h * w)
    dy, dx = tap_offsets(ntaps)
    a0 = torch.randn((h, w, c0), generator=g)
    a1 = torch.randn((h, w, c1), generator=g) if c1 else None
    taps = torch.randn((ntaps, c0 + c1, cout), generator=g) * 0.1
    bias, scale, shift = torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    hw, hb = torch.randn((2, cout), generator=g) * 0.05, torch.randn(2, generator=g) * 0.1
    ref = reference(a0, a1, taps, dy, dx, bias, scale, shift, head=(hw, hb) if cout == 128 else None)
    return dict(a0=a0, a1=a1, taps=taps, dy=dy, dx=dx, bias=bias, scale=scale, shift=shift, hw=hw, hb=hb, ref=ref,
                ref_bias=ref["sum"] + bias.double())


def run_case(mode, code, c, **kw):
    """run_layer on a case of exact_case / random_case"""
    return run_layer(mode, c["a0"], c["a1"], c["taps"], c["dy"], c["dx"], code, **kw)


def bits(t):
    import torch
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
