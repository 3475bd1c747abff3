"""Driver of the hand-written U-Net kernels (csrc/tip_unet_conv.h, tip_unet_first.h, tip_unet_planes.h; launchers in
csrc/tip_unet.hip) for prediction_local._UNet: the arithmetic modes, the C-ABI's convolution descriptor, the splitting and packing of the weights (cached per mode on the network), the
one-pass-at-a-time gate, the fp16 range guard and the launch sequence of a forward pass.  The network's parameters, the decision whether an input takes
this path and the torch / MIOpen restatement of the same layers stay in prediction_local."""
import ctypes
import os
import threading
import warnings

import numpy as np

from . import _lib

_MODES = {  # mode -> (pieces per value, piece format of the C-ABI: 0 bf16, 1 fp16, products per term, dropped part of a term)
    "f16x3": (2, 1, 3, "7.2e-7"),
    "bf16x3": (2, 0, 3, "1.6e-5"),
    "bf16x6": (3, 0, 6, "9e-8"),
}
_F16_ACT_SCALE = 16.0      # fp16 pieces: activations are stored times 2^4 (saturate beyond |v| = 4094, absolute floor 2^-29)
_RANGE_F16 = 1             # TIP_UNET_RANGE_F16: bit 0 of the thread's status word
_RANGE_POLICIES = ("fallback", "raise", "off")
_RANGE_FALLBACK_MODE = "bf16x6"      # float32's exponent range at float32-equivalent precision
CONV_ROWS8_K32 = 1         # TIP_UNET_CONV_ROWS8_K32: flag of tip_unet_conv_ex_dev and its two queries


def conv_flags(mode):
    """The per-call flags a forward pass in `mode` hands tip_unet_conv_ex_dev.  Mode f16x3 runs its 8-row launches of four and more
    taps (the 128-channel 3x3 layers) on the K = 32 kernel; TISSUE_HIP_UNET_ROWS8_K32=0 restores the 32x32x16 launches.
    Read per pass and handed over per call: nothing process-wide changes under the worker threads."""
    return CONV_ROWS8_K32 if mode == "f16x3" and os.environ.get("TISSUE_HIP_UNET_ROWS8_K32", "1") != "0" else 0


class UNetRangeError(_lib.TissueHipError):
    """A forward pass in f16x3 met an activation beyond what its scaled fp16 pieces hold (TISSUE_HIP_UNET_RANGE=raise)."""


def range_policy():
    """TISSUE_HIP_UNET_RANGE: what a forward pass in f16x3 does about activations beyond fp16's range (the kernels clamp them; the
    bf16 modes have float32's exponent range and are never guarded):
    'fallback' (default): the pass is rerun in bf16x6, and the network object stays there (_UNet.range_exceeded, reset_range());
    'raise': UNetRangeError;
    'off': no check -- no reset, no read, no wait on the stream: the clamped result is returned."""
    v = os.environ.get("TISSUE_HIP_UNET_RANGE", "fallback")
    if v not in _RANGE_POLICIES:
        raise ValueError("TISSUE_HIP_UNET_RANGE must be fallback, raise or off")
    return v


class _ConvDesc(ctypes.Structure):
    """tip_unet_conv_desc of include/tissue_hip.h."""
    _fields_ = [("in0", ctypes.c_void_p), ("in1", ctypes.c_void_p), ("c0", ctypes.c_int), ("c1", ctypes.c_int), ("h", ctypes.c_int),
                ("w", ctypes.c_int), ("planes", ctypes.c_int), ("weights", ctypes.c_void_p), ("ntaps", ctypes.c_int),
                ("dy", ctypes.c_int * 9), ("dx", ctypes.c_int * 9), ("cout", ctypes.c_int), ("bias", ctypes.c_void_p),
                ("scale", ctypes.c_void_p), ("shift", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_h", ctypes.c_int),
                ("out_w", ctypes.c_int), ("sy", ctypes.c_int), ("sx", ctypes.c_int), ("oy", ctypes.c_int), ("ox", ctypes.c_int),
                ("pool_out", ctypes.c_void_p), ("head_w", ctypes.c_void_p), ("head_b", ctypes.c_void_p), ("head_out", ctypes.c_void_p),
                ("format", ctypes.c_int), ("acc_scale", ctypes.c_float), ("raw_out", ctypes.c_void_p), ("seed", ctypes.c_void_p)]


def split_pack(taps, planes, fmt=0):
    """taps: (T, Cin, Cout) float32 on the device -> packed split weights [T][Cin/16][Cout/128][plane][128][16] in bf16 (fmt 0) or
    fp16 (fmt 1: the caller has scaled the taps into fp16's range) pieces.

    Row order inside every group of 32 output channels: row 8 g + 4 h + j (g < 4, h < 2, j < 4) holds channel 16 h + 4 g + j --
    the matrix core's output register i = 4 g + j of half-wave h is then channel 16 h + i, i.e. a lane of the kernel ends up with
    sixteen ADJACENT channels of its pixel (csrc/tip_unet_conv.h, epilogue)."""
    import torch
    T, cin, cout = taps.shape
    pieces, rest = [], taps.float()
    for _ in range(planes):
        h = rest.to(torch.float16 if fmt else torch.bfloat16)
        pieces.append(h)
        rest = rest - h.float()
    row = torch.arange(32, device=taps.device)
    chan = 16 * ((row >> 2) & 1) + 4 * (row >> 3) + (row & 3)          # channel (within its group of 32) stored in each row
    pk = torch.stack(pieces, 0).view(planes, T, cin // 16, 16, cout // 32, 32)[..., chan]
    pk = pk.reshape(planes, T, cin // 16, 16, cout // 128, 128)
    return pk.permute(1, 2, 4, 0, 5, 3).contiguous()


_COMPOSE_LEVELS = (0, 1, 2)      # decoder levels whose transposed convolution is folded into the next convolution by default


def compose_levels():
    """TISSUE_HIP_UNET_COMPOSE: unset or 1 = the default levels, 0 = none (a transposed convolution's four parity launches and the
    convolution over [up-sampled, skip], as before), or a list of levels such as u0,u2 (measurements)."""
    v = os.environ.get("TISSUE_HIP_UNET_COMPOSE", "1").strip()
    if v == "0":
        return ()
    if v in ("", "1"):
        return _COMPOSE_LEVELS
    return tuple(sorted({int(t.strip().lstrip("u")) for t in v.split(",") if t.strip()} & {0, 1, 2}))


# Conv2DTranspose(3x3, stride 2, cropped to 2N) followed by Conv2D(3x3) along one axis, with T[k] / Wu[k] the two layers' taps:
#     up[2i] = x[i] T0 + x[i-1] T2,  up[2i+1] = x[i] T1,  out[Y] = sum_k Wu[k] up[Y + k - 1]
# so out[2i + parity] = sum over the pairs below of x[i + offset] T[kt] Wu[kw]:  parity -> [(offset, kw, kt)]
_COMPOSE_AXIS = {0: [(-1, 0, 1), (-1, 1, 2), (0, 1, 0), (0, 2, 1)],
                 1: [(-1, 0, 2), (0, 0, 0), (0, 1, 1), (0, 2, 2), (1, 2, 0)]}
_EDGE_TAPS = [(0, -1), (0, 0), (1, -1), (1, 0), (1, 1)]      # (parity, offset) order of the border pass's weight tables


def compose(tw, bt, w1):
    """The algebra of DESIGN 5.7 in float64.  tw: (2C, C, 3, 3) transposed-convolution weights (torch layout: in, out, ky, kx), bt:
    its bias (C), w1: (Cout, C + Cskip, 3, 3) weights of the convolution that follows (its first C input channels read the
    up-sampled tensor).  Returns
      classes  {(py, px): (taps (T, 2C, Cout), dy list, dx list)}: the composed convolution on the LOW-resolution grid per output parity,
      bias     (Cout) what the transposed convolution's bias adds to an interior pixel of the convolution,
      bias_tab (3, 3, Cout) an edge pixel's bias sum minus the interior's: (top, inside, bottom) x (left, inside, right),
      row_w, col_w (5, 2C, Cout), corner_w (2C, Cout): what the border pass ADDS on the last output row / column / corner pixel
      (taps in _EDGE_TAPS order) to take out the terms through the cropped row / column up[2N] = x[N-1] T2."""
    import torch
    tw, bt, w1 = tw.double(), bt.double().reshape(-1), w1.double()
    C = tw.shape[1]
    wu = w1[:, :C].permute(2, 3, 1, 0)             # [ky][kx] -> (C, Cout)
    t = tw.permute(2, 3, 0, 1)                     # [ky][kx] -> (2C, C)
    prod = {}

    def pair(kty, ktx, kwy, kwx):
        k = (kty, ktx, kwy, kwx)
        if k not in prod:
            prod[k] = t[kty, ktx] @ wu[kwy, kwx]
        return prod[k]

    classes = {}
    for py in (0, 1):
        for px in (0, 1):
            acc = {}
            for dy, kwy, kty in _COMPOSE_AXIS[py]:
                for dx, kwx, ktx in _COMPOSE_AXIS[px]:
                    m = pair(kty, ktx, kwy, kwx)
                    acc[(dy, dx)] = acc[(dy, dx)] + m if (dy, dx) in acc else m
            offs = sorted(acc)
            classes[(py, px)] = (torch.stack([acc[o] for o in offs], 0), [o[0] for o in offs], [o[1] for o in offs])
    through = torch.einsum("yxco,c->yxo", wu, bt)   # the bias through every tap of the convolution
    bias = through.sum((0, 1))
    bias_tab = torch.zeros((3, 3, bias.numel()), dtype=torch.float64, device=bias.device)
    for ry in range(3):
        for rx in range(3):
            for ky in range(3):
                for kx in range(3):
                    if (ry == 0 and ky == 0) or (ry == 2 and ky == 2) or (rx == 0 and kx == 0) or (rx == 2 and kx == 2):
                        bias_tab[ry, rx] -= through[ky, kx]      # the tap reads outside the up-sampled image
    zero = torch.zeros_like(pair(2, 2, 2, 2))
    row_w, col_w = [], []
    for par, off in _EDGE_TAPS:
        # last output row (parity 1): the pair (Wu2, T2) at offset 0 along y, with every pair along x -- and the same along the column
        row_w.append(-sum((pair(2, ktx, 2, kwx) for dx, kwx, ktx in _COMPOSE_AXIS[par] if dx == off), zero))
        col_w.append(-sum((pair(kty, 2, kwy, 2) for dy, kwy, kty in _COMPOSE_AXIS[par] if dy == off), zero))
    return classes, bias, bias_tab, torch.stack(row_w, 0), torch.stack(col_w, 0), pair(2, 2, 2, 2)


def _pack(taps, planes, fmt, bias_only=False):
    """split_pack with the fp16 pieces' per-layer power-of-two weight scale -> (packed weights, accumulator factor)"""
    if not fmt:
        return split_pack(taps, planes), 1.0
    big = float(taps.abs().max())
    wscale = 2.0 ** (14 - int(np.floor(np.log2(big)))) if big > 0 and np.isfinite(big) else 1.0
    inv = 1.0 / (_F16_ACT_SCALE * wscale)
    return split_pack(taps * wscale, planes, fmt), (inv * _F16_ACT_SCALE if bias_only else inv)


def compose_layers(tw, bt, w1, b1, planes, fmt):
    """A transposed convolution (tw, bt) folded into the convolution (w1, b1) behind it, ready to launch: the four composed
    stencils on the low-resolution grid ("x00" .. "x11": raw float32 output, so their accumulator factor yields the layer's true
    units), the convolution's skip half ("skip"), its bias with the transposed convolution's folded in ("bias") and the border
    pass's float32 tables ("border").  Neither the transposed convolution nor the up half is packed."""
    import torch
    w1 = w1.float()
    C = tw.shape[1]
    classes, bias, bias_tab, row_w, col_w, corner_w = compose(tw, bt, w1)
    st = {}
    for (py, px), (taps, dy, dx) in classes.items():
        wp, inv = _pack(taps.float(), planes, fmt)
        st["x%d%d" % (py, px)] = (wp, dy, dx, inv)
    skip = torch.stack([w1[:, C:, ky, kx].t() for ky in range(3) for kx in range(3)], 0)
    wp, inv = _pack(skip, planes, fmt)
    st["skip"] = (wp, [ky - 1 for ky in range(3) for kx in range(3)], [kx - 1 for ky in range(3) for kx in range(3)], inv)
    st["bias"] = (b1.double().reshape(-1) + bias).float().contiguous()
    st["border"] = tuple(v.float().contiguous() for v in (row_w, col_w, corner_w, bias_tab))
    return st


def composed_up(st, planes, fmt, src, h, w, stream, name="", launch=None, flags=0):
    """The launches of compose_layers' `st` over the split low-resolution tensor src (planes, h, w, cin): four composed stencils leave
    the next convolution's sum over its up-sampled half as float32 (2h, 2w, cout), the border pass corrects its edges.  That
    convolution then runs over the skip tensor alone with st["bias"] and seed = the returned tensor.  launch(name, flop, fn): the
    caller's per-launch timing hook; flags: tip_unet_conv_ex_dev's, for the four stencils."""
    import torch
    lib = _lib.lib()
    launch = launch or (lambda name, flop, fn: fn())
    cin, cout = src.shape[3], st["x00"][0].shape[2] * 128
    part = torch.empty((2 * h, 2 * w, cout), dtype=torch.float32, device=src.device)
    for py in (0, 1):
        for px in (0, 1):
            layer = st["x%d%d" % (py, px)]
            d = _conv_desc(layer, planes, fmt, src, None, h, w, None, raw=part, out_h=2 * h, out_w=2 * w, stride=2, oy=py, ox=px)
            launch("%sx.%d%d %dx%d %d+0->%d x%d taps" % (name, py, px, h, w, cin, cout, d.ntaps), 2.0 * h * w * d.ntaps * cout * cin,
                   lambda: _lib.check(lib.tip_unet_conv_ex_dev(ctypes.byref(d), flags, stream)))
    row_w, col_w, corner_w, bias_tab = st["border"]
    launch("%sborder %dx%d %d->%d" % (name, 2 * h, 2 * w, cin, cout), 2.0 * 2.5 * (h + w) * cin * cout,
           lambda: _lib.check(lib.tip_unet_compose_border_dev(src.data_ptr(), planes, fmt, h, w, cin, cout, row_w.data_ptr(),
                                                              col_w.data_ptr(), corner_w.data_ptr(), bias_tab.data_ptr(),
                                                              part.data_ptr(), 1.0 / _F16_ACT_SCALE if fmt else 1.0, stream)))
    return part


def weights(net, mode, levels=None):
    """Packed weights and per-channel constants of one arithmetic mode, cached in net._hipw.  fp16 pieces (mode f16x3) carry
    power-of-two scales: activations are stored times A = 2^4, a layer's weights times W = the power of two that puts its largest
    weight in [2^14, 2^15); the kernel multiplies the accumulator by 1 / (A W) before the bias (entry 3 of a layer's tuple), the
    BatchNorm scale / shift (and a bias-only layer's bias and accumulator factor) are multiplied by A, the head's weights by
    1 / A -- exact, so the stored values are A times what the unscaled network computes, bit for bit."""
    levels = compose_levels() if levels is None else tuple(levels)
    hw = net._hipw.get((mode, levels))
    if hw is not None:
        return hw
    torch = net.torch
    p = net.p
    planes, fmt = _MODES[mode][:2]
    act = _F16_ACT_SCALE if fmt else 1.0
    hw = {}

    def pack(taps, bias_only):
        return _pack(taps, planes, fmt, bias_only)

    def conv3(name):
        w = p[name + ".w"].float()                                  # (cout, cin, 3, 3): cross-correlation, tap (ky, kx) reads (y + ky - 1, x + kx - 1)
        taps = torch.stack([w[:, :, ky, kx].t() for ky in range(3) for kx in range(3)], 0)
        wp, inv = pack(taps, False)
        hw[name] = (wp, [ky - 1 for ky in range(3) for kx in range(3)], [kx - 1 for ky in range(3) for kx in range(3)], inv)

    def conv_t(name):
        # conv_transpose2d(stride 2): out[2 i + k] += in[i] w[k], cropped to the first 2N rows / columns.  Even outputs take
        # k = 0 from i = o / 2 and k = 2 from i = o / 2 - 1, odd outputs k = 1 from i = (o - 1) / 2: four parity classes
        w = p[name + ".w"].float()                                  # (cin, cout, 3, 3)
        per_axis = {0: [(0, 0), (2, -1)], 1: [(1, 0)]}             # parity -> [(k, input offset)]
        for py in (0, 1):
            for px in (0, 1):
                tl = [(ky, dy, kx, dx) for ky, dy in per_axis[py] for kx, dx in per_axis[px]]
                taps = torch.stack([w[:, :, ky, kx] for ky, _, kx, _ in tl], 0)
                wp, inv = pack(taps, True)
                hw["%s.%d%d" % (name, py, px)] = (wp, [t[1] for t in tl], [t[3] for t in tl], inv)

    for blk in ("d0", "d1", "d2", "mid", "u0", "u1", "u2"):
        if blk != "d0" and not (blk[0] == "u" and int(blk[1]) in levels):
            conv3(blk + ".c1")
        conv3(blk + ".c2")
    for i in range(3):
        if i in levels:        # folded into the level's first convolution
            hw["u%d.x" % i] = compose_layers(p["u%d.t.w" % i], p["u%d.t.b" % i], p["u%d.c1.w" % i], p["u%d.c1.b" % i], planes, fmt)
        else:
            conv_t("u%d.t" % i)
    w0 = p["d0.c1.w"].float()                                       # (128, 2, 3, 3) -> [tap][ci][cout]
    hw["first"] = w0.permute(2, 3, 1, 0).reshape(18, 128).contiguous()
    if fmt:
        # the same layer for the matrix cores (k_unet_conv_first_mfma): one tap x 32 input channels, rows k = 2 tap + channel < 18
        # are the layer's terms in hw["first"]'s order, the rest zeros -> (packed weights, accumulator factor)
        rows = torch.zeros((1, 32, 128), dtype=torch.float32, device=w0.device)
        rows[0, :18] = hw["first"]
        hw["first.packed"] = pack(rows, False)
    hw["head"] = (p["head.w"].float().reshape(2, 128) / act).contiguous()
    for k in list(p):
        if k.endswith((".b", ".s", ".t")) and not k.endswith(".t.w"):
            v = p[k].float().reshape(-1)
            # times A: BatchNorm scale (".s") / shift (".t"), and the bias of a bias-only (transposed convolution) layer (".t.b")
            scaled = k.endswith((".s", ".t", ".t.b"))
            hw["f:" + k] = (v * act if scaled else v).contiguous()
    net._hipw[(mode, levels)] = hw
    return hw


_FORWARD_GATES = {}
_FORWARD_GATES_LOCK = threading.Lock()


def _forward_gate(device_index):
    with _FORWARD_GATES_LOCK:
        g = _FORWARD_GATES.get(device_index)
        if g is None:
            g = _FORWARD_GATES[device_index] = {"lock": threading.Lock(), "event": None, "stream": None}
        return g


def forward(net, x, mode, logits):
    """A forward pass in `mode` under the range policy.  Only f16x3 is guarded: the thread's status word is zeroed on the pass's
    stream in front of its first launch (inside the gate: the order of the launches is the gate's), and read behind its last --
    the host waits for this stream alone and OUTSIDE the gate, so that a thread waiting for its own pass holds up nobody's ticket.
    A set bit means some layer's output was clamped and the result is not the network's: `raise` says so, `fallback` runs the
    same pass again in bf16x6 and keeps the network object there (no f16x3 attempt and no warning from then on)."""
    policy = range_policy() if mode == "f16x3" else "off"
    if policy == "fallback" and getattr(net, "range_exceeded", False):
        return _gated(net, x, _RANGE_FALLBACK_MODE, logits)
    out = _gated(net, x, mode, logits, guard=policy != "off")
    if policy == "off":
        return out
    flags = ctypes.c_int(0)
    _lib.check(_lib.lib().tip_unet_range_read(net.torch.cuda.current_stream(x.device).cuda_stream, ctypes.byref(flags)))
    if not flags.value & _RANGE_F16:
        return out
    limit = int(65504 / _F16_ACT_SCALE)
    if policy == "raise":
        raise UNetRangeError("the U-Net's activations leave the range of mode f16x3 (|v| <= %d: fp16 pieces of 16 v), the result would be "
                             "clamped; set TISSUE_HIP_UNET_ARITH=bf16x6 or TISSUE_HIP_UNET_RANGE=fallback" % limit)
    del out
    net.range_exceeded = True
    if not getattr(net, "_range_warned", False):
        net._range_warned = True
        warnings.warn("this U-Net checkpoint's activations leave fp16's range (|v| <= %d in mode f16x3): its forward passes now run in "
                      "%s, at about twice the matrix work" % (limit, _RANGE_FALLBACK_MODE), RuntimeWarning, stacklevel=3)
    return _gated(net, x, _RANGE_FALLBACK_MODE, logits)


def _gated(net, x, mode, logits, guard=False):
    """One network at a time on a device.  Frames in flight (worker threads, each with its own stream: movie.py, bench.py) would
    otherwise run their forward passes CONCURRENTLY -- the queues share the chip kernel by kernel, every pass takes N times as
    long, all of them end together and the frames' tails (small kernels, host stages) then run together with nothing to
    hide behind: the kernel trace shows the matrix cores idle for 8.5 % of the time (profiles/r04n_*).  Here a pass waits ON THE
    DEVICE (stream.wait_event, no host stall) for the pass queued before it, so that the passes run back to back in ticket order
    and the other frames' tails and projections fill in beside them.  TISSUE_HIP_UNET_SERIAL=0 restores the free-for-all.
    guard: the range word of this thread is zeroed on the stream in front of the pass (forward() reads it afterwards)."""
    torch = net.torch

    def run():
        if guard:
            _lib.check(_lib.lib().tip_unet_range_reset(torch.cuda.current_stream(x.device).cuda_stream))
        return _launch(net, x, mode, logits)

    if os.environ.get("TISSUE_HIP_UNET_SERIAL", "1") == "0":
        return run()
    gate = _forward_gate(x.device.index)
    with gate["lock"]:
        s = torch.cuda.current_stream(x.device)
        if gate["event"] is not None and gate["stream"] != s.cuda_stream:
            s.wait_event(gate["event"])
        out = run()
        ev = torch.cuda.Event()
        ev.record(s)
        gate["event"], gate["stream"] = ev, s.cuda_stream
    return out


def _conv_desc(layer, planes, fmt, src, skip, h, w, bias, scale=None, shift=None, out=None, out_h=None, out_w=None, stride=1, oy=0, ox=0,
               pooled=None, head=None, raw=None, seed=None):
    """The descriptor of one tip_unet_conv_dev launch.  layer: (packed weights, dy, dx, accumulator factor) from weights(); src,
    skip: split activations on the h x w grid (skip's channels are appended to src's: the decoder's concatenate); bias, scale,
    shift: float32 vectors (no scale / shift: a bias-only layer); out: split output of out_h x out_w pixels (default: the input
    grid), input-grid pixel (y, x) goes to (y * stride + oy, x * stride + ox); pooled: MaxPool2D(2) of the output; head: (weights,
    bias, float32 output) of the network's head computed in this layer's epilogue -- the layer's own output is then not stored;
    raw: float32 (out_h, out_w, cout) that receives the bare sum through the output mapping instead of everything else (no bias
    needed); seed: float32 (h, w, cout) added to the layer's pre-bias sum."""
    wp, dy, dx, inv = layer
    d = _ConvDesc()
    d.format, d.acc_scale = fmt, inv
    d.in0, d.c0 = src.data_ptr(), src.shape[3]
    d.in1, d.c1 = (skip.data_ptr(), skip.shape[3]) if skip is not None else (None, 0)
    d.h, d.w, d.planes = h, w, planes
    d.weights, d.ntaps, d.cout = wp.data_ptr(), len(dy), wp.shape[2] * 128
    for i in range(len(dy)):
        d.dy[i], d.dx[i] = dy[i], dx[i]
    d.bias = bias.data_ptr() if bias is not None else None
    d.raw_out = raw.data_ptr() if raw is not None else None
    d.seed = seed.data_ptr() if seed is not None else None
    d.scale, d.shift = (scale.data_ptr(), shift.data_ptr()) if scale is not None else (None, None)
    if head is not None:
        d.head_w, d.head_b, d.head_out = (t.data_ptr() for t in head)
    d.out = out.data_ptr() if out is not None else None
    d.out_h, d.out_w = (h, w) if out_h is None else (out_h, out_w)
    d.sy, d.sx, d.oy, d.ox = stride, stride, oy, ox
    d.pool_out = pooled.data_ptr() if pooled is not None else None
    return d


def _launch(net, x, mode, logits):
    """The forward pass on torch's current stream: (1, 2, H, W) float32 -> class probabilities (or logits) (1, 2, H, W)."""
    torch = net.torch
    planes, fmt = _MODES[mode][:2]
    levels = compose_levels()
    hw = weights(net, mode, levels)
    net.last_mode = mode                  # (bench.py / tests: which arithmetic the last forward pass really used)
    net.last_compose = tuple("u%d" % i for i in levels)      # ... and which decoder levels ran composed (empty: none)
    lib = _lib.lib()
    flags = conv_flags(mode)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    H, W = int(x.shape[2]), int(x.shape[3])
    x = x.to(torch.float32).contiguous()
    trace = getattr(net, "trace", None)       # tools/unet_layers.py: [(layer, flop, event, event)] per launch

    def timed(name, flop, fn):
        if trace is None:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        trace.append((name, flop, e0, e1))
        return r

    def buf(h, w, c):
        return torch.empty((planes, h, w, c), dtype=torch.float16 if fmt else torch.bfloat16, device=x.device)

    def launch_conv(name, d):
        timed("%s %dx%d %d+%d->%d x%d taps" % (name, d.h, d.w, d.c0, d.c1, d.cout, d.ntaps), 2.0 * d.h * d.w * d.ntaps * d.cout * (d.c0 + d.c1),
              lambda: _lib.check(lib.tip_unet_conv_ex_dev(ctypes.byref(d), flags, stream)))

    def conv3(name, bn, src, skip, h, w, pooled=None, head=None, seed=None):
        """Conv2D(3x3) -> ReLU -> BatchNormalization `bn`; head: the probabilities' tensor when the head rides in the epilogue;
        seed: the layer's partial sum over the up-sampled half (composed level) -- src is then the skip tensor alone"""
        layer, bias = (hw[name], hw["f:" + name + ".b"]) if seed is None else (hw[name[:2] + ".x"]["skip"], hw[name[:2] + ".x"]["bias"])
        out = buf(h, w, layer[0].shape[2] * 128) if head is None else None
        launch_conv(name if seed is None else name + ".seeded",
                    _conv_desc(layer, planes, fmt, src, skip, h, w, bias, hw["f:" + bn + ".s"], hw["f:" + bn + ".t"],
                               out=out, pooled=pooled, head=None if head is None else (hw["head"], hw["f:head.b"], head), seed=seed))
        return out

    def first(h, w):
        """Conv2D(2 -> 128, 3x3) -> ReLU -> BatchNormalization on the float32 network input"""
        out = buf(h, w, 128)
        if fmt == 1 and lib.tip_unet_first_mfma():       # fp16 pieces: on the matrix cores unless TIP_UNET_FIRST=valu
            wp, inv = hw["first.packed"]
            timed("first %dx%d 2->128" % (h, w), 2.0 * h * w * 18 * 128,
                  lambda: _lib.check(lib.tip_unet_conv_first_packed_dev(x.data_ptr(), h, w, wp.data_ptr(), inv, hw["f:d0.c1.b"].data_ptr(),
                                                                        hw["f:d0.b1.s"].data_ptr(), hw["f:d0.b1.t"].data_ptr(),
                                                                        out.data_ptr(), stream)))
            return out
        timed("first %dx%d 2->128" % (h, w), 2.0 * h * w * 18 * 128,
              lambda: _lib.check(lib.tip_unet_conv_first_dev(x.data_ptr(), h, w, hw["first"].data_ptr(), hw["f:d0.c1.b"].data_ptr(),
                                                             hw["f:d0.b1.s"].data_ptr(), hw["f:d0.b1.t"].data_ptr(), out.data_ptr(),
                                                             planes, fmt, stream)))
        return out

    def double(blk, src, skip, h, w, pooled=None, head=None, seed=None):
        """a block's two convolutions; src None: the block reads the float32 network input (first-layer kernel)"""
        a = first(h, w) if src is None else conv3(blk + ".c1", blk + ".b1", src, skip, h, w, seed=seed)
        return conv3(blk + ".c2", blk + ".b2", a, None, h, w, pooled=pooled, head=head)

    def conv_t(name, src, h, w):
        """Conv2DTranspose(3x3, stride 2): one launch per output parity class, into one 2h x 2w tensor"""
        up = buf(2 * h, 2 * w, hw[name + ".00"][0].shape[2] * 128)
        for py in (0, 1):
            for px in (0, 1):
                cls = "%s.%d%d" % (name, py, px)
                launch_conv(cls, _conv_desc(hw[cls], planes, fmt, src, None, h, w, hw["f:" + name + ".b"], out=up, out_h=2 * h, out_w=2 * w,
                                            stride=2, oy=py, ox=px))
        return up

    with torch.no_grad():
        skips, cur, h, w = [], None, H, W
        for i in range(3):                    # encoder: MaxPool2D(2) comes out of the second convolution's epilogue
            pooled = buf(h // 2, w // 2, net.filters[i])
            skips.append(double("d%d" % i, cur, None, h, w, pooled=pooled))
            cur, h, w = pooled, h // 2, w // 2
        cur = double("mid", cur, None, h, w)  # bottleneck
        for i in range(3):                    # decoder: the convolution reads [up-sampled, skip] as one concatenated tensor
            part = composed_up(hw["u%d.x" % i], planes, fmt, cur, h, w, stream, "u%d." % i, timed, flags) if i in levels else None
            up = conv_t("u%d.t" % i, cur, h, w) if part is None else None
            h, w = 2 * h, 2 * w
            # the last convolution's epilogue computes the head: softmax probabilities instead of the layer's own output
            probs = None
            if i == 2 and not logits and not os.environ.get("TISSUE_HIP_UNET_SEPARATE_HEAD"):
                probs = torch.empty((1, 2, H, W), dtype=torch.float32, device=x.device)
            if part is None:
                cur = double("u%d" % i, up, skips[2 - i], h, w, head=probs)
            else:
                cur = double("u%d" % i, skips[2 - i], None, h, w, head=probs, seed=part)
        if probs is not None:
            return probs
        out = torch.empty((1, 2, H, W), dtype=torch.float32, device=x.device)
        timed("head %dx%d" % (H, W), 2.0 * H * W * 256,
              lambda: _lib.check(lib.tip_unet_head_dev(cur.data_ptr(), H * W, hw["head"].data_ptr(), hw["f:head.b"].data_ptr(),
                                                       out.data_ptr(), planes, fmt, 1 if logits else 0, stream)))
    return out
