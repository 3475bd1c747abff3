"""Drop-in for Segmentation/prediction_local.py (pl.py) on MI355X.

    find_desired_shape, normalize_channel                      pl.py:10-29
    build_unet_model / SegmentationPredictor                   pl.py:31-198

The network (_UNet) runs on the hand-written HIP kernels of libtissue_hip.so (csrc/tip_unet_conv.h: implicit-GEMM convolutions
on the 16-bit matrix cores with split float32 operands; driven by _unet_hip.py) for the reference's widths in float32 on extents
that are multiples of 64 x 256, and otherwise -- or with TISSUE_HIP_UNET_ARITH=miopen -- as the torch expressions of the same
layers (PyTorch-ROCm / MIOpen convolutions, the bias -> ReLU -> BatchNorm epilogue in the library).  Image preparation
(percentiles, clip, scale, transpose, pad: pl.py:90-122) and everything after the network (threshold, 5x5 closing, 7x7 erosion,
boundary, watershed: pl.py:167-194) run in libtissue_hip.so on the same resident buffers.

Deliberate deviations from the reference (documented in DESIGN.md):
  * pl.py:96-135 writes nine debug TIFFs to hard-coded C:\\Users\\... paths on every call; not reproduced.
  * the 101-fold closing loop (pl.py:170-174) is applied once: grey closing with a flat footprint is idempotent
    (pinned by tests/golden/rank_filters.npz closed_101 == closed_once).
  * Keras .h5 checkpoints (gui.py:38-39, pl.py:76-88) are read by a self-contained HDF5 reader (_hdf5.py: no h5py /
    TensorFlow in the image); an .npz holding model.get_weights() in layer order is accepted too, and a path of None
    gives random initialisation.  No weights ship with the reference, so the TRAINED network's parity is unpinned.
"""
import ctypes
import os

import numpy as np

from . import _lib, _unet_hip
from ._unet_hip import _ConvDesc, _MODES, UNetRangeError      # (tests and tools reach the descriptor through this module)


def find_desired_shape(shape_y, shape_x):
    """pl.py:10-19: the smallest power of two >= each extent (the network halves the frame three times)."""
    if shape_y < 1 or shape_x < 1:
        raise UnboundLocalError("find_desired_shape: extents must be >= 1")   # what the reference's empty loop ends in
    return 1 << (int(shape_y) - 1).bit_length(), 1 << (int(shape_x) - 1).bit_length()


def normalize_channel(image):
    """pl.py:21-29: clip to the [1st, 99th] percentile and scale to [0, 1].

    The reference writes the two percentiles INTO a copy of the input, so the clip values take the input's dtype: for
    the uint16 planes the GUI hands over (gui.py:2059-2061) they are truncated to integers, for float32 they are rounded
    to float32 (and numpy 1.x, the reference's environment, then keeps the arithmetic in float32); float64 is plain."""
    image = np.asarray(image)
    per99 = np.percentile(image, 99)
    per1 = np.percentile(image, 1)
    kind = image.dtype
    clipped = np.where(image > per99, np.asarray(per99).astype(kind), image)
    clipped = np.where(image < per1, np.asarray(per1).astype(kind), clipped)
    if kind == np.float32:
        return (clipped - np.float32(per1)) / np.float32(per99 - per1)
    return (clipped - per1) / (per99 - per1)


_shared_runtime = {}


def shares_runtime_with_torch(t):
    """True when libtissue_hip.so and torch use ONE HIP runtime for tensor t's device: the library's runtime attributes
    t's storage to t.device.index.  PyTorch wheels bundle their own libamdhip64; with two runtimes in the process torch's
    pointers and stream handles mean nothing to the library, and the fused passes that take them must not be used (the torch
    expressions run instead).  Checked once per device."""
    idx = t.device.index if t.device.index is not None else 0
    ok = _shared_runtime.get(idx)
    if ok is None:
        ok = _lib.load().tip_pointer_device(t.data_ptr()) == idx
        _shared_runtime[idx] = ok
    return ok


def _unet_mode():
    """TISSUE_HIP_UNET_ARITH: how the hand-written implicit-GEMM convolutions feed the 16-bit matrix cores (float32 accumulation):
    'f16x3' (default): float32 operands split into two fp16 pieces of power-of-two-scaled values, three products per term --
        float32-equivalent (<= 3 x 2^-22 of a term is dropped) at three products;
    'bf16x3': two bf16 pieces, three products per term (<= 2^-15.9 of a term dropped: 16 significand bits);
    'bf16x6': three bf16 pieces, six products (float32-equivalent to 2^-23.4; twice the matrix work);
    'miopen': PyTorch-ROCm / MIOpen float32 convolutions."""
    m = os.environ.get("TISSUE_HIP_UNET_ARITH", "f16x3")
    if m not in _MODES and m != "miopen":
        raise ValueError("TISSUE_HIP_UNET_ARITH must be f16x3, bf16x3, bf16x6 or miopen")
    if os.environ.get("TISSUE_HIP_UNET_DTYPE", "fp32") != "fp32":
        m = "miopen"
    return m


def unet_arithmetic():
    """How the network's convolutions are computed in this process (bench.py reports it with the MFMA roofline)."""
    m = _unet_mode()
    if m == "miopen":
        dt = os.environ.get("TISSUE_HIP_UNET_DTYPE", "fp32")
        if dt == "fp32":
            return {"dtype": "f32", "arithmetic": "float32 convolutions through PyTorch-ROCm / MIOpen (fp32 matrix pipe)", "peak_tflops": 157.3}
        return {"dtype": dt, "arithmetic": "%s convolutions through PyTorch-ROCm / MIOpen" % dt, "peak_tflops": 2500.0}
    planes, fmt, prods, err = _MODES[m]
    piece = "fp16" if fmt else "bf16"
    return {"dtype": "f32(%s)" % m, "mode": m, "peak_tflops": 2500.0 / prods, "issued_flops_factor": prods, "issued_peak_tflops": 2500.0,
            "float32_equivalent": m != "bf16x3",
            "arithmetic": "float32 operands split into %d %s pieces, %d %s MFMA products per term (relative error per term <= %s), "
                          "float32 accumulation; hand-written implicit-GEMM kernels (csrc/tip_unet_conv.h); peak = dense 16-bit MFMA "
                          "peak / %d" % (planes, piece, prods, piece, err, prods)}


def unet_algorithmic_bytes(h, w):
    """Compulsory HBM bytes of one forward pass at float32 width (every layer's input read once, its output written once, the
    split weights read once): what `roofline.traffic` of the network's kernels is compared with."""
    total = 0
    c, hh, ww = 2, h, w
    layers = []
    for f in _FILTERS:
        layers += [(hh, ww, c, f), (hh, ww, f, f)]
        c, hh, ww = f, hh // 2, ww // 2
    layers += [(hh, ww, c, 1024), (hh, ww, 1024, 1024)]
    c = 1024
    for f in reversed(_FILTERS):
        total += 4 * (hh * ww * c + 4 * hh * ww * f) + 4 * 9 * c * f          # transposed convolution: in, out (2h x 2w), weights
        hh, ww = hh * 2, ww * 2
        layers += [(hh, ww, 2 * f, f), (hh, ww, f, f)]
        c = f
    for (lh, lw, ci, co) in layers:
        total += 4 * lh * lw * (ci + co) + 4 * 9 * ci * co
    total += 4 * hh * ww * (c + 2)                                            # head
    total += 4 * sum((h >> (i + 1)) * (w >> (i + 1)) * f for i, f in enumerate(_FILTERS))   # pooled maps (written by the conv epilogue)
    return total


_FILTERS = (128, 256, 512)
_BN_EPS = 1e-3  # Keras BatchNormalization default


def _percentile_linear_t(flat_sorted, q):
    """np.percentile(..., q) ('linear') on an ascending torch tensor, numpy's index / lerp arithmetic in float64."""
    n = flat_sorted.numel()
    quant = q / 100.0
    virt = (n - 1) * quant
    prev = int(np.floor(virt))
    gamma = virt - prev
    prev = min(max(prev, 0), n - 1)
    nxt = min(prev + 1, n - 1)
    lo = float(flat_sorted[prev])
    hi = float(flat_sorted[nxt])
    diff = hi - lo
    res = lo + diff * gamma
    if gamma >= 0.5:
        res = hi - diff * (1 - gamma)
    return res


class _UNet(object):
    """3-level U-Net of pl.py:31-72 as explicit torch functional calls (NCHW, channels_last memory format).

    Keras semantics kept: Conv2D(3, 'same') + ReLU THEN BatchNormalization (eps 1e-3, inference statistics);
    MaxPool2D(2); Dropout is identity at inference; Conv2DTranspose(n, 3, 2, 'same') == torch conv_transpose2d
    (stride 2, padding 0) cropped to the first 2N rows/cols (TF pads SAME with pad_before 0 / pad_after 1);
    concatenate([upsampled, skip]); Conv2D(2, 1) + softmax over channels.
    """

    def __init__(self, in_ch=2, device="cuda", dtype=None, weights=None, seed=0, filters=None, bottleneck=None):
        import torch
        self.torch = torch
        self.device = device
        if weights is not None:                   # the widths are the checkpoint's (12 arrays per double block: 2 x (kernel, bias, 4 BN vectors))
            weights = list(weights)
            if len(weights) != 12 * 7 + 2 * 3 + 2:
                raise ValueError("the U-Net of pl.py:31-72 has 92 weight arrays, the checkpoint holds %d" % len(weights))
            filters = tuple(int(weights[12 * i].shape[3]) for i in range(3))
            bottleneck = int(weights[36].shape[3])
        self.filters = tuple(filters) if filters is not None else _FILTERS
        self.bottleneck = int(bottleneck) if bottleneck is not None else 1024
        self.dtype = dtype or {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[
            os.environ.get("TISSUE_HIP_UNET_DTYPE", "fp32")]
        g = torch.Generator().manual_seed(seed)
        self.p = {}
        self._hipw = {}                           # packed weights of the hand-written path, per arithmetic mode (_unet_hip.weights)
        self.last_mode = None                     # what the last forward pass really ran in
        self.reset_range()
        it = iter(weights) if weights is not None else None

        def expect(name, arr, shape):
            if tuple(arr.shape) != tuple(shape):
                raise ValueError("checkpoint does not fit the U-Net of pl.py:31-72: %s has shape %s, expected %s"
                                 % (name, tuple(arr.shape), tuple(shape)))
            if not np.isfinite(arr).all():        # (would otherwise be packed with scale 1 and poison every pass without a word)
                raise ValueError("checkpoint array %s holds a NaN or an infinity" % name)
            return np.ascontiguousarray(arr, dtype=np.float32)

        def conv(name, cin, cout, k):
            if it is not None:
                kern, bias = next(it), next(it)  # Keras (kh, kw, in, out)
                kern, bias = expect(name + " kernel", kern, (k, k, cin, cout)), expect(name + " bias", bias, (cout,))
                w = torch.from_numpy(np.ascontiguousarray(kern)).permute(3, 2, 0, 1)
                b = torch.from_numpy(np.ascontiguousarray(bias))
            else:
                std = (2.0 / (cin * k * k)) ** 0.5  # he_normal
                w = torch.randn((cout, cin, k, k), generator=g) * std
                b = torch.zeros(cout)
            self.p[name + ".w"] = w.to(device=device, dtype=self.dtype).contiguous(memory_format=torch.channels_last)
            self.p[name + ".b"] = b.to(device=device, dtype=self.dtype)

        def bn(name, c):
            if it is not None:
                gamma, beta, mean, var = (torch.from_numpy(expect(name + " statistics", next(it), (c,))) for _ in range(4))
            else:
                gamma, beta, mean, var = torch.ones(c), torch.zeros(c), torch.zeros(c), torch.ones(c)
            scale = gamma.double() / torch.sqrt(var.double() + _BN_EPS)
            shift = beta.double() - mean.double() * scale
            self.p[name + ".s"] = scale.to(device=device, dtype=self.dtype).view(1, c, 1, 1)
            self.p[name + ".t"] = shift.to(device=device, dtype=self.dtype).view(1, c, 1, 1)

        def convT(name, cin, cout):
            if it is not None:
                kern, bias = next(it), next(it)  # Keras Conv2DTranspose kernel (kh, kw, out, in)
                kern, bias = expect(name + " kernel", kern, (3, 3, cout, cin)), expect(name + " bias", bias, (cout,))
                w = torch.from_numpy(np.ascontiguousarray(kern)).permute(3, 2, 0, 1)  # torch: (in, out, kh, kw)
                b = torch.from_numpy(np.ascontiguousarray(bias))
            else:
                std = (1.0 / (cin * 9)) ** 0.5
                w = torch.randn((cin, cout, 3, 3), generator=g) * std
                b = torch.zeros(cout)
            self.p[name + ".w"] = w.to(device=device, dtype=self.dtype).contiguous()
            self.p[name + ".b"] = b.to(device=device, dtype=self.dtype)

        def double(name, cin, cout):
            conv(name + ".c1", cin, cout, 3)
            bn(name + ".b1", cout)
            conv(name + ".c2", cout, cout, 3)
            bn(name + ".b2", cout)

        c = in_ch
        for i, f in enumerate(self.filters):
            double("d%d" % i, c, f)
            c = f
        double("mid", c, self.bottleneck)
        c = self.bottleneck
        for i, f in enumerate(reversed(self.filters)):
            convT("u%d.t" % i, c, f)
            double("u%d" % i, 2 * f, f)
            c = f
        conv("head", c, 2, 1)

    def _epilogue(self, x, bias, scale, shift):
        """Conv2D's bias -> ReLU -> BatchNormalization (inference: per-channel scale and shift).  float32 on the GPU: one
        in-place pass in libtissue_hip.so on torch's current stream (same float32 operations in the same order as the
        four torch passes it replaces); otherwise the torch expressions."""
        torch = self.torch
        if (x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 4 == 0 and x.shape[0] == 1 and
                x.is_contiguous(memory_format=torch.channels_last) and os.environ.get("TISSUE_HIP_UNET_TORCH_EPILOGUE") != "1"
                and shares_runtime_with_torch(x)):
            lib = _lib.lib()
            stream = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(lib.tip_bias_relu_affine_f32_dev(x.data_ptr(), bias.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                                        x.numel(), x.shape[1], stream))
            return x
        x = torch.nn.functional.relu(x + bias.view(1, -1, 1, 1))
        return x * scale + shift

    def _double(self, x, name):
        F = self.torch.nn.functional
        p = self.p
        for k in ("1", "2"):
            x = F.conv2d(x, p[name + ".c" + k + ".w"], None, padding=1)
            x = self._epilogue(x, p[name + ".c" + k + ".b"], p[name + ".b" + k + ".s"], p[name + ".b" + k + ".t"])
        return x

    def calibrate_head(self, x, fraction):
        """Synthetic-weights helper (bench / tests; no trained weights ship with the reference): shifts the bias of the
        1x1 head so that class 0 exceeds the tail's 0.1 threshold (pl.py:168) on `fraction` of the pixels of input `x`.
        Random-init features follow the input's structure, so the thresholded map then has cell-sized blobs instead of
        being all-or-nothing, and the post-network tail sees a realistic boundary image."""
        torch = self.torch
        z = self.forward(x, logits=True)
        d = (z[0, 0] - z[0, 1]).reshape(-1).float()
        k = min(max(int(round((1.0 - fraction) * d.numel())), 1), d.numel())
        cut = float(torch.kthvalue(d, k).values)
        shift = float(np.log(0.1 / 0.9)) - cut          # p0 > 0.1  <=>  z0 - z1 > ln(1/9)
        self.p["head.b"][0] += shift
        return shift

    def randomize_statistics(self, seed=0):
        """Synthetic-weights helper (tests / bench; no trained weights ship with the reference): gives every convolution a
        non-zero bias and every BatchNormalization non-identity gamma / beta / moving mean / moving variance, drawn from a seeded
        generator on the host (two instances with the same seed get the same values), so that the activations have the dynamic
        range of a trained network instead of the half-zero, unit-scale maps of the he_normal / identity-BatchNorm initialisation."""
        torch = self.torch
        g = torch.Generator().manual_seed(1000 + seed)
        for k in sorted(self.p):
            v = self.p[k]
            if k.endswith(".b") and k != "head.b":
                new = torch.randn(v.numel(), generator=g) * 0.1
            elif k.endswith(".s"):                 # gamma / sqrt(var + eps): gamma in [0.5, 1.5], var in [0.5, 1.5]
                c = v.numel()
                gamma, var = torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) + 0.5
                beta, mean = torch.randn(c, generator=g) * 0.3, torch.randn(c, generator=g) * 0.2
                scale = gamma.double() / torch.sqrt(var.double() + _BN_EPS)
                self.p[k] = scale.to(device=v.device, dtype=v.dtype).view(v.shape)
                t = k[:-2] + ".t"
                self.p[t] = (beta.double() - mean.double() * scale).to(device=v.device, dtype=v.dtype).view(self.p[t].shape)
                continue
            else:
                continue
            self.p[k] = new.to(device=v.device, dtype=v.dtype).view(v.shape)
        self._hipw.clear()
        self.reset_range()

    def reset_range(self):
        """Forgets that a forward pass in f16x3 left fp16's range (TISSUE_HIP_UNET_RANGE=fallback keeps such a network in bf16x6):
        the next pass tries the requested mode again.  For callers that change the parameters in self.p themselves."""
        self.range_exceeded = False
        self._range_warned = False

    # -- hand-written convolution path (csrc/tip_unet_conv.h, driven by _unet_hip.py) -----------------------------------------------
    def _split_pack(self, taps, planes, fmt=0):
        return _unet_hip.split_pack(taps, planes, fmt)

    def _hip_weights(self, mode):
        return _unet_hip.weights(self, mode)

    def hip_path_ok(self, x):
        """The hand-written kernels tile every level's grid in 8 x 32 pixels: extents that are multiples of 64 x 256 (what
        prepare_image's padding to powers of two yields for every frame of at least 33 x 129 pixels).  No size limit: a tile
        addresses its halo window, not the tensor."""
        torch = self.torch
        return (_unet_mode() != "miopen" and x.is_cuda and self.dtype == torch.float32 and x.shape[0] == 1 and x.shape[1] == 2
                and self.filters == _FILTERS and self.bottleneck == 1024        # (the reference's widths, pl.py:60-69)
                and x.shape[2] % 64 == 0 and x.shape[3] % 256 == 0 and shares_runtime_with_torch(x))

    def forward(self, x, logits=False):
        """x: (1, C, H, W) tensor on the device -> class probabilities (1, 2, H, W) float32."""
        torch = self.torch
        F = torch.nn.functional
        if self.hip_path_ok(x):
            return _unet_hip.forward(self, x, _unet_mode(), logits)
        self.last_mode = "miopen"
        self.last_compose = ()
        with torch.no_grad():
            x = x.to(self.dtype).contiguous(memory_format=torch.channels_last)
            skips = []
            for i in range(3):
                f = self._double(x, "d%d" % i)
                skips.append(f)
                x = F.max_pool2d(f, 2)
            x = self._double(x, "mid")
            for i in range(3):
                n_h, n_w = x.shape[2] * 2, x.shape[3] * 2
                x = F.conv_transpose2d(x, self.p["u%d.t.w" % i], self.p["u%d.t.b" % i], stride=2)[:, :, :n_h, :n_w]
                x = torch.cat([x, skips[2 - i]], dim=1)
                x = self._double(x, "u%d" % i)
            x = F.conv2d(x, self.p["head.w"], self.p["head.b"])
            if logits:
                return x.float()
            return torch.softmax(x.float(), dim=1)

    def flops(self, h, w):
        """Dense multiply-add count x2 of one forward pass (for the MFMA roofline)."""
        total = 0
        c, hh, ww = 2, h, w
        for f in self.filters:
            total += 2 * hh * ww * 9 * (c * f + f * f)
            c, hh, ww = f, hh // 2, ww // 2
        total += 2 * hh * ww * 9 * (c * self.bottleneck + self.bottleneck * self.bottleneck)
        c = self.bottleneck
        for f in reversed(self.filters):
            hh, ww = hh * 2, ww * 2
            total += 2 * (hh // 2) * (ww // 2) * 9 * c * f            # transpose conv
            total += 2 * hh * ww * 9 * (2 * f * f + f * f)
            c = f
        total += 2 * hh * ww * c * 2
        return total


def load_keras_weight_list(path):
    """The checkpoint's arrays in model.get_weights() order (layer order of build_unet_model, pl.py:31-72; per layer Conv2D:
    kernel, bias; BatchNormalization: gamma, beta, moving_mean, moving_variance; Conv2DTranspose: kernel, bias).

    `.h5` / `.hdf5` / `.keras`-named HDF5 files -- what model.save_weights() / model.save() write and what pl.py:86
    (`model.load_weights(self.weights_path)`) reads -- go through the self-contained reader of _hdf5.py: like Keras' loading
    by topology, the file's layers that carry weights are taken in file order; the layer kinds are checked against the
    network's (a checkpoint of another architecture raises ValueError, as Keras does).  `.npz`: np.savez(path, *model.get_weights())."""
    if path is None:
        return None
    if not os.path.exists(path):
        raise OSError("Unable to open file (unable to open file: name = '%s')" % path)  # h5py/Keras wording
    if str(path).endswith(".npz"):
        z = np.load(path)
        return [z["arr_%d" % i] for i in range(len(z.files))]
    from . import _hdf5
    layers = [(name, ws) for name, ws in _hdf5.load_keras_weights_h5(path) if ws]
    # build_unet_model's weight-carrying layers: 7 double blocks of (Conv2D, BN, Conv2D, BN), a Conv2DTranspose in front of each
    # of the last three, the 1x1 Conv2D head
    kinds = ["conv", "bn", "conv", "bn"] * 4
    for _ in range(3):
        kinds += ["convT", "conv", "bn", "conv", "bn"]
    kinds += ["conv"]
    if len(layers) != len(kinds):
        raise ValueError("You are trying to load a weight file containing %d layers into a model with %d layers." % (len(layers), len(kinds)))
    out = []
    for (name, ws), kind in zip(layers, kinds):
        arrs = [a for _, a in ws]
        ok = {"conv": len(arrs) == 2 and arrs[0].ndim == 4 and arrs[1].ndim == 1,
              "convT": len(arrs) == 2 and arrs[0].ndim == 4 and arrs[1].ndim == 1 and arrs[0].shape[2] == arrs[1].shape[0],
              "bn": len(arrs) == 4 and all(a.ndim == 1 for a in arrs)}[kind]
        if kind == "conv" and ok:
            ok = arrs[0].shape[3] == arrs[1].shape[0]
        if not ok:
            raise ValueError("checkpoint layer '%s' (%s) does not fit the %s layer of the U-Net of pl.py:31-72 at that position"
                             % (name, ", ".join(str(a.shape) for a in arrs), {"conv": "Conv2D", "convT": "Conv2DTranspose", "bn": "BatchNormalization"}[kind]))
        if kind == "bn":                          # by name where Keras names them (gamma / beta may be absent from odd configurations)
            order = {"gamma": 0, "beta": 1, "moving_mean": 2, "moving_variance": 3}
            keyed = sorted(ws, key=lambda t: order.get(t[0].split("/")[-1].split(":")[0], 99))
            if all(t[0].split("/")[-1].split(":")[0] in order for t in ws):
                arrs = [a for _, a in keyed]
        elif all(t[0].split("/")[-1].split(":")[0] in ("kernel", "bias") for t in ws):
            arrs = [a for _, a in sorted(ws, key=lambda t: 0 if t[0].split("/")[-1].startswith("kernel") else 1)]
        out.extend(arrs)
    return out


class SegmentationPredictor:
    """pl.py:74-198.  `predict(image)` with image (C=2, Y, X) returns (labels int32 (X, Y), HC float64 (X, Y))."""

    def __init__(self, model_weights_path, image_shape, device=None):
        import torch
        self.torch = torch
        self.weights_path = model_weights_path
        if device is None:
            device = int(os.environ.get("TISSUE_HIP_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        self.device_index = int(device)
        _lib.init(self.device_index)
        if not torch.cuda.is_available():
            raise _lib.TissueHipError("SegmentationPredictor needs an MI355X (no CPU fallback)")
        self.device = torch.device("cuda", self.device_index)
        first_axis_shape, second_axis_shape = find_desired_shape(image_shape[-2], image_shape[-1])
        self.model_shape = (first_axis_shape, second_axis_shape, 2)
        self.model = self.initialize_model()
        self.forward_ms = None   # bench.py sets this to a list: per-call duration of the network's forward pass
        self.last_route = None   # predict(): dict(requested=, ran=, range_exceeded=)

    def initialize_model(self):
        weights = load_keras_weight_list(self.weights_path)
        return _UNet(2, self.device, weights=weights)

    # -- U1 -----------------------------------------------------------------------------------------------
    def prepare_image(self, image):
        """pl.py:90-122: per-channel 1/99-percentile normalisation, (C,Y,X)->(1,X,Y,C), front-pad to powers of two.
        Returns a torch tensor laid out (1, C, X', Y') (the NCHW view of the reference's NHWC array) and npad."""
        torch = self.torch
        if isinstance(image, torch.Tensor):
            src_dtype = image.dtype
            t = image.to(device=self.device)
        else:
            arr = np.ascontiguousarray(image)
            if arr.dtype == np.uint16:          # torch has no arithmetic on uint16: the values fit int32
                arr = arr.astype(np.int32)
            elif arr.dtype in (np.uint32, np.uint64):
                arr = arr.astype(np.int64)
            t = torch.as_tensor(arr, device=self.device)
            src_dtype = t.dtype
        if t.dim() != 3:
            raise ValueError("image should be in axes order (C, Y, X)")
        integer_in = not src_dtype.is_floating_point
        single_in = src_dtype == torch.float32
        t = t.to(torch.float64)                 # exact for every integer / float32 input value
        C, Y, X = t.shape
        shape1, shape2 = X, Y
        first_axis_pixels, second_axis_pixels = find_desired_shape(shape1, shape2)
        npad = ((0, 0), (first_axis_pixels - shape1, 0), (second_axis_pixels - shape2, 0), (0, 0))
        # One library submission on torch's stream (tip_unet_prepare_f64_dev): the four order statistics of every channel by
        # radix select, numpy's lerp, clip / scale / transpose / pad in one pass -- nothing comes back to the host.  (The torch
        # expressions below sort every channel and make a dozen elementwise passes: 2.2 ms of a 2048^2 frame against 0.25.)
        dense = t.is_cuda and C <= 8 and ((t.stride(1) == 1 and t.stride(2) == Y) or (t.stride(2) == 1 and t.stride(1) == X))
        if dense and (C == 1 or t.stride(0) >= X * Y) and shares_runtime_with_torch(t) and not os.environ.get("TISSUE_HIP_PREPARE_TORCH"):
            if self.model_shape != (first_axis_pixels, second_axis_pixels, 2):
                self.model_shape = (first_axis_pixels, second_axis_pixels, 2)
            padded = torch.empty((1, C, first_axis_pixels, second_axis_pixels), dtype=torch.float32, device=t.device)
            kind = 2 if integer_in else (1 if single_in else 0)
            _lib.check(_lib.lib().tip_unet_prepare_f64_dev(
                t.data_ptr(), C, Y, X, t.stride(0), t.stride(1), t.stride(2), kind, padded.data_ptr(), second_axis_pixels,
                first_axis_pixels, torch.cuda.current_stream(t.device).cuda_stream))
            return padded, npad
        chans = []
        for c in range(C):
            ch = t[c]
            srt = torch.sort(ch.reshape(-1)).values
            per99 = _percentile_linear_t(srt, 99)
            per1 = _percentile_linear_t(srt, 1)
            # normalize_channel (pl.py:21-29) stores the percentiles into a copy of the INPUT: the clip values take its dtype
            hi, lo = per99, per1
            if integer_in:
                hi, lo = float(np.trunc(per99)), float(np.trunc(per1))
            elif single_in:
                hi, lo = float(np.float32(per99)), float(np.float32(per1))
            clipped = torch.where(ch > per99, torch.full_like(ch, hi), ch)
            clipped = torch.where(ch < per1, torch.full_like(ch, lo), clipped)
            if single_in:                        # numpy 1.x keeps float32 array (op) float64 scalar in float32
                n32 = (clipped.to(torch.float32) - float(np.float32(per1))) / float(np.float32(per99 - per1))
                chans.append(n32.to(torch.float64))
            else:
                chans.append((clipped - per1) / (per99 - per1))
        norm = torch.stack(chans)                      # (C, Y, X) float64
        xy = norm.permute(0, 2, 1)                     # np.transpose(normalized) -> (X, Y, C); NCHW view: (C, X, Y)
        if self.model_shape != (first_axis_pixels, second_axis_pixels, 2):
            self.model_shape = (first_axis_pixels, second_axis_pixels, 2)
        padded = torch.zeros((1, C, first_axis_pixels, second_axis_pixels), dtype=torch.float32, device=self.device)
        padded[0, :, npad[1][0]:, npad[2][0]:] = xy.to(torch.float32)
        return padded, npad

    # -- U2-U5 --------------------------------------------------------------------------------------------
    def predict(self, image, debug=False, return_device=False):
        """debug: prints last_route, the arithmetic the network was asked for (TISSUE_HIP_UNET_ARITH) and the one that ran --
        'miopen' when the torch layers did (small frames, another HIP runtime in the process), 'bf16x6' behind range_exceeded."""
        torch = self.torch
        padded, npad = self.prepare_image(image)
        if self.forward_ms is not None:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
        prob = self.model.forward(padded)                              # (1, 2, X', Y') float32
        if self.forward_ms is not None:
            ev1.record()
            ev1.synchronize()
            self.forward_ms.append(ev0.elapsed_time(ev1))
        self.last_route = dict(requested=_unet_mode(), ran=getattr(self.model, "last_mode", None),
                               range_exceeded=bool(getattr(self.model, "range_exceeded", False)))
        if debug:
            print("U-Net route: requested %(requested)s, ran %(ran)s, range_exceeded %(range_exceeded)s" % self.last_route)
        unp = prob[:, :, npad[1][0]:, npad[2][0]:]
        p0 = unp[0, 0]
        labels, hc = self.segment_probability(p0, return_device=return_device)
        return labels, hc

    def segment_probability(self, p0, thr=0.1, return_device=False):
        """pl.py:167-194 on a device-resident probability map (torch tensor (X, Y)): threshold -> 5x5 closing ->
        7x7 erosion -> boundary -> watershed, one submission on the library's stream (tip_unet_tail_dev).  Returns
        (labels int32, HC float64) as numpy arrays, or as torch tensors with return_device=True.

        Stream ordering: the two output tensors come from torch's caching allocator, whose blocks may still be in use by
        kernels queued on torch's current stream (another worker thread's freed temporaries when the threads share the
        default stream), and p0 is produced on that stream -- so the library's stream waits for the torch stream AFTER the
        allocations (tip_wait_stream), and the host waits for the library before torch sees the results."""
        torch = self.torch
        lib = _lib.lib()
        if p0.dim() != 2:
            raise ValueError("segment_probability takes a 2-D probability map")
        if p0.dtype not in (torch.float32, torch.float64):
            p0 = p0.to(torch.float32)
        if p0.stride(1) != 1:
            p0 = p0.contiguous()
        if not shares_runtime_with_torch(p0):
            raise _lib.TissueHipError("libtissue_hip.so and torch use different HIP runtimes in this process: import torch before "
                                      "the first tissue_image_processing_amd call (see INTEGRATION.md)")
        Xn, Yn = int(p0.shape[0]), int(p0.shape[1])
        lab = torch.empty((Xn, Yn), dtype=torch.int32, device=p0.device)
        hc = torch.empty((Xn, Yn), dtype=torch.float64, device=p0.device)
        stream = torch.cuda.current_stream(p0.device).cuda_stream
        _lib.check(lib.tip_wait_stream(stream))
        flags = ctypes.c_int32(0)
        rc = lib.tip_unet_tail_dev(p0.data_ptr(), 0 if p0.dtype == torch.float32 else 1, p0.stride(0), Xn, Yn, thr,
                                   lab.data_ptr(), hc.data_ptr(), ctypes.byref(flags))
        self.last_flags = flags.value
        self.last_markers = int(lib.tip_last_watershed_labels())
        _lib.check(rc)
        _lib.check(lib.tip_sync())
        if return_device:
            return lab, hc
        return lab.cpu().numpy(), hc.cpu().numpy()
