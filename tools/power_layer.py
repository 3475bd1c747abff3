"""Board power and clocks while ONE f16x3 convolution launch of u2.c2's shape (2048 x 2048, 128 -> 128, nine taps: an 8-row launch)
runs back to back (GPU box): python tools/power_layer.py [flags]   (flags: tip_unet_conv_ex_dev's; 1 = TIP_UNET_CONV_ROWS8_K32)"""
import ctypes, os, re, subprocess, sys, threading, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
flags = int(sys.argv[1]) if len(sys.argv) > 1 else 0
import torch
from tissue_image_processing_amd import _lib, _unet_hip as uh
N, C = 2048, 128
dev = torch.device("cuda", 0)
g = torch.Generator(device="cpu").manual_seed(1)
taps = (torch.randn((9, C, C), generator=g) * 0.05).to(dev)
wp, inv = uh._pack(taps, 2, 1)
# dense activations (a trained network's): fp16 pieces of 16 x uniform values, low pieces random
src = torch.stack([(torch.rand((N, N, C), device=dev) * 16).half(), (torch.rand((N, N, C), device=dev) * 2e-3).half()], 0).contiguous()
out = torch.empty_like(src)
bias, scale, shift = (torch.zeros(C, device=dev), torch.full((C,), 16.0, device=dev), torch.zeros(C, device=dev))
d = uh._conv_desc((wp, [k // 3 - 1 for k in range(9)], [k % 3 - 1 for k in range(9)], inv), 2, 1, src, None, N, N, bias, scale, shift, out=out)
lib = _lib.lib()
stream = torch.cuda.current_stream(dev).cuda_stream
print("code %d, K %d" % (lib.tip_unet_conv_flavour_ex(ctypes.byref(d), flags), lib.tip_unet_conv_mfma_k_ex(ctypes.byref(d), flags)))
_lib.check(lib.tip_unet_conv_ex_dev(ctypes.byref(d), flags, stream)); torch.cuda.synchronize()
stop, samples = False, []
def probe():
    while not stop:
        try:
            samples.append(subprocess.run(["rocm-smi", "--showpower", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=20).stdout)
        except Exception as e:
            samples.append("ERR %r" % (e,))
        time.sleep(0.5)
th = threading.Thread(target=probe); th.start()
t0 = time.time(); n = 0
while time.time() - t0 < 10:
    for _ in range(100):
        _lib.check(lib.tip_unet_conv_ex_dev(ctypes.byref(d), flags, stream))
    torch.cuda.synchronize(); n += 100
dt = time.time() - t0
stop = True; th.join()
print("%d launches, %.3f ms each, %.1f TFLOP/s" % (n, 1e3 * dt / n, 2.0 * N * N * 9 * C * C * n / dt / 1e12))
for s in samples[2:8]:
    print(" | ".join(l.strip() for l in s.splitlines() if re.search(r"Power|sclk|mclk|fclk", l))[:400])
