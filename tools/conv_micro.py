r"""Micro-benchmark of az_conv2d_f32 on one shape (for rocprofv3 PMC passes and A/B tuning).

    python tools/conv_micro.py B H W Cin Cout [ks] [stride] [reps] [C1] [up] [affine]

C1 > 0: a second source of C1 channels behind the Cin of the first, read through nearest upsampling by 2^up (the UNet's merge
layers: C1 = the lower level's channels, up = 1).  C1 = 0 with up > 0: the one source is read through 2^up upsampling (ADM's
up-ResBlocks and Upsample layers).  (H, W) is always the map the convolution runs on.
affine: the input carries a pending normalisation (AzConvArgs.in_affine, the first convolution of a UNetBlock): 1 = plain
(in_act 0), 2 = with SiLU (in_act 1); 0 or absent: none.  AZ_AFFINE=1 / 2 in the environment does the same.
"""
import sys
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from azula_amd.engine import Act, Builder

B, H, W, Cin, Cout = (int(v) for v in sys.argv[1:6])
ks = int(sys.argv[6]) if len(sys.argv) > 6 else 3
stride = int(sys.argv[7]) if len(sys.argv) > 7 else 1
reps = int(sys.argv[8]) if len(sys.argv) > 8 else 20
C1 = int(sys.argv[9]) if len(sys.argv) > 9 else 0
up = int(sys.argv[10]) if len(sys.argv) > 10 else 0
affine = int(sys.argv[11]) if len(sys.argv) > 11 else int(os.environ.get("AZ_AFFINE") or 0)
up0, up1 = (0, up) if C1 else (up, 0)
low = lambda n, u: (n + (1 << u) - 1) >> u  # noqa: E731
dev = torch.device("cuda")
torch.manual_seed(0)
bld = Builder(dev)
scale = 0.0 if os.environ.get("AZ_ZERO") else 1.0
x = Act(torch.randn(B * low(H, up0) * low(W, up0) * Cin, device=dev) * scale, B, low(H, up0), low(W, up0), Cin, Cin, True)
x1 = Act(torch.randn(B * low(H, up1) * low(W, up1) * C1, device=dev) * scale, B, low(H, up1), low(W, up1), C1, C1, True) if C1 else None
w = torch.randn(Cout, Cin + C1, ks, ks, device=dev) / ((Cin + C1) * ks * ks) ** 0.5 * scale
b = torch.randn(Cout, device=dev)
if affine:  # the input carries a pending normalisation (AzConvArgs.in_affine): 1 plain, 2 with SiLU
    x.affine = (torch.randn(2 * B * Cin, device=dev) * scale, affine - 1)
wino = {"1": True, "0": False, "4": 4, "x3": "x3", "wx3": "wx3", "h2": "h2", "wh2": "wh2"}.get(os.environ.get("AZ_WINO", ""), None)
src = dict(src1=x1, up1=up1) if C1 else dict(up0=up0)
y = bld.conv(x, bld.pack_conv(w, b, cin0=Cin) if C1 else bld.pack_conv(w, b), Cout, hin=H, win=W, stride=stride, act=int(os.environ.get("AZ_ACT", "1")),
             winograd=wino, gn_stats=bool(os.environ.get("AZ_GN")), **src)
if os.environ.get("AZ_SPLITK"):  # override the suggested split-K (A/B)
    _d = [k for k in bld.tape.keep if hasattr(k, "_flops")][-1]
    _d.splitk = int(os.environ["AZ_SPLITK"])
    bld._ws_need = max(bld._ws_need, _d.splitk * B * ((H + stride - 1) // stride) * ((W + stride - 1) // stride) * _d.cout_s)
    if _d not in bld._ws_users:
        bld._ws_users.append(_d)
bld.finish()
desc = bld.tape.keep[-1] if hasattr(bld.tape.keep[-1], "_flops") else [k for k in bld.tape.keep if hasattr(k, "_flops")][-1]
for _ in range(3):
    bld.tape.run()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    bld.tape.run()
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / reps
if len(bld.tape.ops) > 1:  # per-op times (e.g. the split pass of AZ_X3_PLANES=1, split-K combine is inside its entry)
    import ctypes
    from azula_amd import _lib
    st = torch.cuda.current_stream().cuda_stream
    per = []
    for fn, args, name in bld.tape.ops:
        e0.record()
        for _ in range(reps):
            fn(*args, st)
        e1.record()
        torch.cuda.synchronize()
        per.append(f"{name} {e0.elapsed_time(e1) / reps * 1e3:.1f} us")
    print("   ", "; ".join(per))
cin = f"{Cin}+{C1}(up{up})" if C1 else (f"{Cin}(up{up})" if up else f"{Cin}")
aff = ("", " affine", " affine+silu")[affine] if desc.in_affine else ""
print(f"conv[{desc._algo[10:-4]}{aff}] {B}x{H}x{W} {cin}->{Cout} k{ks} s{stride} splitk={desc.splitk}: {ms * 1e3:.1f} us  {desc._flops / ms / 1e9:.1f} TF/s")
