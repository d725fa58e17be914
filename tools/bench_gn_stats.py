"""GroupNorm statistics launches and halo convolutions that write epilogue statistics, at workload shapes: median microseconds of
200 event-timed calls per case, one JSON line ``AB_RESULT {case: us}``.  Times the tree in the CURRENT DIRECTORY (its ops.py and
its library), so that two checkouts can be alternated in one job:  (cd parent && python <tree>/tools/bench_gn_stats.py) and
(cd <tree> && python tools/bench_gn_stats.py) in the order P P N P N P N ... -- the parent's A/A spread first
(profiles/gn_stats_offset_ab.txt)."""
import json
import math
import os
import sys

sys.path.insert(0, os.getcwd())
import torch
from rsvld_amd import ops, _lib as L

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(1)
ITERS, WARM = 200, 20


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(ITERS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return round(t[len(t) // 2], 2)


def act(B, H, W, C, dt, off=0.3):
    return (torch.randn(B, H, W, C, generator=g) * 1.5 + off).to(dev, dt)


res = {}
# statistics pass, fp32 input (split precision): Stage-2 UNet level 0 and a VAE decoder map
for name, shp in (("stats_f32 2x128x128x320", (2, 128, 128, 320)), ("stats_f32 1x512x512x128", (1, 512, 512, 128)), ("stats_f32 1x1024x1024x128", (1, 1024, 1024, 128))):
    x = act(*shp, torch.float32)
    with ops.f32_split(ops.ALL_SPLIT):
        res[name] = timed(lambda: ops.group_norm_stats(x, 32))
    ga, be = torch.ones(shp[3], device=dev), torch.zeros(shp[3], device=dev)
    with ops.f32_split(ops.ALL_SPLIT):
        res[name.replace("stats_f32", "scale_shift_f32")] = timed(lambda: ops._gn_scale_shift_f32(x, None, ga, be, 32, 1e-5))
    del x
# statistics pass, fp16 input (SR3 level 0 at 256 x 256, a 128-channel level) and the one-workgroup kernel
for name, shp in (("stats_f16 4x256x256x64", (4, 256, 256, 64)), ("stats_f16 4x128x128x128", (4, 128, 128, 128)), ("stats_f16 1x1024x1024x64", (1, 1024, 1024, 64))):
    x = act(*shp, torch.float16)
    res[name] = timed(lambda: ops.group_norm_stats(x, 32))
    del x
x = act(4, 32, 32, 512, torch.float16)
ga, be = torch.ones(512, device=dev), torch.zeros(512, device=dev)
res["gn_small_f16 4x32x32x512 (norm+apply)"] = timed(lambda: ops.group_norm(x, ga, be, 32, 1e-5, silu=True))
del x
# halo convolutions that write statistics from the epilogue
def conv_case(name, B, H, W, Cin, Cout, dt, policy):
    x = act(B, H, W, Cin, dt, 0.0)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)
    b = torch.randn(Cout, generator=g)
    pc = ops.pack_conv(w, b, torch.float32 if policy else dt, dev)
    with ops.f32_split(policy), ops.tuning(profiler=(prof := ops.LaunchProfiler())):
        ops.conv2d(x, pc, pad=1, stats=True)
    names = [n for n in prof.summary() if n.startswith("conv_halo")]
    assert len(names) == 1, prof.summary().keys()
    with ops.f32_split(policy):
        y = ops.conv2d(x, pc, pad=1, stats=True)
        assert hasattr(y, "_gn_part")
        res[f"{names[0]}+stats {name}"] = timed(lambda: ops.conv2d(x, pc, pad=1, stats=True))
        res[f"{names[0]} no stats {name}"] = timed(lambda: ops.conv2d(x, pc, pad=1, stats=False))
conv_case("f16 2x256x256 64->64", 2, 256, 256, 64, 64, torch.float16, None)
conv_case("f16 4x128x128 128->128", 4, 128, 128, 128, 128, torch.float16, None)
conv_case("f16 2x128x128 256->256", 2, 128, 128, 256, 256, torch.float16, None)
conv_case("split 1x256x256 128->128", 1, 256, 256, 128, 128, torch.float32, ops.ALL_SPLIT)
conv_case("split 2x128x128 320->320", 2, 128, 128, 320, 320, torch.float32, ops.ALL_SPLIT)
print("AB_RESULT " + json.dumps(res))
