"""A/B of the caption's view preparation: host route (PIL image -> ``llava_next.process_images`` -> upload as fp16, what the pipeline does
by default) against device route (resident uint8 image -> ``imageops.caption_views``), with the image processor and grid pinpoints of
the 8 B captioner (tools/synthetic_models.py: S = 336), on seeded uint8 images of 1024^2, 2048^2, 4096^2 and 4096 x 2304.

    python tools/bench_caption_views.py [--out profiles/caption_views_ab.txt]

One process; both routes warm (one untimed run each per size: tables built, code objects loaded).  Per size six pairs, the order
alternating (host first in pairs 0, 2, 4; device first in 1, 3, 5); each run is ``perf_counter`` around the call AND a device
synchronise, and every pair is compared with ``torch.equal``.  Of the device route the host's share (the time until the last launch is
queued) is kept apart, and at 4096^2 each launch is bracketed with HIP events (``ops.LaunchProfiler``) in five further runs."""
import argparse
import os
import statistics
import sys
import time
import types

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = [(1024, 1024), (2048, 2048), (4096, 4096), (4096, 2304)]      # (width, height)
PAIRS = 6


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return out, (t2 - t0) * 1e3, (t1 - t0) * 1e3


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caption_views_ab.txt"))
    ap.add_argument("--sizes", default=None, help="rehearsal: 'WxH,WxH' instead of the four sizes")
    a = ap.parse_args(argv)
    import synthetic_models as SM
    from rsvld_amd import imageops as I, llava_next as LN, ops
    sizes = SIZES if a.sizes is None else [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    dev = torch.device("cuda:0")
    proc, pins = SM.clip_l_336_processor(), SM.LLAVA_MM["image_grid_pinpoints"]
    cfg = types.SimpleNamespace(image_aspect_ratio="anyres", image_grid_pinpoints=pins)
    plan = I.ImagePlan()
    lines = [f"caption views, host route vs device route (tools/bench_caption_views.py) on {torch.cuda.get_device_name(0)}, "
             f"{torch.get_num_threads()} CPU threads",
             f"milliseconds per image, perf_counter around the call and a device synchronise; {PAIRS} alternated pairs per size in one process, "
             "both routes warm; every pair torch.equal", ""]
    all_faster = {}
    for w, h in sizes:
        start = len(lines)
        arr = np.random.default_rng(w * 7 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        pil, u8 = Image.fromarray(arr), torch.from_numpy(arr).to(dev)

        def host():
            return [v.to(dtype=torch.float16, device=dev) for v in LN.process_images([pil], proc, cfg)][0]

        def device():
            return I.caption_views(u8, proc, pins, torch.float16, plan)

        assert torch.equal(host(), device())          # warm-up of both, and the first comparison
        layout = I.anyres_layout((w, h), 336, pins)
        lines.append(f"{w} x {h}: canvas {layout[0]} x {layout[1]}, fit {layout[2]} x {layout[3]} at {layout[4:]}, "
                     f"{1 + (layout[0] // 336) * (layout[1] // 336)} views")
        lines.append(f"  {'pair':<6}{'order':<14}{'host ms':>10}{'device ms':>11}{'(its host part)':>17}{'host/device':>13}")
        hs, ds, qs = [], [], []
        for k in range(PAIRS):
            first_host = k % 2 == 0
            res = {}
            for which in (("host", "device") if first_host else ("device", "host")):
                res[which] = _timed(host if which == "host" else device)
            assert torch.equal(res["host"][0], res["device"][0]), f"{w} x {h}, pair {k}: the routes differ"
            hm, dm, q = res["host"][1], res["device"][1], res["device"][2]
            hs.append(hm), ds.append(dm), qs.append(q)
            lines.append(f"  {k:<6}{'host, device' if first_host else 'device, host':<14}{hm:>10.2f}{dm:>11.3f}{q:>17.3f}{hm / dm:>13.1f}")
        faster = all(d < h_ for d, h_ in zip(ds, hs))
        all_faster[(w, h)] = faster
        lines.append(f"  {'median':<20}{statistics.median(hs):>10.2f}{statistics.median(ds):>11.3f}{statistics.median(qs):>17.3f}"
                     f"{statistics.median(hs) / statistics.median(ds):>13.1f}   device faster in every pair: {'yes' if faster else 'NO'}")
        lines.append(f"  {'min .. max':<20}{min(hs):>6.2f} .. {max(hs):<7.2f}{min(ds):>6.3f} .. {max(ds):<7.3f}")
        if (w, h) == (4096, 4096) or a.sizes is not None:
            runs = []
            for _ in range(5):
                with ops.tuning(profiler=(prof := ops.LaunchProfiler())):
                    device()
                torch.cuda.synchronize()
                runs.append([(r[0], r[3].elapsed_time(r[4])) for r in prof.records])
            names = [n for n, _ in runs[0]]
            assert all([n for n, _ in r] == names for r in runs)
            med = [statistics.median(r[i][1] for r in runs) for i in range(len(names))]
            what = ["fit, horizontal", "fit, vertical", "squash, horizontal", "squash, vertical", "views"]
            lines.append(f"  the launches of the device route (HIP events around each, median of 5 runs; sum {sum(med):.3f} ms):")
            for i, (n, m) in enumerate(zip(names, med)):
                lines.append(f"    {i}  {n:<16}{(what[i] if len(names) == 5 else ''):<20}{m:>9.3f} ms{'   <- the largest' if m == max(med) else ''}")
            lines.append(f"  device time {sum(med):.3f} ms against {statistics.median(qs):.3f} ms of host time to queue the route: "
                         f"the {'launches' if sum(med) > statistics.median(qs) else 'host'} are the larger part")
        lines.append("")
        print("\n".join(lines[start:]), flush=True)
    for size, faster in all_faster.items():
        lines.append(f"device route faster in every pair at {size[0]} x {size[1]}: {'yes' if faster else 'NO'}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
