"""A/B of the image path around the two stages: host route (PIL + numpy + CPU torch, what the pipeline does by default) against device
route (``PipelineConfig.device_io``: rsvld_amd.imageops), step by step, for one 512 x 512 input at x8 (4096) and x4 (2048).

    python tools/bench_image_path.py [--out profiles/image_path_ab.txt]

Each step is timed as the pipeline runs it, transfers included: the host route ends with its tensor on the device (or its image on the
host), the device route starts from the decoded image on the host (or ends with the uint8 image there).  PNG decode / encode are the
same in both routes and left out.  Host route: ``perf_counter`` around the step with a device synchronise, median of 3 after one warm
run.  Device route: HIP events on the current stream, warm, median of 5.  ``bench.py`` keeps its inputs resident and sees none of this."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _host(fn, reps=3):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def _device(fn, reps=5):
    fn()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def steps(lr, scale, dev, plan):
    """[(step, host closure, device closure)] for one LR image; operands of the later steps are made once, outside the timing."""
    from rsvld_amd import imageops as I
    from rsvld_amd.data import dataset as D
    from rsvld_amd.models.util import PIL2Tensor, Tensor2PIL
    from rsvld_amd.utils.tensor2img import tensor2img
    S = lr.size[0] * scale
    g = torch.Generator().manual_seed(0)
    sr = (torch.rand((3, S, S), generator=g) * 2.4 - 1.2).to(dev)          # a Stage-1 result, resident as in the pipeline
    sr_u8 = I.tensor2img(sr)
    sr_pil = Image.fromarray(sr_u8.cpu().numpy())
    out = (torch.rand((3, S, S), generator=g) * 2.4 - 1.2).to(dev)         # a Stage-2 result

    def host_loader():
        img = D.resize_and_convert(lr, scale)
        x = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).float() / 255.0
        return ((x - 0.5) / 0.5).unsqueeze(0).to(dev)

    return [
        ("Stage-1 loader", host_loader, lambda: I.load_sr_input(lr, scale, dev, plan)["SR"]),
        ("8-bit hand-off", lambda: tensor2img(sr, min_max=(-1, 1)), lambda: I.tensor2img(sr).cpu()),
        ("Stage-2 input", lambda: PIL2Tensor(sr_pil, upscale=1, min_size=1024)[0].unsqueeze(0).to(dev),
         lambda: I.pil2tensor(sr_u8, upscale=1, min_size=1024, plan=plan)[0]),
        ("Stage-2 output", lambda: Tensor2PIL(out, S, S), lambda: I.tensor2pil_u8(out, S, S, plan=plan).cpu()),
    ]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "image_path_ab.txt"))
    a = ap.parse_args(argv)
    from rsvld_amd import imageops as I
    dev = torch.device("cuda:0")
    plan = I.ImagePlan()
    lr = Image.fromarray(np.random.default_rng(0).integers(0, 256, (512, 512, 3), dtype=np.uint8))
    lines = [f"image path, host route vs device route (tools/bench_image_path.py) on {torch.cuda.get_device_name(0)}, "
             f"{torch.get_num_threads()} CPU threads", "milliseconds per image; host: perf_counter, median of 3; device: HIP events, median of 5; "
             "transfers included, PNG decode / encode excluded", ""]
    for scale in (8, 4):
        lines.append(f"512 -> {512 * scale} (x{scale})")
        lines.append(f"  {'step':<16}{'host ms':>10}{'device ms':>11}{'host/device':>13}  device faster")
        tot_h = tot_d = 0.0
        for name, host, device in steps(lr, scale, dev, plan):
            h, d = _host(host), _device(device)
            tot_h, tot_d = tot_h + h, tot_d + d
            lines.append(f"  {name:<16}{h:>10.1f}{d:>11.2f}{h / d:>13.1f}  {'yes' if d < h else 'NO'}")
        lines.append(f"  {'all four':<16}{tot_h:>10.1f}{tot_d:>11.2f}{tot_h / tot_d:>13.1f}  the image gains {(tot_h - tot_d) / 1e3:.2f} s")
        lines.append("")
        print("\n".join(lines[-8:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
