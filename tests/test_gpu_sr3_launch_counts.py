"""Which kernels one SR3 UNet forward launches, and how often, per precision: the launch names of the SECOND forward (the first
packs weights and may launch for it) under a ``LaunchProfiler``, as a ``Counter``, against a table written down from the commit
before the UNet became a ``hipnn.HipNet``.  A refactoring of the network runtime must leave every row as it is; a change of a
kernel route changes its row on purpose.  The network is the one of tests/test_gpu_sr3.py, batch 1 at its ``image_size``."""
from collections import Counter

import pytest
import torch

from test_gpu_sr3 import sr3  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

_IGEMM = {"128x128": 1, "128x64": 10, "256x32": 1, "64x128": 1, "64x64": 52}       # the 65 convolutions by tile
_SPLIT = {"conv_halo_128_split": 2, "conv_halo_64_split": 7, "groupnorm_ab_from_partials": 5, "groupnorm_apply_split": 39,
          "groupnorm_stats_split": 34, "split_planes": 32}
EXPECTED = {
    "fp16": {"attention_d512": 4, "groupnorm(3 kernels)": 39, **{f"conv_igemm_{t}": n for t, n in _IGEMM.items()}},
    "w2": {"attention_d512": 4, "groupnorm(3 kernels)": 39, **{f"conv_igemm_{t}_w2": n for t, n in _IGEMM.items()}},
    "bf16": {"attention_d512": 4, "groupnorm(3 kernels)": 39, **{f"conv_igemm_{t}": n for t, n in _IGEMM.items()}},
    "fp32": {"attention_f32_d512": 4, "conv_f32": 65, "groupnorm_apply_f32": 39, "groupnorm_stats_f32": 39},
    # UNET_POLICY: fp16 attention operands (the 16-bit d = 512 kernel; the query and output 1x1 convs of the four sites on fp16 pairs)
    "split": {"attention_d512": 4, "conv_igemm_64x64_w2": 4, "conv_igemm_split": 52, "planes_to_f16": 8, **_SPLIT},
    "split/all": {"attention_split_gemm_qk_d512": 4, "attention_split_softmax": 4, "attention_split_gemm_pv_d512": 4,
                  "conv_igemm_split": 56, **_SPLIT},
}


@pytest.mark.parametrize("mode", ["fp16", "w2", "bf16", "fp32", "split", "split/all"])
def test_second_forward_launch_counts(sr3, cuda, mode):  # noqa: F811
    from oracle import seeded
    from oracle.sr3_oracle import SR3_CFG
    from rsvld_amd import ops
    net, _ = sr3
    unet = net.denoise_fn
    S = SR3_CFG["image_size"]
    unet.set_compute_dtype(mode.split("/")[0], **({"policy": ops.ALL_SPLIT} if mode == "split/all" else {}))
    try:
        xin = ops.nchw_to_nhwc(seeded.synthetic_image((1, SR3_CFG["in_channel"], S, S), seed=3, smooth=3).to(cuda), unet.compute_dtype)
        level = torch.full((1, 1), 0.5, device=cuda)
        with torch.no_grad():
            unet.forward_nhwc(xin, level)
            prof = ops.LaunchProfiler()
            with ops.tuning(profiler=prof):
                unet.forward_nhwc(xin, level)
        torch.cuda.synchronize()
    finally:
        unet.set_compute_dtype("fp16")
    got = Counter(r[0] for r in prof.records)
    print(f"{mode!r}: {dict(sorted(got.items()))},")
    assert got == Counter(EXPECTED[mode])
