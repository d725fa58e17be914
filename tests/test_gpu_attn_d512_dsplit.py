"""The two shared-tile d = 512 attention kernels (keys = values = one tensor, the SR3 form) agree bit for bit.

attn_d512b (a wave owns 32 query rows over all 512 head dims) and attn_d512d (the same scores and online softmax; PV split by
head dim, P exchanged through LDS) accumulate every output element from the same MFMA products in the same order, with the same
rescale factors and row sums, so which one runs is a speed decision only (include/rsvld_hip.h, RSVLD_ATTN_D512_*)."""
import pytest
import torch

from test_gpu_kernels import attn_plan

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]

# (B, Nq, Nk, plan_div, spike): Nk in {4 096, 65 536, 262 144}; a ragged last key tile; Nq not a multiple of 128; B = 2 planned
# per image; split-KV (small query grids) and unsplit (>= 192 query tiles); spike = a key block of large norm in the middle of
# the sequence, so that the deferred running max of the rows that see it moves there (alpha != 1 on a late tile)
CASES = [
    (1, 4096, 4096, 1, False),          # split-KV
    (1, 65536, 65536, 1, True),         # unsplit (512 query tiles), late max move
    (1, 1000, 262144, 1, True),         # 262 144 keys, Nq % 128 != 0
    (1, 300, 4096 + 17, 1, True),       # ragged last tile in the last range
    (1, 24576 + 77, 2048 + 5, 1, False),  # unsplit with a ragged last tile and a partial query tile
    (2, 640, 8192 + 31, 2, True),       # B = 2 planned per image (plan_div 2)
]
RANGES = [8, 1, 16, 15, 1, 16]          # key ranges of each case: what the library's plan must say (asked in the test)


@pytest.fixture
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _run(q, x, kernel, plan_div):
    from rsvld_amd import devtools, ops
    try:
        devtools.d512_kernel(kernel)
        with ops.plan_units(plan_div):
            return ops.attention(q, x, x, heads=1)
    finally:
        devtools.d512_kernel("")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,Nq,Nk,plan_div,spike", CASES)
def test_attention_d512_dsplit_equals_rows_kernel_bit_for_bit(cuda, dtype, B, Nq, Nk, plan_div, spike):
    D = 512
    for tune, row in ((0, "d512d"), (5, "d512d"), (4, "d512b_shared")):     # RSVLD_ATTN_D512_*: default, dsplit, rows
        plan = attn_plan(B, 1, Nq, Nk, D, plan_div=plan_div, tune=tune, shared=True)
        assert (plan.name, plan.nsplit) == (row, RANGES[CASES.index((B, Nq, Nk, plan_div, spike))])
    g = torch.Generator().manual_seed(Nq * 7 + Nk)
    q = torch.randn(B, Nq, D, generator=g)
    x = torch.randn(B, Nk, D, generator=g)
    if spike:   # keys aligned with some queries, 8x their norm: those rows' max jumps by far more than 2^8 mid-sequence
        k0 = Nk // 2 + 3
        x[:, k0:k0 + 9] = q[:, 5:14] * 8.0
        x[-1, Nk - 2] = q[-1, Nq - 1] * 6.0   # and one in the last tile, for the last query row
    q, x = q.to(cuda, dtype), x.to(cuda, dtype)
    rows = _run(q, x, "rows", plan_div)
    dsplit = _run(q, x, "dsplit", plan_div)
    default = _run(q, x, "", plan_div)
    assert bool(torch.isfinite(rows).all())
    assert torch.equal(rows, dsplit)
    assert torch.equal(dsplit, default)
    if spike:   # the spike really dominates the rows that see it (the rescale path ran)
        ref = x[0, Nk // 2 + 3].float()
        assert float((rows[0, 5].float() - ref).abs().max()) < 0.05 * float(ref.abs().max())


def test_attention_d512_dsplit_plan_div_is_batch_invariant(cuda):
    """An image's result does not depend on how many images share the launch (plan_div), in the d-split kernel too."""
    D, Nq, Nk = 512, 384, 6000
    g = torch.Generator().manual_seed(3)
    q = torch.randn(2, Nq, D, generator=g).to(cuda, torch.float16)
    x = torch.randn(2, Nk, D, generator=g).to(cuda, torch.float16)
    both = _run(q, x, "dsplit", 2)
    one = _run(q[1:].contiguous(), x[1:].contiguous(), "dsplit", 1)
    assert torch.equal(both[1:], one)
