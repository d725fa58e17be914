"""The MFMA decode products (``kernel="mfma"``; csrc/gemv_mma.hip) on poisoned, guard-banded buffers (tests/guarded.py, used as it is),
as tests/test_gpu_decode_rows_guarded.py runs the VALU kernels: weight rows past N re-read row N - 1 and are never stored, K pieces
past the end of a wave's range are zeros in registers (nothing is loaded for them, from the weights or from the staged rows), columns
>= B of the MFMA are zero registers and never stored, and the results of the rows lie side by side in ``y`` -- flush against the rear
guard after the last one.  The result is bit-identical to the plain call."""
import pytest
import torch

import guarded
from test_gpu_decode_rows_guarded import _operands

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
_ID = lambda c: f"{c[0]}x{c[1]}_b{c[2]}_{'f16' if c[3] == F16 else 'bf16'}"
NATIVE_CASES = [(N, K, B, dt) for (N, K) in ((37, 1544), (24, 14336)) for B in (1, 3, 8) for dt in (F16, BF16)]
W8_CASES = [(N, K, B, dt) for (N, K) in ((17, 16), (37, 1552)) for B in (1, 3, 8) for dt in (F16, BF16)]


@pytest.mark.parametrize("case", NATIVE_CASES, ids=_ID)
def test_gemv_mma_rows_guarded(cuda, case):
    """Plain (with a bias) and the three fused forms."""
    from rsvld_amd import decode_rows as DR
    w, rest = _operands(cuda, *case)

    def fn(w, x, b, nw, res, gu):
        kw = dict(kernel="mfma")
        return (DR.gemv_rows(w, x, b, **kw), DR.gemv_rows(w, x, None, norm=(nw, 1e-5), **kw), DR.gemv_rows(w, x, None, residual=res, **kw),
                DR.gemv_rows(w, gu, None, glu=True, residual=res, **kw))
    guarded.run_guarded(fn, dict(w=w, **rest), expect="gemv_mma_rows")


@pytest.mark.parametrize("case", W8_CASES, ids=_ID)
def test_gemv_w8_mma_rows_guarded(cuda, case):
    from rsvld_amd import decode_rows as DR, w8
    w, rest = _operands(cuda, *case)
    q, scale = w8.pack_rows_e4m3(w)

    def fn(q, scale, x, b, nw, res, gu):
        kw = dict(kernel="mfma")
        return (DR.gemv_w8_rows(q, scale, x, b, **kw), DR.gemv_w8_rows(q, scale, x, None, norm=(nw, 1e-5), **kw),
                DR.gemv_w8_rows(q, scale, x, None, residual=res, **kw), DR.gemv_w8_rows(q, scale, gu, None, glu=True, residual=res, **kw))
    guarded.run_guarded(fn, dict(q=q, scale=scale, **rest), expect="gemv_w8_mma_rows")
