"""tests/ref64.py on the CPU: the tap-wise float64 convolution against oracle.functions (NumPy, im2col) and against
torch.nn.functional.conv3d + autograd, square and rectangular frames; and the comparator against planted faults that a global
rel-L2 at the tolerance lets through."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import ref64
from oracle import functions as F

STRIDE, PAD = (1, 2, 2), (0, 1, 1)


def _to_dev_act(a):                                     # (N,C,T,H,W) -> [N][T][H][W][C]
    return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 2, 3, 4, 1)))


def _to_dev_w(w):                                       # (Co,Ci,kt,4,4) -> [Co][kt][4][4][Ci]
    return torch.from_numpy(np.ascontiguousarray(w.transpose(0, 2, 3, 4, 1)))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


# (N, Ci real, Ci stored, Co, kt, T, H, W)
CASES = [
    (2, 3, 4, 6, 4, 7, 12, 12),          # the clip: three channels padded to four, Co not a power of two
    (3, 3, 4, 10, 1, 1, 8, 8),
    (2, 5, 5, 7, 4, 5, 16, 8),           # H > W
    (2, 8, 8, 12, 4, 6, 4, 32),          # H < W
    (3, 6, 6, 5, 1, 1, 16, 8),
    (3, 3, 4, 6, 1, 1, 4, 32),
]


@pytest.mark.parametrize("case", CASES, ids=["N%d-Ci%d(%d)-Co%d-kt%d-T%d-%dx%d" % c for c in CASES])
def test_ref64_matches_the_oracle_and_torch(case):
    N, ci, cip, Co, kt, T, H, W = case
    rng = np.random.RandomState(sum(case))
    x = rng.randn(N, ci, T, H, W)
    w = rng.randn(Co, ci, kt, 4, 4)
    b = rng.randn(Co)
    xp = np.zeros((N, cip, T, H, W))
    xp[:, :ci] = x
    wp = np.zeros((Co, cip, kt, 4, 4))
    wp[:, :ci] = w
    xd, wd = _to_dev_act(xp), _to_dev_w(wp)
    y = ref64.fprop(xd, wd, torch.from_numpy(b))
    assert y.dtype == torch.float64 and tuple(y.shape) == (N, T - kt + 1, H // 2, W // 2, Co)
    y_o = F.conv3d_fwd(x, w, b, STRIDE, PAD)
    gy = rng.randn(*y_o.shape)
    gx_o, gw_o, _ = F.conv3d_bwd(x, w, gy, STRIDE, PAD)
    gyd = _to_dev_act(gy)
    gx = ref64.dgrad(gyd, wd, T, H, W)
    dw = ref64.wgrad(xd, gyd, kt)
    # torch + autograd, float64
    xt, wt, bt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w, b))
    yt = TF.conv3d(xt, wt, bt, stride=STRIDE, padding=PAD)
    yt.backward(torch.from_numpy(gy))
    y_n = y.permute(0, 4, 1, 2, 3).numpy()
    gx_n = gx.permute(0, 4, 1, 2, 3).numpy()
    dw_n = dw.permute(0, 4, 1, 2, 3).numpy()
    for name, got, oracle, tch in (("y", y_n, y_o, yt), ("gx", gx_n[:, :ci], gx_o, xt.grad), ("dw", dw_n[:, :ci], gw_o, wt.grad)):
        assert _rel(got, oracle) < 1e-12, (name, "oracle")
        assert _rel(got, tch.detach().numpy()) < 1e-12, (name, "torch")
    # the padded channel stays out of it: its input gradient sees zero filters, its filter gradient zero input
    if cip > ci:
        assert np.abs(gx_n[:, ci:]).max() == 0.0 and np.abs(dw_n[:, ci:]).max() == 0.0


def test_ref64_float32_loops_are_a_float32_computation():
    """dtype=torch.float32 runs the same loops in float32 (how a test measures what plain fp32 summation gives on its data)"""
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn((2, 4, 8, 16, 8), generator=g), torch.randn((6, 4, 4, 4, 8), generator=g)
    y32 = ref64.fprop(x, w, dtype=torch.float32)
    assert y32.dtype == torch.float32
    r = ref64.compare(y32, ref64.fprop(x, w))
    assert 1e-9 < r.rel < 1e-6, str(r)


# ---------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------
M, C, TOL = 200000, 128, 1e-5


@pytest.fixture(scope="module")
def big_ref():
    g = torch.Generator().manual_seed(7)
    return torch.randn((M, C), generator=g, dtype=torch.float64)


def _global_rel(got, ref):
    return float(torch.linalg.vector_norm(got.double() - ref) / torch.linalg.vector_norm(ref))


def test_comparator_passes_a_float32_rounding(big_ref):
    r = ref64.compare(big_ref.float(), big_ref)
    print(r)
    assert r.ok(TOL) and r.rel < 1e-7 and r.block < 2 * r.rel, str(r)
    assert abs(r.rel - _global_rel(big_ref.float(), big_ref)) < 1e-3 * r.rel


def test_comparator_catches_one_scaled_block(big_ref):
    """(a) one 256 x 64 block scaled by 1 + 2e-4: 2e-4 * sqrt(256 * 64 / (200000 * 128)) = 5e-6 globally -- under the 1e-5 a
    forward pass is held to; the block itself is off by 2e-4 = 20 x the tolerance"""
    got = big_ref.float().double()
    r0, c0 = 256 * 317, 64
    got[r0:r0 + 256, c0:c0 + 64] *= 1 + 2e-4
    assert _global_rel(got, big_ref) < TOL                              # the global check alone lets it through
    r = ref64.compare(got, big_ref)
    print(r)
    assert r.rel < TOL and not r.ok(TOL)
    assert r.rows == (r0, r0 + 256) and r.cols == (c0, c0 + 64) and 1.5e-4 < r.block < 2.5e-4, str(r)


def test_comparator_catches_a_block_written_to_the_wrong_rows(big_ref):
    """(b) one 256-row block replaced by the next one: the block is off by sqrt(2) of its norm whatever the tensor's length, while
    the global figure, sqrt(2) * sqrt(256 / M), sinks with M -- 5e-2 here, 8.7e-3 at the 6.8 M rows of D_V.dc1's output at 512
    clips: inside the 2e-2 band the bf16 configuration is held to elsewhere"""
    got = big_ref.float().double()
    r0 = 256 * 500
    got[r0:r0 + 256] = got[r0 + 256:r0 + 512].clone()
    r = ref64.compare(got, big_ref)
    print(r)
    assert abs(r.rel - 2 ** 0.5 * (256.0 / M) ** 0.5) < 2e-3
    assert not r.ok(TOL) and not r.ok(1e-4)
    assert r.rows == (r0, r0 + 256) and abs(r.block - 2 ** 0.5) < 0.1, str(r)
    # the same fault in a tensor 34 times as long: the global figure passes a 2e-2 bound, the block figure is unchanged
    rel_long = 2 ** 0.5 * (256.0 / (34 * M)) ** 0.5
    assert rel_long < 2e-2 and r.block > ref64.BLOCK_FACTOR * 2e-2


def test_comparator_partial_blocks_nan_and_filter_view():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn((1000, 70), generator=g, dtype=torch.float64)    # 1000 = 3 * 256 + 232 rows, 70 = 64 + 6 columns
    got = ref.clone()
    got[999, 69] += 1.0
    r = ref64.compare(got, ref)
    assert r.rows == (768, 1000) and r.cols == (64, 70), str(r)
    assert abs(r.block - 1.0 / (float(torch.linalg.vector_norm(ref)) * (232 * 6 / 70000.0) ** 0.5)) < 1e-9
    got[5, 5] = float('nan')
    r = ref64.compare(got, ref)
    assert not r.ok(1e30) and r.rows == (0, 256) and r.cols == (0, 64), str(r)
    # a filter gradient [Co][kt][4][4][Ci] seen as [Co][kt*16*Ci]
    dw = torch.randn((128, 4, 4, 4, 64), generator=g, dtype=torch.float64)
    bad = dw.clone()
    bad[64:128, 1] *= 1.5
    r = ref64.compare(bad, dw, cols=4 * 16 * 64)
    assert r.shape == (128, 4096) and r.rows == (0, 128) and 1024 <= r.cols[0] < 2048, str(r)
