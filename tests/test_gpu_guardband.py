"""Guard-band runs of the convolution entry points (the GPU box has no AddressSanitizer; this is the substitute).

Every operand and output of a launch lives inside one poisoned arena (tests/guard.py): a consumed load that leaves its tensor
makes the result NaN, a store that leaves its tensor changes a margin.  For every pass x tile code x precision the library
accepts: (1) the output is finite and matches the float64 oracle, (2) every margin still holds the poison, (3) the inputs and
the outputs of EARLIER launches are unchanged (a stray store inside another tensor), (4) a second launch on the same inputs
reproduces the first bit for bit (fprop / dgrad) or to summation order (wgrad: fp32 atomics over the pixel splits).

Written after round 3's driver run: a weight gradient differed by 1.6e-4 between two launches that must agree
(test_gpu_ops.py::test_bf16_stored_operands_equal_rounding_in_the_kernel[0-case2]) on one box and not on others."""
import numpy as np
import pytest
import torch

from oracle import functions as F
from guard import Arena

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 1e-5, 1e-4


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return Arena(192 << 20)


def L():
    import mocogan_chainer_amd.layout as layout
    return layout


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def rel_l2(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _same(a, b):
    """'' when the tensors are bit-identical, else a description of where they differ"""
    if torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)):
        return ''
    d = (a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)).view(a.shape)
    idx = d.nonzero()
    return "%d of %d elements differ (%d NaN in a, %d in b); first at %s: %r vs %r; last-axis indices %s; max |a-b| %.3e" % (
        idx.shape[0], a.numel(), int(torch.isnan(a).sum()), int(torch.isnan(b).sum()), idx[0].tolist(),
        float(a[tuple(idx[0].tolist())]), float(b[tuple(idx[0].tolist())]), sorted(set(idx[:, -1].tolist()))[:16],
        float((a.double() - b.double()).abs().nan_to_num(1e30).max()))


def _bf16_round(a):
    return torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16).double().numpy()


GUARD_CASES = [
    # N, Ti, H (or (H, W)), Ci, Co, kt
    (2, 4, 8, 64, 160, 4),      # round 3's red case: Mpix = 32 < BK, Co not a multiple of the tile
    (2, 7, 16, 8, 64, 4),       # narrow 3-D layer
    (2, 5, 16, 3, 64, 4),       # the clip: 3 channels padded to 4
    (2, 5, 32, 3, 64, 4),       # Ci = 4, Wo = 16: the first-layer kernels
    (3, 1, 16, 128, 64, 1),     # ragged 256-row tile; Co = 64
    (1, 5, 8, 256, 256, 4),     # M = 32: one nearly empty tile, long K
    (5, 1, 4, 32, 256, 1),      # tiny spatial extent, M not a multiple of any tile
    (2, 9, 8, 16, 20, 4),       # Co not a power of two
    (2, 7, 32, 64, 128, 4),     # D_V dc2's geometry: the patch-stationary input gradient
    (5, 1, 8, 128, 512, 1),     # four N tiles
    (3, 5, 16, 128, 128, 4),    # 128 channels on both sides, ragged 256-row tiles, 3-D
    (2, 5, (64, 32), 3, 64, 4), # H != W (given as a pair): the clip with Wo = 16 and four row bands per frame of the first-layer kernels
    (2, 4, (8, 32), 64, 128, 4),    # H < W on a wide layer
]
TILES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 101, 203, 1103, 2203, 1007, 2010]
_refs = {}


def _frame(H):
    """(H, W) of a case: square unless the case gives a pair"""
    return H if isinstance(H, tuple) else (H, H)


def _case_data(case):
    """seeded bf16-representable inputs (every precision then computes the same exact products) and the oracle's results"""
    if case not in _refs:
        N, Ti, H, Ci, Co, kt = case
        H, Wd = _frame(H)
        rng = np.random.RandomState(4000 + GUARD_CASES.index(case))
        x = _bf16_round(rng.uniform(-1, 1, (N, Ci, Ti, H, Wd)))
        W = _bf16_round(rng.randn(Co, Ci, kt, 4, 4) * 0.1)
        gy = _bf16_round(rng.randn(N, Co, Ti - kt + 1, H // 2, Wd // 2))
        y_ref = F.conv3d_fwd(x, W, None, (1, 2, 2), (0, 1, 1))
        gx_ref, gW_ref, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
        _refs[case] = (x, W, gy, y_ref, gx_ref, gW_ref)
    return _refs[case]


def _operands(hl, prec, xd, wd, gyd, kt, Ci):
    """(x, w for fprop, w for dgrad, gy) in the memory form of the precision"""
    if prec == 'bf16s':
        w16 = wd.to(torch.bfloat16)
        return xd.to(torch.bfloat16), w16, w16, gyd.to(torch.bfloat16)
    if prec == 'f32x3':
        return hl.split_planes(xd), hl.split_planes(wd), hl.split_planes(wd, run=16 * kt * 16 * Ci), hl.split_planes(gyd)
    if prec == 'bf16y':                                            # the clip-side layers of bf16 networks: y bf16 beside fp32 x and w
        return xd, wd, wd, gyd.to(torch.bfloat16)
    return xd, wd, wd, gyd


@pytest.mark.parametrize("case", GUARD_CASES)
@pytest.mark.parametrize("prec", ['f32', 'bf16', 'bf16s', 'f32x3', 'bf16y'])
def test_conv_launches_stay_inside_their_tensors(hl, arena, case, prec):
    N, Ti, H, Ci, Co, kt = case
    H, Wd = _frame(H)
    lay = L()
    x, W, gy, y_ref, gx_ref, gW_ref = _case_data(case)
    xd0, wd0, gyd0 = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), lay.act_to_dev(dev(gy))
    Cip = xd0.shape[-1]
    if prec == 'f32x3' and (Cip % 16 or Co % 16):
        pytest.skip("the split form needs groups of 16 channels")
    if prec == 'bf16s' and (Cip % 8 or Co % 8):
        pytest.skip("a 16-byte slot of a bf16 tensor is 8 channels")
    if prec == 'bf16y' and Co % 8:
        pytest.skip("a 16-byte slot of the bf16 y tensor is 8 channels")
    ops0 = _operands(hl, prec, xd0, wd0, gyd0, kt, Cip)
    ran = []
    for tile in TILES:
        arena.reset()
        xa, wa, wda, ga = (arena.put(t) for t in ops0)
        snap = [t.clone() for t in (xa, wa, wda, ga)]
        g = hl.make_geom(N, Ti, H, Wd, Cip, Co, kt, precision=prec, ci_valid=Ci if Cip != Ci else 0)
        g.tile = tile
        kept = []                                          # (name, tensor in the arena, copy taken right after its launch)

        def after(name, out, ref, tol, scale=1.0):
            arena.check()
            assert bool(torch.isfinite(out).all()), (name, tile, "a consumed load left its tensor (NaN poison) or an element was not written")
            for t, s in zip((xa, wa, wda, ga), snap):
                assert torch.equal(t.view(torch.int16), s.view(torch.int16)), (name, tile, "an input was modified")
            for nm, t, c in kept:
                assert torch.equal(t, c), (name, tile, "the output of the earlier %s launch was modified" % nm)
            err = rel_l2(ref[0](out), ref[1] * scale)
            assert err < tol, (name, tile, err)
            kept.append((name, out, out.clone()))
            ran.append((name, tile))

        # ---- forward ----
        try:
            yd = arena.empty((N, g.To, g.Ho, g.Wo, Co))
            hl.conv_fprop(g, xa, wa, None, yd)
            after('fprop', yd, (lambda t: lay.act_from_dev(t, Co), y_ref), FWD_TOL)
            y2 = arena.empty((N, g.To, g.Ho, g.Wo, Co))
            hl.conv_fprop(g, xa, wa, None, y2)
            arena.check()
            if tile < 1000:
                assert not _same(y2, yd), ('fprop', tile, "two launches on the same inputs differ", _same(y2, yd))
        except hl.McgError:
            pass
        # ---- input gradient ----
        try:
            gxd = arena.empty((N, Ti, H, Wd, Cip))
            hl.conv_dgrad(g, ga, wda, None, gxd)
            after('dgrad', gxd, (lambda t: lay.act_from_dev(t, Ci), gx_ref), BWD_TOL)
            if Cip != Ci:
                assert float(gxd[..., Ci:].abs().max()) == 0.0
            gx2 = arena.empty((N, Ti, H, Wd, Cip))
            hl.conv_dgrad(g, ga, wda, None, gx2)
            arena.check()
            if tile < 1000:
                assert not _same(gx2, gxd), ('dgrad', tile, "two launches on the same inputs differ", _same(gx2, gxd))
        except hl.McgError:
            pass
        # ---- weight gradient (adds onto dw) ----
        if tile < 1000:
            try:
                dwd = arena.zeros(tuple(wd0.shape))
                hl.conv_wgrad(g, xa, ga, dwd)
                after('wgrad', dwd, (lambda t: lay.conv_w_from_dev(t, Ci, 3), gW_ref), BWD_TOL)
                first = dwd.clone()
                dw2 = arena.zeros(tuple(wd0.shape))
                hl.conv_wgrad(g, xa, ga, dw2)
                arena.check()
                # exact products of bf16-representable inputs, fp32 sums over <= a few thousand pixels: the order of the
                # atomics moves the last bits only
                assert rel_l2(dw2, first.cpu().double().numpy()) < 1e-6, ('wgrad', tile, "two launches on the same inputs differ")
            except hl.McgError:
                pass
    assert any(t == 0 for _, t in ran), "the library's own tile choice must run for every case"
