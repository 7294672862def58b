"""Op-level parity: every C-ABI entry point of libmocogan_hip.so against the float64 oracle on
seeded inputs.  Tolerances: forward rel-L2 <= 1e-5, gradients <= 1e-4 (fp32 MFMA vs
float64)."""
import numpy as np
import pytest
import torch

from oracle import functions as F
from oracle import net as onet
from oracle import updater as oupd
from oracle import philox

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 1e-5, 1e-4


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


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


CONV_CASES = [
    # N, Ti, H, Ci, Co, kt
    (2, 7, 16, 8, 64, 4),
    (2, 5, 16, 3, 64, 4),      # first layer: 3 channels padded to 4
    (3, 1, 16, 16, 32, 1),     # 2-D, Co < tile
    (2, 4, 8, 64, 160, 4),     # Co not a multiple of the tile
    (5, 1, 4, 32, 256, 1),     # tiny spatial extent, M not a multiple of the tile
    (2, 5, 32, 3, 64, 4),      # Ci = 4, Co = 64, Wo % 16 == 0: the VALU dgrad kernel (tile 0), 3-D
    (3, 1, 32, 3, 64, 1),      # the same, 2-D
    (2, 6, 16, 8, 8, 4),       # narrow 3-D layer (n_filters = 4 nets of the step tests): K-steps straddle temporal taps
    (2, 9, 8, 16, 20, 4),      # Co not a power of two, 3-D, every temporal phase t & 3
]


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 101, 103, 201, 202, 203])     # 1xx / 2xx force BK = 32 / 64
def test_conv_three_passes(hl, case, tile):
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(hash(case) % 2**31)
    x = rng.uniform(-1, 1, (N, Ci, Ti, H, H))
    W = rng.randn(Co, Ci, kt, 4, 4) * 0.1
    b = rng.randn(Co)
    stride, pad = (1, 2, 2), (0, 1, 1)
    y_ref = F.conv3d_fwd(x, W, b, stride, pad)
    gy = rng.randn(*y_ref.shape)
    gx_ref, gW_ref, _ = F.conv3d_bwd(x, W, gy, stride, pad)

    lay = L()
    xd, wd, bd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b)
    Cip = xd.shape[-1]
    g = hl.make_geom(N, Ti, H, H, Cip, Co, kt)
    hl.set_tile_override(tile)
    try:
        yd = torch.empty((N, g.To, g.Ho, g.Wo, Co), device="cuda")
        hl.conv_fprop(g, xd, wd, bd, yd)
        assert rel_l2(lay.act_from_dev(yd, Co), y_ref) < FWD_TOL

        gyd = lay.act_to_dev(dev(gy))
        gxd = torch.full_like(xd, 7.0)
        hl.conv_dgrad(g, gyd, wd, None, gxd)
        assert rel_l2(lay.act_from_dev(gxd, Ci), gx_ref) < BWD_TOL
        if Cip != Ci:
            assert float(gxd[..., Ci:].abs().max()) == 0.0      # padded channels: zero weights -> zero gradient

        hl.conv_dgrad(g, gyd, wd, None, gxd, accumulate=True)
        assert rel_l2(lay.act_from_dev(gxd, Ci), 2 * gx_ref) < BWD_TOL

        dwd = torch.zeros_like(wd)
        hl.conv_wgrad(g, xd, gyd, dwd)
        hl.conv_wgrad(g, xd, gyd, dwd)                           # accumulates
        assert rel_l2(lay.conv_w_from_dev(dwd, Ci, 3), 2 * gW_ref) < BWD_TOL
    finally:
        hl.set_tile_override(0)


RECT_FRAMES = [(16, 64), (64, 16), (8, 32), (128, 32), (64, 32)]       # (Hi, Wi)
RECT_LAYERS = {                                                          # N, Ti, Ci, Co, kt
    "first-3d": (2, 5, 3, 64, 4),      # Ci = 3 -> 4, Co = 64: the first-layer kernels (tile 0 and 6) where Wo is 16 or 32
    "first-2d": (3, 1, 3, 64, 1),
    "wide": (2, 5, 64, 128, 4),
}
SPECIALISED_TILES = (6, 7, 8, 10)      # kernels with limits of their own: a refusal (MCG_ERR_UNSUPPORTED) is an answer, a wrong number is not


def _form_exists(layer, prec):
    """bf16s: a 16-byte slot of a bf16 tensor is 8 channels; f32x3: the split form needs groups of 16 channels"""
    _, _, Ci, Co, _ = RECT_LAYERS[layer]
    Cip = (Ci + 3) // 4 * 4
    return not (prec == "f32x3" and (Cip % 16 or Co % 16)) and not (prec == "bf16s" and (Cip % 8 or Co % 8))


RECT_CASES = [(f, l, p) for f in RECT_FRAMES for l in sorted(RECT_LAYERS) for p in ("f32", "bf16", "bf16s", "f32x3") if _form_exists(l, p)]


@pytest.mark.parametrize("frame,layer,prec", RECT_CASES, ids=["%dx%d-%s-%s" % (f + (l, p)) for f, l, p in RECT_CASES])
def test_conv_three_passes_on_rectangular_frames(hl, frame, layer, prec):
    """mcg_conv_geom takes Hi and Wi separately; every other geometry in the tests is square, so a swapped lgHo / lgWo or a
    row-band halo of the WO = 16 first-layer instantiations (more than one band per frame only when Ho > 8) would go unseen.
    Hi != Wi both ways, Wo = 8 / 16 / 32, Ho from 4 to 64; the tile list of test_conv_three_passes plus the specialised kernels'
    codes; three passes against tests/ref64.py in float64 at the tolerances of test_conv_three_passes (bf16 / bf16s on
    bf16-representable inputs, as test_conv_three_passes_bf16_mfma (1)); the precisions are those whose form exists for the layer
    (RECT_CASES).  The generic tiles and tile 0 must run everywhere, tile 6 wherever the first-layer kernels' predicate admits the
    frame; only the specialised kernels may answer a geometry outside their limits with a refusal."""
    import ref64
    Hi, Wi = frame
    N, Ti, Ci, Co, kt = RECT_LAYERS[layer]
    Cip = (Ci + 3) // 4 * 4
    gen = torch.Generator(device="cuda")
    gen.manual_seed(Hi * 1000 + Wi + Ci + kt)
    exact = prec in ("bf16", "bf16s")
    rnd = lambda shape, s=1.0: (lambda t: t.to(torch.bfloat16).float() if exact else t)(torch.randn(shape, device="cuda", generator=gen) * s)
    x, w, b = rnd((N, Ti, Hi, Wi, Cip)), rnd((Co, kt, 4, 4, Cip), 0.1), torch.randn(Co, device="cuda", generator=gen)
    if Cip != Ci:
        x[..., Ci:] = 0
        w[..., Ci:] = 0
    g0 = hl.make_geom(N, Ti, Hi, Wi, Cip, Co, kt, precision=prec, ci_valid=Ci if Cip != Ci else 0)
    gy = rnd((N, g0.To, g0.Ho, g0.Wo, Co))
    y_ref, gx_ref, dw_ref = ref64.fprop(x, w, b), ref64.dgrad(gy, w, Ti, Hi, Wi), ref64.wgrad(x, gy, kt)
    if prec == "bf16s":
        xs, wf, wd, ys = x.to(torch.bfloat16), w.to(torch.bfloat16), w.to(torch.bfloat16), gy.to(torch.bfloat16)
    elif prec == "f32x3":
        xs, wf, wd, ys = hl.split_planes(x), hl.split_planes(w), hl.split_planes(w, run=16 * kt * 16 * Cip), hl.split_planes(gy)
    else:
        xs, wf, wd, ys = x, w, w, gy
    tiles = [0, 7, 8, 10] if prec == "f32x3" else [0, 1, 2, 3, 4, 5, 101, 103, 201, 202, 203] + ([6] if Cip == 4 else [7, 8, 10])
    bad, ran, refused = [], [], []
    for tile in tiles:
        g = hl.with_precision(g0, prec)
        g.tile = tile
        for kind in ("fprop", "dgrad", "wgrad"):
            try:
                if kind == "fprop":
                    out = torch.full(y_ref.shape, 3.0, device="cuda")
                    hl.conv_fprop(g, xs, wf, b, out)
                    rep, tol = ref64.compare(out, y_ref), FWD_TOL
                elif kind == "dgrad":
                    out = torch.full(gx_ref.shape, 7.0, device="cuda")
                    hl.conv_dgrad(g, ys, wd, None, out)
                    rep, tol = ref64.compare(out, gx_ref), BWD_TOL
                    if Cip != Ci and float(out[..., Ci:].abs().max()) != 0.0:
                        bad.append("dgrad tile %d: the padded channel is not zero" % tile)
                else:
                    out = torch.zeros_like(w)
                    hl.conv_wgrad(g, xs, ys, out)
                    hl.conv_wgrad(g, xs, ys, out)                    # accumulates
                    rep, tol = ref64.compare(out, 2 * dw_ref, cols=kt * 16 * Cip), BWD_TOL
            except hl.McgError as e:
                if tile not in SPECIALISED_TILES:
                    bad.append("%s tile %d refused: %s" % (kind, tile, e))
                refused.append((kind, tile))
                continue
            ran.append((kind, tile))
            if not rep.rel < tol:
                bad.append("%s tile %d: %s" % (kind, tile, rep))
    print("%dx%d %s %s: ran %d launches, refused %s" % (Hi, Wi, layer, prec, len(ran), refused))
    assert not bad, "\n".join(bad)
    assert all((k, 0) in ran for k in ("fprop", "dgrad", "wgrad"))
    if Cip == 4 and g0.Wo in (16, 32) and g0.Ho % (128 // g0.Wo) == 0:
        # the frames the first-layer kernels' dispatch predicate admits (Wo 16 or 32, Ho a multiple of the 128 / Wo row band;
        # several bands per frame at 128x32 and 64x32): tile 6 must really run them -- forward and input gradient in both forms,
        # the weight gradient on fp32 operands (its bf16 form is 'bf16y': tests/test_gpu_guardband.py's 64x32 row)
        must = [("fprop", 6), ("dgrad", 6)] + ([("wgrad", 6)] if prec == "f32" else [])
        assert all(m in ran for m in must), "the first-layer kernels (tile 6) did not run: %r refused" % refused


def _bf16_round(a):
    """round-to-nearest-even to bf16, returned as float64 (what v_cvt_pk_bf16_f32 does to an fp32 operand)"""
    return torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16).double().numpy()


BF16_TOL = 2e-2      # bf16 configuration, forward rel-L2 <= 2e-2


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 101, 102, 103, 201, 202, 203])
def test_conv_three_passes_bf16_mfma(hl, case, tile):
    """precision = bf16: operands are rounded to bf16 in the kernel, products accumulate in fp32.
    (1) On inputs that are already bf16-representable the rounding is the identity, so the result must
    match the float64 oracle as tightly as the fp32 path does -- this pins the operand layout of the
    32x32x16 MFMA and of the transposing LDS reads.  (2) On general fp32 inputs the result is within the
    bf16 tolerance of the oracle."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(hash(case) % 2**31 + 1)
    stride, pad = (1, 2, 2), (0, 1, 1)
    lay = L()
    hl.set_tile_override(tile)
    try:
        for exact in (True, False):
            x = rng.uniform(-1, 1, (N, Ci, Ti, H, H))
            W = rng.randn(Co, Ci, kt, 4, 4) * 0.1
            b = rng.randn(Co)
            gy = rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2)
            if exact:
                x, W, gy = _bf16_round(x), _bf16_round(W), _bf16_round(gy)
            y_ref = F.conv3d_fwd(x, W, b, stride, pad)
            gx_ref, gW_ref, _ = F.conv3d_bwd(x, W, gy, stride, pad)
            ftol, btol = (FWD_TOL, BWD_TOL) if exact else (BF16_TOL, BF16_TOL)

            xd, wd, bd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b)
            g = hl.make_geom(N, Ti, H, H, xd.shape[-1], Co, kt, precision='bf16')
            yd = torch.empty((N, g.To, g.Ho, g.Wo, Co), device="cuda")
            hl.conv_fprop(g, xd, wd, bd, yd)
            assert rel_l2(lay.act_from_dev(yd, Co), y_ref) < ftol
            gyd = lay.act_to_dev(dev(gy))
            gxd = torch.full_like(xd, 7.0)
            hl.conv_dgrad(g, gyd, wd, None, gxd)
            assert rel_l2(lay.act_from_dev(gxd, Ci), gx_ref) < btol
            dwd = torch.zeros_like(wd)
            hl.conv_wgrad(g, xd, gyd, dwd)
            assert rel_l2(lay.conv_w_from_dev(dwd, Ci, 3), gW_ref) < btol
    finally:
        hl.set_tile_override(0)


def test_conv_tile_field_and_autotune(hl):
    """mcg_conv_geom.tile selects the block tile per call (no process-global state), bad codes are rejected,
    and the autotuner (times the candidates on scratch, keeps the winner) leaves results and accumulators
    untouched."""
    N, Ti, H, Ci, Co, kt = 2, 6, 16, 16, 96, 4
    rng = np.random.RandomState(5)
    x = rng.uniform(-1, 1, (N, Ci, Ti, H, H))
    W = rng.randn(Co, Ci, kt, 4, 4) * 0.1
    y_ref = F.conv3d_fwd(x, W, None, (1, 2, 2), (0, 1, 1))
    gy = rng.randn(*y_ref.shape)
    gx_ref, gW_ref, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
    lay = L()
    xd, wd, gyd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), lay.act_to_dev(dev(gy))
    for code in (1, 2, 3, 101, 203, 1103, 2203, 1202, 2001):       # 1xxx / 2xxx: 2- / 4-way split-K in fprop
        g = hl.make_geom(N, Ti, H, H, Ci, Co, kt)
        g.tile = code
        yd = torch.full((N, g.To, g.Ho, g.Wo, Co), 3.0, device="cuda")          # split-K must clear y itself
        bd = dev(rng.randn(Co))
        hl.conv_fprop(g, xd, wd, bd, yd)
        assert rel_l2(lay.act_from_dev(yd, Co), y_ref + bd.cpu().double().numpy().reshape(1, Co, 1, 1, 1)) < FWD_TOL, code
    for code in (1203, 2103, 2202):                                  # split-K in dgrad: plain and accumulating
        g = hl.make_geom(N, Ti, H, H, Ci, Co, kt)
        g.tile = code
        gxd = torch.full_like(xd, 5.0)
        hl.conv_dgrad(g, gyd, wd, None, gxd)                         # must clear x itself
        assert rel_l2(lay.act_from_dev(gxd, Ci), gx_ref) < BWD_TOL, code
        hl.conv_dgrad(g, gyd, wd, None, gxd, accumulate=True)
        assert rel_l2(lay.act_from_dev(gxd, Ci), 2 * gx_ref) < BWD_TOL, code
        dwd = torch.zeros_like(wd)
        hl.conv_wgrad(g, xd, gyd, dwd)                               # wgrad: 1xxx / 2xxx = more / fewer pixel splits
        assert rel_l2(lay.conv_w_from_dev(dwd, Ci, 3), gW_ref) < BWD_TOL, code
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt)
    g.tile = 7
    with pytest.raises(hl.McgError):
        hl.conv_fprop(g, xd, wd, None, yd)

    hl.set_autotune(True, use_pretuned=False)
    try:
        g = hl.make_geom(N, Ti, H, H, Ci, Co, kt)
        before = len(hl.tile_choices())
        for rep in range(2):                                      # second round: cache hits
            yd = torch.empty((N, g.To, g.Ho, g.Wo, Co), device="cuda")
            hl.conv_fprop(g, xd, wd, None, yd)
            assert rel_l2(lay.act_from_dev(yd, Co), y_ref) < FWD_TOL
            gxd = torch.ones_like(xd)
            hl.conv_dgrad(g, gyd, wd, None, gxd, accumulate=True)  # tuning must not accumulate into gxd
            assert rel_l2(lay.act_from_dev(gxd, Ci), gx_ref + 1.0) < BWD_TOL
            dwd = torch.zeros_like(wd)
            hl.conv_wgrad(g, xd, gyd, dwd)                        # ... nor into dwd
            assert rel_l2(lay.conv_w_from_dev(dwd, Ci, 3), gW_ref) < BWD_TOL
        assert len(hl.tile_choices()) == before + 3
        assert g.tile == 0                                        # the caller's geometry is not modified
    finally:
        hl.set_autotune(False)


def test_conv_frame_view_and_frame_permutation(hl):
    """x[:, :, t] as the x side (model/updater.py:97) and the (T,N)->(N,T) output permutation of the
    generator's last layer (model/updater.py:102)."""
    lay = L()
    rng = np.random.RandomState(11)
    N, T, H, C, Co, t = 3, 5, 16, 3, 64, 2
    clip = rng.uniform(-1, 1, (N, C, T, H, H))
    W = rng.randn(Co, C, 4, 4) * 0.1
    y_ref = F.conv2d_fwd(clip[:, :, t], W, None, 2, 1)
    clipd = lay.act_to_dev(dev(clip))                       # [N][T][H][W][4]
    g = hl.make_geom(N, 1, H, H, 4, Co, 1, x_stride0=T * H * H * 4)
    yd = torch.empty((N, 1, H // 2, H // 2, Co), device="cuda")
    hl.conv_fprop(g, clipd[:, t], lay.conv_w_to_dev(dev(W)), None, yd)
    assert rel_l2(lay.act_from_dev(yd, Co, 2), y_ref) < FWD_TOL

    # deconv forward of T*N frames written straight into clip order, with bias + tanh
    for Ci_d, H in ((16, 16), (64, 32)):                    # GEMM path / VALU path (Ci = 4, Co = 64, Wo = 16)
        _deconv_into_clip_order(hl, lay, rng, N, T, H, C, Ci_d)


def _deconv_into_clip_order(hl, lay, rng, N, T, H, C, Ci_d):
    xin = rng.randn(T * N, Ci_d, H // 2, H // 2)
    Wd = rng.randn(Ci_d, C, 4, 4) * 0.1
    bd = rng.randn(C) * 0.1
    out_ref = np.tanh(F.deconv2d_fwd(xin, Wd, bd, 2, 1)).reshape(T, N, C, H, H).transpose(1, 2, 0, 3, 4)
    g2 = hl.make_geom(T * N, 1, H, H, 4, Ci_d, 1, x_stride0=T * H * H * 4, x_perm_n=N, x_stride1=H * H * 4)
    outd = torch.zeros((N, T, H, H, 4), device="cuda")
    hl.conv_dgrad(g2, lay.act_to_dev(dev(xin)), lay.deconv_w_to_dev(dev(Wd)), lay.vec_to_dev(dev(bd)), outd, act=hl.ACT_TANH)
    assert rel_l2(lay.act_from_dev(outd, C), out_ref) < FWD_TOL


def test_conv_rejects_bad_geometry(hl):
    g = hl.make_geom(1, 4, 12, 12, 4, 64, 4)                # Ho = 6 is not a power of two
    x = torch.zeros(1, device="cuda")
    with pytest.raises(hl.McgError):
        hl.conv_fprop(g, x, x, None, x)
    g = hl.make_geom(1, 4, 16, 16, 3, 64, 4)                # unpadded channel count
    with pytest.raises(hl.McgError):
        hl.conv_fprop(g, x, x, None, x)
    with pytest.raises(hl.McgError):
        hl.conv_fprop(hl.make_geom(1, 4, 16, 16, 4, 64, 4), torch.zeros(1), x, None, x)   # host tensor


@pytest.mark.parametrize("M,K,Co", [(4, 512, 1), (3, 2048, 7), (32, 1024, 60),
                                    (512, 8192, 60), (100, 1024, 60), (77, 2048, 20),     # M >= 64, Co >= 16: the MFMA GEMM path
                                    (64, 32768, 7), (64, 8192, 7), (64, 32768, 1),        # D_V / D_I dc5 at the batch-32 step's 2n rows (infogan: 7)
                                    (512, 32768, 1), (5, 64, 3),                          # ... at the batch-256 step's; fewer rows than slices
                                    # G's dc1 at n_hidden = 50 + dim_zm off the default 60, and the thresholds of the three dispatches.
                                    # fprop: GEMM | dot product per block; dgrad: eight rows | one row per block; wgrad (no db): GEMM | row slices
                                    (64, 1024, 62),      # GEMM with Co % 4 != 0 | eight rows, Co % 4 != 0 (its loop is unrolled by 4) | row slices: Co % 4 != 0 at M >= 64
                                    (80, 1024, 66),      # GEMM, a second column tile, a ragged second row tile | eight rows | row slices
                                    (64, 1024, 114),     # GEMM, two column tiles, Co % 4 != 0 | eight rows | row slices
                                    (72, 1024, 68),      # GEMM, Co > 64 | eight rows (M % 8 == 0, M % 64 != 0) | GEMM with Co > 64, M no multiple of its K-step
                                    (64, 96, 20),        # dot products after the GEMM refuses K % 64 != 0 | eight rows | GEMM, two ragged tiles of K
                                    (64, 1024, 8),       # dot products (Co < 16) | eight rows at their smallest Co | row slices
                                    (63, 1024, 16),      # one row short of every M threshold: dot products | one row per block | row slices
                                    (64, 1024, 16)])     # exactly on every threshold: GEMM | eight rows | GEMM
def test_fc_ops(hl, M, K, Co):
    rng = np.random.RandomState(M * 7 + Co)
    x, w, b, gy = rng.randn(M, K), rng.randn(Co, K) * 0.05, rng.randn(Co), rng.randn(M, Co)
    xd, wd, bd, gyd = dev(x), dev(w), dev(b), dev(gy)
    yd = torch.empty((M, Co), device="cuda")
    hl.fc_fprop(M, K, Co, xd, wd, bd, yd)
    errs = {'fprop': rel_l2(yd, x @ w.T + b)}
    yd = torch.full((M, Co), float('nan'), device="cuda")
    hl.fc_fprop(M, K, Co, xd, wd, None, yd)
    errs['fprop, no bias'] = rel_l2(yd, x @ w.T)
    period = 64 if K % 64 == 0 else 32                           # (the period divides K: K = 96)
    bias_k = rng.randn(period)
    gxd = torch.empty((M, K), device="cuda")
    hl.fc_dgrad(M, K, Co, gyd, wd, dev(bias_k), period, gxd)
    errs['dgrad'] = rel_l2(gxd, gy @ w + np.tile(bias_k, K // period))
    gxd = torch.full((M, K), float('nan'), device="cuda")
    hl.fc_dgrad(M, K, Co, gyd, wd, None, 0, gxd)                # the discriminators' last layer: no bias plane behind it
    errs['dgrad, no bias'] = rel_l2(gxd, gy @ w)
    dwd = torch.ones((Co, K), device="cuda")
    hl.fc_wgrad(M, K, Co, xd, gyd, dwd)
    errs['wgrad'] = rel_l2(dwd, gy.T @ x + 1)
    dwd, dbd = torch.ones((Co, K), device="cuda"), torch.ones(Co, device="cuda")      # with the bias gradient (the row-sliced kernel)
    hl.fc_wgrad(M, K, Co, xd, gyd, dwd, dbd)
    errs['wgrad with db'], errs['db'] = rel_l2(dwd, gy.T @ x + 1), rel_l2(dbd, gy.sum(0) + 1)
    print("fc M=%d K=%d Co=%d:" % (M, K, Co), " ".join("%s %.2e" % kv for kv in errs.items()))
    for k, v in errs.items():                                       # (measured first, then held: a failure leaves every figure behind)
        assert v < (BWD_TOL if k in ('wgrad', 'wgrad with db', 'db') else FWD_TOL), (k, v)


@pytest.mark.parametrize("C,M,act", [(64, 5000, 2), (128, 777, 1), (512, 64, 2), (256, 4096, 1)])
def test_batchnorm_activation_fwd_bwd(hl, C, M, act):
    rng = np.random.RandomState(C + M)
    y = rng.randn(M, C) * 1.7 + 0.3
    gamma, beta = 1 + 0.1 * rng.randn(C), 0.1 * rng.randn(C)
    noise = 0.2 * rng.randn(M, C)
    am, av = np.zeros(C), np.ones(C)
    y4 = y.T.reshape(1, C, M, 1)                                  # oracle layout (N,C,H,W)
    bn, cache = F.bn_train_fwd(y4, gamma, beta, am, av)
    out_ref = (F.leaky_relu_fwd(bn) if act == 2 else F.relu_fwd(bn))
    ws = torch.empty(hl.bn_workspace_floats(C), device="cuda")
    yd, gd, bd = dev(y), dev(gamma), dev(beta)
    stats = torch.empty(4 * C, device="cuda")
    amd, avd = dev(am * 0), dev(av * 0 + 1)
    hl.bn_stats(M, C, yd, gd, bd, stats, amd, avd, ws)
    assert rel_l2(stats[:C], cache['mean']) < 1e-5 and rel_l2(stats[C:2 * C], cache['inv_std']) < 1e-5
    assert rel_l2(amd, am) < 1e-5 and rel_l2(avd, av) < 1e-5
    outd = torch.empty_like(yd)
    hl.bn_act_fwd(M, C, yd, stats[2 * C:], act, outd, addend=dev(noise))
    assert rel_l2(outd, out_ref[0, :, :, 0].T + noise) < FWD_TOL

    g_out = rng.randn(M, C)
    g4 = g_out.T.reshape(1, C, M, 1)
    g_bn = F.leaky_relu_bwd(out_ref, g4) if act == 2 else F.relu_bwd(out_ref, g4)
    gamma_new = gamma * 1.01                                      # Q5: backward sees the updated gamma
    gx_ref, gg_ref, gb_ref = F.bn_train_bwd(cache, gamma_new, g_bn)
    dg, db = torch.ones(C, device="cuda"), torch.ones(C, device="cuda")
    gxd = torch.empty_like(yd)
    hl.bn_act_bwd(M, C, dev(g_out), yd, stats, dev(gamma_new), act, gxd, dg, db, ws)
    assert rel_l2(gxd, gx_ref[0, :, :, 0].T) < BWD_TOL
    assert rel_l2(dg, gg_ref + 1) < BWD_TOL and rel_l2(db, gb_ref + 1) < BWD_TOL
    # no-BN form (D's first layer): lrelu only
    hl.bn_act_bwd(M, C, dev(g_out), yd, None, None, hl.ACT_LRELU, gxd, None, None, ws)
    assert rel_l2(gxd, F.leaky_relu_bwd(F.leaky_relu_fwd(y), g_out)) < 1e-6
    cs = torch.ones(C, device="cuda")
    hl.colsum_acc(M, C, dev(g_out), cs, ws)
    assert rel_l2(cs, g_out.sum(0) + 1) < 1e-5


def _act64(v, act):
    return (v, np.maximum(v, 0), np.where(v >= 0, v, 0.2 * v), np.tanh(v))[act]


def _bn_edge_fwd_bwd(hl, M, C, bf16, bn, act, seed, scale_shift=False, addend=False, sigma=0.0, split=False):
    """Every form of bn_act_fwd / bn_act_bwd that the library accepts at one shape.  The all-fp32 form is held against float64;
    every other form -- bf16 output, bf16 inputs (the same numbers as the fp32 run's), split output -- against that, bit for bit."""
    rng = np.random.RandomState(seed)
    bf, f32 = torch.bfloat16, torch.float32
    y, g = dev(rng.randn(M, C) * 1.5 + 0.3), dev(rng.randn(M, C))
    gamma, beta = 1 + 0.1 * rng.randn(C), 0.1 * rng.randn(C)
    yb = y.to(bf)
    if bf16:
        y = yb.float()
    y64 = y.double().cpu().numpy()
    ws = torch.empty(hl.bn_workspace_floats(C), device="cuda")
    stats = None
    if bn:
        stats, am, av = torch.empty(4 * C, device="cuda"), torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        hl.bn_stats(M, C, y, dev(gamma), dev(beta), stats, am, av, ws)
        mean, var = y64.mean(0), y64.var(0) + 2e-5
        istd = 1 / np.sqrt(var)
        sc, sh = gamma * istd, beta - mean * gamma * istd
        for got, want in zip(stats.view(4, C), (mean, istd, sc, sh)):
            assert rel_l2(got, want) < 1e-5
        assert rel_l2(am, 0.1 * mean) < 1e-5 and rel_l2(av, 0.9 + 0.1 * var * M / max(M - 1, 1)) < 1e-5
        ss = stats[2 * C:]
    elif scale_shift:
        sc, sh = 1 + 0.1 * rng.randn(C), 0.1 * rng.randn(C)
        ss = dev(np.concatenate([sc, sh]))
    else:
        sc, sh, ss = np.ones(C), np.zeros(C), None
    pre = y64 * sc + sh
    # the incoming gradient is zero where the pre-activation lies within 1e-4 of the activation's kink: the sign of an fp32 value
    # that close to zero is not the float64 value's, and one flipped mask is worth more than BWD_TOL of the whole tensor
    g = g * dev(np.abs(pre) > 1e-4)
    gb = g.to(bf)
    if bf16:
        g = gb.float()
    g64 = g.double().cpu().numpy()
    forms = [(False, f32), (False, bf)] + ([(True, f32), (True, bf)] if bf16 else [])      # (inputs held in bf16, output type)

    add = dev(0.2 * rng.randn(M, C)) if addend else None

    def fwd(in16, odt, sig=0.0, split_out=False):
        o = torch.full((M, 4 * C), 7.0, device="cuda", dtype=bf) if split_out else torch.empty((M, C), device="cuda", dtype=odt)
        hl.bn_act_fwd(M, C, yb if in16 else y, ss, act, o, addend=add, sigma=sig, seed=11, stream_id=5, split_out=split_out)
        return o

    o32 = fwd(False, f32)
    assert rel_l2(o32, _act64(pre, act) + (add.double().cpu().numpy() if addend else 0)) < FWD_TOL
    for sig in (0.0, sigma) if sigma else (0.0,):
        base = fwd(False, f32, sig)
        if sig:             # element e takes normal e of the stream (fma(sigma, z, v) here, sigma * z rounded first in mcg_randn:
            z = torch.empty(M * C, device="cuda")                       # 1.5 ulp of |v| < 32 apart at the most)
            hl.randn(z, sig, 11, 5)
            assert float((base - (o32 + z.view(M, C))).abs().max()) < 4e-6
        for in16, odt in forms[1:]:
            assert torch.equal(fwd(in16, odt, sig), base.to(odt)), ("fwd", in16, odt, sig)
    if split:
        want = hl.split_planes(o32, out=torch.full((M, 4 * C), 7.0, device="cuda", dtype=bf))
        assert torch.equal(fwd(False, None, split_out=True).view(torch.int16), want.view(torch.int16))

    gamma2 = dev(gamma * 1.01) if bn else None

    def bwd(in16, odt, split_out=False):
        o = torch.full((M, 4 * C), 7.0, device="cuda", dtype=bf) if split_out else torch.empty((M, C), device="cuda", dtype=odt)
        dg, db = (torch.ones(C, device="cuda"), torch.ones(C, device="cuda")) if bn else (None, None)
        hl.bn_act_bwd(M, C, gb if in16 else g, yb if in16 else y, stats, gamma2, act, o, dg, db, ws, split_out=split_out)
        return o, dg, db

    if not bn:
        gx32 = bwd(False, f32)[0]
        assert rel_l2(gx32, g64 * (1 - y64 * y64) if act == 3 else np.where(y64 > 0, g64, (0, 0, 0.2)[act] * g64)) < BWD_TOL
        for in16, odt in forms[1:]:
            assert torch.equal(bwd(in16, odt)[0], gx32.to(odt)), ("bwd", in16, odt)
        return
    gbn, xh = g64 * np.where(pre > 0, 1.0, (0, 0, 0.2)[act]), (y64 - mean) * istd
    gg, gbeta = (gbn * xh).sum(0), gbn.sum(0)
    gx_ref = 1.01 * gamma * istd * (gbn - (xh * gg + gbeta) / M)
    for in16 in (False, True) if bf16 else (False,):
        # fp32 and bf16 inputs sum the per-channel partials in different trees: each against float64, the bf16 output against
        # the fp32 output of the same inputs
        gx32, dg, db = bwd(in16, f32)
        assert rel_l2(gx32, gx_ref) < BWD_TOL and rel_l2(dg, gg + 1) < BWD_TOL and rel_l2(db, gbeta + 1) < BWD_TOL, in16
        gx16, dg16, db16 = bwd(in16, bf)
        assert torch.equal(gx16, gx32.to(bf)) and torch.equal(dg16, dg) and torch.equal(db16, db), in16
        if split and not in16:
            # The split gradient comes from the eight-wide apply kernel, the fp32 one from the four-wide.  Both now compute
            # fmaf(-xh, k1, gb) - k2 (written out in the kernel; the compiler used to contract gb - xh * k1 differently in the
            # two), but in the eight-wide one the compiler still fuses the last product k0 * (...) into the subtraction of the
            # first plane, so mid and lo carry bits BELOW the fp32 value's last: the planes are neither split_planes(gx32) nor the
            # split form of any fp32 tensor (measured at this shape before the fma was written out: 35 of 592 values differ
            # from gx32, by up to 6 ulp; hi + mid + lo is no fp32 number for 518 of them).  The forward pass, whose
            # fmaf is written out, is held to split_planes above.  Held here: the same per-channel sums; the first plane equal to
            # the bf16 output of the same kernel, bit for bit; each further plane within half a bf16 ulp of the one before (what
            # "the bf16 rounding of what the planes before left" means for the sizes); their sum against float64 and, to fp32
            # accuracy, against gx32; the padding plane untouched.
            gxs, dgs, dbs = bwd(False, None, split_out=True)
            assert torch.equal(dgs, dg) and torch.equal(dbs, db)
            hi, mid, lo, pad = (gxs.view(M, C // 16, 4, 16)[:, :, i].float() for i in range(4))
            half_ulp = lambda t: torch.ldexp(torch.ones_like(t), torch.frexp(t).exponent - 9)      # of a bf16 value (8 significant bits)
            assert bool((pad == 7.0).all()) and torch.equal(hi.reshape(M, C).to(bf), gx16)
            assert bool((mid.abs() <= half_ulp(hi)).all()) and bool((lo.abs() <= half_ulp(mid)).all())
            v = (hi.double() + mid.double() + lo.double()).reshape(M, C).cpu().numpy()
            assert rel_l2(v, gx_ref) < BWD_TOL and rel_l2(v, gx32.double().cpu().numpy()) < FWD_TOL
    if bf16:                # one input in bf16, the other the same numbers in fp32
        for g_in, y_in in ((gb, y), (g, yb)):
            o, dg, db = torch.empty((M, C), device="cuda"), torch.ones(C, device="cuda"), torch.ones(C, device="cuda")
            hl.bn_act_bwd(M, C, g_in, y_in, stats, gamma2, act, o, dg, db, ws)
            assert rel_l2(o, gx_ref) < BWD_TOL and rel_l2(dg, gg + 1) < BWD_TOL and rel_l2(db, gbeta + 1) < BWD_TOL


EW_THREADS = 2048 * 256           # an element-wise grid is capped at this many threads: beyond as many channel groups a thread takes more than one
BN_EDGE_CASES = {
    "one-group": dict(M=1, C=4, bf16=False, bn=False, act=3),
    "one-eight-wide-column": dict(M=37, C=8, bf16=True, bn=True, act=2),
    "smallest-split-output": dict(M=37, C=16, bf16=False, bn=True, act=1, split=True),
    "paired-trips-w4": dict(M=EW_THREADS + 300, C=4, bf16=False, bn=False, act=2, scale_shift=True, addend=True),
    "paired-trips-w8": dict(M=EW_THREADS + 300, C=8, bf16=True, bn=True, act=2, sigma=0.2),
    "moving-channel-group": dict(M=175000, C=12, bf16=False, bn=False, act=2, scale_shift=True),
}


@pytest.mark.parametrize("case", list(BN_EDGE_CASES) + ["padded-channel", "frame-view", "refusals"])
def test_bn_elementwise_edge_shapes(hl, case):
    """The smallest shapes at which each path of the BatchNorm / activation passes can go wrong: a single group (one thread, the
    pair loop's tail branch), one eight-channel column (more row lanes than rows in the partial sums), the smallest split output,
    more groups than a capped grid has threads (full pairs and half pairs in one launch, four and eight channels per thread), a
    channel count whose groups move between a thread's trips (per-channel constants reloaded), the masked pad channel, the
    frame-strided source view, and the shapes the library refuses."""
    if case in BN_EDGE_CASES:
        _bn_edge_fwd_bwd(hl, seed=list(BN_EDGE_CASES).index(case), **BN_EDGE_CASES[case])
        return
    torch.manual_seed(4)
    if case == "padded-channel":
        M, C = 1000, 4
        y = torch.randn((M, C), device="cuda")
        o3, o4 = torch.empty_like(y), torch.empty_like(y)
        hl.bn_act_fwd(M, C, y, None, hl.ACT_LRELU, o3, sigma=0.2, seed=7, stream_id=3, c_valid=3)
        hl.bn_act_fwd(M, C, y, None, hl.ACT_LRELU, o4, sigma=0.2, seed=7, stream_id=3, c_valid=4)
        assert torch.equal(o3[:, :3], o4[:, :3]) and torch.equal(o3[:, 3], torch.where(y[:, 3] >= 0, y[:, 3], 0.2 * y[:, 3]))
        assert not torch.equal(o3[:, 3], o4[:, 3])
    elif case == "frame-view":
        items, frames, rows, C = 6, 3, 5, 8                      # frame 1 of a [items][frames][rows][C] tensor
        M = items * rows
        ss = torch.cat([1 + 0.1 * torch.randn(C, device="cuda"), 0.1 * torch.randn(C, device="cuda")])
        for dt in (torch.float32, torch.bfloat16):
            clip = torch.randn((items, frames, rows, C), device="cuda").to(dt)
            view, dense = clip[:, 1], clip[:, 1].contiguous()
            assert view.data_ptr() == clip.data_ptr() + rows * C * clip.element_size() and not view.is_contiguous()
            for sigma in (0.0, 0.2):
                ov, od = torch.empty((M, C), device="cuda"), torch.empty((M, C), device="cuda")
                hl.bn_act_fwd(M, C, view, ss, hl.ACT_LRELU, ov, sigma=sigma, seed=7, stream_id=3, rows_per_item=rows, item_stride=frames * rows * C)
                hl.bn_act_fwd(M, C, dense.view(M, C), ss, hl.ACT_LRELU, od, sigma=sigma, seed=7, stream_id=3)
                assert torch.equal(ov, od), (dt, sigma)
                if sigma == 0.0:
                    pre = dense.view(M, C).double().cpu().numpy() * ss[:C].double().cpu().numpy() + ss[C:].double().cpu().numpy()
                    assert rel_l2(ov, _act64(pre, 2)) < FWD_TOL
    else:
        M = 64
        ws = torch.empty(hl.bn_workspace_floats(64), device="cuda")
        y, g = torch.randn((M, 24), device="cuda"), torch.randn((M, 24), device="cuda")
        gamma, beta, stats = torch.ones(24, device="cuda"), torch.zeros(24, device="cuda"), torch.zeros(4 * 24, device="cuda")
        with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):           # 6 channel quads do not divide a block
            hl.bn_stats(M, 24, y, gamma, beta, stats, None, None, ws)
        with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
            hl.bn_act_bwd(M, 24, g, y, stats, gamma, hl.ACT_LRELU, torch.empty_like(g), None, None, ws)
        y8, s8 = torch.randn((M, 8), device="cuda"), torch.zeros((M, 32), device="cuda", dtype=torch.bfloat16)
        with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):           # split output wants C % 16 == 0
            hl.bn_act_fwd(M, 8, y8, None, hl.ACT_RELU, s8, split_out=True)
        assert not bool(s8.any())
        C = 16                                                                   # split output over its own input gradient
        store = torch.zeros(M * C * 2, device="cuda")
        g16 = store[:M * C].view(M, C)
        alias = torch.empty(0, dtype=torch.bfloat16, device="cuda").set_(store.untyped_storage(), 0, (M, 4 * C), (4 * C, 1))
        assert alias.data_ptr() == g16.data_ptr()
        y16 = torch.randn((M, C), device="cuda")
        st = torch.cat([torch.zeros(C), torch.ones(C), torch.ones(C), torch.zeros(C)]).cuda()
        with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
            hl.bn_act_bwd(M, C, g16, y16, st, torch.ones(C, device="cuda"), hl.ACT_RELU, alias, None, None, ws, split_out=True)
        assert not bool(store.any())


def test_philox_noise_matches_oracle_stream(hl):
    n = 100003
    out = torch.empty(n, device="cuda")
    hl.randn(out, 0.2, 0x1234567887654321, 42)
    ref = philox.randn(n, 0.2, 0x1234567887654321, 42)
    assert np.abs(out.cpu().numpy() - ref).max() < 4e-6            # sigma = 0.2: 2e-5 per unit normal (hardware log2 / sin / cos)
    # the fused paths draw the SAME stream: lrelu(y) + sigma*randn, padded channel masked
    M, C = 1000, 4
    y = torch.randn(M, C, device="cuda")
    o = torch.empty_like(y)
    hl.bn_act_fwd(M, C, y, None, hl.ACT_LRELU, o, sigma=0.2, seed=7, stream_id=3, c_valid=3)
    z = philox.randn(M * C, 0.2, 7, 3).reshape(M, C)
    z[:, 3] = 0
    yl = torch.where(y >= 0, y, 0.2 * y).cpu().numpy()
    assert np.abs(o.cpu().numpy() - (yl + z)).max() < 5e-6


def test_pack_unpack_and_tanh_bwd_to_frames(hl):
    rng = np.random.RandomState(3)
    N, C, T, H = 3, 3, 5, 8
    x = rng.randn(N, C, T, H, H)
    noise = rng.randn(N, C, T, H, H)
    lay = L()
    out = torch.empty((N, T, H, H, 4), device="cuda")
    hl.pack_clip(N, C, 4, T, H * H, dev(x), out, addend=lay.act_to_dev(dev(noise)))
    assert rel_l2(lay.act_from_dev(out, C), x + noise) < 1e-6
    assert float(out[..., 3].abs().max()) == 0.0
    back = torch.empty((N, C, T, H, H), device="cuda")
    hl.unpack_clip(N, C, 4, T, H * H, out, back)
    assert rel_l2(back, x + noise) < 1e-6
    g = rng.randn(N, T, H, H, 4)
    xc = np.tanh(rng.randn(N, T, H, H, 4))
    gf = torch.empty((T * N, H, H, 4), device="cuda")
    hl.tanh_bwd_to_frames(N, T, H * H * 4, dev(g), dev(xc), gf)
    ref = (g * (1 - xc * xc)).transpose(1, 0, 2, 3, 4).reshape(T * N, H, H, 4)
    assert rel_l2(gf, ref) < 1e-6


@pytest.mark.parametrize("C,Cp", [(3, 4), (1, 4), (4, 4), (6, 8)])
def test_pack_clip_u8_equals_the_reference_normalisation(hl, C, Cp):
    """mcg_pack_clip_u8 on the loader's uint8 (N,T,H,W,C) clips against the reference's host arithmetic (datasets.py:95:
    (x - 128) / 128, then the (C,T,H,W) transpose of updater.py:87-92) -- exact: both are exact in fp32 -- and, bit for bit, against
    mcg_pack_clip on the float batch, with injected and with in-kernel Philox noise, for the clip and for one frame of every clip."""
    rng = np.random.RandomState(17)
    N, T, H = 3, 5, 8
    u8 = rng.randint(0, 256, (N, T, H, H, C)).astype(np.uint8)
    u8[0, 0, 0, 0, :] = 0
    u8[0, 0, 0, 1, :] = 255
    ref = ((u8.astype(np.float32) - 128.) / 128.).transpose(0, 4, 1, 2, 3)               # (N,C,T,H,W), what the reference feeds D
    xu, xf = torch.tensor(u8, device="cuda"), dev(ref).contiguous()       # (torch.tensor keeps a transposed NumPy view's strides)
    out = torch.full((N, T, H, H, Cp), 9.0, device="cuda")
    hl.pack_clip_u8(N, C, Cp, T, H * H, xu, out)
    got = out.cpu().numpy()
    assert np.array_equal(got[..., :C].transpose(0, 4, 1, 2, 3), ref) and float(out[..., C:].abs().sum()) == 0.0
    noise = torch.randn((N, T, H, H, Cp), device="cuda")
    for kw in (dict(addend=noise), dict(sigma=0.2, seed=11, stream_id=5)):
        a, b = torch.empty_like(out), torch.empty_like(out)
        hl.pack_clip_u8(N, C, Cp, T, H * H, xu, a, **kw)
        hl.pack_clip(N, C, Cp, T, H * H, xf, b, **kw)
        assert torch.equal(a, b), kw.keys()
        if 'sigma' in kw:
            assert float(a[..., C:].abs().sum()) == 0.0 and float((a - out).abs().max()) > 0.1
        t = 3                                                     # frame t of every clip (the ImageDiscriminator's input, updater.py:96-97)
        a1, b1 = torch.empty((N, 1, H, H, Cp), device="cuda"), torch.empty((N, 1, H, H, Cp), device="cuda")
        kw1 = dict(kw, addend=kw['addend'][:, :1].contiguous()) if 'addend' in kw else kw
        hl.pack_clip_u8(N, C, Cp, 1, H * H, xu[:, t], a1, stride_n=T * H * H * C, **kw1)
        hl.pack_clip(N, C, Cp, 1, H * H, xf[:, :, t], b1, stride_n=C * T * H * H, stride_c=T * H * H, **kw1)
        assert torch.equal(a1, b1)
        if 'addend' in kw:
            assert float((a1[:, 0] - kw1['addend'][:, 0] - out[:, t]).abs().max()) < 1e-6      # (frame t of the clip, up to the rounding of + / - noise)
    with pytest.raises(hl.McgError):
        hl.pack_clip_u8(N, C, Cp, T, H * H, xf, out)                # a float tensor is not the loader's form


def gru_branch(dz, dl):
    """Which kernel pair mcg_gru_seq_fwd / _bwd launch, restated from the words of include/mocogan_hip.h (dim_zm <= 16 and
    dim_zm + dim_zl <= 32: a thread's weight rows in registers; beyond, up to 64 / 128, the weights are read from memory) and of
    the host dispatch in csrc/small_ops.hip (the register kernels pad the input row, one-hot label + noise, to 16 or to 32)."""
    if dz <= 16 and dz + dl <= 16:
        return '<16>'
    if dz <= 16 and dz + dl <= 32:
        return '<32>'
    return 'wide'


GRU_BASE_CASES = [(5, 0, 10), (37, 6, 10), (7, 0, 24), (9, 6, 40), (3, 64, 64)]        # test_gru_sequence's rows: (N, dim_zl, dim_zm), T = 16

# (N, dim_zm, dim_zl, T) beside the branch the row is there for
GRU_BRANCH_CASES = [
    ('<16>', (17, 16, 0, 16)),        # every unit lane live; a second block with one sample
    ('<16>', (3, 1, 0, 2)),           # one unit
    ('<16>', (4, 10, 6, 1)),          # one step: nothing to prefetch
    ('<16>', (16, 10, 0, 24)),        # the sampler's other length; exactly one full block
    ('<32>', (17, 10, 7, 16)),        # the smallest input count past 16
    ('<32>', (5, 12, 6, 16)),         # --dim_zm 12 on the six MUG labels
    ('<32>', (33, 16, 16, 16)),       # every unit lane and every input column live; three blocks
    ('<32>', (6, 10, 22, 16)),        # the one-hot fill takes a second trip; in = 32
    ('<32>', (3, 16, 1, 16)),         # in = 17
    ('wide', (5, 17, 0, 16)),         # the smallest wide state
    ('wide', (5, 16, 17, 16)),        # wide by the input count alone (in = 33)
    ('wide', (6, 64, 0, 16)),         # the largest state, no labels
    ('wide', (5, 2, 126, 16)),        # the largest input count; the one-hot fill takes a second trip of 64
]


@pytest.fixture(scope="module")
def gru_arena():
    from guard import Arena
    return Arena(16 << 20)


def _gru_fwd_bwd(hl, arena, N, dz, dim_zl, T, seed):
    """mcg_gru_seq_fwd / _bwd inside guard bands against the oracle's StatelessGRU steps in float64: the state columns of z, the
    four saved vectors and every link's gradient each to a bound of their own; the zc columns bit for bit; dparams += (a second
    call doubles the first)."""
    rng = np.random.RandomState(seed)
    dc = 50
    p = onet.init_generator(rng, dim_zl=dim_zl, dim_zm=dz, n_filters=2, dtype=np.float64)
    gp = {k: (v + 0.1 * rng.randn(*v.shape)) for k, v in p.items() if k.startswith('g0/')}
    draw = onet.gen_draw(rng, N, dim_zl=dim_zl, dim_zm=dz, video_len=T, dtype=np.float64)
    if dim_zl and N >= 2:
        draw['labels'][0], draw['labels'][1] = 0, dim_zl - 1        # the first and the last column of the one-hot always occur
    # oracle: run the recurrence alone
    gpo = {k[3:]: v for k, v in gp.items()}
    zl = np.eye(dim_zl)[draw['labels']] if dim_zl else None
    h, hs, caches = draw['h0'], [], []
    for t in range(T):
        et = draw['e'][t] if zl is None else np.concatenate((zl, draw['e'][t]), 1)
        h, c = F.gru_step_fwd(gpo, h, et)
        hs.append(h), caches.append(c)
    z_ref = np.concatenate((np.tile(draw['zc'], (T, 1, 1)), np.stack(hs)), 2).reshape(T * N, dc + dz)
    lay = L()
    arena.reset()
    flat = arena.put(lay.gru_to_dev({k: dev(v) for k, v in gp.items()}))
    labels = arena.put(dev(draw['labels'], torch.int32)) if dim_zl else None
    h0, e, zc = arena.put(dev(draw['h0'])), arena.put(dev(draw['e'])), arena.put(dev(draw['zc']))
    z = arena.empty((T * N, dc + dz))                              # (poison: every element must be written)
    saved = arena.empty((T, N, 4 * dz))
    hl.gru_seq_fwd(N, T, dz, dim_zl, dc, flat, h0, e, labels, zc, z, saved)
    arena.check()
    tag = "gru N=%d dz=%d dl=%d T=%d %s:" % (N, dz, dim_zl, T, gru_branch(dz, dim_zl))
    errs = {'z': rel_l2(z, z_ref), 'state': rel_l2(z[:, dc:], np.stack(hs).reshape(T * N, dz))}
    for i, name in enumerate(('r', 'z', 'h_bar', 'h')):            # saved: [T][N][r | z | h_bar | h_prev]
        errs['saved ' + name] = rel_l2(saved[:, :, i * dz:(i + 1) * dz], np.stack([c[name] for c in caches]))
    print(tag, "fwd", " ".join("%s %.2e" % kv for kv in errs.items()))
    assert torch.equal(z[:, :dc], zc.repeat(T, 1))
    for k, v in errs.items():
        assert v < FWD_TOL, (k, v)
    gz = rng.randn(T * N, dc + dz)
    grads = {k: np.zeros_like(v) for k, v in gpo.items()}
    gh = np.zeros((N, dz))
    for t in reversed(range(T)):
        gh = gh + gz.reshape(T, N, -1)[t][:, dc:]
        gh, _ = F.gru_step_bwd(gpo, caches[t], gh, grads)
    gzd = arena.put(dev(gz))
    dflat = arena.zeros(tuple(flat.shape))
    for call in (1, 2):                                             # dparams +=: the second call adds the same gradient again
        hl.gru_seq_bwd(N, T, dz, dim_zl, dc, flat, e, labels, saved, gzd, dflat)
        arena.check()
        got = lay.gru_from_dev(dflat, dz, dim_zl, prefix='')
        errs = {k: rel_l2(got[k], call * grads[k]) for k in grads}
        print(tag, "bwd call %d" % call, " ".join("%s %.2e" % kv for kv in errs.items()))
        for k, v in errs.items():
            assert v < BWD_TOL, (call, k, v)


@pytest.mark.parametrize("N,dim_zl,dz", GRU_BASE_CASES)
def test_gru_sequence(hl, gru_arena, N, dim_zl, dz):
    """mcg_gru_seq_fwd / _bwd against the oracle's StatelessGRU steps: the register-resident kernels (dim_zm <= 16, the reference's
    default 10 with and without labels) and the wide-state pair (weights in memory: --dim_zm up to 64, model/net.py:38-41)."""
    _gru_fwd_bwd(hl, gru_arena, N, dz, dim_zl, 16, seed=N)


def test_gru_sequence_tables_reach_every_dispatch_branch():
    """the two tables the GRU tests are parametrised with, as they stand: a later edit of either cannot silently drop a branch"""
    from collections import Counter
    hit = Counter(gru_branch(dz, dl) for _, dl, dz in GRU_BASE_CASES) + Counter(gru_branch(dz, dl) for _, (_, dz, dl, _) in GRU_BRANCH_CASES)
    assert all(hit[b] >= 2 for b in ('<16>', '<32>', 'wide')), hit
    assert all(gru_branch(dz, dl) == b for b, (_, dz, dl, _) in GRU_BRANCH_CASES)


@pytest.mark.parametrize("branch,case", GRU_BRANCH_CASES, ids=["%s-N%d-zm%d-zl%d-T%d" % ((b,) + c) for b, c in GRU_BRANCH_CASES])
def test_gru_sequence_dispatch_branches(hl, gru_arena, branch, case):
    """Every kernel pair of the GRU dispatch at its boundaries (dim_zm 1, 16, 17, 64; 16, 17, 32, 33 and 128 inputs; one step and
    24).  Measured on an MI355X (worst over the rows, bounds 1e-5 / 1e-5 / 1e-4): profiles/generator_head_parity.md."""
    N, dz, dl, T = case
    assert gru_branch(dz, dl) == branch
    _gru_fwd_bwd(hl, gru_arena, N, dz, dl, T, seed=N + 100 * dz + 10000 * dl + 1000000 * T)


@pytest.mark.parametrize("C,with_ce", [(1, False), (7, False), (7, True)])
def test_losses(hl, C, with_ce):
    rng = np.random.RandomState(C)
    N = 19
    model = 'infogan' if C == 7 else 'normal'
    yr, yf = rng.randn(N, C, 1, 1, 1) * 3, rng.randn(N, C, 1, 1, 1) * 3
    tr, tf = rng.randint(0, 6, N), rng.randint(0, 6, N)
    l_ref, gr_ref, gf_ref = oupd.loss_dis(model, with_ce, yr, yf, tr, tf)
    loss = torch.empty(1, device="cuda")
    gr, gf = torch.empty((N, C), device="cuda"), torch.empty((N, C), device="cuda")
    hl.loss_dis(N, C, dev(yr.reshape(N, C)), dev(yf.reshape(N, C)), dev(tr, torch.int32), dev(tf, torch.int32), with_ce, loss, gr, gf)
    assert abs(float(loss) - l_ref) < 1e-5
    assert rel_l2(gr, gr_ref.reshape(N, C)) < 1e-5 and rel_l2(gf, gf_ref.reshape(N, C)) < 1e-5
    if C == 7 and not with_ce:
        return
    yi = rng.randn(N, C, 1, 1) * 3
    l_ref, gi_ref, gv_ref = oupd.loss_gen(model, yi, yf, tf)
    gi, gv = torch.empty((N, C), device="cuda"), torch.empty((N, C), device="cuda")
    hl.loss_gen(N, C, dev(yi.reshape(N, C)), dev(yf.reshape(N, C)), dev(tf, torch.int32), C == 7, loss, gi, gv)
    assert abs(float(loss) - l_ref) < 1e-5
    assert rel_l2(gi, gi_ref.reshape(N, C)) < 1e-5 and rel_l2(gv, gv_ref.reshape(N, C)) < 1e-5


SATURATED = np.array([-100, -20, -1e-3, 0, 1e-3, 20, 100], np.float32).astype(np.float64)     # (as the device holds them)


@pytest.mark.parametrize("N", [19, 300])
@pytest.mark.parametrize("C,with_ce", [(1, False), (7, False), (7, True)])
def test_losses_at_saturated_logits(hl, C, with_ce, N):
    """Logits where softplus and sigmoid leave their comfortable range: +-100 (exp overflows fp32 one way, the term vanishes the
    other), +-20 (1 + exp(-20) rounds to 1), +-1e-3 and 0.  Sample 0, the only one whose GAN term mcg_loss_dis evaluates, holds
    the extremes.  The loss is held to 1e-5 relative to max(1, |loss|) (it reaches the hundreds), every gradient element to
    1e-5 / N absolutely (an element is at most 2 / N; half of the reference underflows to zero, so a relative norm says nothing).
    Measured on an MI355X: profiles/generator_head_parity.md."""
    rng = np.random.RandomState(1000 * N + 10 * C + with_ce)
    model = 'infogan' if C == 7 else 'normal'
    yr, yf, yi = (SATURATED[rng.randint(0, 7, (N, C))] for _ in range(3))
    first = SATURATED if C == 7 else SATURATED[6:]
    yr[0], yf[0], yi[0] = first, first[::-1], first
    tr, tf = rng.randint(0, 6, N), rng.randint(0, 6, N)
    loss = torch.empty(1, device="cuda")
    ga, gb = torch.empty((N, C), device="cuda"), torch.empty((N, C), device="cuda")

    def check(what, refs):
        l_ref, ga_ref, gb_ref = refs
        l, da, db = float(loss), np.abs(ga.cpu().double().numpy() - ga_ref.reshape(N, C)).max(), np.abs(gb.cpu().double().numpy() - gb_ref.reshape(N, C)).max()
        print("%s C=%d ce=%d N=%d: loss %.9g ref %.9g, |d| / max(1, |ref|) %.2e; max |dg| * N %.2e %.2e" % (
            what, C, with_ce, N, l, l_ref, abs(l - l_ref) / max(1.0, abs(l_ref)), da * N, db * N))
        assert np.isfinite(l) and bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gb).all())
        assert abs(l - l_ref) <= 1e-5 * max(1.0, abs(l_ref))
        assert da <= 1e-5 / N and db <= 1e-5 / N

    hl.loss_dis(N, C, dev(yr), dev(yf), dev(tr, torch.int32), dev(tf, torch.int32), with_ce, loss, ga, gb)
    check("loss_dis", oupd.loss_dis(model, with_ce, yr.reshape(N, C, 1, 1, 1), yf.reshape(N, C, 1, 1, 1), tr, tf))
    if C == 7 and not with_ce:
        return
    hl.loss_gen(N, C, dev(yi), dev(yf), dev(tf, torch.int32), C == 7, loss, ga, gb)
    check("loss_gen", oupd.loss_gen(model, yi.reshape(N, C, 1, 1), yf.reshape(N, C, 1, 1, 1), tf))


def test_adam_weight_decay(hl):
    rng = np.random.RandomState(9)
    n = 10007
    p = {'x/W': rng.randn(n).astype(np.float32)}
    st = oupd.new_adam_state(p)
    pd, md, vd = dev(p['x/W']), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for t in (1, 2, 3):
        g = (rng.randn(n) * 10.0 ** rng.uniform(-9, 0, n)).astype(np.float32)
        oupd.adam_wd_update(p, {'x/W': g}, st)
        lr_t = oupd.ADAM_ALPHA * np.sqrt(1 - oupd.ADAM_BETA2 ** t) / (1 - oupd.ADAM_BETA1 ** t)
        hl.adam_wd(pd, dev(g), md, vd, lr_t, oupd.ADAM_BETA1, oupd.ADAM_BETA2, oupd.ADAM_EPS, oupd.WEIGHT_DECAY)
        assert np.abs(pd.cpu().numpy() - p['x/W']).max() < 1e-6


def _adam_grad_sums(W, n=10007, steps=3, seed=9):
    """p0 and, per step, the fp32 SUM of W gradients drawn as test_adam_weight_decay draws its one (what the all-reduce hands to Adam)"""
    rng = np.random.RandomState(seed + W)
    p0 = rng.randn(n).astype(np.float32)
    sums = []
    for _ in range(steps):
        acc = np.zeros(n, np.float32)
        for _ in range(W):
            acc += (rng.randn(n) * 10.0 ** rng.uniform(-9, 0, n)).astype(np.float32)
        sums.append(acc)
    return p0, sums


def _offset_tensor(a, offset, dtype=torch.float32):
    """a copy of `a` that starts `offset` elements past an aligned address"""
    buf = torch.zeros(len(a) + offset, dtype=dtype, device="cuda")
    out = buf[offset:]
    out.copy_(torch.as_tensor(a).to(dtype))
    assert out.data_ptr() % 16 == offset * out.element_size() % 16
    return out


def _adam_lr(t):
    return oupd.ADAM_ALPHA * np.sqrt(1 - oupd.ADAM_BETA2 ** t) / (1 - oupd.ADAM_BETA1 ** t)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_adam_grad_scale_against_float64(hl, W, offset):
    """grad_scale = 1 / W on the all-reduced SUM of W ranks' gradients is Adam on their mean: against the oracle's update in
    float64, fed g_sum / W formed in float64.  p to test_adam_weight_decay's 1e-6 absolute; m and v to rel-L2 1e-6, ten times the
    fp32 rounding (2^-24 = 6e-8 each) of the three fused operations behind each of them (g * gscale, the fma with wd * p, the
    fma of the moment; for v the square in place of the scaling) -- three steps do not add up, (1 - beta) of the old error stays."""
    p0, sums = _adam_grad_sums(W)
    p = {'x/W': p0.astype(np.float64)}
    st = oupd.new_adam_state(p)
    n = len(p0)
    pd, md, vd = _offset_tensor(p0, offset), _offset_tensor(np.zeros(n), offset), _offset_tensor(np.zeros(n), offset)
    for t, g_sum in enumerate(sums, 1):
        oupd.adam_wd_update(p, {'x/W': g_sum.astype(np.float64) / W}, st)
        hl.adam_wd(pd, _offset_tensor(g_sum, offset), md, vd, _adam_lr(t), oupd.ADAM_BETA1, oupd.ADAM_BETA2, oupd.ADAM_EPS, oupd.WEIGHT_DECAY,
                   grad_scale=1.0 / W)
        e_p = np.abs(pd.cpu().double().numpy() - p['x/W']).max()
        e_m, e_v = rel_l2(md, st['m']['x/W']), rel_l2(vd, st['v']['x/W'])
        print("PARITY adam_wd W=%d offset %d step %d: max |p - p64| %.2e (1e-6), m %.2e, v %.2e (rel-L2, 1e-6)" % (W, offset, t, e_p, e_m, e_v))
        assert e_p < 1e-6 and e_m < 1e-6 and e_v < 1e-6, (t, e_p, e_m, e_v)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("W", [2, 8])
def test_adam_grad_scale_equals_scaling_the_gradient(hl, W, offset):
    """1 / W is a power of two: g_sum * (1 / W) in the kernel and g_sum / W formed beforehand (then times 1.0f) are the same fp32
    number -- no gradient here is near the subnormal range -- so p, m, v and the bf16 copy come out bit for bit the same."""
    p0, sums = _adam_grad_sums(W)
    n = len(p0)
    a = [_offset_tensor(p0, offset), _offset_tensor(np.zeros(n), offset), _offset_tensor(np.zeros(n), offset),
         _offset_tensor(np.zeros(n), offset, torch.bfloat16)]
    b = [_offset_tensor(p0, offset), _offset_tensor(np.zeros(n), offset), _offset_tensor(np.zeros(n), offset),
         _offset_tensor(np.zeros(n), offset, torch.bfloat16)]
    for t, g_sum in enumerate(sums, 1):
        scaled = g_sum / np.float32(W)
        assert scaled.dtype == np.float32 and np.array_equal(scaled * np.float32(W), g_sum) and np.abs(scaled[scaled != 0]).min() > 1e-30
        args = (_adam_lr(t), oupd.ADAM_BETA1, oupd.ADAM_BETA2, oupd.ADAM_EPS, oupd.WEIGHT_DECAY)
        hl.adam_wd(a[0], _offset_tensor(g_sum, offset), a[1], a[2], *args, grad_scale=1.0 / W, p16=a[3])
        hl.adam_wd(b[0], _offset_tensor(scaled, offset), b[1], b[2], *args, grad_scale=1.0, p16=b[3])
        for name, x, y in zip(("p", "m", "v", "p16"), a, b):
            assert torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int16),
                               y.view(torch.int32 if y.dtype == torch.float32 else torch.int16)), (name, t)
    assert not torch.equal(a[0], torch.as_tensor(p0).cuda())


@pytest.mark.parametrize("n", [1, 5, 1027, 4 * 256 * 2048 + 7])
def test_randint_matches_oracle_stream(hl, n):
    """hl.randint against oracle.philox.randint, exactly: one element, a partial counter, several blocks with a partial last
    counter (n % 4 = 3), and more counters than a capped element-wise grid has threads (2048 x 256: a thread's second trip);
    moduli 1, 6 (the label count), an odd one and the largest positive int32; a seed and a stream id that need all 64 bits.  The
    n-element output lies between poisoned margins: the last counter's n % 4 words and nothing more are written."""
    from guard import Arena
    arena = Arena(((n * 4 + 255) // 256 * 256) + (4 << 16))
    seed, stream = 0xFEDCBA9876543210, 0x8123456789ABCDEF
    for modulus in (1, 6, 7, 2 ** 31 - 1):
        arena.reset()
        out = arena.empty((n,), torch.int32)
        hl.randint(out, modulus, seed, stream)
        arena.check()
        ref = philox.randint(n, modulus, seed, stream)
        got = out.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, ref), (modulus, int((got != ref).sum()), np.flatnonzero(got != ref)[:8])
        assert ref.min() >= 0 and ref.max() < modulus
    if n > 1000:                                    # (the stream is not a constant, and the four words of a counter differ)
        assert len(np.unique(ref[:1000])) > 900
    # another stream id or seed is another stream
    if n == 1027:
        out2 = torch.empty(n, dtype=torch.int32, device="cuda")
        hl.randint(out2, 2 ** 31 - 1, seed, stream ^ (1 << 63))
        assert not np.array_equal(out2.cpu().numpy(), ref) and np.array_equal(out2.cpu().numpy(), philox.randint(n, 2 ** 31 - 1, seed, stream ^ (1 << 63)))
        hl.randint(out2, 2 ** 31 - 1, seed ^ (1 << 32), stream)
        assert np.array_equal(out2.cpu().numpy(), philox.randint(n, 2 ** 31 - 1, seed ^ (1 << 32), stream))


def test_randint_refusals(hl):
    out = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(hl.McgError, match="MCG_ERR_BAD_ARG"):
        hl.randint(out, 0, 1, 2)
    with pytest.raises(hl.McgError, match="MCG_ERR_BAD_ARG"):
        hl.randint(out, -6, 1, 2)
    with pytest.raises(hl.McgError, match="MCG_ERR_BAD_ARG"):
        hl.randint(out[:0], 6, 1, 2)
    assert hl.load().mcg_randint(0, 6, 1, 2, hl._p(out, torch.int32), hl._stream()) == -1       # n = 0 with a real pointer
    assert bool((out == -7).all())


# ------------------------------------------------------------------------------------------------------------------
# fused conv epilogues (mcg_conv_fprop_ex / mcg_conv_dgrad_ex): each must reproduce what the stand-alone passes compute
# ------------------------------------------------------------------------------------------------------------------
EPI_CASES = [
    # N, Ti, H, Ci, Co, kt   (N even: two statistics groups)
    (4, 5, 16, 8, 64, 4),      # 3-D, one 64-column block
    (2, 1, 16, 16, 160, 1),    # 2-D, Co not a multiple of the tile, rows not a multiple of the tile
    (6, 4, 8, 64, 40, 4),      # a group boundary inside a block tile (6*1*4*4 = 96 rows, 48 per group)
    (2, 6, 32, 4, 8, 4),       # first-layer shape of a narrow net: Ci = 4, fewer than 32 output channels
]


def _mask_bits(mask, C):
    m = mask.cpu().numpy().astype(np.uint32)
    cols = np.arange(C)
    return ((m[:, cols >> 5] >> (cols & 31).astype(np.uint32)) & 1).astype(bool)


@pytest.mark.parametrize("case", EPI_CASES)
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 101, 203])
def test_fprop_epilogue_statistics_and_first_layer(hl, case, tile):
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(hash(case) % 2**31 + 7)
    x = rng.uniform(-1, 1, (N, Ci, Ti, H, H))
    W = rng.randn(Co, Ci, kt, 4, 4) * 0.1
    b = rng.randn(Co) * 0.3
    y_ref = F.conv3d_fwd(x, W, b, (1, 2, 2), (0, 1, 1))                   # (N,Co,To,Ho,Wo)
    lay = L()
    xd, wd, bd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b)
    for groups in (1, 2):
        g = hl.make_geom(N, Ti, H, H, xd.shape[-1], Co, kt)
        g.tile = tile
        M = N * g.To * g.Ho * g.Wo
        mg = M // groups
        # ---- (sum y, sum y^2) per channel and group -> BatchNorm statistics
        part = torch.full((hl.epilogue_part_floats(g, "fprop", groups),), float('nan'), device="cuda")
        ep = hl.epilogue(sums=hl.SUMS_STATS, groups=groups, part=part)
        yd = torch.empty((N, g.To, g.Ho, g.Wo, Co), device="cuda")
        assert hl.conv_fprop(g, xd, wd, bd, yd, ep=ep)
        assert rel_l2(lay.act_from_dev(yd, Co), y_ref) < FWD_TOL
        assert ep.n_slots > 0 and ep.slot_stride == groups * 2 * Co
        gamma, beta = 1 + 0.1 * rng.randn(Co), 0.1 * rng.randn(Co)
        ws = torch.empty(hl.bn_workspace_floats(max(Co, 64)), device="cuda")
        for gi in range(groups):
            yg = y_ref[gi * (N // groups):(gi + 1) * (N // groups)]
            am, av = np.zeros(Co), np.ones(Co)
            _, cache = F.bn_train_fwd(yg, gamma, beta, am, av)
            stats = torch.empty(4 * Co, device="cuda")
            amd, avd = dev(np.zeros(Co)), dev(np.ones(Co))
            hl.bn_stats_from_partials(mg, Co, part[gi * 2 * Co:], ep.n_slots, ep.slot_stride, dev(gamma), dev(beta), stats, amd, avd, ws)
            assert rel_l2(stats[:Co], cache['mean']) < 1e-5 and rel_l2(stats[Co:2 * Co], cache['inv_std']) < 1e-5, (groups, gi)
            assert rel_l2(amd, am) < 1e-5 and rel_l2(avd, av) < 1e-5
        # ---- leaky_relu + injected noise + sign bits (D's first layer, parity mode)
        noise = 0.2 * rng.randn(*y_ref.shape)
        nd = lay.act_to_dev(dev(noise))
        ng = N // groups
        mask = torch.zeros((M, (Co + 31) // 32), dtype=torch.int32, device="cuda")
        ep = hl.epilogue(act=hl.ACT_LRELU, groups=groups, addend=[nd[i * ng:(i + 1) * ng] for i in range(groups)], mask_out=mask)
        ad = torch.empty_like(yd)
        assert hl.conv_fprop(g, xd, wd, bd, ad, ep=ep, must_fuse=True)
        assert rel_l2(lay.act_from_dev(ad, Co), F.leaky_relu_fwd(y_ref) + noise) < FWD_TOL
        bits = _mask_bits(mask, Co)
        pre = lay.act_to_dev(dev(y_ref)).reshape(M, Co).cpu().numpy()
        sure = np.abs(pre) > 1e-5                                            # away from the kink the sign is unambiguous
        assert np.array_equal(bits[sure], (pre >= 0)[sure])
        # ---- the same with in-kernel Philox noise: one counter per (row quad, channel) of each group
        ep = hl.epilogue(act=hl.ACT_LRELU, groups=groups, sigma=0.2, seed=77, stream_id=[5, 9][:groups], mask_out=mask)
        hl.conv_fprop(g, xd, wd, bd, ad, ep=ep, must_fuse=True)
        got = ad.reshape(M, Co).cpu().double().numpy() - np.where(pre >= 0, pre, 0.2 * pre)
        for gi in range(groups):
            z = philox.randn_rowquad(mg, Co, 0.2, 77, [5, 9][gi])
            assert np.abs(got[gi * mg:(gi + 1) * mg] - z).max() < 2e-5, (groups, gi)
            zd = torch.empty((mg, Co), device="cuda")
            hl.randn_rowquad(zd, Co, 0.2, 77, [5, 9][gi])
            assert np.abs(zd.cpu().double().numpy() - z).max() < 4e-6


@pytest.mark.parametrize("case", [(2, 6, 64, 4), (4, 5, 32, 4), (2, 4, 64, 4), (3, 9, 32, 4)])        # N, Ti, H, kt: Wo = 32 / 16; To = 3, 2, 1, 6
def test_weight_stationary_first_layer_forward_via_tile_codes_0_and_6(hl, case):
    """The first layer's weight-stationary forward (fprop_c4_kernel), reached through tile code 0 (the library's choice) and tile
    code 6: the two codes dispatch to the same kernel, so every launch is BIT-identical between them.  Against the float64 oracle:
    the plain store, the leaky_relu + injected-noise epilogue and its sign bits (model/net.py:148-149,189-190); the in-kernel
    Philox form and two noise groups through the equality of the two codes."""
    N, Ti, H, kt = case
    Ci, Co = 3, 64
    rng = np.random.RandomState(900 + Ti * H)
    x = rng.uniform(-1, 1, (N, Ci, Ti, H, H))
    W = rng.randn(Co, Ci, kt, 4, 4) * 0.1
    b = rng.randn(Co) * 0.3
    y_ref = F.conv3d_fwd(x, W, b, (1, 2, 2), (0, 1, 1))
    lay = L()
    xd, wd, bd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b)
    out = {}
    for tile in (0, 6):
        g = hl.make_geom(N, Ti, H, H, 4, Co, kt, ci_valid=3)
        g.tile = tile
        M = N * g.To * g.Ho * g.Wo
        yd = torch.full((N, g.To, g.Ho, g.Wo, Co), 5.0, device="cuda")
        hl.conv_fprop(g, xd, wd, bd, yd)
        res = [yd]
        for groups in ((1, 2) if N % 2 == 0 else (1,)):
            ng = N // groups
            noise = lay.act_to_dev(dev(0.2 * np.random.RandomState(5).randn(*y_ref.shape)))
            for kw in (dict(addend=[noise[i * ng:(i + 1) * ng] for i in range(groups)]), dict(sigma=0.2, seed=31, stream_id=[4, 8][:groups])):
                mask = torch.zeros((M, 2), dtype=torch.int32, device="cuda")
                ad = torch.full_like(yd, 7.0)
                assert hl.conv_fprop(g, xd, wd, bd, ad, ep=hl.epilogue(act=hl.ACT_LRELU, groups=groups, mask_out=mask, **kw), must_fuse=True)
                res += [ad, mask]
        out[tile] = res
    assert rel_l2(lay.act_from_dev(out[0][0], Co), y_ref) < FWD_TOL
    noise_np = lay.act_from_dev(noise, Co).cpu().double().numpy()
    assert rel_l2(lay.act_from_dev(out[0][1], Co), F.leaky_relu_fwd(y_ref) + noise_np) < FWD_TOL
    bits = _mask_bits(out[0][2], Co)
    pre = lay.act_to_dev(dev(y_ref)).reshape(-1, Co).cpu().numpy()
    sure = np.abs(pre) > 1e-5
    assert np.array_equal(bits[sure], (pre >= 0)[sure])
    for i, (a, c) in enumerate(zip(out[0], out[6])):
        assert torch.equal(a, c), "launch %d differs from fprop_c4_kernel" % i


@pytest.mark.parametrize("case", [(2, 5, 32, 3, 64, 4, 0), (2, 6, 64, 3, 64, 4, 6), (4, 1, 32, 3, 64, 1, 0), (2, 5, 16, 8, 32, 4, 0), (2, 5, 16, 8, 32, 4, 2)])
def test_first_layer_epilogue_writes_the_split_form(hl, case):
    """Round 6 (MCG_IO_OUT_SPLIT): the first layer's leaky_relu + noise epilogue of an 'f32x3' network writes the three bf16 terms
    layer 2's split GEMMs read (model/net.py:148-149,189-190 feeding :150,191) -- bit for bit mcg_split_planes of the fp32 tensor
    the same launch writes otherwise, sign bits unchanged, for the weight-stationary first-layer kernels and the generic tiles,
    injected and in-kernel noise, one and two groups; the fp32 terms add up to the oracle's activation."""
    N, Ti, H, Ci, Co, kt, tile = case
    rng = np.random.RandomState(40 + H + Co)
    x = rng.uniform(-1, 1, (N, Ci, Ti, H, H))
    W = rng.randn(Co, Ci, kt, 4, 4) * 0.1
    b = rng.randn(Co) * 0.3
    y_ref = F.conv3d_fwd(x, W, b, (1, 2, 2), (0, 1, 1))
    lay = L()
    xd, wd, bd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b)
    g = hl.make_geom(N, Ti, H, H, xd.shape[-1], Co, kt, ci_valid=Ci if xd.shape[-1] != Ci else 0)
    g.tile = tile
    M = N * g.To * g.Ho * g.Wo
    noise = 0.2 * rng.randn(*y_ref.shape)
    nd = lay.act_to_dev(dev(noise))
    for groups in (1, 2):
        ng = N // groups
        for kw in (dict(addend=[nd[i * ng:(i + 1) * ng] for i in range(groups)]), dict(sigma=0.2, seed=3, stream_id=[6, 2][:groups])):
            m32, m16 = (torch.zeros((M, (Co + 31) // 32), dtype=torch.int32, device="cuda") for _ in range(2))
            a32 = torch.empty((N, g.To, g.Ho, g.Wo, Co), device="cuda")
            asp = torch.full((N, g.To, g.Ho, g.Wo, 4 * Co), 3.0, device="cuda", dtype=torch.bfloat16)
            assert hl.conv_fprop(g, xd, wd, bd, a32, ep=hl.epilogue(act=hl.ACT_LRELU, groups=groups, mask_out=m32, **kw), must_fuse=True)
            assert hl.conv_fprop(g, xd, wd, bd, asp, ep=hl.epilogue(act=hl.ACT_LRELU, groups=groups, mask_out=m16, out_split=True, **kw), must_fuse=True)
            want = hl.split_planes(a32).view(M, Co // 16, 4, 16)
            got = asp.view(M, Co // 16, 4, 16)
            assert torch.equal(got[:, :, :3], want[:, :, :3]) and torch.equal(m32, m16), (groups, list(kw))
            assert float((got[:, :, 3].float() - 3.0).abs().max()) == 0.0                    # the padding plane is not written
            if 'addend' in kw:
                terms = got[:, :, :3].double().sum(2).reshape(N, g.To, g.Ho, g.Wo, Co)
                assert rel_l2(lay.act_from_dev(terms.float(), Co), F.leaky_relu_fwd(y_ref) + noise) < FWD_TOL
    with pytest.raises(hl.McgError):                                                          # only with the activation epilogue
        hl.conv_fprop(g, xd, wd, bd, asp, ep=hl.epilogue(out_split=True), must_fuse=True)


@pytest.mark.parametrize("case", EPI_CASES[:3])
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 103, 201])
def test_dgrad_epilogue_sums_and_mask(hl, case, tile):
    """dgrad epilogues: (a) column statistics of the output (the generator's deconvolution feeding BatchNorm), (b) the
    sums of BatchNorm's backward pass over the produced gradient, (c) leaky_relu's backward from stored sign bits plus
    the bias gradient."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(hash(case) % 2**31 + 11)
    gy = rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2)
    W = rng.randn(Co, Ci, kt, 4, 4) * 0.1
    x0 = np.zeros((N, Ci, Ti, H, H))
    gx_ref, _, _ = F.conv3d_bwd(x0, W, gy, (1, 2, 2), (0, 1, 1))             # (N,Ci,Ti,H,H)
    lay = L()
    gyd, wd = lay.act_to_dev(dev(gy)), lay.conv_w_to_dev(dev(W))
    Cp = wd.shape[-1]
    g = hl.make_geom(N, Ti, H, H, Cp, Co, kt)
    g.tile = tile
    M = N * Ti * H * H
    ref_rows = lay.act_to_dev(dev(gx_ref)).reshape(M, Cp).cpu().double().numpy()
    for groups in (1, 2):
        mg = M // groups
        # (a) statistics of the output, with a bias (deconvolution forward)
        bias = rng.randn(Cp) * 0.2
        part = torch.full((hl.epilogue_part_floats(g, "dgrad", groups),), float('nan'), device="cuda")
        ws0 = torch.empty(hl.bn_workspace_floats(max(Cp, 64)), device="cuda")
        ep = hl.epilogue(sums=hl.SUMS_STATS, groups=groups, part=part)
        xd = torch.empty((N, Ti, H, H, Cp), device="cuda")
        assert hl.conv_dgrad(g, gyd, wd, dev(bias), xd, ep=ep)
        out = ref_rows + bias
        assert rel_l2(xd.reshape(M, Cp), out) < BWD_TOL
        for gi in range(groups):
            stats = torch.empty(4 * Cp, device="cuda")
            hl.bn_stats_from_partials(mg, Cp, part[gi * 2 * Cp:], ep.n_slots, ep.slot_stride, dev(np.ones(Cp)), dev(np.zeros(Cp)), stats, None, None, ws0)
            o = out[gi * mg:(gi + 1) * mg]
            assert np.abs(stats[:Cp].cpu().numpy() - o.mean(0)).max() < 1e-5 * max(1.0, np.abs(o).max())
            assert rel_l2(stats[Cp:2 * Cp], 1 / np.sqrt(o.var(0) + 2e-5)) < 1e-5
        # (b) BatchNorm-backward sums against the stand-alone pass
        ybn = rng.randn(M, Cp) * 1.3 + 0.2
        ybnd = dev(ybn).reshape(N, Ti, H, H, Cp)
        gam = 1 + 0.1 * rng.randn(Cp)
        ws = torch.empty(hl.bn_workspace_floats(max(Cp, 64)), device="cuda")
        st = []
        for gi in range(groups):
            s_ = torch.empty(4 * Cp, device="cuda")
            hl.bn_stats(mg, Cp, ybnd.reshape(M, Cp)[gi * mg:(gi + 1) * mg], dev(gam), dev(0.1 * rng.randn(Cp)), s_, None, None, ws)
            st.append(s_)
        for act in (hl.ACT_LRELU, hl.ACT_RELU):
            ep = hl.epilogue(sums=hl.SUMS_BN_BWD, groups=groups, part=part, bn_y=ybnd, bn_stats=st, bn_act=act)
            assert hl.conv_dgrad(g, gyd, wd, None, xd, ep=ep)
            assert rel_l2(xd.reshape(M, Cp), ref_rows) < BWD_TOL
            for gi in range(groups):
                sl = slice(gi * mg, (gi + 1) * mg)
                gref, dg_ref, db_ref = torch.empty((mg, Cp), device="cuda"), torch.zeros(Cp, device="cuda"), torch.zeros(Cp, device="cuda")
                hl.bn_act_bwd(mg, Cp, xd.reshape(M, Cp)[sl].contiguous(), ybnd.reshape(M, Cp)[sl].contiguous(), st[gi], dev(gam), act, gref,
                              dg_ref, db_ref, ws)
                got, dg, db = torch.empty((mg, Cp), device="cuda"), torch.zeros(Cp, device="cuda"), torch.zeros(Cp, device="cuda")
                hl.bn_act_bwd_from_partials(mg, Cp, xd.reshape(M, Cp)[sl].contiguous(), ybnd.reshape(M, Cp)[sl].contiguous(), st[gi], dev(gam),
                                            act, part[gi * 2 * Cp:], ep.n_slots, ep.slot_stride, got, dg, db, ws)
                assert rel_l2(got, gref.cpu().double().numpy()) < 1e-5, (groups, gi, act)
                assert rel_l2(dg, dg_ref.cpu().double().numpy()) < 1e-5 and rel_l2(db, db_ref.cpu().double().numpy()) < 1e-5
    # (c) leaky_relu backward from sign bits + column sums (dc1's bias gradient)
    sign = rng.rand(M, Cp) > 0.4
    words = np.zeros((M, (Cp + 31) // 32), dtype=np.uint32)
    for c in range(Cp):
        words[:, c >> 5] |= (sign[:, c].astype(np.uint32) << np.uint32(c & 31))
    maskd = torch.tensor(words.view(np.int32), device="cuda")
    part = torch.full((hl.epilogue_part_floats(g, "dgrad", 1),), float('nan'), device="cuda")
    ep = hl.epilogue(mask_in=maskd, sums=hl.SUMS_COL, groups=1, part=part)
    xd = torch.empty((N, Ti, H, H, Cp), device="cuda")
    assert hl.conv_dgrad(g, gyd, wd, None, xd, ep=ep, must_fuse=True)
    want = ref_rows * np.where(sign, 1.0, 0.2)
    assert rel_l2(xd.reshape(M, Cp), want) < BWD_TOL
    db = torch.ones(Cp, device="cuda")
    hl.colsum_from_partials(Cp, part, ep.n_slots, ep.slot_stride, db, torch.empty(hl.bn_workspace_floats(max(Cp, 64)), device="cuda"))
    assert np.abs(db.cpu().double().numpy() - (1 + want.sum(0))).max() < 1e-4 * max(1.0, np.abs(want.sum(0)).max())


def test_fused_epilogue_refuses_what_it_cannot_own(hl):
    lay = L()
    g = hl.make_geom(2, 4, 16, 16, 8, 64, 4)
    g.tile = 1103                                                          # split-K: partial tiles
    x = torch.zeros((2, 4, 16, 16, 8), device="cuda")
    w = torch.zeros((64, 4, 4, 4, 8), device="cuda")
    y = torch.zeros((2, 1, 8, 8, 64), device="cuda")
    part = torch.zeros(hl.epilogue_part_floats(g, "fprop", 1), device="cuda")
    ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part)
    assert hl.conv_fprop(g, x, w, None, y, ep=ep) is False                 # declined: the plain launch ran
    lib = hl.load()
    import ctypes
    assert lib.mcg_conv_fprop_ex(ctypes.byref(g), hl._p(x), hl._p(w), None, hl._p(y), ctypes.byref(ep), None) == -2
    g.tile = 0
    bad = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=None)             # sums without a partial buffer
    with pytest.raises(hl.McgError):
        hl.conv_fprop(g, x, w, None, y, ep=bad)
    ep3 = hl.epilogue(sums=hl.SUMS_STATS, groups=2, part=part)
    g3 = hl.make_geom(3, 4, 16, 16, 8, 64, 4)                              # odd batch cannot form two groups
    with pytest.raises(hl.McgError):
        hl.conv_fprop(g3, torch.zeros((3, 4, 16, 16, 8), device="cuda"), w, None, torch.zeros((3, 1, 8, 8, 64), device="cuda"), ep=ep3)


C4_CASES = [
    # N, Ti, H, kt     (Ci = 3 padded to 4, Co = 64: D's first layer / the generator's last layer read backwards)
    (2, 6, 32, 4),       # Wo = 16: one block of 256 output pixels per batch item, three frame steps through the slab ring
    (3, 1, 32, 1),       # 2-D
    (2, 5, 64, 4),       # Wo = 32: four blocks per batch item
    (2, 1, 64, 1),
    (150, 1, 64, 1),     # more (row block, batch item) pairs than blocks: a block of the weight-gradient kernel walks two items
]


@pytest.mark.parametrize("case", C4_CASES)
def test_weight_stationary_first_layer_kernels(hl, case):
    """tile code 6 (and the heuristic, tile 0) runs the weight-stationary Ci = 4 kernels; they must agree with the
    oracle like the generic GEMM kernels (tile 2), with and without the fused first-layer epilogue."""
    N, Ti, H, kt = case
    Ci, Co = 3, 64
    rng = np.random.RandomState(hash(case) % 2**31 + 3)
    x = rng.uniform(-1, 1, (N, Ci, Ti, H, H))
    W = rng.randn(Co, Ci, kt, 4, 4) * 0.1
    b = rng.randn(Co) * 0.2
    y_ref = F.conv3d_fwd(x, W, b, (1, 2, 2), (0, 1, 1))
    lay = L()
    xd, wd, bd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b)
    for tile, cv in ((6, 3), (6, 0), (0, 3), (2, 3)):         # cv = 3: the kernels skip the products with the padded channel
        g = hl.make_geom(N, Ti, H, H, 4, Co, kt, ci_valid=cv)
        g.tile = tile
        yd = torch.full((N, g.To, g.Ho, g.Wo, Co), 5.0, device="cuda")
        hl.conv_fprop(g, xd, wd, bd, yd)
        assert rel_l2(lay.act_from_dev(yd, Co), y_ref) < FWD_TOL, tile
        M = N * g.To * g.Ho * g.Wo
        for groups in ((1, 2) if N % 2 == 0 else (1,)):
            noise = 0.2 * rng.randn(*y_ref.shape)
            nd = lay.act_to_dev(dev(noise))
            ng = N // groups
            mask = torch.zeros((M, 2), dtype=torch.int32, device="cuda")
            ep = hl.epilogue(act=hl.ACT_LRELU, groups=groups, addend=[nd[i * ng:(i + 1) * ng] for i in range(groups)], mask_out=mask)
            ad = torch.empty_like(yd)
            hl.conv_fprop(g, xd, wd, bd, ad, ep=ep, must_fuse=True)
            assert rel_l2(lay.act_from_dev(ad, Co), F.leaky_relu_fwd(y_ref) + noise) < FWD_TOL, (tile, groups)
            pre = lay.act_to_dev(dev(y_ref)).reshape(M, Co).cpu().numpy()
            sure = np.abs(pre) > 1e-5
            assert np.array_equal(_mask_bits(mask, Co)[sure], (pre >= 0)[sure]), (tile, groups)
            mg = M // groups
            ep = hl.epilogue(act=hl.ACT_LRELU, groups=groups, sigma=0.2, seed=5, stream_id=[11, 12][:groups], mask_out=mask)
            hl.conv_fprop(g, xd, wd, bd, ad, ep=ep, must_fuse=True)
            got = ad.reshape(M, Co).cpu().double().numpy() - np.where(pre >= 0, pre, 0.2 * pre)
            for gi in range(groups):
                assert np.abs(got[gi * mg:(gi + 1) * mg] - philox.randn_rowquad(mg, Co, 0.2, 5, [11, 12][gi])).max() < 2e-5
    # bf16 networks: the weight-stationary kernel on the bf16 MFMA, plain and with the first-layer epilogue (bf16 output)
    for exact in (True, False):
        x2, W2 = (_bf16_round(x), _bf16_round(W)) if exact else (x, W)
        y2 = F.conv3d_fwd(x2, W2, b, (1, 2, 2), (0, 1, 1))
        g = hl.make_geom(N, Ti, H, H, 4, Co, kt, ci_valid=3, precision='bf16')
        g.tile = 6
        yd = torch.full((N, g.To, g.Ho, g.Wo, Co), 5.0, device="cuda")
        hl.conv_fprop(g, lay.act_to_dev(dev(x2)), lay.conv_w_to_dev(dev(W2)), bd, yd)
        assert rel_l2(lay.act_from_dev(yd, Co), y2) < (FWD_TOL if exact else BF16_TOL), exact
        if exact:
            M = N * g.To * g.Ho * g.Wo
            mask = torch.zeros((M, 2), dtype=torch.int32, device="cuda")
            a16 = torch.empty((N, g.To, g.Ho, g.Wo, Co), device="cuda", dtype=torch.bfloat16)
            hl.conv_fprop(g, lay.act_to_dev(dev(x2)), lay.conv_w_to_dev(dev(W2)), bd, a16, must_fuse=True,
                          ep=hl.epilogue(act=hl.ACT_LRELU, groups=1, mask_out=mask, out_bf16=True))
            want = torch.tensor(F.leaky_relu_fwd(y2), dtype=torch.float32).to(torch.bfloat16).double().numpy()
            got = lay.act_from_dev(a16.float(), Co).cpu().double().numpy()
            assert np.abs(got - want).max() <= 2.0 ** -7 * np.abs(want).max()      # one bf16 ulp at most (fp32 sums rounded once)
    # input gradient: the MFMA col2im kernel (ci_valid = 3, tile 0 / 6) against the oracle; the accumulating call and
    # ci_valid = 0 take the VALU kernel
    gy = rng.randn(*y_ref.shape)
    gx_ref, _, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
    gyd = lay.act_to_dev(dev(gy))
    for tile, cv in ((6, 3), (0, 3), (0, 0)):
        g = hl.make_geom(N, Ti, H, H, 4, Co, kt, ci_valid=cv)
        g.tile = tile
        gxd = torch.full_like(xd, 7.0)
        hl.conv_dgrad(g, gyd, wd, None, gxd)
        assert rel_l2(lay.act_from_dev(gxd, Ci), gx_ref) < BWD_TOL, (tile, cv)
        assert float(gxd[..., 3].abs().max()) == 0.0
        again = torch.full_like(xd, -3.0)
        hl.conv_dgrad(g, gyd, wd, None, again)
        assert torch.equal(again, gxd), "the shared rows are added by two blocks: the sum must not depend on their order"
        hl.conv_dgrad(g, gyd, wd, None, gxd, accumulate=True)
        assert rel_l2(lay.act_from_dev(gxd, Ci), 2 * gx_ref) < BWD_TOL, (tile, cv)
    # bf16 networks: the same col2im kernel on the bf16 MFMA (y and w rounded on their way into LDS): digit-exact on
    # bf16-representable operands, within the bf16 tolerance otherwise
    for exact in (True, False):
        gy2 = _bf16_round(gy) if exact else gy
        W2 = _bf16_round(W) if exact else W
        ref2, _, _ = F.conv3d_bwd(x, W2, gy2, (1, 2, 2), (0, 1, 1))
        g = hl.make_geom(N, Ti, H, H, 4, Co, kt, ci_valid=3, precision='bf16')
        gxd = torch.full_like(xd, 7.0)
        hl.conv_dgrad(g, lay.act_to_dev(dev(gy2)), lay.conv_w_to_dev(dev(W2)), None, gxd)
        assert rel_l2(lay.act_from_dev(gxd, Ci), ref2) < (BWD_TOL if exact else BF16_TOL), exact
        assert float(gxd[..., 3].abs().max()) == 0.0
    # weight gradient: the patch-in-LDS kernel (ci_valid = 3, tile 6, fp32) accumulates onto dw like the generic one
    # (tiles 0 and 3; ci_valid = 0); the padded channel's gradient stays exactly zero
    _, gW_ref, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
    for tile, cv in ((6, 3), (0, 3), (3, 3), (0, 0)):
        g = hl.make_geom(N, Ti, H, H, 4, Co, kt, ci_valid=cv)
        g.tile = tile
        dwd = torch.zeros_like(wd)
        hl.conv_wgrad(g, xd, gyd, dwd)
        assert rel_l2(lay.conv_w_from_dev(dwd, Ci, 3), gW_ref) < BWD_TOL, (tile, cv)
        assert float(dwd[..., 3].abs().max()) == 0.0
        hl.conv_wgrad(g, xd, gyd, dwd)
        assert rel_l2(lay.conv_w_from_dev(dwd, Ci, 3), 2 * gW_ref) < BWD_TOL, (tile, cv)
    g = hl.make_geom(N, Ti, H, H, 4, Co, kt, ci_valid=3, precision='bf16')     # bf16 networks: no such kernel, the code is refused
    g.tile = 6
    with pytest.raises(hl.McgError):
        hl.conv_wgrad(g, xd, gyd, torch.zeros_like(wd))
    g = hl.make_geom(2, 5, 16, 16, 8, 64, 4)                  # not a first-layer geometry: the code is refused
    g.tile = 6
    z = torch.zeros(1, device="cuda")
    with pytest.raises(hl.McgError):
        hl.conv_fprop(g, torch.zeros((2, 5, 16, 16, 8), device="cuda"), torch.zeros((64, 4, 4, 4, 8), device="cuda"), None,
                      torch.zeros((2, 2, 8, 8, 64), device="cuda"))


# ------------------------------------------------------------------------------------------------------------------
# MCG_PREC_BF16_STORE ('bf16s'): operands that are bf16 IN MEMORY (BASELINE configs[2] networks keep the tensors that are
# only read by GEMMs -- activations, output gradients, a weight copy -- in bf16)
# ------------------------------------------------------------------------------------------------------------------
BF16S_CASES = [(2, 7, 16, 8, 64, 4), (3, 1, 16, 16, 32, 1), (2, 4, 8, 64, 160, 4), (2, 9, 8, 16, 24, 4)]


@pytest.mark.parametrize("case", BF16S_CASES)
@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 101, 203])
def test_bf16_stored_operands_equal_rounding_in_the_kernel(hl, case, tile):
    """Rounding an operand to bf16 when it is stored or when it is loaded yields the same number, so a 'bf16s' launch on
    bf16 tensors must reproduce the 'bf16' launch on the fp32 tensors holding the same (bf16-representable) values: bit
    for bit for fprop / dgrad (same MFMA sequence), to summation order for wgrad (atomics); and both match the oracle."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(hash(case) % 2**31 + 5)
    lay = L()
    x, W = _bf16_round(rng.uniform(-1, 1, (N, Ci, Ti, H, H))), _bf16_round(rng.randn(Co, Ci, kt, 4, 4) * 0.1)
    b = rng.randn(Co)
    gy = _bf16_round(rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2))
    y_ref = F.conv3d_fwd(x, W, b, (1, 2, 2), (0, 1, 1))
    gx_ref, gW_ref, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
    xd, wd, bd, gyd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b), lay.act_to_dev(dev(gy))
    x16, w16, gy16 = xd.to(torch.bfloat16), wd.to(torch.bfloat16), gyd.to(torch.bfloat16)
    assert torch.equal(x16.float(), xd) and torch.equal(w16.float(), wd)
    res = {}
    for prec, (xa, wa, ga) in (('bf16', (xd, wd, gyd)), ('bf16s', (x16, w16, gy16))):
        g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision=prec)
        g.tile = tile
        yd = torch.empty((N, g.To, g.Ho, g.Wo, Co), device="cuda")
        hl.conv_fprop(g, xa, wa, bd, yd)
        gxd = torch.full((N, Ti, H, H, Ci), 7.0, device="cuda")
        hl.conv_dgrad(g, ga, wa, None, gxd)
        dwd = torch.zeros_like(wd)
        hl.conv_wgrad(g, xa, ga, dwd)
        res[prec] = (yd, gxd, dwd)
    assert rel_l2(lay.act_from_dev(res['bf16s'][0], Co), y_ref) < FWD_TOL
    assert rel_l2(lay.act_from_dev(res['bf16s'][1], Ci), gx_ref) < BWD_TOL
    assert rel_l2(lay.conv_w_from_dev(res['bf16s'][2], Ci, 3), gW_ref) < BWD_TOL
    assert torch.equal(res['bf16'][0], res['bf16s'][0]) and torch.equal(res['bf16'][1], res['bf16s'][1])
    if not rel_l2(res['bf16s'][2], res['bf16'][2].cpu().double().numpy()) < 1e-5:      # (seen once, on the driver's box in round 3: leave evidence)
        from guard import describe_diff
        ref_dev = lay.conv_w_to_dev(dev(gW_ref)).cpu().double().numpy()
        raise AssertionError(describe_diff(res['bf16s'][2], res['bf16'][2], ref_dev, names=("bf16s", "bf16")))
    # a stats epilogue rides on a 'bf16s' launch too; host tensors / wrong dtypes are refused
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='bf16s')
    g.tile = tile
    part = torch.empty(hl.epilogue_part_floats(g, "fprop", 1), device="cuda")
    ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part)
    y2 = torch.empty_like(res['bf16s'][0])
    assert hl.conv_fprop(g, x16, w16, bd, y2, ep=ep) and torch.equal(y2, res['bf16s'][0])
    with pytest.raises(hl.McgError):
        hl.conv_fprop(g, xd, w16, bd, y2)                     # fp32 tensor where the geometry promises bf16


def test_elementwise_passes_write_bf16_operands(hl):
    """bn_act_fwd / bn_act_bwd with a bf16 output tensor store round-to-nearest-even of what they store in fp32, and Adam's
    bf16 weight copy is the rounded master parameter."""
    rng = np.random.RandomState(12)
    M, C = 3000, 64
    y, gamma, beta = dev(rng.randn(M, C) * 1.5), dev(1 + 0.1 * rng.randn(C)), dev(0.1 * rng.randn(C))
    ws = torch.empty(hl.bn_workspace_floats(C), device="cuda")
    stats = torch.empty(4 * C, device="cuda")
    hl.bn_stats(M, C, y, gamma, beta, stats, None, None, ws)
    o32, o16 = torch.empty((M, C), device="cuda"), torch.empty((M, C), device="cuda", dtype=torch.bfloat16)
    hl.bn_act_fwd(M, C, y, stats[2 * C:], hl.ACT_LRELU, o32, sigma=0.2, seed=3, stream_id=9)
    hl.bn_act_fwd(M, C, y, stats[2 * C:], hl.ACT_LRELU, o16, sigma=0.2, seed=3, stream_id=9)
    assert torch.equal(o16, o32.to(torch.bfloat16))
    g = dev(rng.randn(M, C))
    g32, g16 = torch.empty((M, C), device="cuda"), torch.empty((M, C), device="cuda", dtype=torch.bfloat16)
    hl.bn_act_bwd(M, C, g, y, stats, gamma, hl.ACT_LRELU, g32, None, None, ws)
    hl.bn_act_bwd(M, C, g, y, stats, gamma, hl.ACT_LRELU, g16, None, None, ws)
    assert torch.equal(g16, g32.to(torch.bfloat16))
    n = 5001
    p, gr, m, v = dev(rng.randn(n)), dev(rng.randn(n) * 1e-2), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    p16 = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    hl.adam_wd(p, gr, m, v, 2e-4, 5e-5, 0.999, 1e-8, 1e-5, p16=p16)
    assert torch.equal(p16, p.to(torch.bfloat16))
    # bf16 INPUTS (the GEMM outputs of a bf16 network): the same numbers held in bf16 or in fp32 give the same results, bit
    # for bit, whatever the mix of element types (MCG_IO_* flags); in place on a bf16 gradient too
    yb, gb = y.to(torch.bfloat16), g.to(torch.bfloat16)
    yr, gr_ = yb.float(), gb.float()
    hl.bn_stats(M, C, yr, gamma, beta, stats, None, None, ws)
    ref_f = torch.empty((M, C), device="cuda")
    hl.bn_act_fwd(M, C, yr, stats[2 * C:], hl.ACT_LRELU, ref_f, sigma=0.2, seed=3, stream_id=9)
    for out_dt in (torch.float32, torch.bfloat16):
        o = torch.empty((M, C), device="cuda", dtype=out_dt)
        hl.bn_act_fwd(M, C, yb, stats[2 * C:], hl.ACT_LRELU, o, sigma=0.2, seed=3, stream_id=9)
        assert torch.equal(o, ref_f.to(out_dt)), out_dt
    ref_b, dg_ref, db_ref = torch.empty((M, C), device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    hl.bn_act_bwd(M, C, gr_, yr, stats, gamma, hl.ACT_LRELU, ref_b, dg_ref, db_ref, ws)
    for g_in in (gr_, gb):
        for y_in in (yr, yb):
            for out_dt in (torch.float32, torch.bfloat16):
                o, dg, db = torch.empty((M, C), device="cuda", dtype=out_dt), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
                hl.bn_act_bwd(M, C, g_in, y_in, stats, gamma, hl.ACT_LRELU, o, dg, db, ws)
                # (with a bf16 input the per-channel sums come from the eight-channels-per-thread kernel: the same addends in
                #  another tree, so dgamma / dbeta -- and through them every output -- agree to fp32 rounding, not bit for bit)
                assert torch.allclose(dg, dg_ref, rtol=2e-5, atol=1e-5) and torch.allclose(db, db_ref, rtol=2e-5, atol=1e-5)
                tol = 2.0 ** -7 if out_dt == torch.bfloat16 else 2e-5
                assert bool(((o.float() - ref_b).abs() <= tol * ref_b.abs() + 1e-5).all()), (g_in.dtype, y_in.dtype, out_dt)
    gi = gb.clone()
    hl.bn_act_bwd(M, C, gi, yb, stats, gamma, hl.ACT_LRELU, gi, None, None, ws)            # in place, bf16 -> bf16
    assert bool(((gi.float() - ref_b).abs() <= 2.0 ** -7 * ref_b.abs() + 1e-5).all())
    alias = torch.empty(0, dtype=torch.bfloat16, device="cuda").set_(gr_.untyped_storage(), 0, (M, C), (C, 1))
    assert alias.data_ptr() == gr_.data_ptr()
    with pytest.raises(hl.McgError):                                                       # in place across element types: refused
        hl.bn_act_bwd(M, C, gr_, yb, stats, gamma, hl.ACT_LRELU, alias, None, None, ws)


BF16_OUT_CASES = [(2, 7, 16, 64, 128, 4), (4, 1, 16, 128, 64, 1)]


@pytest.mark.parametrize("case", BF16_OUT_CASES)
def test_bf16_gemm_outputs(hl, case):
    """bf16 networks keep the GEMM outputs the element-wise passes read in bf16: a launch that writes y (fprop) or x (dgrad)
    in bf16 stores the round-to-nearest-even of what the fp32 launch stores -- plain and with the statistics epilogue, whose
    sums are those of the values as stored; split-K, accumulating and first-layer launches refuse a bf16 output."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(hash(case) % 2**31 + 9)
    lay = L()
    x, W = _bf16_round(rng.uniform(-1, 1, (N, Ci, Ti, H, H))), _bf16_round(rng.randn(Co, Ci, kt, 4, 4) * 0.1)
    b = rng.randn(Co)
    gy = _bf16_round(rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2))
    xd, wd, bd, gyd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b), lay.act_to_dev(dev(gy))
    x16, w16, gy16 = xd.to(torch.bfloat16), wd.to(torch.bfloat16), gyd.to(torch.bfloat16)
    for tile in (0, 2, 3):
        g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='bf16s')
        g.tile = tile
        y32 = torch.empty((N, g.To, g.Ho, g.Wo, Co), device="cuda")
        y16 = torch.empty_like(y32, dtype=torch.bfloat16)
        hl.conv_fprop(g, x16, w16, bd, y32)
        hl.conv_fprop(g, x16, w16, bd, y16)
        assert torch.equal(y16, y32.to(torch.bfloat16)), tile
        M = N * g.To * g.Ho * g.Wo
        parts = []
        for out in (y32, y16):
            part = torch.zeros(hl.epilogue_part_floats(g, 'fprop', 1), device="cuda")
            ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part, out_bf16=out.dtype == torch.bfloat16)
            out.zero_()
            assert hl.conv_fprop(g, x16, w16, bd, out, ep=ep, must_fuse=True)
            parts.append((part, ep.n_slots, ep.slot_stride))
        assert torch.equal(y16, y32.to(torch.bfloat16)) and parts[0][1:] == parts[1][1:], tile
        # the statistics are those of the tensor as STORED: column sums of the fp32 values / of the rounded values
        for (part, n_slots, stride), out in zip(parts, (y32, y16)):
            s = part[:n_slots * stride].view(n_slots, stride).double().sum(0)
            v = out.double().view(M, Co)
            assert torch.allclose(s[:Co], v.sum(0), rtol=1e-5, atol=1e-3) and torch.allclose(s[Co:2 * Co], (v * v).sum(0), rtol=1e-5, atol=1e-3), tile
        gx32 = torch.empty_like(xd)
        gx16 = torch.empty_like(xd, dtype=torch.bfloat16)
        hl.conv_dgrad(g, gy16, w16, None, gx32)
        hl.conv_dgrad(g, gy16, w16, None, gx16)
        assert torch.equal(gx16, gx32.to(torch.bfloat16)), tile
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='bf16s')
    g.tile = 1203                                                  # split K: partial tiles are added in fp32
    with pytest.raises(hl.McgError):
        hl.conv_fprop(g, x16, w16, bd, torch.empty((N, g.To, g.Ho, g.Wo, Co), device="cuda", dtype=torch.bfloat16))
    g.tile = 0
    with pytest.raises(AssertionError):                            # the binding refuses an accumulating call with a bf16 result
        hl.conv_dgrad(g, gy16, w16, None, torch.zeros_like(xd, dtype=torch.bfloat16), accumulate=True)


# ------------------------------------------------------------------------------------------------------------------
# The LDS-DMA GEMM kernels of bf16 networks (tile codes 7 = 256x128, 8 = 256x256: gemm_bf16_v2_kernel): wide layers
# only (channel counts powers of two >= 64), bf16-stored operands
# ------------------------------------------------------------------------------------------------------------------
V2_CASES = [(2, 7, 16, 64, 128, 4),      # M = 512 rows, 3-D
            (3, 1, 16, 128, 64, 1),      # M = 192: a ragged 256-row tile; Co = 64 < BN
            (1, 5, 8, 256, 256, 4),      # M = 32: one nearly empty tile, long K
            (2, 6, 32, 64, 128, 4),      # M = 1536: several tiles per frame
            (5, 1, 8, 128, 512, 1)]      # 2-D, four N tiles of 128


@pytest.mark.parametrize("case", V2_CASES)
@pytest.mark.parametrize("tile", [7, 8, 10])
@pytest.mark.parametrize("prec", ['bf16s', 'f32'])
def test_lds_dma_kernels_match_the_oracle(hl, case, tile, prec):
    """fprop / dgrad / wgrad of the round-3 bf16 kernels (operands straight from global memory into a swizzled LDS image,
    a ring of tile buffers, 8 waves) on bf16-representable inputs against the float64 oracle at the fp32 tolerances, plain
    and with the statistics epilogue / a bf16 output; the padding taps are the zeros the buffer range check writes."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(9000 + V2_CASES.index(case))
    lay = L()
    x, W = _bf16_round(rng.uniform(-1, 1, (N, Ci, Ti, H, H))), _bf16_round(rng.randn(Co, Ci, kt, 4, 4) * 0.1)
    b = rng.randn(Co)
    gy = _bf16_round(rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2))
    y_ref = F.conv3d_fwd(x, W, b, (1, 2, 2), (0, 1, 1))
    gx_ref, gW_ref, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
    xd, wd, bd, gyd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b), lay.act_to_dev(dev(gy))
    s16 = prec == 'bf16s'                                         # fp32 networks: the same kernels on the fp32 MFMA, fp32 tensors
    odt = torch.bfloat16 if s16 else torch.float32
    x16, w16, gy16 = (xd.to(torch.bfloat16), wd.to(torch.bfloat16), gyd.to(torch.bfloat16)) if s16 else (xd, wd, gyd)
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision=prec)
    g.tile = tile
    M = N * g.To * g.Ho * g.Wo
    yd = torch.full((N, g.To, g.Ho, g.Wo, Co), 3.0, device="cuda")
    hl.conv_fprop(g, x16, w16, bd, yd)
    assert rel_l2(lay.act_from_dev(yd, Co), y_ref) < FWD_TOL
    # statistics epilogue (+ bf16 output in bf16 networks)
    y16 = torch.empty_like(yd, dtype=odt)
    part = torch.zeros(hl.epilogue_part_floats(g, 'fprop', 1), device="cuda")
    ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part, out_bf16=s16)
    assert hl.conv_fprop(g, x16, w16, bd, y16, ep=ep, must_fuse=True)
    assert torch.equal(y16, yd.to(odt))
    sums = part[:ep.n_slots * ep.slot_stride].view(ep.n_slots, ep.slot_stride).double().sum(0)
    v = y16.double().view(M, Co)
    assert torch.allclose(sums[:Co], v.sum(0), rtol=1e-5, atol=1e-3) and torch.allclose(sums[Co:2 * Co], (v * v).sum(0), rtol=1e-5, atol=1e-3)
    if tile != 10 or Ci >= 128 or (Ci == 64 and s16):             # (tile 10 at 64 output columns: 256x64 with two buffers, bf16-stored / split operands)
        # input gradient (the filter tile stays in global orientation: transposing LDS reads), plain / bf16 output / column sums
        gxd = torch.full((N, Ti, H, H, Ci), 7.0, device="cuda")
        hl.conv_dgrad(g, gy16, w16, None, gxd)
        assert rel_l2(lay.act_from_dev(gxd, Ci), gx_ref) < BWD_TOL
        gx16 = torch.empty_like(gxd, dtype=odt)
        part = torch.zeros(hl.epilogue_part_floats(g, 'dgrad', 1), device="cuda")
        ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part, out_bf16=s16)
        assert hl.conv_dgrad(g, gy16, w16, None, gx16, ep=ep, must_fuse=True)
        assert torch.equal(gx16, gxd.to(odt))
        sums = part[:ep.n_slots * ep.slot_stride].view(ep.n_slots, ep.slot_stride).double().sum(0)
        v = gx16.double().view(-1, Ci)
        assert torch.allclose(sums[:Ci], v.sum(0), rtol=1e-5, atol=1e-3)
        # leaky_relu mask multiply + column sums (what dc2's input gradient carries for D's first layer)
        bits = torch.randint(0, 2, (N * Ti * H * H, Ci), device="cuda", dtype=torch.int64)
        words = (bits.view(-1, Ci // 32, 32) << torch.arange(32, device="cuda")).sum(-1)
        words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()
        part = torch.zeros(hl.epilogue_part_floats(g, 'dgrad', 1), device="cuda")
        ep = hl.epilogue(mask_in=words, sums=hl.SUMS_COL, groups=1, part=part)
        gxm = torch.empty_like(gxd)
        assert hl.conv_dgrad(g, gy16, w16, None, gxm, ep=ep, must_fuse=True)
        want = gxd.view(-1, Ci) * torch.where(bits.bool(), 1.0, 0.2).float()
        assert torch.equal(gxm.view(-1, Ci), want)
        sums = part[:ep.n_slots * ep.slot_stride].view(ep.n_slots, ep.slot_stride).double().sum(0)
        assert torch.allclose(sums[:Ci], want.double().sum(0), rtol=1e-5, atol=1e-3)
        gxa = torch.full((N, Ti, H, H, Ci), 0.5, device="cuda")
        hl.conv_dgrad(g, gy16, w16, dev(rng.randn(Ci) * 0), gxa, accumulate=True)          # accumulate onto x (the frame-t add of the step)
        assert rel_l2(lay.act_from_dev(gxa, Ci), gx_ref + 0.5) < BWD_TOL
    # weight gradient (both tiles in global orientation), added onto what dw holds
    if Co >= 128:
        dwd = torch.ones_like(wd)
        hl.conv_wgrad(g, x16, gy16, dwd)
        assert rel_l2(lay.conv_w_from_dev(dwd, Ci, 3), gW_ref + 1) < BWD_TOL
    # a narrow layer is refused (the caller keeps such layers on the register-staged kernels)
    gn = hl.make_geom(2, 5, 16, 16, 16, 32, 4, precision=prec)
    gn.tile = tile
    with pytest.raises(hl.McgError):
        hl.conv_fprop(gn, torch.zeros((2, 5, 16, 16, 16), device="cuda", dtype=odt),
                      torch.zeros((32, 4, 4, 4, 16), device="cuda", dtype=odt), None, torch.zeros((2, 2, 8, 8, 32), device="cuda"))


@pytest.mark.parametrize("case", [(2, 6, 16, 128, 256, 4), (4, 1, 16, 128, 128, 1), (2, 5, 8, 256, 256, 4)])
@pytest.mark.parametrize("tile", [7, 8, 10])
@pytest.mark.parametrize("prec", ['bf16s', 'f32x3'])
def test_lds_dma_kernels_carry_batchnorm_backward_sums(hl, case, tile, prec):
    """MCG_SUMS_BN_BWD in the row-wise epilogue of the LDS-DMA kernels (round 3): the input-gradient GEMM of a discriminator layer /
    the backward-data GEMM of a generator layer also produces (sum g', sum g' x_hat) of the BatchNorm backward pass that reads its
    output -- with bf16 tensors around it in bf16 networks (the sums are those of the STORED gradient) and with split operands.
    Checked against the stand-alone pass on the same stored values, for one and two groups, both activations, both passes."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(9300 + 7 * tile + (prec == 'bf16s'))
    lay = L()
    s16 = prec == 'bf16s'
    rnd = _bf16_round if s16 else (lambda a: np.asarray(a, np.float32).astype(np.float64))
    x, W = rnd(rng.uniform(-1, 1, (N, Ci, Ti, H, H))), rnd(rng.randn(Co, Ci, kt, 4, 4) * 0.1)
    gy = rnd(rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2))
    xd, wd, gyd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), lay.act_to_dev(dev(gy))
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision=prec)
    g.tile = tile
    if s16:
        ops = dict(x=xd.to(torch.bfloat16), w=wd.to(torch.bfloat16), wd=wd.to(torch.bfloat16), gy=gyd.to(torch.bfloat16))
    else:
        ops = dict(x=hl.split_planes(xd), w=hl.split_planes(wd), wd=hl.split_planes(wd, run=16 * kt * 16 * Ci), gy=hl.split_planes(gyd))
    odt = torch.bfloat16 if s16 else torch.float32
    ws = torch.empty(hl.bn_workspace_floats(max(Ci, Co, 64)), device="cuda")
    for kind in ('dgrad', 'fprop'):
        C_out = Ci if kind == 'dgrad' else Co
        oshape = (N, Ti, H, H, Ci) if kind == 'dgrad' else (N, g.To, g.Ho, g.Wo, Co)
        M = int(np.prod(oshape[:-1]))

        def launch(out, ep=None):
            if kind == 'dgrad':
                return hl.conv_dgrad(g, ops['gy'], ops['wd'], None, out, ep=ep, must_fuse=ep is not None)
            return hl.conv_fprop(g, ops['x'], ops['w'], None, out, ep=ep, must_fuse=ep is not None)
        plain = torch.empty(oshape, device="cuda", dtype=odt)
        launch(plain)
        ybn = (torch.randn((M, C_out), device="cuda") * 1.3 + 0.2).to(odt)          # the saved BatchNorm input (bf16 in bf16 networks)
        gam = dev(1 + 0.1 * rng.randn(C_out))
        for groups in (1, 2):
            mg = M // groups
            st = []
            for gi in range(groups):
                s_ = torch.empty(4 * C_out, device="cuda")
                hl.bn_stats(mg, C_out, ybn[gi * mg:(gi + 1) * mg].float(), gam, dev(0.1 * rng.randn(C_out)), s_, None, None, ws)
                st.append(s_)
            for act in (hl.ACT_LRELU, hl.ACT_RELU):
                part = torch.full((hl.epilogue_part_floats(g, kind, groups),), float('nan'), device="cuda")
                ep = hl.epilogue(sums=hl.SUMS_BN_BWD, groups=groups, part=part, bn_y=ybn.view(oshape), bn_stats=st, bn_act=act, out_bf16=s16)
                out = torch.empty(oshape, device="cuda", dtype=odt)
                assert launch(out, ep)
                assert torch.equal(out, plain)
                for gi in range(groups):
                    sl = slice(gi * mg, (gi + 1) * mg)
                    gin, yin = out.view(M, C_out)[sl].contiguous(), ybn[sl].contiguous()
                    gref, dg_ref, db_ref = torch.empty((mg, C_out), device="cuda"), torch.zeros(C_out, device="cuda"), torch.zeros(C_out, device="cuda")
                    hl.bn_act_bwd(mg, C_out, gin, yin, st[gi], gam, act, gref, dg_ref, db_ref, ws)
                    got, dg, db = torch.empty((mg, C_out), device="cuda"), torch.zeros(C_out, device="cuda"), torch.zeros(C_out, device="cuda")
                    hl.bn_act_bwd_from_partials(mg, C_out, gin, yin, st[gi], gam, act, part[gi * 2 * C_out:], ep.n_slots, ep.slot_stride, got, dg, db, ws)
                    assert rel_l2(got, gref.cpu().double().numpy()) < 1e-5, (kind, groups, gi, act)
                    assert rel_l2(dg, dg_ref.cpu().double().numpy()) < 1e-5 and rel_l2(db, db_ref.cpu().double().numpy()) < 1e-5
    # the kernels of the fp32-MFMA family refuse the combination with bf16 tensors (the caller then runs the stand-alone pass)
    if s16:
        g.tile = 1
        with pytest.raises(hl.McgError):
            hl.conv_dgrad(g, ops['gy'], ops['wd'], None, torch.empty((N, Ti, H, H, Ci), device="cuda", dtype=odt),
                          ep=hl.epilogue(sums=hl.SUMS_BN_BWD, groups=1, part=torch.zeros(hl.epilogue_part_floats(g, 'dgrad', 1), device="cuda"),
                                         bn_y=torch.zeros((N, Ti, H, H, Ci), device="cuda", dtype=odt), bn_stats=[torch.ones(4 * Ci, device="cuda")],
                                         bn_act=hl.ACT_RELU, out_bf16=True), must_fuse=True)


SPLIT_CASES = [(2, 7, 16, 64, 128, 4),      # 3-D, Ci = 64 (dgrad: the 256 x 64 tile)
               (3, 1, 16, 128, 64, 1),      # ragged 256-row tile; Co = 64
               (1, 5, 8, 256, 256, 4),      # long K, the 256 x 256 tile when asked for
               (2, 1, 32, 16, 32, 1),       # the narrowest layer the split form admits (one group of 16 channels)
               (5, 1, 8, 128, 512, 1)]


def test_split_planes_are_an_exact_expansion(hl):
    """mcg_split_planes: hi + mid + lo == v exactly (three bf16 terms carry the 24 bits of an fp32), each term the bf16 rounding of
    what the terms before it left; both run lengths (channels-last groups of 16, planes of 16 filters)."""
    torch.manual_seed(5)
    v = torch.randn((37, 5, 48), device="cuda") * torch.logspace(-6, 6, 48, device="cuda")
    v[0, 0, :4] = torch.tensor([0.0, -0.0, 1.0, -3.0e-39], device="cuda")
    for run, shape in ((16, (37, 5, 3, 4, 16)), (16 * 5 * 3, None)):
        s = hl.split_planes(v.view(37, 5 * 48) if shape is None else v, run=run)
        if shape is None:
            pl = s.view(37 * 240 // run, 4, run)                    # [run index][plane][position]
            src = v.view(-1, run)
            hi, mid, lo, z = (pl[:, i] for i in range(4))
        else:
            pl = s.view(shape)
            src = v.view(37, 5, 3, 16)
            hi, mid, lo, z = (pl[:, :, :, i] for i in range(4))
        assert torch.equal(hi, src.to(torch.bfloat16))
        r1 = src - hi.float()
        assert torch.equal(mid, r1.to(torch.bfloat16))
        r2 = r1 - mid.float()
        assert torch.equal(lo, r2.to(torch.bfloat16))                 # (z, the padding plane, is left as it was)
        big = src.abs() > 1e-30                                      # (bf16 keeps fp32's exponent range: only subnormal leftovers are lost)
        assert torch.equal((hi.double() + mid.double() + lo.double())[big], src.double()[big])


def test_split_planes_multi_equals_the_single_launches(hl):
    """mcg_split_planes_multi (ABI 6): several (source, run) segments in one launch -- the filters of an 'f32x3' network after its
    Adam update -- write bit for bit what one mcg_split_planes per segment writes, into destinations of different sizes (incl. a
    segment smaller than a block and one larger than the per-segment block cap), and leave the padding planes alone; bad segments
    are refused."""
    torch.manual_seed(9)
    srcs = [(torch.randn((64, 4 * 16 * 64), device="cuda"), 16), (torch.randn((64, 4 * 16 * 64), device="cuda"), 16 * 4 * 16 * 64),
            (torch.randn((16, 32), device="cuda"), 16), (torch.randn((512, 64 * 128), device="cuda") * 1e-3, 16),
            (torch.randn((512, 64 * 128), device="cuda"), 16 * 64 * 128)]
    want = [hl.split_planes(t, run=r, out=torch.full((t.shape[0], 4 * t.shape[1]), 7.0, device="cuda", dtype=torch.bfloat16)) for t, r in srcs]
    got = [torch.full((t.shape[0], 4 * t.shape[1]), 7.0, device="cuda", dtype=torch.bfloat16) for t, _ in srcs]
    hl.split_planes_multi([(t, r, o) for (t, r), o in zip(srcs, got)])
    for w, g in zip(want, got):
        assert torch.equal(w.view(torch.int16), g.view(torch.int16))
    with pytest.raises(hl.McgError):
        hl.split_planes_multi([(srcs[2][0], 24, got[2])])             # run not a multiple of 16
    with pytest.raises(hl.McgError):
        hl.split_planes_multi([(srcs[2][0], 16, got[2])] * 33)        # more segments than one launch takes


@pytest.mark.parametrize("case", SPLIT_CASES)
@pytest.mark.parametrize("tile", [0, 8, 10, 2007])           # (10: 128x128, two blocks per CU; 2007: the K range of a tile over four blocks)
def test_split_fp32_products_match_the_oracle(hl, case, tile):
    """MCG_PREC_SPLIT: fp32 operands as three bf16 terms, six bf16 products per fp32 product on the bf16 MFMA, fp32 accumulation --
    forward, input gradient and weight gradient on full-mantissa fp32 inputs against the float64 oracle at the fp32 tolerances, and no worse than the
    fp32-MFMA kernels on the same inputs (the dropped products are below 2^-24 of |a||b|)."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(9100 + SPLIT_CASES.index(case))
    lay = L()
    x = rng.uniform(-1, 1, (N, Ci, Ti, H, H)).astype(np.float32).astype(np.float64)
    W = (rng.randn(Co, Ci, kt, 4, 4) * 0.1).astype(np.float32).astype(np.float64)
    b = rng.randn(Co).astype(np.float32).astype(np.float64)
    gy = rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2).astype(np.float32).astype(np.float64)
    y_ref = F.conv3d_fwd(x, W, b, (1, 2, 2), (0, 1, 1))
    gx_ref, _, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
    xd, wd, bd, gyd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b), lay.act_to_dev(dev(gy))
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='f32x3')
    g.tile = tile
    g32 = hl.make_geom(N, Ti, H, H, Ci, Co, kt)
    xs, ws, gys = hl.split_planes(xd), hl.split_planes(wd), hl.split_planes(gyd)
    wsd = hl.split_planes(wd, run=16 * kt * 16 * Ci)
    assert xs.shape[-1] == 4 * Ci and ws.shape[-1] == 4 * Ci and gys.shape[-1] == 4 * Co
    yd = torch.full((N, g.To, g.Ho, g.Wo, Co), 3.0, device="cuda")
    hl.conv_fprop(g, xs, ws, bd, yd)
    y32 = torch.empty_like(yd)
    hl.conv_fprop(g32, xd, wd, bd, y32)
    err, err32 = rel_l2(lay.act_from_dev(yd, Co), y_ref), rel_l2(lay.act_from_dev(y32, Co), y_ref)
    assert err < 2e-6 and err < 2 * err32 + 1e-7, (err, err32)
    if tile >= 1000:                                                 # (the remaining checks -- fused epilogues, weight gradient -- have no K split;
        g.tile = tile % 1000                                         #  partial tiles are added in another order: not bit for bit the unsplit y)
        hl.conv_fprop(g, xs, ws, bd, yd)
    # statistics epilogue: the same output, the sums of it
    part = torch.zeros(hl.epilogue_part_floats(g, 'fprop', 1), device="cuda")
    ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part)
    y2 = torch.empty_like(yd)
    assert hl.conv_fprop(g, xs, ws, bd, y2, ep=ep, must_fuse=True)
    assert torch.equal(y2, yd)
    sums = part[:ep.n_slots * ep.slot_stride].view(ep.n_slots, ep.slot_stride).double().sum(0)
    v = y2.double().view(-1, Co)
    assert torch.allclose(sums[:Co], v.sum(0), rtol=1e-5, atol=1e-3) and torch.allclose(sums[Co:2 * Co], (v * v).sum(0), rtol=1e-5, atol=1e-3)
    if Ci >= 64:                                                    # input gradient: the LDS-DMA dgrad tiles need >= 64 output columns
        gxd = torch.full((N, Ti, H, H, Ci), 7.0, device="cuda")
        g.tile = tile
        hl.conv_dgrad(g, gys, wsd, None, gxd)
        g.tile = tile % 1000
        gx32 = torch.empty_like(gxd)
        hl.conv_dgrad(g32, gyd, wd, None, gx32)
        err, err32 = rel_l2(lay.act_from_dev(gxd, Ci), gx_ref), rel_l2(lay.act_from_dev(gx32, Ci), gx_ref)
        assert err < 2e-6 and err < 2 * err32 + 1e-7, (err, err32)
    # weight gradient: the sum runs over pixels -- 16 pixels x 4 planes per K-step from the same split tensors; added onto dw
    if Co >= 128 and Ci >= 64:
        _, gW_ref, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
        dwd, dw32 = torch.ones_like(wd), torch.ones_like(wd)
        hl.conv_wgrad(g, xs, gys, dwd)
        hl.conv_wgrad(g32, xd, gyd, dw32)
        err, err32 = rel_l2(lay.conv_w_from_dev(dwd, Ci, 3), gW_ref + 1), rel_l2(lay.conv_w_from_dev(dw32, Ci, 3), gW_ref + 1)
        assert err < 2e-6 and err < 2 * err32 + 1e-7, (err, err32)
    else:
        with pytest.raises(hl.McgError):                            # narrower layers keep the fp32 kernels
            hl.conv_wgrad(g, xs, gys, torch.zeros_like(wd))


PATCH_CASES = [(2, 7, 32, 64, 128, 4),       # D_V dc2's geometry (two clips)
               (3, 1, 32, 64, 128, 1),       # D_I dc2 / G dc4 (2-D)
               (1, 5, 32, 64, 64, 4),        # one y channel chunk
               (2, 4, 32, 64, 256, 4)]       # To = 1: every frame of x sees exactly one temporal tap


@pytest.mark.parametrize("case", PATCH_CASES)
def test_patch_stationary_input_gradient_split_fp32(hl, case):
    """tile code 9 with MCG_PREC_SPLIT operands (fp32 values as three bf16 terms): full-mantissa inputs, the oracle at the fp32
    tolerance and no worse than the fp32-MFMA kernels; bias + statistics, and the mask-multiply epilogue, on the same output."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(9200 + PATCH_CASES.index(case))
    lay = L()
    x = rng.uniform(-1, 1, (N, Ci, Ti, H, H))
    W = (rng.randn(Co, Ci, kt, 4, 4) * 0.1).astype(np.float32).astype(np.float64)
    gy = rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2).astype(np.float32).astype(np.float64)
    gx_ref, _, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
    wd, gyd = lay.conv_w_to_dev(dev(W)), lay.act_to_dev(dev(gy))
    gys, wsd = hl.split_planes(gyd), hl.split_planes(wd, run=16 * kt * 16 * Ci)
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='f32x3')
    g.tile = 9
    gxd = torch.full((N, Ti, H, H, Ci), 7.0, device="cuda")
    hl.conv_dgrad(g, gys, wsd, None, gxd)
    gx32 = torch.empty_like(gxd)
    hl.conv_dgrad(hl.make_geom(N, Ti, H, H, Ci, Co, kt), gyd, wd, None, gx32)
    err, err32 = rel_l2(lay.act_from_dev(gxd, Ci), gx_ref), rel_l2(lay.act_from_dev(gx32, Ci), gx_ref)
    assert err < 2e-6 and err < 2 * err32 + 1e-7, (err, err32)
    b = dev(rng.randn(Ci))
    part = torch.zeros(hl.epilogue_part_floats(g, 'dgrad', 1), device="cuda")
    ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part)
    gxb = torch.empty_like(gxd)
    assert hl.conv_dgrad(g, gys, wsd, b, gxb, ep=ep, must_fuse=True)
    assert torch.equal(gxb, gxd + b)
    sums = part[:ep.n_slots * ep.slot_stride].view(ep.n_slots, ep.slot_stride).double().sum(0)
    v = gxb.double().view(-1, Ci)
    assert torch.allclose(sums[:Ci], v.sum(0), rtol=1e-5, atol=1e-3) and torch.allclose(sums[Ci:2 * Ci], (v * v).sum(0), rtol=1e-5, atol=1e-3)
    bits = torch.randint(0, 2, (N * Ti * H * H, Ci), device="cuda", dtype=torch.int64)
    words = (bits.view(-1, Ci // 32, 32) << torch.arange(32, device="cuda")).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()
    part = torch.zeros(hl.epilogue_part_floats(g, 'dgrad', 1), device="cuda")
    ep = hl.epilogue(mask_in=words, sums=hl.SUMS_COL, groups=1, part=part)
    gxm = torch.empty_like(gxd)
    assert hl.conv_dgrad(g, gys, wsd, None, gxm, ep=ep, must_fuse=True)
    assert torch.equal(gxm.view(-1, Ci), gxd.view(-1, Ci) * torch.where(bits.bool(), 1.0, 0.2).float())


@pytest.mark.parametrize("case", PATCH_CASES)
def test_patch_stationary_input_gradient(hl, case):
    """mcg_conv_dgrad tile code 9 (bf16-stored operands, Ci = 64, 16 x 16 small side): the four parity classes of a frame in one
    block, y patch in LDS.  Against the float64 oracle and, bit for bit, against the per-class kernels' result for the same K
    order is not required -- the sum order differs -- so: oracle at the fp32 tolerance; every launch form the step uses."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(9100 + PATCH_CASES.index(case))
    lay = L()
    x, W = _bf16_round(rng.uniform(-1, 1, (N, Ci, Ti, H, H))), _bf16_round(rng.randn(Co, Ci, kt, 4, 4) * 0.1)
    gy = _bf16_round(rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2))
    gx_ref, _, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
    wd, gyd = lay.conv_w_to_dev(dev(W)), lay.act_to_dev(dev(gy))
    w16, gy16 = wd.to(torch.bfloat16), gyd.to(torch.bfloat16)
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='bf16s')
    g.tile = 9
    gxd = torch.full((N, Ti, H, H, Ci), 7.0, device="cuda")
    hl.conv_dgrad(g, gy16, w16, None, gxd)
    assert rel_l2(lay.act_from_dev(gxd, Ci), gx_ref) < BWD_TOL
    # bias + statistics + bf16 output (the generator's dc4 forward: model/net.py:113)
    b = dev(rng.randn(Ci))
    gx16 = torch.empty_like(gxd, dtype=torch.bfloat16)
    part = torch.zeros(hl.epilogue_part_floats(g, 'dgrad', 1), device="cuda")
    ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part, out_bf16=True)
    assert hl.conv_dgrad(g, gy16, w16, b, gx16, ep=ep, must_fuse=True)
    assert torch.equal(gx16, (gxd + b).to(torch.bfloat16))
    sums = part[:ep.n_slots * ep.slot_stride].view(ep.n_slots, ep.slot_stride).double().sum(0)
    v = gx16.double().view(-1, Ci)
    assert torch.allclose(sums[:Ci], v.sum(0), rtol=1e-5, atol=1e-3) and torch.allclose(sums[Ci:2 * Ci], (v * v).sum(0), rtol=1e-5, atol=1e-3)
    # two groups (real | fake halves of the batch) when N is even
    if N % 2 == 0:
        part2 = torch.zeros(hl.epilogue_part_floats(g, 'dgrad', 2), device="cuda")
        ep2 = hl.epilogue(sums=hl.SUMS_STATS, groups=2, part=part2)
        gx2 = torch.empty_like(gxd)
        assert hl.conv_dgrad(g, gy16, w16, None, gx2, ep=ep2, must_fuse=True) and torch.equal(gx2, gxd)
        s2 = part2[:ep2.n_slots * ep2.slot_stride].view(ep2.n_slots, ep2.slot_stride).double().sum(0)
        half = gxd.double().view(N, -1, Ci)
        assert torch.allclose(s2[:Ci], half[:N // 2].reshape(-1, Ci).sum(0), rtol=1e-5, atol=1e-3)
        assert torch.allclose(s2[2 * Ci:3 * Ci], half[N // 2:].reshape(-1, Ci).sum(0), rtol=1e-5, atol=1e-3)
    # leaky_relu mask multiply + column sums (D's dc2 input gradient)
    bits = torch.randint(0, 2, (N * Ti * H * H, Ci), device="cuda", dtype=torch.int64)
    words = (bits.view(-1, Ci // 32, 32) << torch.arange(32, device="cuda")).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()
    part = torch.zeros(hl.epilogue_part_floats(g, 'dgrad', 1), device="cuda")
    ep = hl.epilogue(mask_in=words, sums=hl.SUMS_COL, groups=1, part=part)
    gxm = torch.empty_like(gxd)
    assert hl.conv_dgrad(g, gy16, w16, None, gxm, ep=ep, must_fuse=True)
    want = gxd.view(-1, Ci) * torch.where(bits.bool(), 1.0, 0.2).float()
    assert torch.equal(gxm.view(-1, Ci), want)
    sums = part[:ep.n_slots * ep.slot_stride].view(ep.n_slots, ep.slot_stride).double().sum(0)
    assert torch.allclose(sums[:Ci], want.double().sum(0), rtol=1e-5, atol=1e-3)
    # accumulate onto x; a geometry it does not cover is refused
    gxa = torch.full((N, Ti, H, H, Ci), 0.5, device="cuda")
    hl.conv_dgrad(g, gy16, w16, None, gxa, accumulate=True)
    assert rel_l2(lay.act_from_dev(gxa, Ci), gx_ref + 0.5) < BWD_TOL
    gn = hl.make_geom(2, 5, 16, 16, 64, 128, 4, precision='bf16s')
    gn.tile = 9
    with pytest.raises(hl.McgError):
        hl.conv_dgrad(gn, torch.zeros((2, 2, 8, 8, 128), device="cuda", dtype=torch.bfloat16),
                      torch.zeros((128, 4, 4, 4, 64), device="cuda", dtype=torch.bfloat16), None, torch.zeros((2, 5, 16, 16, 64), device="cuda"))


def test_concat_label_planes(hl):
    """mcg_concat_label_planes against Updater.concat_label_video's arithmetic (model/updater.py:65-76): the clip's channels, +1 on
    the item's label plane and -1 on the others, zero padding; dl = 0 is the channel slice used on the way back."""
    rng = np.random.RandomState(3)
    n, T, H, c, dl = 3, 2, 8, 3, 6
    x = dev(rng.randn(n, T, H, H, 4))
    labels = dev(np.array([5, 0, 2]), torch.int32)
    out = hl.concat_label_planes(x, c, dl, labels, torch.full((n, T, H, H, 12), 7.0, device="cuda"))
    want = torch.zeros((n, T, H, H, 12), device="cuda")
    want[..., :c] = x[..., :c]
    want[..., c:c + dl] = -1.0
    for i, lab in enumerate((5, 0, 2)):
        want[i, ..., c + lab] = 1.0
    assert torch.equal(out, want)
    back = hl.concat_label_planes(out, c, 0, None, torch.full((n, T, H, H, 4), 7.0, device="cuda"))
    want_b = torch.zeros_like(back)
    want_b[..., :c] = x[..., :c]
    assert torch.equal(back, want_b)
    with pytest.raises(hl.McgError):
        hl.concat_label_planes(x, c, dl, labels, torch.empty((n, T, H, H, 8), device="cuda"))      # 3 + 6 channels do not fit 8


@pytest.mark.parametrize("case", [(2, 5, 32, 3, 64, 4), (3, 1, 32, 3, 64, 1), (2, 6, 64, 3, 64, 4), (2, 7, 16, 8, 64, 4), (2, 4, 8, 64, 160, 4)])
def test_bf16_y_beside_fp32_clip(hl, case):
    """MCG_PREC_BF16_Y16 ('bf16y'): the y-side tensor bf16 in memory, x and w fp32 -- the clip-side layers of bf16 networks (dc1's output
    gradient in D, the last layer's input in G are 16x the clip).  On bf16-representable values the launch must reproduce the 'bf16'
    launch on fp32 tensors: bit for bit in the input gradient (same MFMA sequence), to summation order in the weight gradient; both
    match the oracle.  Geometries without such a kernel are refused."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(7000 + Ci + H)
    lay = L()
    x, W = _bf16_round(rng.uniform(-1, 1, (N, Ci, Ti, H, H))), _bf16_round(rng.randn(Co, Ci, kt, 4, 4) * 0.1)
    gy = _bf16_round(rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2))
    gx_ref, gW_ref, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
    xd, wd, gyd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), lay.act_to_dev(dev(gy))
    gy16 = gyd.to(torch.bfloat16)
    Cip = xd.shape[-1]
    cv = Ci if Cip != Ci else 0
    g1, g2 = hl.make_geom(N, Ti, H, H, Cip, Co, kt, precision='bf16', ci_valid=cv), hl.make_geom(N, Ti, H, H, Cip, Co, kt, precision='bf16y', ci_valid=cv)
    for tile in (0, 3, 103, 201):
        g1.tile = g2.tile = tile
        dw1, dw2 = torch.zeros_like(wd), torch.zeros_like(wd)
        hl.conv_wgrad(g1, xd, gyd, dw1)
        hl.conv_wgrad(g2, xd, gy16, dw2)
        assert rel_l2(lay.conv_w_from_dev(dw2, Ci, 3), gW_ref) < BWD_TOL, tile
        assert rel_l2(dw2, dw1.cpu().double().numpy()) < 1e-6, tile
    g1.tile = g2.tile = 0
    if hl.dgrad_c4_mfma_covers(g2):
        gx1, gx2 = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
        hl.conv_dgrad(g1, gyd, wd, None, gx1)
        hl.conv_dgrad(g2, gy16, wd, None, gx2)
        assert torch.equal(gx1, gx2) and rel_l2(lay.act_from_dev(gx2, Ci), gx_ref) < BWD_TOL
    else:
        with pytest.raises(hl.McgError):                               # (no kernel reads a bf16 y beside fp32 filters there)
            hl.conv_dgrad(g2, gy16, wd, None, torch.zeros_like(xd))
    with pytest.raises(hl.McgError):
        hl.conv_wgrad(g2, xd, gyd, torch.zeros_like(wd))                # an fp32 y where the geometry promises bf16
    # a plain bf16 output of the 4-channel layers' forward kernel (G's last layer read backwards) equals the rounded fp32 output
    if Cip == 4 and Co == 64:
        y32 = torch.empty((N, g1.To, g1.Ho, g1.Wo, Co), device="cuda")
        hl.conv_fprop(g1, xd, wd, None, y32)
        y16 = torch.empty_like(y32, dtype=torch.bfloat16)
        hl.conv_fprop(g1, xd, wd, None, y16)
        assert torch.equal(y16, y32.to(torch.bfloat16))


@pytest.mark.parametrize("case", [(2, 6, 64, 4), (3, 1, 64, 1), (4, 5, 32, 4), (2, 1, 32, 1), (5, 16, 64, 4), (140, 5, 64, 4), (600, 1, 32, 1)])
def test_first_layer_weight_gradient_of_bf16_networks(hl, case):
    """Round 6: wgrad_c4_bf16_kernel (tile code 6 on a 'bf16y' launch: y bf16 in memory beside the fp32 clip -- the weight gradient of
    D's dc1 and of G's dc5 in bf16 networks, model/net.py:148,189 / :114 backwards): patch ring + y tile in LDS, both MFMA operands
    through the transposing read.  On bf16-representable inputs every product is exact, so the kernel must equal the generic tile
    (code 0) to fp32 summation order and the float64 oracle to the backward tolerance; Wo = 32 / 16, 3-D and 2-D, frames split over
    blocks (5 clips x 16 frames), several batch items per block (140 clips: 560 (row block, item) pairs on 512 blocks; 600 frames)."""
    N, Ti, H, kt = case
    Ci, Co = 3, 64
    rng = np.random.RandomState(7100 + N + Ti + H)
    lay = L()
    x = _bf16_round(rng.uniform(-1, 1, (N, Ci, Ti, H, H)))
    gy = _bf16_round(rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2))
    xd, gyd = lay.act_to_dev(dev(x)), lay.act_to_dev(dev(gy))
    gy16 = gyd.to(torch.bfloat16)
    g = hl.make_geom(N, Ti, H, H, 4, Co, kt, precision='bf16y', ci_valid=3)
    dw = {}
    for tile in (0, 6):
        g.tile = tile
        dw[tile] = torch.zeros((Co, kt, 4, 4, 4), device="cuda")
        hl.conv_wgrad(g, xd, gy16, dw[tile])
        hl.conv_wgrad(g, xd, gy16, dw[tile])                           # dw += ...: the second launch adds onto the first
    assert float(dw[6][..., 3].abs().max()) == 0.0                     # the padded channel has no gradient
    assert rel_l2(dw[6], dw[0].cpu().double().numpy()) < 2e-6, case
    if N <= 5:
        W0 = np.zeros((Co, Ci, kt, 4, 4))
        _, gW_ref, _ = F.conv3d_bwd(x, W0, gy, (1, 2, 2), (0, 1, 1))
        assert rel_l2(lay.conv_w_from_dev(dw[6], Ci, 3), 2 * gW_ref) < BWD_TOL, case
    g32 = hl.make_geom(N, Ti, H, H, 4, Co, kt, precision='bf16', ci_valid=3)
    g32.tile = 6
    with pytest.raises(hl.McgError):                                   # (an fp32 y under tile code 6 in a bf16 network: no such kernel)
        hl.conv_wgrad(g32, xd, gyd, torch.zeros_like(dw[0]))


@pytest.mark.parametrize("case", [(160, 1, 64, 3, 64, 1), (130, 5, 64, 3, 64, 4)])
def test_first_layer_input_gradient_walks_more_tiles_than_blocks(hl, case):
    """The first-layer input-gradient kernel is persistent (round 4): at most 1024 blocks walk the (batch item, 4 output rows) tiles.
    These geometries have 1280 / 1040 tiles, so blocks process a SECOND tile -- ring cleared by the first one's last frames, y
    prefetched across the tile boundary -- and the rows two tiles share are completed by atomics from different blocks.  fp32,
    bf16 MFMA and a bf16 y tensor against the float64 oracle; G's last layer forward (model/net.py:114) and D's first layer
    backwards (model/updater.py:113) at batch sizes the other tests do not reach."""
    N, Ti, H, Ci, Co, kt = case
    rng = np.random.RandomState(8100 + kt)
    lay = L()
    W = _bf16_round(rng.randn(Co, Ci, kt, 4, 4) * 0.1)
    gy = _bf16_round(rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2))
    x0 = np.zeros((N, Ci, Ti, H, H))
    gx_ref, _, _ = F.conv3d_bwd(x0, W, gy, (1, 2, 2), (0, 1, 1))
    wd, gyd = lay.conv_w_to_dev(dev(W)), lay.act_to_dev(dev(gy))
    for prec, ga in (('f32', gyd), ('bf16', gyd), ('bf16y', gyd.to(torch.bfloat16))):
        g = hl.make_geom(N, Ti, H, H, 4, Co, kt, precision=prec, ci_valid=Ci)
        assert hl.dgrad_c4_mfma_covers(g)
        gxd = torch.full((N, Ti, H, H, 4), 7.0, device="cuda")
        hl.conv_dgrad(g, ga, wd, None, gxd)
        assert rel_l2(lay.act_from_dev(gxd, Ci), gx_ref) < BWD_TOL, prec
        assert float(gxd[..., 3].abs().max()) == 0.0
        gx2 = torch.full_like(gxd, -3.0)
        hl.conv_dgrad(g, ga, wd, None, gx2)
        assert torch.equal(gx2, gxd), prec                           # (two addends per shared element: the order cannot matter)
