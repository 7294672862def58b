"""CPU-only checks of the sampling path: the new entry points validate their arguments on the host, generate_samples.py's
parser takes the new flags with today's defaults, and the BatchNorm fold the kernel implements is pinned against the oracle."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def fold_deconv(W, b, gamma, beta, mean, var, eps=2e-5):
    """NumPy statement of mcg_bn_fold_deconv on a Chainer deconvolution weight (Cin, Cout, kh, kw): the BatchNorm channel is Cout"""
    s = gamma / np.sqrt(var + eps)
    return W * s[None, :, None, None], b * s + beta - mean * s


def test_fold_equals_test_mode_batchnorm_behind_the_deconvolution():
    from oracle import functions as F
    rng = np.random.RandomState(3)
    ci, co = 6, 8
    x = rng.randn(3, ci, 4, 4)
    W, b = rng.randn(ci, co, 4, 4) * 0.2, rng.randn(co) * 0.3
    gamma, beta = rng.uniform(0.5, 1.5, co), rng.randn(co) * 0.2
    mean, var = rng.randn(co) * 0.05, rng.uniform(0.02, 0.2, co)
    ref = F.bn_test_fwd(F.deconv2d_fwd(x, W, b, 2, 1), gamma, beta, mean, var)
    Wf, bf = fold_deconv(W, b, gamma, beta, mean, var)
    got = F.deconv2d_fwd(x, Wf, bf, 2, 1)
    assert ref.dtype == np.float64 and ref.shape == (3, co, 8, 8)
    assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max()
    assert np.abs(np.maximum(got, 0) - F.relu_fwd(ref)).max() < 1e-12 * np.abs(ref).max()


def test_new_entry_points_validate_on_the_host(hl):
    lib = hl.load()
    assert lib.mcg_version() == 8 and hl.ABI_VERSION == 8
    one = ctypes.c_void_p(16)                        # a non-null pointer that is never dereferenced: every call below fails before a launch
    HW = 64 * 64
    # mcg_clip_to_u8(N, C, Cp, T, HW, in, bias, act, out, stride_n, stride_t, stream)
    assert lib.mcg_clip_to_u8(2, 3, 4, 16, HW, None, None, 0, one, 16 * HW * 3, HW * 3, None) == -1
    assert lib.mcg_clip_to_u8(2, 3, 4, 16, HW, one, None, 0, None, 16 * HW * 3, HW * 3, None) == -1
    assert lib.mcg_clip_to_u8(2, 3, 4, 16, HW, one, None, 0, one, 16 * HW * 3, HW * 3 - 1, None) == -1     # frames overlap
    assert lib.mcg_clip_to_u8(2, 3, 4, 16, HW, one, None, 0, one, -1, HW * 3, None) == -1
    assert lib.mcg_clip_to_u8(2, 3, 4, 16, HW, one, None, 0, one, 8 * HW * 3, HW * 3, None) == -1         # items overlap
    assert lib.mcg_clip_to_u8(2, 3, 4, 16, HW, one, None, 0, one, HW * 3, HW * 3, None) == -1             # neither (N,T) nor (T,N)
    assert lib.mcg_clip_to_u8(2, 5, 4, 16, HW, one, None, 0, one, 16 * HW * 5, HW * 5, None) == -1        # C > Cp
    assert lib.mcg_clip_to_u8(2, 3, 4, 16, HW, one, None, hl.ACT_RELU, one, 16 * HW * 3, HW * 3, None) == -1
    assert lib.mcg_clip_to_u8(2, 3, 8, 16, HW, one, None, 0, one, 16 * HW * 3, HW * 3, None) == -2        # the clip side only
    # mcg_bn_fold_deconv(rows, C, Cp, w, bias, gamma, beta, mean, var, eps, w_out, bias_out, stream)
    assert lib.mcg_bn_fold_deconv(16, 8, 8, None, one, one, one, one, one, 2e-5, one, one, None) == -1
    assert lib.mcg_bn_fold_deconv(16, 8, 8, one, one, None, one, one, one, 2e-5, one, one, None) == -1
    assert lib.mcg_bn_fold_deconv(16, 8, 8, one, one, one, one, one, None, 2e-5, one, one, None) == -1
    assert lib.mcg_bn_fold_deconv(16, 8, 8, one, one, one, one, one, one, 2e-5, None, one, None) == -1
    assert lib.mcg_bn_fold_deconv(16, 8, 8, one, one, one, one, one, one, 2e-5, one, None, None) == -1
    assert lib.mcg_bn_fold_deconv(0, 8, 8, one, one, one, one, one, one, 2e-5, one, one, None) == -1
    assert lib.mcg_bn_fold_deconv(16, 8, 6, one, one, one, one, one, one, 2e-5, one, one, None) == -1      # unpadded / Cp < C
    assert lib.mcg_bn_fold_deconv(16, 8, 8, one, one, one, one, one, one, -1.0, one, one, None) == -1


def test_relu_deconvolution_is_refused_where_the_store_cannot_carry_it(hl):
    """host-side: ReLU together with a split-K tile code, accumulate, or the clip-side layer (nothing is launched)"""
    lib = hl.load()
    one = ctypes.c_void_p(16)
    g = hl.make_geom(32, 1, 16, 16, 128, 256, 1)
    g.tile = 1203
    assert lib.mcg_conv_dgrad(ctypes.byref(g), one, one, one, one, hl.ACT_RELU, 0, None) == -2
    g.tile = 203
    assert lib.mcg_conv_dgrad(ctypes.byref(g), one, one, one, one, hl.ACT_RELU, 1, None) == -2
    g4 = hl.make_geom(32, 1, 64, 64, 4, 64, 1, ci_valid=3)
    assert lib.mcg_conv_dgrad(ctypes.byref(g4), one, one, one, one, hl.ACT_RELU, 0, None) == -2
    ep = hl.epilogue(sums=hl.SUMS_STATS, act=hl.ACT_RELU)
    ep.part = 16
    assert lib.mcg_conv_dgrad_ex(ctypes.byref(g), one, one, one, one, ctypes.byref(ep), None) == -2


def test_generate_samples_parser_takes_the_new_flags_and_keeps_the_defaults():
    import generate_samples as gs
    a = gs.parse_args(['w.npz', 'out'])
    assert (a.num, a.gpu, a.dim_zl, a.n_filters) == (36, -1, 0, 64)                      # today's
    assert (a.test_mode, a.labels, a.fix_content, a.fix_motion, a.video_len, a.seed, a.mfma) == (0, None, False, False, 16, None, 'f32')
    a = gs.parse_args(['w.npz', 'out', '--num', '4', '--test_mode', '1', '--dim_zl', '6', '--labels', '0,3,5,1', '--fix_content',
                       '--video_len', '24', '--seed', '7', '--mfma', 'bf16'])
    assert a.labels == [0, 3, 5, 1] and a.fix_content and not a.fix_motion and a.video_len == 24 and a.seed == 7 and a.mfma == 'bf16'
    assert gs.parse_args(['w.npz', 'out', '--test_mode', '1', '--dim_zl', '6', '--labels', '3', '--fix_motion']).labels == [3]
    for bad in (['--test_mode', '1', '--dim_zl', '6', '--labels', '6'],          # a label >= dim_zl
                ['--test_mode', '1', '--dim_zl', '6', '--labels', '0,-1'],
                ['--test_mode', '1', '--labels', '0'],                           # no label input
                ['--test_mode', '1', '--dim_zl', '6', '--labels', '0,1', '--num', '4'],     # neither one nor one per video
                ['--dim_zl', '6', '--labels', '0'],                              # choosing latents needs the test-mode path
                ['--fix_content'],
                ['--video_len', '0'],
                ['--mfma', 'fp8']):
        with pytest.raises(SystemExit):
            gs.parse_args(['w.npz', 'out'] + bad)
    with pytest.raises(ValueError):
        gs.parse_args(['w.npz', 'out', '--num', '5'])


def test_latents_follow_the_reference_draw_order():
    """ImageGenerator._latents draws what is missing in the order of oracle.net.gen_draw, and shares single rows"""
    from oracle import net as onet
    import model.net as mnet
    gen = mnet.ImageGenerator.__new__(mnet.ImageGenerator)          # (host logic only: no device, no weights)
    gen.dim_zc, gen.dim_zm, gen.dim_zl, gen.use_label, gen.video_len = 50, 10, 6, True, 16
    np.random.seed(5)
    labels, h0, e, zc = gen._latents(3, None, None, None, None, 24)
    ref = onet.gen_draw(np.random.RandomState(5), 3, dim_zl=6, video_len=24)
    assert np.array_equal(labels, ref['labels']) and np.array_equal(h0, ref['h0']) and np.array_equal(e, ref['e']) and np.array_equal(zc, ref['zc'])
    labels, h0, e, zc = gen._latents(3, 4, np.ones(50), None, np.zeros((24, 10)), 24)
    assert labels.tolist() == [4, 4, 4] and zc.shape == (3, 50) and float(zc.min()) == 1.0 and e.shape == (24, 3, 10)
    assert all(a.flags['C_CONTIGUOUS'] and a.flags['WRITEABLE'] for a in (labels, h0, e, zc))
    full = np.random.RandomState(0).randn(24, 5, 10).astype(np.float32)
    assert gen._latents(3, [0, 1, 2], None, None, full[:, [4, 0, 2]], 24)[2].flags['C_CONTIGUOUS']       # (a permuted view comes out dense)
    for bad in (dict(labels=[0, 6, 1]), dict(zc=np.ones((2, 50))), dict(e=np.zeros((16, 3, 10))), dict(h0=np.zeros((3, 9)))):
        kw = dict(labels=None, zc=None, h0=None, e=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            gen._latents(3, kw['labels'], kw['zc'], kw['h0'], kw['e'], 24)
    gen.dim_zl, gen.use_label = 0, False
    with pytest.raises(ValueError):
        gen._latents(3, [0, 1, 2], None, None, None, 16)
