"""The generator's sampling path on the GPU: the BatchNorm fold kernel, ReLU in the deconvolution's store, the clip leaving as
bytes, ImageGenerator.sample / sample_many against the float64 oracle in test mode, the latent controls, generate_samples.py's
test-mode flags, and the memory bounds.  Tolerances are those of the existing tests for the same quantities (named where used)."""
import gc
import os

import numpy as np
import pytest
import torch

from mocogan_chainer_amd import tiles
from oracle import functions as F
from oracle import net as onet

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 1e-5, 1e-4       # tests/test_gpu_ops.py: bn_act_fwd / the fp32 forward; the fp32 input-gradient GEMM
BF16_TOL = 2e-2                     # bf16 configuration, forward rel-L2 <= 2e-2 (tests/test_gpu_ops.py, tests/test_gpu_step.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "the gpu-marked tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def rel_l2(a, b):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _f64(p):
    return {k: (np.asarray(v).astype(np.float64) if np.asarray(v).dtype.kind == 'f' else v) for k, v in p.items()}


def quantise(x):
    """the reference's bytes (generate_samples.py:39) of a float32 array"""
    x = np.asarray(x, np.float32)
    return ((x / 2. + 0.5) * 255).astype(np.uint8)


def nontrivial_stats(gen, seed):
    """running statistics and affine parameters a trained generator could hold (defaults (0, 1) leave a nearly flat image)"""
    rng = np.random.RandomState(seed)
    p = dict(gen.serialize_dict())
    for l in (1, 2, 3, 4):
        c = p['bn%d/gamma' % l].shape[0]
        p['bn%d/avg_mean' % l] = rng.normal(0, 0.05, c).astype(np.float32)
        p['bn%d/avg_var' % l] = rng.uniform(0.02, 0.2, c).astype(np.float32)
        p['bn%d/gamma' % l] = rng.uniform(0.5, 1.5, c).astype(np.float32)
        p['bn%d/beta' % l] = rng.normal(0, 0.2, c).astype(np.float32)
    for l in (1, 2, 3, 4, 5):
        c = p['dc%d/b' % l].shape[0]
        p['dc%d/b' % l] = rng.normal(0, 0.1, c).astype(np.float32)
    gen.load_dict(p)
    return p


def oracle_clip(p, draw, T):
    d = {k: (v.astype(np.float64) if k != 'labels' and v is not None else v) for k, v in draw.items()}
    return onet.gen_forward(_f64(p), d, video_len=T, train=False)[0]


# ------------------------------------------------------------------------------------------------------------
# ops
# ------------------------------------------------------------------------------------------------------------
G_LAYERS = [(60, 512), (512, 256), (256, 128), (128, 64)]          # (Cin, Cout) of dc1..dc4 at n_filters = 64


@pytest.mark.parametrize("layer", G_LAYERS)
def test_fold_kernel_matches_the_float64_formula(hl, layer):
    import mocogan_chainer_amd.layout as lay
    ci, co = layer
    rng = np.random.RandomState(ci + co)
    W, b = rng.randn(ci, co, 4, 4) * 0.05, rng.randn(co) * 0.1
    gamma, beta = rng.uniform(0.5, 1.5, co), rng.normal(0, 0.2, co)
    mean, var = rng.normal(0, 0.05, co), rng.uniform(0.02, 0.2, co)
    s = gamma / np.sqrt(var + 2e-5)
    W_ref, b_ref = W * s[None, :, None, None], b * s + beta - mean * s
    wd, bd = lay.deconv_w_to_dev(dev(W)), lay.vec_to_dev(dev(b))
    w_out, b_out = torch.full_like(wd, 7.0), torch.full_like(bd, 7.0)
    hl.bn_fold_deconv(wd, bd, co, dev(gamma), dev(beta), dev(mean), dev(var), w_out, b_out)
    assert rel_l2(lay.deconv_w_from_dev(w_out, co), W_ref) < FWD_TOL
    assert rel_l2(b_out[:co], b_ref) < FWD_TOL
    # bias = NULL means zero
    hl.bn_fold_deconv(wd, None, co, dev(gamma), dev(beta), dev(mean), dev(var), w_out, b_out)
    assert rel_l2(b_out[:co], beta - mean * s) < FWD_TOL


def _relu_case(l, frames, seed):
    """dc<l> of the full-width generator as the library sees it: conv-form Ci = its output channels, Co = its input's"""
    cin, cout = G_LAYERS[l - 1]
    h = 4 << (l - 2)                                               # input extent of dc<l>
    rng = np.random.RandomState(seed)
    x = np.maximum(rng.randn(frames, cin, h, h), 0) * 0.7          # (a ReLU output, as in the network)
    W, b = rng.randn(cin, cout, 4, 4) * (1.0 / np.sqrt(4 * cin)), rng.randn(cout) * 0.3
    return x, W, b, h


F32_CASES = [(l, t) for l in (2, 3, 4) for t in (0, 1, 2, 3, 101, 103, 201, 202, 203, 7, 8, 10)
             if not (t == 10 and l == 4)]          # tile 10 on fp32 operands exists for Ci >= 128 only (include/mocogan_hip.h)
TILE9_ONLY_DC4 = lambda l, t: t == 9 and l != 4    # tile 9 is the Ci = 64, 16 x 16 kernel: dc4


@pytest.mark.parametrize("l,tile", F32_CASES)
def test_dgrad_relu_f32(hl, l, tile):
    """x = max(conv_transpose(y, w) + b, 0) against np.maximum(oracle deconv2d_fwd, 0): the shipped table's codes for G's dc2..dc4
    (fp32: 0 / 101 / 102 / 103 / 201 / 202 / 203 and, with the split-K part dropped, 1203 / 2203 -> 203), the other register-staged
    tiles, and the LDS-DMA kernels on fp32 operands (7 / 8; 10 where it exists: Ci >= 128).  Tolerance: test_conv_three_passes' dgrad."""
    import mocogan_chainer_amd.layout as lay
    frames = 32
    x, W, b, h = _relu_case(l, frames, 100 + l)
    ref = np.maximum(F.deconv2d_fwd(x, W, b, 2, 1), 0)
    cin, cout = G_LAYERS[l - 1]
    g = hl.make_geom(frames, 1, 2 * h, 2 * h, cout, cin, 1)
    g.tile = tile
    yd, wd, bd = lay.act_to_dev(dev(x)), lay.deconv_w_to_dev(dev(W)), dev(b)
    out = torch.full((frames, 1, 2 * h, 2 * h, cout), -3.0, device="cuda")
    hl.conv_dgrad(g, yd, wd, bd, out, act=hl.ACT_RELU)
    err = rel_l2(lay.act_from_dev(out, cout, 2), ref)
    print("dc%d tile %d relu f32 rel-L2 %.2e" % (l, tile, err))
    assert err < BWD_TOL
    assert float(out.min()) >= 0.0 and float((out == 0).float().mean()) > 0.05          # ReLU really clipped something
    hl.conv_dgrad_relu(g, yd, wd, bd, out)                          # the sampling path's wrapper: same launch
    assert rel_l2(lay.act_from_dev(out, cout, 2), ref) < BWD_TOL


@pytest.mark.parametrize("l,tile", [(l, t) for l in (2, 3, 4) for t in (0, 2, 3, 201, 203, 7, 8, 10, 9) if not TILE9_ONLY_DC4(l, t)])
def test_dgrad_relu_bf16_stored_out_bf16(hl, l, tile):
    """the same on bf16-stored operands with the bf16 store (what a bf16 network's sample() launches): the table's codes for these
    geometries (0 / 203 / 201 / 7 / 8 / 10, and 9 -- the patch kernel -- for dc4).  Tolerance: the bf16 one of
    test_conv_three_passes_bf16_mfma (general fp32 inputs)."""
    import mocogan_chainer_amd.layout as lay
    frames = 32
    x, W, b, h = _relu_case(l, frames, 200 + l)
    ref = np.maximum(F.deconv2d_fwd(x, W, b, 2, 1), 0)
    cin, cout = G_LAYERS[l - 1]
    g = hl.make_geom(frames, 1, 2 * h, 2 * h, cout, cin, 1, precision='bf16s')
    g.tile = tile
    yd, wd, bd = lay.act_to_dev(dev(x)).to(torch.bfloat16), lay.deconv_w_to_dev(dev(W)).to(torch.bfloat16), dev(b)
    out = torch.full((frames, 1, 2 * h, 2 * h, cout), -3.0, device="cuda", dtype=torch.bfloat16)
    hl.conv_dgrad(g, yd, wd, bd, out, act=hl.ACT_RELU)
    err = rel_l2(lay.act_from_dev(out.float(), cout, 2), ref)
    print("dc%d tile %d relu bf16 rel-L2 %.2e" % (l, tile, err))
    assert err < BF16_TOL
    assert float(out.float().min()) >= 0.0 and float((out == 0).float().mean()) > 0.05
    out32 = torch.full(out.shape, -3.0, device="cuda")              # ... and with the fp32 store
    hl.conv_dgrad(g, yd, wd, bd, out32, act=hl.ACT_RELU)
    assert rel_l2(lay.act_from_dev(out32, cout, 2), ref) < BF16_TOL and float(out32.min()) >= 0.0


@pytest.mark.parametrize("l,tile", [(l, t) for l in (2, 3, 4) for t in (0, 7, 10, 9) if not TILE9_ONLY_DC4(l, t)])
def test_dgrad_relu_split_operands(hl, l, tile):
    """'f32x3': split operands in, fp32 + ReLU out (the fp32 tolerance: the split form is an fp32 product)"""
    import mocogan_chainer_amd.layout as lay
    frames = 32
    x, W, b, h = _relu_case(l, frames, 300 + l)
    ref = np.maximum(F.deconv2d_fwd(x, W, b, 2, 1), 0)
    cin, cout = G_LAYERS[l - 1]
    g = hl.make_geom(frames, 1, 2 * h, 2 * h, cout, cin, 1, precision='f32x3')
    g.tile = tile
    wd = lay.deconv_w_to_dev(dev(W))
    ys, ws = hl.split_planes(lay.act_to_dev(dev(x))), hl.split_planes(wd, run=16 * (wd.numel() // wd.shape[0]))
    out = torch.full((frames, 1, 2 * h, 2 * h, cout), -3.0, device="cuda")
    hl.conv_dgrad(g, ys, ws, dev(b), out, act=hl.ACT_RELU)
    err = rel_l2(lay.act_from_dev(out, cout, 2), ref)
    print("dc%d tile %d relu f32x3 rel-L2 %.2e" % (l, tile, err))
    assert err < BWD_TOL and float(out.min()) >= 0.0


def test_dgrad_relu_refusals(hl):
    """ReLU with a split-K tile code, accumulate or a sums epilogue: MCG_ERR_UNSUPPORTED, nothing written"""
    import mocogan_chainer_amd.layout as lay
    frames = 32
    x, W, b, h = _relu_case(3, frames, 1)
    g = hl.make_geom(frames, 1, 2 * h, 2 * h, 128, 256, 1)
    yd, wd, bd = lay.act_to_dev(dev(x)), lay.deconv_w_to_dev(dev(W)), dev(b)
    out = torch.full((frames, 1, 2 * h, 2 * h, 128), -3.0, device="cuda")
    for code in (1203, 2203, 1103):
        g.tile = code
        with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
            hl.conv_dgrad(g, yd, wd, bd, out, act=hl.ACT_RELU)
    g.tile = 203
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        hl.conv_dgrad(g, yd, wd, bd, out, act=hl.ACT_RELU, accumulate=True)
    part = torch.empty(hl.epilogue_part_floats(g, 'dgrad', 1), device="cuda")
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        hl._dgrad_ex(g, yd, wd, bd, out, hl.epilogue(sums=hl.SUMS_STATS, part=part, act=hl.ACT_RELU))
    torch.cuda.synchronize()
    assert float(out.max()) == -3.0 and float(out.min()) == -3.0
    # the table's split-K codes reach the launch without their split part
    tiles.table.set(tiles.geom_key("dgrad", hl.make_geom(frames, 1, 2 * h, 2 * h, 128, 256, 1), (hl.ACT_NONE, 0)), 2203)
    try:
        g0 = hl.make_geom(frames, 1, 2 * h, 2 * h, 128, 256, 1)
        hl.conv_dgrad_relu(g0, yd, wd, bd, out)
        assert rel_l2(lay.act_from_dev(out, 128, 2), np.maximum(F.deconv2d_fwd(x, W, b, 2, 1), 0)) < BWD_TOL
    finally:
        hl.reset_tuning()


# ------------------------------------------------------------------------------------------------------------
# bytes
# ------------------------------------------------------------------------------------------------------------
def _boundary_values():
    k = np.arange(256, dtype=np.float64)
    x = ((k / 255.0) - 0.5) * 2.0                                   # values whose byte boundary is an integer k
    x = x.astype(np.float32)
    v = np.concatenate([x, np.nextafter(x, np.float32(2)), np.nextafter(x, np.float32(-2)), np.nextafter(np.nextafter(x, np.float32(2)), np.float32(2)),
                        np.array([1.0, -1.0, 0.0, -0.0, 0.5, -0.5, 0.99999994, -0.99999994], np.float32)])
    return np.clip(v, -1.0, 1.0).astype(np.float32)


@pytest.mark.parametrize("hw", [64, 6])                             # 64: the packed 12-byte stores; 6: the byte-wise kernel
def test_clip_to_u8_equals_numpy_exactly(hl, hw):
    """(a) on one x held on the device the bytes equal ((x/2.+0.5)*255).astype(np.uint8) of NumPy exactly -- x = +-1 and values at
    and next to every byte boundary included -- in both output orders; padded strides leave the gaps untouched"""
    N, T, C, Cp = 3, 5, 3, 4
    rng = np.random.RandomState(hw)
    x = rng.uniform(-1, 1, (N, T, hw, Cp)).astype(np.float32)
    bv = _boundary_values()
    flat = x.reshape(-1)
    m = min(bv.size, flat.size)
    flat[:m] = bv[:m]
    xd = dev(x)
    want = quantise(x[..., :C])                                     # (N,T,HW,C)
    out = torch.zeros((N, T, hw, C), device="cuda", dtype=torch.uint8)
    hl.clip_to_u8(N, C, Cp, T, hw, xd, out)
    assert np.array_equal(out.cpu().numpy(), want)
    out_tn = torch.zeros((T, N, hw, C), device="cuda", dtype=torch.uint8)
    hl.clip_to_u8(N, C, Cp, T, hw, xd, out_tn, stride_n=hw * C, stride_t=N * hw * C)
    assert np.array_equal(out_tn.cpu().numpy(), want.transpose(1, 0, 2, 3))
    pad = 8
    out_p = torch.full((N, T, hw * C + pad), 77, device="cuda", dtype=torch.uint8)
    hl.clip_to_u8(N, C, Cp, T, hw, xd, out_p, stride_n=T * (hw * C + pad), stride_t=hw * C + pad)
    got = out_p.cpu().numpy()
    assert np.array_equal(got[..., :hw * C].reshape(N, T, hw, C), want) and (got[..., hw * C:] == 77).all()
    # bias + tanh taken over from the element-wise pass: the bytes of what that pass would have stored
    pre = dev(rng.randn(N, T, hw, Cp).astype(np.float32) * 1.5)
    bias = dev(np.array([0.1, -0.2, 0.3, 0.0], np.float32))
    one_bias = torch.cat((torch.ones(Cp, device="cuda"), bias))
    xt = torch.empty_like(pre)
    hl.bn_act_fwd(pre.numel() // Cp, Cp, pre, one_bias, hl.ACT_TANH, xt)
    hl.clip_to_u8(N, C, Cp, T, hw, pre, out, bias=bias, act=hl.ACT_TANH)
    assert np.array_equal(out.cpu().numpy(), quantise(xt.cpu().numpy()[..., :C]))


# ------------------------------------------------------------------------------------------------------------
# network
# ------------------------------------------------------------------------------------------------------------
def _gen(nf, dim_zl, seed, video_len=16):
    from model.net import ImageGenerator
    np.random.seed(seed)
    g = ImageGenerator(dim_zl=dim_zl, n_filters=nf, video_len=video_len)
    p = nontrivial_stats(g, seed + 1)
    return g, p


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("precision", ['f32', 'f32x3', 'bf16'])
@pytest.mark.parametrize("nf,dim_zl,T", [(8, 0, 16), (8, 6, 24), (64, 6, 16), (64, 0, 24)])
def test_sample_matches_the_oracle_in_test_mode(hl, nf, dim_zl, T, precision, monkeypatch):
    """ImageGenerator.sample against oracle.net.gen_forward(train=False) in float64, with non-trivial running statistics, from
    np.random draws and from the same draws given explicitly.  rel-L2 < 1e-5 for f32 / f32x3 (the bound of
    test_generator_call_matches_oracle_under_the_numpy_generator), < 2e-2 for bf16 (as x_fake in
    test_update_core_bf16_mfma_one_step).  State and parameters stay bit-identical; np.random advances as under __call__."""
    from model.net import config
    if precision == 'f32x3':
        monkeypatch.setenv('MCG_SPLIT', 'always')                   # (no table in the tests: take the split form wherever it exists)
    n = 3
    g, p = _gen(nf, dim_zl, 40 + nf + dim_zl)
    g.impl.set_precision(precision)
    before = g.serialize_dict()
    p16_before = g.impl.fp.p16.clone() if precision == 'bf16' else None
    split_before = hl.split_launches
    np.random.seed(17)
    x, labels = g.sample(n, video_len=T)
    state_sample = np.random.get_state()
    assert tuple(x.shape) == (T, n, 3, 64, 64) and x.is_cuda and x.dtype == torch.float32
    draw = onet.gen_draw(np.random.RandomState(17), n, dim_zl=dim_zl, video_len=T)
    x_ref = oracle_clip(p, draw, T)
    assert (labels is None) == (dim_zl == 0) and (labels is None or np.array_equal(labels, draw['labels']))
    tol = BF16_TOL if precision == 'bf16' else 1e-5
    err = rel_l2(x, x_ref)
    print("sample nf=%d dim_zl=%d T=%d %s: rel-L2 %.2e, oracle std %.2f range (%.4f, %.4f)" % (nf, dim_zl, T, precision, err, x_ref.std(), x_ref.min(), x_ref.max()))
    assert err < tol
    assert x_ref.std() > 0.2                                        # the statistics above leave a real image to compare
    if precision == 'bf16' and nf == 64:
        assert err > 1e-5, "bf16 rounding left no trace: the bf16 kernels did not run"
    if precision == 'f32x3' and nf == 64:
        assert hl.split_launches - split_before == 3, "the split form of dc2..dc4 did not run"
    # the same latents, given
    x2, labels2 = g.sample(n, labels=draw['labels'], zc=draw['zc'], h0=draw['h0'], e=draw['e'], video_len=T)
    assert rel_l2(x2, x_ref) < tol and (labels2 is None or np.array_equal(labels2, draw['labels']))
    after = g.serialize_dict()
    assert set(after) == set(before)
    for k in before:
        assert np.array_equal(np.asarray(before[k]), np.asarray(after[k])), k
    if p16_before is not None:
        assert torch.equal(p16_before, g.impl.fp.p16)
    if T == g.video_len:                                            # __call__ draws the constructor's video_len
        np.random.seed(17)
        prev, config.train = config.train, False
        try:
            xc, _ = g(n)
        finally:
            config.train = prev
        assert _state_equal(state_sample, np.random.get_state())
        assert rel_l2(xc, x_ref) < tol                              # (and the unchanged __call__ in test mode is the same clip)


def _parent_error(g, p, n, seed, T=16):
    """max |x - x_oracle| of the unchanged __call__ under config.train = False, and the oracle's clip"""
    from model.net import config
    np.random.seed(seed)
    prev, config.train = config.train, False
    try:
        xc, _ = g(n)
    finally:
        config.train = prev
    draw = onet.gen_draw(np.random.RandomState(seed), n, dim_zl=g.dim_zl, video_len=T)
    x_ref = oracle_clip(p, draw, T)
    return float(np.abs(xc.cpu().double().numpy() - x_ref).max()), x_ref, draw


@pytest.mark.parametrize("nf", [8, 16])
def test_sample_bytes_against_the_oracle(hl, nf):
    """(b) sample(as_uint8=True) at f32 against the oracle's bytes: equal wherever the oracle's v = (x/2 + 0.5) * 255 lies farther
    than delta from an integer, at most 1 apart elsewhere.  delta = 127.5 * 4 * (max |x - x_oracle| of the unchanged test-mode
    __call__ on the same inputs; the factor 4 because folding reorders roundings), measured in the test.  Conditions: delta <= 0.0128
    (an error budget of 1e-4 on x) and an excluded share <= 3 %.
    Measured on the MI355X (profiles/sampler_notes.md): n_filters 8: max |x - x_oracle| 9.9e-07, delta 5.0e-04, excluded share 0.10 %,
    9 of 786432 bytes differ (all inside the band, by 1); n_filters 16: 2.0e-06, delta 1.0e-03, 0.20 %, 16 bytes differ."""
    n, seed = 4, 23
    g, p = _gen(nf, 6, 60 + nf)
    perr, x_ref, draw = _parent_error(g, p, n, seed)
    delta = 127.5 * 4 * perr
    v = (x_ref / 2. + 0.5) * 255
    near = np.abs(v - np.rint(v)) <= delta
    np.random.seed(seed)
    xb, _ = g.sample(n, as_uint8=True)
    assert xb.dtype == torch.uint8 and tuple(xb.shape) == (16, n, 3, 64, 64)
    got = xb.cpu().numpy().astype(np.int64)
    want = np.floor(v).astype(np.int64)
    diff = np.abs(got - want)
    print("bytes nf=%d: parent max|x - x_oracle| %.3e -> delta %.3e; excluded share %.4f; differing bytes %d of %d (all inside the band: %s)"
          % (nf, perr, delta, near.mean(), int((diff != 0).sum()), diff.size, bool((diff[~near] == 0).all())))
    assert delta <= 0.0128, (perr, delta)
    assert near.mean() <= 0.03, near.mean()
    assert (diff[~near] == 0).all()
    assert diff.max() <= 1


def test_sample_bytes_bf16_self_consistency(hl):
    """(c) a SELF-CONSISTENCY check (the float output carries the oracle comparison): at bf16 the bytes are within +-1 of the
    quantisation of the same latents' float output"""
    g, _ = _gen(16, 0, 91)
    g.impl.set_precision('bf16')
    np.random.seed(5)
    xf, _ = g.sample(4)
    np.random.seed(5)
    xb, _ = g.sample(4, as_uint8=True)
    d = np.abs(xb.cpu().numpy().astype(np.int64) - quantise(xf.cpu().numpy()).astype(np.int64))
    assert d.max() <= 1


# ------------------------------------------------------------------------------------------------------------
# controls
# ------------------------------------------------------------------------------------------------------------
def test_latent_controls(hl):
    g, _ = _gen(8, 6, 70)
    rng = np.random.RandomState(1)
    n, T = 6, 16
    zc = rng.normal(0, 0.33, (n, 50)).astype(np.float32)
    h0 = rng.normal(0, 0.33, (n, 10)).astype(np.float32)
    e = rng.normal(0, 0.33, (T, n, 10)).astype(np.float32)
    labels = np.array([0, 3, 5, 1, 3, 2])
    # rows 1 and 4 share every latent: the same video wherever it sits in the batch (not bit for bit: rows may fall into different tiles)
    zc[4], h0[4], e[:, 4] = zc[1], h0[1], e[:, 1]
    x, lab = g.sample(n, labels=labels, zc=zc, h0=h0, e=e)
    x = x.cpu().double().numpy()
    assert np.array_equal(lab, labels)
    assert rel_l2(x[:, 4], x[:, 1]) < 1e-6
    perm = np.array([4, 2, 0, 5, 3, 1])
    xp, _ = g.sample(n, labels=labels[perm], zc=zc[perm], h0=h0[perm], e=e[:, perm])
    assert rel_l2(xp.cpu().double().numpy(), x[:, perm]) < 1e-6
    xs, _ = g.sample(2, labels=labels[2:4], zc=zc[2:4], h0=h0[2:4], e=e[:, 2:4])       # ... and whatever the batch size
    assert rel_l2(xs.cpu().double().numpy(), x[:, 2:4]) < 1e-6
    # one content code for all, distinct motion: the videos differ; one motion path, distinct content: they differ too
    xc, _ = g.sample(n, labels=3, zc=zc[0], h0=h0, e=e)
    xc = xc.cpu().double().numpy()
    xm, _ = g.sample(n, labels=3, zc=zc, h0=h0[0], e=e[:, 0])
    xm = xm.cpu().double().numpy()
    for a in range(n):
        for b in range(a + 1, n):
            if (a, b) == (1, 4):
                continue                                            # (made equal above)
            assert rel_l2(xc[:, a], xc[:, b]) > 1e-3 and rel_l2(xm[:, a], xm[:, b]) > 1e-3
    assert rel_l2(xc[:, 4], xc[:, 1]) < 1e-6                        # (same motion, same content)
    # fixed content AND motion: identical videos
    xe, _ = g.sample(3, labels=3, zc=zc[0], h0=h0[0], e=e[:, 0])
    xe = xe.cpu().double().numpy()
    assert rel_l2(xe[:, 1], xe[:, 0]) < 1e-6 and rel_l2(xe[:, 2], xe[:, 0]) < 1e-6
    # changing one label changes that video only
    l2 = labels.copy()
    l2[2] = (l2[2] + 1) % 6
    x2, lab2 = g.sample(n, labels=l2, zc=zc, h0=h0, e=e)
    x2 = x2.cpu().double().numpy()
    assert np.array_equal(lab2, l2)
    assert rel_l2(x2[:, 2], x[:, 2]) > 1e-3
    keep = [i for i in range(n) if i != 2]
    assert rel_l2(x2[:, keep], x[:, keep]) < 1e-6
    with pytest.raises(ValueError):
        g.sample(n, labels=[0, 1, 2, 3, 4, 6])


def test_sample_many_equals_sample(hl):
    g, _ = _gen(8, 6, 80)
    np.random.seed(9)
    xb, labels = g.sample(40, as_uint8=True)
    want = xb.cpu().numpy().transpose(1, 0, 3, 4, 2)               # (N,T,H,W,C)
    np.random.seed(9)
    xf, _ = g.sample(40)
    xf = xf.cpu().double().numpy().transpose(1, 0, 3, 4, 2)
    np.random.seed(9)
    chunks = list(g.sample_many(40, chunk=16))
    assert [c.shape for c in chunks] == [(16, 16, 64, 64, 3), (16, 16, 64, 64, 3), (8, 16, 64, 64, 3)] and chunks[0].dtype == np.uint8
    got = np.concatenate(chunks)
    # clip for clip the same video to 1e-6 (rows may fall into other tiles than in the batch of 40): the bytes are those of
    # sample(40) except where a value sits within that error of a byte boundary, and there they are 1 apart at most
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    v = (xf / 2. + 0.5) * 255
    assert d.max() <= 1 and (d[np.abs(v - np.rint(v)) > 127.5 * 4e-6] == 0).all()
    np.random.seed(9)
    whole = list(g.sample_many(40, chunk=40))
    assert len(whole) == 1 and np.abs(whole[0].astype(np.int64) - want.astype(np.int64)).max() <= 1


def test_generate_samples_test_mode_flags(hl, tmp_path):
    """generate_samples.py --test_mode 1 --labels ... --video_len 24 on a snapshot written by save_npz writes grid/, 000/ ... with 24
    frames each (where ffmpeg is absent save_video leaves the frames in place, as test_train_and_generate_entry_points relies on)"""
    import generate_samples
    from mocogan_chainer_amd.trainer import save_npz
    g, _ = _gen(8, 6, 90)
    save_npz(tmp_path / 'gen.npz', g)
    out = tmp_path / 'samples'
    generate_samples.main([str(tmp_path / 'gen.npz'), str(out), '--num', '4', '--dim_zl', '6', '--n_filters', '8', '--test_mode', '1',
                           '--labels', '0,3,5,1', '--video_len', '24', '--seed', '3', '--fix_content'])
    from PIL import Image
    for d in ('grid', '000', '001', '002', '003'):
        frames = sorted((out / d).glob('*.jpg'))
        assert len(frames) == 24, d
    assert Image.open(sorted((out / 'grid').glob('*.jpg'))[0]).size == (128, 128)
    assert Image.open(sorted((out / '002').glob('*.jpg'))[5]).size == (64, 64)
    # the same seed gives the same frames; --fix_motion and bf16 run too
    out2 = tmp_path / 'samples2'
    generate_samples.main([str(tmp_path / 'gen.npz'), str(out2), '--num', '4', '--dim_zl', '6', '--n_filters', '8', '--test_mode', '1',
                           '--labels', '0,3,5,1', '--video_len', '24', '--seed', '3', '--fix_content'])
    a, b = np.asarray(Image.open(out / '001' / '07.jpg')), np.asarray(Image.open(out2 / '001' / '07.jpg'))
    assert np.array_equal(a, b)
    out3 = tmp_path / 'samples3'
    generate_samples.main([str(tmp_path / 'gen.npz'), str(out3), '--num', '4', '--dim_zl', '6', '--n_filters', '8', '--test_mode', '1',
                           '--labels', '2', '--fix_motion', '--mfma', 'bf16'])
    assert len(sorted((out3 / '003').glob('*.jpg'))) == 16
    hl.reset_tuning()                                               # (main() loaded the shipped tile table)


# ------------------------------------------------------------------------------------------------------------
# memory
# ------------------------------------------------------------------------------------------------------------
def test_sample_peak_memory(hl):
    """in one process: sample at 64 clips peaks below the unchanged test-mode __call__ at 64 clips (which keeps every tensor a
    backward pass would read), and sample_many's peak is set by the chunk, not by the number of clips"""
    from model.net import config
    g, _ = _gen(64, 0, 95)
    np.random.seed(1)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    x, _ = g.sample(64, as_uint8=True)
    torch.cuda.synchronize()
    peak_sample = torch.cuda.max_memory_allocated() - base
    del x
    g.impl._sbuf = [None, None, None]                               # (its buffers must not count against __call__)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    prev, config.train = config.train, False
    try:
        xc, _ = g(64)
    finally:
        config.train = prev
    torch.cuda.synchronize()
    peak_call = torch.cuda.max_memory_allocated() - base
    print("peak device memory at 64 clips, n_filters 64: sample %.1f MB, test-mode __call__ %.1f MB" % (peak_sample / 2**20, peak_call / 2**20))
    assert peak_sample < peak_call
    del xc
    g.last_saved = None

    del g
    peaks = []
    for num in (16, 160):                                           # each from the same clean state: a fresh generator, an emptied cache
        gc.collect()
        g2, _ = _gen(16, 0, 96)
        np.random.seed(2)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        count = sum(c.shape[0] for c in g2.sample_many(num, chunk=16))
        assert count == num
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated())
        del g2
        gc.collect()
        torch.cuda.empty_cache()
    print("sample_many peak: %d bytes at 16 clips, %d at 160 (chunk 16)" % tuple(peaks))
    assert peaks[0] == peaks[1]
