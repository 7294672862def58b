"""CPU-only checks of the differentiable augmentation: the entry points are declared, exported and validate their arguments on the
host; the policy parser; the flag and keyword plumbing; the float64 reference of tests/augment_ref.py against torch autograd of an
independent torch statement, and its own adjoint identity; fp32 evaluations of the reference against the bound the GPU tests use;
the ranges and the mask independence of the parameter draw."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import augment_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('mcg_augment_workspace_bytes', 'mcg_augment_draw', 'mcg_augment_fwd', 'mcg_augment_bwd')
UNIT = 2.0 ** -24


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def _ptr(addr):
    return ctypes.c_void_p(addr)       # non-null and never dereferenced: every call below fails before a launch


def test_header_and_library_declare_and_export_the_entry_points(hl):
    header = open(os.path.join(ROOT, 'include', 'mocogan_hip.h')).read()
    lib = hl.load()
    for name in ENTRY_POINTS:
        assert name + '(' in header, name
        assert name in hl.SIGNATURES and getattr(lib, name) is not None, name
    assert 'MCG_AUG_COLOR = 1, MCG_AUG_TRANSLATION = 2, MCG_AUG_CUTOUT = 4' in header
    assert (hl.AUG_COLOR, hl.AUG_TRANSLATION, hl.AUG_CUTOUT) == (1, 2, 4)
    assert '#define MCG_ABI_VERSION 8' in header and lib.mcg_version() == 8 and hl.ABI_VERSION == 8
    assert lib.mcg_augment_workspace_bytes(32) >= 32 * 8 and lib.mcg_augment_workspace_bytes(0) == 0


def test_entry_points_validate_on_the_host(hl):
    lib = hl.load()
    a, g, c, w, o = (_ptr(0x100000 * (i + 1)) for i in range(5))
    for fn in (lib.mcg_augment_fwd, lib.mcg_augment_bwd):
        def call(N=2, C=3, Cp=4, T=2, H=16, W=16, a=a, g=g, c=c, w=w, o=o):
            return fn(N, C, Cp, T, H, W, a, g, c, w, o, None)
        for null in ('a', 'g', 'c', 'w', 'o'):
            assert call(**{null: None}) == -1, null
        for bad in (dict(C=0), dict(C=4), dict(C=-1), dict(N=0), dict(T=0), dict(H=0), dict(W=-16), dict(N=-2)):
            assert call(**bad) == -1, bad
        assert call(Cp=8) == -2 and call(Cp=3) == -2
        assert call(o=a) == -1                                       # a gather cannot run in place
    assert lib.mcg_augment_draw(4, 64, 64, 7, 0, 0, None, c, None) == -1
    assert lib.mcg_augment_draw(4, 64, 64, 7, 0, 0, g, None, None) == -1
    assert lib.mcg_augment_draw(0, 64, 64, 7, 0, 0, g, c, None) == -1
    assert lib.mcg_augment_draw(4, 0, 64, 7, 0, 0, g, c, None) == -1
    assert lib.mcg_augment_draw(4, 64, 64, 8, 0, 0, g, c, None) == -1 and lib.mcg_augment_draw(4, 64, 64, -1, 0, 0, g, c, None) == -1


def test_policy_parsing(hl):
    p = hl.parse_augment
    assert p(None) == 0 and p('') == 0 and p(0) == 0
    assert p('color') == 1 and p('translation') == 2 and p('cutout') == 4
    assert p('color,translation,cutout') == 7 and p(' cutout , color ') == 5 and p('color,color') == 1
    assert p(7) == 7 and p(6) == 6
    for bad in ('colour', 'color,flip', 'color translation', 8, -1, 1.5, True):
        with pytest.raises(ValueError):
            p(bad)


def test_flag_and_keywords():
    import train
    import mocogan_chainer_amd.step as step
    import model.updater as mu
    from model.net import ImageGenerator, ImageDiscriminator, VideoDiscriminator
    from mocogan_chainer_amd import trainer as T
    from datasets import SyntheticDataset
    assert train.parse_args([]).augment == ''
    assert train.parse_args(['--augment', 'color,cutout']).augment == 'color,cutout'
    with pytest.raises(SystemExit):
        train.parse_args(['--augment', 'color,flip'])
    gen, di, dv = step.make_models('normal', n_filters=8, device='cpu', seed=0)
    assert step.TrainStep('normal', gen, di, dv).augment == 0
    assert step.TrainStep('normal', gen, di, dv, augment=None).augment == 0
    assert step.TrainStep('normal', gen, di, dv, augment='color,translation,cutout').augment == 7
    assert step.TrainStep('normal', gen, di, dv, augment=4).augment == 4
    with pytest.raises(ValueError):
        step.TrainStep('normal', gen, di, dv, augment='mirror')

    def updater(**kw):
        np.random.seed(0)
        nets = (ImageGenerator(50, 10, 0, 3, 8, 16, device='cpu'), ImageDiscriminator(3, 1, 8, True, 0.2, device='cpu'),
                VideoDiscriminator(3, 1, 8, True, 0.2, device='cpu'))
        opts = {}
        for k, n in zip(('image_gen', 'image_dis', 'video_dis'), nets):
            opts[k] = T.Adam(alpha=2e-4, beta1=5e-5)
            opts[k].setup(n)
        return mu.Updater(model='normal', models=nets, video_length=16, img_size=64, channel=3, dim_zl=0,
                          iterator=T.SerialIterator(SyntheticDataset(8, 6), 4), tensorboard_writer=T.NullWriter(), optimizer=opts, **kw)
    assert updater()._step.augment == 0
    assert updater(augment='color,cutout')._step.augment == 5
    assert updater(augment=None)._step.augment == 0
    with pytest.raises(ValueError):
        updater(augment='mirror')


# ---- the float64 reference --------------------------------------------------------------------------------------------------
hand_placed = ar.hand_placed


CASES = [(6, 3, 2, 16, 16), (4, 1, 2, 8, 24)]


def torch_forward(x, geo, col):
    """an independent torch statement: subtract-mean / scale / add-mean colour, F.pad translation, a mask for the cutout"""
    n, _, T, H, W = x.shape
    b, s, c = (torch.tensor(np.asarray(col[:, k], np.float64)).view(-1, 1, 1, 1, 1) for k in range(3))
    v = x + b
    mu = v.mean(dim=1, keepdim=True)
    v = (v - mu) * s + mu
    m = v.mean(dim=(1, 2, 3, 4), keepdim=True)
    v = (v - m) * c + m
    outs = []
    for i in range(n):
        dx, dy, x0, x1, y0, y1 = (int(q) for q in geo[i, :6])
        px, py = W // 8, H // 8
        padded = TF.pad(v[i], (px, px, py, py))                          # out(y, x) = padded(y - dy + py, x - dx + px)
        o = padded[:, :, py - dy:py - dy + H, px - dx:px - dx + W]
        mask = torch.ones(H, W, dtype=x.dtype)
        mask[y0:y1, x0:x1] = 0
        outs.append(o * mask)
    return torch.stack(outs)


@pytest.mark.parametrize("n,C,T,H,W", CASES)
def test_reference_against_torch_autograd(n, C, T, H, W):
    rng = np.random.RandomState(7 + C)
    geo, col = hand_placed(n, H, W)
    x = rng.uniform(-1, 1, (n, C, T, H, W))
    g = rng.randn(n, C, T, H, W)
    xt = torch.tensor(x, requires_grad=True)
    out_t = torch_forward(xt, geo, col)
    out_t.backward(torch.tensor(g))
    out = ar.forward(x, geo, col)
    gx = ar.adjoint(g, geo, col)
    assert np.abs(out - out_t.detach().numpy()).max() <= 2e-15 * max(1.0, np.abs(out).max())
    assert np.abs(gx - xt.grad.numpy()).max() <= 2e-15 * max(1.0, np.abs(gx).max())
    # <L u, g> == <u, L^T g> for the linear part L u = A(u) - A(0)
    u = rng.randn(n, C, T, H, W)
    lu = ar.forward(u, geo, col) - ar.forward(np.zeros_like(u), geo, col)
    lhs, rhs = np.sum(lu * g), np.sum(u * ar.adjoint(g, geo, col))
    assert abs(lhs - rhs) <= 1e-14 * np.sum(np.abs(lu * g))
    # identity parameters: the input itself
    gi, ci = ar.identity_params(n)
    assert np.array_equal(ar.forward(x, gi, ci), x) and np.array_equal(ar.forward(x.astype(np.float32), gi, ci, np.float32), x.astype(np.float32))


@pytest.mark.parametrize("n,C,T,H,W", CASES + [(2, 3, 16, 64, 64)])
def test_fp32_evaluation_stays_inside_the_bound_of_the_gpu_tests(n, C, T, H, W):
    """the GPU tests allow 16 units of 2^-24 * max(1, max|ref|): an fp32 NumPy evaluation of the forward and of the adjoint stays
    below 4, which leaves the kernels room for another contraction and summation order"""
    rng = np.random.RandomState(11 + C)
    geo, col = hand_placed(n, H, W)
    x = rng.uniform(-1, 1, (n, C, T, H, W)).astype(np.float32)
    g = rng.randn(n, C, T, H, W).astype(np.float32)
    for fn, a in ((ar.forward, x), (ar.adjoint, g)):
        ref = fn(a, geo, col)
        got = fn(a, geo, col, np.float32)
        assert got.dtype == np.float32
        units = np.abs(got - ref).max() / (UNIT * max(1.0, np.abs(ref).max()))
        assert units < 4.0, (fn.__name__, units)


def test_restated_iteration_with_identity_parameters_is_the_oracle_iteration():
    """pins augment_ref.update_core's composition: with identity parameters it is oracle.updater.update_core"""
    from oracle import net as onet
    from oracle import updater as oupd
    for model, dim_zl in (('normal', 0), ('cgan', 6)):
        rng = np.random.RandomState(5)
        c_d = 3 + (dim_zl if model == 'cgan' else 0)
        nets = [onet.init_generator(rng, dim_zl=dim_zl, n_filters=4), onet.init_discriminator(rng, 2, c_d, 1, 4),
                onet.init_discriminator(rng, 3, c_d, 1, 4)]
        nets = [{k: (v.astype(np.float64) if v.dtype.kind == 'f' else v) for k, v in p.items()} for p in nets]
        x_real, t_real = rng.uniform(-1, 1, (2, 3, 16, 64, 64)), rng.randint(0, 6, 2)
        rnd = oupd.draw_step_randomness(rng, model, 2, 3, 4, dim_zl=dim_zl, dtype=np.float64)
        a, b = copy.deepcopy(nets), copy.deepcopy(nets)
        ref = oupd.update_core(model, *a, *(oupd.new_adam_state(p) for p in a), x_real, t_real, rnd, dim_zl=dim_zl, keep=True)
        rnd['augment'] = {'real': ar.identity_params(2), 'fake': ar.identity_params(2)}
        got = ar.update_core(model, *b, *(oupd.new_adam_state(p) for p in b), x_real, t_real, rnd, dim_zl=dim_zl)
        for k in ('loss_dis_i', 'loss_dis_v', 'loss_gen', 'min_margin'):
            assert got[k] == ref[k], k
        assert np.array_equal(got['gx_fake'], ref['gx_fake']) and np.array_equal(got['x_fake_aug'], ref['x_fake'][:, :3])
        for pa, pb in zip(a, b):
            for k in pa:
                assert np.array_equal(pa[k], pb[k]), k


# ---- the draw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (16, 16), (8, 24)])
def test_drawn_ranges(H, W):
    geo, col = ar.draw(4096, H, W, ar.FULL, 12345, (3 << 32) + 40)
    dx, dy, x0, x1, y0, y1 = (geo[:, k] for k in range(6))
    assert np.abs(dx).max() == W // 8 and np.abs(dy).max() == H // 8             # the bounds are met, and kept
    assert dx.min() == -(W // 8) and dy.min() == -(H // 8)
    assert (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all() and (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all()
    assert (x1 - x0).max() == W // 2 and (y1 - y0).max() == H // 2 and (x1 - x0).min() == W // 4 and (y1 - y0).min() == H // 4
    assert (geo[:, 6:] == 0).all() and (col[:, 3] == 0).all()
    b, s, c = col[:, 0], col[:, 1], col[:, 2]
    assert (-0.5 <= b).all() and (b < 0.5).all() and (0 <= s).all() and (s < 2).all() and (0.5 <= c).all() and (c < 1.5).all()
    assert b.min() < -0.49 and b.max() > 0.49 and s.min() < 0.01 and s.max() > 1.99 and c.min() < 0.51 and c.max() > 1.49


def test_mask_independence_of_the_draw():
    full_g, full_c = ar.draw(257, 64, 64, ar.FULL, 99, 1000)
    ig, ic = ar.identity_params(257)
    for policy in range(8):
        geo, col = ar.draw(257, 64, 64, policy, 99, 1000)
        assert np.array_equal(col, full_c if policy & 1 else ic), policy
        assert np.array_equal(geo[:, :2], (full_g if policy & 2 else ig)[:, :2]), policy
        assert np.array_equal(geo[:, 2:], (full_g if policy & 4 else ig)[:, 2:]), policy
    other_g, other_c = ar.draw(257, 64, 64, ar.FULL, 99, 1001)
    assert not np.array_equal(other_c, full_c) and not np.array_equal(other_g, full_g)
    p = ar.perf_mode_params(5, 2, 3, 4)
    assert np.array_equal(p['real'][1], ar.draw(4, 64, 64, 7, 5, (2 * 64 + 3 + 1) * 64 + 40)[1])
    assert np.array_equal(p['fake'][0], ar.draw(4, 64, 64, 7, 5, (2 * 64 + 3 + 1) * 64 + 41)[0])
