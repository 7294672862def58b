"""The differentiable augmentation on the device: mcg_augment_fwd / mcg_augment_bwd / mcg_augment_draw against the float64
statement of tests/augment_ref.py (op level, inside a poisoned arena), and whole iterations with the augmentation in front of both
discriminators against the augmented oracle (step level, teacher-forced like tests/test_gpu_step.py, same tolerances)."""
import numpy as np
import pytest
import torch

import augment_ref as ar
import guard
from test_gpu_step import TIGHT_MARGIN, check_params, dev, draw_to_dev, is_pre_bn_bias, noise_to_dev, rel_l2

pytestmark = pytest.mark.gpu

F64 = np.float64
UNIT = 2.0 ** -24
FULL = 'color,translation,cutout'


@pytest.fixture(scope="module")
def pkg():
    assert torch.cuda.is_available()
    import mocogan_chainer_amd.hiplib as hl
    import mocogan_chainer_amd.layout as lay
    import mocogan_chainer_amd.nets as nets
    import mocogan_chainer_amd.step as step
    hl.load()
    return hl, lay, nets, step


@pytest.fixture(scope="module")
def arena():
    return guard.Arena()


def params_to_dev(geo, col, arena=None):
    g, c = torch.tensor(geo, dtype=torch.int32, device="cuda"), torch.tensor(col, dtype=torch.float32, device="cuda")
    return (arena.put(g), arena.put(c)) if arena is not None else (g, c)


def clip_to_dev(lay, arena, a, pad_value=0.0):
    """(N,C,T,H,W) -> the device layout inside the arena; pad_value fills the pad channel (a gradient's may hold anything)"""
    t = lay.act_to_dev(dev(a))
    if pad_value:
        t[..., a.shape[1]:] = pad_value
    return arena.put(t)


def both_passes(hl, lay, arena, x, g, geo, col, g_pad=0.0):
    n, C = x.shape[:2]
    gd, cd = params_to_dev(geo, col, arena)
    ws = arena.full((hl.load().mcg_augment_workspace_bytes(n) // 8,), float('nan'), torch.float64)
    xd, gdev = clip_to_dev(lay, arena, x), clip_to_dev(lay, arena, g, g_pad)
    out, gx = arena.empty(tuple(xd.shape)), arena.empty(tuple(xd.shape))
    hl.augment_fwd(xd, C, gd, cd, ws, out)
    hl.augment_bwd(gdev, C, gd, cd, ws, gx)
    arena.check()
    return out, gx


def check_against(got, ref, C, what):
    pad = got[..., C:]
    assert pad.numel() and float(pad.abs().max()) == 0.0 and not bool(torch.signbit(pad).any()), what     # exactly 0.0
    g = got[..., :C].permute(0, 4, 1, 2, 3).double().cpu().numpy()
    units = np.abs(g - ref).max() / (UNIT * max(1.0, np.abs(ref).max()))
    print("%s: %.2f units of 2^-24 max(1, max|ref|)" % (what, units))
    assert units <= 16.0, (what, units)


# ---- op level ---------------------------------------------------------------------------------------------------------------
CASES = [(6, 3, 2, 16, 16), (4, 1, 2, 8, 24)]


@pytest.mark.parametrize("n,C,T,H,W", CASES)
def test_forward_and_backward_against_float64(pkg, arena, n, C, T, H, W):
    """hand-placed parameters that hit every edge (augment_ref.hand_placed); clip 0 / row 0 and the last row of the last clip sit at
    the arena's margins, so a tap outside a clip reads poison.  A wrong tap, sign of a shift or mean moves elements by > 1e-2."""
    hl, lay = pkg[:2]
    arena.reset()
    rng = np.random.RandomState(7 + C)
    geo, col = ar.hand_placed(n, H, W)
    x, g = rng.uniform(-1, 1, (n, C, T, H, W)), rng.randn(n, C, T, H, W)
    out, gx = both_passes(hl, lay, arena, x, g, geo, col, g_pad=3.25)        # (the gradient's pad channel is ignored)
    check_against(out, ar.forward(x, geo, col), C, "forward")
    check_against(gx, ar.adjoint(g, geo, col), C, "backward")


@pytest.mark.parametrize("n,C,T,H,W", CASES)
def test_adjoint_on_the_device(pkg, arena, n, C, T, H, W):
    """<A(u) - A(0), g> == <u, bwd(g)>, both accumulated in float64 from the device's results"""
    hl, lay = pkg[:2]
    arena.reset()
    rng = np.random.RandomState(17 + C)
    geo, col = ar.hand_placed(n, H, W)
    u, g = rng.randn(n, C, T, H, W), rng.randn(n, C, T, H, W)
    a_u, gx = both_passes(hl, lay, arena, u, g, geo, col)
    a_0, _ = both_passes(hl, lay, arena, np.zeros_like(u), g, geo, col)
    ud, gd = lay.act_to_dev(dev(u)).double(), lay.act_to_dev(dev(g)).double()
    terms = (a_u.double() - a_0.double()) * gd
    lhs, rhs = float(terms.sum()), float((ud * gx.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * float(terms.abs().sum()), (lhs, rhs)


@pytest.mark.parametrize("n,C,T,H,W", CASES)
def test_identity_parameters_return_the_input_bit_for_bit(pkg, arena, n, C, T, H, W):
    hl, lay = pkg[:2]
    arena.reset()
    rng = np.random.RandomState(27 + C)
    x, g = rng.uniform(-1, 1, (n, C, T, H, W)), rng.randn(n, C, T, H, W)
    out, gx = both_passes(hl, lay, arena, x, g, *ar.identity_params(n), g_pad=-1.5)
    assert torch.equal(out, lay.act_to_dev(dev(x))) and torch.equal(gx, lay.act_to_dev(dev(g)))
    # ... and a brightness alone leaves the pad channel exactly zero
    geo, col = ar.identity_params(n)
    col[:, 0] = 0.5
    out, gx = both_passes(hl, lay, arena, x, g, geo, col, g_pad=-1.5)
    assert float(out[..., C:].abs().max()) == 0.0 and float(gx[..., C:].abs().max()) == 0.0
    assert torch.equal(out[..., :C], (lay.act_to_dev(dev(x)) + 0.5)[..., :C])


@pytest.mark.parametrize("n", [1, 5, 257])
def test_draw_bit_for_bit(pkg, arena, n):
    hl = pkg[0]
    for H, W, seed, sid in ((64, 64, 1234567, (7 << 32) + 40), (8, 24, 3, 41)):
        for policy in range(8):
            arena.reset()
            geo, col = arena.empty((n, 8), torch.int32), arena.empty((n, 4))
            hl.augment_draw(n, H, W, policy, seed, sid, geo, col)
            arena.check()
            rg, rc = ar.draw(n, H, W, policy, seed, sid)
            assert np.array_equal(geo.cpu().numpy(), rg), (H, W, policy)
            assert np.array_equal(col.cpu().numpy().view(np.uint32), rc.view(np.uint32)), (H, W, policy)


def test_full_clips_and_run_to_run_bit_identity(pkg, arena):
    """production extents (several partial-sum blocks per clip), drawn parameters; two runs on the same inputs are bit-identical"""
    hl, lay = pkg[:2]
    arena.reset()
    n, C, T, H, W = 4, 3, 16, 64, 64
    rng = np.random.RandomState(41)
    geo, col = ar.draw(n, H, W, 7, 2024, 40)
    x = rng.uniform(-1, 1, (n, C, T, H, W)) + 0.75           # (a clip mean far from zero: the contrast term carries it)
    g = rng.randn(n, C, T, H, W) + 0.5
    out, gx = both_passes(hl, lay, arena, x, g, geo, col)
    check_against(out, ar.forward(x, geo, col), C, "forward")
    check_against(gx, ar.adjoint(g, geo, col), C, "backward")
    out1, gx1 = out.clone(), gx.clone()
    arena.reset()
    out2, gx2 = both_passes(hl, lay, arena, x, g, geo, col)
    assert torch.equal(out1, out2) and torch.equal(gx1, gx2)


def test_argument_errors(pkg):
    hl = pkg[0]
    lib = hl.load()
    n, T, H, W = 2, 2, 16, 16
    x, o = torch.zeros((n, T, H, W, 4), device="cuda"), torch.zeros((n, T, H, W, 4), device="cuda")
    geo, col = params_to_dev(*ar.identity_params(n))
    ws = hl.augment_workspace(n, "cuda")
    P = hl._p
    for fn in (lib.mcg_augment_fwd, lib.mcg_augment_bwd):
        def call(N=n, C=3, Cp=4, T=T, H=H, W=W, x=P(x), geo=P(geo, torch.int32), col=P(col), ws=P(ws, torch.float64), o=P(o)):
            return fn(N, C, Cp, T, H, W, x, geo, col, ws, o, None)
        assert call() == 0
        for null in ('x', 'geo', 'col', 'ws', 'o'):
            assert call(**{null: None}) == -1, null
        for bad in (dict(C=0), dict(C=4), dict(N=0), dict(T=0), dict(H=-1), dict(W=0)):
            assert call(**bad) == -1, bad
        assert call(Cp=8) == -2
        assert call(o=P(x)) == -1
    torch.cuda.synchronize()
    with pytest.raises(hl.McgError):
        hl.augment_fwd(x, 3, geo[:1], col, ws, o)                       # fewer parameter sets than clips
    with pytest.raises(hl.McgError):
        hl.augment_fwd(x, 3, geo, col, ws[:1], o)


# ---- step level -------------------------------------------------------------------------------------------------------------
# Seeds searched on the CPU with the augmented oracle (augment_ref.Case): every compared iteration keeps every pre-activation more
# than TIGHT_MARGIN away from its kink (margins 4.6e-6; 4.3e-6; 2.7e-6, 3.3e-6; 4.3e-6, 3.6e-6), so every gradient and update is
# held to the tight tolerances -- asserted below, no loose fallback.
SEED_NORMAL, SEED_CGAN = 502, 501
DATA_SEED_PERF, PERF_SEED = 1303, {0: 70, 3: 74}


def _nets(pkg, model, dim_zl, nf=4):
    nets = pkg[2]
    c_d = 3 + (dim_zl if model == 'cgan' else 0)
    return nets.GenNet(dim_zl=dim_zl, n_filters=nf), nets.DisNet(2, c_d, 1, nf, use_noise=True), nets.DisNet(3, c_d, 1, nf, use_noise=True)


def _load(devnets, before):
    for net, p, st in zip(devnets, *before):
        net.load_reference_params(p)
        net.load_adam_state(st)


def _inject(lay, rnd):
    inject = {'t': rnd['t'], 'gen': draw_to_dev(rnd['gen']), 'augment': {k: params_to_dev(*v) for k, v in rnd['augment'].items()}}
    for k in ('noise_i_real', 'noise_v_real', 'noise_i_fake', 'noise_v_fake'):
        inject[k] = noise_to_dev(lay, rnd[k])
    return inject


def _run_case(pkg, model, dim_zl, seed, steps, perf=None, overlap=False):
    hl, lay, nets, step = pkg
    case = ar.Case(model, dim_zl, 4, 2, seed, perf=perf)
    G, DI, DV = devnets = _nets(pkg, model, dim_zl)
    ts = step.TrainStep(model, G, DI, DV, overlap=overlap, augment=FULL, **({'seed': perf[0], 'rank': perf[1]} if perf else {}))
    for s in range(steps):
        before, x_real, t_real, rnd, ref = case.next()
        _load(devnets, before)
        assert ref['min_margin'] > TIGHT_MARGIN, "seed no longer yields a well-conditioned iteration"
        out = ts.run(dev(x_real), dev(t_real, torch.int32), None if perf else _inject(lay, rnd))
        losses = ts.losses()
        if perf:
            assert out['t'] == rnd['t']
            for k in ('real', 'fake'):                                   # the in-kernel draw on ids base + 40 / 41, bit for bit
                assert np.array_equal(out['augment'][k][0].cpu().numpy(), rnd['augment'][k][0]), (s, k)
                assert np.array_equal(out['augment'][k][1].cpu().numpy(), rnd['augment'][k][1]), (s, k)
        assert abs(losses['image_dis/loss'] - ref['loss_dis_i']) < 1e-5, s
        assert abs(losses['video_dis/loss'] - ref['loss_dis_v']) < 1e-5, s
        assert abs(losses['image_gen/loss'] - ref['loss_gen']) < 1e-5, s
        for k in ('x_fake', 'x_fake_aug', 'x_real_aug'):
            assert rel_l2(lay.act_from_dev(out[k], 3), ref[k]) < 1e-5, (s, k)
            assert float(out[k][..., 3].abs().max()) == 0.0, (s, k)
        for k in ('y_real_i', 'y_real_v', 'y_fake_i', 'y_fake_v'):
            assert rel_l2(out[k], ref[k].reshape(out[k].shape)) < 2e-5, (s, k)
        assert rel_l2(lay.act_from_dev(out['gx_aug'], 3), ref['gx_aug']) < 1e-4, s
        assert rel_l2(lay.act_from_dev(out['gx_fake'], 3), ref['gx_fake']) < 1e-4, s
        for name, net, kind, refg in (('D_I', DI, 'dis', ref['grads_dis_i']), ('D_V', DV, 'dis', ref['grads_dis_v']),
                                      ('G', G, 'gen', ref['grads_gen'])):
            got = net.export_reference_grads()
            for k in refg:
                if not is_pre_bn_bias(k, kind):
                    tiny = refg[k].size <= 8 and np.abs(np.asarray(got[k], F64) - refg[k]).max() < 5e-7     # (test_gpu_step._run_steps)
                    assert tiny or rel_l2(got[k], refg[k]) < 1e-4, (s, name, k)
        gen, di, dv = case.nets
        check_params(DI.export_reference_params(), di, 'dis', 1e-4, 'D_I step %d' % s, ref['grads_dis_i'])
        check_params(DV.export_reference_params(), dv, 'dis', 1e-4, 'D_V step %d' % s, ref['grads_dis_v'])
        check_params(G.export_reference_params(), gen, 'gen', 1e-4, 'G step %d' % s, ref['grads_gen'])
    return ts


@pytest.mark.parametrize("model,dim_zl,seed", [("normal", 0, SEED_NORMAL), ("cgan", 6, SEED_CGAN)])
def test_injected_iteration(pkg, model, dim_zl, seed):
    _run_case(pkg, model, dim_zl, seed, steps=1)


@pytest.mark.parametrize("rank", [0, 3])
def test_perf_mode_two_iterations(pkg, rank):
    _run_case(pkg, "normal", 0, DATA_SEED_PERF, steps=2, perf=(PERF_SEED[rank], rank))


def test_with_side_streams(pkg):
    _run_case(pkg, "normal", 0, SEED_NORMAL, steps=1, overlap=True)


def test_with_the_two_chain_schedule(pkg, monkeypatch):
    step = pkg[3]
    monkeypatch.setattr(step, 'CHAINS_MIN_N', 1)
    before = step.chain_iterations
    _run_case(pkg, "normal", 0, SEED_NORMAL, steps=1, overlap=True)
    assert step.chain_iterations - before == 1, "the two-chain schedule did not run"


def test_missing_parameters_in_parity_mode_are_refused(pkg):
    hl, lay, nets, step = pkg
    G, DI, DV = _nets(pkg, 'normal', 0)
    ts = step.TrainStep('normal', G, DI, DV, augment=FULL)
    with pytest.raises(ValueError):
        ts.run(torch.zeros((2, 3, 16, 64, 64), device="cuda"), None, {'t': 0})


def test_identity_policy_matches_the_plain_step(pkg):
    """augmentation on with identity parameters injected: the plain TrainStep's iteration from the same state (weight gradients use
    float atomics, so not bit for bit)"""
    hl, lay, nets, step = pkg
    case = ar.Case('normal', 0, 4, 2, SEED_NORMAL)
    before, x_real, t_real, rnd, _ = case.next()
    results = []
    for augment in (None, FULL):
        devnets = _nets(pkg, 'normal', 0)
        _load(devnets, before)
        ts = step.TrainStep('normal', *devnets, augment=augment)
        rnd['augment'] = {'real': ar.identity_params(2), 'fake': ar.identity_params(2)}
        inject = _inject(lay, rnd)
        if augment is None:
            del inject['augment']
        out = ts.run(dev(x_real), dev(t_real, torch.int32), inject)
        torch.cuda.synchronize()
        results.append((out, [net.export_reference_params() for net in devnets]))
    (plain, p_plain), (aug, p_aug) = results
    assert 'x_fake_aug' not in plain and 'augment' not in plain
    assert torch.equal(aug['x_fake_aug'], aug['x_fake']) and torch.equal(aug['gx_aug'], aug['gx_fake'])
    for k in ('y_real_i', 'y_real_v', 'y_fake_i', 'y_fake_v', 'x_fake'):
        assert rel_l2(aug[k], plain[k].cpu().numpy()) < 1e-6, k
    # (check_params: rel-L2 per tensor; the biases in front of a BatchNorm -- true gradient zero, so Adam steps on rounding noise --
    #  and the running means that absorb them are held to its absolute bound, as everywhere in test_gpu_step.py)
    for a, b, kind in zip(p_aug, p_plain, ('gen', 'dis', 'dis')):
        check_params(a, b, kind, 1e-5, 'identity policy, ' + kind)


# ---- surface ----------------------------------------------------------------------------------------------------------------
def test_updater_runs_with_the_option(pkg):
    from model.net import ImageGenerator, ImageDiscriminator, VideoDiscriminator
    from model.updater import Updater
    from datasets import SyntheticDataset
    from mocogan_chainer_amd import trainer as T
    np.random.seed(0)
    g, di, dv = ImageGenerator(dim_zl=6, n_filters=8), ImageDiscriminator(3, 1, 8, True, 0.2), VideoDiscriminator(3, 1, 8, True, 0.2)
    opts = {}
    for name, link in (('image_gen', g), ('image_dis', di), ('video_dis', dv)):
        o = T.Adam(alpha=2e-4, beta1=5e-5)
        o.setup(link)
        o.add_hook(T.WeightDecay(1e-5), 'hook_dec')
        opts[name] = o
    u = Updater(model='normal', models=(g, di, dv), video_length=16, img_size=64, channel=3, dim_zl=6, tensorboard_writer=T.NullWriter(),
                iterator=T.SerialIterator(SyntheticDataset(8, 6), 4), optimizer=opts, device=0, augment=FULL)
    for _ in range(2):
        u.update()
        assert all(np.isfinite(v) for v in u._step.losses().values())
    assert u._step.augment == 7 and u.iteration == 2


def test_train_entry_point_with_the_flag(pkg, tmp_path, monkeypatch):
    import train
    monkeypatch.chdir(tmp_path)
    try:
        tr = train.main(['--dataset_type', 'synthetic', '--synthetic_size', '8', '--batchsize', '4', '--max_epoch', '1', '--n_filters_gen', '8',
                         '--snapshot_interval', '1', '--log_tensorboard_interval', '100', '--num_gen_samples', '4', '--save_name', 'aug',
                         '--augment', 'color,cutout'])
        assert tr.updater.iteration == 2 and tr.updater._step.augment == 5
        assert all(np.isfinite(v) for v in tr.updater._step.losses().values())
    finally:
        pkg[0].reset_tuning()                                            # (main() switched the tile tuner on with the shipped table)
