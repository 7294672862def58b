"""The geometric augmentation on the device: mcg_warp_fwd / mcg_warp_bwd / mcg_warp_draw / mcg_warp_draw_gated against the NumPy
statement of tests/warp_ref.py (op level, every operand inside the poisoned arena), and whole iterations with the warp and the
colour / translation / cutout augmentation in front of both discriminators against the oracle (step level: the runner, the
tolerances and the conditioning rule are those of tests/test_gpu_augment.py, used as they stand)."""
import functools

import numpy as np
import pytest
import torch

import augment_ref as ar
import guard
import test_gpu_augment as tga
import warp_ref as wr
from test_gpu_step import check_params, dev, rel_l2

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -24
FULL = 'flip,rot90,scale,rotate'
AUG_FULL = 'color,translation,cutout'


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


def bits(t):
    return t.cpu().numpy().view(np.uint32 if t.element_size() == 4 else np.uint64)


def mat_to_dev(mat, arena=None):
    m = torch.tensor(np.asarray(mat, np.float32), device="cuda")
    return arena.put(m) if arena is not None else m


def clip_to_dev(lay, arena, a, pad_value=0.0):
    t = lay.act_to_dev(dev(a))
    if pad_value:
        t[..., a.shape[1]:] = pad_value
    return arena.put(t)


def both_passes(hl, lay, arena, x, g, mat, pad=0.0):
    """warp_fwd on x and warp_bwd on g with the same matrices, every operand and result in the arena; the arena is checked"""
    C = x.shape[1]
    md = mat_to_dev(mat, arena)
    xd, gd = clip_to_dev(lay, arena, x, pad), clip_to_dev(lay, arena, g, pad)
    out, gx = arena.empty(tuple(xd.shape)), arena.empty(tuple(xd.shape))
    hl.warp_fwd(xd, C, md, out)
    hl.warp_bwd(gd, C, md, gx)
    arena.check()
    return xd, gd, out, gx


def check_against(got, ref, mag, C, what):
    """|got - ref| <= 16 * 2^-24 * S per element, S = the reference's sum of |w| |value| over that element's terms, floored at
    2^-24 max|ref|.  Derived, not measured: the coordinates agree bit for bit, so a term differs by the roundings of 1 - f, of the
    product of the two weights and of the multiply-add (three or four half-units of its size), and the bound grows with the
    number of terms a gradient element collects because S does.  The pad channel is exactly +0.0."""
    pad = got[..., C:]
    assert pad.numel() and float(pad.abs().max()) == 0.0 and not bool(torch.signbit(pad).any()), what
    g = got[..., :C].permute(0, 4, 1, 2, 3).double().cpu().numpy()
    assert np.isfinite(g).all(), what
    S = np.maximum(mag, UNIT * np.abs(ref).max())
    err = np.abs(g - ref)
    units = float(np.divide(err, UNIT * S, out=np.zeros_like(err), where=S > 0).max())
    print("%s: %.2f units of 2^-24 S" % (what, units))
    assert (err <= 16.0 * UNIT * S).all(), (what, units, float(err.max()))        # (S == 0, an all-zero reference: exactly zero)


# ---- forward and backward against float64 -------------------------------------------------------------------------------------
CASES = [(7, 3, 2, 8, 8), (5, 1, 2, 6, 10)]


@pytest.mark.parametrize("n,C,T,H,W", CASES)
def test_forward_and_backward_against_float64(pkg, arena, n, C, T, H, W):
    """every hand-placed matrix (warp_ref.hand_placed_sets), n at a time; clip 0 and the last clip sit at the arena's margins, so a
    tap outside a clip reads poison and a store outside it is caught.  The offset that moves every source outside the frame, the
    all-zero matrix (every output reads the centre taps, the backward box is the whole frame) and the 1e6 scale are the cases
    where a kernel can go wrong with nothing but indexing."""
    hl, lay = pkg[:2]
    rng = np.random.RandomState(7 + C)
    for first in range(0, wr.N_HAND_PLACED, n):
        arena.reset()
        mat = wr.hand_placed(n, H, W, first)
        x, g = rng.uniform(-1, 1, (n, C, T, H, W)), rng.randn(n, C, T, H, W)
        _, _, out, gx = both_passes(hl, lay, arena, x, g, mat)
        check_against(out, *wr.forward(x, mat, with_terms=True), C, "forward, sets from %d" % first)
        check_against(gx, *wr.adjoint(g, mat, with_terms=True), C, "backward, sets from %d" % first)
        for i in range(n):
            if (first + i) % wr.N_HAND_PLACED in (11, 13):               # all sources outside: output and gradient all zero
                assert not bool(out[i].any()) and not bool(gx[i].any()), (first, i)


@pytest.mark.parametrize("n,C,T,H,W", CASES)
def test_exact_cases_bit_for_bit(pkg, arena, n, C, T, H, W):
    """identity: input and gradient come back bit for bit (all four lanes: the pad lane is warped like the others); a flip, and on
    square frames the quarter turns, are torch.flip / torch.rot90 of the input, and their backward the inverse permutation"""
    hl, lay = pkg[:2]
    arena.reset()
    rng = np.random.RandomState(27 + C)
    x, g = rng.uniform(-1, 1, (n, C, T, H, W)), rng.randn(n, C, T, H, W)
    xd, gd, out, gx = both_passes(hl, lay, arena, x, g, wr.identity_mats(n), pad=-1.5)
    assert np.array_equal(bits(out), bits(xd)) and np.array_equal(bits(gx), bits(gd))
    arena.reset()
    mat = wr.hand_placed(n, H, W)                                        # identity, flip, Q_1, Q_2, Q_3, ...
    xd, gd, out, gx = both_passes(hl, lay, arena, x, g, mat, pad=0.75)
    assert np.array_equal(bits(out[1]), bits(torch.flip(xd[1], dims=(2,)))) and np.array_equal(bits(gx[1]), bits(torch.flip(gd[1], dims=(2,))))
    if H == W:
        # the sense of Q_1 from the statement itself (tests/test_warp_cpu.py holds it to np.rot90)
        probe = np.arange(16.0).reshape(1, 1, 1, 4, 4)
        sense = 1 if np.array_equal(wr.forward(probe, wr.hand_placed(1, 4, 4, first=2)), np.rot90(probe, 1, axes=(-2, -1))) else -1
        for k in (1, 2, 3):
            assert np.array_equal(bits(out[1 + k]), bits(torch.rot90(xd[1 + k], sense * k, dims=(1, 2)))), k
            assert np.array_equal(bits(gx[1 + k]), bits(torch.rot90(gd[1 + k], -sense * k, dims=(1, 2)))), k


@pytest.mark.parametrize("n,C,T,H,W", CASES)
def test_adjoint_on_the_device(pkg, arena, n, C, T, H, W):
    """<A u, g> == <u, A^T g>, both accumulated in float64 from the device's results (the map is linear: no A(0) to take off)"""
    hl, lay = pkg[:2]
    rng = np.random.RandomState(17 + C)
    for first in range(0, wr.N_HAND_PLACED, n):
        arena.reset()
        u, g = rng.randn(n, C, T, H, W), rng.randn(n, C, T, H, W)
        ud, gd, a_u, gx = both_passes(hl, lay, arena, u, g, wr.hand_placed(n, H, W, first))
        terms = a_u.double() * gd.double()
        lhs, rhs = float(terms.sum()), float((ud.double() * gx.double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * float(terms.abs().sum()), (first, lhs, rhs)


# ---- the draws ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 257])
def test_draw_bit_for_bit(pkg, arena, n):
    hl = pkg[0]
    lib = hl.load()
    for H, W, seed, sid in ((64, 64, 1234567, (7 << 32) + 44), (8, 24, 3, 45)):
        for policy in range(16):
            arena.reset()
            mat = arena.empty((n, 8))
            if H != W and policy & wr.WARP_ROT90:                        # refused, and nothing is written
                assert lib.mcg_warp_draw(n, H, W, policy, seed, sid, hl._p(mat), None) == -2
                torch.cuda.synchronize()
                assert bool((mat.view(torch.int32) == guard.POISON).all()), policy
                continue
            hl.warp_draw(n, H, W, policy, seed, sid, mat)
            arena.check()
            assert np.array_equal(bits(mat), wr.draw(n, H, W, policy, seed, sid).view(np.uint32)), (H, W, policy)


PROBS = [0.0, 2.0 ** -23, 0.5, 1.0 - 2.0 ** -23, 1.0]


@pytest.mark.parametrize("n", [1, 5, 257])
def test_gated_draw_bit_for_bit(pkg, arena, n):
    hl = pkg[0]
    lib = hl.load()
    seed, sid, gsid = 7654321 + n, (7 << 32) + 44, (7 << 32) + 46
    block = [0.0, 3.0, -5.0, 77.0, 2.0, 0.25, -0.5, 9.0]
    for H, W in ((64, 64), (8, 24)):
        for policy in range(16):
            arena.reset()
            if H != W and policy & wr.WARP_ROT90:
                ada, mat = arena.put(hl.ada_state(0.5, "cuda")), arena.empty((n, 8))
                assert lib.mcg_warp_draw_gated(n, H, W, policy, seed, sid, gsid, hl._p(ada, torch.float64), hl._p(mat), None) == -2
                torch.cuda.synchronize()
                assert bool((mat.view(torch.int32) == guard.POISON).all()), policy
                continue
            plain = arena.empty((n, 8))
            hl.warp_draw(n, H, W, policy, seed, sid, plain)
            for p in PROBS:
                ada = arena.put(torch.tensor([p] + block[1:], dtype=torch.float64, device="cuda"))
                before = bits(ada)
                mat = arena.empty((n, 8))
                hl.warp_draw_gated(n, H, W, policy, seed, sid, gsid, ada, mat)
                arena.check()
                ref, mask = wr.draw_gated(n, H, W, policy, seed, sid, gsid, p)
                assert np.array_equal(bits(mat), ref.view(np.uint32)), (H, W, policy, p)
                assert np.array_equal(mat[:, 6].cpu().numpy(), mask.astype(np.float32)) and not bool(mat[:, 7].any()), (policy, p)
                assert np.array_equal(bits(ada), before), (policy, p)    # the draw reads the block, never writes it
                if p >= 1.0:
                    assert np.array_equal(bits(mat[:, :6]), bits(plain[:, :6])) and bool((mat[:, 6] == policy).all()), (policy, p)
                if p == 0.0:
                    assert np.array_equal(bits(mat), wr.identity_mats(n).view(np.uint32)), policy


# ---- production extents -------------------------------------------------------------------------------------------------------
def test_full_clips_and_run_to_run_bit_identity(pkg, arena):
    hl, lay = pkg[:2]
    arena.reset()
    n, C, T, H, W = 4, 3, 16, 64, 64
    rng = np.random.RandomState(41)
    mat = wr.draw(n, H, W, 15, 2024, 44)
    x, g = rng.uniform(-1, 1, (n, C, T, H, W)) + 0.75, rng.randn(n, C, T, H, W) + 0.5
    _, _, out, gx = both_passes(hl, lay, arena, x, g, mat)
    check_against(out, *wr.forward(x, mat, with_terms=True), C, "forward")
    check_against(gx, *wr.adjoint(g, mat, with_terms=True), C, "backward")
    out1, gx1 = out.clone(), gx.clone()
    arena.reset()
    _, _, out2, gx2 = both_passes(hl, lay, arena, x, g, mat)
    assert np.array_equal(bits(out1), bits(out2)) and np.array_equal(bits(gx1), bits(gx2))


# ---- argument errors ----------------------------------------------------------------------------------------------------------
def test_argument_errors(pkg, arena):
    """every refusal of the header, with device pointers; the outputs (poison inside the arena) are untouched afterwards"""
    hl = pkg[0]
    lib, P = hl.load(), hl._p
    arena.reset()
    n, T, H, W = 2, 2, 8, 8
    x, o = arena.zeros((n, T, H, W, 4)), arena.empty((n, T, H, W, 4))
    mat, ada = mat_to_dev(wr.identity_mats(n), arena), arena.put(hl.ada_state(0.5, "cuda"))
    for fn in (lib.mcg_warp_fwd, lib.mcg_warp_bwd):
        def call(N=n, C=3, Cp=4, T=T, H=H, W=W, x=P(x), mat=P(mat), o=P(o)):
            return fn(N, C, Cp, T, H, W, x, mat, o, None)
        for null in ('x', 'mat', 'o'):
            assert call(**{null: None}) == -1, null
        for bad in (dict(C=0), dict(C=5), dict(N=0), dict(T=0), dict(H=-1), dict(W=0), dict(o=P(x))):
            assert call(**bad) == -1, bad
        for bad in (dict(Cp=8), dict(N=65536), dict(T=1 << 12, H=1 << 9, W=1 << 8)):
            assert call(**bad) == -2, bad
    dmat = arena.empty((n, 8))

    def draw(N=n, H=64, W=64, policy=15, m=P(dmat)):
        return lib.mcg_warp_draw(N, H, W, policy, 1, 44, m, None)

    def gated(N=n, H=64, W=64, policy=15, sid=44, gsid=46, a=P(ada, torch.float64), m=P(dmat)):
        return lib.mcg_warp_draw_gated(N, H, W, policy, 1, sid, gsid, a, m, None)

    for bad in (dict(N=0), dict(H=0), dict(W=-1), dict(policy=-1), dict(policy=16), dict(m=None)):
        assert draw(**bad) == -1 and gated(**bad) == -1, bad
    for bad in (dict(a=None), dict(gsid=44)):
        assert gated(**bad) == -1, bad
    assert draw(H=8, W=24, policy=2) == -2 and gated(H=8, W=24, policy=15) == -2
    arena.check()
    assert bool((o.view(torch.int32) == guard.POISON).all()) and bool((dmat.view(torch.int32) == guard.POISON).all())
    assert ada.tolist() == [0.5] + [0.0] * 7
    assert call() == 0 and draw() == 0 and gated() == 0                  # ... and the acceptable calls run
    arena.check()
    with pytest.raises(hl.McgError):
        hl.warp_fwd(x, 3, mat[:1], o)                                    # fewer matrices than clips


# ---- step level ---------------------------------------------------------------------------------------------------------------
# Seeds searched on the CPU with the oracle behind both stages (warp_ref.Case): every compared iteration keeps every pre-activation
# more than TIGHT_MARGIN away from its kink, which tests/test_gpu_augment.py's runner asserts (margins 2.8e-6; 4.5e-6; 4.0e-6,
# 2.5e-6; 3.3e-6, 5.1e-6 -- and at GATED_SEED the gates both pass and fail over the two iterations' clips).
SEED_NORMAL, SEED_CGAN = 570, 514
DATA_SEED_PERF, PERF_SEED, GATED_SEED = 1303, 607, 619
FIXED_P = 0.5


def _run(pkg, monkeypatch, model, dim_zl, seed, steps, perf=None, overlap=False, p=None):
    """tests/test_gpu_augment.py's _run_case -- its comparisons, its tolerances, its assertion of min_margin > TIGHT_MARGIN -- with
    the oracle of warp_ref.Case (warp, then augmentation, then the networks) and the step built with warp = FULL (and augment_p);
    parity mode gets inject['warp'].  Returns the step and what every run() returned."""
    step = pkg[3]
    outs = []
    monkeypatch.setattr(ar, 'Case', functools.partial(wr.Case, p=p))
    plain_inject = tga._inject

    def inject(lay, rnd):
        d = plain_inject(lay, rnd)
        d['warp'] = {k: mat_to_dev(v) for k, v in rnd['warp'].items()}
        return d
    monkeypatch.setattr(tga, '_inject', inject)
    plain_run = step.TrainStep.run

    def run(self, *a, **kw):
        outs.append(plain_run(self, *a, **kw))
        return outs[-1]
    monkeypatch.setattr(step.TrainStep, 'run', run)
    monkeypatch.setattr(step, 'TrainStep', functools.partial(step.TrainStep, warp=FULL, **({} if p is None else {'augment_p': p})))
    ts = tga._run_case(pkg, model, dim_zl, seed, steps, perf=perf, overlap=overlap)
    assert len(outs) == steps and ts.warp == 15 and ts.augment == 7
    return ts, outs


@pytest.mark.parametrize("model,dim_zl,which", [("normal", 0, 'normal'), ("cgan", 6, 'cgan')])
def test_injected_iteration(pkg, monkeypatch, model, dim_zl, which):
    seed = {'normal': SEED_NORMAL, 'cgan': SEED_CGAN}[which]
    _, outs = _run(pkg, monkeypatch, model, dim_zl, seed, steps=1)
    assert set(outs[0]['warp']) == {'real', 'fake'} and outs[0]['x_real_aug'].shape == outs[0]['x_fake_aug'].shape


def test_perf_mode_two_iterations(pkg, monkeypatch):
    _, outs = _run(pkg, monkeypatch, "normal", 0, DATA_SEED_PERF, steps=2, perf=(PERF_SEED, 0))
    for it, out in enumerate(outs):                                      # the in-kernel draw on ids base + 44 / 45, bit for bit
        ref = wr.perf_mode_mats(PERF_SEED, it, 0, 2)
        for k in ('real', 'fake'):
            assert np.array_equal(bits(out['warp'][k]), ref[k].view(np.uint32)), (it, k)


def test_with_side_streams(pkg, monkeypatch):
    _run(pkg, monkeypatch, "normal", 0, SEED_NORMAL, steps=1, overlap=True)


def test_fixed_probability_against_the_gated_reference(pkg, monkeypatch):
    ts, outs = _run(pkg, monkeypatch, "normal", 0, DATA_SEED_PERF, steps=2, perf=(GATED_SEED, 0), p=FIXED_P)
    assert ts.ada_stats() == {'p': FIXED_P, 'rt_video': 0.0, 'rt_image': 0.0, 'adjustments': 0}
    seen = []
    for it, out in enumerate(outs):
        ref = wr.perf_mode_mats(GATED_SEED, it, 0, 2, p=FIXED_P)
        for k in ('real', 'fake'):
            assert np.array_equal(bits(out['warp'][k]), ref[k].view(np.uint32)), (it, k)
            seen += ref[k][:, 6].astype(int).tolist()
    assert len(set(seen)) > 1, seen                                      # the gates did something


def test_missing_matrices_in_parity_mode_are_refused(pkg):
    hl, lay, nets, step = pkg
    ts = step.TrainStep('normal', *tga._nets(pkg, 'normal', 0), warp=FULL)
    with pytest.raises(ValueError, match="inject\\['warp'\\]"):
        ts.run(torch.zeros((2, 3, 16, 64, 64), device="cuda"), None, {'t': 0})


def test_warp_off_is_the_plain_step(pkg):
    """warp=None: the step of before -- x_fake bit for bit, no new key in the result, parameters within the un-augmented step's
    tolerance (weight gradients use float atomics, so not bit for bit); and the warp on with identity matrices injected gives the
    same iteration"""
    hl, lay, nets, step = pkg
    case = ar.Case('normal', 0, 4, 2, tga.SEED_NORMAL)
    before, x_real, t_real, rnd, _ = case.next()
    results = []
    for kw in ({}, {'warp': None}, {'warp': FULL}):
        devnets = tga._nets(pkg, 'normal', 0)
        tga._load(devnets, before)
        ts = step.TrainStep('normal', *devnets, **kw)
        inject = tga._inject(lay, rnd)
        del inject['augment']
        if kw.get('warp'):
            inject['warp'] = {k: mat_to_dev(wr.identity_mats(2)) for k in ('real', 'fake')}
        out = ts.run(dev(x_real), dev(t_real, torch.int32), inject)
        torch.cuda.synchronize()
        results.append((out, [net.export_reference_params() for net in devnets]))
    (plain, p_plain), (off, p_off), (ident, p_ident) = results
    assert set(off) == set(plain) and 'warp' not in off and 'x_fake_aug' not in off
    assert np.array_equal(bits(off['x_fake']), bits(plain['x_fake']))
    assert np.array_equal(bits(ident['x_fake']), bits(plain['x_fake'])) and np.array_equal(bits(ident['x_fake_aug']), bits(ident['x_fake']))
    assert np.array_equal(bits(ident['gx_aug']), bits(ident['gx_fake'])) and 'augment' not in ident
    for k in ('y_real_i', 'y_real_v', 'y_fake_i', 'y_fake_v'):
        assert rel_l2(off[k], plain[k].cpu().numpy()) < 1e-6 and rel_l2(ident[k], plain[k].cpu().numpy()) < 1e-6, k
    for params, what in ((p_off, 'warp=None'), (p_ident, 'identity matrices')):
        for a, b, kind in zip(params, p_plain, ('gen', 'dis', 'dis')):
            check_params(a, b, kind, 1e-5, what + ', ' + kind)


# ---- surface ------------------------------------------------------------------------------------------------------------------
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
                iterator=T.SerialIterator(SyntheticDataset(8, 6), 4), optimizer=opts, device=0, warp=FULL)
    for _ in range(2):
        u.update()
        assert all(np.isfinite(v) for v in u._step.losses().values())
    assert u._step.warp == 15 and u._step.augment == 0 and u.iteration == 2


def test_train_entry_point_with_the_flag(pkg, tmp_path, monkeypatch):
    import train
    monkeypatch.chdir(tmp_path)
    try:
        tr = train.main(['--dataset_type', 'synthetic', '--synthetic_size', '8', '--batchsize', '4', '--max_epoch', '1', '--n_filters_gen', '8',
                         '--snapshot_interval', '1', '--log_tensorboard_interval', '100', '--num_gen_samples', '4', '--save_name', 'warp',
                         '--warp', 'flip,scale', '--augment_p', '0.5'])
        st = tr.updater._step
        assert tr.updater.iteration == 2 and st.warp == 5 and st.augment == 0
        assert all(np.isfinite(v) for v in st.losses().values())
        assert st.ada_stats()['p'] == 0.5
    finally:
        pkg[0].reset_tuning()                                            # (main() switched the tile tuner on with the shipped table)
