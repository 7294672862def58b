"""The adaptive augmentation on the device: mcg_augment_draw_gated and mcg_ada_update against tests/ada_ref.py inside the poisoned
arena (every comparison is exact: integers, Philox words and double arithmetic that Python restates operation by operation), the
controller inside whole iterations on every schedule (the draws of iteration k + 1 read the p iteration k left), a fixed
probability against the augmented oracle, and the surface (snapshot round trip, train.py's flags)."""
import functools

import numpy as np
import pytest
import torch

import ada_ref
import augment_ref as ar
import guard
import test_gpu_augment as tga
from test_gpu_step import dev

pytestmark = pytest.mark.gpu

FULL = 'color,translation,cutout'
NAN, INF = float('nan'), float('inf')
PROBS = [0.0, 2.0 ** -23, 0.3, 0.5, 1.0 - 2.0 ** -23, 1.0, 1.5]


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


# ---- the gated draw ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (16, 32)])
@pytest.mark.parametrize("n", [1, 5, 255, 256, 257])
def test_gated_draw_bit_for_bit(pkg, arena, n, H, W):
    """the block edges of the 256-thread launch x every policy x probabilities at both ends of u's range (u is a multiple of 2^-23
    below 1: p = 2^-23 passes only u = 0, p = 1 - 2^-23 refuses only the largest u)"""
    hl = pkg[0]
    seed, sid, gsid = 1234567 + n, (7 << 32) + 40, (7 << 32) + 42
    block = [0.0, 3.0, -5.0, 77.0, 2.0, 0.25, -0.5, 9.0]
    for policy in range(1, 8):
        arena.reset()
        plain_geo, plain_col = arena.empty((n, 8), torch.int32), arena.empty((n, 4))
        hl.augment_draw(n, H, W, policy, seed, sid, plain_geo, plain_col)
        for p in PROBS:
            ada = arena.put(torch.tensor([p] + block[1:], dtype=torch.float64, device="cuda"))
            before = bits(ada)
            geo, col = arena.empty((n, 8), torch.int32), arena.empty((n, 4))
            hl.augment_draw_gated(n, H, W, policy, seed, sid, gsid, ada, geo, col)
            arena.check()
            rg, rc, mask = ada_ref.gated_draw(n, H, W, policy, seed, sid, gsid, p)
            assert np.array_equal(geo.cpu().numpy(), rg), (policy, p)
            assert np.array_equal(bits(col), rc.view(np.uint32)), (policy, p)
            assert np.array_equal(bits(ada), before), (policy, p)                     # the draw reads the block, never writes it
            if p >= 1.0:
                assert torch.equal(geo[:, :6], plain_geo[:, :6]) and torch.equal(geo[:, 7], plain_geo[:, 7]), (policy, p)
                assert np.array_equal(bits(col), bits(plain_col)), (policy, p)
                assert bool((geo[:, 6] == policy).all()), (policy, p)
            if p == 0.0:
                ig, ic = ar.identity_params(n)
                assert np.array_equal(geo.cpu().numpy(), ig) and np.array_equal(bits(col), ic.view(np.uint32)), policy


@pytest.mark.parametrize("H,W", [(64, 64), (16, 32)])
@pytest.mark.parametrize("n", [1, 5, 255, 256, 257])
def test_gated_draw_at_p0_leaves_the_clips_untouched(pkg, arena, n, H, W):
    hl = pkg[0]
    arena.reset()
    ada = arena.put(hl.ada_state(0.0, "cuda"))
    geo, col = arena.empty((n, 8), torch.int32), arena.empty((n, 4))
    hl.augment_draw_gated(n, H, W, 7, 5, 40, 42, ada, geo, col)
    g = torch.Generator().manual_seed(n)
    x = torch.rand((n, 1, H, W, 4), generator=g) * 2 - 1
    x[..., 3] = 0.0
    xd = arena.put(x.cuda())
    ws = arena.full((hl.load().mcg_augment_workspace_bytes(n) // 8,), NAN, torch.float64)
    out = arena.empty(tuple(xd.shape))
    hl.augment_fwd(xd, 3, geo, col, ws, out)
    arena.check()
    assert np.array_equal(bits(out), bits(xd))


# ---- the controller ---------------------------------------------------------------------------------------------------------
POS = [1.5, INF, 1e-45, 3e-39, 7.0]                              # (1e-45, 3e-39: fp32 denormals)
NEG = [-2.5, -INF, -1e-45, -3e-39, -0.125]
SPECIAL = [0.0, -0.0, NAN, INF, -INF, 1e-45, -1e-45, 1.0, -2.0]    # the signs of one cycle add up to 0


def logits(kind, N):
    if kind == 'pos':
        v = [POS[k % len(POS)] for k in range(N)]
    elif kind == 'neg':
        v = [NEG[k % len(NEG)] for k in range(N)]
    elif kind == 'balanced':                                     # N // 2 of either sign (and a NaN in the middle of an odd N): sum exactly 0
        v = [POS[k % len(POS)] for k in range(N // 2)] + [NAN] * (N % 2) + [NEG[k % len(NEG)] for k in range(N // 2)]
    else:
        v = [SPECIAL[k % len(SPECIAL)] for k in range(N)]
    return np.asarray(v, np.float32)


# (video, image) logits of call k of an adjustment's interval; r = max(r_v, r_i) lies above the target in UP, below it in the others
UP = [('pos', 'neg'), ('pos', 'special'), ('pos', 'balanced'), ('pos', 'neg')]
DOWN_A = [('neg', 'special'), ('neg', 'balanced'), ('balanced', 'neg'), ('special', 'neg')]
DOWN_B = [('special', 'balanced'), ('neg', 'neg'), ('balanced', 'special'), ('neg', 'special')]
TARGET, STEP = 0.6, 0.75            # up, down, down: 0 -> 0.75 -> 0 -> (-0.75) 0;  0.5 -> (1.25) 1 -> 0.25 -> (-0.5) 0;  1 -> (1.75) 1 -> ...


def _controller_run(hl, arena, N, C, interval, p0):
    arena.reset()
    ada = arena.put(hl.ada_state(p0, "cuda"))
    state, states, clamped = ada_ref.new_state(p0), [], set()
    for phase in (UP, DOWN_A, DOWN_B):
        for k in range(interval):
            yv, yi = (logits(kind, N) for kind in phase[k])
            dv, di = arena.empty((N, C)), arena.empty((N, C))     # columns 1.. stay arena poison (NaN): they must not matter
            dv[:, 0], di[:, 0] = torch.tensor(yv, device="cuda"), torch.tensor(yi, device="cuda")
            hl.ada_update(dv, di, TARGET, STEP, interval, ada)
            before = state
            state = ada_ref.controller(state, yv, yi, TARGET, STEP, interval)
            if state[7] != before[7]:                                 # an adjustment: did it leave [0, 1]?
                if phase is UP and before[0] + STEP > 1.0:
                    clamped.add('hi')
                if phase is not UP and before[0] - STEP < 0.0:
                    clamped.add('lo')
            got = ada.cpu().numpy()
            assert np.array_equal(got.view(np.uint64), np.asarray(state, np.float64).view(np.uint64)), (interval, p0, phase[k], got, state)
            states.append(got)
    arena.check()
    return states, clamped, state


@pytest.mark.parametrize("C", [1, 7])
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1000])
def test_controller_bit_for_bit(pkg, arena, N, C):
    hl = pkg[0]
    for interval in (1, 4):
        hit = set()
        for p0 in (0.0, 0.5, 1.0):
            states, clamped, last = _controller_run(hl, arena, N, C, interval, p0)
            hit |= clamped
            assert len(states) == 3 * interval and last[7] == 3.0 and last[1:5] == [0.0] * 4
            assert last[0] == 0.0 and last[5] < TARGET and last[6] < TARGET
            again = _controller_run(hl, arena, N, C, interval, p0)[0]
            assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(states, again))
        assert hit == {'hi', 'lo'}, (interval, hit)


def test_controller_at_the_target_moves_nothing(pkg, arena):
    hl = pkg[0]
    arena.reset()
    ada = arena.put(hl.ada_state(0.25, "cuda"))
    yv, yi = arena.put(torch.tensor([[1.0], [2.0], [3.0], [-1.0]], device="cuda")), arena.put(torch.full((4, 1), -1.0, device="cuda"))
    hl.ada_update(yv, yi, 0.5, 0.125, 1, ada)
    arena.check()
    assert ada.tolist() == [0.25, 0.0, 0.0, 0.0, 0.0, 0.5, -1.0, 1.0]


def test_argument_errors_on_the_device(pkg):
    hl = pkg[0]
    lib, P = hl.load(), hl._p
    n = 3
    geo, col = torch.zeros((n, 8), dtype=torch.int32, device="cuda"), torch.zeros((n, 4), device="cuda")
    ada, y = hl.ada_state(0.5, "cuda"), torch.ones((n, 1), device="cuda")
    pa, pg, pc, py = P(ada, torch.float64), P(geo, torch.int32), P(col), P(y)
    assert lib.mcg_augment_draw_gated(n, 64, 64, 7, 1, 40, 42, pa, pg, pc, None) == 0
    assert lib.mcg_augment_draw_gated(n, 64, 64, 7, 1, 40, 40, pa, pg, pc, None) == -1
    assert lib.mcg_augment_draw_gated(n, 64, 64, 7, 1, 40, 42, None, pg, pc, None) == -1
    assert lib.mcg_ada_update(n, 1, py, py, 0.6, 0.0, 1, pa, None) == 0
    assert lib.mcg_ada_update(n, 1, py, py, 1.0, 0.1, 1, pa, None) == -1
    assert lib.mcg_ada_update(n, 1, py, py, 0.6, -0.1, 1, pa, None) == -1
    torch.cuda.synchronize()
    assert ada.tolist() == [0.5, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0]                  # (step 0: r = 1 recorded, p stays)


# ---- whole iterations -------------------------------------------------------------------------------------------------------
def _nets(pkg, nf=4):
    return tga._nets(pkg, 'normal', 0, nf)


def _clips(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, 3, 16, 64, 64), generator=g) * 2 - 1).cuda()


ADAPTIVE = dict(n=4, interval=2, kimg=0.032, iterations=6, p0=0.5, seed=31)


def _adaptive_run(pkg, **kw):
    """six iterations with interval 2 and step 0.25 (target 0.1: no mean of four signs equals it, every adjustment moves p); after each, the reference controller replayed on the logits run() returned
    must be what ada_stats() reads, and the parameters run() drew must be the gated draw at the p the iteration before left"""
    hl, lay, nets, step = pkg
    c = ADAPTIVE
    n = c['n']
    assert ada_ref.step_size(c['interval'], n, c['kimg']) == 0.25
    ts = step.TrainStep('normal', *_nets(pkg), seed=c['seed'], augment=FULL, augment_p=c['p0'],
                        ada={'target': 0.1, 'interval': c['interval'], 'kimg': c['kimg']}, **kw)
    x = _clips(n)
    state, ps = ada_ref.new_state(c['p0']), []
    for it in range(c['iterations']):
        out = ts.run(x, None)
        ref, masks = ada_ref.perf_mode_params(c['seed'], it, 0, n, state[0])
        for k in ('real', 'fake'):
            assert np.array_equal(out['augment'][k][0].cpu().numpy(), ref[k][0]), (it, k, state[0])
            assert np.array_equal(bits(out['augment'][k][1]), ref[k][1].view(np.uint32)), (it, k, state[0])
        state = ada_ref.controller(state, out['y_real_v'].cpu().numpy(), out['y_real_i'].cpu().numpy(), 0.1, 0.25, c['interval'])
        assert ts.ada_stats() == ada_ref.stats(state), (it, ts.ada_stats(), state)
        assert np.array_equal(ts.ada_state(), np.asarray(state)), it
        ps.append(state[0])
    assert state[7] == 3.0 and len(set(ps)) > 1, ps                                   # p visibly moved
    assert all(np.isfinite(v) for v in ts.losses().values())
    return ps


def test_adaptive_step(pkg):
    _adaptive_run(pkg)


def test_adaptive_step_with_side_streams(pkg):
    _adaptive_run(pkg, overlap=True)


@pytest.mark.parametrize("early", [False, True])
def test_adaptive_step_with_the_two_chain_schedule(pkg, monkeypatch, early):
    """early: the real chain -- it draws the real clips' parameters -- waits for events only and may run an iteration ahead of the
    main stream: the event behind the controller's launch is what keeps its gates behind the p of the iteration before"""
    step = pkg[3]
    monkeypatch.setattr(step, 'CHAINS_MIN_N', 1)
    before = step.chain_iterations
    _adaptive_run(pkg, overlap=True, input_ready_early=early)
    assert step.chain_iterations - before == ADAPTIVE['iterations'], "the two-chain schedule did not run"


# Seeds searched on the CPU with the augmented oracle fed the gated parameters (augment_ref.Case with ada_ref.perf_mode_params at
# p = 0.5, as the header of the step tests in tests/test_gpu_augment.py describes): both iterations keep every pre-activation more than
# TIGHT_MARGIN from its kink, and over the two iterations' real and generated clips every component both passes and fails its gate.
FIXED_P, FIXED_DATA_SEED, FIXED_PERF_SEED = 0.5, 1303, 258         # (margins 4.6e-6, 2.7e-6)


def test_fixed_probability_against_the_oracle(pkg, monkeypatch):
    """test_gpu_augment._run_case -- its comparisons, its tolerances, its assertion of min_margin > TIGHT_MARGIN in every iteration
    -- with the oracle fed ada_ref's gated parameters and the step built with augment_p = 0.5; the draw is compared bit for bit
    there, geo[:, 6] (the mask) included"""
    step = pkg[3]
    masks = []

    def gated(seed, it, rank, n, policy=ar.FULL, H=64, W=64):
        par, m = ada_ref.perf_mode_params(seed, it, rank, n, FIXED_P, policy, H, W)
        masks.append(np.concatenate([m['real'], m['fake']]))
        return par
    monkeypatch.setattr(ar, 'perf_mode_params', gated)
    monkeypatch.setattr(step, 'TrainStep', functools.partial(step.TrainStep, augment_p=FIXED_P))
    ts = tga._run_case(pkg, "normal", 0, FIXED_DATA_SEED, steps=2, perf=(FIXED_PERF_SEED, 0))
    assert ts.ada_stats() == {'p': FIXED_P, 'rt_video': 0.0, 'rt_image': 0.0, 'adjustments': 0}      # no controller: the block stays
    assert len(masks) == 2
    seen = np.concatenate(masks)
    for flag in ada_ref.COMPONENTS:
        assert ((seen & flag) != 0).any() and ((seen & flag) == 0).any(), (flag, seen)


def test_p0_and_p1_through_the_step(pkg):
    hl, lay, nets, step = pkg
    n, seed = 2, 77
    x = _clips(n, 5)
    packed = torch.empty((n, 16, 64, 64, 4), device="cuda")
    hl.pack_clip(n, 3, 4, 16, 64 * 64, x, packed)
    runs = {}
    for name, kw in (('plain', {}), ('p0', {'augment_p': 0.0}), ('p1', {'augment_p': 1.0})):
        torch.manual_seed(0)
        ts = step.TrainStep('normal', *_nets(pkg), seed=seed, augment=FULL, **kw)
        runs[name] = ts.run(x, None)
        torch.cuda.synchronize()
    assert np.array_equal(bits(runs['p0']['x_real_aug']), bits(packed))
    assert torch.equal(runs['p0']['x_fake_aug'], runs['p0']['x_fake'])
    assert np.array_equal(bits(runs['p1']['x_real_aug']), bits(runs['plain']['x_real_aug']))
    for k in ('real', 'fake'):
        assert torch.equal(runs['p1']['augment'][k][0][:, :6], runs['plain']['augment'][k][0][:, :6])
        assert bool((runs['p1']['augment'][k][0][:, 6] == 7).all()) and not bool(runs['p0']['augment'][k][0].any())


def test_parity_mode_uses_the_callers_parameters_and_still_updates(pkg):
    hl, lay, nets, step = pkg
    case = ar.Case('normal', 0, 4, 2, tga.SEED_NORMAL)
    before, x_real, t_real, rnd, _ = case.next()
    devnets = _nets(pkg)
    tga._load(devnets, before)
    ts = step.TrainStep('normal', *devnets, augment=FULL, augment_p=0.0, ada={'interval': 1, 'kimg': 0.016})
    inject = tga._inject(lay, rnd)
    out = ts.run(dev(x_real), dev(t_real, torch.int32), inject)
    for k in ('real', 'fake'):                                       # p = 0 would have drawn the identity: the caller's are used as they are
        assert out['augment'][k][0] is inject['augment'][k][0] and out['augment'][k][1] is inject['augment'][k][1]
    state = ada_ref.controller(ada_ref.new_state(0.0), out['y_real_v'].cpu().numpy(), out['y_real_i'].cpu().numpy(), 0.6,
                               ada_ref.step_size(1, 2, 0.016), 1)
    assert ts.ada_stats() == ada_ref.stats(state) and state[7] == 1.0


def test_options_off_change_nothing(pkg):
    hl, lay, nets, step = pkg
    ts = step.TrainStep('normal', *_nets(pkg), augment=FULL)
    assert ts.ada is None and ts.ada_state() is None and ts._ev_ada is None
    with pytest.raises(ValueError):
        ts.ada_stats()
    out = ts.run(_clips(2), None)
    assert ts._ev_ada is None and not bool(out['augment']['real'][0][:, 6].any())     # the plain draw: geo[6] = 0


# ---- surface ----------------------------------------------------------------------------------------------------------------
def _train_args(name, *more):
    return ['--dataset_type', 'synthetic', '--synthetic_size', '8', '--batchsize', '4', '--n_filters_gen', '8', '--snapshot_interval', '1',
            '--log_tensorboard_interval', '100', '--num_gen_samples', '4', '--save_name', name, '--augment', 'color,cutout',
            '--augment_p', '0.5', '--ada_target', '0.1', '--ada_interval', '1', '--ada_kimg', '0.032'] + list(more)


def test_train_entry_point_snapshot_and_resume(pkg, tmp_path, monkeypatch):
    """train.py with the four flags (batch 4, interval 1, kimg 0.032: steps of 0.125); the state block goes into the snapshot as
    updater/ada/state and comes back on --resume, after which the run continues from it"""
    import train
    monkeypatch.chdir(tmp_path)
    try:
        tr = train.main(_train_args('ada', '--max_epoch', '1'))
        st = tr.updater._step
        assert tr.updater.iteration == 2 and st.augment == 5 and st.ada == {'target': 0.1, 'interval': 1, 'kimg': 0.032}
        saved = st.ada_state()
        assert saved[7] == 2.0 and saved[0] in (0.25, 0.5, 0.75)
        for key, v in (('augment/p', saved[0]), ('video_dis/rt', saved[5]), ('image_dis/rt', saved[6])):
            assert tr.updater.observation[key] == v, key
        snap = tmp_path / 'result' / 'ada' / 'snapshot_epoch_1.npz'
        assert np.array_equal(np.load(snap)['updater/ada/state'], saved)
        tr2 = train.main(_train_args('ada2', '--max_epoch', '2', '--resume', str(snap)))
        st2 = tr2.updater._step.ada_state()
        assert tr2.updater.iteration == 4 and st2[7] == 4.0                         # two more adjustments on top of the restored two
        assert abs(st2[0] - saved[0]) in (0.0, 0.125, 0.25) and all(np.isfinite(v) for v in tr2.updater._step.losses().values())
        # a snapshot without the key loads as before: p starts where the flags put it
        plain = dict(np.load(snap))
        del plain['updater/ada/state']
        np.savez(tmp_path / 'plain.npz', **plain)
        tr3 = train.main(_train_args('ada3', '--max_epoch', '1', '--resume', str(tmp_path / 'plain.npz')))
        assert tr3.updater._step.ada_state()[7] == 0.0 and tr3.updater._step.ada_state()[0] == 0.5
    finally:
        pkg[0].reset_tuning()                                            # (main() switched the tile tuner on with the shipped table)


def test_state_round_trip_through_the_step(pkg):
    hl, lay, nets, step = pkg
    ts = step.TrainStep('normal', *_nets(pkg), augment=FULL, ada=True)
    block = np.array([0.375, 5.0, -3.0, 12.0, 3.0, 0.25, -0.5, 17.0])
    ts.load_ada_state(block)
    assert np.array_equal(ts.ada_state(), block)
    assert ts.ada_stats() == {'p': 0.375, 'rt_video': 0.25, 'rt_image': -0.5, 'adjustments': 17}
    with pytest.raises(ValueError):
        ts.load_ada_state(block[:7])
