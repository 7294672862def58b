"""The adaptive augmentation without a GPU: properties of its NumPy statement (tests/ada_ref.py: the gate, the controller), the
host-side refusals of mcg_augment_draw_gated / mcg_ada_update (the pattern of tests/test_cabi_cpu.py: a never-dereferenced pointer,
outputs untouched), and the argument errors of TrainStep, Updater and train.py's flags."""
import ctypes
import math

import numpy as np
import pytest

import ada_ref
import augment_ref as ar

FULL, NAMES = ar.FULL, 'color,translation,cutout'
NAN, INF = float('nan'), float('inf')


# ---- the gate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(64, 64), (16, 32)])
@pytest.mark.parametrize("policy", range(1, 8))
def test_p0_is_the_identity_and_p1_the_plain_draw(policy, H, W):
    n, seed, sid, gsid = 300, 99, (3 << 32) + 40, (3 << 32) + 42
    geo, col, mask = ada_ref.gated_draw(n, H, W, policy, seed, sid, gsid, 0.0)
    ig, ic = ar.identity_params(n)
    assert np.array_equal(geo, ig) and np.array_equal(col.view(np.uint32), ic.view(np.uint32)) and not mask.any()
    for p in (1.0, 1.5):
        geo, col, mask = ada_ref.gated_draw(n, H, W, policy, seed, sid, gsid, p)
        rg, rc = ar.draw(n, H, W, policy, seed, sid)
        assert np.array_equal(geo[:, :6], rg[:, :6]) and np.array_equal(col.view(np.uint32), rc.view(np.uint32))
        assert np.all(mask == policy) and np.all(geo[:, 6] == policy) and not geo[:, 7].any()
    # the largest u is 1 - 2^-23: p = 1 - 2^-23 is the first probability that can refuse, p = 2^-23 the first that can pass
    u = ada_ref.gate_units(n, seed, gsid)
    assert u.max() <= 1.0 - 2.0 ** -23 and u.min() >= 0.0


@pytest.mark.parametrize("policy", range(1, 8))
def test_a_component_outside_the_policy_is_never_set(policy):
    for p in (0.3, 0.7, 1.0):
        geo, col, mask = ada_ref.gated_draw(1000, 64, 64, policy, 5, 40, 42, p)
        assert not (mask & ~policy).any()
        assert np.array_equal(geo[:, 6], mask)
        ig, ic = ar.identity_params(1000)
        off_c, off_t, off_o = ((mask & f) == 0 for f in ada_ref.COMPONENTS)
        assert np.array_equal(col[off_c], ic[off_c]) and not geo[off_t, 0:2].any() and not geo[off_o, 2:6].any()
        # ... and a component that passed carries exactly the plain draw's values (its words are not shifted by the gates)
        rg, rc = ar.draw(1000, 64, 64, policy, 5, 40)
        assert np.array_equal(col[~off_c], rc[~off_c]) and np.array_equal(geo[~off_t, 0:2], rg[~off_t, 0:2])
        assert np.array_equal(geo[~off_o, 2:6], rg[~off_o, 2:6])


def test_pass_rates_and_independence_of_the_gates():
    """n = 2^16 clips at p = 0.3: a pass rate is a binomial mean with sigma sqrt(p (1 - p) / n) = 0.00179, held to 5 sigma = 0.009;
    the sample covariance of two independent gates has sigma p (1 - p) / sqrt(n) = 0.00082, held to 5 of those (0.0041 < 0.009).
    Fixed seed: the figures are printed."""
    n, p = 1 << 16, 0.3
    bound = 5.0 * math.sqrt(p * (1.0 - p) / n)
    assert abs(bound - 0.009) < 1e-4
    _, _, mask = ada_ref.gated_draw(n, 64, 64, FULL, 2024, 40, 42, p)
    bits = [((mask & f) != 0).astype(np.float64) for f in ada_ref.COMPONENTS]
    for k, b in enumerate(bits):
        print("component %d: pass rate %.5f" % (k, b.mean()))
        assert abs(b.mean() - p) <= bound, (k, b.mean())
    cov_bound = 5.0 * p * (1.0 - p) / math.sqrt(n)
    assert cov_bound <= bound
    for a, b in ((0, 1), (0, 2), (1, 2)):
        cov = float((bits[a] * bits[b]).mean() - bits[a].mean() * bits[b].mean())
        print("gates %d, %d: covariance %.5f" % (a, b, cov))
        assert abs(cov) <= cov_bound, (a, b, cov)


def test_gated_perf_mode_params_use_the_documented_stream_ids():
    seed, it, rank, n, p = 11, 3, 2, 9, 0.5
    base = (it * 64 + rank + 1) * 64
    par, masks = ada_ref.perf_mode_params(seed, it, rank, n, p)
    for which, sid in (('real', 40), ('fake', 41)):
        geo, col, mask = ada_ref.gated_draw(n, 64, 64, FULL, seed, base + sid, base + sid + 2, p)
        assert np.array_equal(par[which][0], geo) and np.array_equal(par[which][1], col) and np.array_equal(masks[which], mask)
    full, _ = ada_ref.perf_mode_params(seed, it, rank, n, 1.0)
    plain = ar.perf_mode_params(seed, it, rank, n)
    for which in ('real', 'fake'):
        assert np.array_equal(full[which][0][:, :6], plain[which][0][:, :6]) and np.array_equal(full[which][1], plain[which][1])


# ---- the controller ---------------------------------------------------------------------------------------------------------
def test_sign_of_special_values():
    assert [ada_ref.sign(v) for v in (0.0, -0.0, NAN, INF, -INF, 1e-45, -1e-45, 3.0, -2.0)] == [0, 0, 0, 1, -1, 1, -1, 1, -1]
    st = ada_ref.controller(ada_ref.new_state(0.5), [NAN, 0.0, -0.0, INF], [-INF, NAN, -0.0, 0.0], 0.6, 0.125, 1)
    assert st == [0.375, 0.0, 0.0, 0.0, 0.0, 0.25, -0.25, 1.0]          # r = 0.25 < 0.6: p goes down


def test_clamps_at_zero_and_one():
    up, down = [1.0, 2.0, 3.0], [-1.0, -2.0, -3.0]
    st = ada_ref.new_state(0.5)
    for want in (0.9, 1.0, 1.0):
        st = ada_ref.controller(st, up, down, 0.6, 0.4, 1)              # r = max(1, -1) = 1 > target
        assert st[0] == want
    for want in (0.6, 0.19999999999999996, 0.0, 0.0):
        st = ada_ref.controller(st, down, down, 0.6, 0.4, 1)            # r = -1 < target
        assert st[0] == want
    assert st[7] == 7.0 and st[5] == -1.0 and st[6] == -1.0


def test_r_equal_to_the_target_moves_nothing():
    st = ada_ref.controller(ada_ref.new_state(0.25), [1.0, 2.0, 3.0, -1.0], [-1.0] * 4, 0.5, 0.125, 1)
    assert st == [0.25, 0.0, 0.0, 0.0, 0.0, 0.5, -1.0, 1.0]             # three of four positive: r_v = 0.5 = target


@pytest.mark.parametrize("interval", [1, 4])
def test_interval(interval):
    st = ada_ref.new_state(0.0)
    yv, yi = [1.0, -1.0, 1.0], [1.0, 1.0, 1.0]
    for call in range(1, 2 * interval + 1):
        st = ada_ref.controller(st, yv, yi, 0.6, 0.125, interval)
        if call % interval == 0:
            assert st == [0.125 * (call // interval), 0.0, 0.0, 0.0, 0.0, 1.0 / 3.0, 1.0, float(call // interval)]
        else:
            k = call % interval
            assert st[:5] == [0.125 * (call // interval), 1.0 * k, 3.0 * k, 3.0 * k, float(k)] and st[7] == call // interval
    # a state left with more calls than a (smaller) interval asks for adjusts at the next call
    st = ada_ref.controller([0.5, 2.0, 2.0, 4.0, 5.0, 0.0, 0.0, 0.0], [1.0], [1.0], 0.0, 0.25, 2)
    assert st == [0.75, 0.0, 0.0, 0.0, 0.0, 0.6, 0.6, 1.0]


def test_only_column_zero_is_read():
    y = np.full((5, 7), NAN, np.float32)
    y[:, 0] = [1, -1, 1, 1, 0]
    a = ada_ref.controller(ada_ref.new_state(0.5), y, y, 0.6, 0.1, 1)
    b = ada_ref.controller(ada_ref.new_state(0.5), y[:, 0], y[:, :1], 0.6, 0.1, 1)
    assert a == b and a[5] == 0.4


# ---- host-side refusals of the two entry points -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def test_entry_points_refuse_on_the_host(hl):
    """`one` is a non-null pointer that is never dereferenced; the outputs are small host buffers that must come back untouched;
    no call below passes an acceptable argument set."""
    lib = hl.load()
    one = ctypes.c_void_p(16)
    BAD = -1
    bufs = [(ctypes.c_double * 8)(*([3.0] * 8)) for _ in range(3)]
    geo, col, ada = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    calls = []

    def refused(rc, *what):
        calls.append(what)
        assert rc == BAD, (what, rc)
        assert all(list(b) == [3.0] * 8 for b in bufs), what

    def draw(N=4, H=64, W=64, policy=7, sid=40, gsid=42, a=one, g=geo, c=col):
        return lib.mcg_augment_draw_gated(N, H, W, policy, 1, sid, gsid, a, g, c, None)

    for bad in (dict(N=0), dict(N=-3), dict(H=0), dict(W=0), dict(H=-64), dict(policy=-1), dict(policy=8), dict(a=None), dict(g=None),
                dict(c=None), dict(gsid=40), dict(sid=(5 << 32) + 1, gsid=(5 << 32) + 1)):
        refused(draw(**bad), "mcg_augment_draw_gated", bad)
    # (what mcg_augment_draw refuses, it refuses too)
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(policy=8), dict(g=None), dict(c=None)):
        kw = dict(dict(N=4, H=64, W=64, policy=7, g=geo, c=col), **bad)
        assert lib.mcg_augment_draw(kw['N'], kw['H'], kw['W'], kw['policy'], 1, 40, kw['g'], kw['c'], None) == BAD, bad

    def update(N=4, C=1, yv=one, yi=one, target=0.6, step=0.01, interval=4, a=ada):
        return lib.mcg_ada_update(N, C, yv, yi, target, step, interval, a, None)

    for bad in (dict(N=0), dict(N=-1), dict(C=0), dict(C=-7), dict(interval=0), dict(interval=-4), dict(yv=None), dict(yi=None),
                dict(step=-1e-9), dict(step=NAN), dict(step=-INF), dict(target=NAN), dict(target=1.0), dict(target=-1.0),
                dict(target=1.5), dict(target=INF), dict(target=-INF)):
        refused(update(**bad), "mcg_ada_update", bad)
    assert lib.mcg_ada_update(4, 1, one, one, 0.6, 0.01, 4, None, None) == BAD
    assert len(calls) == 29


def test_wrappers_check_the_state_block(hl):
    import torch
    geo, col = torch.zeros((2, 8), dtype=torch.int32), torch.zeros((2, 4))
    with pytest.raises(hl.McgError):
        hl.augment_draw_gated(2, 64, 64, 7, 1, 40, 42, torch.zeros(8, dtype=torch.float32), geo, col)       # not doubles
    with pytest.raises(hl.McgError):
        hl.augment_draw_gated(2, 64, 64, 7, 1, 40, 42, torch.zeros(7, dtype=torch.float64), geo, col)       # too short
    with pytest.raises(hl.McgError):
        hl.augment_draw_gated(2, 64, 64, 7, 1, 40, 42, torch.zeros(8, dtype=torch.float64), geo, col)       # a host tensor
    with pytest.raises(hl.McgError):
        hl.ada_update(torch.zeros((2, 1)), torch.zeros((3, 1)), 0.6, 0.01, 4, torch.zeros(8, dtype=torch.float64))
    for p in (-0.1, 1.1, NAN):
        with pytest.raises(ValueError):
            hl.ada_state(p, 'cpu')
    assert hl.ada_state(0.25, 'cpu').tolist() == [0.25] + [0.0] * 7 and hl.ADA_DOUBLES == 8
    assert (hl.ADA_P, hl.ADA_RT_V, hl.ADA_RT_I, hl.ADA_ADJUSTMENTS) == (ada_ref.ADA_P, ada_ref.ADA_RT_V, ada_ref.ADA_RT_I,
                                                                        ada_ref.ADA_ADJUSTMENTS)


# ---- TrainStep / Updater / train.py -----------------------------------------------------------------------------------------
class _Exchange:
    def __init__(self, active):
        self.active = active


def test_train_step_argument_errors():
    """the options are checked before the networks are touched: None stands for them here"""
    import mocogan_chainer_amd.step as step
    for kw in (dict(augment_p=0.5), dict(ada=True), dict(augment='', ada=True), dict(augment=0, augment_p=0.5),
               dict(augment=FULL, augment_p=0.5, exchange=_Exchange(True)), dict(augment=FULL, ada=True, exchange=_Exchange(True)),
               dict(augment=FULL, augment_p=-0.01), dict(augment=FULL, augment_p=1.01), dict(augment=FULL, augment_p=NAN),
               dict(augment=FULL, ada={'target': 1.0}), dict(augment=FULL, ada={'target': NAN}), dict(augment=FULL, ada={'interval': 0}),
               dict(augment=FULL, ada={'interval': 2.5}), dict(augment=FULL, ada={'kimg': 0}), dict(augment=FULL, ada={'kimg': INF}),
               dict(augment=FULL, ada={'speed': 3}), dict(augment=FULL, ada='yes')):
        with pytest.raises(ValueError):
            step.TrainStep('normal', None, None, None, **kw)
    assert step.check_augment_gate(None, None, None) == (None, None)
    assert step.check_augment_gate(FULL, None, None, _Exchange(True)) == (None, None)
    assert step.check_augment_gate('cutout', 0.25, None) == (0.25, None)
    assert step.check_augment_gate(FULL, None, True, _Exchange(False)) == (0.0, {'target': 0.6, 'interval': 4, 'kimg': 500.0})
    assert step.check_augment_gate(5, 1, {'interval': 2, 'kimg': 0.5}) == (1.0, {'target': 0.6, 'interval': 2, 'kimg': 0.5})
    assert step.TrainStep.AUG_GATE_REAL == 42 and step.TrainStep.AUG_GATE_FAKE == 43 and step.TrainStep.STREAMS_PER_RANK > 43
    assert ada_ref.step_size(2, 4, 0.032) == 0.25


def test_updater_argument_errors():
    from model.updater import Updater
    base = dict(model='normal', models=(None, None, None), video_length=16, img_size=64, channel=3, dim_zl=6, tensorboard_writer=None,
                iterator=None, optimizer={})
    for kw in (dict(augment_p=0.5), dict(ada=True), dict(augment=FULL, augment_p=2.0), dict(augment=FULL, ada={'target': -1.0}),
               dict(augment=FULL, ada=True, exchange=_Exchange(True))):
        with pytest.raises(ValueError):
            Updater(**dict(base, **kw))
    with pytest.raises(TypeError):
        Updater(**dict(base, augment=FULL, ada_p=0.5))


def test_command_line_flags():
    import train
    a = train.parse_args([])
    assert (a.augment_p, a.ada_target, a.ada_interval, a.ada_kimg) == (None, None, 4, 500.0) and train.ada_option(a) is None
    assert (a.batchsize, a.max_epoch, a.dim_zc, a.dim_zm, a.n_filters_gen, a.augment) == (100, 1000, 50, 10, 64, '')    # the reference's
    a = train.parse_args(['--augment', 'color,cutout', '--augment_p', '0.5'])
    assert a.augment_p == 0.5 and train.ada_option(a) is None
    a = train.parse_args(['--augment', NAMES, '--ada_target', '0.6'])
    assert a.augment_p is None and train.ada_option(a) == {'target': 0.6, 'interval': 4, 'kimg': 500.0}
    a = train.parse_args(['--augment', NAMES, '--augment_p', '0.2', '--ada_target', '0.5', '--ada_interval', '2', '--ada_kimg', '100'])
    assert a.augment_p == 0.2 and train.ada_option(a) == {'target': 0.5, 'interval': 2, 'kimg': 100.0}
    for argv in (['--augment_p', '0.5'], ['--ada_target', '0.6'], ['--augment', NAMES, '--augment_p', '1.5'],
                 ['--augment', NAMES, '--ada_target', '1'], ['--augment', NAMES, '--ada_target', '0.6', '--ada_interval', '0'],
                 ['--augment', NAMES, '--ada_target', '0.6', '--ada_kimg', '0'], ['--augment', NAMES, '--ada_target', 'nan']):
        with pytest.raises(SystemExit):
            train.parse_args(argv)
