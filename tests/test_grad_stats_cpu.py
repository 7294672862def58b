"""CPU-only checks of the gradient statistics / clipping feature: the C ABI's new symbols and refusals, the optimizer hook, which
launches step.adam_update makes with the options absent and present, train.py's flags, and the NumPy statement the GPU tests
compare with (tests/grad_stats_ref.py)."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import grad_stats_ref as gref
from oracle import updater as oupd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -1


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


# ---- symbols and refusals --------------------------------------------------------------------------------------------------------
NEW = ('mcg_grad_stats_workspace_bytes', 'mcg_grad_stats_span', 'mcg_grad_stats', 'mcg_adam_wd_ctl')


def test_new_symbols_are_exported_and_prototyped(hl):
    lib = hl.load()
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mocogan_hip.h')).read(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in hl.SIGNATURES and re.search(r'\b%s\s*\(' % name, src), name
    assert 'typedef struct mcg_stat_seg { int64_t offset; int64_t n; } mcg_stat_seg;' in src
    assert lib.mcg_version() == hl.ABI_VERSION == 8
    assert ctypes.sizeof(hl.StatSeg) == 16
    span = lib.mcg_grad_stats_span()
    assert span > 0 and span % 4 == 0
    for nseg in (1, 10, 32):                                    # 32 bytes for each of MAX_PART = 512 blocks, whatever nseg
        assert int(lib.mcg_grad_stats_workspace_bytes(nseg)) == 512 * 32
    for nseg in (0, -1, 33):
        assert int(lib.mcg_grad_stats_workspace_bytes(nseg)) == 0


def test_grad_stats_refuses_on_the_host(hl):
    """`one` is a non-null pointer that is never dereferenced: no call below passes an acceptable argument set, null streams"""
    lib = hl.load()
    one = ctypes.c_void_p(16)
    segs = hl.stat_segs([(0, 8), (8, 5)])
    sp = ctypes.cast(segs, ctypes.c_void_p)

    def call(nseg=2, segs_p=sp, g=one, gs=1.0, thr=1.0, stats=one, ctl=one, ws=one):
        return lib.mcg_grad_stats(nseg, segs_p, g, gs, thr, stats, ctl, ws, None)
    for hole in ('segs_p', 'g', 'stats', 'ctl', 'ws'):
        assert call(**{hole: None}) == BAD, hole
    for nseg in (0, -1, 33):
        assert call(nseg=nseg) == BAD, nseg
    for items in ([(0, 0)], [(0, -4)], [(-1, 4)], [(0, 4), (4, 0)], [(0, 4), (-8, 4)]):
        s = hl.stat_segs(items)
        assert call(nseg=len(items), segs_p=ctypes.cast(s, ctypes.c_void_p)) == BAD, items
    for gs in (0.0, -1.0, math.inf, -math.inf, math.nan):
        assert call(gs=gs) == BAD, gs
    for thr in (0.0, -2.5, math.nan, -math.inf):
        assert call(thr=thr) == BAD, thr


def test_adam_wd_ctl_refuses_on_the_host(hl):
    lib = hl.load()
    one = ctypes.c_void_p(16)
    far = ctypes.c_void_p(1 << 20)

    def call(n=8, p=one, g=one, m=one, v=one, ctl=one, p16=one, ema=far, rate=0.5):
        return lib.mcg_adam_wd_ctl(n, p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 1e-5, ctl, p16, ema, rate, None)
    for hole in ('p', 'g', 'm', 'v', 'ctl'):
        assert call(**{hole: None}) == BAD, hole
    for n in (0, -3):
        assert call(n=n) == BAD, n
    for rate in (0.0, -0.1, 1.5, math.nan):                     # with an average: mcg_adam_wd_ema's rules
        assert call(rate=rate) == BAD, rate
    assert call(ema=one) == BAD                                 # the average overlaps p


# ---- the hook -----------------------------------------------------------------------------------------------------------------------
def test_adam_hyper_picks_up_gradient_clipping():
    from mocogan_chainer_amd import trainer as T
    from mocogan_chainer_amd import step
    h0 = step.AdamHyper()
    assert (h0.alpha, h0.beta1, h0.beta2, h0.eps, h0.weight_decay) == (2e-4, 5e-5, 0.999, 1e-8, 1e-5) and h0.clip is None
    assert T.GradientClipping.name == 'GradientClipping'
    o = T.Adam(alpha=2e-4, beta1=5e-5)
    o.add_hook(T.WeightDecay(1e-5), 'hook_dec')
    assert o.hyper().clip is None and o.hyper().weight_decay == 1e-5
    a, b = T.Adam(alpha=2e-4, beta1=5e-5), T.Adam(alpha=2e-4, beta1=5e-5)
    a.add_hook(T.WeightDecay(1e-5), 'w1'); a.add_hook(T.GradientClipping(5.0)); a.add_hook(T.WeightDecay(2e-5), 'w2')
    b.add_hook(T.GradientClipping(5.0), 'c'); b.add_hook(T.WeightDecay(2e-5), 'w2'); b.add_hook(T.WeightDecay(1e-5), 'w1')
    for o in (a, b):                                            # hook order does not matter; WeightDecay is still summed
        h = o.hyper()
        assert h.clip == 5.0 and h.weight_decay == pytest.approx(3e-5) and (h.alpha, h.beta1, h.beta2, h.eps) == (2e-4, 5e-5, 0.999, 1e-8)
    c = T.Adam()
    c.add_hook(T.GradientClipping(math.inf))
    assert c.hyper().clip == math.inf
    for bad in (0.0, -1.0, math.nan, -math.inf):
        d = T.Adam()
        d.add_hook(T.GradientClipping(bad))
        with pytest.raises(ValueError):
            d.hyper()
        with pytest.raises(ValueError):
            step.AdamHyper(clip=bad)


# ---- which launches adam_update makes ---------------------------------------------------------------------------------------------
class _Fp:
    def __init__(self):
        self.p, self.g, self.m, self.v, self.e, self.p16 = 'p', 'g', 'm', 'v', 'e', 'p16'
        self.touched = 0

    def touch(self):
        self.touched += 1


def _stub_net(precision='f32', ema=False, gstats=None):
    net = types.SimpleNamespace(t=4, fp=_Fp(), precision=precision, ema=None, gstats=gstats, running={'bn1/avg_mean': 'rm'}, refreshed=0)
    net.refresh_wsplits = lambda: setattr(net, 'refreshed', net.refreshed + 1)
    if ema:
        net.ema = types.SimpleNamespace(decay=0.999, k=2, running={'bn1/avg_mean': 'em'}, seen=0)
        net.ema.written = lambda live: setattr(net.ema, 'seen', net.ema.seen + 1)
    return net


@pytest.fixture()
def calls(monkeypatch):
    from mocogan_chainer_amd import hiplib
    rec = []
    for name in ('adam_wd', 'adam_wd_ema', 'adam_wd_ctl', 'grad_stats', 'ema_multi'):
        monkeypatch.setattr(hiplib, name, (lambda nm: lambda *a, **k: rec.append((nm, a, k)))(name))
    return rec


def test_off_is_off(calls):
    """options absent: exactly the launches and arguments of before the feature existed"""
    from mocogan_chainer_amd import step
    h = step.AdamHyper()
    net = _stub_net()
    step.adam_update(net, h, 0.25)
    assert calls == [('adam_wd', ('p', 'g', 'm', 'v', h.lr(5), h.beta1, h.beta2, h.eps, h.weight_decay, 0.25), {'p16': None})]
    assert net.t == 5 and net.fp.touched == 1 and net.refreshed == 1
    del calls[:]
    net = _stub_net('bf16', ema=True)
    step.adam_update(net, h)
    r = step.ema_rate(0.999, 2)
    assert calls == [('adam_wd_ema', ('p', 'g', 'm', 'v', h.lr(5), h.beta1, h.beta2, h.eps, h.weight_decay, 'e', r, 1.0), {'p16': 'p16'}),
                     ('ema_multi', ([('rm', 'em')], r), {})]
    assert net.ema.k == 3 and net.ema.seen == 1


class _Stats:
    ctl = 'ctl'

    def __init__(self):
        self.launched = []

    def launch(self, fp, grad_scale, threshold):
        self.launched.append((fp.g, grad_scale, threshold))


def test_statistics_alone_keep_the_update_on_its_launch(calls):
    from mocogan_chainer_amd import step
    h = step.AdamHyper()
    gs = _Stats()
    step.adam_update(_stub_net(gstats=gs), h, 0.5)
    assert gs.launched == [('g', 0.5, None)]
    assert [c[0] for c in calls] == ['adam_wd'] and calls[0][1][-1] == 0.5


def test_a_threshold_takes_the_ctl_route(calls):
    from mocogan_chainer_amd import step
    h = step.AdamHyper(clip=3.0)
    gs = _Stats()
    net = _stub_net('bf16', gstats=gs)
    step.adam_update(net, h, 0.5)
    assert gs.launched == [('g', 0.5, 3.0)]
    assert calls == [('adam_wd_ctl', ('p', 'g', 'm', 'v', h.lr(5), h.beta1, h.beta2, h.eps, h.weight_decay, 'ctl'),
                      {'ema': None, 'ema_rate': 0.0, 'p16': 'p16'})]
    del calls[:]
    net = _stub_net(ema=True, gstats=_Stats())
    step.adam_update(net, h)
    r = step.ema_rate(0.999, 2)
    assert calls[0] == ('adam_wd_ctl', ('p', 'g', 'm', 'v', h.lr(5), h.beta1, h.beta2, h.eps, h.weight_decay, 'ctl'),
                        {'ema': 'e', 'ema_rate': r, 'p16': None})
    assert calls[1] == ('ema_multi', ([('rm', 'em')], r), {}) and net.ema.k == 3          # (the host side advances, skipped or not)
    with pytest.raises(RuntimeError):                                                     # a threshold without the buffers: an error, no quiet plain update
        step.adam_update(_stub_net(), h)


# ---- train.py ------------------------------------------------------------------------------------------------------------------------
def test_train_flags_parse():
    import train
    a = train.parse_args([])
    assert a.grad_clip == 0.0 and a.grad_stats == 0
    a = train.parse_args(['--grad_clip', '5', '--grad_stats', '1'])
    assert a.grad_clip == 5.0 and a.grad_stats == 1
    assert train.parse_args(['--grad_clip', 'inf']).grad_clip == math.inf
    for bad in (['--grad_clip', '-1'], ['--grad_clip', 'nan'], ['--grad_clip', 'x'], ['--grad_stats', '2'], ['--grad_stats', 'yes']):
        with pytest.raises(SystemExit):
            train.parse_args(bad)


# ---- the reference statement ------------------------------------------------------------------------------------------------------
def test_reference_statistics_by_hand():
    g = np.array([3.0, -4.0, np.nan, 0.5, np.inf, -np.inf, 12.0, 0.0], np.float32)
    rows = gref.stats_rows(g, [(0, 2), (2, 3), (5, 1), (6, 2)])
    assert rows.tolist() == [[25.0, 4.0, 0.0, 0.0], [0.25, 0.5, 2.0, 0.0], [0.0, 0.0, 1.0, 0.0], [144.0, 12.0, 0.0, 0.0],
                             [169.25, 12.0, 3.0, 0.0]]
    assert np.array_equal(gref.total_row(rows[:-1]), rows[-1])
    # squares are exact in float64 (an fp32 accumulation would lose the small one), and the sum has no order: 2^-53 twice beside 1
    # vanishes when added one by one and must not
    y = np.array([2.0 ** -12, 1.0], np.float32)
    assert gref.segment_stats(y) == (1.0 + 2.0 ** -24, 1.0, 0)
    z = np.array([1.0, 2.0 ** -27, 2.0 ** -27, 2.0 ** -27], np.float32)
    assert 1.0 + 2.0 ** -54 == 1.0 and gref.segment_stats(z)[0] == 1.0 + 2.0 ** -52         # (1 + 3 * 2^-54, correctly rounded)


def test_reference_control_block_by_hand():
    f = lambda v: float(np.float32(v))
    # norm 5, threshold 2.5: rate 0.5
    assert gref.control(25.0, 0, 1.0, 2.5) == [0.5, 0.0, 0.5, 5.0, 5.0, 0.0]
    # threshold above the norm, +inf, and a zero gradient: rate 1 and ctl[0] is grad_scale itself
    for thr, ss in ((10.0, 25.0), (math.inf, 25.0), (1.0, 0.0)):
        c = gref.control(ss, 0, 1.0 / 3.0, thr, peak=1.0)
        assert c[0] == f(1.0 / 3.0) and c[1] == 0.0 and c[2] == 1.0 and c[3] == f(math.sqrt(ss) / 3.0) and c[4] == max(1.0, c[3])
    # grad_scale 0.25: the norm is the mean gradient's
    assert gref.control(64.0, 0, 0.25, 1.0, peak=3.0) == [0.125, 0.0, 0.5, 2.0, 3.0, 0.0]
    # a non-finite element: grad_scale, the flag, the counter; the peak stays
    assert gref.control(64.0, 2, 0.25, 1.0, peak=1.5, skipped=4.0) == [0.25, 1.0, 0.5, 2.0, 1.5, 5.0]


def test_reference_clipped_adam_is_scale_then_update():
    rng = np.random.RandomState(5)
    p0 = {'a/W': rng.randn(7, 3), 'a/b': rng.randn(3)}
    g = {k: rng.randn(*v.shape) * 4 for k, v in p0.items()}
    norm = math.sqrt(sum(float((v * v).sum()) for v in g.values()))
    for thr, gs in ((0.5 * norm, 1.0), (2 * norm, 1.0), (0.5 * norm * 0.25, 0.25), (math.inf, 1.0 / 3.0)):
        p, q = {k: v.copy() for k, v in p0.items()}, {k: v.copy() for k, v in p0.items()}
        sp, sq = oupd.new_adam_state(p), oupd.new_adam_state(q)
        for _ in range(3):
            rate, n_ = gref.clipped_adam_step(p, g, sp, thr, gs)
            want = min(1.0, thr / (gs * norm))
            assert rate == pytest.approx(want, rel=1e-15) and n_ == pytest.approx(gs * norm, rel=1e-15)
            oupd.adam_wd_update(q, {k: v * (gs * want) for k, v in g.items()}, sq)
        for k in p0:
            assert np.allclose(p[k], q[k], rtol=0, atol=1e-15) and np.allclose(sp['m'][k], sq['m'][k], rtol=1e-13, atol=0)
            assert np.allclose(sp['v'][k], sq['v'][k], rtol=1e-13, atol=0)
        assert sp['t'] == 3


def test_reference_reduce_callable_clips_in_place():
    rng = np.random.RandomState(6)
    grads = {'x/W': rng.randn(5, 4), 'x/b': rng.randn(4)}
    norm = math.sqrt(sum(float((v * v).sum()) for v in grads.values()))
    seen = {}
    red = gref.clipping_reduce({'image_dis': 0.5 * norm, 'video_dis': 2 * norm}, seen)
    a = {k: v.copy() for k, v in grads.items()}
    red('image_dis', a)
    assert all(np.allclose(a[k], 0.5 * grads[k], rtol=1e-15) for k in grads) and seen['image_dis'][0] == pytest.approx(0.5)
    b = {k: v.copy() for k, v in grads.items()}
    red('video_dis', b); red('image_gen', b)
    assert all(np.array_equal(b[k], grads[k]) for k in grads) and seen['video_dis'] == (1.0, pytest.approx(norm)) and seen['image_gen'][0] == 1.0
