"""Gradient statistics, norm clipping and the non-finite skip on the device: mcg_grad_stats and mcg_adam_wd_ctl at op level against
tests/grad_stats_ref.py (every tensor a view into a poisoned arena), the training step with clipping against the float64 oracle
(teacher-forced like tests/test_gpu_step.py, whose helpers and tolerances are imported), the skip, and the public surface."""
import copy
import math

import numpy as np
import pytest
import torch

import grad_stats_ref as gref
from guard import Arena
from oracle import net as onet
from oracle import updater as oupd
from test_gpu_step import (F64, PERF_SEEDS, TIGHT_MARGIN, _f64, check_params, dev, draw_to_dev, is_pre_bn_bias, noise_to_dev,
                           perf_mode_randomness, rel_l2)

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN, INF = float('nan'), float('inf')


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
def hl(pkg):
    return pkg[0]


@pytest.fixture(scope="module")
def _arena():
    return Arena(16 << 20)


@pytest.fixture()
def arena(_arena):
    _arena.reset()
    return _arena


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# ---- the apportioning rule of include/mocogan_hip.h, restated -------------------------------------------------------------------------
def max_part(hl):
    return int(hl.load().mcg_grad_stats_workspace_bytes(1)) // 32


def blocks_of(hl, sizes):
    S, N, P = hl.grad_stats_span(), sum(sizes), max_part(hl)
    return [min(-(-n // S), 1 + (P - len(sizes)) * n // N) for n in sizes]


def edge_sizes(hl):
    """1, 3, 4, 5, 255, S-1, S, S+1, 3S+2 and one segment that owns several blocks, in the ten-segment call and alone"""
    S = hl.grad_stats_span()
    sizes = [1, 3, 4, 5, 255, S - 1, S, S + 1, 3 * S + 2, 5 * S + 3]
    assert max_part(hl) == 512
    assert blocks_of(hl, sizes) == [1] * 7 + [2, 4, 6] and sum(blocks_of(hl, sizes)) <= max_part(hl)      # (a block per trip: none is short of blocks here)
    assert blocks_of(hl, [sizes[-1]]) == [6] and blocks_of(hl, [S + 1]) == [2] and blocks_of(hl, [600 * S]) == [512]
    return sizes


GAP = 8          # poisoned elements between two segments (a multiple of 4: every segment start keeps its alignment)


def lay_out(sizes):
    """[(offset, n)] with every segment on a 16-byte boundary and GAP elements between neighbours; total length"""
    segs, off = [], GAP
    for n in sizes:
        segs.append((off, n))
        off = (off + n + GAP + 3) // 4 * 4
    return segs, off


def make_gradient(arena, segs, total, rng, shift=0, zero=False):
    """the flat gradient in the arena: values randn * 10^U(-3, 3) inside the segments, the arena's NaN poison everywhere else (between
    the segments too).  shift = 1: the view starts one element late, so that every segment start is only 4-byte aligned.
    -> (device view, host copy)"""
    host = np.full(total, np.nan, F32)
    for off, n in segs:
        host[off:off + n] = 0.0 if zero else (rng.randn(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(F32)
    base = arena.empty((total + shift,))
    g = base[shift:]
    assert g.data_ptr() % 16 == 4 * shift
    for off, n in segs:
        g[off:off + n].copy_(torch.from_numpy(host[off:off + n]))
    assert bool(torch.isnan(g[:GAP]).all())
    return g, host


class Bufs:
    def __init__(self, hl, arena, nseg, ctl0=None):
        self.stats = arena.empty(((nseg + 1) * 4,), torch.float64)
        self.ctl = arena.put(torch.tensor(ctl0 if ctl0 is not None else [0.0] * 6 + [-7.0, 9.0], dtype=torch.float32))
        nws = int(hl.load().mcg_grad_stats_workspace_bytes(nseg)) // 8
        self.ws = arena.empty((nws,), torch.float64)


def run_stats(hl, arena, segs, g, grad_scale=1.0, threshold=INF, bufs=None):
    b = bufs or Bufs(hl, arena, len(segs))
    hl.grad_stats(hl.stat_segs(segs), g, grad_scale, threshold, b.stats, b.ctl, b.ws)
    torch.cuda.synchronize()
    return b.stats.cpu().numpy().reshape(-1, 4).copy(), b.ctl.cpu().numpy().copy(), b


def check_rows(rows, ref, segs, what):
    for i, (off, n) in enumerate(segs):
        err = abs(rows[i, 0] - ref[i, 0])
        print("PARITY grad_stats %s segment %d n=%d: |sumsq - fsum| / fsum %.2e (bound n * 2^-53 = %.2e)"
              % (what, i, n, err / max(ref[i, 0], 1e-300), n * 2.0 ** -53))
        assert math.isfinite(rows[i, 0]) and err <= n * 2.0 ** -53 * ref[i, 0], (what, i, n, rows[i, 0], ref[i, 0])
        assert rows[i, 1] == ref[i, 1] and rows[i, 2] == ref[i, 2] and rows[i, 3] == 0.0, (what, i, rows[i], ref[i])
    assert np.array_equal(rows[-1], gref.total_row(rows[:-1])), (what, rows[-1])


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
def test_statistics_at_the_edges(hl, arena, shift):
    """ten segments in one call and each size alone, on 16-byte boundaries (shift 0) and one element off them (shift 1: scalar head,
    16-byte body, scalar tail): the sum of squares within n * 2^-53 relative of math.fsum of the exact squares -- the worst case of
    ANY order of adding n non-negative doubles, each addition relative 2^-53 -- maximum and count exact, the total row formed from
    the segment rows as specified, two calls bit for bit the same, and the NaN poison around every segment never consumed"""
    rng = np.random.RandomState(11 + shift)
    sizes = edge_sizes(hl)
    segs, total = lay_out(sizes)
    g, host = make_gradient(arena, segs, total, rng, shift)
    ref = gref.stats_rows(host, segs)
    assert ref[-1, 2] == 0
    rows, ctl, _ = run_stats(hl, arena, segs, g)
    check_rows(rows, ref, segs, "ten segments, shift %d" % shift)
    again, ctl2, _ = run_stats(hl, arena, segs, g)
    assert np.array_equal(rows.view(np.int64), again.view(np.int64)) and np.array_equal(ctl[:4].view(np.int32), ctl2[:4].view(np.int32))
    assert ctl[1] == 0.0 and ctl[2] == 1.0 and ctl[6] == -7.0 and ctl[7] == 9.0
    for i, seg in enumerate(segs):
        one, _, _ = run_stats(hl, arena, [seg], g)
        check_rows(one, ref[[i, i]], [seg], "n = %d alone, shift %d" % (seg[1], shift))
        two, _, _ = run_stats(hl, arena, [seg], g)
        assert np.array_equal(one.view(np.int64), two.view(np.int64))
    arena.check()


def test_statistics_of_32_segments(hl, arena):
    rng = np.random.RandomState(13)
    S = hl.grad_stats_span()
    sizes = [int(v) for v in rng.choice([1, 2, 3, 4, 5, 7, 64, 255, 256, 1023, S - 3, S, S + 5, 2 * S + 1], 32)]
    assert len(set(sizes)) >= 8 and sum(blocks_of(hl, sizes)) > 32
    segs, total = lay_out(sizes)
    g, host = make_gradient(arena, segs, total, rng)
    rows, _, _ = run_stats(hl, arena, segs, g)
    check_rows(rows, gref.stats_rows(host, segs), segs, "32 segments")
    again, _, _ = run_stats(hl, arena, segs, g)
    assert np.array_equal(rows.view(np.int64), again.view(np.int64))
    arena.check()


@pytest.mark.parametrize("shift", [0, 1])
def test_statistics_when_blocks_take_several_trips(hl, arena, shift):
    """more trips than MAX_PART blocks: 600 S + 5 elements are 601 trips for 512 blocks, so the first 89 blocks take two (the smallest
    size at which a block's second trip runs) -- and beside it a 3 S + 2 segment that the size rule leaves 3 blocks for 4 trips"""
    rng = np.random.RandomState(37 + shift)
    S = hl.grad_stats_span()
    sizes = [600 * S + 5, 3 * S + 2]
    both = blocks_of(hl, sizes)
    assert 300 < both[0] < 601 and both[1] == 3 and sum(both) <= max_part(hl) and blocks_of(hl, sizes[:1]) == [512]
    segs, total = lay_out(sizes)
    g, host = make_gradient(arena, segs, total, rng, shift)
    ref = gref.stats_rows(host, segs)
    rows, _, _ = run_stats(hl, arena, segs, g)
    check_rows(rows, ref, segs, "several trips, shift %d" % shift)
    one, _, _ = run_stats(hl, arena, segs[:1], g)
    check_rows(one, ref[[0, 0]], segs[:1], "several trips, alone, shift %d" % shift)
    again, _, _ = run_stats(hl, arena, segs, g)
    assert np.array_equal(rows.view(np.int64), again.view(np.int64))
    arena.check()


# ---- non-finite elements ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
def test_non_finite_elements_are_counted_and_skip_the_update(hl, arena, shift):
    rng = np.random.RandomState(17 + shift)
    sizes = edge_sizes(hl)
    S = hl.grad_stats_span()
    segs, total = lay_out(sizes)
    g, host = make_gradient(arena, segs, total, rng, shift)
    clean, ctl_clean, b = run_stats(hl, arena, segs, g, threshold=1.0)
    assert ctl_clean[1] == 0.0 and ctl_clean[5] == 0.0 and ctl_clean[4] == ctl_clean[3] > 0.0
    # segment index -> [(element, value)]: first, last and tail (n % 4 last) elements; segment 3 (n = 5) and 7 (n = S + 1) have a
    # one-element tail, 5 (n = S - 1) a three-element one, 9 owns several blocks
    hits = {1: [(0, NAN)], 3: [(4, -INF)], 5: [(S - 2, INF), (S - 4, NAN), (0, INF)], 7: [(S, NAN)], 9: [(0, -INF), (5 * S + 2, NAN), (2 * S + 1, INF)]}
    for s, lst in hits.items():
        off, n = segs[s]
        assert all(0 <= e < n for e, _ in lst)
        for e, v in lst:
            host[off + e] = v
            g[off + e] = v
    ref = gref.stats_rows(host, segs)
    assert [int(c) for c in ref[:-1, 2]] == [0, 1, 0, 1, 0, 3, 0, 1, 0, 3] and ref[-1, 2] == 9
    rows, ctl, _ = run_stats(hl, arena, segs, g, threshold=1.0, bufs=b)
    check_rows(rows, ref, segs, "non-finite, shift %d" % shift)
    for s in range(len(segs)):
        if s not in hits:
            assert np.array_equal(rows[s].view(np.int64), clean[s].view(np.int64)), s
    assert ctl[1] == 1.0 and ctl[5] == 1.0 and ctl[0] == 1.0                       # grad_scale itself; the flag; one skipped update
    assert ctl[4].view(np.int32) == ctl_clean[4].view(np.int32)                     # the peak is that of the clean call
    _, ctl, _ = run_stats(hl, arena, segs, g, threshold=1.0, bufs=b)
    assert ctl[1] == 1.0 and ctl[5] == 2.0 and ctl[4].view(np.int32) == ctl_clean[4].view(np.int32)
    assert ctl[6] == -7.0 and ctl[7] == 9.0
    arena.check()


# ---- the control block --------------------------------------------------------------------------------------------------------------------
def within_one_ulp(got, want):
    want = F32(want)
    return abs(float(got) - float(want)) <= float(np.spacing(np.abs(want)))


@pytest.mark.parametrize("grad_scale", [1.0, 0.25, 1.0 / 3.0])
def test_control_block(hl, arena, grad_scale):
    """ctl[0], ctl[2], ctl[3] within one fp32 ulp of the float64 statement (the device's double sum and fsum may differ in the last
    bits before the rounding to float); ctl[0] exactly (float)grad_scale when nothing is clipped; the peak; ctl[6..7] left alone"""
    rng = np.random.RandomState(19)
    sizes = [5, 255, hl.grad_stats_span() + 1, 1027]
    segs, total = lay_out(sizes)
    g, host = make_gradient(arena, segs, total, rng)
    ref = gref.stats_rows(host, segs)
    norm = grad_scale * math.sqrt(ref[-1, 0])
    b = Bufs(hl, arena, len(segs))
    peak = 0.0
    for factor in (2.0, 0.5, INF):
        thr = factor * norm
        _, ctl, _ = run_stats(hl, arena, segs, g, grad_scale, thr, bufs=b)
        want = gref.control(ref[-1, 0], 0, grad_scale, thr, peak=peak)
        print("PARITY ctl gs=%.4f factor %s: got %r want %r" % (grad_scale, factor, ctl[:6].tolist(), want))
        for i in (0, 2, 3):
            assert within_one_ulp(ctl[i], want[i]), (factor, i, ctl[i], want[i])
        assert ctl[1] == 0.0 and ctl[5] == 0.0 and ctl[6] == -7.0 and ctl[7] == 9.0
        if factor >= 1.0:
            assert ctl[2] == 1.0 and ctl[0] == F32(grad_scale)
        else:
            assert ctl[2] < 1.0
        peak = max(peak, float(ctl[3]))
        assert ctl[4] == F32(peak)
    # an all-zero gradient: norm 0, rate 1, the scale is grad_scale
    gz, _ = make_gradient(arena, segs, total, rng, zero=True)
    rows, ctl, _ = run_stats(hl, arena, segs, gz, grad_scale, 1e-3, bufs=b)
    assert np.array_equal(rows, np.zeros_like(rows)) and ctl[:4].tolist() == [float(F32(grad_scale)), 0.0, 1.0, 0.0] and ctl[4] == F32(peak)
    arena.check()


# ---- Adam through the control block -------------------------------------------------------------------------------------------------------
def _offset(arena, a, offset, dtype=torch.float32):
    base = arena.zeros((len(a) + 4,), dtype)
    t = base[offset:offset + len(a)]
    t.copy_(torch.as_tensor(np.asarray(a)).to(dtype))
    return t


ADAM = (oupd.ADAM_BETA1, oupd.ADAM_BETA2, oupd.ADAM_EPS, oupd.WEIGHT_DECAY)


def _lr(t):
    return oupd.ADAM_ALPHA * math.sqrt(1 - oupd.ADAM_BETA2 ** t) / (1 - oupd.ADAM_BETA1 ** t)


@pytest.mark.parametrize("with_p16", [False, True])
@pytest.mark.parametrize("with_ema", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
def test_adam_ctl_equals_adam_with_the_scale_read_back(hl, arena, offset, with_ema, with_p16):
    """mcg_adam_wd_ctl with the control block a real mcg_grad_stats call left is bit for bit mcg_adam_wd / mcg_adam_wd_ema called
    with grad_scale = float(ctl[0]) -- p, m, v, p16, ema; with ctl[1] = 1 all five keep their bits"""
    rng = np.random.RandomState(23)
    for n in (1, 3, 4, 5, 1027):
        p0, g0 = rng.randn(n).astype(F32), (rng.randn(n) * 3).astype(F32)
        m0, v0, e0 = (rng.randn(n) * 0.1).astype(F32), (rng.rand(n) * 0.1).astype(F32), rng.randn(n).astype(F32)
        g = _offset(arena, g0, offset)
        norm = math.sqrt(gref.segment_stats(g0)[0])
        b = Bufs(hl, arena, 1)
        hl.grad_stats(hl.stat_segs([(0, n)]), g, 0.5, 0.25 * norm * 0.5, b.stats, b.ctl, b.ws)
        ctl = b.ctl.cpu().numpy()
        assert ctl[1] == 0.0 and within_one_ulp(ctl[0], 0.125) and ctl[0] != 0.5

        def state():
            return [_offset(arena, p0, offset), _offset(arena, m0, offset), _offset(arena, v0, offset),
                    _offset(arena, np.zeros(n), offset, torch.bfloat16) if with_p16 else None, _offset(arena, e0, offset) if with_ema else None]
        a, c = state(), state()
        hl.adam_wd_ctl(a[0], g, a[1], a[2], _lr(3), *ADAM, b.ctl, ema=a[4], ema_rate=0.25, p16=a[3])
        if with_ema:
            hl.adam_wd_ema(c[0], g, c[1], c[2], _lr(3), *ADAM, c[4], 0.25, grad_scale=float(ctl[0]), p16=c[3])
        else:
            hl.adam_wd(c[0], g, c[1], c[2], _lr(3), *ADAM, grad_scale=float(ctl[0]), p16=c[3])
        for name, x, y in zip(("p", "m", "v", "p16", "ema"), a, c):
            if x is not None:
                assert same_bits(x, y), (n, name)
        assert not torch.equal(a[0], torch.from_numpy(p0).cuda())
        # ... and the skip
        b.ctl[1] = 1.0
        snap = [None if x is None else x.clone() for x in a]
        hl.adam_wd_ctl(a[0], g, a[1], a[2], _lr(4), *ADAM, b.ctl, ema=a[4], ema_rate=0.25, p16=a[3])
        for name, x, y in zip(("p", "m", "v", "p16", "ema"), a, snap):
            if x is not None:
                assert same_bits(x, y), (n, name, "skip")
    arena.check()


@pytest.mark.parametrize("offset", [0, 1])
def test_three_clipped_steps_against_float64(hl, arena, offset):
    """grad_stats -> adam_wd_ctl, three chained steps with the all-reduced SUM of three ranks (grad_scale 1 / 3) and a threshold
    half the first norm, against tests/grad_stats_ref.py in float64; tolerances of test_gpu_ops.test_adam_grad_scale_against_float64
    (p 1e-6 absolute, m and v rel-L2 1e-6: its docstring derives them; the scale read from ctl[0] is one more fp32 rounding of the
    same size as the ones counted there)"""
    rng = np.random.RandomState(29)
    n, W = 1027, 3
    p0 = rng.randn(n).astype(F32)
    sums = [(rng.randn(n) * 2.0).astype(F32) for _ in range(3)]
    thr = 0.5 * math.sqrt(gref.segment_stats(sums[0])[0]) / W
    p = {'x/W': p0.astype(F64)}
    st = oupd.new_adam_state(p)
    pd, md, vd = _offset(arena, p0, offset), _offset(arena, np.zeros(n), offset), _offset(arena, np.zeros(n), offset)
    b = Bufs(hl, arena, 1)
    clipped = 0
    for t, g_sum in enumerate(sums, 1):
        rate, _ = gref.clipped_adam_step(p, {'x/W': g_sum.astype(F64)}, st, thr, 1.0 / W)
        clipped += rate < 1.0
        gd = _offset(arena, g_sum, offset)
        hl.grad_stats(hl.stat_segs([(0, n)]), gd, 1.0 / W, thr, b.stats, b.ctl, b.ws)
        hl.adam_wd_ctl(pd, gd, md, vd, _lr(t), *ADAM, b.ctl)
        e_p = np.abs(pd.cpu().double().numpy() - p['x/W']).max()
        e_m, e_v = rel_l2(md, st['m']['x/W']), rel_l2(vd, st['v']['x/W'])
        print("PARITY clipped adam offset %d step %d: rate %.4f, max |p - p64| %.2e (1e-6), m %.2e, v %.2e (rel-L2, 1e-6)" % (offset, t, rate, e_p, e_m, e_v))
        assert within_one_ulp(b.ctl.cpu().numpy()[2], rate)
        assert e_p < 1e-6 and e_m < 1e-6 and e_v < 1e-6, (t, e_p, e_m, e_v)
    assert clipped == 3
    arena.check()


# ---- the training step ----------------------------------------------------------------------------------------------------------------------
NETS = ('image_gen', 'image_dis', 'video_dis')
FACTORS = {'image_dis': 0.5, 'video_dis': 2.0, 'image_gen': 0.25}        # threshold / un-clipped oracle norm: D_I and G clip, D_V does not


def _clipped_steps(pkg, model, dim_zl, seed, steps, overlap=False, perf=None, min_tight_steps=None, nf=4, n=2):
    """tests/test_gpu_step._run_steps with a GradientClipping threshold on every optimizer: the oracle clips through update_core's
    reduce= callable, thresholds FACTORS x the norms of an un-clipped oracle pass from the same state.  The comparisons and their
    tolerances are _run_steps' (forward 1e-5 / 2e-5, gradients and parameters 1e-4 on a well-conditioned iteration); on top the
    device's norms and clipping rates against the oracle's to the gradient tolerance."""
    hl, lay, nets, step = pkg
    rng = np.random.RandomState(seed)
    out_c = 7 if model == 'infogan' else 1
    c_d = 3 + (dim_zl if model == 'cgan' else 0)
    gen = _f64(onet.init_generator(rng, dim_zl=dim_zl, n_filters=nf))
    di = _f64(onet.init_discriminator(rng, 2, c_d, out_c, nf))
    dv = _f64(onet.init_discriminator(rng, 3, c_d, out_c, nf))
    G = nets.GenNet(dim_zl=dim_zl, n_filters=nf)
    DI = nets.DisNet(2, c_d, out_c, nf, use_noise=True)
    DV = nets.DisNet(3, c_d, out_c, nf, use_noise=True)
    hyper = {k: step.AdamHyper(clip=math.inf) for k in NETS}
    ts = step.TrainStep(model, G, DI, DV, hyper=hyper, overlap=overlap, **({'seed': perf[0], 'rank': perf[1]} if perf else {}))
    og, oi, ov = (oupd.new_adam_state(q) for q in (gen, di, dv))
    tight_steps = 0
    for s in range(steps):
        for net, p, st in ((G, gen, og), (DI, di, oi), (DV, dv, ov)):      # teacher forcing
            net.load_reference_params(p)
            net.load_adam_state(st)
        x_real = rng.uniform(-1, 1, (n, 3, 16, 64, 64))
        t_real = rng.randint(0, 6, n)
        if perf:
            assert ts.iteration == s
            rnd = perf_mode_randomness(perf[0], s, perf[1], model, n, nf, dim_zl)
            inject = None
        else:
            rnd = oupd.draw_step_randomness(rng, model, n, 3, nf, dim_zl=dim_zl, dtype=F64)
            inject = {'t': rnd['t'], 'gen': draw_to_dev(rnd['gen'])}
            for k in ('noise_i_real', 'noise_v_real', 'noise_i_fake', 'noise_v_fake'):
                inject[k] = noise_to_dev(lay, rnd[k])
        plain = {}
        oupd.update_core(model, *copy.deepcopy((gen, di, dv, og, oi, ov)), x_real, t_real, rnd, dim_zl=dim_zl,
                         reduce=gref.clipping_reduce({}, plain))
        thresholds = {k: FACTORS[k] * plain[k][1] for k in NETS}
        for k in NETS:
            ts.hyper[k].clip = thresholds[k]
        seen = {}
        ref = oupd.update_core(model, gen, di, dv, og, oi, ov, x_real, t_real, rnd, dim_zl=dim_zl, keep=True,
                               reduce=gref.clipping_reduce(thresholds, seen))
        assert seen['image_dis'][0] == pytest.approx(0.5) and seen['video_dis'][0] == 1.0 and 0.2 < seen['image_gen'][0] < 0.3
        out = ts.run(dev(x_real), dev(t_real, torch.int32), inject)
        losses = ts.losses()
        stats = ts.grad_stats()
        assert abs(losses['image_dis/loss'] - ref['loss_dis_i']) < 1e-5, s
        assert abs(losses['video_dis/loss'] - ref['loss_dis_v']) < 1e-5, s
        assert abs(losses['image_gen/loss'] - ref['loss_gen']) < 1e-5, s
        assert rel_l2(lay.act_from_dev(out['x_fake'], 3), ref['x_fake'][:, :3]) < 1e-5, s
        for k in ('y_real_i', 'y_real_v', 'y_fake_i', 'y_fake_v'):
            assert rel_l2(out[k], ref[k].reshape(out[k].shape)) < 2e-5, (s, k)
        tight = ref['min_margin'] > TIGHT_MARGIN
        print("clipped step %s seed %d iteration %d: min_margin %.3e" % (model, seed, s, ref['min_margin']))
        tight_steps += tight
        gtol, ptol = (1e-4, 1e-4) if tight else (0.15, 1e-2)
        assert rel_l2(lay.act_from_dev(out['gx_fake'], 3), ref['gx_fake']) < gtol, (s, ref['min_margin'])
        for name, key, net, kind, refg, p in (('D_I', 'image_dis', DI, 'dis', ref['grads_dis_i'], di), ('D_V', 'video_dis', DV, 'dis', ref['grads_dis_v'], dv),
                                              ('G', 'image_gen', G, 'gen', ref['grads_gen'], gen)):
            got = net.export_reference_grads()                                # (the flat gradient is left un-clipped: the scale lives in the Adam launch)
            for k in refg:
                if not is_pre_bn_bias(k, kind):
                    tiny = refg[k].size <= 8 and np.abs(np.asarray(got[k], F64) - refg[k]).max() < 5e-7
                    assert tiny or rel_l2(got[k], refg[k]) < gtol, (s, name, k, ref['min_margin'])
            rate, norm = seen[key]
            check_params(net.export_reference_params(), p, kind, ptol, '%s step %d' % (name, s), {k: rate * v for k, v in refg.items()},
                         0.0 if tight else gtol)
            st = stats[key]
            print("PARITY grad_stats %s: norm %.6e (oracle %.6e), clip_rate %.6f (oracle %.6f)" % (key, st['grad_norm'], norm, st['clip_rate'], rate))
            assert abs(st['grad_norm'] - norm) < gtol * norm and abs(st['clip_rate'] - rate) < gtol * rate, (s, key, st, seen[key])
            assert st['grad_norm_peak'] == st['grad_norm'] and st['nonfinite'] == 0 and st['skipped'] == 0 and st['grad_max'] > 0
            assert list(st['tensors']) == net.fp.names and all(math.isfinite(v) for v in st['tensors'].values())
            assert math.sqrt(sum(v * v for v in st['tensors'].values())) == pytest.approx(st['grad_norm'], rel=1e-6)
        assert stats['video_dis']['clip_rate'] == 1.0 and stats['image_dis']['clip_rate'] < 1.0
        assert G.t == DI.t == DV.t == s + 1
    if min_tight_steps is None:
        min_tight_steps = steps
    assert tight_steps >= min_tight_steps, "seed no longer yields a well-conditioned iteration"


@pytest.mark.parametrize("model,dim_zl,seed", [("normal", 0, 1267), ("cgan", 6, 320)])
def test_clipped_step_matches_the_oracle(pkg, model, dim_zl, seed):
    """one injected iteration each, the seeds of test_update_core_three_steps: clipping changes nothing before the first Adam launch,
    so the iteration's min_margin is theirs -- asserted > TIGHT_MARGIN all the same"""
    _clipped_steps(pkg, model, dim_zl, seed, steps=1)


def test_clipped_step_with_side_streams(pkg):
    _clipped_steps(pkg, "normal", 0, 1267, steps=1, overlap=True)


CLIP_PERF = ("normal", 0, 1303, PERF_SEEDS[("normal", 0, 0)])     # (model, dim_zl, NumPy seed, Philox seed): see the test below


def test_clipped_step_in_perf_mode(pkg):
    """two iterations of the benchmarked schedule (in-kernel Philox) with clipping.  The second iteration starts from parameters a
    CLIPPED update wrote, so its pre-activations are not those of the un-clipped seeds: the pair of seeds was checked on the CPU
    with the oracle (this file's _clipped_steps loop without the device half) for min_margin > TIGHT_MARGIN in both iterations,
    as tests/test_gpu_augment.py documents doing for its cases: 2.66e-6 and 2.37e-6 (of the 27 pairs tried -- NumPy seeds 1303,
    1311, 1400..1411 with rank 0's Philox seeds of PERF_SEEDS -- the only one with both above the margin)."""
    model, dim_zl, seed, pseed = CLIP_PERF
    _clipped_steps(pkg, model, dim_zl, seed, steps=2, overlap=True, perf=(pseed, 0))


def _fresh_nets(pkg, seed, nf=4):
    hl, lay, nets, step = pkg
    rng = np.random.RandomState(seed)
    params = (_f64(onet.init_generator(rng, dim_zl=0, n_filters=nf)), _f64(onet.init_discriminator(rng, 2, 3, 1, nf)),
              _f64(onet.init_discriminator(rng, 3, 3, 1, nf)))
    devnets = (nets.GenNet(dim_zl=0, n_filters=nf), nets.DisNet(2, 3, 1, nf, use_noise=True), nets.DisNet(3, 3, 1, nf, use_noise=True))
    for net, p in zip(devnets, params):
        net.load_reference_params(p)
    return rng, params, devnets


def test_statistics_alone_leave_the_step_as_it_is(pkg):
    """grad_stats=True without a threshold: the plain TrainStep's iteration from the same state, to the 1e-5 check_params bound of
    test_gpu_augment.test_identity_policy_matches_the_plain_step (weight gradients use float atomics, so not bit for bit); the
    statistics are there and nothing was clipped"""
    hl, lay, nets, step = pkg
    results = []
    for flag in (False, True):
        rng, _, devnets = _fresh_nets(pkg, 1267)
        x_real, t_real = rng.uniform(-1, 1, (2, 3, 16, 64, 64)), rng.randint(0, 6, 2)
        rnd = oupd.draw_step_randomness(rng, 'normal', 2, 3, 4, dim_zl=0, dtype=F64)
        inject = {'t': rnd['t'], 'gen': draw_to_dev(rnd['gen'])}
        for k in ('noise_i_real', 'noise_v_real', 'noise_i_fake', 'noise_v_fake'):
            inject[k] = noise_to_dev(lay, rnd[k])
        ts = step.TrainStep('normal', *devnets, **({'grad_stats': True} if flag else {}))
        ts.run(dev(x_real), dev(t_real, torch.int32), inject)
        torch.cuda.synchronize()
        results.append((ts, [net.export_reference_params() for net in devnets], [net.export_reference_grads() for net in devnets]))
    (plain, p_plain, _), (withs, p_with, grads) = results
    assert plain.grad_stats() == {} and all(net.gstats is None for net in (plain.gen, plain.dis_i, plain.dis_v))
    for a, b, kind in zip(p_with, p_plain, ('gen', 'dis', 'dis')):
        check_params(a, b, kind, 1e-5, 'statistics only, ' + kind)
    st = withs.grad_stats()
    assert sorted(st) == sorted(NETS)
    for key, gr in zip(NETS, grads):
        norm = math.sqrt(sum(float((np.asarray(v, F64) ** 2).sum()) for v in gr.values()))
        assert st[key]['grad_norm'] == pytest.approx(norm, rel=1e-6) and st[key]['clip_rate'] == 1.0 and st[key]['skipped'] == 0
    assert withs.grad_stats()['image_gen']['grad_norm_peak'] == 0.0               # zeroed behind the first read


def test_a_non_finite_gradient_skips_the_update(pkg):
    """a NaN written into D_V's flat gradient between backward and update: parameters and moments keep their bits, skipped == 1, the
    host's step counter has advanced (nothing waits for the device), and the next clean update proceeds"""
    hl, lay, nets, step = pkg
    rng, _, (G, DI, DV) = _fresh_nets(pkg, 7)
    DV.enable_grad_stats()
    h = step.AdamHyper(clip=math.inf)
    DV.fp.g.copy_(torch.from_numpy(rng.randn(DV.fp.size).astype(F32)))
    DV.fp.m.copy_(torch.from_numpy((rng.randn(DV.fp.size) * 0.1).astype(F32)))
    DV.fp.v.copy_(torch.from_numpy((rng.rand(DV.fp.size) * 0.1).astype(F32)))
    before = [t.clone() for t in (DV.fp.p, DV.fp.m, DV.fp.v)]
    clean_g = DV.fp.g.clone()
    DV.fp.g[DV.fp.offsets['dc3/W'] + 5] = NAN
    step.adam_update(DV, h)
    for name, x, y in zip("pmv", (DV.fp.p, DV.fp.m, DV.fp.v), before):
        assert same_bits(x, y), name
    st = DV.gstats.read()
    assert st['skipped'] == 1 and st['nonfinite'] == 1 and st['clip_rate'] == 1.0 and DV.t == 1
    assert math.isfinite(st['grad_norm']) and st['grad_norm_peak'] == 0.0 and math.isfinite(st['tensors']['dc3/W'])
    DV.fp.g.copy_(clean_g)
    step.adam_update(DV, h)
    st = DV.gstats.read()
    assert st['skipped'] == 1 and st['nonfinite'] == 0 and DV.t == 2 and st['grad_norm_peak'] == st['grad_norm'] > 0
    assert not torch.equal(DV.fp.p, before[0]) and not torch.equal(DV.fp.m, before[1]) and bool(torch.isfinite(DV.fp.p).all())
    # ... bit for bit the plain update of the same state at t = 2
    ref_p, ref_m, ref_v = [t.clone() for t in before]
    hl.adam_wd(ref_p, clean_g, ref_m, ref_v, h.lr(2), h.beta1, h.beta2, h.eps, h.weight_decay, 1.0)
    assert same_bits(ref_p, DV.fp.p) and same_bits(ref_m, DV.fp.m) and same_bits(ref_v, DV.fp.v)


# ---- surface ----------------------------------------------------------------------------------------------------------------------------------
NEW_KEYS = ['%s/%s' % (n, k) for n in NETS for k in ('grad_norm', 'grad_norm_peak', 'clip_rate', 'skipped')]


def test_updater_reports_the_statistics(pkg):
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
        if name == 'video_dis':
            o.add_hook(T.GradientClipping(1e-3))
        opts[name] = o

    class Writer(T.NullWriter):
        tags = []

        def add_scalar(self, tag, *a, **k):
            self.tags.append(tag)
    u = Updater(model='normal', models=(g, di, dv), video_length=16, img_size=64, channel=3, dim_zl=6, tensorboard_writer=Writer(),
                iterator=T.SerialIterator(SyntheticDataset(12, 6), 4), optimizer=opts, device=0, grad_stats=True)
    for i in range(3):
        u.update()
        assert (set(NEW_KEYS) <= set(u.observation)) == (i == 2)                 # with the losses, at the new epoch
    assert u.is_new_epoch and u.iteration == 3
    assert all(math.isfinite(u.observation[k]) for k in NEW_KEYS + ['image_gen/loss', 'image_dis/loss', 'video_dis/loss'])
    assert u.observation['video_dis/clip_rate'] < 1.0 and u.observation['image_dis/clip_rate'] == 1.0 and u.observation['video_dis/skipped'] == 0
    assert u.observation['video_dis/grad_norm_peak'] >= u.observation['video_dis/grad_norm'] > 0
    assert any(t.startswith('grad_norm:') for t in Writer.tags) and any(t.startswith('clip_rate:') for t in Writer.tags)


def test_train_entry_point_with_the_flags(pkg, tmp_path, monkeypatch):
    import json
    import train
    monkeypatch.chdir(tmp_path)
    try:
        tr = train.main(['--dataset_type', 'synthetic', '--synthetic_size', '8', '--batchsize', '4', '--max_epoch', '1', '--n_filters_gen', '8',
                         '--snapshot_interval', '1', '--log_tensorboard_interval', '100', '--num_gen_samples', '4', '--save_name', 'gs',
                         '--grad_clip', '5', '--grad_stats', '1'])
        assert tr.updater.iteration == 2
        assert all(tr.updater._step.hyper[k].clip == 5.0 for k in NETS)
        assert all(np.isfinite(v) for v in tr.updater._step.losses().values())
        log = json.load(open(tmp_path / 'result' / 'gs' / 'log'))
        assert all(math.isfinite(log[-1][k]) for k in NEW_KEYS)
    finally:
        pkg[0].reset_tuning()                                            # (main() switched the tile tuner on with the shipped table)
