"""The averaged generator on the GPU: the fused Adam + average kernel against the plain Adam kernel (bit for bit) and against the
float64 recurrence, the multi-segment average of the running statistics, the averaged generator following a training step through
every copy derived from its weights, and train.py / generate_samples.py on the averaged files.

The reference for the average is its recurrence in float64, teacher-forced: fed the device's own fp32 parameters after each step
and the rate as the float the kernel was given,

    e64 <- x                          if r == 1
    e64 <- e64 + r * (x - e64)        otherwise

Bound after s updates: |e - e64| <= s * 2^-22 * M, M the largest |x| or |e| seen.  One rounding of x - e (|x - e| <= 2 M) and one of
the fma (|result| <= M) give at most 3 * 2^-24 * M per update, and what was there before is multiplied by 1 - r <= 1."""
import numpy as np
import pytest
import torch

from guard import Arena

pytestmark = pytest.mark.gpu

ADAM = dict(lr_t=2e-4 * np.sqrt(1 - 0.999) / (1 - 5e-5), beta1=5e-5, beta2=0.999, eps=1e-8, wd=1e-5)
SIZES = [1, 3, 4, 5, 255, 257, 1027, 4194309]          # the last: two sweeps of a 2048 x 256 x 4 grid and a tail of 5
ULP22 = 2.0 ** -22


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return Arena(32 << 20)


def schedule(D, steps):
    from mocogan_chainer_amd.step import ema_rate
    return [ema_rate(D, k) for k in range(steps)]


def _operands(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.05
    grad = torch.randn(n, generator=g) * 1e-2
    m = torch.randn(n, generator=g) * 1e-2
    v = torch.rand(n, generator=g) * 1e-4
    e = torch.randn(n, generator=g) * 0.05
    return p, grad, m, v, e


class _Alloc:
    """n-element tensors inside the guard arena (small n) or plain device tensors (large n), optionally one element past an
    aligned address: every pointer then misses the 16-byte boundary (the bf16 copy misses its 8-byte one)"""

    def __init__(self, arena, offset):
        self.arena, self.offset = arena, offset

    def put(self, t):
        n, o = t.numel(), self.offset
        if self.arena is None:
            buf = torch.empty(n + o, dtype=t.dtype, device='cuda')
        else:
            buf = self.arena.empty((n + o,), t.dtype)
            if o:
                buf[:o].zero_()                            # (the element in front is the test's own: it must stay as it is)
        out = buf[o:]
        out.copy_(t)
        assert out.data_ptr() % 16 == (o * t.element_size()) % 16 and out.is_contiguous()
        return out


def _alloc(arena, n, offset):
    if n > 4096:
        return _Alloc(None, offset)
    arena.reset()
    return _Alloc(arena, offset)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_fused_kernel_writes_what_adam_wd_writes(hl, arena, n, offset):
    """p, m, v and the bf16 copy bit for bit, at every size class (single element, below / at / above one 16-byte group, around one
    block, tail behind full groups, more than one sweep of the capped grid) on aligned and on unaligned pointers"""
    a = _alloc(arena, n, offset)
    ops = _operands(n, 100 + n % 97)
    p1, g1, m1, v1, _ = (a.put(t) for t in ops)
    p2, g2, m2, v2, e2 = (a.put(t) for t in ops)
    q1 = a.put(torch.zeros(n, dtype=torch.bfloat16))
    q2 = a.put(torch.zeros(n, dtype=torch.bfloat16))
    hl.adam_wd(p1, g1, m1, v1, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], 0.5, p16=q1)
    hl.adam_wd_ema(p2, g2, m2, v2, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], e2, 0.25, 0.5, p16=q2)
    torch.cuda.synchronize()
    assert not torch.equal(p1, ops[0].cuda())                            # (the update is not a no-op)
    for name, x, y in (('p', p1, p2), ('m', m1, m2), ('v', v1, v2), ('p16', q1, q2)):
        assert torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int16),
                           y.view(torch.int32 if y.dtype == torch.float32 else torch.int16)), name
    assert torch.equal(g2, ops[1].cuda())
    # the average moved towards the new parameter: |e - e64| within one update's bound
    e64 = ops[4].double() + float(np.float32(0.25)) * (p2.cpu().double() - ops[4].double())
    M = max(float(p2.abs().max()), float(ops[4].abs().max()), float(e2.abs().max()))
    assert float((e2.cpu().double() - e64).abs().max()) <= ULP22 * M
    # without the bf16 copy the same three buffers come out
    p3, g3, m3, v3, e3 = (a.put(t) for t in ops) if n <= 4096 else (t.cuda() for t in ops)
    hl.adam_wd_ema(p3, g3, m3, v3, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], e3, 0.25, 0.5)
    assert torch.equal(p3, p1) and torch.equal(m3, m1) and torch.equal(v3, v1) and torch.equal(e3, e2)
    if a.arena is not None:
        a.arena.check()


def test_fused_kernel_with_only_the_average_unaligned(hl, arena):
    n = 1027
    arena.reset()
    ops = _operands(n, 7)
    al, un = _Alloc(arena, 0), _Alloc(arena, 1)
    p1, g1, m1, v1, e1 = (al.put(t) for t in ops)
    p2, g2, m2, v2 = (al.put(t) for t in ops[:4])
    e2 = un.put(ops[4])
    for p, g, m, v, e in ((p1, g1, m1, v1, e1), (p2, g2, m2, v2, e2)):
        hl.adam_wd_ema(p, g, m, v, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], e, 0.125)
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2) and torch.equal(e1, e2)
    arena.check()


@pytest.mark.parametrize("off16", [1, 2, 3])
def test_fused_kernel_with_only_the_bf16_copy_unaligned(hl, arena, off16):
    """every fp32 pointer on a 16-byte boundary, the bf16 copy 2, 4 or 6 bytes past an 8-byte one: the scalar form runs"""
    n = 1027
    arena.reset()
    ops = _operands(n, 9)
    al = _Alloc(arena, 0)
    p1, g1, m1, v1 = (al.put(t) for t in ops[:4])
    p2, g2, m2, v2, e2 = (al.put(t) for t in ops)
    q1 = al.put(torch.zeros(n, dtype=torch.bfloat16))
    q2 = _Alloc(arena, off16).put(torch.zeros(n, dtype=torch.bfloat16))
    assert all(t.data_ptr() % 16 == 0 for t in (p2, g2, m2, v2, e2)) and q2.data_ptr() % 8 == 2 * off16
    hl.adam_wd(p1, g1, m1, v1, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], p16=q1)
    hl.adam_wd_ema(p2, g2, m2, v2, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], e2, 0.125, p16=q2)
    assert torch.equal(p1, p2) and torch.equal(m1, m2) and torch.equal(v1, v2) and torch.equal(q1.view(torch.int16), q2.view(torch.int16))
    e64 = ops[4].double() + 0.125 * (p2.cpu().double() - ops[4].double())
    M = max(float(p2.abs().max()), float(ops[4].abs().max()), float(e2.abs().max()))
    assert float((e2.cpu().double() - e64).abs().max()) <= ULP22 * M
    arena.check()


def test_binding_refuses_buffers_of_another_size(hl):
    p, g, m, v, e = (t.cuda() for t in _operands(64, 1))
    with pytest.raises(hl.McgError):
        hl.adam_wd_ema(p, g, m, v, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], e[:63], 0.5)
    with pytest.raises(hl.McgError):
        hl.adam_wd_ema(p, g, m[:32], v, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], e, 0.5)


RATES = [('D=0.5', schedule(0.5, 8)), ('D=0.999', schedule(0.999, 8)), ('r=1e-3', [1e-3] * 8)]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name,rates", RATES, ids=[r[0] for r in RATES])
def test_average_against_float64(hl, arena, name, rates, offset):
    n = 1027
    a = _alloc(arena, n, offset)
    p, g, m, v, e = (a.put(t) for t in _operands(n, 11))
    e64 = e.cpu().double()
    M = float(e.abs().max())
    gen = torch.Generator().manual_seed(12)
    worst = 0.0
    for s, r in enumerate(rates, 1):
        g.copy_(torch.randn(n, generator=gen) * 1e-2)
        hl.adam_wd_ema(p, g, m, v, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], e, r)
        r32 = float(np.float32(r))                                       # the float actually passed
        x = p.cpu().double()
        e64 = x.clone() if r32 == 1.0 else e64 + r32 * (x - e64)
        M = max(M, float(x.abs().max()), float(e.abs().max()))
        err = float((e.cpu().double() - e64).abs().max())
        worst = max(worst, err / (s * ULP22 * M))
        assert err <= s * ULP22 * M, (name, s, err, s * ULP22 * M)
    print('%s offset %d: worst |e - e64| / bound = %.3f' % (name, offset, worst))
    a.arena.check()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [5, 1027])
def test_rate_one_stores_the_parameter_itself(hl, arena, n, offset):
    a = _alloc(arena, n, offset)
    p, g, m, v, e = (a.put(t) for t in _operands(n, 21))
    e.mul_(1e3)                                                          # (e + (x - e) would lose x's low bits)
    hl.adam_wd_ema(p, g, m, v, ADAM['lr_t'], ADAM['beta1'], ADAM['beta2'], ADAM['eps'], ADAM['wd'], e, 1.0)
    assert torch.equal(e.view(torch.int32), p.view(torch.int32))
    a.arena.check()


def _grad_sums(W, n=10007, steps=3, seed=9):
    """p0 and, per step, the fp32 SUM of W gradients drawn as tests/test_gpu_ops.py::test_adam_weight_decay draws its one"""
    rng = np.random.RandomState(seed + W)
    p0 = rng.randn(n).astype(np.float32)
    sums = []
    for _ in range(steps):
        acc = np.zeros(n, np.float32)
        for _ in range(W):
            acc += (rng.randn(n) * 10.0 ** rng.uniform(-9, 0, n)).astype(np.float32)
        sums.append(acc)
    return p0, sums


def _oracle_adam():
    from oracle import updater as oupd
    lr = lambda t: oupd.ADAM_ALPHA * np.sqrt(1 - oupd.ADAM_BETA2 ** t) / (1 - oupd.ADAM_BETA1 ** t)
    return oupd, lr, (oupd.ADAM_BETA1, oupd.ADAM_BETA2, oupd.ADAM_EPS, oupd.WEIGHT_DECAY)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_fused_kernel_grad_scale_against_float64(hl, arena, W, offset):
    """adam_wd_ema(grad_scale = 1 / W) on the fp32 sum of W gradients against the oracle's Adam in float64 on g_sum / W, on aligned
    pointers (the 16-byte kernel) and one float past them (the scalar kernel): p to 1e-6 absolute, m and v to rel-L2 1e-6 (the
    bounds of tests/test_gpu_ops.py::test_adam_grad_scale_against_float64, where they are derived)."""
    oupd, lr, consts = _oracle_adam()
    p0, sums = _grad_sums(W)
    n = len(p0)
    arena.reset()
    a = _Alloc(arena, offset)
    p, m, v, e, g = (a.put(torch.as_tensor(t)) for t in (p0, np.zeros(n, np.float32), np.zeros(n, np.float32), p0, np.zeros(n, np.float32)))
    p64 = {'x/W': p0.astype(np.float64)}
    st = oupd.new_adam_state(p64)
    for t, g_sum in enumerate(sums, 1):
        oupd.adam_wd_update(p64, {'x/W': g_sum.astype(np.float64) / W}, st)
        g.copy_(torch.as_tensor(g_sum))
        hl.adam_wd_ema(p, g, m, v, lr(t), *consts, e, 0.25, grad_scale=1.0 / W)
        e_p = float(np.abs(p.cpu().double().numpy() - p64['x/W']).max())
        e_m, e_v = rel_l2(m, torch.as_tensor(st['m']['x/W'])), rel_l2(v, torch.as_tensor(st['v']['x/W']))
        print("PARITY adam_wd_ema W=%d offset %d step %d: max |p - p64| %.2e (1e-6), m %.2e, v %.2e (rel-L2, 1e-6)" % (W, offset, t, e_p, e_m, e_v))
        assert e_p < 1e-6 and e_m < 1e-6 and e_v < 1e-6, (t, e_p, e_m, e_v)
    arena.check()


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("W", [2, 8])
def test_fused_kernel_grad_scale_equals_scaling_the_gradient(hl, arena, W, offset):
    """grad_scale = 1 / W on g_sum and grad_scale = 1 on g_sum / W (exact: a power of two, nothing near the subnormal range) write
    the same p, m, v, bf16 copy and average, bit for bit"""
    _, lr, consts = _oracle_adam()
    p0, sums = _grad_sums(W)
    n = len(p0)
    arena.reset()
    a = _Alloc(arena, offset)
    zero = torch.zeros(n)
    mk = lambda: [a.put(torch.as_tensor(p0)), a.put(zero), a.put(zero), a.put(torch.as_tensor(p0) * 0.5), a.put(torch.zeros(n, dtype=torch.bfloat16)),
                  a.put(zero)]
    x, y = mk(), mk()                                                      # p, m, v, average, bf16 copy, gradient
    for t, g_sum in enumerate(sums, 1):
        scaled = g_sum / np.float32(W)
        assert np.array_equal(scaled * np.float32(W), g_sum) and np.abs(scaled[scaled != 0]).min() > 1e-30
        x[5].copy_(torch.as_tensor(g_sum)), y[5].copy_(torch.as_tensor(scaled))
        hl.adam_wd_ema(x[0], x[5], x[1], x[2], lr(t), *consts, x[3], 0.25, grad_scale=1.0 / W, p16=x[4])
        hl.adam_wd_ema(y[0], y[5], y[1], y[2], lr(t), *consts, y[3], 0.25, grad_scale=1.0, p16=y[4])
        for name, u, w in zip(("p", "m", "v", "average", "p16"), x, y):
            assert torch.equal(u.view(torch.int32 if u.dtype == torch.float32 else torch.int16),
                               w.view(torch.int32 if w.dtype == torch.float32 else torch.int16)), (name, t)
    assert not torch.equal(x[0].cpu(), torch.as_tensor(p0))
    arena.check()


def _segments(buf_src, buf_dst, sizes, gap=3):
    """(src, dst) views of the given sizes at ODD float offsets of two buffers, `gap` (or gap + 1) floats apart"""
    pairs, off = [], 1
    for n in sizes:
        pairs.append((buf_src[off:off + n], buf_dst[off:off + n]))
        off += n + gap
        off += 1 - off % 2                                               # the next one starts at an odd offset again
    assert off <= buf_src.numel()
    return pairs


SENTINEL = 12345.0


def _check_multi(hl, pairs, buf_dst, rates, seed):
    gen = torch.Generator().manual_seed(seed)
    covered = torch.zeros(buf_dst.numel(), dtype=torch.bool, device='cuda')
    base = buf_dst.data_ptr()
    for _, d in pairs:
        d.copy_(torch.randn(d.numel(), generator=gen))
        o = (d.data_ptr() - base) // 4
        assert o % 2 == 1
        covered[o:o + d.numel()] = True
    e64 = [d.cpu().double() for _, d in pairs]
    M = [float(d.abs().max()) for _, d in pairs]
    for s, r in enumerate(rates, 1):
        for src, _ in pairs:
            src.copy_(torch.randn(src.numel(), generator=gen) * 2.0)
        hl.ema_multi(pairs, r)
        r32 = float(np.float32(r))
        for i, (src, dst) in enumerate(pairs):
            x = src.cpu().double()
            e64[i] = x.clone() if r32 == 1.0 else e64[i] + r32 * (x - e64[i])
            M[i] = max(M[i], float(x.abs().max()), float(dst.abs().max()))
            err = float((dst.cpu().double() - e64[i]).abs().max())
            assert err <= s * ULP22 * M[i], (i, dst.numel(), s, err, s * ULP22 * M[i])
    assert bool((buf_dst[~covered] == SENTINEL).all()), "a store between two segments"


def test_ema_multi_segments_at_odd_offsets(hl, arena):
    arena.reset()
    sizes = [1, 8, 16, 33, 512, 4099]
    total = sum(sizes) + 8 * len(sizes)
    buf_src, buf_dst = arena.full((total,), 0.0), arena.full((total,), SENTINEL)
    pairs = _segments(buf_src, buf_dst, sizes)
    _check_multi(hl, pairs, buf_dst, schedule(0.5, 8), 31)
    arena.check()
    hl.ema_multi(pairs, 1.0)                                             # rate 1: the source itself
    assert all(torch.equal(s.view(torch.int32), d.view(torch.int32)) for s, d in pairs)
    arena.check()


def test_ema_multi_takes_exactly_32_segments(hl):
    sizes = [1 + 37 * i for i in range(31)] + [40001]                    # (the last one is longer than its blocks cover in one sweep)
    total = sum(sizes) + 8 * len(sizes)
    buf_src = torch.zeros(total, device='cuda')
    buf_dst = torch.full((total,), SENTINEL, device='cuda')
    pairs = _segments(buf_src, buf_dst, sizes)
    assert len(pairs) == 32
    _check_multi(hl, pairs, buf_dst, [0.9, 0.82, 1e-3], 32)
    with pytest.raises(hl.McgError):
        hl.ema_multi(pairs + pairs[:1], 0.5)


# ------------------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------------------
def _clips(n, seed):
    rng = np.random.RandomState(seed)
    x = torch.tensor(rng.uniform(-1, 1, (n, 3, 16, 64, 64)), dtype=torch.float32, device='cuda')
    t = torch.tensor(rng.randint(0, 6, n), dtype=torch.int32, device='cuda')
    return x, t


@pytest.mark.parametrize("model", ['normal', 'infogan'])
def test_average_tracks_the_training_step(hl, model):
    """three iterations with D = 0.5: after each, the averaged parameters (every Chainer key) and the averaged running statistics
    equal the float64 recurrence fed with the device's parameters and statistics"""
    import mocogan_chainer_amd.step as step
    gen, di, dv = step.make_models(model, num_labels=6, n_filters=8, seed=3)
    ts = step.TrainStep(model, gen, di, dv, seed=1, ema_decay=0.5)
    ema = gen.ema
    assert ema.k == 0 and di.ema is None and dv.ema is None
    keys = [k for k in gen.ref_shapes if not k.endswith('/N')]
    e64 = {k: np.asarray(v, np.float64) for k, v in ema.export_reference_params().items() if k in keys}
    live0 = gen.export_reference_params()
    assert all(np.array_equal(e64[k], live0[k]) for k in keys)          # enabled: the live values
    M = {k: float(np.abs(e64[k]).max()) for k in keys}
    n = 3
    for s in range(1, 4):
        r32 = float(np.float32(step.ema_rate(0.5, s - 1)))
        ts.run(*_clips(n, 40 + s))
        torch.cuda.synchronize()
        assert ema.k == s and gen.t == s
        live, avg = gen.export_reference_params(), ema.export_reference_params()
        assert list(avg) == list(live)
        moved = 0
        for k in keys:
            x = np.asarray(live[k], np.float64)
            e64[k] = e64[k] + r32 * (x - e64[k])
            M[k] = max(M[k], float(np.abs(x).max()), float(np.abs(avg[k]).max()))
            err = float(np.abs(avg[k].astype(np.float64) - e64[k]).max())
            assert err <= s * ULP22 * M[k], (k, s, err, s * ULP22 * M[k])
            moved += int(not np.array_equal(avg[k], live[k]))
        assert moved > len(keys) // 2                                     # (an average, not a second name for the parameters)
        for k in live:
            if k.endswith('/N'):
                assert int(avg[k]) == int(live[k]) == s
    assert set(k for k in keys if k.endswith(('avg_mean', 'avg_var'))) == set(gen.running)


def _updater(precision, seed=0, batch=4, ema_decay=0.5):
    from model.net import ImageGenerator, ImageDiscriminator, VideoDiscriminator
    from model.updater import Updater
    from datasets import SyntheticDataset
    from mocogan_chainer_amd import trainer as T
    np.random.seed(seed)
    g, di, dv = ImageGenerator(dim_zl=6, n_filters=8), ImageDiscriminator(3, 1, 8, True, 0.2), VideoDiscriminator(3, 1, 8, True, 0.2)
    opts = {}
    for name, link in (('image_gen', g), ('image_dis', di), ('video_dis', dv)):
        o = T.Adam(alpha=2e-4, beta1=5e-5)
        o.setup(link)
        o.add_hook(T.WeightDecay(1e-5), 'hook_dec')
        opts[name] = o
    it = T.SerialIterator(SyntheticDataset(8, 6), batch)
    return Updater(model='normal', models=(g, di, dv), video_length=16, img_size=64, channel=3, dim_zl=6, tensorboard_writer=T.NullWriter(),
                   iterator=it, optimizer=opts, device=0, precision=precision, ema_decay=ema_decay)


def rel_l2(a, b):
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize("precision", ['f32', 'f32x3', 'bf16'])
def test_nothing_derived_from_the_average_goes_stale(hl, precision, tmp_path):
    """sample (folded BatchNorm, bf16 shadow, split filters) and test-mode __call__ (the bf16 copy of the weights, the versioned
    split filters) from the averaged generator, one more iteration, the same again: what comes out is what a fresh generator
    loaded from the averaged generator's npz gives, and not what came out before"""
    from model.net import ImageGenerator, config
    from mocogan_chainer_amd import trainer as T
    u = _updater(precision)
    u.update()
    ema = u.image_gen.ema
    n = 3
    rng = np.random.RandomState(5)
    lat = dict(labels=rng.randint(0, 6, n), zc=rng.normal(0, 0.33, (n, 50)), h0=rng.normal(0, 0.33, (n, 10)), e=rng.normal(0, 0.33, (16, n, 10)))

    def outputs(g):
        x, _ = g.sample(n, **lat)
        b, _ = g.sample(n, as_uint8=True, **lat)
        config.train = False
        try:
            np.random.seed(77)
            y, _ = g(n)
        finally:
            config.train = True
        return x.clone(), b.clone(), y.clone()
    x1, b1, y1 = outputs(ema)
    u.update()
    x2, b2, y2 = outputs(ema)
    T.save_npz(tmp_path / 'ema.npz', ema)
    fresh = ImageGenerator(dim_zl=6, n_filters=8)
    T.load_npz(tmp_path / 'ema.npz', fresh)
    fresh.impl.set_precision(precision)
    x3, b3, y3 = outputs(fresh)
    assert rel_l2(x2, x3) < 1e-6 and rel_l2(y2, y3) < 1e-6
    d = (b2.cpu().numpy().astype(np.int64) - b3.cpu().numpy().astype(np.int64))
    v = (x3.cpu().double().numpy() / 2. + 0.5) * 255
    near = np.abs(v - np.rint(v)) <= 127.5 * 4e-6
    assert np.abs(d).max() <= 1 and (d[~near] == 0).all()
    # the test's power: one iteration moves the average (rates 0.9, 0.82) by far more than the tolerance
    assert rel_l2(x1, x2) > 1e-4 and rel_l2(y1, y2) > 1e-4
    d12 = np.abs(b1.cpu().numpy().astype(np.int64) - b2.cpu().numpy().astype(np.int64))
    assert (d12[~near] != 0).any()
    # ... and the averaged generator is not the live one
    x_live, _ = u.image_gen.sample(n, **lat)
    assert rel_l2(x_live, x2) > 1e-4
    with pytest.raises(hl.McgError):
        ema(n)                                                           # (train mode: the averaged generator has no batch statistics)


def test_train_and_generate_entry_points_with_the_averaged_generator(hl, tmp_path, monkeypatch):
    import train
    import generate_samples
    monkeypatch.chdir(tmp_path)
    common = ['--dataset_type', 'synthetic', '--synthetic_size', '8', '--batchsize', '4', '--max_epoch', '2', '--n_filters_gen', '8',
              '--snapshot_interval', '1', '--log_tensorboard_interval', '100', '--num_gen_samples', '4']
    try:
        tr = train.main(common + ['--save_name', 'avg', '--ema_decay', '0.99'])
        out = tmp_path / 'result' / 'avg'
        assert tr.updater.iteration == 4 and tr.updater.image_gen.ema is not None and tr.updater.image_gen.impl.ema.k == 4
        for f in ('image_gen_ema_epoch_1.npz', 'image_gen_ema_epoch_2.npz', 'image_gen_ema_epoch_fianl.npz', 'image_gen_epoch_fianl.npz'):
            assert (out / f).exists(), f
        with np.load(out / 'image_gen_epoch_fianl.npz') as f:
            live = {k: f[k] for k in f.files}
        for name in ('image_gen_ema_epoch_2.npz', 'image_gen_ema_epoch_fianl.npz'):
            with np.load(out / name) as f:
                avg = {k: f[k] for k in f.files}
            assert set(avg) == set(live) and all(avg[k].shape == live[k].shape for k in live)
            assert not np.array_equal(avg['dc3/W'], live['dc3/W']) and not np.array_equal(avg['bn2/avg_var'], live['bn2/avg_var'])
        with np.load(out / 'snapshot_epoch_2.npz') as f:
            assert 'updater/ema:image_gen/k' in f.files and int(f['updater/ema:image_gen/k']) == 4
            assert np.array_equal(f['updater/ema:image_gen/dc3/W'], avg['dc3/W'])
        generate_samples.main([str(out / 'image_gen_ema_epoch_fianl.npz'), str(tmp_path / 'samples'), '--num', '4', '--dim_zl', '6',
                               '--n_filters', '8', '--test_mode', '1', '--seed', '3'])
        assert len(sorted((tmp_path / 'samples' / 'grid').glob('*.jpg'))) == 16
        # without the flag: the files and keys of before
        tr = train.main(common + ['--save_name', 'plain'])
        plain = tmp_path / 'result' / 'plain'
        assert tr.updater.image_gen.ema is None and tr.updater.image_gen.impl.fp.e is None
        assert (plain / 'image_gen_epoch_fianl.npz').exists() and not list(plain.glob('*ema*'))
        with np.load(plain / 'snapshot_epoch_2.npz') as f:
            assert not [k for k in f.files if 'ema' in k]
        assert sorted(p.name for p in plain.iterdir()) == sorted(p.name for p in out.iterdir() if 'ema' not in p.name)
    finally:
        hl.reset_tuning()                                                # (main() switched the tile tuner on with the shipped table)
