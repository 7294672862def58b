"""The losses (mcg_loss_dis / mcg_loss_gen) in the guard arena, laid out as the training step lays them out.

The step hands the one-block loss kernels views into shared tensors: the loss word is one float BETWEEN two other loss words, the two
logit tensors are the halves of one tensor and so are the two gradients.  Here the loss word is element 1 of a 3-float arena tensor
filled with sentinels, the gradients are the halves g[:N], g[N:] of one poisoned (2N, C) arena tensor, and everything else the launch
reads is carved from the same arena.  Cases (N, C, with_ce): one sample; one class (C = 2: the cross entropy and its gradient are
exactly 0); class columns with the cross entropy off; N C = 256 / 257 / 259, the edge of both loops' first trip; C = 127, the GRU's widest label; N = 257 and 300, a second
trip of the per-row loop.  Checked against oracle.updater in float64 with the bounds of test_losses_at_saturated_logits (loss within
1e-5 max(1, |ref|), every gradient element within 1e-5 / N):
  * every gradient element is written, zeros included (no poison left); without the cross entropy the positions outside the GAN term
    are exactly 0.0; for C = 2 the cross entropy adds exactly nothing: the loss and row 0 are bit-equal to the launch without it,
    every other class-column element is exactly 0;
  * the loss word's neighbours, the inputs and the arena's margins are unchanged; a second launch is bit-identical.
Refused argument sets leave every output as poison.  Measured on an MI355X: profiles/fc_loss_parity.md."""
import numpy as np
import pytest
import torch

from oracle import updater as oupd
from guard import Arena, POISON

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 0), (1, 2, 1), (256, 1, 0), (257, 1, 0), (37, 7, 1), (32, 8, 1), (3, 127, 1), (257, 2, 1), (300, 127, 1),
         (37, 7, 0)]      # class columns without the cross entropy (the image discriminator of an infogan step): zeros that only this launch writes
SENTINELS = (12345.0, -777.0, 4321.0)


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return Arena(16 << 20)


def _words(t):
    return t.reshape(-1).view(torch.int32)


def _bit_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_words(a), _words(b))


def _is_poison(t):
    return bool((_words(t) == POISON).all())


def _labels(rng, N, C):
    """labels in [0, C-2] that include both ends (one sample: the only label a single class has, else the last)"""
    hi = max(C - 2, 0)
    t = rng.randint(0, hi + 1, N)
    t[0], t[-1] = 0, hi
    return t.astype(np.int32)


def _layout(arena, N, C, ya, yb, ta, tb):
    """the step's layout: logits as halves of one tensor, the loss word between two others, gradients as halves of one tensor"""
    arena.reset()
    y = arena.put(torch.from_numpy(np.concatenate([ya, yb]).astype(np.float32)))
    ta_d, tb_d = arena.put(torch.from_numpy(ta)), arena.put(torch.from_numpy(tb))
    loss3 = arena.put(torch.tensor(SENTINELS))
    g = arena.empty((2 * N, C))
    return y, ta_d, tb_d, loss3, g


def _launch_and_check(tag, arena, launch, N, C, with_ce, ins, loss3, g, refs):
    """launch(loss word, g_a, g_b) -> the figures, then the assertions; returns (loss word, gradients) of the first launch"""
    snaps = [t.clone() for t in ins]
    launch(loss3[1:2], g[:N], g[N:])
    arena.check()
    loss1, g1 = loss3.clone(), g.clone()
    l_ref, ga_ref, gb_ref = refs
    g_ref = np.concatenate([ga_ref.reshape(N, C), gb_ref.reshape(N, C)])
    l, gd = float(loss1[1]), g1.cpu().double().numpy()
    written = not bool((_words(g1) == POISON).any())
    dl, dg = abs(l - l_ref) / max(1.0, abs(l_ref)), (np.abs(gd - g_ref).max() if np.isfinite(gd).all() else float('inf'))
    print("loss-guard %s N=%d C=%d ce=%d: loss %.9g ref %.9g, |d| / max(1, |ref|) %.2e; max |dg| * N %.2e" % (tag, N, C, with_ce, l, l_ref, dl, dg * N))
    assert written, "%s: %d gradient words were never written" % (tag, int((_words(g1) == POISON).sum()))
    assert np.isfinite(l) and np.isfinite(gd).all()
    assert abs(l - l_ref) <= 1e-5 * max(1.0, abs(l_ref))
    assert dg <= 1e-5 / N
    assert float(loss1[0]) == SENTINELS[0] and float(loss1[2]) == SENTINELS[2], "the loss word's neighbours were written"
    for i, (t, s) in enumerate(zip(ins, snaps)):
        assert _bit_equal(t, s), "%s: input %d was written" % (tag, i)
    # a second launch from the same starting state
    _words(g).fill_(POISON)
    loss3.copy_(torch.tensor(SENTINELS))
    launch(loss3[1:2], g[:N], g[N:])
    arena.check()
    assert _bit_equal(loss3, loss1) and _bit_equal(g, g1), "%s: a second launch differs" % tag
    return loss1[1:2].clone(), g1


@pytest.mark.parametrize("N,C,with_ce", CASES, ids=["N%d-C%d-ce%d" % c for c in CASES])
def test_loss_dis_in_the_step_layout(hl, arena, N, C, with_ce):
    rng = np.random.RandomState(100000 + 1000 * N + 10 * C + with_ce)
    yr, yf = (np.float32(3) * rng.randn(N, C).astype(np.float32) for _ in range(2))
    tr, tf = _labels(rng, N, C), _labels(rng, N, C)
    refs = oupd.loss_dis('infogan' if with_ce else 'normal', bool(with_ce), yr.astype(np.float64).reshape(N, C, 1, 1, 1),
                         yf.astype(np.float64).reshape(N, C, 1, 1, 1), tr, tf)
    y, tr_d, tf_d, loss3, g = _layout(arena, N, C, yr, yf, tr, tf)
    launch = lambda ce: (lambda lw, ga, gb: hl.loss_dis(N, C, y[:N], y[N:], tr_d, tf_d, ce, lw, ga, gb))
    l1, g1 = _launch_and_check("loss_dis", arena, launch(with_ce), N, C, with_ce, [y, tr_d, tf_d], loss3, g, refs)
    gan = torch.zeros((2 * N, C), dtype=torch.bool, device="cuda")
    gan[0], gan[N] = True, True                                      # sample 0 of each half, every column (model/updater.py:25-26)
    if not with_ce:
        assert bool((g1[~gan] == 0.0).all())
    if C == 2:                                                       # one class: softmax = 1 = the one-hot
        assert bool((g1[~gan] == 0.0).all())
        _words(g).fill_(POISON)
        hl.loss_dis(N, C, y[:N], y[N:], tr_d, tf_d, 0, loss3[1:2], g[:N], g[N:])
        arena.check()
        assert _bit_equal(loss3[1:2], l1) and _bit_equal(g, g1), "the cross entropy of one class is not exactly zero"


@pytest.mark.parametrize("N,C,with_ce", CASES, ids=["N%d-C%d-ce%d" % c for c in CASES])
def test_loss_gen_in_the_step_layout(hl, arena, N, C, with_ce):
    rng = np.random.RandomState(200000 + 1000 * N + 10 * C + with_ce)
    yi, yv = (np.float32(3) * rng.randn(N, C).astype(np.float32) for _ in range(2))
    tf = _labels(rng, N, C)
    refs = oupd.loss_gen('infogan' if with_ce else 'normal', yi.astype(np.float64).reshape(N, C, 1, 1),
                         yv.astype(np.float64).reshape(N, C, 1, 1, 1), tf)
    y, tf_d, _, loss3, g = _layout(arena, N, C, yi, yv, tf, tf)
    launch = lambda ce: (lambda lw, ga, gb: hl.loss_gen(N, C, y[:N], y[N:], tf_d, ce, lw, ga, gb))
    l1, g1 = _launch_and_check("loss_gen", arena, launch(with_ce), N, C, with_ce, [y, tf_d], loss3, g, refs)
    if not with_ce or C == 2:
        assert bool((g1[:, 1:] == 0.0).all())                        # channel 0 alone carries the GAN term (model/updater.py:50-51)
    if C == 2:
        _words(g).fill_(POISON)
        hl.loss_gen(N, C, y[:N], y[N:], tf_d, 0, loss3[1:2], g[:N], g[N:])
        arena.check()
        assert _bit_equal(loss3[1:2], l1) and _bit_equal(g, g1), "the cross entropy of one class is not exactly zero"


def test_refused_losses_leave_the_outputs_poison(hl, arena):
    """the cross entropy without a class column (C = 1) or without labels: MCG_ERR_BAD_ARG (the codes: tests/test_cabi_cpu.py), and
    neither the loss word nor a gradient word changes"""
    arena.reset()
    N = 5
    rng = np.random.RandomState(3)
    y1, y7 = (arena.put(torch.from_numpy(rng.randn(2 * N, c).astype(np.float32))) for c in (1, 7))
    t = arena.put(torch.from_numpy(_labels(rng, N, 7)))
    loss3, g1, g7 = arena.empty((3,)), arena.empty((2 * N, 1)), arena.empty((2 * N, 7))
    lw = loss3[1:2]
    calls = [lambda: hl.loss_dis(N, 1, y1[:N], y1[N:], t, t, 1, lw, g1[:N], g1[N:]),
             lambda: hl.loss_gen(N, 1, y1[:N], y1[N:], t, 1, lw, g1[:N], g1[N:]),
             lambda: hl.loss_dis(N, 7, y7[:N], y7[N:], None, t, 1, lw, g7[:N], g7[N:]),
             lambda: hl.loss_dis(N, 7, y7[:N], y7[N:], t, None, 1, lw, g7[:N], g7[N:]),
             lambda: hl.loss_gen(N, 7, y7[:N], y7[N:], None, 1, lw, g7[:N], g7[N:])]
    for call in calls:
        with pytest.raises(hl.McgError, match="MCG_ERR_BAD_ARG"):
            call()
    arena.check()
    assert _is_poison(loss3) and _is_poison(g1) and _is_poison(g7)
