"""The NumPy statement of mcg_grad_stats and of the clipped Adam update (include/mocogan_hip.h) that the GPU tests compare with.

Sums of squares are math.fsum of EXACT squares: the square of an fp32 value has at most 48 significant bits, so it is exact in
float64, and fsum returns the correctly rounded sum of its addends -- the reference has no summation order.  The control block is
formed in float64 and rounded to fp32 once per entry, as the finalize launch does."""
import math

import numpy as np

from oracle import updater as oupd

F32, F64 = np.float32, np.float64


def segment_stats(x):
    """(sum of squares, max |x|, non-finite count) of a float32 array; non-finite elements are counted and left out of both others"""
    x = np.asarray(x)
    assert x.dtype == F32
    fin = np.isfinite(x)
    v = x[fin].astype(F64)
    return math.fsum((v * v).tolist()), float(np.abs(v).max()) if v.size else 0.0, int(x.size - fin.sum())


def stats_rows(g, segs):
    """[(offset, n), ...] over the flat float32 gradient g -> float64 [(nseg + 1)][4], the total last: the sums added in segment
    order (plain float64 additions, as the device adds them), the largest maximum, the counts added"""
    rows = np.zeros((len(segs) + 1, 4), F64)
    for i, (off, n) in enumerate(segs):
        rows[i, :3] = segment_stats(g[off:off + n])
    tot = 0.0
    for i in range(len(segs)):
        tot = tot + rows[i, 0]
    rows[-1, :3] = tot, rows[:-1, 1].max(), rows[:-1, 2].sum()
    return rows


def total_row(rows):
    """the total row that belongs to the given segment rows (what the device must have formed from ITS segment rows)"""
    tot = 0.0
    for v in rows[:, 0]:
        tot = tot + float(v)
    return np.array([tot, rows[:, 1].max(), rows[:, 2].sum(), 0.0], F64)


def control(total_sumsq, nonfinite, grad_scale, threshold, peak=0.0, skipped=0.0):
    """ctl[0..5] after one call, float64 throughout except the final roundings; peak / skipped: ctl[4] / ctl[5] before the call"""
    bad = nonfinite > 0
    norm = grad_scale * math.sqrt(total_sumsq)
    rate = 1.0 if norm == 0.0 else min(1.0, threshold / norm)
    f = lambda v: float(F32(v))
    c3 = f(norm)
    return [f(grad_scale) if bad else f(grad_scale * rate), 1.0 if bad else 0.0, f(rate), c3,
            peak if (bad or not math.isfinite(c3)) else max(peak, c3), skipped + (1.0 if bad else 0.0)]


def clip_rate(grads, threshold, grad_scale=1.0):
    """min(1, T / ||grad_scale * g||_2) over ALL arrays of the dict, in float64 (chainer.optimizer.GradientClipping); 1 for a zero norm"""
    norm = grad_scale * math.sqrt(math.fsum(float(np.sum(np.asarray(v, F64) ** 2)) for v in grads.values()))
    return (1.0 if norm == 0.0 else min(1.0, threshold / norm)), norm


def clipped_adam_step(p, g, state, threshold, grad_scale=1.0):
    """float64: scale the gradient by grad_scale * rate, then oracle.updater.adam_wd_update (weight decay acts AFTER the clipping).
    p, state: updated in place; g: {key: float64 array}, left alone.  Returns (rate, norm)."""
    rate, norm = clip_rate(g, threshold, grad_scale)
    oupd.adam_wd_update(p, {k: np.asarray(v, F64) * (grad_scale * rate) for k, v in g.items()}, state)
    return rate, norm


def clipping_reduce(thresholds, seen=None):
    """oracle.updater.update_core's `reduce=` callable: every network's gradients are scaled IN PLACE by min(1, T / norm), T =
    thresholds[network] (None / missing: no clipping).  seen (a dict): gets {network: (rate, norm)} of the un-clipped gradient."""
    def reduce(name, grads):
        keys = [k for k in grads if k.endswith(('/W', '/b', '/gamma', '/beta'))]
        t = thresholds.get(name)
        rate, norm = clip_rate({k: grads[k] for k in keys}, math.inf if t is None else t)
        if seen is not None:
            seen[name] = (rate, norm)
        if rate < 1.0:
            for k in keys:
                grads[k] *= rate
    return reduce
