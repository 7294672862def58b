#!/usr/bin/env python
"""What the geometric augmentation's passes cost, on one MI355X.

    python tools/bench_warp.py [--rounds 5]

mcg_warp_fwd and mcg_warp_bwd on 32 and on 256 full clips (16 x 64 x 64 x 4 floats each) with drawn matrices of the full policy
and, for comparison, with identity matrices, beside a bn_act_fwd(ACT_NONE) copy of the same tensor -- the yardstick of
tools/bench_augment.py -- alternating in one process, `--rounds` times each after a warm-up, timed with HIP events.  Every launch
works on another of `--sets` buffer pairs.  Reported as microseconds per call and as a ratio to the copy's time; and the mean
number of candidate output pixels the backward gather visits per source pixel (the bounding box of include/mocogan_hip.h, restated
here in NumPy).  The step time is tools/bench_train.py's to measure (--warp)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl


def events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(v):
    return '%.2f (min %.2f, max %.2f, n %d)' % (statistics.median(v), min(v), max(v), len(v))


def mean_candidates(mat, H, W):
    """the backward kernel's bounding box, per source pixel: (x_hi - x_lo + 1) (y_hi - y_lo + 1), averaged over clips and pixels"""
    m = np.asarray(mat, np.float64)
    total = 0.0
    cx, cy = (W - 1) / 2, (H - 1) / 2
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    for a, b, ox, c, d, oy in m[:, :6]:
        det = a * d - b * c
        with np.errstate(all='ignore'):
            i00, i01, i10, i11 = d / det, -b / det, -c / det, a / det
            ex, ey = abs(i00) + abs(i01), abs(i10) + abs(i11)
            mag = (abs(a) + abs(b) + abs(c) + abs(d)) * (H + W) + abs(cx + ox) + abs(cy + oy)
            whole = not abs(det) > 0 or not (ex + ey) * mag * 2.0 ** -21 < 0.5
        if whole:
            total += H * W * H * W
            continue
        du, dv = u - (cx + ox), v - (cy + oy)
        xo, yo = cx + i00 * du + i01 * dv, cy + i10 * du + i11 * dv
        x_lo, x_hi = np.clip(np.floor(xo - ex - 1), 0, W), np.clip(np.ceil(xo + ex + 1), -1, W - 1)
        y_lo, y_hi = np.clip(np.floor(yo - ey - 1), 0, H), np.clip(np.ceil(yo + ey + 1), -1, H - 1)
        total += float((np.maximum(x_hi - x_lo + 1, 0) * np.maximum(y_hi - y_lo + 1, 0)).sum())
    return total / (len(m) * H * W)


def measure(n, args):
    T, H, W = 16, 64, 64
    sets = max(2, min(args.sets, (1 << 30) // (n * T * H * W * 16 * 2)))
    bufs = [(torch.rand((n, T, H, W, 4), device='cuda') * 2 - 1, torch.empty((n, T, H, W, 4), device='cuda')) for _ in range(sets)]
    for x, _ in bufs:
        x[..., 3] = 0
    drawn = hl.warp_draw(n, H, W, 15, 1, 44, device='cuda')
    ident = hl.warp_draw(n, H, W, 0, 1, 44, device='cuda')
    one_pass = n * T * H * W * 16
    rows = n * T * H * W
    print('%d clips: %.1f MB per pass, %d buffer pairs (%.0f MB); candidates per source pixel: drawn %.1f, identity %.1f' % (
        n, one_pass * 1e-6, sets, 2e-6 * one_pass * sets, mean_candidates(drawn.cpu().numpy(), H, W), mean_candidates(ident.cpu().numpy(), H, W)))

    def copy(i):
        x, o = bufs[i % sets]
        hl.bn_act_fwd(rows, 4, x, None, hl.ACT_NONE, o, c_valid=3)

    def call(fn, mat):
        def run(i):
            x, o = bufs[i % sets]
            fn(x, 3, mat, o)
        return run
    variants = (('copy', copy), ('warp_fwd drawn', call(hl.warp_fwd, drawn)), ('warp_bwd drawn', call(hl.warp_bwd, drawn)),
                ('warp_fwd identity', call(hl.warp_fwd, ident)), ('warp_bwd identity', call(hl.warp_bwd, ident)))
    for _, fn in variants:
        events_ms(fn, 3 * sets)
    us = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, fn in variants:
            t = events_ms(fn, args.iters) * 1e3
            us[name].append(t)
            print('round %d  n %3d  %-18s %8.2f us' % (r, n, name, t))
    base = statistics.median(us['copy'])
    for name, _ in variants:
        print('n %3d  %-18s us per call: %s   %.2f x the copy' % (n, name, spread(us[name]), statistics.median(us[name]) / base))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--sets', type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_warp.py needs an MI355X')
    hl.load()
    for n in (32, 256):
        measure(n, args)


if __name__ == '__main__':
    main()
