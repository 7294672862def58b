#!/usr/bin/env python
"""What the differentiable augmentation's passes cost, on one MI355X.

    python tools/bench_augment.py [--rounds 5]

mcg_augment_fwd and mcg_augment_bwd on 32 and on 256 full clips (16 x 64 x 64 x 4 floats each, drawn parameters, full policy)
beside a bn_act_fwd(ACT_NONE) copy of the same tensor -- the form in which the discriminators' first launches read the clips --
alternating in one process, `--rounds` times each after a warm-up, timed with HIP events.  Every launch works on another of
`--sets` buffer pairs (together larger than the 256 MB Infinity Cache at 256 clips).  Bytes counted per launch: the copy reads
and writes the tensor once (2 passes); an augmentation call reads it twice and writes it once (3 passes).  Reported as
bytes / time and as a fraction of the copy's rate.  The step time is tools/bench_train.py's to measure (--augment)."""
import argparse
import os
import statistics
import sys

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


def measure(n, args):
    T, H, W = 16, 64, 64
    sets = max(2, min(args.sets, (1 << 30) // (n * T * H * W * 16 * 2)))
    bufs = [(torch.rand((n, T, H, W, 4), device='cuda') * 2 - 1, torch.empty((n, T, H, W, 4), device='cuda')) for _ in range(sets)]
    for x, _ in bufs:
        x[..., 3] = 0
    geo, col = hl.augment_draw(n, H, W, 7, 1, 40, device='cuda')
    ws = hl.augment_workspace(n, 'cuda')
    one_pass = n * T * H * W * 16
    rows = n * T * H * W
    print('%d clips: %.1f MB per pass, %d buffer pairs (%.0f MB)' % (n, one_pass * 1e-6, sets, 2e-6 * one_pass * sets))

    def copy(i):
        x, o = bufs[i % sets]
        hl.bn_act_fwd(rows, 4, x, None, hl.ACT_NONE, o, c_valid=3)

    def fwd(i):
        x, o = bufs[i % sets]
        hl.augment_fwd(x, 3, geo, col, ws, o)

    def bwd(i):
        x, o = bufs[i % sets]
        hl.augment_bwd(x, 3, geo, col, ws, o)
    variants = (('copy', copy, 2), ('augment_fwd', fwd, 3), ('augment_bwd', bwd, 3))
    for _, fn, _ in variants:
        events_ms(fn, 3 * sets)
    us = {name: [] for name, _, _ in variants}
    for r in range(args.rounds):
        for name, fn, passes in variants:
            t = events_ms(fn, args.iters) * 1e3
            us[name].append(t)
            print('round %d  n %3d  %-12s %8.2f us   %5.2f TB/s' % (r, n, name, t, passes * one_pass / t * 1e-6))
    rate = {name: passes * one_pass / statistics.median(us[name]) * 1e-6 for name, _, passes in variants}
    for name, _, passes in variants:
        print('n %3d  %-12s us per call: %s   %5.2f TB/s = %.2f of the copy\'s rate' % (n, name, spread(us[name]), rate[name], rate[name] / rate['copy']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--sets', type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_augment.py needs an MI355X')
    hl.load()
    for n in (32, 256):
        measure(n, args)


if __name__ == '__main__':
    main()
