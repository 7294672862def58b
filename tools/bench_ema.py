#!/usr/bin/env python
"""What the averaged generator costs, on one MI355X.

    python tools/bench_ema.py [--rounds 5]     mcg_adam_wd against mcg_adam_wd_ema at the generator's real flat size

The two kernels alternate in one process, `--rounds` times each after a warm-up, timed with HIP events; one line per measurement
plus a summary: a difference counts only against the spread of a variant's own repeats.  Every launch works on another of `--sets`
buffer sets (together larger than the 256 MB Infinity Cache), so that the streams come from HBM as they do inside a training
step; the time is reported as a fraction of bytes / 6.3 TB/s (28 B per parameter for mcg_adam_wd: p, g, m, v in, p, m, v out;
36 B with the average).  The step time is tools/bench_train.py's to measure (--ema_decay 0 against 0.999)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl
import mocogan_chainer_amd.step as step

HBM_TBS = 6.3
ADAM = (2e-4, 5e-5, 0.999, 1e-8, 1e-5)


def events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(v):
    return '%.3f (min %.3f, max %.3f, n %d)' % (statistics.median(v), min(v), max(v), len(v))


def kernel(args):
    gen = step.make_models('normal', num_labels=6, n_filters=64)[0]
    n = gen.fp.size
    del gen
    sets = [[torch.randn(n, device='cuda') * s for s in (0.05, 1e-2, 1e-2, 0.0, 0.05)] for _ in range(args.sets)]
    for s in sets:
        s[3].uniform_(0, 1e-4)                                          # v >= 0
    print('n = %d parameters (%.1f MB per stream), %d buffer sets of 5 streams (%.0f MB)' % (n, 4e-6 * n, args.sets, 20e-6 * n * args.sets))

    def plain(i):
        p, g, m, v, _ = sets[i % len(sets)]
        hl.adam_wd(p, g, m, v, *ADAM)

    def fused(i):
        p, g, m, v, e = sets[i % len(sets)]
        hl.adam_wd_ema(p, g, m, v, *ADAM, e, 1e-3)
    variants = (('adam_wd', plain, 28), ('adam_wd_ema', fused, 36))
    for _, fn, _ in variants:
        events_ms(fn, 3 * len(sets))
    got = {name: [] for name, _, _ in variants}
    for r in range(args.rounds):
        for name, fn, b in variants:
            ms = events_ms(fn, args.iters)
            got[name].append(ms * 1e3)
            floor = b * n / (HBM_TBS * 1e12) * 1e6
            print('round %d  %-12s %8.2f us   bytes / 6.3 TB/s = %6.2f us   fraction of that bound reached %.2f' % (r, name, ms * 1e3, floor, floor / (ms * 1e3)))
    for name, _, b in variants:
        print('%-12s us per launch: %s' % (name, spread(got[name])))
    print('difference of the medians: %.2f us' % (statistics.median(got['adam_wd_ema']) - statistics.median(got['adam_wd'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--sets', type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ema.py needs an MI355X')
    hl.load()
    kernel(args)


if __name__ == '__main__':
    main()
