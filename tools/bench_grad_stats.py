#!/usr/bin/env python
"""What the gradient statistics and the clipped update cost, on one MI355X.

    python tools/bench_grad_stats.py [--rounds 5]

  * mcg_grad_stats (both launches) over the flat gradient of each of the three networks at its real size and segment table
    (n_filters 64): 4 B per element read, reported against bytes / 6.3 TB/s;
  * mcg_adam_wd against mcg_adam_wd_ctl at the generator's size (28 B per parameter either way: p, g, m, v in, p, m, v out).

The variants alternate in one process, `--rounds` times each after a warm-up, timed with HIP events; one line per measurement plus
a summary: a difference counts only against the spread of a variant's own repeats.  Every launch works on another of `--sets`
buffer sets (together larger than the 256 MB Infinity Cache), so that the streams come from HBM as they do inside a training step.
The step time is tools/bench_train.py's to measure (--grad_stats 1, --grad_clip T)."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl
import mocogan_chainer_amd.nets as nets
import mocogan_chainer_amd.step as step

HBM_TBS = 6.3
ADAM = (2e-4, 5e-5, 0.999, 1e-8, 1e-5)


def events_ms(fn, iters):
    """-> (ms per call between two events on the stream, ms per call the HOST took to queue them): where the two are close the figure
    is the host's enqueue rate, not the kernels' time (those are then rocprofv3 --kernel-trace's to give)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, host * 1e3 / iters


def spread(v):
    return '%.3f (min %.3f, max %.3f, n %d)' % (statistics.median(v), min(v), max(v), len(v))


def report(args, variants, n_of):
    """variants: [(name, fn(i), bytes per element)]; alternating rounds, medians"""
    for _, fn, _ in variants:
        events_ms(fn, 3 * args.sets)
    got = {name: [] for name, _, _ in variants}
    for r in range(args.rounds):
        for name, fn, b in variants:
            ms, host_ms = events_ms(fn, args.iters)
            us = ms * 1e3
            got[name].append(us)
            floor = b * n_of[name] / (HBM_TBS * 1e12) * 1e6
            print('round %d  %-22s %8.2f us (host enqueue %6.2f us)   bytes / 6.3 TB/s = %6.2f us   fraction of that bound reached %.2f'
                  % (r, name, us, host_ms * 1e3, floor, floor / us))
    for name, _, _ in variants:
        print('%-22s us per launch: %s' % (name, spread(got[name])))
    return {name: statistics.median(v) for name, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--sets', type=int, default=6)
    ap.add_argument('--nets', default='image_gen,image_dis,video_dis', help='the networks whose gradient is reduced (a profiler run takes one at a time)')
    ap.add_argument('--adam', type=int, default=1, help='0: leave the Adam comparison out')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_grad_stats.py needs an MI355X')
    hl.load()
    models = dict(zip(('image_gen', 'image_dis', 'video_dis'), step.make_models('normal', num_labels=6, n_filters=64)))
    print('span %d elements per block and trip' % hl.grad_stats_span())
    variants, n_of = [], {}
    for name, net in models.items():
        if name not in args.nets.split(','):
            continue
        gs = nets.GradStats(net.fp)
        n = net.fp.size
        sets = max(args.sets, int(math.ceil(512e6 / (4.0 * n))))        # (the small networks need more sets to leave the cache)
        grads = [torch.randn(n, device='cuda') * 1e-2 for _ in range(min(sets, 64))]
        sizes = sorted(int(q.n) for q in gs.segs)
        print('%-10s n = %d (%.1f MB), %d segments from %d to %d elements, %d gradient copies' % (name, n, 4e-6 * n, len(sizes), sizes[0], sizes[-1], len(grads)))
        label = 'grad_stats ' + name
        n_of[label] = n
        variants.append((label, (lambda gs, grads: lambda i: hl.grad_stats(gs.segs, grads[i % len(grads)], 1.0, 1e30, gs.stats, gs.ctl, gs.ws))(gs, grads), 4))
    report(args, variants, n_of)
    if not args.adam:
        return

    n = models['image_gen'].fp.size
    sets = [[torch.randn(n, device='cuda') * s for s in (0.05, 1e-2, 1e-2, 0.0)] for _ in range(args.sets)]
    for s in sets:
        s[3].uniform_(0, 1e-4)                                          # v >= 0
    ctl = torch.zeros(hl.CTL_FLOATS, device='cuda')
    ctl[0] = 1.0

    def plain(i):
        p, g, m, v = sets[i % len(sets)]
        hl.adam_wd(p, g, m, v, *ADAM)

    def through_ctl(i):
        p, g, m, v = sets[i % len(sets)]
        hl.adam_wd_ctl(p, g, m, v, *ADAM, ctl)
    print('Adam at the generator\'s size, n = %d' % n)
    med = report(args, [('adam_wd', plain, 28), ('adam_wd_ctl', through_ctl, 28)], {'adam_wd': n, 'adam_wd_ctl': n})
    print('difference of the medians: %.2f us' % (med['adam_wd_ctl'] - med['adam_wd']))


if __name__ == '__main__':
    main()
