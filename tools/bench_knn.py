#!/usr/bin/env python
"""What the stages of the nearest-neighbour metrics cost, on one MI355X.

    python tools/bench_knn.py [--n 4096] [--dim 12288] [--k 5] [--rounds 5] [--out FILE]

n descriptors against n of `--dim` bytes (4096 x 4096 x 12288 by default: --pool 4 on 16-frame RGB clips), timed with HIP events
after a warm-up, `--rounds` times each in alternating rounds in one process:
  descriptors of `--clips` clips (64 by default; the stage is linear in the clips), squared distances, the k smallest with the
  diagonal left out, the nearest (k = 1), the ball counts, and the whole KnnMetrics.report of two sets with a held-out third.
Derived: the int8 operation rate of the distances, 2 n^2 D over the time, as a share of twice the bf16 MFMA peak (the int8 forms
take the cycles of the bf16 forms at twice the K), and the share of 6.3 TB/s the row passes reach.
The outside yardstick: torch.matmul on the same matrices cast to fp32 -- a TIME reference only: fp32 products of length 12288 are
not exact here.  No pass mark is set against it; the ratio is reported as measured."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl
from mocogan_chainer_amd.metrics import KnnMetrics, KnnSet

PEAK_I8_MFMA, HBM = 2 * 2516.8e12, 6.3e12


def events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(v):
    return '%.3f (min %.3f, max %.3f, n %d)' % (statistics.median(v), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--dim', type=int, default=12288)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the figures as JSON')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_knn.py needs an MI355X')
    hl.load()
    n, D, k = args.n, args.dim, args.k
    g = torch.Generator(device='cuda')
    g.manual_seed(1)
    clips = torch.randint(0, 256, (args.clips, 16, 64, 64, 3), dtype=torch.uint8, device='cuda', generator=g)

    def make_set():
        desc = torch.randint(-128, 128, (n, D), dtype=torch.int8, device='cuda', generator=g)
        return KnnSet(desc, (desc.to(torch.int32) ** 2).sum(dim=1, dtype=torch.int32), (16, 64, 64, 3), 4)

    a, b, h = make_set(), make_set(), make_set()
    dist = torch.empty(n, n, dtype=torch.int32, device='cuda')
    radius = torch.randint(0, 2 ** 30, (n,), dtype=torch.int32, device='cuda', generator=g)
    af, bf = a.desc.float(), b.desc.float()
    tout = torch.empty(n, n, device='cuda')
    knn = KnnMetrics(k, 4, n)
    hl.knn_sqdist(a.desc, a.norms, b.desc, b.norms, dist)
    stages = (('descriptors (%d clips, pool 4)' % args.clips, lambda: hl.knn_descriptors(clips, 4)),
              ('sqdist', lambda: hl.knn_sqdist(a.desc, a.norms, b.desc, b.norms, dist)),
              ('smallest k=%d, no diagonal' % k, lambda: hl.knn_smallest(dist, k, exclude_self=True)),
              ('smallest k=1', lambda: hl.knn_smallest(dist, 1)),
              ('smallest k=16', lambda: hl.knn_smallest(dist, 16)),
              ('ball_counts', lambda: hl.knn_ball_counts(dist, radius)),
              ('report (real, fake, holdout)', lambda: knn.report(a, b, h)),
              ('torch.matmul fp32', lambda: torch.matmul(af, bf.t(), out=tout)))
    for _, fn in stages:
        fn()
    torch.cuda.synchronize()
    dot = (a.norms[:, None].double() + b.norms[None, :].double() - dist.double()) / 2
    print('int8 dots against torch.matmul in fp32: max |difference| %.1f (fp32 is the inexact one)' % float((dot - tout.double()).abs().max()))
    ms = {name: [] for name, _ in stages}
    for r in range(args.rounds):
        for name, fn in stages:
            ms[name].append(events_ms(fn, 1 if name.startswith('report') else args.iters))
    med = {key: statistics.median(v) for key, v in ms.items()}
    print('n = %d against %d descriptors of D = %d bytes, k = %d; times in ms per call' % (n, n, D, k))
    for name, _ in stages:
        print('  %-36s %s' % (name, spread(ms[name])))
    ops = 2.0 * n * n * D
    t = med['sqdist'] * 1e-3
    print('sqdist: %.3f T integer operations in %.3f ms -> %.1f TOP/s = %.1f%% of the int8 MFMA peak (2 x %.1f); torch.matmul fp32 %.3f ms: ratio %.2f'
          % (ops * 1e-12, t * 1e3, ops / t * 1e-12, 100 * ops / t / PEAK_I8_MFMA, PEAK_I8_MFMA / 2e12, med['torch.matmul fp32'],
             med['sqdist'] / med['torch.matmul fp32']))
    for name in ('smallest k=%d, no diagonal' % k, 'smallest k=1', 'smallest k=16', 'ball_counts'):
        print('%s: reads %.1f MB in %.3f ms -> %.2f TB/s = %.1f%% of 6.3 TB/s' % (name, 4e-6 * n * n, med[name], 4.0 * n * n / med[name] * 1e-9,
                                                                                100 * 4.0 * n * n / (med[name] * 1e-3) / HBM))
    five = 5 * med['sqdist']
    print('report: %.3f ms, of which five distance matrices %.3f ms (%.0f%%)' % (med['report (real, fake, holdout)'], five,
                                                                                100 * five / med['report (real, fake, holdout)']))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'n': n, 'D': D, 'k': k, 'ms': ms}, f)


if __name__ == '__main__':
    main()
