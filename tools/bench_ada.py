#!/usr/bin/env python
"""What the adaptive augmentation's two launches cost, on one MI355X.

    python tools/bench_ada.py [--rounds 5] [--iters 200]

mcg_augment_draw_gated beside mcg_augment_draw (full policy, 64 x 64 frames, p = 0.5) and mcg_ada_update (one logit column,
interval 4) on 32 and on 256 clips, alternating in one process, `--rounds` times each after a warm-up, timed with HIP events
around `--iters` back-to-back launches on one stream: for kernels this small the figure is the launch-to-launch time of the
stream, which is what one more launch adds to an iteration whose stream is busy.  The step time is tools/bench_train.py's to
measure (--augment ... --ada_target ...)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl
from bench_augment import events_ms, spread


def measure(n, args):
    H = W = 64
    geo, col = torch.empty((n, 8), dtype=torch.int32, device='cuda'), torch.empty((n, 4), device='cuda')
    ada = hl.ada_state(0.5, 'cuda')
    yv, yi = torch.randn((n, 1), device='cuda'), torch.randn((n, 1), device='cuda')

    def draw(i):
        hl.augment_draw(n, H, W, 7, 1, 40 + 64 * i, geo, col)

    def gated(i):
        hl.augment_draw_gated(n, H, W, 7, 1, 40 + 64 * i, 42 + 64 * i, ada, geo, col)

    def update(i):
        hl.ada_update(yv, yi, 0.6, 1e-4, 4, ada)
    variants = (('augment_draw', draw), ('augment_draw_gated', gated), ('ada_update', update))
    for _, fn in variants:
        events_ms(fn, 50)
    us = {name: [] for name, _ in variants}
    for r in range(args.rounds):
        for name, fn in variants:
            t = events_ms(fn, args.iters) * 1e3
            us[name].append(t)
            print('round %d  n %3d  %-20s %7.2f us' % (r, n, name, t))
    for name, _ in variants:
        print('n %3d  %-20s us per launch: %s' % (n, name, spread(us[name])))
    print('n %3d  gated - plain draw: %+.2f us (medians)' % (n, statistics.median(us['augment_draw_gated']) - statistics.median(us['augment_draw'])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ada.py needs an MI355X')
    hl.load()
    for n in (32, 256):
        measure(n, args)


if __name__ == '__main__':
    main()
