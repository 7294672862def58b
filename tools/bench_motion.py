#!/usr/bin/env python
"""What the stages of the motion and content metrics cost, on one MI355X.

    python tools/bench_motion.py [--n 4096] [--frames 16] [--dim 768] [--k 5] [--rounds 5] [--out FILE]

n clips of `--frames` per-frame descriptors of `--dim` bytes (4096 x 16 x 768 by default: --pool 4 on 16-frame RGB clips), timed
with HIP events after a warm-up, `--rounds` times each in alternating rounds in one process:
  the frame distances, the clip statistics, the motion descriptors, MotionContent.clip_set on `--clips` uint8 clips (256 by default;
  the stage is linear in the clips) and one whole MotionContent.report of two sets with its host work.
The three kernels are bound by their bytes, so each is set against the time its bytes take at 6.3 TB/s.  One set of descriptors
(50 MB) fits the 256 MB Infinity Cache; the kernels therefore walk `--sets` independent sets (8: 400 MB) in turn, so that every
call reads its descriptors from HBM.
The outside yardstick: torch.bmm on the fp32 casts of the same frames -- a TIME reference only (it reads four times the bytes and
leaves the norms and the subtraction undone).  No pass mark is set against it; the ratio is reported as measured."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl
from mocogan_chainer_amd.metrics import KnnSet, MotionContent, MotionSet

HBM = 6.3e12


def events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def spread(v):
    return '%.4f (min %.4f, max %.4f, n %d)' % (statistics.median(v), min(v), max(v), len(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=4096)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--dim', type=int, default=768)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--sets', type=int, default=8)
    ap.add_argument('--clips', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=64)
    ap.add_argument('--out', default=None, help='also write the figures as JSON')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_motion.py needs an MI355X')
    hl.load()
    n, T, Df, k, S = args.n, args.frames, args.dim, args.k, args.sets
    g = torch.Generator(device='cuda')
    g.manual_seed(1)
    descs = [torch.randint(-128, 128, (n, T, Df), dtype=torch.int8, device='cuda', generator=g) for _ in range(S)]
    dists = [torch.empty(n, T, T, dtype=torch.int32, device='cuda') for _ in range(S)]
    mdesc, mnorms = torch.empty(n, (T - 1) * Df, dtype=torch.int8, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda')
    pair, lag = torch.empty(n, dtype=torch.float64, device='cuda'), torch.empty(n, T, dtype=torch.int64, device='cuda')
    for d, o in zip(descs, dists):
        hl.mc_frame_sqdist(d, o)
    af = descs[0].float()
    tout = torch.empty(n, T, T, device='cuda')
    clips = torch.randint(0, 256, (args.clips, T, 64, 64, 3), dtype=torch.uint8, device='cuda', generator=g)
    mc = MotionContent(k, 4, n)

    def make_set(i):
        md, mn = hl.mc_motion_descriptors(descs[i])
        ps, ls = hl.mc_clip_stats(dists[i])
        flat = descs[i].view(n, T * Df)
        shape = (T, 64, 64, 3)
        return MotionSet(KnnSet(flat, (flat.to(torch.int32) ** 2).sum(dim=1, dtype=torch.int32), shape, 4), KnnSet(md, mn, shape, 4),
                         ps.cpu().numpy(), ls.cpu().numpy())

    real, fake = make_set(0), make_set(1)
    stages = (('frame_sqdist', lambda i: hl.mc_frame_sqdist(descs[i % S], dists[i % S])),
              ('clip_stats', lambda i: hl.mc_clip_stats(dists[i % S], pair, lag)),
              ('motion_descriptors', lambda i: hl.mc_motion_descriptors(descs[i % S], mdesc, mnorms)),
              ('torch.bmm fp32', lambda i: torch.bmm(af, af.transpose(1, 2), out=tout)),
              ('clip_set (%d uint8 clips, pool 4)' % args.clips, lambda i: mc.clip_set([clips])),
              ('report (two sets, host work included)', lambda i: mc.report(real, fake)))
    whole = lambda name: name.startswith(('clip_set', 'report'))
    for name, fn in stages:
        fn(0)
    torch.cuda.synchronize()
    t64 = tout.double()                                                 # (dots of 768 int8 products stay below 2^24: exact in fp32)
    gram = torch.diagonal(t64, 0, 1, 2)[:, :, None] + torch.diagonal(t64, 0, 1, 2)[:, None, :] - 2 * t64
    print('int8 frame distances against torch.bmm in fp32: max |difference| %.1f' % float((dists[0].double() - gram).abs().max()))
    ms = {name: [] for name, _ in stages}
    for r in range(args.rounds):
        for name, fn in stages:
            ms[name].append(events_ms(fn, 2 if whole(name) else args.iters))
    med = {key: statistics.median(v) for key, v in ms.items()}
    print('n = %d clips of %d frames of Df = %d bytes, k = %d, %d sets in turn; times in ms per call' % (n, T, Df, k, S))
    for name, _ in stages:
        print('  %-40s %s' % (name, spread(ms[name])))
    nbytes = {'frame_sqdist': n * T * Df + 4 * n * T * T, 'clip_stats': 4 * n * T * T + 8 * n + 8 * n * T,
              'motion_descriptors': n * T * Df + n * (T - 1) * Df + 4 * n}
    floor = {}
    for name, b in nbytes.items():
        floor[name] = b / HBM * 1e3
        print('%s: moves %.2f MB, at 6.3 TB/s %.4f ms; measured %.4f ms = %.2f x the byte floor (%.2f TB/s)'
              % (name, b * 1e-6, floor[name], med[name], med[name] / floor[name], b / (med[name] * 1e-3) * 1e-12))
    print('frame_sqdist: %.2f G integer MACs; torch.bmm fp32 %.4f ms: ratio %.2f' % (1e-9 * n * T * T * Df, med['torch.bmm fp32'],
                                                                                   med['frame_sqdist'] / med['torch.bmm fp32']))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'n': n, 'T': T, 'Df': Df, 'k': k, 'ms': ms, 'floor_ms': floor}, f)


if __name__ == '__main__':
    main()
