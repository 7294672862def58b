#!/usr/bin/env python
"""What the stages of the sliced Wasserstein distance cost, on one MI355X.

    python tools/bench_swd.py [--log2n 19] [--channels 3] [--patch_frames 1] [--dirs 128] [--rounds 5] [--out FILE]

Per-stage times at n = 2^log2n descriptors of D = patch_frames * 49 * channels values (2^19 x 147 by default: 4096 clips x 128
patches) and K = 128 directions, timed with HIP events after a warm-up, `--rounds` times each:
  pyramid + gather of `--clips` clips (64 by default; the stage is linear in the clips), channel sums, normalisation,
  directions (mcg_randn + unit columns), projection, sort, distance; and the total of one (level, repeat) for two sets.
Derived figures (operations and bytes from the shapes, over the measured time):
  projection: 2 n D K FLOP over the time, as a share of the 157.3 TFLOP/s fp32 MFMA peak; its least time is the larger of that and
              of its bytes (n D read, n K written) at 6.3 TB/s;
  sort:       launches, bytes moved per pass (a row is read and written once per pass: 8 n2 K bytes) and the share of 6.3 TB/s
              the whole sort reaches.
The outside yardstick: the same projection and sort composed from torch.matmul + torch.sort on the same tensors, in alternating
rounds in this process.  No pass mark is set against it; the ratio is reported as measured."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl

PEAK_F32_MFMA, HBM = 157.3e12, 6.3e12


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


def sort_passes(n):
    """(launches, passes over the padded rows, padded length) of mcg_sort_rows on rows of n elements"""
    L = hl.sort_local_span()
    n2 = 2
    while n2 < n:
        n2 *= 2
    if n2 <= L:
        return 1, 1, n2
    launches, k = 1, 2 * L
    while k <= n2:
        j = k // 2
        while j >= L:                                 # two steps to a launch where both are at least L wide
            launches, j = launches + 1, (j // 4 if j // 2 >= L else j // 2)
        launches, k = launches + 1, 2 * k
    return launches, launches, n2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--log2n', type=int, default=19)
    ap.add_argument('--channels', type=int, default=3)
    ap.add_argument('--patch_frames', type=int, default=1)
    ap.add_argument('--dirs', type=int, default=128)
    ap.add_argument('--clips', type=int, default=64)
    ap.add_argument('--patches', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the figures as JSON')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_swd.py needs an MI355X')
    hl.load()
    n, C, pt, K = 1 << args.log2n, args.channels, args.patch_frames, args.dirs
    D = pt * 49 * C
    g = torch.Generator(device='cuda')
    g.manual_seed(1)
    clips = torch.randint(0, 256, (args.clips, 16, 64, 64, C), dtype=torch.uint8, device='cuda', generator=g)
    raw = torch.randn(n, D, device='cuda', generator=g) * 20 + 3
    desc = [raw.clone(), raw.clone()]
    dirs = torch.empty(D, K, device='cuda')
    proj = [torch.empty(K, n, device='cuda') for _ in range(2)]
    tproj = [torch.empty(n, K, device='cuda') for _ in range(2)]
    ws = hl.swd_workspace(n, D, K, 'cuda')
    sums = torch.empty(2 * C, dtype=torch.float64, device='cuda')
    out = torch.zeros(1, dtype=torch.float64, device='cuda')
    gout = torch.empty(args.clips * args.patches, D, device='cuda')
    levels = hl.swd_pyramid(clips)

    def directions():
        hl.randn(dirs, 1.0, 1, 77)
        hl.swd_unit_columns(dirs)

    def sort_fresh():
        hl.swd_project(desc[0], dirs, proj[0])           # (a sort of sorted rows would be another measurement: project first,
        hl.sort_rows(proj[0], n, ws)                     #  and subtract the projection's time)

    def pair():
        directions()
        for x, p in zip(desc, proj):
            hl.swd_project(x, dirs, p)
            hl.sort_rows(p, n, ws)
        hl.swd_distance(proj[0], proj[1], n, ws, out)

    def torch_project():
        torch.matmul(desc[0], dirs, out=tproj[0])

    def torch_project_sort():
        torch.matmul(desc[0], dirs, out=tproj[0])
        torch.sort(tproj[0], dim=0)

    def torch_project_sort_rows():                           # the same in the direction-major layout of the hand-written chain
        torch.matmul(dirs.t(), desc[0].t(), out=proj[1])
        torch.sort(proj[1], dim=1)

    stages = (('pyramid (%d clips)' % args.clips, lambda: hl.swd_pyramid(clips)),
              ('gather l64 (%d clips)' % args.clips, lambda: hl.swd_gather(levels[0], C, 0, args.patches, pt, 1, 2, gout)),
              ('channel_sums', lambda: hl.swd_channel_sums(raw, C, ws, sums)),
              ('normalize', lambda: hl.swd_normalize(desc[1], C, sums)),
              ('directions', directions),
              ('project', lambda: hl.swd_project(desc[0], dirs, proj[0])),
              ('project+sort', sort_fresh),
              ('distance', lambda: hl.swd_distance(proj[0], proj[1], n, ws, out)),
              ('pair: directions, 2 x (project, sort), distance', pair),
              ('torch.matmul', torch_project),
              ('torch.matmul+torch.sort', torch_project_sort),
              ('torch.matmul+torch.sort, direction-major', torch_project_sort_rows))
    directions()
    hl.swd_channel_sums(raw, C, ws, sums)
    for _, fn in stages:
        fn()
    torch.cuda.synchronize()
    # the hand-written chain against the torch composition on the same tensors
    hl.swd_project(desc[0], dirs, proj[0])
    hl.swd_project(desc[0], dirs, proj[1])
    torch.matmul(desc[0], dirs, out=tproj[0])
    print('projection against torch.matmul: max |difference| %.3e' % float((proj[0].t() - tproj[0]).abs().max()))
    hl.sort_rows(proj[0], n, ws)
    print('sort against torch.sort of the same rows: equal = %s' % torch.equal(proj[0], torch.sort(proj[1], dim=1).values))
    ms = {name: [] for name, _ in stages}
    for r in range(args.rounds):
        for name, fn in stages:                                   # alternating rounds in one process
            ms[name].append(events_ms(fn, args.iters))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print('n = 2^%d = %d descriptors, D = %d, K = %d directions; times in ms per call' % (args.log2n, n, D, K))
    for name, _ in stages:
        print('  %-52s %s' % (name, spread(ms[name])))
    flop = 2.0 * n * D * K
    pbytes = 4.0 * (n * D + n * K + D * K)
    t_proj = med['project'] * 1e-3
    least = max(flop / PEAK_F32_MFMA, pbytes / HBM)
    print('projection: %.2f GFLOP, %.1f MB -> %.1f TFLOP/s = %.1f%% of the fp32 MFMA peak; least time %.3f ms (%s-bound) = %.1f%% of the measured'
          % (flop * 1e-9, pbytes * 1e-6, flop / t_proj * 1e-12, 100 * flop / t_proj / PEAK_F32_MFMA, least * 1e3,
             'compute' if flop / PEAK_F32_MFMA > pbytes / HBM else 'memory', 100 * least / t_proj))
    launches, passes, n2 = sort_passes(n)
    t_sort = (med['project+sort'] - med['project']) * 1e-3
    per_pass = 8.0 * n2 * K
    print('sort: %d launches = passes over [%d][%d] floats, %.1f MB per pass, %.3f ms -> %.2f TB/s = %.1f%% of 6.3 TB/s'
          % (launches, K, n2, per_pass * 1e-6, t_sort * 1e3, passes * per_pass / t_sort * 1e-12, 100 * passes * per_pass / t_sort / HBM))
    ours, theirs = med['project+sort'], med['torch.matmul+torch.sort']
    print('project+sort %.3f ms against torch.matmul+torch.sort %.3f ms: ratio %.2f (above 1: the hand-written chain is slower)'
          % (ours, theirs, ours / theirs))
    rows_ = med['torch.matmul+torch.sort, direction-major']
    print('project+sort %.3f ms against the direction-major torch composition (dirs^T @ desc^T, sort along dim 1) %.3f ms: ratio %.2f' % (ours, rows_, ours / rows_))
    print('  of which projection %.3f ms against torch.matmul %.3f ms; sort %.3f ms against torch.sort %.3f ms'
          % (med['project'], med['torch.matmul'], t_sort * 1e3, theirs - med['torch.matmul']))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump({'n': n, 'D': D, 'K': K, 'ms': ms, 'sort_launches': launches, 'sort_bytes_per_pass': per_pass}, f)


if __name__ == '__main__':
    main()
