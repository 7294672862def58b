#!/usr/bin/env python
"""Row-major against position-major rows (live K-steps) of the 'f32x3' (MCG_PREC_SPLIT) forward and weight-gradient launches, per
launch of the shipped tile table, in ONE process.

For every fprop / wgrad entry of mocogan-chainer_amd/tuned_tiles_mi355x.json with split operands: the code the launch runs today (the dense
list's, else the table's own) and the position-major candidates (forward, hiplib.LIVE_CANDIDATES: 27 / 40 one block per tile, + 1000 /
+ 2000 tiles cut by live steps; weight gradient, hiplib.LIVE_WGRAD_CANDIDATES: 27 / 28 and their pixel-split variants) are timed in alternating rounds on the same tensors.  An entry moves only where the best
candidate's median beats the current median by more than the spread (max - min) of the current form's own rounds.  Raw lines go
to --raw, the per-entry table to stdout, and the entries that pass -- [[key, code], ...], the form of
mocogan-chainer_amd/live_tiles_mi355x.json -- to --out.  That file is a list of CANDIDATES for the shipped list, which is curated:
the plain launch is timed here, and a forward launch that carries an epilogue in the network (or moves to a cut code >= 1000 and
then pays for the stand-alone pass) can behave otherwise there.  An entry is shipped only when a one-stream kernel trace of the
iteration (bench.py --overlap 0 with MCG_LIVE_STEPS=0 / 1) confirms it; profiles/live_steps_notes.md records which were.
usage: python tools/ab_live_steps.py --raw <raw lines file> --out <list file> [--rounds 5] [--batch 64,512]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl
from tools.ab_dense_split import timeit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--raw', required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--batch', default='', help='comma-separated N: only the entries of these batch sizes')
    args = ap.parse_args()
    pkg = os.path.dirname(hl.__file__)
    hl.load()
    table = json.load(open(os.path.join(pkg, 'tuned_tiles_mi355x.json')))
    dense = {tuple(k): v for k, v in json.load(open(os.path.join(pkg, 'dense_tiles_mi355x.json')))}
    only = [int(v) for v in args.batch.split(',') if v]
    raw = open(args.raw, 'w')
    print('%-5s %5s %3s %3s %4s %4s %2s | %6s %9s %9s | %6s %9s %7s  %s' % ('pass', 'N', 'Ti', 'H', 'Ci', 'Co', 'kt', 'now', 'median ms', 'spread', 'live', 'median ms', 'gain %', 'verdict'))
    moved = []
    for key, code in table:
        if key[0] not in ('fprop', 'wgrad') or key[9] != hl.PREC_SPLIT or len(key) > 10 or key[8] or (only and key[1] not in only):
            continue
        kind, N, Ti, Hi, Wi, Ci, Co, kt = key[:8]
        g = hl.make_geom(N, Ti, Hi, Wi, Ci, Co, kt, precision='f32x3')
        x = torch.randn((N, Ti, Hi, Wi, Ci), device='cuda')
        y = torch.randn((N, g.To, g.Ho, g.Wo, Co), device='cuda')
        w = torch.randn((Co, kt, 4, 4, Ci), device='cuda') * 0.05
        if kind == 'fprop':
            xs, ws = hl.split_planes(x), hl.split_planes(w)
            run = lambda: hl.conv_fprop(g, xs, ws, None, y)
        else:
            xs, ws, dw = hl.split_planes(x), hl.split_planes(y), torch.zeros_like(w)
            run = lambda: hl.conv_wgrad(g, xs, ws, dw)
        codes = [dense.get(tuple(key), code) or 7]
        for c in (hl.LIVE_CANDIDATES if kind == 'fprop' else hl.LIVE_WGRAD_CANDIDATES):
            g.tile = c
            try:
                run()
                torch.cuda.synchronize()
                codes.append(c)
            except hl.McgError:
                pass
        ms = {c: [] for c in codes}
        for r in range(args.rounds):
            for c in codes:
                g.tile = c
                t = timeit(run)
                ms[c].append(t)
                raw.write(kind + " %s code %d round %d %.5f ms\n" % (' '.join(str(v) for v in key[1:]), c, r, t))
        raw.flush()
        now = ms[codes[0]]
        nmed, spread = statistics.median(now), max(now) - min(now)
        if len(codes) == 1:
            print('%-5s %5d %3d %3d %4d %4d %2d | %6d %9.4f %9.4f | no position-major form' % (kind, N, Ti, Hi, Ci, Co, kt, codes[0], nmed, spread))
            continue
        best = min(codes[1:], key=lambda c: statistics.median(ms[c]))
        bmed = statistics.median(ms[best])
        win = nmed - bmed > spread
        print('%-5s %5d %3d %3d %4d %4d %2d | %6d %9.4f %9.4f | %6d %9.4f %7.1f  %s   [%s]' % (
            kind, N, Ti, Hi, Ci, Co, kt, codes[0], nmed, spread, best, bmed, 100 * (nmed - bmed) / nmed, 'passes' if win else 'stays',
            ' '.join('%d: %.4f' % (c, statistics.median(ms[c])) for c in codes[1:])))
        if win:
            moved.append([key, best])
        del x, y, w, xs, ws
    print('%d entries pass' % len(moved))
    json.dump(moved, open(args.out, 'w'))


if __name__ == '__main__':
    main()
