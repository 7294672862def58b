#!/usr/bin/env python
"""Padded against dense LDS form of the 'f32x3' (MCG_PREC_SPLIT) conv launches, per launch of the shipped tile table, in ONE process.

For every fprop / dgrad / wgrad entry of mocogan-chainer_amd/tuned_tiles_mi355x.json with split operands: the entry's own tile code
(padded form) and the dense candidates (17 / 20 and their K-split / pixel-split variants) are timed in alternating rounds on the
same tensors.  An entry moves to the best dense code only where that code's median beats the padded median by more than the
spread (max - min) of the padded form's own rounds.  Raw lines go to --raw, the per-entry table to stdout, and the entries that
moved -- [[key, dense code], ...], the form of mocogan-chainer_amd/dense_tiles_mi355x.json -- to --out.
usage: python tools/ab_dense_split.py --raw <raw lines file> --out <dense list file> [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mocogan_chainer_amd.hiplib as hl

DENSE = {"fprop": (17, 20, 1017, 2017, 1020, 2020), "dgrad": (17, 20, 1017, 2017, 1020, 2020), "wgrad": (17, 20, 2017, 2020, 1020)}


def timeit(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--raw', required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--table', default=os.path.join(os.path.dirname(hl.__file__), 'tuned_tiles_mi355x.json'))
    args = ap.parse_args()
    hl.load()
    table = json.load(open(args.table))
    raw = open(args.raw, 'w')
    print('%-6s %5s %3s %3s %4s %4s %2s | %6s %9s %9s | %6s %9s %7s  %s' % ('pass', 'N', 'Ti', 'H', 'Ci', 'Co', 'kt', 'padded', 'median ms', 'spread', 'dense', 'median ms', 'gain %', 'verdict'))
    moved = []
    for entry in table:
        key, code = entry
        kind = key[0]
        if kind not in DENSE or key[9] != hl.PREC_SPLIT or len(key) > 12:
            continue
        _, N, Ti, Hi, Wi, Ci, Co, kt, perm, _ = key[:10]
        if perm or (kind == "dgrad" and tuple(key[10:12]) != (0, 0)):
            continue
        g = hl.make_geom(N, Ti, Hi, Wi, Ci, Co, kt, precision='f32x3')
        x = torch.randn((N, Ti, Hi, Wi, Ci), device='cuda')
        y = torch.randn((N, g.To, g.Ho, g.Wo, Co), device='cuda')
        w = torch.randn((Co, kt, 4, 4, Ci), device='cuda') * 0.05
        if kind == "fprop":
            xs, ws = hl.split_planes(x), hl.split_planes(w)
            run = lambda: hl.conv_fprop(g, xs, ws, None, y)
        elif kind == "dgrad":
            ys, wd = hl.split_planes(y), hl.split_planes(w, run=16 * kt * 16 * Ci)
            run = lambda: hl.conv_dgrad(g, ys, wd, None, x)
        else:
            xs, ys, dw = hl.split_planes(x), hl.split_planes(y), torch.zeros_like(w)
            run = lambda: hl.conv_wgrad(g, xs, ys, dw)
        codes = [code or 7]                               # (0 is the library's choice for split operands: 7)
        for c in DENSE[kind]:
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
                raw.write("%s %s code %d round %d %.5f ms\n" % (kind, ' '.join(str(v) for v in key[1:]), c, r, t))
        raw.flush()
        pad = ms[codes[0]]
        pmed, spread = statistics.median(pad), max(pad) - min(pad)
        best = min(codes[1:], key=lambda c: statistics.median(ms[c])) if len(codes) > 1 else None
        if best is None:
            print('%-6s %5d %3d %3d %4d %4d %2d | %6d %9.4f %9.4f | no dense form' % (kind, N, Ti, Hi, Ci, Co, kt, codes[0], pmed, spread))
            continue
        bmed = statistics.median(ms[best])
        win = pmed - bmed > spread
        print('%-6s %5d %3d %3d %4d %4d %2d | %6d %9.4f %9.4f | %6d %9.4f %7.1f  %s' % (kind, N, Ti, Hi, Ci, Co, kt, codes[0], pmed, spread, best, bmed,
                                                                                  100 * (pmed - bmed) / pmed, 'dense' if win else 'stays'))
        if win:
            moved.append([key, best])
        del x, y, w
    print('%d entries moved to the dense form' % len(moved))
    json.dump(moved, open(args.out, 'w'))


if __name__ == '__main__':
    main()
