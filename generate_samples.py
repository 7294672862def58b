#!/usr/bin/env python
"""Sample clips from a trained generator (raahii/mocogan-chainer generate_samples.py:17-58).
Like the reference it builds ``ImageGenerator()`` with default arguments and runs it in train mode
(batch-statistic BatchNorm, quirk Q11); ``--dim_zl`` lets a label-conditioned (MUG-trained) generator load.
``--test_mode 1`` samples with the running statistics instead (``ImageGenerator.sample``) and lets the caller choose
the labels, hold the content or the motion code fixed, and set the number of frames."""
import argparse
import os
from pathlib import Path

import numpy as np

from model.net import ImageGenerator
from util import to_grid, save_video
from mocogan_chainer_amd.trainer import load_npz
import mocogan_chainer_amd.hiplib as hl


def build_parser():
    cli = argparse.ArgumentParser(description='sample videos from a trained ImageGenerator (reference generate_samples.py)')
    for positional in ('model_weight', 'save_path'):
        cli.add_argument(positional)
    for flags, default, text in ((('--num', '-n'), 36, 'number of videos, a square number'),
                                 (('--gpu', '-g'), -1, 'kept for command-line compatibility; the MI355X path always runs on the GPU'),
                                 (('--dim_zl',), 0, 'label dimension the generator was trained with (extension)'),
                                 (('--n_filters',), 64, 'generator width (extension)')):
        cli.add_argument(*flags, type=int, default=default, help=text)
    # extensions; the defaults reproduce the reference run (train-mode BatchNorm statistics, quirk Q11)
    cli.add_argument('--test_mode', type=int, choices=[0, 1], default=0,
                     help="1: BatchNorm's running statistics through ImageGenerator.sample (folded BatchNorm, bytes formed on the device)")
    cli.add_argument('--labels', default=None, help='with --dim_zl: the label of every video, "0,3,5" (one per video) or one value for all')
    cli.add_argument('--fix_content', action='store_true', help='one content code zc shared by all videos (the motion varies)')
    cli.add_argument('--fix_motion', action='store_true', help='one motion path (h0, e) shared by all videos (the content varies)')
    cli.add_argument('--video_len', type=int, default=16, help='frames per video')
    cli.add_argument('--seed', type=int, default=None, help='np.random.seed before the latent draws')
    cli.add_argument('--mfma', choices=['f32', 'bf16', 'f32x3'], default='f32', help='MFMA operand type of the generator (as train.py)')
    return cli


def parse_args(argv=None):
    cli = build_parser()
    args = cli.parse_args(argv)
    n = int(round(np.sqrt(args.num)))
    if n * n != args.num:
        raise ValueError('--num must be n^2 (n: natural number).')
    if args.video_len < 1:
        cli.error('--video_len must be positive')
    if args.labels is not None:
        if not args.dim_zl:
            cli.error('--labels needs --dim_zl')
        try:
            labels = [int(v) for v in args.labels.split(',')]
        except ValueError:
            cli.error('--labels: integers separated by commas')
        if any(v < 0 or v >= args.dim_zl for v in labels):
            cli.error('--labels: every value must lie in [0, --dim_zl)')
        if len(labels) not in (1, args.num):
            cli.error('--labels: one value, or one per video (--num)')
        args.labels = labels
    if (args.labels is not None or args.fix_content or args.fix_motion) and not args.test_mode:
        cli.error('--labels / --fix_content / --fix_motion choose the latents: they need --test_mode 1')
    return args


def draw_latents(gen, args):
    """The latents of --test_mode 1 in the reference's order (labels, h0, e_0 .. e_{T-1}, zc); a fixed part is drawn once, for
    one video, and shared."""
    labels = None
    if gen.use_label:
        labels = np.random.randint(gen.dim_zl, size=args.num) if args.labels is None else np.asarray(args.labels)
    m = 1 if args.fix_motion else args.num
    h0 = gen.make_hidden(m, gen.dim_zm)
    e = np.stack([gen.make_hidden(m, gen.dim_zm) for _ in range(args.video_len)])
    zc = gen.make_hidden(1 if args.fix_content else args.num, gen.dim_zc)
    return dict(labels=labels, h0=h0, e=e, zc=zc)


def main(argv=None):
    args = parse_args(argv)
    n = int(round(np.sqrt(args.num)))

    gen = ImageGenerator(dim_zl=args.dim_zl, n_filters=args.n_filters, video_len=args.video_len)
    load_npz(args.model_weight, gen)
    if args.mfma != 'f32':
        gen.impl.set_precision(args.mfma)
    if args.seed is not None:
        np.random.seed(args.seed)
    print(">>> generating...")
    if args.test_mode:
        hl.use_pretuned_table()                                          # (sample never times candidates: the shipped table or the heuristic)
        videos = gen.sample(args.num, video_len=args.video_len, as_uint8=True, **draw_latents(gen, args))[0].cpu().numpy()
    else:
        videos = gen(args.num)[0].detach().cpu().numpy()                 # (T, N, C, H, W) in [-1, 1]
        videos = (255 * (0.5 * videos + 0.5)).astype(np.uint8)           # truncating cast, as the reference (:41)
    print(">>> saving...")
    save_path = Path(args.save_path)
    os.makedirs(save_path, exist_ok=True)
    save_video(to_grid(videos, n).transpose(0, 2, 3, 1), save_path / 'grid.mp4', True, save_path / 'grid')
    for i, video in enumerate(videos.transpose(1, 0, 3, 4, 2)):
        save_video(video, save_path / '{:03d}.mp4'.format(i), True, save_path / '{:03d}'.format(i))


if __name__ == "__main__":
    main()
