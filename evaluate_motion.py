#!/usr/bin/env python
"""Motion and content metrics between clips of a dataset and clips of a trained generator, on the device
(mocogan-chainer_amd/metrics.py: MotionContent; no reference counterpart -- the reference has no metric).  Prints one JSON line:
per set the Average Content Distance (after Tulyakov et al. 2018, section 5: the mean distance between the frames of one clip)
and the lag profile (frame distance against temporal lag), both as RMS differences per descriptor byte; their comparison
(acd_ratio, lag_l1); and k-NN precision / recall / density / coverage on motion descriptors (halved differences of consecutive
frames).  With --grid K it samples K content codes x K motion paths and reports how far each code sets what it is named after.
The frame distance is L2 on --pool x --pool box means, as bytes: content means appearance, not identity -- the paper's ACD uses
OpenFace features or frame-mean colour; a difference image still depends on what moves; and every k-NN figure depends on --num
and --k: compare at equal settings."""
import argparse
import json

import numpy as np

from evaluate_swd import fake_chunks, make_dataset, real_chunks


def build_parser():
    cli = argparse.ArgumentParser(description='content distance, lag profile, motion k-NN figures and the content x motion grid between real '
                                              'clips and an ImageGenerator\'s clips')
    cli.add_argument('model_weight', help='generator .npz (image_gen_epoch_*.npz or image_gen_ema_epoch_*.npz)')
    cli.add_argument('--dataset_type', default='mug', choices=['mug', 'mnist', 'synthetic'], help='as train.py')
    cli.add_argument('--dataset', default='data/dataset/train', help='root directory of the frame-directory dataset (as train.py)')
    cli.add_argument('--synthetic_size', type=int, default=256, help='clips in the synthetic dataset (as train.py)')
    for flags, default, text in ((('--num', '-n'), 1024, 'clips per set (the first --num clips of the dataset against --num generated ones)'),
                                 (('--k',), 5, 'the neighbour that sets a clip\'s radius in the motion k-NN figures (1..16; at most --num - 1)'),
                                 (('--pool',), 4, 'box the frames are averaged over: 2, 4 or 8 (2 only for short or grey clips: '
                                                  'video_len * (64 / pool)^2 * channel may not exceed 32768)'),
                                 (('--grid',), 0, 'K >= 2: also sample K content codes x K motion paths (K^2 clips; a path is h0, e and, with '
                                                  '--dim_zl, its label) and report content_ratio, motion_leak, motion_ratio, content_leak; 0: off'),
                                 (('--seed',), 0, 'seed of the latent draws'),
                                 (('--chunk',), 64, 'clips generated / uploaded at a time'),
                                 (('--dim_zl',), 0, 'label dimension the generator was trained with'),
                                 (('--n_filters',), 64, 'generator width'),
                                 (('--channel',), 3, 'image channels (1 or 3)'),
                                 (('--video_len',), 16, 'frames per clip (2..64)')):
        cli.add_argument(*flags, type=int, default=default, help=text)
    cli.add_argument('--dump', default=None, metavar='OUT.npz',
                     help='write pair_sum and lag_sum of both sets (real_*, fake_*) and, with --grid, the two K^2 x K^2 distance matrices '
                          '(grid_appearance_dist, grid_motion_dist) to this .npz')
    cli.add_argument('--test_mode', type=int, choices=[0, 1], default=1,
                     help="1 (default): BatchNorm's running statistics (ImageGenerator.sample_many); 0: batch statistics per chunk, as "
                          "generate_samples.py's default")
    cli.add_argument('--labels', default=None, help='with --dim_zl: the label of every generated clip, "0,3,5" (one per clip) or one value for all')
    cli.add_argument('--mfma', choices=['f32', 'bf16', 'f32x3'], default='f32', help='MFMA operand type of the generator (as train.py)')
    return cli


def parse_args(argv=None):
    cli = build_parser()
    args = cli.parse_args(argv)
    if args.num < 1 or args.chunk < 1:
        cli.error('--num and --chunk are positive')
    if not 2 <= args.video_len <= 64:
        cli.error('--video_len lies in 2..64: a frame distance needs two frames')
    if not 1 <= args.k <= 16:
        cli.error('--k lies in 1..16')
    if args.k > args.num - 1:
        cli.error('--k may not exceed --num - 1')
    if args.pool not in (2, 4, 8):
        cli.error('--pool is 2, 4 or 8')
    if args.channel not in (1, 3):
        cli.error('--channel is 1 or 3')
    if args.video_len * (64 // args.pool) ** 2 * args.channel > 32768:
        cli.error('--video_len * (64 / --pool)^2 * --channel exceeds 32768: use a larger --pool')
    if args.grid != 0 and args.grid < 2:
        cli.error('--grid is 0 (off) or at least 2')
    if args.grid and not args.test_mode:
        cli.error('--grid chooses the latents: it needs --test_mode 1')
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
            cli.error('--labels: one value, or one per clip (--num)')
        args.labels = labels
        if not args.test_mode:
            cli.error('--labels chooses the latents: it needs --test_mode 1')
    return args


def grid_latents(gen, K, video_len):
    """K content codes and K motion paths drawn from np.random in the reference's order (labels, h0, e_0 .. e_{T-1}, zc), repeated
    over the K^2 clips in content-major order: clip c K + m gets zc[c] and (labels[m], h0[m], e[:, m])"""
    labels, h0, e, zc = gen._latents(K, None, None, None, None, video_len)
    return {'labels': None if labels is None else np.tile(labels, K), 'h0': np.tile(h0, (K, 1)), 'e': np.tile(e, (1, K, 1)),
            'zc': np.repeat(zc, K, axis=0)}


def main(argv=None):
    args = parse_args(argv)
    from model.net import ImageGenerator
    from mocogan_chainer_amd.trainer import load_npz
    from mocogan_chainer_amd.metrics import MotionContent
    import mocogan_chainer_amd.hiplib as hl

    gen = ImageGenerator(dim_zl=args.dim_zl, out_channels=args.channel, n_filters=args.n_filters, video_len=args.video_len)
    load_npz(args.model_weight, gen)
    if args.mfma != 'f32':
        gen.impl.set_precision(args.mfma)
    hl.use_pretuned_table()                                              # (sampling never times candidates)
    np.random.seed(args.seed)
    mc = MotionContent(args.k, args.pool)
    real = mc.clip_set(real_chunks(make_dataset(args), args.num, args.chunk))
    fake = mc.clip_set(fake_chunks(gen, args))
    out = mc.report(real, fake)
    dump = {'real_pair_sum': real.pair_sum, 'real_lag_sum': real.lag_sum, 'fake_pair_sum': fake.pair_sum, 'fake_lag_sum': fake.lag_sum}
    if args.grid:                                                        # (drawn after the fake set: the figures above do not depend on --grid)
        K = args.grid
        grid = mc.grid_report(mc.clip_set(gen.sample_many(K * K, args.chunk, video_len=args.video_len, **grid_latents(gen, K, args.video_len))), K)
        dump.update({'grid_' + key: grid.pop(key) for key in ('appearance_dist', 'motion_dist')})
        out.update(grid)
    if args.dump:
        np.savez(args.dump, **dump)
    out.update(num=args.num, k=args.k, pool=args.pool, grid=args.grid, frames=real.frames, frame_dim=real.frame_dim, seed=args.seed,
               test_mode=args.test_mode, model_weight=str(args.model_weight), dataset_type=args.dataset_type)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
