"""Sliced Wasserstein distance between two sets of uint8 clips (Karras et al. 2018, section 5), composed from the mcg_swd_* stages
of libmocogan_hip.so (include/mocogan_hip.h).  torch supplies memory and the stream; every arithmetic step is a HIP kernel.

What the number is: per pyramid level, how far the distributions of normalised 7x7(x patch_frames) Laplacian patches of the two
sets lie apart, x 1e3 as ProGAN reports it.  What it is not: it sees nothing a 7x7(x patch_frames) patch cannot see -- no global
layout, no identity, no motion beyond patch_frames frames.

KnnMetrics, below it, is the complement: nearest-neighbour precision / recall, density / coverage and a data-copying score on
whole-clip descriptors, composed from the mcg_knn_* stages (exact integer distances on the int8 matrix pipe).

MotionContent, last, looks inside a clip: the distances between its own frames (Average Content Distance, a lag profile), the k-NN
figures on motion descriptors, and the content x motion grid, composed from the mcg_mc_* stages.
"""
import math

import numpy as np
import torch

from . import hiplib as hl

LEVELS = hl.SWD_LEVELS                                            # (64, 32, 16)
STREAM_BASE = 0x535744 << 32                                      # Philox stream ids of the metric ('SWD' in the high word)


def position_stream(level_index):
    """stream id of the patch positions of pyramid level LEVELS[level_index]"""
    return STREAM_BASE + level_index


def direction_stream(level_index, repeat):
    """stream id of the directions of (level, repeat)"""
    return STREAM_BASE + ((level_index + 1) << 24) + repeat


class DescriptorSet:
    """The normalised descriptors of one set of clips: desc[level] is [n][D] fp32 on the device (n = clips * patches)."""

    def __init__(self, clips, channels, frames, desc, sums):
        self.clips, self.channels, self.frames, self.desc, self.sums = clips, channels, frames, desc, sums
        self.n, self.dim = desc[LEVELS[0]].shape                 # (sums is None: gathered, not yet normalised)


class SlicedWasserstein:
    def __init__(self, patches=128, patch_frames=1, repeats=4, dirs=128, seed=0, device='cuda'):
        if min(patches, patch_frames, repeats, dirs) < 1:
            raise ValueError('patches, patch_frames, repeats and dirs are positive')
        self.patches, self.patch_frames, self.repeats, self.dirs, self.seed = patches, patch_frames, repeats, dirs, seed
        self.device = torch.device(device)

    def raw_descriptors(self, chunks):
        """chunks: an iterable of uint8 arrays / tensors (N_i, T, 64, 64, C), host or device, N_i of any size -> the descriptors as
        gathered (not normalised).  Clip i of the concatenation takes the Philox counters i * patches .. of every level, so the
        chunking does not change the result."""
        P, pt = self.patches, self.patch_frames
        parts = {s: [] for s in LEVELS}
        first, shape = 0, None
        for chunk in chunks:
            u8 = torch.as_tensor(np.ascontiguousarray(chunk) if isinstance(chunk, np.ndarray) else chunk)
            if u8.dtype != torch.uint8 or u8.dim() != 5:
                raise ValueError('clips are uint8 (N,T,64,64,C), got %s %s' % (u8.dtype, tuple(u8.shape)))
            if shape is None:
                shape = tuple(u8.shape[1:])
                if pt > shape[0]:
                    raise ValueError('patch_frames %d exceeds the clip length %d' % (pt, shape[0]))
            elif tuple(u8.shape[1:]) != shape:
                raise ValueError('chunks differ in shape: %s and %s' % (shape, tuple(u8.shape[1:])))
            if u8.shape[0] == 0:
                continue
            u8 = u8.to(self.device).contiguous()
            c = shape[3]
            for li, (s, level) in enumerate(zip(LEVELS, hl.swd_pyramid(u8))):
                out = torch.empty(u8.shape[0] * P, pt * 49 * c, dtype=torch.float32, device=self.device)
                parts[s].append(hl.swd_gather(level, c, first, P, pt, self.seed, position_stream(li), out))
            first += u8.shape[0]
        if not first:
            raise ValueError('no clips')
        desc = {s: (parts[s][0] if len(parts[s]) == 1 else torch.cat(parts[s])) for s in LEVELS}     # (a copy, no arithmetic)
        return DescriptorSet(first, shape[3], shape[0], desc, None)

    def normalized(self, raw, lo=0, hi=None, inplace=False):
        """The set made of clips lo .. hi of a raw set, normalised per channel and level with ITS OWN statistics (a copy unless
        inplace)."""
        if raw.sums is not None:
            raise ValueError('the set is normalised already')
        hi = raw.clips if hi is None else hi
        if not 0 <= lo < hi <= raw.clips:
            raise ValueError('clips %d .. %d of a set of %d' % (lo, hi, raw.clips))
        P, c = self.patches, raw.channels
        ws = hl.swd_workspace((hi - lo) * P, raw.dim, 1, self.device)
        desc, sums = {}, {}
        for s in LEVELS:
            rows = raw.desc[s][lo * P:hi * P]
            desc[s] = rows if inplace else rows.clone()
            sums[s] = hl.swd_channel_sums(desc[s], c, ws)
            hl.swd_normalize(desc[s], c, sums[s])
        if inplace:
            raw.desc = None
        return DescriptorSet(hi - lo, c, raw.frames, desc, sums)

    def descriptors(self, chunks):
        """the normalised descriptors of the clips of `chunks` (raw_descriptors, then normalised in place)"""
        return self.normalized(self.raw_descriptors(chunks), inplace=True)

    def distance(self, a, b):
        """{'64': .., '32': .., '16': .., 'avg': ..}: 1e3 x the mean over repeats, directions and ranks of |sorted projection of a -
        sorted projection of b| per level, and the levels' average.  One projection buffer per set is alive at a time."""
        if a.sums is None or b.sums is None:
            raise ValueError('distance takes normalised sets (descriptors / normalized)')
        if (a.n, a.dim, a.channels) != (b.n, b.dim, b.channels):
            raise ValueError('the sets differ in size: %d x %d and %d x %d descriptors' % (a.n, a.dim, b.n, b.dim))
        n, d, K, R = a.n, a.dim, self.dirs, self.repeats
        ws = hl.swd_workspace(n, d, K, self.device)
        proj = [torch.empty(K, n, dtype=torch.float32, device=self.device) for _ in range(2)]
        dirs = torch.empty(d, K, dtype=torch.float32, device=self.device)
        out = torch.zeros(len(LEVELS) * R, dtype=torch.float64, device=self.device)
        for li, s in enumerate(LEVELS):
            for r in range(R):
                hl.randn(dirs, 1.0, self.seed, direction_stream(li, r))
                hl.swd_unit_columns(dirs)
                for x, p in zip((a, b), proj):
                    hl.swd_project(x.desc[s], dirs, p)
                    hl.sort_rows(p, n, ws)
                hl.swd_distance(proj[0], proj[1], n, ws, out[li * R + r:li * R + r + 1])
        vals = out.cpu().numpy().reshape(len(LEVELS), R)
        res = {str(s): float(np.sum(vals[li]) / R * 1e3) for li, s in enumerate(LEVELS)}
        res['avg'] = float(sum(res[str(s)] for s in LEVELS) / len(LEVELS))
        return res


# ---- nearest-neighbour metrics: precision / recall, density / coverage, a data-copying score (mcg_knn_*) ----------------------------
class KnnSet:
    """The whole-clip descriptors of one set of clips: desc [n][D] int8 and norms [n] int32 (sum of squares) on the device."""

    def __init__(self, desc, norms, shape, pool):
        self.desc, self.norms, self.shape, self.pool = desc, norms, shape, pool
        self.n, self.dim = desc.shape


class KnnMetrics:
    """Improved precision / recall (Kynkaanniemi et al. 2019), density / coverage (Naeem et al. 2020) and a data-copying score
    (after Meehan et al. 2020) between sets of uint8 clips, composed from the mcg_knn_* stages of libmocogan_hip.so.  Distances are
    squared L2 between pool x pool box means of whole clips, as bytes: every quantity is an integer, the distances come exact from
    the int8 matrix pipe, and the figures equal tests/knn_ref.py's bit for bit.

    What the numbers are not: the distance compares ALIGNED clips, so a shifted copy is not a copy; the radii, and with them
    every figure, depend on the set sizes and on k -- compare at equal settings; copy_auc means something only with held-out
    clips that training never saw."""

    def __init__(self, k=5, pool=4, row_block=4096, device='cuda'):
        if not 1 <= k <= hl.KNN_MAX_K:
            raise ValueError('k lies in 1..%d' % hl.KNN_MAX_K)
        if pool not in hl.KNN_POOLS:
            raise ValueError('pool is one of %s' % (hl.KNN_POOLS,))
        if row_block < 1:
            raise ValueError('row_block is positive')
        self.k, self.pool, self.row_block, self.device = k, pool, row_block, torch.device(device)

    def descriptors(self, chunks):
        """chunks: an iterable of uint8 arrays / tensors (N_i, T, 64, 64, C), host or device, N_i of any size (as
        SlicedWasserstein.raw_descriptors) -> the KnnSet of their concatenation.  A clip's row depends on that clip alone, so the
        chunking does not change the result."""
        desc, norms, shape = [], [], None
        for chunk in chunks:
            u8 = torch.as_tensor(np.ascontiguousarray(chunk) if isinstance(chunk, np.ndarray) else chunk)
            if u8.dtype != torch.uint8 or u8.dim() != 5:
                raise ValueError('clips are uint8 (N,T,64,64,C), got %s %s' % (u8.dtype, tuple(u8.shape)))
            if shape is None:
                shape = tuple(u8.shape[1:])
                d = shape[0] * (64 // self.pool) ** 2 * shape[3]
                if shape[1:3] != (64, 64) or not 1 <= shape[3] <= 3:
                    raise ValueError('clips are (N,T,64,64,C) with C in 1..3, got %s' % (tuple(u8.shape),))
                if d > hl.KNN_MAX_D:
                    raise ValueError('pool %d gives descriptors of %d bytes, the limit is %d: use a larger pool' % (self.pool, d, hl.KNN_MAX_D))
            elif tuple(u8.shape[1:]) != shape:
                raise ValueError('chunks differ in shape: %s and %s' % (shape, tuple(u8.shape[1:])))
            if u8.shape[0] == 0:
                continue
            dn = hl.knn_descriptors(u8.to(self.device).contiguous(), self.pool)
            desc.append(dn[0])
            norms.append(dn[1])
        if not desc:
            raise ValueError('no clips')
        one = len(desc) == 1
        return KnnSet(desc[0] if one else torch.cat(desc), norms[0] if one else torch.cat(norms), shape, self.pool)     # (copies, no arithmetic)

    def _rows(self, a, b, fn):
        """the device tensors fn(dist block, first row) returns, concatenated over blocks of row_block rows of the squared
        distances of set a (rows) to set b (columns).  Every stage is per row, so the blocking is exact."""
        out = torch.empty(min(self.row_block, a.n), b.n, dtype=torch.int32, device=self.device)
        parts = []
        for lo in range(0, a.n, self.row_block):
            hi = min(lo + self.row_block, a.n)
            parts.append(fn(hl.knn_sqdist(a.desc[lo:hi], a.norms[lo:hi], b.desc, b.norms, out[:hi - lo]), lo))
        return [torch.cat(p) for p in zip(*parts)]

    def radii(self, x):
        """rad[i]: the k-th smallest squared distance from x[i] to the other members of x (int32, on the device)"""
        k = self.k
        return self._rows(x, x, lambda d, lo: (hl.knn_smallest(d, k, exclude_self=True, self_col0=lo)[0][:, k - 1],))[0].contiguous()

    def report(self, real, fake, holdout=None):
        """{'precision', 'recall', 'density', 'coverage', 'copy_auc' (None without holdout), 'nn_index', 'nn_dist'} of KnnSets:
        R = real (the training clips), F = fake, H = held-out real clips.  With rad_X[i] the k-th smallest squared distance of X_i
        to the rest of X:  precision = share of F inside some ball (R_j, rad_R[j]); recall = share of R inside some ball (F_j,
        rad_F[j]); density = balls of R a fake lies in, on average, over k; coverage = share of R whose nearest fake lies within
        rad_R; copy_auc = P(dF < dH) + P(dF == dH) / 2 for dF, dH the distances of a fake / a held-out clip to its nearest
        training clip (0.5: as far as fresh real clips; towards 1: closer -- copying); nn_index, nn_dist: every fake clip's
        nearest training clip and its squared distance.  Every O(n^2) step is a kernel; the scalars are integer counts over the
        O(n) arrays and one float64 division."""
        sets = [s for s in (real, fake, holdout) if s is not None]
        if any((s.dim, s.pool) != (real.dim, real.pool) for s in sets):
            raise ValueError('the sets differ in descriptor size or pool')
        k = self.k
        if k > min(real.n, fake.n) - 1:
            raise ValueError('k = %d needs sets of at least %d clips (got %d real, %d fake)' % (k, k + 1, real.n, fake.n))
        rad_r, rad_f = self.radii(real), self.radii(fake)
        one = lambda dist: hl.knn_smallest(dist, 1)
        counts_f, nn_dist, nn_index = self._rows(fake, real, lambda d, lo: (hl.knn_ball_counts(d, rad_r),) + tuple(v[:, 0] for v in one(d)))
        counts_r, near_f = self._rows(real, fake, lambda d, lo: (hl.knn_ball_counts(d, rad_f), one(d)[0][:, 0]))
        host = lambda t: t.cpu().numpy().astype(np.int64)
        counts_f, nn_dist, nn_index, counts_r, near_f, rad_r = (host(t) for t in (counts_f, nn_dist, nn_index, counts_r, near_f, rad_r))
        out = {'precision': int((counts_f > 0).sum()) / fake.n, 'recall': int((counts_r > 0).sum()) / real.n,
               'density': int(counts_f.sum()) / (k * fake.n), 'coverage': int((near_f <= rad_r).sum()) / real.n,
               'copy_auc': None, 'nn_index': nn_index, 'nn_dist': nn_dist}
        if holdout is not None:
            d_h = np.sort(host(self._rows(holdout, real, lambda d, lo: (one(d)[0][:, 0],))[0]))
            lo_, hi_ = np.searchsorted(d_h, nn_dist, 'left'), np.searchsorted(d_h, nn_dist, 'right')
            less, equal = int((holdout.n - hi_).sum()), int((hi_ - lo_).sum())       # pairs with dF < dH, with dF == dH
            out['copy_auc'] = (2 * less + equal) / (2 * fake.n * holdout.n)
        return out


# ---- motion and content: frame distances inside a clip, a lag profile, k-NN on motion descriptors, the code grid (mcg_mc_*) ---------
class MotionSet:
    """One set of clips for MotionContent: pair_sum [n] float64 and lag_sum [n][T] int64 on the host (mcg_mc_clip_stats), the
    whole-clip KnnSet `clips` and the motion KnnSet `motion` (halved differences of consecutive frames) on the device."""

    def __init__(self, clips, motion, pair_sum, lag_sum):
        self.clips, self.motion, self.pair_sum, self.lag_sum = clips, motion, pair_sum, lag_sum
        self.n, self.frames = lag_sum.shape
        self.frame_dim = clips.dim // self.frames
        self.shape, self.pool = clips.shape, clips.pool


class MotionContent:
    """What a clip's frames do to one another, composed from the mcg_mc_* and mcg_knn_* stages of libmocogan_hip.so: the mean
    pairwise frame distance of a clip (Average Content Distance after Tulyakov et al. 2018, section 5, in the descriptor space of
    KnnMetrics), the temporal structure function (frame distance against lag), the k-NN figures of KnnMetrics on motion
    descriptors, and for a content x motion grid of generated clips how far each code sets what it is named after.  The frame
    distances are exact integers from the int8 matrix pipe; the figures equal tests/motion_ref.py's (acd up to the rounding of a
    sum of square roots).

    What the numbers are not: the frame distance is L2 on pooled bytes, so content means appearance, not identity; the paper's ACD
    uses OpenFace features or frame-mean colour -- this is the same statistic in another feature space; the motion descriptors are
    difference images, and a difference image still depends on what moves; every k-NN figure depends on the set sizes and on k."""

    def __init__(self, k=5, pool=4, row_block=4096, device='cuda'):
        self.knn = KnnMetrics(k, pool, row_block, device)
        self.k, self.pool, self.row_block, self.device = k, pool, row_block, self.knn.device

    def clip_set(self, chunks):
        """chunks: uint8 (N_i, T, 64, 64, C) arrays / tensors as KnnMetrics.descriptors takes them -> the MotionSet of their
        concatenation.  Per chunk: descriptors, frame distances (a scratch block, reused), clip statistics, motion descriptors.  A
        clip's rows depend on that clip alone, so the chunking changes no bit."""
        desc, norms, mdesc, mnorms, pair, lag, shape, scratch = [], [], [], [], [], [], None, None
        for chunk in chunks:
            if len(chunk) == 0:
                continue
            if shape is None and len(chunk.shape) == 5 and not 2 <= chunk.shape[1] <= hl.MC_MAX_T:
                raise ValueError('frame distances need clips of 2..%d frames, got %d' % (hl.MC_MAX_T, chunk.shape[1]))
            # refuses other shapes, and rows past 32768 bytes ('use a larger pool'): a motion row, (T - 1) Df bytes, is shorter than that
            part = self.knn.descriptors([chunk])
            if shape is None:
                shape = part.shape
                T = shape[0]
            elif part.shape != shape:
                raise ValueError('chunks differ in shape: %s and %s' % (shape, part.shape))
            frames = part.desc.view(part.n, T, part.dim // T)
            if scratch is None or scratch.shape[0] < part.n:
                scratch = torch.empty(part.n, T, T, dtype=torch.int32, device=self.device)
            ps, ls = hl.mc_clip_stats(hl.mc_frame_sqdist(frames, scratch[:part.n]))
            md, mn = hl.mc_motion_descriptors(frames)
            for lst, v in ((desc, part.desc), (norms, part.norms), (mdesc, md), (mnorms, mn), (pair, ps), (lag, ls)):
                lst.append(v)
        if not desc:
            raise ValueError('no clips')
        cat = lambda v: v[0] if len(v) == 1 else torch.cat(v)        # (copies, no arithmetic)
        clips = KnnSet(cat(desc), cat(norms), shape, self.pool)
        motion = KnnSet(cat(mdesc), cat(mnorms), shape, self.pool)
        return MotionSet(clips, motion, cat(pair).cpu().numpy(), cat(lag).cpu().numpy())

    def summary(self, s):
        """{'acd': the mean over clips and frame pairs of the frame distance as an RMS difference per descriptor byte (0..255; 0: a
        frozen clip), 'lag': [l = 1 .. T-1] the RMS difference per byte of frames l apart (lag[0]: frame-to-frame motion energy; flat:
        flicker; zero: a still), 'lag1_q': the 5 / 50 / 95 % quantiles over clips of the lag-1 figure}.  Integer sums in int64 on
        the host, one float64 expression each."""
        n, T, Df = s.n, s.frames, s.frame_dim
        P = T * (T - 1) // 2
        lag_tot = s.lag_sum.astype(np.int64).sum(axis=0)
        return {'acd': float(np.mean(s.pair_sum)) / (P * math.sqrt(Df)),
                'lag': [math.sqrt(int(lag_tot[l]) / (n * (T - l) * Df)) for l in range(1, T)],
                'lag1_q': [float(v) for v in np.quantile(np.sqrt(s.lag_sum[:, 1].astype(np.int64) / ((T - 1) * Df)), [0.05, 0.5, 0.95])]}

    def report(self, real, fake):
        """{'real', 'fake': the summaries; 'acd_ratio': acd_fake / acd_real (None when acd_real is 0); 'lag_l1': the mean over lags
        of |lag_fake - lag_real|; 'motion_precision', 'motion_recall', 'motion_density', 'motion_coverage': KnnMetrics.report on
        the motion descriptors -- whether the generator produces the frame-to-frame changes the data has}"""
        if (real.shape[0], real.shape[3], real.pool) != (fake.shape[0], fake.shape[3], fake.pool):
            raise ValueError('the sets differ in frames, channels or pool')
        sr, sf = self.summary(real), self.summary(fake)
        motion = self.knn.report(real.motion, fake.motion)
        out = {'real': sr, 'fake': sf, 'acd_ratio': sf['acd'] / sr['acd'] if sr['acd'] != 0 else None,
               'lag_l1': float(np.mean(np.abs(np.asarray(sf['lag']) - np.asarray(sr['lag']))))}
        out.update({'motion_' + key: motion[key] for key in ('precision', 'recall', 'density', 'coverage')})
        return out

    def _self_dist(self, x):
        out = torch.empty(x.n, x.n, dtype=torch.int32, device=self.device)
        return hl.knn_sqdist(x.desc, x.norms, x.desc, x.norms, out).cpu().numpy().astype(np.int64)

    def grid_report(self, s, K):
        """s holds K^2 clips in content-major order: clip c K + m has content code c and motion path m.  From the exact K^2 x K^2
        distance matrices of the whole-clip descriptors (appearance) and of the motion descriptors, the means over the ordered
        pairs (same content, other motion), (other content, same motion), (neither), and their ratios (None over a zero):
        content_ratio = appearance same_content / neither (small: the content code sets the appearance), motion_leak = appearance
        same_motion / neither (near 1: the motion path does not), motion_ratio = motion same_motion / neither (small: the path sets
        the motion whatever the content), content_leak = motion same_content / neither (near 1: the content code does not).
        'appearance_dist' and 'motion_dist' are the two matrices (int64, host)."""
        if K < 2 or s.n != K * K:
            raise ValueError('a K x K grid (K >= 2) holds K^2 clips, got K = %d and %d clips' % (K, s.n))
        idx = np.arange(K * K)
        c, m = idx // K, idx % K
        same_c, same_m = c[:, None] == c[None, :], m[:, None] == m[None, :]
        masks = {'same_content': same_c & ~same_m, 'same_motion': ~same_c & same_m, 'neither': ~same_c & ~same_m}
        means = lambda dist: {key: int(dist[mask].sum()) / int(mask.sum()) for key, mask in masks.items()}
        app_dist, mot_dist = self._self_dist(s.clips), self._self_dist(s.motion)
        app, mot = means(app_dist), means(mot_dist)
        ratio = lambda a, b: a / b if b != 0 else None
        return {'content_ratio': ratio(app['same_content'], app['neither']), 'motion_leak': ratio(app['same_motion'], app['neither']),
                'motion_ratio': ratio(mot['same_motion'], mot['neither']), 'content_leak': ratio(mot['same_content'], mot['neither']),
                'appearance_means': app, 'motion_means': mot, 'appearance_dist': app_dist, 'motion_dist': mot_dist}
