"""Sliced Wasserstein distance between two sets of uint8 clips (Karras et al. 2018, section 5), composed from the mcg_swd_* stages
of libmocogan_hip.so (include/mocogan_hip.h).  torch supplies memory and the stream; every arithmetic step is a HIP kernel.

What the number is: per pyramid level, how far the distributions of normalised 7x7(x patch_frames) Laplacian patches of the two
sets lie apart, x 1e3 as ProGAN reports it.  What it is not: it sees nothing a 7x7(x patch_frames) patch cannot see -- no global
layout, no identity, no motion beyond patch_frames frames.
"""
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
