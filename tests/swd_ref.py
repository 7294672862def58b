"""float64 NumPy statement of the sliced Wasserstein distance over Laplacian-pyramid patches (TEST INFRASTRUCTURE; the device
statement is mocogan-chainer_amd/csrc/metrics.hip, the specification include/mocogan_hip.h).  Karras et al. 2018, "Progressive
Growing of GANs", section 5.  Draws come from oracle.philox with the stream ids restated here."""
import numpy as np

from oracle import philox

LEVELS = (64, 32, 16)
STREAM_BASE = 0x535744 << 32
F5 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def position_stream(level_index):
    return STREAM_BASE + level_index


def direction_stream(level_index, repeat):
    return STREAM_BASE + ((level_index + 1) << 24) + repeat


# ---- 1. pyramid ---------------------------------------------------------------------------------------------------------------
def blur(x, gain=1.0):
    """x (..., H, W) convolved with gain * F5 (x) F5, boundary d c b | a b c d | c b a (scipy 'mirror', NumPy 'reflect')"""
    H, W = x.shape[-2:]
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(2, 2), (2, 2)], mode='reflect')
    out = np.zeros_like(x, dtype=np.float64)
    for i in range(5):
        for j in range(5):
            out += (gain * F5[i] * F5[j]) * p[..., i:i + H, j:j + W]
    return out


def down(x):
    return blur(x)[..., ::2, ::2]


def up(x):
    z = np.zeros(x.shape[:-2] + (2 * x.shape[-2], 2 * x.shape[-1]))
    z[..., ::2, ::2] = x
    return blur(z, 4.0)


def pyramid(clips_u8):
    """uint8 (N,T,64,64,C) -> {64: L64, 32: L32, 16: L16}, each (N,T,h,h,C) float64; the coarsest level is the low-pass itself"""
    g64 = np.asarray(clips_u8).astype(np.float64).transpose(0, 1, 4, 2, 3)
    g32 = down(g64)
    g16 = down(g32)
    back = lambda a: np.ascontiguousarray(a.transpose(0, 1, 3, 4, 2))
    return {64: back(g64 - up(g32)), 32: back(g32 - up(g16)), 16: back(g16)}


# ---- 2. descriptors -----------------------------------------------------------------------------------------------------------
def positions(first, n_clips, P, pt, T, hw, seed, stream_id):
    """(t0, y0, x0) of the rows of clips first .. first + n_clips: row j of clip i takes Philox counter i * P + j"""
    g = (np.uint64(first) * np.uint64(P) + np.arange(n_clips * P, dtype=np.uint64))
    z = np.zeros(len(g), np.uint32)
    w = philox.philox4x32_10((g & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32),
                             z + np.uint32(stream_id & 0xFFFFFFFF), z + np.uint32(stream_id >> 32), seed & 0xFFFFFFFF, seed >> 32)
    return (w[0] % np.uint32(T - pt + 1)).astype(np.int64), (w[1] % np.uint32(hw - 6)).astype(np.int64), \
        (w[2] % np.uint32(hw - 6)).astype(np.int64)


def gather(level, first, P, pt, seed, stream_id):
    """level (N,T,h,h,C) -> (N*P, pt*49*C): element ((dt*7+dy)*7+dx)*C + c of a row is level[i][t0+dt][y0+dy][x0+dx][c]"""
    N, T, hw = level.shape[:3]
    t0, y0, x0 = positions(first, N, P, pt, T, hw, seed, stream_id)
    rows = [level[r // P, t0[r]:t0[r] + pt, y0[r]:y0[r] + 7, x0[r]:x0[r] + 7, :].reshape(-1) for r in range(N * P)]
    return np.stack(rows)


# ---- 3. normalisation ---------------------------------------------------------------------------------------------------------
def channel_sums(desc, C):
    v = np.asarray(desc, np.float64).reshape(-1, C)
    return np.concatenate([v.sum(0), (v * v).sum(0)])


def normalize(desc, C):
    """per channel: subtract the mean, divide by the population standard deviation; a constant channel (variance not above 1e-12 of
    the mean square) becomes zeros, where ProGAN's NumPy would write NaN"""
    v = np.asarray(desc, np.float64).reshape(desc.shape[0], -1, C)
    mean, var, ms = v.mean((0, 1)), v.var((0, 1)), (v * v).mean((0, 1))
    inv = np.where(var > 1e-12 * ms, 1.0 / np.sqrt(np.where(var > 0, var, 1.0)), 0.0)
    return ((v - mean) * inv).reshape(desc.shape)


def descriptors(levels, C, P, pt, seed, first=0):
    return {s: normalize(gather(levels[s], first, P, pt, seed, position_stream(li)), C) for li, s in enumerate(LEVELS)}


# ---- 4. directions ------------------------------------------------------------------------------------------------------------
def raw_directions(level_index, repeat, D, K, seed):
    return philox.randn(D * K, 1.0, seed, direction_stream(level_index, repeat)).reshape(D, K)


def unit_columns(raw):
    raw = np.asarray(raw, np.float64)
    return raw / np.sqrt((raw * raw).sum(0, keepdims=True))


# ---- 5. project, sort, compare ------------------------------------------------------------------------------------------------
def sliced_distance(desc_a, desc_b, dirs):
    """mean over directions and ranks of |sorted projection of a - sorted projection of b|"""
    pa, pb = np.sort(desc_a @ dirs, axis=0), np.sort(desc_b @ dirs, axis=0)
    return float(np.abs(pa - pb).mean())


def distance(desc_a, desc_b, R, K, seed, raw=None):
    """{'64', '32', '16', 'avg'} x 1e3.  raw(level_index, repeat, D, K) supplies the normals the directions are made of (default:
    the oracle's statement of the device's draw)."""
    raw = raw or (lambda li, r, D, K_: raw_directions(li, r, D, K_, seed))
    res = {}
    for li, s in enumerate(LEVELS):
        D = desc_a[s].shape[1]
        res[str(s)] = 1e3 * float(np.mean([sliced_distance(desc_a[s], desc_b[s], unit_columns(raw(li, r, D, K))) for r in range(R)]))
    res['avg'] = float(np.mean([res[str(s)] for s in LEVELS]))
    return res


def projection_bound(desc, dirs, extra=0):
    """the classical bound of an fp32 dot product of length D against float64, per element: (D + extra) 2^-24 (|desc| @ |dirs|);
    it holds for any summation order"""
    return (desc.shape[1] + extra) * 2.0 ** -24 * (np.abs(desc) @ np.abs(dirs))


# ---- 6. the reductions' launch geometry and error bound -----------------------------------------------------------------------
RED_THREADS, RED_BLOCKS, NORM_BLOCKS = 256, 1024, 8192    # metrics.hip: NT, RED_BLOCKS, the grid cap of mcg_swd_normalize


def reduction_blocks(total, cap=RED_BLOCKS):
    """blocks of the statistics / distance partial pass over `total` elements (`cap` blocks of 256 threads at most)"""
    return min(cap, -(-total // RED_THREADS))


def reduction_trips(total, cap=RED_BLOCKS):
    """the most elements one thread of that pass adds: ceil(total / (blocks * 256)); above one the grid-stride loop repeats"""
    return -(-total // (reduction_blocks(total, cap) * RED_THREADS))


def double_sum_bound(total, abs_sum):
    """|device sum - math.fsum| <= (trips + 24) 2^-53 fsum(|terms|) for the two-pass double sums of metrics.hip over `total` terms.
    A term passes through at most `trips` additions in its thread, 8 levels of the block's tree, ceil(blocks / 256) <= 4 additions
    of the fold kernel's thread and 8 more tree levels: depth d <= trips + 20, and a sum whose every term passes through at most d
    roundings of 2^-53 errs by at most ((1 + 2^-53)^d - 1) sum |terms| = d 2^-53 sum |terms| (1 + 1e-14).  The terms themselves are
    exact (an fp32 value, the square of one, the difference of two of like magnitude are doubles).  One of the four spare units is
    the rounding of math.fsum's own result; the others are slack, not measured."""
    return (reduction_trips(total) + 24) * 2.0 ** -53 * abs_sum


# ---- 7. the launch schedule of mcg_sort_rows, emulated -------------------------------------------------------------------------
def sort_rows_emulation(x, L):
    """one row through the launch schedule of mcg_sort_rows with a local span of L: (the sorted row, the launches as
    ('local_full',), ('global', k, j), ('global2', k, j), ('local', k)).  Element i meets i ^ j in step j and sorts ascending in
    stage k where (i & k) == 0; a 'global2' launch is the steps j and j / 2, a 'local' launch the steps L / 2 .. 1 of its stage."""
    x = np.asarray(x)
    n2 = 2
    while n2 < len(x):
        n2 <<= 1
    v = np.full(n2, np.inf, x.dtype)
    v[:len(x)] = x
    idx = np.arange(n2)

    def step(k, j):
        lo = idx[(idx & j) == 0]
        a, b = v[lo], v[lo | j]
        swap = (a > b) == ((lo & k) == 0)
        v[lo], v[lo | j] = np.where(swap, b, a), np.where(swap, a, b)

    launches = [('local_full',)]
    k = 2
    while k <= min(L, n2):
        j = k >> 1
        while j > 0:
            step(k, j)
            j >>= 1
        k <<= 1
    while k <= n2:
        j = k >> 1
        while j >= L:
            if (j >> 1) >= L:
                launches.append(('global2', k, j))
                step(k, j)
                step(k, j >> 1)
                j >>= 2
            else:
                launches.append(('global', k, j))
                step(k, j)
                j >>= 1
        launches.append(('local', k))
        while j > 0:
            step(k, j)
            j >>= 1
        k <<= 1
    return v[:len(x)], launches


# ---- the fixed test sets ------------------------------------------------------------------------------------------------------
def blob_clips(N, T, C, seed, contrast=1.0, smooth=6):
    """smooth random blobs as uint8 clips (N,T,64,64,C): white noise, `smooth` passes of a [1,2,1]/4 blur per axis (wrapping), scaled
    to a standard deviation of 48 * contrast around 128, drifting one pixel per frame"""
    rng = np.random.RandomState(seed)
    x = rng.randn(N, 1, 64, 64, C)
    for _ in range(smooth):
        for ax in (2, 3):
            x = 0.25 * np.roll(x, 1, ax) + 0.5 * x + 0.25 * np.roll(x, -1, ax)
    x = x / x.std()
    x = np.concatenate([np.roll(x, t, 3) for t in range(T)], axis=1)
    x = x + 0.05 * rng.randn(N, T, 64, 64, C)                      # (a little pixel noise: no exactly constant region)
    return np.clip(128 + 48 * contrast * x, 0, 255).astype(np.uint8)


def fixed_sets(C):
    """the 'real' and 'fake' sets of the tests: N = 3, T = 4; the fake set has another contrast and blur"""
    return blob_clips(3, 4, C, 100 + C), blob_clips(3, 4, C, 200 + C, contrast=0.6, smooth=2)
