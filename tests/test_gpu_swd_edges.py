"""GPU checks of the metric kernels (csrc/metrics.hip) past the sizes of tests/test_gpu_swd.py: more than one tile and every
accumulator register of the projection, every launch pattern of the sort's wide steps up to 16 local spans, the statistics,
normalisation, fold and distance loops past one trip, the gather's ragged last block, high counter word and modulus 1, a second
block and a zero column of the unit columns, C = 2 throughout -- and one chain above every one of those edges at once.
Every operand, output and workspace of a stage call is a view into ONE guard.Arena (NaN-poisoned margins; outputs start as poison),
arena.check() follows every launch sequence, and inputs a call does not write are compared bit for bit with a snapshot.
References are float64 / math.fsum statements of tests/swd_ref.py; every bound is derived there or where it is used; each test
prints its figures before it asserts."""
import math

import numpy as np
import pytest
import torch

import guard
import swd_ref as sr

pytestmark = pytest.mark.gpu
SEED = 5
U = 2.0 ** -24
POISON = np.uint32(guard.POISON)


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    assert torch.cuda.is_available()
    return hiplib


@pytest.fixture(scope="module")
def _arena():
    return guard.Arena(64 << 20)


@pytest.fixture()
def arena(_arena):
    _arena.reset()
    return _arena


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


def host64(t):
    return t.cpu().numpy().astype(np.float64)


def bits(t):
    """the bit patterns of a device tensor or host array of 4- or 8-byte elements, on the host"""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def workspace(hl, arena, n, d, rows):
    """the stages' scratch at exactly mcg_swd_workspace_bytes (a multiple of 16), poisoned"""
    nbytes = hl.load().mcg_swd_workspace_bytes(n, d, rows)
    assert nbytes > 0 and nbytes % 16 == 0
    return arena.empty((nbytes // 8,), torch.float64)


def pyramid(hl, arena, u8):
    """mcg_swd_pyramid with clips and levels inside the arena -> the levels [N][T][h][h][4]"""
    n, t, h, w, c = u8.shape
    clips = arena.put(dev(u8))
    lv = [arena.empty((n, t, s, s, 4)) for s in sr.LEVELS]
    hl._check(hl.load().mcg_swd_pyramid(n, c, t, h, w, hl._p(clips, torch.uint8), hl._p(lv[0]), hl._p(lv[1]), hl._p(lv[2]), hl._stream()),
              "mcg_swd_pyramid")
    arena.check()
    assert np.array_equal(clips.cpu().numpy(), u8)
    return lv


# ---- 1. projection -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,K", [(128, 64, 128), (129, 33, 136), (1, 1, 1), (127, 32, 129), (257, 31, 300), (130, 147, 128)])
def test_projection_every_register_and_tile(hl, arena, n, D, K):
    """every element within D 2^-24 (|A| @ |dirs|) of float64 (swd_ref.projection_bound: the classical bound of an fp32 dot
    product of length D, whatever the summation order; at D = 1 it is the one rounding of the product).  (128, 64, 128): one full
    tile, all 16 registers of all four sub-tiles of all four waves stored; (129, 33, 136): a second row and a second direction
    tile, both ragged, a D tail of one; (127, 32, 129): one chunk, no prefetch; (257, 31, 300): three direction tiles; (130, 147,
    128): the production D."""
    rng = np.random.default_rng(1000 * n + 10 * D + K)
    A32 = rng.standard_normal((n, D)).astype(np.float32)
    B32 = sr.unit_columns(rng.standard_normal((D, K))).astype(np.float32)
    desc, dirs = arena.put(dev(A32)), arena.put(dev(B32))
    out = arena.empty((K, n + 3))
    hl.swd_project(desc, dirs, out)
    arena.check()
    assert np.array_equal(bits(desc), bits(A32)) and np.array_equal(bits(dirs), bits(B32))
    got = out.cpu().numpy()
    A, B = A32.astype(np.float64), B32.astype(np.float64)
    ref, bound = (A @ B).T, sr.projection_bound(A, B).T
    err = np.abs(got[:, :n].astype(np.float64) - ref)
    ratio = (err / bound).max()
    print("projection n=%d D=%d K=%d: max err / bound = %.3f; max |err| %.3e" % (n, D, K, ratio, err.max()))
    assert not np.isnan(got[:, :n]).any()                            # every element written
    assert (err <= bound).all()
    assert np.array_equal(bits(got[:, n:]), np.full((K, 3), POISON))  # beyond n, within the stride: still poison


# ---- 2. sort -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", ['4L+1', '8L+5'])
def test_sort_rows_through_every_wide_launch_pattern(hl, arena, length):
    """4 L + 1 pads to 8 L: stage 4 L is a two-step launch with descending quadruples, stage 8 L a two-step launch followed by a
    one-step launch; 8 L + 5 pads to 16 L, whose last stage is two two-step launches (tests/test_swd_cpu.py runs the same schedule
    in NumPy).  Bit-equal to np.sort per row; with NaN in a row only: the output is a permutation of the input's bit patterns."""
    L = hl.sort_local_span()
    n = {'4L+1': 4 * L + 1, '8L+5': 8 * L + 5}[length]
    rng = np.random.RandomState(n)
    pad = 5
    for rows in (1, 3):
        base = rng.randn(rows, n).astype(np.float32)
        with_inf = base.copy()
        with_inf[:, ::7] = np.inf
        with_inf[:, 3::11] = -np.inf
        with_nan = base.copy()
        with_nan[:, [0, n // 3, n - 1]] = np.nan
        with_nan[:, L + 1] = np.uint32(0xffc12345).view(np.float32)   # (a negative NaN with a payload)
        kinds = {'random': base, 'sorted': np.sort(base, axis=1), 'reversed': np.sort(base, axis=1)[:, ::-1], 'equal': np.full((rows, n), 2.5, np.float32),
                 'inf': with_inf, 'duplicates': rng.randint(-3, 4, (rows, n)).astype(np.float32), 'nan': with_nan}
        for name, x in kinds.items():
            arena.reset()
            ws = workspace(hl, arena, n, 1, rows)
            t = arena.empty((rows, n + pad))
            t[:, :n] = dev(x)
            hl.sort_rows(t, n, ws)
            arena.check()
            got = bits(t)
            assert np.array_equal(got[:, n:], np.full((rows, pad), POISON)), (name, rows, n)       # the stride elements: untouched
            if name == 'nan':
                assert np.array_equal(np.sort(got[:, :n], axis=1), np.sort(bits(x), axis=1)), (name, rows, n)
            else:
                want = bits(np.sort(x, axis=1))
                bad = np.argwhere(got[:, :n] != want)
                print("sort n=%d rows=%d %s: %d elements differ%s" % (n, rows, name, len(bad), (", first at %s" % bad[0]) if len(bad) else ""))
                assert len(bad) == 0, (name, rows, n)


# ---- 3. channel sums, fold and normalisation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,C", [(14300, 147, 3), (476, 147, 3), (50, 98, 2), (300, 49, 1)])
def test_channel_sums_and_normalisation_past_one_trip(hl, arena, n, D, C):
    """channel c is N(10 (c + 1), 1) rounded to fp32, so a misassigned channel moves a sum grossly.  (14300, 147): 2 102 100
    elements -- 9 trips of the statistics' 1024 x 256 threads (step mod 3 = 1) and a second trip of the normalisation's 8192 x 256
    (step mod 3 = 2), so both wrap statements run, and the fold adds 4 partials per thread.  (476, 147): 69 972 elements (no
    multiple of 3 is nearer 70 000) in 274 blocks -- the fold's loop passes 256 partials with one trip per statistics thread.
    Sums against math.fsum within swd_ref.double_sum_bound; normalised values within 2^-21 max(1, |ref|) of float64 (the device
    evaluates (v - mean) / std in double from those sums and rounds once)."""
    total = n * D
    rng = np.random.default_rng(n + D + C)
    x = (10.0 * (np.arange(total) % C + 1) + rng.standard_normal(total)).astype(np.float32).reshape(n, D)
    blocks, trips = sr.reduction_blocks(total), sr.reduction_trips(total)
    if n == 14300:
        assert trips == 9 and total > sr.NORM_BLOCKS * sr.RED_THREADS and sr.reduction_trips(total, sr.NORM_BLOCKS) == 2
    if n == 476:
        assert 256 < blocks < sr.RED_BLOCKS and trips == 1
    desc = arena.put(dev(x))
    ws = workspace(hl, arena, n, D, 1)
    sums = arena.empty((2 * C,), torch.float64)
    hl.swd_channel_sums(desc, C, ws, sums)
    arena.check()
    assert np.array_equal(bits(desc), bits(x))
    got = sums.cpu().numpy()
    v = x.astype(np.float64).reshape(-1, C)
    worst = 0.0
    for c in range(C):
        for k, terms in ((c, v[:, c]), (C + c, v[:, c] * v[:, c])):                        # (squares of fp32 values: exact doubles)
            ref, bound = math.fsum(terms), sr.double_sum_bound(total, math.fsum(np.abs(terms)))
            err = abs(got[k] - ref)
            worst = max(worst, err / bound)
            print("sums n=%d D=%d C=%d [%d]: %.17g (ref %.17g), |err| %.3e, bound %.3e" % (n, D, C, k, got[k], ref, err, bound))
            assert err <= bound
    print("sums n=%d D=%d C=%d: blocks %d, trips %d, worst err / bound %.3f" % (n, D, C, blocks, trips, worst))
    snap = bits(sums)
    hl.swd_normalize(desc, C, sums)
    arena.check()
    assert np.array_equal(bits(sums), snap)
    ref = sr.normalize(x.astype(np.float64), C)
    ratio = (np.abs(host64(desc) - ref) / np.maximum(1.0, np.abs(ref))).max()
    print("normalise n=%d D=%d C=%d: max err / max(1,|ref|) = %.3e (bound %.3e)" % (n, D, C, ratio, 2.0 ** -21))
    assert ratio <= 2.0 ** -21


# ---- 4. distance -----------------------------------------------------------------------------------------------------------------
def test_distance_past_one_trip(hl, arena):
    """K = 2 rows of n = 262 144 + 77: the last 77 elements of each row are a thread's second trip.  The terms |a - b| are
    non-negative, so the relative error is at most the depth of the sum times 2^-53 (about 3e-15, printed); asserted is 1e-12, the
    bound tests/test_gpu_swd.py holds the same call to.  The strides differ and their elements hold NaN: a read past n would show."""
    K, n = 2, 262144 + 77
    rng = np.random.default_rng(77)
    xa, xb = (rng.standard_normal((K, n)).astype(np.float32) for _ in range(2))
    a, b = arena.empty((K, n + 5)), arena.empty((K, n + 9))
    a[:, :n], b[:, :n] = dev(xa), dev(xb)
    snap_a, snap_b = bits(a), bits(b)
    ws = workspace(hl, arena, n, 1, 1)
    out = arena.empty((3,), torch.float64)
    assert sr.reduction_trips(n) == 2
    hl.swd_distance(a, b, n, ws, out[0:1])
    hl.swd_distance(b, a, n, ws, out[1:2])
    hl.swd_distance(a, a, n, ws, out[2:3])
    arena.check()
    assert np.array_equal(bits(a), snap_a) and np.array_equal(bits(b), snap_b)
    ab, ba, aa = out.cpu().numpy()
    terms = np.abs(xa.astype(np.float64) - xb.astype(np.float64)).reshape(-1)
    want = math.fsum(terms) / (K * n)
    print("distance n=%d: %.17g (ref %.17g), rel err %.3e (bound 1e-12; derived %.1e)" % (
        n, ab, want, abs(ab - want) / want, (K * sr.reduction_trips(n) + 22) * 2.0 ** -53))   # K trips' additions, 8 + 4 + 8, scale, fsum
    assert abs(ab - want) <= 1e-12 * want
    assert aa == 0.0                                                 # exactly
    assert bits(out[0:1])[0] == bits(out[1:2])[0]                    # symmetric bit for bit


# ---- 5. gather, unit columns, pyramid --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,pt,first", [(3, 1, 0), (3, 2, 1 << 32), (1, 4, 0), (2, 4, 1 << 32), (2, 1, 0)],
                         ids=['ragged', 'high-word', 'pt=T', 'C=2-pt=T-high-word', 'C=2'])
def test_gather_ragged_high_counter_word_and_modulus_one(hl, arena, C, pt, first):
    """3 clips of 5 patches: 15 rows, so the last block of four has three missing rows (and the 2 + 1 split ends in blocks of two
    and one).  first = 2^32 at P = 5 makes the Philox counter's high word 5.  pt = T = 4 draws the frame modulo one.  Every level
    (64, 32 and 16 pixels) is bit-equal to indexing the device's own level at swd_ref.positions."""
    N, P = 3, 5
    u8 = sr.fixed_sets(C)[0]
    lv = pyramid(hl, arena, u8)
    D = pt * 49 * C
    for li, s in enumerate(sr.LEVELS):
        snap = bits(lv[li])
        one, two_a, two_b = arena.empty((N * P, D)), arena.empty((2 * P, D)), arena.empty((P, D))
        hl.swd_gather(lv[li], C, first, P, pt, SEED, sr.position_stream(li), one)
        hl.swd_gather(lv[li][:2], C, first, P, pt, SEED, sr.position_stream(li), two_a)
        hl.swd_gather(lv[li][2:], C, first + 2, P, pt, SEED, sr.position_stream(li), two_b)
        arena.check()
        assert np.array_equal(bits(lv[li]), snap)
        want = sr.gather(host64(lv[li])[..., :C], first, P, pt, SEED, sr.position_stream(li)).astype(np.float32)
        t0 = sr.positions(first, N, P, pt, u8.shape[1], s, SEED, sr.position_stream(li))[0]
        print("gather C=%d pt=%d first=%d level %d: %d of %d elements differ; frame origins %d..%d" % (
            C, pt, first, s, int((bits(one) != bits(want)).sum()), want.size, t0.min(), t0.max()))
        assert want.shape == (N * P, D) and np.array_equal(bits(one), bits(want)), s
        assert np.array_equal(np.concatenate([bits(two_a), bits(two_b)]), bits(one)), s    # 2 + 1 clips == one call
        assert (t0.max() == 0) == (pt == u8.shape[1])


def test_unit_columns_second_block_and_zero_column(hl, arena):
    """K = 300 columns take a second block of 256 threads; column 17 is all zeros and stays so (no 0 / 0).  | ||d|| - 1 | <= 2^-20
    and |d - ref| <= 2^-24 as in tests/test_gpu_swd.py: every element is the double quotient rounded once, and |d| <= 1."""
    D, K = 147, 300
    raw = np.random.default_rng(17).standard_normal((D, K)).astype(np.float32)
    raw[:, 17] = 0.0
    d = arena.put(dev(raw))
    hl.swd_unit_columns(d)
    arena.check()
    col = host64(d)
    live = np.arange(K) != 17
    norm = np.sqrt((col * col).sum(0))
    ref = sr.unit_columns(raw[:, live])
    print("unit columns D=%d K=%d: max | ||d|| - 1 | = %.3e (bound %.3e); max |d - ref| = %.3e (bound %.3e)" % (
        D, K, np.abs(norm[live] - 1).max(), 2.0 ** -20, np.abs(col[:, live] - ref).max(), U))
    assert np.abs(norm[live] - 1).max() <= 2.0 ** -20
    assert np.abs(col[:, live] - ref).max() <= U
    assert np.array_equal(bits(d)[:, 17], np.zeros(D, np.uint32))    # exactly zero


def test_pyramid_two_channels(hl, arena):
    """C = 2 on random uint8 frames: |err| <= 2^-11 against float64 (the bound derived at tests/test_gpu_swd.py's pyramid test),
    pad channels 2 and 3 zero"""
    C = 2
    clips = np.random.RandomState(2).randint(0, 256, (2, 3, 64, 64, C)).astype(np.uint8)
    ref = sr.pyramid(clips)
    for s, g in zip(sr.LEVELS, pyramid(hl, arena, clips)):
        g = host64(g)
        err = np.abs(g[..., :C] - ref[s]).max()
        print("pyramid C=2 level %d: max |err| %.3e (bound %.3e)" % (s, err, 2.0 ** -11))
        assert err <= 2.0 ** -11
        assert np.array_equal(bits(g[..., C:].astype(np.float32)), np.zeros(g[..., C:].shape, np.uint32))


# ---- 6. one chain above every edge at once -------------------------------------------------------------------------------------
def test_whole_chain_above_every_edge(hl, arena):
    """SlicedWasserstein(patches=10923, patch_frames=1, repeats=1, dirs=136) on the fixed sets at C = 3: n = 3 x 10923 = 32769 =
    4 L + 1 rows of D = 147 (4.8 M elements: 19 statistics trips, 3 normalisation trips), two direction tiles, sort rows padded to
    8 L, a distance of 129 blocks.  The class owns its buffers (it is the product path); the arena holds what this test calls
    itself -- the pyramids the reference indexes and the normals it is given.  Tolerance as in tests/test_gpu_swd.py's chain:
    errA + errB, err_X = max (D + 8) 2^-24 (|desc_X| @ |dirs|), since sorting is 1-Lipschitz in the max norm."""
    from mocogan_chainer_amd.metrics import SlicedWasserstein
    C, P, K = 3, 10923, 136
    ua, ub = sr.fixed_sets(C)
    swd = SlicedWasserstein(patches=P, patch_frames=1, repeats=1, dirs=K, seed=SEED)
    a, b = swd.descriptors([ua]), swd.descriptors([ub])
    assert (a.n, a.dim) == (4 * hl.sort_local_span() + 1, 147)
    got = swd.distance(a, b)
    lv64 = [{s: host64(l)[..., :C] for s, l in zip(sr.LEVELS, pyramid(hl, arena, u8))} for u8 in (ua, ub)]
    raws = {}
    for li in range(3):
        d = arena.empty((147, K))
        hl.randn(d, 1.0, SEED, sr.direction_stream(li, 0))
        raws[li] = host64(d)
    arena.check()
    ra, rb = sr.descriptors(lv64[0], C, P, 1, SEED), sr.descriptors(lv64[1], C, P, 1, SEED)
    ref = sr.distance(ra, rb, 1, K, SEED, raw=lambda li, r, D, K_: raws[li])
    for li, s in enumerate(sr.LEVELS):
        dirs = sr.unit_columns(raws[li])
        tol = sr.projection_bound(ra[s], dirs, 8).max() + sr.projection_bound(rb[s], dirs, 8).max()
        err = abs(got[str(s)] - ref[str(s)]) * 1e-3
        print("edge chain level %d: swd %.6f (ref %.6f) x1e-3, |err| %.3e, tol %.3e, err / tol %.2e, ref / tol %.0f" % (
            s, got[str(s)], ref[str(s)], err, tol, err / tol, ref[str(s)] * 1e-3 / tol))
        assert err <= tol
        assert ref[str(s)] * 1e-3 >= 100 * tol                       # (tests/test_swd_cpu.py checks the same of the reference's levels)
    assert got['avg'] == sum(got[str(s)] for s in sr.LEVELS) / 3
