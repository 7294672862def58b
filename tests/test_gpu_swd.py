"""GPU checks of the sliced Wasserstein distance (csrc/metrics.hip) against the float64 statement of tests/swd_ref.py, stage by
stage and as a whole chain, on sets of N = 3 clips of T = 4 frames, C in {1, 3}, P = 16 patches, pt in {1, 2}, R = 2, K = 8.
Every tolerance is derived where it is used; each test prints its figures before it asserts."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import swd_ref as sr

pytestmark = pytest.mark.gpu
N, T, P, R, K, SEED = 3, 4, 16, 2, 8, 5
U = 2.0 ** -24


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    assert torch.cuda.is_available()
    return hiplib


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device='cuda')


def host64(t):
    return t.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def device_levels(C):
    """the fixed sets and the DEVICE's pyramid of each: (u8, [l64, l32, l16] tensors, {hw: float64 (N,T,h,h,C)}) for real and fake"""
    import mocogan_chainer_amd.hiplib as hiplib
    out = []
    for u8 in sr.fixed_sets(C):
        lv = hiplib.swd_pyramid(dev(u8))
        out.append((u8, lv, {s: host64(l)[..., :C] for s, l in zip(sr.LEVELS, lv)}))
    return out


def raw_descriptors(hl, levels, C, pt, first=0):
    """device gather of every level: list of [n][D] tensors"""
    out = []
    for li, lv in enumerate(levels):
        o = torch.empty(lv.shape[0] * P, pt * 49 * C, dtype=torch.float32, device='cuda')
        out.append(hl.swd_gather(lv, C, first, P, pt, SEED, sr.position_stream(li), o))
    return out


def normalised(hl, raw, C):
    ws = hl.swd_workspace(raw[0].shape[0], raw[0].shape[1], 1, 'cuda')
    out = []
    for d in raw:
        d = d.clone()
        out.append(hl.swd_normalize(d, C, hl.swd_channel_sums(d, C, ws)))
    return out


def unit_dirs(hl, li, r, D):
    """(the device's raw normals, its unit directions) of (level, repeat)"""
    d = torch.empty(D, K, dtype=torch.float32, device='cuda')
    hl.randn(d, 1.0, SEED, sr.direction_stream(li, r))
    raw = d.clone()
    return raw, hl.swd_unit_columns(d)


def by_hand(hl, desc_a, desc_b):
    """the stage calls of SlicedWasserstein.distance made one by one -> ({level: x 1e3}, the raw normals per (level, repeat))"""
    n, D = desc_a[0].shape
    ws = hl.swd_workspace(n, D, K, 'cuda')
    pa, pb = (torch.empty(K, n, dtype=torch.float32, device='cuda') for _ in range(2))
    out = torch.zeros(3 * R, dtype=torch.float64, device='cuda')
    raws = {}
    for li in range(3):
        for r in range(R):
            raws[li, r], d = unit_dirs(hl, li, r, D)
            hl.sort_rows(hl.swd_project(desc_a[li], d, pa), n, ws)
            hl.sort_rows(hl.swd_project(desc_b[li], d, pb), n, ws)
            hl.swd_distance(pa, pb, n, ws, out[li * R + r:li * R + r + 1])
    v = out.cpu().numpy().reshape(3, R)
    res = {str(s): float(np.sum(v[li]) / R * 1e3) for li, s in enumerate(sr.LEVELS)}
    res['avg'] = float(sum(res[str(s)] for s in sr.LEVELS) / 3)
    return res, raws


# ---- pyramid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
def test_pyramid_against_float64(hl, C):
    """absolute error <= 2^-11 on values of range +-255: at most 6 separable passes and one subtraction, 5 roundings each, each at
    most half an ulp of 255 (2^-17): about 45 * 2^-17 = 3.4e-4 < 2^-11 = 4.9e-4.  A wrong tap or boundary errs by at least 1/16."""
    rng = np.random.RandomState(3)
    clips = np.zeros((2, 4, 64, 64, C), np.uint8)
    clips[0, 0] = 200                                                # constant
    for k, (y, x) in enumerate(((0, 0), (0, 63), (63, 0), (63, 63))):
        clips[0, 1, y, x, k % C] = 255                               # a single bright pixel in each corner, one frame
        clips[1, k % 2, y, x, :] = 255 - 40 * k                      # ... and spread over frames
    clips[0, 2] = rng.randint(0, 256, (64, 64, C))                   # random
    clips[0, 3] = rng.randint(0, 2, (64, 64, C)) * 255               # random, extreme
    clips[1, 2:] = sr.fixed_sets(C)[0][0, :2]
    ref = sr.pyramid(clips)
    got = hl.swd_pyramid(dev(clips))
    for s, g in zip(sr.LEVELS, got):
        assert tuple(g.shape) == (2, 4, s, s, 4) and g.dtype == torch.float32
        g = host64(g)
        err = np.abs(g[..., :C] - ref[s]).max()
        print("pyramid C=%d level %d: max |err| %.3e (bound %.3e), range %.1f .. %.1f" % (C, s, err, 2.0 ** -11, ref[s].min(), ref[s].max()))
        assert err <= 2.0 ** -11
        assert np.array_equal(g[..., C:], np.zeros_like(g[..., C:]))                       # the pad channels hold zeros
    assert np.array_equal(host64(got[0])[0, 0], np.zeros((64, 64, 4)))                     # a constant frame: L64 = 0 exactly
    assert np.array_equal(host64(got[2])[0, 0, :, :, :C], np.full((16, 16, C), 200.0))


# ---- gather --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,pt", [(1, 1), (3, 1), (1, 2), (3, 2)])
def test_gather_is_an_exact_copy_at_the_oracles_positions(hl, C, pt):
    (_, lv, lv64), _ = device_levels(C)
    one = raw_descriptors(hl, lv, C, pt)
    two_a = raw_descriptors(hl, [l[:2] for l in lv], C, pt, first=0)
    two_b = raw_descriptors(hl, [l[2:] for l in lv], C, pt, first=2)
    ws = hl.swd_workspace(N * P, pt * 49 * C, 1, 'cuda')
    for li, s in enumerate(sr.LEVELS):
        want = sr.gather(lv64[s], 0, P, pt, SEED, sr.position_stream(li)).astype(np.float32)
        got = one[li].cpu().numpy()
        assert got.shape == (N * P, pt * 49 * C) and np.array_equal(got, want), s          # bit-equal to indexing the device's levels
        assert torch.equal(torch.cat([two_a[li], two_b[li]]), one[li]), s                  # 2 + 1 clips == one call
        sums = hl.swd_channel_sums(one[li], C, ws).cpu().numpy()
        v = want.astype(np.float64).reshape(-1, C)
        ref = np.array([math.fsum(v[:, c]) for c in range(C)] + [math.fsum(v[:, c] ** 2) for c in range(C)])      # correctly rounded
        assert np.allclose(ref, sr.channel_sums(v, C), rtol=1e-9, atol=1e-6)
        rel = np.abs(sums - ref) / np.abs(ref)
        print("gather C=%d pt=%d level %d: sums rel err %.2e" % (C, pt, s, rel.max()))
        assert sums.shape == (2 * C,) and rel.max() <= 1e-12


# ---- normalisation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,pt", [(1, 1), (3, 2)])
def test_normalised_descriptors(hl, C, pt):
    """|got - ref| <= 2^-21 max(1, |ref|): the device evaluates (v - mean) / std in double from sums that agree with float64 to
    1e-12 and rounds once (2^-24 relative)"""
    (_, lv, _), _ = device_levels(C)
    raw = raw_descriptors(hl, lv, C, pt)
    got = normalised(hl, raw, C)
    for li, s in enumerate(sr.LEVELS):
        ref = sr.normalize(host64(raw[li]), C)
        g = host64(got[li])
        ratio = (np.abs(g - ref) / np.maximum(1.0, np.abs(ref))).max()
        print("normalise C=%d pt=%d level %d: max err / max(1,|ref|) = %.3e (bound %.3e)" % (C, pt, s, ratio, 2.0 ** -21))
        assert ratio <= 2.0 ** -21
    if C == 3:                                                       # a constant channel gives zeros (ProGAN would write NaN)
        d = raw[2].clone()
        d.view(d.shape[0], -1, C)[:, :, 1] = 7.25
        ws = hl.swd_workspace(d.shape[0], d.shape[1], 1, 'cuda')
        ref = sr.normalize(host64(d), C)
        g = host64(hl.swd_normalize(d, C, hl.swd_channel_sums(d, C, ws)))
        assert np.array_equal(g.reshape(g.shape[0], -1, C)[:, :, 1], np.zeros((g.shape[0], g.shape[1] // C)))
        assert (np.abs(g - ref) / np.maximum(1.0, np.abs(ref))).max() <= 2.0 ** -21 and np.isfinite(g).all()


# ---- directions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [49, 98, 147, 294, 441])
def test_unit_columns(hl, D):
    """| ||d||_2 - 1 | <= 2^-20: every element is the double product v / ||v|| rounded once (2^-24 relative), so the norm of the
    rounded column is within 2^-24 of one"""
    raw, d = unit_dirs(hl, 1, 0, D)
    col = host64(d)
    norm = np.sqrt((col * col).sum(0))
    ref = sr.unit_columns(host64(raw))
    print("unit columns D=%d: max | ||d|| - 1 | = %.3e (bound %.3e); max |d - ref| = %.3e" % (D, np.abs(norm - 1).max(), 2.0 ** -20, np.abs(col - ref).max()))
    assert col.shape == (D, K) and np.abs(norm - 1).max() <= 2.0 ** -20
    assert np.abs(col - ref).max() <= U
    want = sr.raw_directions(1, 0, D, K, SEED)                        # the oracle's statement of the same draw (fp32 intrinsics: 2e-5)
    assert np.abs(host64(raw) - want).max() <= 2e-5


# ---- projection ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,pt", [(1, 1), (3, 2)])
@pytest.mark.parametrize("n", [48, 130])
def test_projection_against_float64(hl, C, pt, n):
    """every element within D 2^-24 (|A| @ |dirs|) of float64 -- the classical bound of an fp32 dot product of length D, whatever
    the summation order.  D = 49 and 294 are no multiples of the kernel's K-step; n = 130 leaves a partial row tile."""
    (_, la, _), (_, lb, _) = device_levels(C)
    da, db = normalised(hl, raw_descriptors(hl, la, C, pt), C)[0], normalised(hl, raw_descriptors(hl, lb, C, pt), C)[0]
    desc = torch.cat([da, db, da])[:n].contiguous()                  # the device's normalised descriptors, 48 or 130 rows
    D = pt * 49 * C
    _, dirs = unit_dirs(hl, 0, 1, D)
    stride = n + 3
    out = torch.full((K, stride), -777.0, dtype=torch.float32, device='cuda')
    hl.swd_project(desc, dirs, out)
    got = host64(out)
    A, B = host64(desc), host64(dirs)
    ref = (A @ B).T
    bound = (D * U * (np.abs(A) @ np.abs(B))).T
    ratio = (np.abs(got[:, :n] - ref) / bound).max()
    print("projection D=%d n=%d: max err / bound = %.3f; max |err| %.3e" % (D, n, ratio, np.abs(got[:, :n] - ref).max()))
    assert ratio <= 1.0
    assert np.array_equal(got[:, n:], np.full((K, 3), -777.0))       # beyond n, within the stride: untouched


# ---- sort ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", ['1', '2', '63', '64', '1000', 'L', 'L+1', '2L+3'])
def test_sort_rows_is_numpy_sort(hl, length):
    """L is the span the kernel sorts in LDS (hiplib.sort_local_span): up to L one launch, above it the global merge passes"""
    L = hl.sort_local_span()
    n = {'L': L, 'L+1': L + 1, '2L+3': 2 * L + 3}.get(length) or int(length)
    rng = np.random.RandomState(n)
    pad, sentinel = 5, np.float32(-12345.0)
    for rows in (1, 5):
        base = rng.randn(rows, n).astype(np.float32)
        with_inf = base.copy()
        with_inf[:, ::7] = np.inf
        with_inf[:, 3::11] = -np.inf
        kinds = {'random': base, 'sorted': np.sort(base, axis=1), 'reversed': np.sort(base, axis=1)[:, ::-1], 'equal': np.full((rows, n), 2.5, np.float32),
                 'inf': with_inf, 'duplicates': rng.randint(-3, 4, (rows, n)).astype(np.float32)}
        ws = hl.swd_workspace(n, 1, rows, 'cuda')
        for name, x in kinds.items():
            buf = np.full((rows, n + pad), sentinel, np.float32)
            buf[:, :n] = x
            t = dev(buf)
            hl.sort_rows(t, n, ws)
            got = t.cpu().numpy()
            assert np.array_equal(got[:, :n], np.sort(x, axis=1)), (name, rows, n)         # bit-equal per row
            assert np.array_equal(got[:, n:], np.full((rows, pad), sentinel)), (name, rows, n)   # the padding within row_stride: untouched
    if n <= hl.sort_local_span():                                    # short rows need no workspace
        t = dev(base[:1].copy())
        hl.sort_rows(t)
        assert np.array_equal(t.cpu().numpy(), np.sort(base[:1], axis=1))


# ---- distance and the whole chain ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,pt", [(1, 1), (3, 1), (1, 2), (3, 2)])
def test_distance_and_whole_chain_from_the_devices_levels(hl, C, pt):
    """the result is within tol = errA + errB of swd_ref run on the same levels, err_X = max over elements of
    (D + 8) 2^-24 (|desc_X| @ |dirs|) in float64: sorting is 1-Lipschitz in the max norm, so the projection error bounds the
    distance error; the + 8 covers the roundings of the normalisation and of the unit columns.  The reference makes its directions
    from the normals the device drew (test_unit_columns pins those to the oracle's draw within the 2e-5 of the fp32 intrinsics --
    more than this tolerance, and a property of mcg_randn, not of this chain)."""
    (_, la, la64), (_, lb, lb64) = device_levels(C)
    da, db = normalised(hl, raw_descriptors(hl, la, C, pt), C), normalised(hl, raw_descriptors(hl, lb, C, pt), C)
    got, raws = by_hand(hl, da, db)
    ra, rb = sr.descriptors(la64, C, P, pt, SEED), sr.descriptors(lb64, C, P, pt, SEED)
    ref = sr.distance(ra, rb, R, K, SEED, raw=lambda li, r, D, K_: host64(raws[li, r]))
    D = pt * 49 * C
    for li, s in enumerate(sr.LEVELS):
        tol = max(sr.projection_bound(ra[s], sr.unit_columns(host64(raws[li, r])), 8).max() +
                  sr.projection_bound(rb[s], sr.unit_columns(host64(raws[li, r])), 8).max() for r in range(R))
        err = abs(got[str(s)] - ref[str(s)]) * 1e-3
        print("chain C=%d pt=%d D=%d level %d: swd %.6f (ref %.6f) x1e-3, |err| %.3e, tol %.3e" % (C, pt, D, s, got[str(s)], ref[str(s)], err, tol))
        assert err <= tol
        assert ref[str(s)] * 1e-3 >= 100 * tol                       # (tests/test_swd_cpu.py checks the same of the reference's levels)
    assert np.isfinite(got['avg'])
    # mcg_swd_distance on its own: the mean of |a - b| in double, to the rounding of a double sum
    n = N * P
    a, b = (dev(np.sort(np.random.RandomState(k).randn(K, n).astype(np.float32), axis=1)) for k in (1, 2))
    out = torch.zeros(1, dtype=torch.float64, device='cuda')
    hl.swd_distance(a, b, n, hl.swd_workspace(n, D, K, 'cuda'), out)
    want = np.abs(host64(a) - host64(b)).mean()
    assert abs(float(out[0]) - want) <= 1e-12 * want


# ---- properties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,pt", [(3, 1), (1, 2)])
def test_identity_symmetry_and_reproducibility(hl, C, pt):
    from mocogan_chainer_amd.metrics import SlicedWasserstein
    (ua, _, _), (ub, _, _) = device_levels(C)
    swd = SlicedWasserstein(P, pt, R, K, SEED)
    a, b = swd.descriptors([ua]), swd.descriptors([ub])
    ab, ba, aa = swd.distance(a, b), swd.distance(b, a), swd.distance(a, a)
    print("properties C=%d pt=%d: d(A,B) = %s" % (C, pt, json.dumps(ab)))
    assert aa == {'64': 0.0, '32': 0.0, '16': 0.0, 'avg': 0.0}       # exactly
    assert ab == ba                                                  # bit for bit
    a2, b2 = SlicedWasserstein(P, pt, R, K, SEED).descriptors([ua]), SlicedWasserstein(P, pt, R, K, SEED).descriptors([ub])
    assert all(torch.equal(a.desc[s], a2.desc[s]) and torch.equal(b.desc[s], b2.desc[s]) for s in sr.LEVELS)
    assert SlicedWasserstein(P, pt, R, K, SEED).distance(a2, b2) == ab                     # two runs: bit-equal
    assert all(v > 0 and np.isfinite(v) for v in ab.values())
    assert SlicedWasserstein(P, pt, R, K, SEED + 1).distance(a, b) != ab                   # (another seed: other directions)


# ---- plumbing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,pt", [(3, 2), (1, 1)])
def test_class_equals_the_stage_calls_made_by_hand(hl, C, pt):
    from mocogan_chainer_amd.metrics import SlicedWasserstein
    (ua, la, _), (ub, lb, _) = device_levels(C)
    want, _ = by_hand(hl, normalised(hl, raw_descriptors(hl, la, C, pt), C), normalised(hl, raw_descriptors(hl, lb, C, pt), C))
    swd = SlicedWasserstein(patches=P, patch_frames=pt, repeats=R, dirs=K, seed=SEED)
    a = swd.descriptors([ua[:2], dev(ua[2:])])                       # host and device chunks, 2 + 1 clips
    b = swd.descriptors(iter([ub[:1], ub[1:1], ub[1:]]))             # 1 + 0 + 2
    assert (a.n, a.dim, a.clips, a.channels) == (N * P, pt * 49 * C, N, C)
    assert swd.distance(a, b) == want                                # bit for bit
    with pytest.raises(ValueError):
        swd.distance(a, swd.descriptors([ub[:2]]))                   # unequal set sizes
    raw = swd.raw_descriptors([ua])
    half = swd.normalized(raw, 0, 2)
    assert torch.equal(half.desc[64], swd.descriptors([ua[:2]]).desc[64]) and raw.desc is not None


def test_cli_on_the_synthetic_dataset_with_a_fresh_generator(hl, tmp_path, capsys):
    import evaluate_swd
    from model.net import ImageGenerator
    from mocogan_chainer_amd import trainer
    np.random.seed(4)
    gen = ImageGenerator(n_filters=8, video_len=4)
    path = tmp_path / 'image_gen_ema_epoch_1.npz'
    trainer.save_npz(path, gen)
    common = [str(path), '--dataset_type', 'synthetic', '--synthetic_size', '16', '--num', '8', '--patches', '16', '--n_filters', '8',
              '--video_len', '4', '--repeats', '2', '--dirs', '8', '--chunk', '3', '--seed', '2']
    res = evaluate_swd.main(common + ['--baseline', '--patch_frames', '2'])
    line = [l for l in capsys.readouterr().out.splitlines() if l.startswith('{')]
    assert len(line) == 1 and json.loads(line[0]) == res             # one JSON line
    print("evaluate_swd:", line[0])
    for key in ('swd', 'baseline'):
        assert set(res[key]) == {'64', '32', '16', 'avg'} and all(np.isfinite(v) and v > 0 for v in res[key].values()), key
    assert res['baseline_clips'] == 4 and res['num'] == 8 and res['patch_frames'] == 2
    again = evaluate_swd.main(common + ['--patch_frames', '2'])
    assert again['swd'] == res['swd'] and again['baseline'] is None                        # the same run: the same numbers
    assert evaluate_swd.main(common + ['--test_mode', '0'])['swd']['avg'] > 0
