"""CPU-only checks of the sliced Wasserstein distance: the float64 reference of tests/swd_ref.py against scipy (pyramid filter,
per-direction Wasserstein distance), its identities, the patch-position draw, the exported symbols and their host-side validation,
the CLI's parser, and the fixed test sets the GPU tests use (no constant channel; a distance far above the GPU tolerance)."""
import ctypes
import os

import numpy as np
import pytest

import swd_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('mcg_swd_workspace_bytes', 'mcg_swd_pyramid', 'mcg_swd_gather', 'mcg_swd_channel_sums', 'mcg_swd_normalize',
                'mcg_swd_unit_columns', 'mcg_swd_project', 'mcg_sort_local_span', 'mcg_sort_rows', 'mcg_swd_distance')
P, R, K, SEED = 16, 2, 8, 5            # the sizes of the GPU tests (tests/test_gpu_swd.py)


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def _ptr(addr):
    return ctypes.c_void_p(addr)       # non-null and never dereferenced: every call below fails before a launch


# ---- the reference against scipy -----------------------------------------------------------------------------------------------
def test_reference_pyramid_is_scipys_mirror_convolution():
    from scipy import ndimage
    rng = np.random.RandomState(0)
    k = np.outer(sr.F5, sr.F5)
    for hw in (64, 32, 16):
        x = rng.randint(0, 256, (hw, hw)).astype(np.float64)
        assert np.abs(sr.blur(x) - ndimage.convolve(x, k, mode='mirror')).max() <= 1e-12
        assert np.array_equal(sr.down(x), sr.blur(x)[::2, ::2])
        z = np.zeros((2 * hw, 2 * hw))
        z[::2, ::2] = x
        assert np.abs(sr.up(x) - ndimage.convolve(z, 4 * k, mode='mirror')).max() <= 1e-12
    clips = rng.randint(0, 256, (2, 3, 64, 64, 3)).astype(np.uint8)
    lv = sr.pyramid(clips)
    assert [lv[s].shape for s in sr.LEVELS] == [(2, 3, s, s, 3) for s in sr.LEVELS]
    g64 = clips[1, 2, :, :, 1].astype(np.float64)
    g32 = ndimage.convolve(g64, k, mode='mirror')[::2, ::2]
    g16 = ndimage.convolve(g32, k, mode='mirror')[::2, ::2]
    assert np.abs(lv[16][1, 2, :, :, 1] - g16).max() <= 1e-12
    z = np.zeros((64, 64))
    z[::2, ::2] = g32
    assert np.abs(lv[64][1, 2, :, :, 1] - (g64 - ndimage.convolve(z, 4 * k, mode='mirror'))).max() <= 1e-11
    # a constant frame: the Laplacian levels vanish, the coarsest level is the constant
    flat = sr.pyramid(np.full((1, 1, 64, 64, 1), 77, np.uint8))
    assert np.abs(flat[64]).max() <= 1e-12 and np.abs(flat[32]).max() <= 1e-12 and np.abs(flat[16] - 77).max() <= 1e-12


def test_reference_distance_is_scipys_wasserstein_distance_per_direction():
    from scipy import stats
    rng = np.random.RandomState(1)
    a, b = rng.randn(40, 49), 0.5 * rng.randn(40, 49) + 0.3
    dirs = sr.unit_columns(rng.randn(49, 6))
    assert np.abs(np.sqrt((dirs * dirs).sum(0)) - 1).max() <= 1e-15
    per_dir = [stats.wasserstein_distance(a @ dirs[:, k], b @ dirs[:, k]) for k in range(6)]
    assert abs(sr.sliced_distance(a, b, dirs) - np.mean(per_dir)) <= 1e-14
    assert sr.sliced_distance(a, a, dirs) == 0.0 and sr.sliced_distance(a, b, dirs) == sr.sliced_distance(b, a, dirs)


@pytest.mark.parametrize("C", [1, 3])
def test_swd_of_a_set_with_itself_is_zero(C):
    real, _ = sr.fixed_sets(C)
    d = sr.descriptors(sr.pyramid(real), C, P, 1, SEED)
    assert sr.distance(d, d, R, K, SEED) == {'64': 0.0, '32': 0.0, '16': 0.0, 'avg': 0.0}


def test_normalisation_and_the_constant_channel():
    rng = np.random.RandomState(2)
    desc = rng.randn(20, 49 * 3) * np.tile([1.0, 30.0, 0.0], 49) + np.tile([5.0, -100.0, 7.25], 49)
    out = sr.normalize(desc, 3).reshape(20, 49, 3)
    assert np.abs(out[..., :2].mean((0, 1))).max() <= 1e-13 and np.abs(out[..., :2].std((0, 1)) - 1).max() <= 1e-13
    assert np.array_equal(out[..., 2], np.zeros((20, 49)))              # zero variance -> zeros (ProGAN would write NaN)
    s = sr.channel_sums(desc, 3)
    assert np.allclose(s[:3], desc.reshape(-1, 3).sum(0)) and np.allclose(s[3:], (desc.reshape(-1, 3) ** 2).sum(0))


# ---- the draw ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pt", [1, 2, 3])
def test_position_draw_stays_inside_the_frame(pt):
    T = 4
    for li, hw in enumerate(sr.LEVELS):
        t0, y0, x0 = sr.positions(0, 64, 128, pt, T, hw, 12345, sr.position_stream(li))
        assert t0.min() == 0 and t0.max() == T - pt and (t0 + pt <= T).all()
        assert y0.min() == 0 and y0.max() == hw - 7 and x0.min() == 0 and x0.max() == hw - 7      # the bounds are met, and kept
        assert (y0 + 7 <= hw).all() and (x0 + 7 <= hw).all()
    # levels draw from streams of their own
    assert not np.array_equal(sr.positions(0, 8, 16, 1, T, 16, 1, sr.position_stream(0))[1],
                              sr.positions(0, 8, 16, 1, T, 16, 1, sr.position_stream(2))[1])


def test_chunked_and_unchunked_positions_agree():
    whole = sr.positions(0, 5, P, 2, 4, 32, SEED, sr.position_stream(1))
    parts = [sr.positions(f, n, P, 2, 4, 32, SEED, sr.position_stream(1)) for f, n in ((0, 2), (2, 1), (3, 2))]
    for k in range(3):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts]))
    real, _ = sr.fixed_sets(3)
    lv = sr.pyramid(real)
    one = sr.gather(lv[32], 0, P, 2, SEED, sr.position_stream(1))
    two = np.concatenate([sr.gather(lv[32][:2], 0, P, 2, SEED, sr.position_stream(1)), sr.gather(lv[32][2:], 2, P, 2, SEED, sr.position_stream(1))])
    assert one.shape == (3 * P, 2 * 49 * 3) and np.array_equal(one, two)
    # element ((dt*7 + dy)*7 + dx)*C + c
    t0, y0, x0 = (v[17] for v in whole)
    assert one[17, ((1 * 7 + 3) * 7 + 5) * 3 + 2] == lv[32][1, t0 + 1, y0 + 3, x0 + 5, 2]


# ---- the library ---------------------------------------------------------------------------------------------------------------
def test_header_and_library_declare_and_export_the_entry_points(hl):
    header = open(os.path.join(ROOT, 'include', 'mocogan_hip.h')).read()
    lib = hl.load()
    for name in ENTRY_POINTS:
        assert name + '(' in header, name
        assert name in hl.SIGNATURES and getattr(lib, name) is not None, name
    L = hl.sort_local_span()
    assert L >= 64 and L & (L - 1) == 0
    assert lib.mcg_swd_workspace_bytes(0, 49, 1) == 0 and lib.mcg_swd_workspace_bytes(48, 0, 1) == 0
    assert lib.mcg_swd_workspace_bytes(L, 49, 8) > 0 and lib.mcg_swd_workspace_bytes(L, 49, 8) % 16 == 0
    assert lib.mcg_swd_workspace_bytes(L + 1, 49, 8) >= 8 * 2 * L * 4           # rows padded to a power of two
    import mocogan_chainer_amd.metrics as m
    assert (m.position_stream(2), m.direction_stream(1, 3)) == (sr.position_stream(2), sr.direction_stream(1, 3))
    assert m.LEVELS == sr.LEVELS


def test_entry_points_validate_on_the_host(hl):
    lib = hl.load()
    a, b, c, d, w = (_ptr(0x100000 * (i + 1)) for i in range(5))

    def pyramid(N=2, C=3, T=4, H=64, W=64, x=a, l0=b, l1=c, l2=d):
        return lib.mcg_swd_pyramid(N, C, T, H, W, x, l0, l1, l2, None)
    for null in ('x', 'l0', 'l1', 'l2'):
        assert pyramid(**{null: None}) == -1, null
    for bad in (dict(N=0), dict(T=0), dict(C=0), dict(C=4), dict(H=-64)):
        assert pyramid(**bad) == -1, bad
    for other in (dict(H=32, W=32), dict(H=128, W=128), dict(H=64, W=32), dict(H=63, W=64)):
        assert pyramid(**other) == -2, other                          # frame sizes other than 64x64: MCG_ERR_UNSUPPORTED

    def gather(N=2, C=3, T=4, hw=32, lv=a, first=0, P_=16, pt=2, out=b):
        return lib.mcg_swd_gather(N, C, T, hw, lv, first, P_, pt, 1, 2, out, None)
    assert gather(lv=None) == -1 and gather(out=None) == -1
    for bad in (dict(pt=5), dict(pt=0), dict(P_=0), dict(N=0), dict(C=4), dict(first=-1), dict(T=0)):
        assert gather(**bad) == -1, bad                               # pt > T among them
    assert gather(hw=48) == -2 and gather(hw=8) == -2

    assert lib.mcg_swd_channel_sums(48, 147, 3, None, b, w, None) == -1 and lib.mcg_swd_channel_sums(48, 147, 3, a, None, w, None) == -1
    assert lib.mcg_swd_channel_sums(48, 147, 3, a, b, None, None) == -1
    assert lib.mcg_swd_channel_sums(0, 147, 3, a, b, w, None) == -1 and lib.mcg_swd_channel_sums(48, 148, 3, a, b, w, None) == -1
    assert lib.mcg_swd_normalize(48, 147, 3, None, b, None) == -1 and lib.mcg_swd_normalize(48, 147, 3, a, None, None) == -1
    assert lib.mcg_swd_normalize(0, 147, 3, a, b, None) == -1 and lib.mcg_swd_normalize(48, 147, 4, a, b, None) == -1
    assert lib.mcg_swd_unit_columns(49, 8, None, None) == -1 and lib.mcg_swd_unit_columns(0, 8, a, None) == -1
    assert lib.mcg_swd_unit_columns(49, 0, a, None) == -1

    def project(n=48, D=49, K_=8, x=a, dr=b, out=c, stride=48):
        return lib.mcg_swd_project(n, D, K_, x, dr, out, stride, None)
    for null in ('x', 'dr', 'out'):
        assert project(**{null: None}) == -1, null
    for bad in (dict(n=0), dict(D=0), dict(K_=0), dict(stride=47), dict(n=-3)):
        assert project(**bad) == -1, bad

    L = hl.sort_local_span()
    assert lib.mcg_sort_rows(2, 48, None, 48, w, None) == -1
    assert lib.mcg_sort_rows(0, 48, a, 48, w, None) == -1 and lib.mcg_sort_rows(2, 0, a, 48, w, None) == -1      # n < 1
    assert lib.mcg_sort_rows(2, -5, a, 48, w, None) == -1 and lib.mcg_sort_rows(2, 48, a, 47, w, None) == -1
    assert lib.mcg_sort_rows(2, L + 1, a, L + 1, None, None) == -1                                                # needs the workspace
    assert lib.mcg_sort_rows(2, L + 1, a, L + 1, _ptr(0x100004), None) == -1                                      # ... 16-byte aligned
    assert lib.mcg_sort_rows(70000, 48, a, 48, w, None) == -2

    def distance(K_=8, na=48, nb=48, x=a, sa=48, y=b, sb=48, out=c, ws=w):
        return lib.mcg_swd_distance(K_, na, nb, x, sa, y, sb, out, ws, None)
    for null in ('x', 'y', 'out', 'ws'):
        assert distance(**{null: None}) == -1, null
    assert distance(nb=47, sb=47) == -1 and distance(na=64, sa=64) == -1                                         # unequal set sizes
    for bad in (dict(K_=0), dict(na=0, nb=0), dict(sa=40), dict(sb=40)):
        assert distance(**bad) == -1, bad


def test_product_path_refuses_host_tensors(hl):
    import torch
    with pytest.raises(hl.McgError):
        hl.swd_pyramid(torch.zeros(1, 2, 64, 64, 3, dtype=torch.uint8))
    with pytest.raises(hl.McgError):
        hl.swd_pyramid(torch.zeros(1, 2, 64, 64, 3))
    with pytest.raises(hl.McgError):
        hl.sort_rows(torch.zeros(2, 8))


def test_cli_parses():
    import evaluate_swd as ev
    a = ev.parse_args(['g.npz'])
    assert (a.num, a.patches, a.patch_frames, a.repeats, a.dirs, a.seed, a.test_mode, a.baseline) == (1024, 128, 1, 4, 128, 0, 1, False)
    assert (a.dataset_type, a.dataset, a.synthetic_size, a.mfma, a.labels) == ('mug', 'data/dataset/train', 256, 'f32', None)
    a = ev.parse_args(['g.npz', '--dataset_type', 'synthetic', '--synthetic_size', '32', '--num', '8', '--patches', '16', '--patch_frames', '2',
                       '--seed', '3', '--mfma', 'f32x3', '--test_mode', '0', '--baseline', '--n_filters', '8'])
    assert (a.dataset_type, a.synthetic_size, a.num, a.patches, a.patch_frames, a.seed, a.mfma, a.test_mode, a.baseline) == \
        ('synthetic', 32, 8, 16, 2, 3, 'f32x3', 0, True)
    assert ev.parse_args(['g.npz', '--dim_zl', '6', '--labels', '2', '--num', '4']).labels == [2]
    for bad in (['g.npz', '--num', '0'], ['g.npz', '--patch_frames', '17'], ['g.npz', '--labels', '1'], ['g.npz', '--baseline', '--num', '7'],
                ['g.npz', '--dim_zl', '6', '--labels', '7'], ['g.npz', '--channel', '2'], ['--num', '4'], ['g.npz', '--mfma', 'fp8']):
        with pytest.raises(SystemExit):
            ev.parse_args(bad)
    x = np.linspace(-1, 1, 3 * 2 * 4 * 4, dtype=np.float32).reshape(3, 2, 4, 4)
    u8 = ev.to_bytes(x)
    assert u8.shape == (2, 4, 4, 3) and u8.dtype == np.uint8 and u8.min() == 0 and u8.max() == 255
    ds = ev.make_dataset(ev.parse_args(['g.npz', '--dataset_type', 'synthetic', '--synthetic_size', '5', '--channel', '1', '--video_len', '4']))
    chunks = list(ev.real_chunks(ds, 5, 2))
    assert [c.shape for c in chunks] == [(2, 4, 64, 64, 1), (2, 4, 64, 64, 1), (1, 4, 64, 64, 1)] and chunks[0].dtype == np.uint8
    with pytest.raises(ValueError):
        list(ev.real_chunks(ds, 6, 2))


# ---- the fixed test sets of the GPU tests --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,pt", [(1, 1), (3, 1), (1, 2), (3, 2)])
def test_fixed_sets_have_no_constant_channel_and_a_distance_far_above_the_gpu_tolerance(C, pt):
    """the whole-chain GPU test allows errA + errB, err_X = max (D + 8) 2^-24 (|desc_X| @ |dirs|): the reference distance of the two
    sets must be at least 100 times that at every level, otherwise that comparison shows nothing"""
    real, fake = sr.fixed_sets(C)
    assert real.shape == fake.shape == (3, 4, 64, 64, C) and real.dtype == np.uint8
    la, lb = sr.pyramid(real), sr.pyramid(fake)
    for lv in (la, lb):
        for s in sr.LEVELS:
            assert lv[s].reshape(-1, C).std(0).min() > 1.0, s                       # no zero-variance channel at any level
    da, db = sr.descriptors(la, C, P, pt, SEED), sr.descriptors(lb, C, P, pt, SEED)
    res = sr.distance(da, db, R, K, SEED)
    for li, s in enumerate(sr.LEVELS):
        D = pt * 49 * C
        assert da[s].shape == (3 * P, D)
        tol = 0.0
        for r in range(R):
            dirs = sr.unit_columns(sr.raw_directions(li, r, D, K, SEED))
            tol = max(tol, sr.projection_bound(da[s], dirs, 8).max() + sr.projection_bound(db[s], dirs, 8).max())
        assert res[str(s)] * 1e-3 >= 100 * tol, (s, res[str(s)] * 1e-3, tol)
    assert res['avg'] == pytest.approx(np.mean([res[str(s)] for s in sr.LEVELS]))


def test_edge_chain_shape_has_a_distance_far_above_the_gpu_tolerance():
    """the same margin for the chain of tests/test_gpu_swd_edges.py: P = 10923 patches of each of 3 clips (n = 32769 = 4 L + 1 at
    L = 8192), D = 147, K = 136 directions (two tiles), one repeat, on the reference's own levels"""
    C, P_, K_ = 3, 10923, 136
    real, fake = sr.fixed_sets(C)
    da, db = sr.descriptors(sr.pyramid(real), C, P_, 1, SEED), sr.descriptors(sr.pyramid(fake), C, P_, 1, SEED)
    res = sr.distance(da, db, 1, K_, SEED)
    for li, s in enumerate(sr.LEVELS):
        assert da[s].shape == (32769, 147)
        dirs = sr.unit_columns(sr.raw_directions(li, 0, 147, K_, SEED))
        tol = sr.projection_bound(da[s], dirs, 8).max() + sr.projection_bound(db[s], dirs, 8).max()
        print("edge chain level %d: ref %.6f, tol %.3e, ref / tol %.0f" % (s, res[str(s)] * 1e-3, tol, res[str(s)] * 1e-3 / tol))
        assert res[str(s)] * 1e-3 >= 100 * tol, (s, res[str(s)] * 1e-3, tol)


# ---- the sort's launch schedule, scaled down -----------------------------------------------------------------------------------
@pytest.mark.parametrize("length", ['L', '2L+3', '4L+1', '8L+5', '16L+1', '64L'])
def test_emulated_sort_schedule_sorts_and_has_the_launch_patterns_the_gpu_tests_name(length):
    """the host loop of mcg_sort_rows, restated in swd_ref.sort_rows_emulation and run with a local span of 16: it sorts at the
    lengths the GPU tests use (so a failure there is the kernels', not the schedule's), and a 'global2' launch is followed by a
    'global' one in a stage first at n2 = 8 L, by a second 'global2' first at n2 = 16 L"""
    L = 16
    m, r = length.split('L')
    n = (int(m) if m else 1) * L + (int(r) if r else 0)
    rng = np.random.RandomState(n)
    for x in (rng.randn(n).astype(np.float32), rng.randint(-3, 4, n).astype(np.float32), np.sort(rng.randn(n).astype(np.float32))[::-1]):
        got, launches = sr.sort_rows_emulation(x, L)
        assert np.array_equal(got, np.sort(x))
    stages = {}
    for la in launches[1:]:
        stages.setdefault(la[1], []).append(la[0])
    n2 = 1 << (n - 1).bit_length()
    assert sorted(stages) == [L << s for s in range(1, (n2 // L).bit_length())]
    kinds = set(tuple(v) for v in stages.values())
    assert all(v[-1] == 'local' for v in kinds)
    assert (('global2', 'global', 'local') in kinds) == (n2 >= 8 * L)
    assert (('global2', 'global2', 'local') in kinds) == (n2 >= 16 * L)
    # the descending half of a 'global2' launch: some element of it has (i & k) != 0 exactly when k < n2
    assert any(la[0] == 'global2' and la[1] < n2 for la in launches) == (n2 >= 8 * L)
