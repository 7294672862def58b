"""The geometric augmentation without a GPU: hl.parse_warp and train.py's --warp, the stream ids and the gate's argument check,
properties of the NumPy statement (tests/warp_ref.py: adjoint, exact permutations, draw statistics), and the host-side refusals
of the four entry points (the pattern of tests/test_cabi_cpu.py: a never-dereferenced pointer, outputs untouched)."""
import ctypes

import numpy as np
import pytest

import warp_ref as wr

NAMES = 'flip,rot90,scale,rotate'
F32 = np.float32


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


# ---- the options --------------------------------------------------------------------------------------------------------------
def test_parse_warp(hl):
    assert (hl.WARP_FLIP, hl.WARP_ROT90, hl.WARP_SCALE, hl.WARP_ROTATE) == (1, 2, 4, 8) == wr.COMPONENTS
    assert hl.WARP_NAMES == {'flip': 1, 'rot90': 2, 'scale': 4, 'rotate': 8}
    for off in (None, '', 0, ' ', ','):
        assert hl.parse_warp(off) == 0
    assert hl.parse_warp(NAMES) == 15 and hl.parse_warp('rotate, flip') == 9 and hl.parse_warp('rot90') == 2
    assert hl.parse_warp('scale,scale,') == 4 and hl.parse_warp(15) == 15 and hl.parse_warp(6) == 6
    for bad in ('color', 'flip,cutout', 'Flip', 'rot', 16, -1, True, False, 1.0, ['flip'], b'flip'):
        with pytest.raises(ValueError):
            hl.parse_warp(bad)
    # the two option spaces stay apart: the augmentation's parser still knows its three names and its masks 0..7 only
    for bad in ('color,flip', 'rotate', 8):
        with pytest.raises(ValueError):
            hl.parse_augment(bad)


def test_command_line_flag():
    import train
    a = train.parse_args([])
    assert a.warp == '' and a.augment == ''
    a = train.parse_args(['--warp', NAMES])
    assert a.warp == NAMES and a.augment == '' and a.augment_p is None
    assert train.parse_args(['--warp', 'scale,flip']).warp == 'scale,flip'
    # --augment_p and --ada_target are accepted with --warp alone
    a = train.parse_args(['--warp', 'flip,scale', '--augment_p', '0.5'])
    assert a.augment_p == 0.5 and train.ada_option(a) is None
    a = train.parse_args(['--warp', NAMES, '--ada_target', '0.6'])
    assert train.ada_option(a) == {'target': 0.6, 'interval': 4, 'kimg': 500.0}
    a = train.parse_args(['--warp', 'rotate', '--augment', 'color,cutout', '--augment_p', '0.25', '--ada_target', '0.5'])
    assert (a.warp, a.augment, a.augment_p) == ('rotate', 'color,cutout', 0.25)
    for argv in (['--warp', 'color'], ['--warp', 'flip,translation'], ['--augment', 'color,flip'], ['--augment', 'rot90'],
                 ['--augment_p', '0.5'], ['--ada_target', '0.6'], ['--warp', '', '--augment_p', '0.5'], ['--warp', NAMES, '--augment_p', '1.5'],
                 ['--warp', NAMES, '--ada_target', '1']):
        with pytest.raises(SystemExit):
            train.parse_args(argv)


class _Exchange:
    def __init__(self, active):
        self.active = active


def test_stream_ids_and_the_gate_check():
    import mocogan_chainer_amd.step as step
    ts = step.TrainStep
    ids = [ts.AUG_STREAM_REAL, ts.AUG_STREAM_FAKE, ts.AUG_GATE_REAL, ts.AUG_GATE_FAKE, ts.WARP_STREAM_REAL, ts.WARP_STREAM_FAKE,
           ts.WARP_GATE_REAL, ts.WARP_GATE_FAKE]
    assert ids == list(range(40, 48)) and max(ids) < ts.STREAMS_PER_RANK
    mats = wr.perf_mode_mats(11, 3, 2, 5)
    base = ts.stream_base(3, 2)
    assert np.array_equal(mats['real'], wr.draw(5, 64, 64, 15, 11, base + 44)) and np.array_equal(mats['fake'], wr.draw(5, 64, 64, 15, 11, base + 45))
    gated = wr.perf_mode_mats(11, 3, 2, 5, p=0.5)
    assert np.array_equal(gated['real'], wr.draw_gated(5, 64, 64, 15, 11, base + 44, base + 46, 0.5)[0])
    assert np.array_equal(gated['fake'], wr.draw_gated(5, 64, 64, 15, 11, base + 45, base + 47, 0.5)[0])
    # the gate accepts a non-empty augment OR warp; with both empty it raises the error it always raised
    assert step.check_augment_gate(None, 0.25, None, warp='flip') == (0.25, None)
    assert step.check_augment_gate('', None, True, warp=NAMES) == (0.0, {'target': 0.6, 'interval': 4, 'kimg': 500.0})
    assert step.check_augment_gate('cutout', 1, None, _Exchange(False), 'rotate') == (1.0, None)
    assert step.check_augment_gate(None, None, None, warp=NAMES) == (None, None)
    assert step.check_augment_gate(None, None, None, _Exchange(True), NAMES) == (None, None)          # ungated: fine with data parallelism
    for kw in (dict(warp=None), dict(warp=''), dict(warp=0), dict()):
        with pytest.raises(ValueError, match='^augment_p / ada set how often the augmentation is applied: they need a non-empty augment policy$'):
            step.check_augment_gate(None, 0.5, None, **kw)
    with pytest.raises(ValueError, match='gradient exchange'):
        step.check_augment_gate(None, 0.5, None, _Exchange(True), 'flip')
    with pytest.raises(ValueError):
        step.check_augment_gate(None, 0.5, None, warp='cutout')
    for kw in (dict(warp='color'), dict(warp=16), dict(warp=NAMES, augment_p=2.0), dict(warp=NAMES, ada=True, exchange=_Exchange(True))):
        with pytest.raises(ValueError):
            step.TrainStep('normal', None, None, None, **kw)
    from model.updater import Updater
    base_kw = dict(model='normal', models=(None, None, None), video_length=16, img_size=64, channel=3, dim_zl=6, tensorboard_writer=None,
                   iterator=None, optimizer={})
    for kw in (dict(warp='cutout', augment_p=0.5), dict(augment_p=0.5), dict(warp=NAMES, augment_p=-1.0), dict(warp=NAMES, ada={'target': 1.0})):
        with pytest.raises(ValueError):
            Updater(**dict(base_kw, **kw))


# ---- the NumPy statement ------------------------------------------------------------------------------------------------------
def test_adjoint_is_the_transpose_of_forward():
    """<A u, g> == <u, A^T g> on 2x1x1x5x6 for every hand-placed matrix and drawn ones: A applied column by column IS the matrix"""
    H, W = 5, 6
    rng = np.random.RandomState(3)
    mats = np.concatenate([wr.hand_placed(wr.N_HAND_PLACED, H, W), wr.draw(6, 6, 6, 15, 5, 44), wr.draw(4, H, W, 13, 6, 45)])
    if len(mats) % 2:
        mats = mats[:-1]
    for pair in mats.reshape(-1, 2, 8):
        u, g = rng.randn(2, 1, 1, H, W), rng.randn(2, 1, 1, H, W)
        lhs, rhs = float((wr.forward(u, pair) * g).sum()), float((u * wr.adjoint(g, pair)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, float(np.abs(wr.forward(u, pair) * g).sum())), (pair, lhs, rhs)
        # ... and element by element: column (v, u) of the forward map is row (v, u) of the adjoint
        basis = [np.tile(e.reshape(1, 1, 1, H, W), (2, 1, 1, 1, 1)) for e in np.eye(H * W)]
        A = np.stack([wr.forward(e, pair).reshape(2, H * W) for e in basis], axis=2)           # A[clip][out][in]
        At = np.stack([wr.adjoint(e, pair).reshape(2, H * W) for e in basis], axis=2)          # At[clip][in][out]
        assert np.allclose(A, At.transpose(0, 2, 1), rtol=0, atol=1e-15)


def test_flip_and_quarter_turns_are_exact_permutations():
    rng = np.random.RandomState(4)
    x = rng.randn(5, 2, 3, 8, 8)
    sets = wr.hand_placed(5, 8, 8)                                     # identity, flip, Q_1, Q_2, Q_3
    out = wr.forward(x, sets)
    assert np.array_equal(out[0], x[0])
    assert np.array_equal(out[1], np.flip(x[1], axis=-1))
    turns = [[k for k in range(4) if np.array_equal(out[2 + j], np.rot90(x[2 + j], k, axes=(-2, -1)))] for j in range(3)]
    assert turns in ([[1], [2], [3]], [[3], [2], [1]]), turns          # Q_k is k quarter turns, all in one sense
    g = rng.randn(5, 2, 3, 8, 8)
    back = wr.adjoint(g, sets)
    assert np.array_equal(back[0], g[0]) and np.array_equal(back[1], np.flip(g[1], axis=-1))
    for j in range(3):
        assert np.array_equal(back[2 + j], np.rot90(g[2 + j], -turns[j][0], axes=(-2, -1)))
    # a flip on a non-square frame is exact as well; the draw composes the same matrices
    y = rng.randn(1, 1, 2, 6, 10)
    assert np.array_equal(wr.forward(y, wr.hand_placed(1, 6, 10, first=1)), np.flip(y, axis=-1))
    for k in range(4):
        m = wr.compose(1.0, k, 1.0, 1.0, 0.0)
        assert np.array_equal(m[0, :6], ([1, 0, 0, 0, 1, 0], [0, -1, 0, 1, 0, 0], [-1, 0, 0, 0, -1, 0], [0, 1, 0, -1, 0, 0])[k])
        assert not (np.signbit(m) & (m == 0)).any()                        # no -0 is stored
    assert np.array_equal(wr.compose(-1.0, 1, 1.0, 1.0, 0.0)[0, :6], [0, -1, 0, -1, 0, 0])


def test_special_matrices_of_the_statement():
    rng = np.random.RandomState(5)
    H, W = 6, 10
    x = rng.randn(4, 1, 2, H, W)
    mats = wr.hand_placed(4, H, W, first=10)                             # half-pixel offset, all outside, all-zero, 1e6 scale
    out, mag = wr.forward(x, mats, with_terms=True)
    # sx = x + 0.5, sy = y - 0.5: the mean of the four neighbours, zero outside the frame
    xp = np.pad(x[0], ((0, 0), (0, 0), (1, 1), (1, 1)))
    assert np.allclose(out[0], 0.25 * (xp[..., 0:H, 1:W + 1] + xp[..., 0:H, 2:W + 2] + xp[..., 1:H + 1, 1:W + 1] + xp[..., 1:H + 1, 2:W + 2]), atol=1e-15)
    assert not out[1].any() and not wr.adjoint(x, mats)[1].any()
    # the all-zero matrix: every output is the mean of the four centre pixels; the gradient lands on those four
    centre = x[2][..., H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].mean(axis=(-2, -1))
    assert np.allclose(out[2], centre[..., None, None], atol=1e-15)
    back = wr.adjoint(x, mats)[2]
    assert np.count_nonzero(back[0, 0]) == 4 and np.allclose(back.sum(axis=(-2, -1)), x[2].sum(axis=(-2, -1)))
    assert not out[3].any()                                              # even extents: no pixel sits on the centre
    assert (mag >= np.abs(out) - 1e-15).all()


def test_draw_statistics():
    """n = 4096: a flag or a turn count is a binomial / multinomial mean, sigma <= sqrt(0.25 / n) = 0.0078, held to 5 sigma = 0.04"""
    n = 4096
    f, k, s, c, sn = wr.components(n, 15, 2024, 44)
    assert abs((f < 0).mean() - 0.5) <= 0.04
    for j in range(4):
        assert abs((k == j).mean() - 0.25) <= 0.04, j
    assert s.dtype == F32 and (s > F32(5) / F32(7)).all() and (s < F32(7) / F32(5)).all()
    assert abs(np.log(s.astype(np.float64)).mean()) <= 5 * np.log(1.4) / np.sqrt(3 * n)          # symmetric in the logarithm
    one = c.astype(np.float64) ** 2 + sn.astype(np.float64) ** 2
    assert np.abs(one - 1.0).max() <= 4 * 2.0 ** -23, np.abs(one - 1.0).max()
    assert (c >= 0).all() and sn.min() < -0.99 and sn.max() > 0.99
    # the matrices: determinant f / s^2 within rounding, flags 0, offsets 0
    mat = wr.draw(n, 64, 64, 15, 2024, 44)
    det = mat[:, 0].astype(np.float64) * mat[:, 4] - mat[:, 1].astype(np.float64) * mat[:, 3]
    assert np.allclose(det, f / s.astype(np.float64) ** 2, rtol=1e-6)
    assert not mat[:, 2].any() and not mat[:, 5:].any()
    # a component that is off takes its identity value and its word is still consumed
    for policy in range(16):
        fp, kp, sp, cp, snp = wr.components(n, policy, 2024, 44)
        for flag, got, full, ident in ((1, fp, f, 1.0), (2, kp, k, 0), (4, sp, s, 1.0), (8, cp, c, 1.0), (8, snp, sn, 0.0)):
            assert np.array_equal(got, full) if policy & flag else (got == ident).all(), (policy, flag)
    assert np.array_equal(wr.draw(7, 64, 64, 0, 1, 44), wr.identity_mats(7))


def test_gated_draw_statement():
    n = 2048
    plain = wr.draw(n, 64, 64, 15, 9, 44)
    mat, mask = wr.draw_gated(n, 64, 64, 15, 9, 44, 46, 0.0)
    assert np.array_equal(mat, wr.identity_mats(n)) and not mask.any()
    for p in (1.0, 1.5):
        mat, mask = wr.draw_gated(n, 64, 64, 15, 9, 44, 46, p)
        assert np.array_equal(mat[:, :6].view(np.uint32), plain[:, :6].view(np.uint32)) and (mat[:, 6] == 15).all() and (mask == 15).all()
    mat, mask = wr.draw_gated(n, 64, 64, 13, 9, 44, 46, 0.5)
    assert not (mask & 2).any() and np.array_equal(mat[:, 6], mask.astype(F32))
    for j, flag in enumerate((1, 4, 8)):
        assert abs(((mask & flag) != 0).mean() - 0.5) <= 5 * np.sqrt(0.25 / n), flag
    kept = mask == 13
    assert kept.any() and np.array_equal(mat[kept, :6], wr.draw(n, 64, 64, 13, 9, 44)[kept, :6])
    assert np.array_equal(mat[mask == 0, :6], wr.identity_mats(int((mask == 0).sum()))[:, :6])


# ---- host-side refusals -------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_on_the_host(hl):
    """`one` / `two` are non-null pointers that are never dereferenced; the outputs are small host buffers that must come back
    untouched; no call below passes an acceptable argument set"""
    lib = hl.load()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(4096)
    BAD, UNSUPPORTED = -1, -2
    buf = (ctypes.c_float * 16)(*([3.0] * 16))
    out = ctypes.cast(buf, ctypes.c_void_p)

    def refused(rc, want, *what):
        assert rc == want, (what, rc)
        assert list(buf) == [3.0] * 16, what

    for fn in (lib.mcg_warp_fwd, lib.mcg_warp_bwd):
        def call(N=2, C=3, Cp=4, T=2, H=8, W=8, x=one, mat=two, o=out):
            return fn(N, C, Cp, T, H, W, x, mat, o, None)
        for bad in (dict(x=None), dict(mat=None), dict(o=None), dict(N=0), dict(N=-1), dict(T=0), dict(H=0), dict(W=-8), dict(C=0), dict(C=5),
                    dict(C=9, Cp=8), dict(x=out)):
            refused(call(**bad), BAD, bad)
        for bad in (dict(Cp=8), dict(C=1, Cp=1), dict(N=65536), dict(T=1 << 12, H=1 << 9, W=1 << 8)):
            refused(call(**bad), UNSUPPORTED, bad)

    def draw(N=4, H=64, W=64, policy=15, m=out):
        return lib.mcg_warp_draw(N, H, W, policy, 1, 44, m, None)

    def gated(N=4, H=64, W=64, policy=15, sid=44, gsid=46, a=one, m=out):
        return lib.mcg_warp_draw_gated(N, H, W, policy, 1, sid, gsid, a, m, None)

    for bad in (dict(N=0), dict(N=-3), dict(H=0), dict(W=0), dict(policy=-1), dict(policy=16), dict(m=None)):
        refused(draw(**bad), BAD, 'mcg_warp_draw', bad)
        refused(gated(**bad), BAD, 'mcg_warp_draw_gated', bad)
    for bad in (dict(a=None), dict(gsid=44), dict(sid=(5 << 32) + 1, gsid=(5 << 32) + 1)):
        refused(gated(**bad), BAD, 'mcg_warp_draw_gated', bad)
    for policy in (2, 3, 15):                                            # a quarter turn needs a square frame
        refused(draw(H=8, W=24, policy=policy), UNSUPPORTED, policy)
        refused(gated(H=8, W=24, policy=policy), UNSUPPORTED, policy)


def test_wrappers_check_their_tensors(hl):
    import torch
    with pytest.raises(hl.McgError):
        hl.warp_draw(3, 64, 64, 15, 1, 44, torch.zeros((2, 8)))            # fewer matrices than clips
    with pytest.raises(hl.McgError):
        hl.warp_draw_gated(2, 64, 64, 15, 1, 44, 46, torch.zeros(8, dtype=torch.float32), torch.zeros((2, 8)))     # not doubles
    x = torch.zeros((2, 1, 4, 4, 4))
    with pytest.raises(hl.McgError):
        hl.warp_fwd(x, 3, torch.zeros((1, 8)), torch.zeros_like(x))
    with pytest.raises(hl.McgError):
        hl.warp_bwd(x, 3, torch.zeros((2, 8)), torch.zeros((2, 1, 4, 4, 3)))
    with pytest.raises(hl.McgError):
        hl.warp_fwd(x, 3, torch.zeros((2, 8)), torch.zeros_like(x))        # host tensors
