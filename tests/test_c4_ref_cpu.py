"""tests/c4_ref.py held to account without a GPU: the dispatch mirror against the library's own return codes, the launch plans against
the figures the case table is built on, the float64 references against oracle.functions and hand-computed cases, and the acceptance
check of tests/test_gpu_c4_guard.py against simulated defects -- each must leave at least one element of some output outside the bound,
on the very inputs the GPU test uses.

The library validates geometry and tile code before it launches: a refused argument set answers MCG_ERR_UNSUPPORTED whatever its
pointers are (they are a host buffer nothing reads), an accepted one is asked with null pointers and answers MCG_ERR_BAD_ARG for them --
nothing is launched either way."""
import ctypes

import numpy as np
import pytest

from oracle import functions as F
import c4_ref as R

BAD_ARG, UNSUPPORTED = -1, -2
DGRAD_FORMS = [dict(bias=False, act=False, accumulate=False), dict(bias=False, act=False, accumulate=True),
               dict(bias=True, act=True, accumulate=False)]


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def _geoms():
    """every geometry the GPU test launches: the rows, and the views of the 2-D rows"""
    out = [R.Geo(row) for row in R.C4_ROWS]
    for row in R.VIEW_ROWS:
        for clips in R.VIEW_CLIPS:
            out += [R.Geo(row, 'frame', clips), R.Geo(row, 'perm', clips)]
    return out


def _lib_geom(hl, g, tile, prec):
    lg = hl.make_geom(g.N, g.Ti, g.Hi, g.Wi, R.CI, R.CO, g.kt, x_stride0=g.x_stride0, x_perm_n=g.x_perm_n, x_stride1=g.x_stride1,
                      precision=prec, ci_valid=R.CV)
    lg.tile = tile
    return lg


def _launches():
    for g in _geoms():
        for tile in R.TILES:
            for prec in R.PRECS:
                yield g, 'fprop', tile, prec, {}
                yield g, 'wgrad', tile, prec, {}
                for form in DGRAD_FORMS:
                    yield g, 'dgrad', tile, prec, form


def test_the_mirror_accepts_and_refuses_what_the_library_does(hl):
    lib = hl.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    seen = {BAD_ARG: 0, UNSUPPORTED: 0}
    for g, pass_, tile, prec, form in _launches():
        kernel = R.dispatch(g, pass_, tile, prec, **form)[0]
        q = p if kernel == R.UNSUPPORTED else None           # only a launch the mirror AND the library refuse sees a non-null pointer
        lg = ctypes.byref(_lib_geom(hl, g, tile, prec))
        if pass_ == 'fprop':
            st = lib.mcg_conv_fprop(lg, q, q, None, q, None)
        elif pass_ == 'wgrad':
            st = lib.mcg_conv_wgrad(lg, q, q, q, None)
        else:
            st = lib.mcg_conv_dgrad(lg, q, q, q if form['bias'] else None, q, hl.ACT_TANH if form['act'] else hl.ACT_NONE,
                                    int(form['accumulate']), None)
        want = UNSUPPORTED if kernel == R.UNSUPPORTED else BAD_ARG
        assert st == want, (R.row_id((g.N, g.Ti, (g.Hi, g.Wi), g.kt)), g.view, pass_, tile, prec, form, kernel, st)
        seen[st] += 1
        if pass_ == 'dgrad' and not any(form.values()):
            assert hl.dgrad_c4_mfma_covers(_lib_geom(hl, g, tile, prec)) == (kernel == 'dgrad_c4_mfma_kernel'), (g.view, tile, prec)
    assert seen[UNSUPPORTED] >= 50 and seen[BAD_ARG] >= 500, seen
    assert bytes(buf) == bytes(64)


def test_geometry_of_the_views():
    g = R.Geo(R.VIEW_ROWS[0], 'frame', 2)
    assert (g.N, g.dense, g.whole, g.x_perm_n, g.x_stride0) == (2, False, False, 0, 3 * 32 * 32 * 4)
    g = R.Geo(R.VIEW_ROWS[1], 'perm', 2)
    assert (g.N, g.dense, g.whole, g.x_perm_n, g.x_stride0, g.x_stride1) == (6, False, True, 2, 3 * 16 * 64 * 4, 16 * 64 * 4)
    # launch item t * clips + b is frame t of clip b: the six frames tile the clip buffer one to one
    assert sorted(g.item_offset(n) for n in range(6)) == [i * 16 * 64 * 4 for i in range(6)]
    assert g.item_offset(3) == 1 * g.x_stride0 + 1 * g.x_stride1
    frames = np.arange(6, dtype=np.float64).reshape(6, 1, 1, 1, 1)
    assert R.to_clip_order(frames, 2)[:, :, 0, 0, 0].tolist() == [[0, 2, 4], [1, 3, 5]]


def test_the_table_reaches_every_instantiation_and_plan_class():
    kernels, classes = set(), {}
    for g, pass_, tile, prec, form in _launches():
        kernel, inst, plan = R.dispatch(g, pass_, tile, prec, **form)
        if kernel in (R.UNSUPPORTED, 'gemm'):
            continue
        kernels.add((kernel, inst) + ((prec,) if kernel == 'dgrad_c4_mfma_kernel' else ()))
        classes.setdefault(kernel.replace('_bf16', ''), set()).update(plan['cls'])
    insts = [(kt, wo) for kt in (1, 4) for wo in (16, 32)]
    want = {(k, i) for k in ('fprop_c4_kernel', 'fprop_c4_bf16_kernel', 'wgrad_c4_kernel', 'wgrad_c4_bf16_kernel') for i in insts}
    want |= {('dgrad_c4_mfma_kernel', i, p) for i in insts for p in R.PRECS}
    want |= {('dgrad_c4_kernel', (1,)), ('dgrad_c4_kernel', (4,))}
    assert kernels == want, (sorted(want - kernels), sorted(kernels - want))
    assert classes == {
        'fprop_c4_kernel': {'one block per item', 'row blocks'},
        'dgrad_c4_mfma_kernel': {'one tile per block', 'ntiles > 1024'},
        'dgrad_c4_kernel': {'full blocks', 'partly filled block'},
        'wgrad_c4_kernel': {'tsplit = 1', 'tsplit = 2', 'tsplit = 4', 'tsplit = 8', 'ragged part', 'one-step part', 'empty part', 'nsplit < N'},
    }, classes


def test_the_plans_are_the_ones_the_table_is_built_on():
    rows = {R.row_id(r): R.Geo(r) for r in R.C4_ROWS}
    lens = lambda plan: [b - a for a, b in plan['parts']]
    want = {4: (2, [2, 2]), 5: (2, [3, 2]), 9: (4, [3, 3, 3, 0]), 13: (4, [4, 4, 4, 1]), 17: (8, [3, 3, 3, 3, 3, 2, 0, 0])}
    for To, (tsplit, parts) in want.items():
        g = rows["1x%dx16x64-kt4" % (To + 3)]
        for prec, hblocks in (('f32', 1), ('bf16y', 2)):
            plan = R.plan_wgrad(g, prec)
            assert (plan['tsplit'], lens(plan), plan['hblocks'], plan['grid']) == (tsplit, parts, hblocks, hblocks * tsplit), (To, prec, plan)
            assert sum(lens(plan)) == To
    g = rows["520x1x16x64-kt1"]
    plan = R.plan_wgrad(g, 'f32')
    assert (plan['nsplit'], plan['tsplit'], plan['grid']) == (512, 1, 512)
    assert (R.plan_col2im(g)['ntiles'], R.plan_col2im(g)['grid']) == (1040, 1024)
    assert R.plan_fprop(g)['grid'] == 520
    assert [R.plan_valu(rows[k])['runs'] for k in ("3x1x2x32-kt1", "17x1x2x32-kt1", "1x1x4x128-kt1")] == [3, 17, 8]
    assert [R.plan_valu(rows[k])['grid'] for k in ("3x1x2x32-kt1", "17x1x2x32-kt1", "1x1x4x128-kt1")] == [1, 2, 1]
    for k in ("1x1x32x32-kt1", "1x1x16x64-kt1", "2x4x32x32-kt4", "2x5x16x64-kt4"):
        g = rows[k]
        assert R.plan_fprop(g)['grid'] == g.N and R.plan_col2im(g)['ntiles'] == 2 * g.N
    assert R.plan_fprop(rows["1x1x64x32-kt1"])['grid'] == 2
    g = rows["2x1x16x32-kt1"]                                  # Ho = 8, Wo = 16
    assert R.c4_layer(g, 128) and not R.c4_layer(g, 256)
    assert [R.dispatch(g, p, 6, 'f32')[0] for p in R.PASSES] == [R.UNSUPPORTED, 'dgrad_c4_mfma_kernel', R.UNSUPPORTED]
    assert [R.dispatch(g, p, 0, 'f32')[0] for p in R.PASSES] == ['gemm', 'dgrad_c4_mfma_kernel', 'gemm']
    assert R.plan_ksplit(2048, 32, 256, 4) == (16, 128) and R.plan_ksplit(100, 32, 8, 4) == (1, 128)


# ---- the references ----
def _to_oracle(a):
    """device layout [..][T][H][W][C] -> the oracle's [..][C][T][H][W], data channels only where the last axis is the padded clip's"""
    return np.moveaxis(np.asarray(a, np.float64), -1, 1)


def test_references_agree_with_the_oracle():
    rng = np.random.RandomState(3)
    for N, T, H, W, kt in ((2, 5, 8, 12, 4), (3, 1, 4, 8, 1)):
        x, w = rng.randn(N, T, H, W, 4), rng.randn(6, kt, 4, 4, 4)
        x[..., 3] = 0
        w[..., 3] = 0
        gy, b = rng.randn(N, T - kt + 1, H // 2, W // 2, 6), rng.randn(6)
        xo, wo, gyo = _to_oracle(x)[:, :3], _to_oracle(w)[:, :3], _to_oracle(gy)
        y, S = R.fprop(x, w, b)
        assert np.allclose(_to_oracle(y), F.conv3d_fwd(xo, wo, b, (1, 2, 2), (0, 1, 1)), rtol=1e-12, atol=1e-12)
        assert (S >= np.abs(y) - 1e-12).all()
        gx_o, gw_o, _ = F.conv3d_bwd(xo, wo, gyo, (1, 2, 2), (0, 1, 1))
        gx, S = R.dgrad(gy, w, T, H, W)
        assert np.allclose(_to_oracle(gx)[:, :3], gx_o, rtol=1e-12, atol=1e-12) and (gx[..., 3] == 0).all() and (S[..., 3] == 0).all()
        dw, S = R.wgrad(x, gy, kt)
        assert np.allclose(_to_oracle(dw)[:, :3], gw_o, rtol=1e-12, atol=1e-12) and (dw[..., 3] == 0).all() and (S[..., 3] == 0).all()
        # the parts of a frame split add up; what is accumulated onto is added once
        To = T - kt + 1
        dw0 = rng.randn(*dw.shape)
        parts = [(0, To // 2), (To // 2, To), (To, To)]
        assert np.allclose(R.wgrad(x, gy, kt, dw0, frames=parts)[0], dw + dw0, rtol=1e-12, atol=1e-12)
        x0, b4 = rng.randn(*x.shape), rng.randn(4)
        assert np.allclose(R.dgrad(gy, w, T, H, W, b4, x0)[0], gx + b4 + x0, rtol=1e-12, atol=1e-12)


def test_references_on_hand_computed_cases():
    N, T, H, W, kt = 1, 5, 4, 8, 4
    x, w = np.zeros((N, T, H, W, 4)), np.zeros((2, kt, 4, 4, 4))
    x[..., 0], w[0, ..., 0] = 1, 1
    y, S = R.fprop(x, w, np.array([0.5, -2.0]))
    # 4 x 4 taps per frame, one row / column of them in the padding at each border: corner 3 x 3, edge 3 x 4, inside 4 x 4
    assert y.shape == (1, 2, 2, 4, 2) and (y[..., 1] == -2.0).all() and (S[..., 1] == 2.0).all()
    assert y[0, 0, :, :, 0].tolist() == [[kt * 9 + .5, kt * 12 + .5, kt * 12 + .5, kt * 9 + .5]] * 2
    gy = np.zeros((1, 2, 2, 4, 2))
    gy[0, 1, 1, 2, 0] = 3.0                                   # one output pixel: its 4 x 4 x kt window, rows 1 .. 4 (4 is outside), columns 3 .. 6
    gx, S = R.dgrad(gy, w, T, H, W)
    want = np.zeros((T, H, W))
    want[1:5, 1:4, 3:7] = 3.0
    assert (gx[0, ..., 0] == want).all() and (gx[..., 1:] == 0).all() and (S == np.abs(gx)).all()
    dw, S = R.wgrad(x, np.ones((1, 2, 2, 4, 2)), kt)
    cnt = lambda k, n: n - (k == 0) - (k == 3)                # output positions whose tap k is inside the image
    for kh in range(4):
        for kw in range(4):
            assert (dw[:, :, kh, kw, 0] == 2 * cnt(kh, 2) * cnt(kw, 4)).all() and (dw[:, :, kh, kw, 1:] == 0).all()
    assert R.bound(10, np.array([2.0])) == 18 * 2.0 ** -24 * 2 and R.bound(10, np.array([2.0]), True) == (18 * 2.0 ** -24 + 2.0 ** -8) * 2
    assert R.violations(np.array([1.0, np.nan, 1.0]), np.array([1.0, 1.0, 1.1]), 4, np.array([1.0, 1.0, 1.0])).tolist() == [False, True, True]
    assert R.violations(np.array([1e-30]), np.array([0.0]), 4, np.array([0.0])).tolist() == [True]     # a bound of zero: exact or wrong
    v = R.bf16_round(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -0.3], np.float32))              # ties to even; 8 bits kept
    assert v.tolist()[:2] == [1.0, 1.0 + 2.0 ** -6] and (v.view(np.uint32) & 0xffff == 0).all() and abs(v[2] + 0.3) < 0.3 * 2.0 ** -8


# ---- the acceptance check notices the defects the table is there to find ----
def _flags(out, ref, L, S):
    return bool(R.violations(out, ref, L, S).any())


def _defects(row):
    """(name, violates) for every defect that has something to act on in this row; the unharmed result, rounded to fp32, first"""
    g = R.Geo(row)
    d = R.inputs(row)
    x, w, gy, kt = d['x'].astype(np.float64), d['w'].astype(np.float64), d['gy'].astype(np.float64), g.kt
    Lf, Ld = R.terms('fprop', g), R.terms('dgrad', g)
    plan = R.plan_wgrad(g, 'f32')
    Lw = R.terms('wgrad', g, plan['blocks_per_element'])
    y, Sy = R.fprop(x, w, d['bias'])
    gx, Sg = R.dgrad(gy, w, g.Ti, g.Hi, g.Wi)
    dw, Sw = R.wgrad(x, gy, kt, d['dw0'])
    for name, out, ref, L, S in (('fprop', y, y, Lf, Sy), ('dgrad', gx, gx, Ld, Sg), ('wgrad', dw, dw, Lw, Sw)):
        yield 'unharmed ' + name, not _flags(out.astype(np.float32), ref, L, S)

    live = [p for p in plan['parts'] if p[1] > p[0]]
    if len(live) >= 2 or g.To >= 2:
        kept = live[:-1] if len(live) >= 2 else [(0, g.To - 1)]
        yield 'a frame part dropped', _flags(R.wgrad(x, gy, kt, d['dw0'], frames=kept)[0], dw, Lw, Sw)
    yield 'the last frame of a part counted twice', _flags(R.wgrad(x, gy, kt, d['dw0'], twice=live[0][1] - 1)[0], dw, Lw, Sw)

    # the top halo row (hi = -1) of every frame taken from the row in front of it in memory -- the last row of the frame before
    flat = x.reshape(g.N * g.Ti, g.Hi, g.Wi, 4)
    halo = np.zeros((g.N * g.Ti, g.Wi + 2, 4))
    halo[:, 1:-1] = np.roll(flat, 1, axis=0)[:, g.Hi - 1]
    halo = halo.reshape(g.N, g.Ti, g.Wi + 2, 4)
    bad = y.copy()
    for a in range(kt):
        for kw in range(4):
            bad[:, :, 0] += halo[:, a:a + g.To, kw:kw + 2 * g.Wo:2, :] @ w[:, a, 0, kw, :].T
    yield 'a halo row from the neighbouring frame', _flags(bad, y, Lf, Sy)

    xp = R._pad_hw(x)
    a = kt - 1
    shift = (R._tap_rows(xp, a, 1, 3, g.To, g.Ho, g.Wo) - R._tap_rows(xp, a, 1, 2, g.To, g.Ho, g.Wo)) @ w[:, a, 1, 2, :].T
    yield 'a tap shifted by one', _flags(y + shift.reshape(y.shape), y, Lf, Sy)

    if g.N >= 2:
        n_kept = plan['nsplit'] if plan['nsplit'] < g.N else g.N - 1
        yield 'the second walked item dropped', _flags(R.wgrad(x[:n_kept], gy[:n_kept], kt, d['dw0'])[0], dw, Lw, Sw)
    col = R.plan_col2im(g) if R.c4_layer(g, 128) else None
    if col is not None and col['ntiles'] > col['grid']:
        rows_per, hblocks = 128 // g.Wo, g.Ho // (128 // g.Wo)
        cut = gy.copy()
        for tile in range(col['grid'], col['ntiles']):
            cut[tile // hblocks, :, (tile % hblocks) * rows_per:(tile % hblocks + 1) * rows_per] = 0
        yield "a block's second tile dropped", _flags(R.dgrad(cut, w, g.Ti, g.Hi, g.Wi)[0], gx, Ld, Sg)

    pre, Sp = R.dgrad(gy, w, g.Ti, g.Hi, g.Wi, d['bias4'])
    bad = pre.copy()
    bad[..., 3] += d['bias4'][0]
    yield 'bias on the padded channel', _flags(bad, pre, Ld, Sp)

    if row in R.VIEW_ROWS:                                    # the row as frame t = 0 of a clip whose other frames hold a sentinel
        clip = np.repeat(d['x0'].astype(np.float64)[:, None, 0], R.CLIP_T, axis=1)          # [N][T][Hi][Wi][4]
        ref, S, bad = clip.copy(), np.zeros_like(clip), clip.copy()
        ref[:, 0], S[:, 0], bad[:, 1] = gx[:, 0], Sg[:, 0], gx[:, 0]
        yield 'frame t + 1 written instead of t', _flags(bad, ref, Ld, S)
        yield 'unharmed view', not _flags(ref.astype(np.float32).astype(np.float64) * (S > 0) + clip * (S == 0), ref, Ld, S)


ALL_DEFECTS = {'a frame part dropped', 'the last frame of a part counted twice', 'a halo row from the neighbouring frame', 'a tap shifted by one',
               'the second walked item dropped', "a block's second tile dropped", 'frame t + 1 written instead of t', 'bias on the padded channel'}
_applied = set()


@pytest.mark.parametrize("row", R.C4_ROWS, ids=[R.row_id(r) for r in R.C4_ROWS])
def test_simulated_defects_leave_the_bound(row):
    seen = []
    for name, ok in _defects(row):
        assert ok, (R.row_id(row), name, "not noticed" if not name.startswith('unharmed') else "the reference itself fails the check")
        seen.append(name)
    real = [n for n in seen if not n.startswith('unharmed')]
    assert len(real) >= 4, real                              # halo, tap, double count and bias act on every row
    _applied.update(real)


def test_every_defect_of_the_list_was_simulated():
    assert _applied == ALL_DEFECTS, sorted(ALL_DEFECTS - _applied)


def test_inputs_are_what_the_bound_assumes():
    for exact in (True, False):
        d = R.inputs(R.C4_ROWS[2], exact=exact)
        for k in ('x', 'w', 'bias4', 'dw0', 'x0'):
            assert d[k].dtype == np.float32 and (d[k][..., 3] == 0).all() and (d[k][..., :3] != 0).all(), k
        representable = all((d[k].view(np.uint32) & 0xffff == 0).all() for k in d)
        assert representable == exact
    a, b = R.inputs(R.C4_ROWS[2]), R.inputs(R.C4_ROWS[2])
    assert all((a[k] == b[k]).all() for k in a)
