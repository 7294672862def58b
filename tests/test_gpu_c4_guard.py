"""The six kernels written for the Ci = 4 layers (fprop_c4[_bf16]_kernel, dgrad_c4_mfma_kernel, dgrad_c4_kernel, wgrad_c4[_bf16]_kernel)
in the guard arena, element by element against float64 -- every <KT, WO> instantiation and every launch plan of tests/c4_ref.py's table.

Every operand and output of a launch is a view into ONE poisoned arena (tests/guard.py).  For every row of C4_ROWS, every pass, the
tile codes 0, 6 and 2 and every precision of the pass:
  * the library accepts exactly what c4_ref.dispatch says (tests/test_c4_ref_cpu.py pins the mirror to the return codes without a
    device); a refusal is MCG_ERR_UNSUPPORTED and leaves the poisoned output as it was; hl.dgrad_c4_mfma_covers agrees;
  * the margins are intact after every launch;
  * every output element is finite and within c4_ref.bound of the float64 statement -- the DERIVED bound (L + 8) 2^-24 S of an fp32
    inner product in any order.  fp32 launches run on full-mantissa operands; the bf16 modes on bf16-representable ones (exact products:
    the same bound), and once per pass on the full-mantissa operands of FULL_MANTISSA_ROW with 2^-8 S for the roundings in the kernel;
  * inputs, and the first launch's output while the second runs, are bit-unchanged;
  * a repeat launch is bit-equal (forward, col2im with its two commuting addends, VALU, GEMM) or within 2 x bound (weight gradients);
  * the padded channel is exactly zero in gx and dw; the weight gradient adds onto a non-zero dw, the accumulating input gradient onto
    a non-zero x.
The views of the 2-D rows -- frame t of a clip as the forward input, the (accumulating) input gradient into frame t of a clip, the
generator's clip-order write plain and with bias + tanh -- keep every other frame of the clip bit-unchanged (finite values, compared by
value); the tanh launches have no derived element bound and keep the project's rel-L2 < 1e-5.  The last test asserts that the kernels,
instantiations and plan classes that ran are the ones the table promises.  Figures measured on an MI355X: profiles/c4_guard_parity.md."""
import numpy as np
import pytest
import torch

from guard import Arena, POISON
import c4_ref as R

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5                             # tests/test_gpu_ops.py: the rel-L2 limit of a forward launch (the tanh launches)
RAN = set()                                # (kernel, <KT, WO>[, precision of the col2im kernel])
CLASSES = {}                               # kernel family -> plan classes that ran
RATIO = {}                                 # (kernel, precision, operands) -> [worst |error| / bound, launches checked]


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return Arena(160 << 20)                # the N = 520 row: y twice (2 x 34 MB), gy as fp32 and bf16, x, margins


def _words(t):
    return t.reshape(-1).view(torch.int32) if t.element_size() == 4 else t.reshape(-1).view(torch.int16)


def _bit_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_words(a), _words(b))


def _is_poison(t):
    return bool((_words(t) == POISON).all())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _geom(hl, g, tile, prec):
    lg = hl.make_geom(g.N, g.Ti, g.Hi, g.Wi, R.CI, R.CO, g.kt, x_stride0=g.x_stride0, x_perm_n=g.x_perm_n, x_stride1=g.x_stride1,
                      precision=prec, ci_valid=R.CV)
    lg.tile = tile
    return lg


def _note(kernel, inst, plan, prec):
    if kernel == 'gemm':
        return
    RAN.add((kernel, inst) + ((prec,) if kernel == 'dgrad_c4_mfma_kernel' else ()))
    CLASSES.setdefault(kernel.replace('_bf16', ''), set()).update(plan['cls'])


def _accept(tag, key, out, ref, L, S, rounded):
    """finite, every element within the bound; the figures first"""
    ratio = R.worst_ratio(out, ref, L, S, rounded)
    print("c4-guard %s: worst |err| / bound %.3g" % (tag, ratio))
    r = RATIO.setdefault(key, [0.0, 0])
    r[0], r[1] = max(r[0], ratio), r[1] + 1
    assert bool(torch.isfinite(out).all()), "%s: a consumed load left its tensor (NaN poison) or an element was not written" % tag
    bad = R.violations(out, ref, L, S, rounded=rounded).nonzero()
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        assert False, "%s: %d of %d elements outside the bound, first at %s: %r against %r (bound %.3e)" % (
            tag, len(bad), out.numel(), at, float(out[at]), float(ref[at]), float(R.bound(L, S, rounded)[at]))


def _unchanged(tag, tensors, snaps):
    for i, (t, s) in enumerate(zip(tensors, snaps)):
        assert _bit_equal(t, s), "%s: input %d (or an earlier output) was written" % (tag, i)


def _refused(hl, tag, call, outs):
    """MCG_ERR_UNSUPPORTED, and nothing written: the outputs are what they were"""
    snaps = [o.clone() for o in outs]
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        call()
    _unchanged(tag + " (refused)", outs, snaps)


class Operands:
    """the two operand sets of a row on the device (full mantissa; bf16-representable) and the float64 references computed from them,
    each once"""

    def __init__(self, row, seed=0):
        self.row, self.seed, self.sets, self.refs = row, seed, {}, {}

    def get(self, kind):
        if kind not in self.sets:
            self.sets[kind] = {k: _dev(v) for k, v in R.inputs(self.row, exact=kind == 'exact', seed=self.seed).items()}
        return self.sets[kind]

    def ref(self, kind, name, make):
        if (kind, name) not in self.refs:
            self.refs[kind, name] = make(self.get(kind))
        return self.refs[kind, name]


def _operand_kinds(row, prec):
    """fp32 launches: full-mantissa operands; the bf16 modes: bf16-representable ones, and on one row the full-mantissa ones too"""
    if prec == 'f32':
        return ['full']
    return ['exact'] + (['full'] if row == R.FULL_MANTISSA_ROW else [])


def _launches(row, pass_):
    precs = ('f32', 'bf16') if pass_ == 'fprop' else R.PRECS
    for tile in R.TILES:
        for prec in precs:
            for kind in _operand_kinds(row, prec):
                yield tile, prec, kind


# ---- the three passes on a dense row ----
def _fprop_row(hl, arena, row, ops):
    g = R.Geo(row)
    L = R.terms('fprop', g)
    for tile, prec, kind in _launches(row, 'fprop'):
        d = ops.get(kind)
        ref, S = ops.ref(kind, 'fprop', lambda d: R.fprop(d['x'], d['w'], d['bias']))
        kernel, inst, plan = R.dispatch(g, 'fprop', tile, prec)
        tag = "%s fprop tile %d %s %s -> %s" % (R.row_id(row), tile, prec, kind, kernel)
        arena.reset()
        ins = [arena.put(d[k]) for k in ('x', 'w', 'bias')]
        snaps = [t.clone() for t in ins]
        lg = _geom(hl, g, tile, prec)
        y1 = arena.empty(tuple(ref.shape))
        if kernel == R.UNSUPPORTED:
            _refused(hl, tag, lambda: hl.conv_fprop(lg, ins[0], ins[1], ins[2], y1), [y1])
            assert _is_poison(y1)
            arena.check()
            continue
        hl.conv_fprop(lg, ins[0], ins[1], ins[2], y1)
        arena.check()
        _accept(tag, (kernel, prec, kind), y1, ref, L, S, rounded=kind == 'full' and prec != 'f32')
        _unchanged(tag, ins, snaps)
        keep = y1.clone()
        y2 = arena.empty(tuple(ref.shape))
        hl.conv_fprop(lg, ins[0], ins[1], ins[2], y2)
        arena.check()
        assert _bit_equal(y2, y1), "%s: a repeat launch differs" % tag
        _unchanged(tag, ins + [y1], snaps + [keep])
        _note(kernel, inst, plan, prec)


def _dgrad_row(hl, arena, row, ops):
    g = R.Geo(row)
    L = R.terms('dgrad', g)
    for tile, prec, kind in _launches(row, 'dgrad'):
        d = ops.get(kind)
        for form in R.dgrad_variants(g):
            acc = form['accumulate']
            ref, S = ops.ref(kind, 'dgrad+x0' if acc else 'dgrad',
                             lambda d: R.dgrad(d['gy'], d['w'], g.Ti, g.Hi, g.Wi, None, d['x0'] if acc else None))
            kernel, inst, plan = R.dispatch(g, 'dgrad', tile, prec, **form)
            tag = "%s dgrad%s tile %d %s %s -> %s" % (R.row_id(row), "+acc" if acc else "", tile, prec, kind, kernel)
            arena.reset()
            gy = arena.put(d['gy'].to(torch.bfloat16) if prec == 'bf16y' else d['gy'])
            ins = [gy, arena.put(d['w'])]
            snaps = [t.clone() for t in ins]
            lg = _geom(hl, g, tile, prec)
            start = lambda: arena.put(d['x0']) if acc else arena.empty(tuple(ref.shape))
            gx1 = start()
            if not acc:
                assert hl.dgrad_c4_mfma_covers(lg) == (kernel == 'dgrad_c4_mfma_kernel'), tag
            if kernel == R.UNSUPPORTED:
                _refused(hl, tag, lambda: hl.conv_dgrad(lg, ins[0], ins[1], None, gx1, accumulate=acc), [gx1])
                assert acc or _is_poison(gx1)
                arena.check()
                continue
            hl.conv_dgrad(lg, ins[0], ins[1], None, gx1, accumulate=acc)
            arena.check()
            _accept(tag, (kernel, prec, kind), gx1, ref, L, S, rounded=kind == 'full' and prec != 'f32')
            assert bool((gx1[..., R.CV:] == 0).all()), "%s: the padded channel is not exactly zero" % tag
            _unchanged(tag, ins, snaps)
            keep = gx1.clone()
            gx2 = start()
            hl.conv_dgrad(lg, ins[0], ins[1], None, gx2, accumulate=acc)
            arena.check()
            assert _bit_equal(gx2, gx1), "%s: a repeat launch differs" % tag
            _unchanged(tag, ins + [gx1], snaps + [keep])
            _note(kernel, inst, plan, prec)


def _wgrad_row(hl, arena, row, ops):
    g = R.Geo(row)
    for tile, prec, kind in _launches(row, 'wgrad'):
        d = ops.get(kind)
        ref, S = ops.ref(kind, 'wgrad', lambda d: R.wgrad(d['x'], d['gy'], g.kt, d['dw0']))
        kernel, inst, plan = R.dispatch(g, 'wgrad', tile, prec)
        tag = "%s wgrad tile %d %s %s -> %s" % (R.row_id(row), tile, prec, kind, kernel)
        arena.reset()
        ins = [arena.put(d['x']), arena.put(d['gy'].to(torch.bfloat16) if prec == 'bf16y' else d['gy'])]
        snaps = [t.clone() for t in ins]
        lg = _geom(hl, g, tile, prec)
        dw1 = arena.put(d['dw0'])                              # the launch adds onto a non-zero dw
        if kernel == R.UNSUPPORTED:
            _refused(hl, tag, lambda: hl.conv_wgrad(lg, ins[0], ins[1], dw1), [dw1])
            arena.check()
            continue
        L = R.terms('wgrad', g, plan['blocks_per_element'])
        rounded = kind == 'full' and prec != 'f32'
        hl.conv_wgrad(lg, ins[0], ins[1], dw1)
        arena.check()
        _accept(tag, (kernel, prec, kind), dw1, ref, L, S, rounded)
        assert bool((dw1[..., R.CV:] == 0).all()), "%s: the padded channel is not exactly zero" % tag
        _unchanged(tag, ins, snaps)
        keep = dw1.clone()
        dw2 = arena.put(d['dw0'])
        hl.conv_wgrad(lg, ins[0], ins[1], dw2)
        arena.check()
        assert not bool(R.violations(dw2, dw1.double(), L, S, scale=2.0).any()), "%s: two launches further apart than 2 x bound" % tag
        assert bool((dw2[..., R.CV:] == 0).all()), tag
        _unchanged(tag, ins + [dw1], snaps + [keep])
        _note(kernel, inst, plan, prec)


ROW_IDS = [R.row_id(r) for r in R.C4_ROWS]


@pytest.mark.parametrize("row", R.C4_ROWS, ids=ROW_IDS)
def test_c4_fprop_in_the_arena(hl, arena, row):
    _fprop_row(hl, arena, row, Operands(row))


@pytest.mark.parametrize("row", R.C4_ROWS, ids=ROW_IDS)
def test_c4_dgrad_in_the_arena(hl, arena, row):
    _dgrad_row(hl, arena, row, Operands(row))


@pytest.mark.parametrize("row", R.C4_ROWS, ids=ROW_IDS)
def test_c4_wgrad_in_the_arena(hl, arena, row):
    _wgrad_row(hl, arena, row, Operands(row))


# ---- the views of the 2-D rows: frames of a clip [clips][T][Hi][Wi][4] ----
def _view_cases():
    return [(row, clips) for row in R.VIEW_ROWS for clips in R.VIEW_CLIPS]


VIEW_IDS = ["%s-clips%d" % (R.row_id(r), c) for r, c in _view_cases()]


def _clip_operands(row, clips):
    """the operands of a clip-shaped row (kt = 1: x, x0 are clips, gy holds one output frame per clip frame)"""
    _, _, hw, _ = row
    return Operands((clips, R.CLIP_T, hw, 1), seed=1 + 2 * R.C4_ROWS.index(row) + clips)


@pytest.mark.parametrize("row,clips", _view_cases(), ids=VIEW_IDS)
def test_c4_frame_view_forward(hl, arena, row, clips):
    """x[:, t] of a clip through x_stride0: no dense x, so the layer's forward kernel refuses (tile 6) and tile 0 takes the GEMM"""
    ops = _clip_operands(row, clips)
    g = R.Geo(row, 'frame', clips)
    L = R.terms('fprop', g)
    for t in (0, R.CLIP_T - 1):
        for tile in R.TILES:
            for prec in ('f32', 'bf16'):
                kind = 'full' if prec == 'f32' else 'exact'
                d = ops.get(kind)
                ref, S = ops.ref(kind, 'fprop%d' % t, lambda d: R.fprop(d['x'][:, t:t + 1], d['w'], d['bias']))
                kernel, inst, plan = R.dispatch(g, 'fprop', tile, prec)
                tag = "%s clips %d frame %d fprop tile %d %s -> %s" % (R.row_id(row), clips, t, tile, prec, kernel)
                arena.reset()
                ins = [arena.put(d[k]) for k in ('x', 'w', 'bias')]
                snaps = [v.clone() for v in ins]
                lg = _geom(hl, g, tile, prec)
                y1 = arena.empty(tuple(ref.shape))
                if kernel == R.UNSUPPORTED:
                    _refused(hl, tag, lambda: hl.conv_fprop(lg, ins[0][:, t], ins[1], ins[2], y1), [y1])
                    assert _is_poison(y1)
                    arena.check()
                    continue
                hl.conv_fprop(lg, ins[0][:, t], ins[1], ins[2], y1)
                arena.check()
                _accept(tag, (kernel + ' frame view', prec, kind), y1, ref, L, S, rounded=False)
                _unchanged(tag, ins, snaps)
                keep = y1.clone()
                y2 = arena.empty(tuple(ref.shape))
                hl.conv_fprop(lg, ins[0][:, t], ins[1], ins[2], y2)
                arena.check()
                assert _bit_equal(y2, y1), "%s: a repeat launch differs" % tag
                _unchanged(tag, ins + [y1], snaps + [keep])


@pytest.mark.parametrize("row,clips", _view_cases(), ids=VIEW_IDS)
def test_c4_frame_view_input_gradient(hl, arena, row, clips):
    """the input gradient written into / added onto frame t of a clip of finite values: every other frame keeps them bit for bit"""
    ops = _clip_operands(row, clips)
    g = R.Geo(row, 'frame', clips)
    L = R.terms('dgrad', g)
    for t in (0, R.CLIP_T - 1):
        for acc in (False, True):
            for tile in R.TILES:
                for prec in R.PRECS:
                    kind = 'full' if prec == 'f32' else 'exact'
                    d = ops.get(kind)

                    def make(d):
                        fr, Sf = R.dgrad(d['gy'][:, t:t + 1], d['w'], 1, g.Hi, g.Wi, None, d['x0'][:, t:t + 1] if acc else None)
                        ref, S = d['x0'].double(), torch.zeros_like(d['x0'], dtype=torch.float64)    # elsewhere: as it was, bound 0
                        ref[:, t:t + 1], S[:, t:t + 1] = fr, Sf
                        return ref, S
                    ref, S = ops.ref(kind, 'dgrad%d%d' % (t, acc), make)
                    kernel, inst, plan = R.dispatch(g, 'dgrad', tile, prec, accumulate=acc)
                    tag = "%s clips %d frame %d dgrad%s tile %d %s -> %s" % (R.row_id(row), clips, t, "+acc" if acc else "", tile, prec, kernel)
                    arena.reset()
                    ins = [arena.put(d['gy'][:, t:t + 1].contiguous().to(torch.bfloat16 if prec == 'bf16y' else torch.float32)), arena.put(d['w'])]
                    snaps = [v.clone() for v in ins]
                    lg = _geom(hl, g, tile, prec)
                    assert not hl.dgrad_c4_mfma_covers(lg)
                    clip1 = arena.put(d['x0'])
                    if kernel == R.UNSUPPORTED:
                        _refused(hl, tag, lambda: hl.conv_dgrad(lg, ins[0], ins[1], None, clip1[:, t], accumulate=acc), [clip1])
                        arena.check()
                        continue
                    hl.conv_dgrad(lg, ins[0], ins[1], None, clip1[:, t], accumulate=acc)
                    arena.check()
                    _accept(tag, (kernel + ' frame view', prec, kind), clip1, ref, L, S, rounded=False)
                    others = [u for u in range(R.CLIP_T) if u != t]
                    assert _bit_equal(clip1[:, others].contiguous(), d['x0'][:, others].contiguous()), "%s: another frame of the clip was written" % tag
                    assert bool((clip1[..., R.CV:] == 0).all()), "%s: the padded channel is not exactly zero" % tag
                    _unchanged(tag, ins, snaps)
                    clip2 = arena.put(d['x0'])
                    hl.conv_dgrad(lg, ins[0], ins[1], None, clip2[:, t], accumulate=acc)
                    arena.check()
                    assert _bit_equal(clip2, clip1), "%s: a repeat launch differs" % tag
                    _note(kernel, inst, plan, prec)


@pytest.mark.parametrize("row,clips", _view_cases(), ids=VIEW_IDS)
def test_c4_clip_order_write(hl, arena, row, clips):
    """T * clips frames written straight into clip order (x_perm_n = clips): plain -- the col2im kernel takes the buffer as whole --
    and with bias + tanh (VALU)"""
    ops = _clip_operands(row, clips)
    g = R.Geo(row, 'perm', clips)
    L = R.terms('dgrad', g)
    launch_order = lambda gy: gy.permute(1, 0, 2, 3, 4).reshape((g.N, 1) + tuple(gy.shape[2:])).contiguous()     # item t * clips + b
    for tanh in (False, True):
        for tile in R.TILES:
            for prec in R.PRECS:
                kind = 'full' if prec == 'f32' else 'exact'
                d = ops.get(kind)

                def make(d):
                    pre, S = R.dgrad(launch_order(d['gy']), d['w'], 1, g.Hi, g.Wi, d['bias4'] if tanh else None)
                    return R.to_clip_order(torch.tanh(pre) if tanh else pre, clips), R.to_clip_order(S, clips)
                ref, S = ops.ref(kind, 'perm%d' % tanh, make)
                kernel, inst, plan = R.dispatch(g, 'dgrad', tile, prec, bias=tanh, act=tanh)
                tag = "%s clips %d clip order%s tile %d %s -> %s" % (R.row_id(row), clips, " bias+tanh" if tanh else "", tile, prec, kernel)
                arena.reset()
                ins = [arena.put(launch_order(d['gy']).to(torch.bfloat16 if prec == 'bf16y' else torch.float32)), arena.put(d['w']),
                       arena.put(d['bias4'])]
                snaps = [v.clone() for v in ins]
                lg = _geom(hl, g, tile, prec)
                run = lambda out: hl.conv_dgrad(lg, ins[0], ins[1], ins[2] if tanh else None, out, act=hl.ACT_TANH if tanh else hl.ACT_NONE)
                if not tanh:
                    assert hl.dgrad_c4_mfma_covers(lg) == (kernel == 'dgrad_c4_mfma_kernel'), tag
                clip1 = arena.empty(tuple(ref.shape))
                if kernel == R.UNSUPPORTED:
                    _refused(hl, tag, lambda: run(clip1), [clip1])
                    assert _is_poison(clip1)
                    arena.check()
                    continue
                run(clip1)
                arena.check()
                assert bool(torch.isfinite(clip1).all()), "%s: poison consumed or an element not written" % tag
                if tanh:
                    rel = float((clip1.double() - ref).norm() / ref.norm())
                    print("c4-guard %s: rel-L2 %.2e" % (tag, rel))
                    assert rel < FWD_TOL, (tag, rel)
                else:
                    _accept(tag, (kernel + ' clip order', prec, kind), clip1, ref, L, S, rounded=False)
                assert bool((clip1[..., R.CV:] == 0).all()), "%s: the padded channel is not exactly zero" % tag
                _unchanged(tag, ins, snaps)
                keep = clip1.clone()
                clip2 = arena.empty(tuple(ref.shape))
                run(clip2)
                arena.check()
                assert _bit_equal(clip2, clip1), "%s: a repeat launch differs" % tag
                _unchanged(tag, ins + [clip1], snaps + [keep])
                _note(kernel, inst, plan, prec)


def test_every_promised_kernel_and_plan_ran():
    """every kernel x <KT, WO> instantiation and every plan class tests/test_c4_ref_cpu.py derives from the table did run"""
    insts = [(kt, wo) for kt in (1, 4) for wo in (16, 32)]
    want = {(k, i) for k in ('fprop_c4_kernel', 'fprop_c4_bf16_kernel', 'wgrad_c4_kernel', 'wgrad_c4_bf16_kernel') for i in insts}
    want |= {('dgrad_c4_mfma_kernel', i, p) for i in insts for p in R.PRECS}
    want |= {('dgrad_c4_kernel', (1,)), ('dgrad_c4_kernel', (4,))}
    assert RAN == want, (sorted(want - RAN), sorted(RAN - want))
    assert CLASSES == {
        'fprop_c4_kernel': {'one block per item', 'row blocks'},
        'dgrad_c4_mfma_kernel': {'one tile per block', 'ntiles > 1024'},
        'dgrad_c4_kernel': {'full blocks', 'partly filled block'},
        'wgrad_c4_kernel': {'tsplit = 1', 'tsplit = 2', 'tsplit = 4', 'tsplit = 8', 'ragged part', 'one-step part', 'empty part', 'nsplit < N'},
    }, CLASSES
    for key in sorted(RATIO):
        print("c4-guard worst |err| / bound  %-34s %-5s %-5s %.3g over %d launches" % (key + tuple(RATIO[key])))
