"""The fused convolution epilogues (mcg_conv_fprop_ex / mcg_conv_dgrad_ex) in the guard arena, their partial sums against float64.

Every operand, side input (bias, addend, bn_y, bn_stats, mask_in) and output (the tensor, mask_out, part) of a fused launch is a view
into ONE poisoned arena (tests/guard.py); `part` is carved with exactly mcg_conv_epilogue_part_bytes bytes and never initialised.  For
every (pass, kernel family, precision, epilogue class, output type) of tests/epilogue_ref.py's SUPPORT matrix, at cases that put a
ragged row tile, a ragged column tile and a group boundary inside a tile:
  runs    -> margins intact; output finite, within the project's tolerance of the float64 oracle and bit-equal to the plain launch
             where the form does not change the stored value; n_slots * slot_stride inside the promised bytes, every float of it
             written, everything behind still poison; the slots added in float64 within the DERIVED bound (epilogue_ref.sums_bound)
             of the sums of the stored values; mask bits against the oracle's pre-activation; inputs and earlier outputs unchanged;
             a second launch bit-identical (no atomics)
  refused -> McgError, and output, part and mask_out still poison.
A combination SUPPORT says runs and the library refuses fails (nothing here catches McgError outside pytest.raises).  The last test
asserts that what ran fused is exactly the "runs" part of SUPPORT."""
import time

import numpy as np
import pytest
import torch

from oracle import functions as F
from oracle import philox
from guard import Arena, POISON
import epilogue_ref as ER

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 1e-5, 1e-4
BF16_HALF_ULP = 2.0 ** -9                  # a bf16 store moves an element by at most that much of itself
SIGMA, SEED, STREAMS = 0.2, 77, (5, 9)

RAN, REFUSED = set(), set()                # (pass, family, precision, class, output type)
RATIO = {}                                 # class -> largest observed |error| / bound of a partial sum
T0 = time.time()


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return Arena(256 << 20)


def L():
    import mocogan_chainer_amd.layout as layout
    return layout


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _bf16_round(a):
    return torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16).double().numpy()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _words(t):
    """a dense tensor of any type as int32 words"""
    return t.reshape(-1).view(torch.int32)


def _bit_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_words(a), _words(b))


def _is_poison(t):
    return bool((_words(t) == POISON).all())


_data, _sides, _noise = {}, {}, {}


def _case_data(case):
    """seeded bf16-representable operands (every precision forms the same exact products) and the oracle's results, once per case"""
    if case not in _data:
        d = ER.dims(case)
        rng = np.random.RandomState(7100 + ER.CASES.index(case))
        x = _bf16_round(rng.uniform(-1, 1, (d['N'], d['Ci'], d['Ti'], d['H'], d['W'])))
        W = _bf16_round(rng.randn(d['Co'], d['Ci'], d['kt'], 4, 4) * 0.1)
        gy = _bf16_round(rng.randn(d['N'], d['Co'], d['To'], d['Ho'], d['Wo']))
        y_ref = F.conv3d_fwd(x, W, None, (1, 2, 2), (0, 1, 1))
        gx_ref, _, _ = F.conv3d_bwd(x, W, gy, (1, 2, 2), (0, 1, 1))
        lay = L()
        gx_rows = np.zeros((d['rows_d'], d['Cip']))
        gx_rows[:, :d['Ci']] = gx_ref.transpose(0, 2, 3, 4, 1).reshape(d['rows_d'], d['Ci'])
        bias_d = np.zeros(d['Cip'], np.float32)
        bias_d[:d['Ci']] = rng.randn(d['Ci']) * 0.2                       # (a padded channel stays zero)
        _data[case] = dict(xd=lay.act_to_dev(dev(x)), wd=lay.conv_w_to_dev(dev(W)), gyd=lay.act_to_dev(dev(gy)),
                           y_rows=y_ref.transpose(0, 2, 3, 4, 1).reshape(d['rows_f'], d['Co']), gx_rows=gx_rows,
                           bias_f=(rng.randn(d['Co']) * 0.3).astype(np.float32), bias_d=bias_d)
    return _data[case]


def _side(pass_, case, groups):
    """side inputs of the epilogues for the output [rows][C] of a pass: noise, the saved BatchNorm input (bf16-representable, so one
    array serves the fp32 and the bf16 form) with synthesized statistics per group -- resampled until |y scale + shift| > 1e-4
    everywhere: the activation mask is then unambiguous -- and random sign words"""
    key = (pass_, case, groups)
    if key not in _sides:
        d = ER.dims(case)
        fp = pass_ == 'fprop'
        rows, C = (d['rows_f'], d['Co']) if fp else (d['rows_d'], d['Cip'])
        shape = (d['N'], d['To'], d['Ho'], d['Wo']) if fp else (d['N'], d['Ti'], d['H'], d['W'])
        sels = ER.group_rows(pass_, *shape, groups)
        rng = np.random.RandomState(9300 + 10 * ER.CASES.index(case) + groups + (0 if fp else 5))
        y = _bf16_round(rng.randn(rows, C) * 1.3 + 0.2)
        stats = []
        for _ in sels:
            mean, istd = 0.2 + 0.1 * rng.randn(C), 0.6 + 0.3 * rng.rand(C)
            gamma, beta = 1 + 0.1 * rng.randn(C), 0.1 * rng.randn(C)
            stats.append(np.concatenate([mean, istd, gamma * istd, beta - mean * gamma * istd]).astype(np.float32))
        for _ in range(50):
            pre = np.empty((rows, C))
            for sel, st in zip(sels, stats):
                pre[sel] = ER.bn_pre_activation(y[sel], st, C)
            bad = np.abs(pre) <= 1e-4
            if not bad.any():
                break
            y[bad] = _bf16_round(rng.randn(int(bad.sum())) * 1.3 + 0.2)
        else:
            raise AssertionError("could not move every pre-activation off its kink")
        words = rng.randint(0, 2 ** 32, (rows, (C + 31) // 32), dtype=np.uint64).astype(np.uint32)      # (bits of columns >= C: anything)
        _sides[key] = dict(sels=sels, bn_y=y, stats=stats, words=words, noise=(0.2 * rng.randn(rows, C)).astype(np.float32))
    return _sides[key]


def _philox_rows(rows, C, groups):
    """the in-kernel noise of all rows: one counter per (row quad, channel) of each GROUP's rows, its own stream per group"""
    key = (rows, C, groups)
    if key not in _noise:
        mg = rows // groups
        _noise[key] = np.concatenate([philox.randn_rowquad(mg, C, SIGMA, SEED, STREAMS[gi]) for gi in range(groups)])
    return _noise[key]


def _operands(hl, pass_, prec, data, d):
    """(the GEMM's activation operand, the filter in the form this pass reads, the filter's other form or None) in the precision's
    memory form"""
    a = data['xd'] if pass_ == 'fprop' else data['gyd']
    wd = data['wd']
    if prec == 'bf16s':
        return a.to(torch.bfloat16), wd.to(torch.bfloat16), None
    if prec == 'f32x3':
        wf = hl.split_planes(wd) if d['Cip'] % 16 == 0 else None
        wb = hl.split_planes(wd, run=16 * d['kt'] * 16 * d['Cip']) if d['Co'] % 16 == 0 else None
        return hl.split_planes(a), (wf if pass_ == 'fprop' else wb), (wb if pass_ == 'fprop' else wf)
    return a, wd, None


def _run(hl, arena, pass_, case, prec):
    d, data = ER.dims(case), _case_data(case)
    fp = pass_ == 'fprop'
    N, C, rows = d['N'], (d['Co'] if fp else d['Cip']), (d['rows_f'] if fp else d['rows_d'])
    oshape = (N, d['To'], d['Ho'], d['Wo'], C) if fp else (N, d['Ti'], d['H'], d['W'], C)
    ref_rows, tol = (data['y_rows'], FWD_TOL) if fp else (data['gx_rows'], BWD_TOL)
    bias_np = data['bias_f'] if fp else data['bias_d']
    nw, vbits = (C + 31) // 32, ER.valid_bits(C)
    a_src, w_src, w_other = _operands(hl, pass_, prec, data, d)
    tiles = ER.tiles_of(pass_, prec, case)
    assert tiles
    for tile in tiles:
        for groups in ((1, 2) if N % 2 == 0 else (1,)):
            side = _side(pass_, case, groups)
            sels, mg = side['sels'], rows // groups
            arena.reset()
            A, Wt = arena.put(a_src), arena.put(w_src)
            inputs = [A, Wt] + ([arena.put(w_other)] if w_other is not None else [])
            bias = arena.put(dev(bias_np))
            bn_y32 = arena.put(dev(side['bn_y']))
            bn_y16 = arena.put(dev(side['bn_y']).to(torch.bfloat16))
            bn_stats = [arena.put(dev(s)) for s in side['stats']]
            addend = [arena.put(dev(side['noise'][sel])) for sel in sels] if fp else []
            mask_in = arena.put(torch.tensor(side['words'].view(np.int32), device="cuda")) if not fp else None
            inputs += [bias, bn_y32, bn_y16] + bn_stats + addend + ([mask_in] if mask_in is not None else [])
            snaps = [t.clone() for t in inputs]
            kept = []                                      # (what, tensor in the arena, copy taken right after its launch)
            g = hl.make_geom(N, d['Ti'], d['H'], d['W'], d['Cip'], d['Co'], d['kt'], precision=prec, ci_valid=d['Ci'] if d['Cip'] != d['Ci'] else 0)
            g.tile = tile
            part_floats = hl.epilogue_part_floats(g, pass_, groups)
            where = (pass_, case, prec, tile, groups)

            def undisturbed(what):
                arena.check()
                for t, s in zip(inputs, snaps):
                    assert _bit_equal(t, s), (where, what, "an input was modified")
                for nm, t, c in kept:
                    assert _bit_equal(t, c), (where, what, "the output of the earlier %s launch was modified" % (nm,))

            def launch(ep, out, b):
                if fp:
                    hl._fprop_ex(g, A, Wt, b, out, ep, split_ok=True)
                else:
                    hl._dgrad_ex(g, A, Wt, b, out, ep, split_ok=True)

            def new_out(kind):
                if kind == 'split':
                    return arena.empty(oshape[:-1] + (4 * C,), torch.bfloat16)
                return arena.empty(oshape, torch.bfloat16 if kind == 'bf16' else torch.float32)

            # ---- the plain launches of this tile code: with the bias and without
            plain = {}
            for nm, b in (('bias', bias), ('none', None)):
                o = arena.empty(oshape)
                if fp:
                    hl._fprop(g, A, Wt, b, o)
                else:
                    hl._dgrad(g, A, Wt, b, o, hl.ACT_NONE, False)
                undisturbed('plain')
                assert bool(torch.isfinite(o).all()), (where, 'plain')
                assert rel_l2(o.reshape(rows, C).cpu().numpy(), ref_rows + (bias_np if b is not None else 0.0)) < tol, (where, 'plain')
                kept.append(('plain', o, o.clone()))
                plain[nm] = o
            f32_of = {}                                    # form tag -> the fp32 output / masked words of the form's fp32 launch

            def fused(cls, out, tag, kw, b, want, same_as=None, bn=None, stats=(None, None)):
                """one fused form: launch (or see it refused), run every check, launch again.  want: the oracle's stored rows."""
                fam = ER.family_of(tile)
                exp = ER.expected(pass_, tile, prec, cls, out, case, groups)
                if fam == 'c4' and tile == 0 and not exp:
                    # the library's own choice: what the Ci = 4 kernel does not carry goes to the register-staged tiles
                    fam = 'reg'
                    exp = ER.SUPPORT[(pass_, fam, prec, cls, out)] and ER.form_ok(pass_, cls, out, case, groups)
                    same_as = None                         # (the plain launch of code 0 is the other kernel)
                key, what = (pass_, fam, prec, cls, out), (cls, out, tag)
                sums = cls in ('stats', 'bn_bwd', 'col')

                def fresh():
                    o = new_out(out)
                    part = arena.empty((part_floats,)) if sums else None
                    mo = arena.empty((rows, nw), torch.int32) if cls == 'act' else None
                    ep = hl.epilogue(groups=groups, part=part, mask_out=mo, out_bf16=out == 'bf16', out_split=out == 'split', **kw)
                    return o, part, mo, ep

                o, part, mo, ep = fresh()
                if not exp:
                    with pytest.raises(hl.McgError):
                        launch(ep, o, b)
                    undisturbed(what)
                    for t in (o, part, mo):
                        assert t is None or _is_poison(t), (where, what, "a refused launch wrote")
                    REFUSED.add(key)
                    return
                launch(ep, o, b)                           # (a refusal here is a failure: SUPPORT says it runs)
                undisturbed(what)
                # -- the stored output
                if out == 'split':
                    planes = o.view(rows, C // 16, 4, 16)
                    assert _is_poison(planes[:, :, 3].contiguous()), (where, what, "the padding plane was written")
                    ref32 = f32_of[(cls, tag)][0]
                    assert torch.equal(planes[:, :, :3], hl.split_planes(ref32).view(rows, C // 16, 4, 16)[:, :, :3]), (where, what)
                    v = planes[:, :, :3].double().sum(2).reshape(rows, C).cpu().numpy()
                else:
                    assert bool(torch.isfinite(o).all()), (where, what, "a consumed load left its tensor or an element was not written")
                    v = o.reshape(rows, C).double().cpu().numpy()
                if out == 'f32':
                    if tag == 'philox':
                        # as test_gpu_ops.py: the drawn normals element by element against oracle/philox.py -- taken off the launch's own
                        # pre-activation (the plain launch of the tile code), so that a long K's fp32 sum does not count as noise
                        drawn = v - ER.leaky_relu(plain['bias'].reshape(rows, C).double().cpu().numpy())
                        assert np.abs(drawn - _philox_rows(rows, C, groups)).max() < 2e-5, (where, what)
                    assert rel_l2(v, want) < tol, (where, what, rel_l2(v, want))
                    f32_of[(cls, tag)] = [o, None]
                else:
                    assert rel_l2(v, want) < tol + (BF16_HALF_ULP if out == 'bf16' else 0.0), (where, what, rel_l2(v, want))
                    if out == 'bf16' and (cls, tag) in f32_of:     # round-to-nearest-even of what the fp32 launch of the form stores
                        assert _bit_equal(o, f32_of[(cls, tag)][0].to(torch.bfloat16)), (where, what)
                if same_as is not None:
                    src = plain[same_as] if out == 'f32' else plain[same_as].to(torch.bfloat16)
                    assert _bit_equal(o, src), (where, what, "the stored value differs from the plain launch")
                # -- the partial sums
                if sums:
                    used = ep.n_slots * ep.slot_stride
                    assert ep.n_slots > 0 and ep.slot_stride == groups * 2 * C, (where, what, ep.n_slots, ep.slot_stride)
                    assert used * 4 <= part_floats * 4, (where, what, "n_slots * slot_stride exceeds mcg_conv_epilogue_part_bytes", used, part_floats)
                    assert bool(torch.isfinite(part[:used]).all()), (where, what, "a slot entry was not written")
                    assert _is_poison(part[used:]), (where, what, "a store behind the last slot")
                    got = part[:used].double().cpu().numpy().reshape(ep.n_slots, groups, 2, C).sum(0)
                    ref, asum = ER.partial_sums(cls, v, sels, bn=bn, stats=stats)
                    err, bound = np.abs(got - ref), ER.sums_bound(asum)
                    if cls == 'col':                       # (sum v, -)
                        err, bound = err[:, :1], bound[:, :1]
                    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
                    print("%s %s: n_slots %d, max |sum - ref| / bound %.4f" % (where, what, ep.n_slots, ratio))
                    RATIO[cls] = max(RATIO.get(cls, 0.0), ratio)
                    assert (err <= bound).all(), (where, what, "partial sums off the float64 sums of the stored values", ratio,
                                                  np.argwhere(err > bound)[:8].tolist())
                # -- the sign bits
                if mo is not None:
                    w = mo.cpu().numpy().view(np.uint32) & vbits
                    pre = ref_rows + bias_np
                    sure = np.abs(pre) > 1e-5
                    assert np.array_equal(ER.unpack_bits(w, C)[sure], (pre >= 0)[sure]), (where, what, "mask_out")
                    if out == 'f32':
                        f32_of[(cls, tag)][1] = w
                    elif (cls, tag) in f32_of:
                        assert np.array_equal(w, f32_of[(cls, tag)][1]), (where, what, "mask words differ between output types")
                # -- a second launch on the same inputs
                o2, part2, mo2, ep2 = fresh()
                launch(ep2, o2, b)
                undisturbed(what)
                if out == 'split':
                    assert torch.equal(o2.view(rows, C // 16, 4, 16)[:, :, :3], o.view(rows, C // 16, 4, 16)[:, :, :3]), (where, what, "two launches differ")
                else:
                    assert _bit_equal(o2, o), (where, what, "two launches differ")
                assert part is None or (ep2.n_slots == ep.n_slots and _bit_equal(part2[:used], part[:used])), (where, what, "part differs between two launches")
                assert mo is None or _bit_equal(mo2, mo), (where, what, "mask_out differs between two launches")
                for t in (o, part, mo):
                    if t is not None:
                        kept.append((what, t, t.clone()))
                RAN.add(key)

            with_bias = ref_rows + bias_np
            fused('stats', 'f32', '', dict(sums=hl.SUMS_STATS), bias, with_bias, same_as='bias')
            for out, y_t, acts in (('f32', bn_y32, ('relu', 'lrelu')), ('bf16', bn_y16, ('relu',) if fp else ('lrelu',))):
                for act in acts:
                    fused('bn_bwd', out, act, dict(sums=hl.SUMS_BN_BWD, bn_y=y_t, bn_stats=bn_stats, bn_act=hl.ACT_RELU if act == 'relu' else hl.ACT_LRELU),
                          None, ref_rows, same_as='none', bn=(side['bn_y'], act), stats=side['stats'])
            if fp:
                lre = ER.leaky_relu(with_bias)
                for out in ('f32', 'bf16', 'split'):
                    fused('act', out, 'addend', dict(act=hl.ACT_LRELU, addend=addend), bias, lre + side['noise'])
                    if mg % 4 == 0:
                        fused('act', out, 'philox', dict(act=hl.ACT_LRELU, sigma=SIGMA, seed=SEED, stream_id=STREAMS[:groups]), bias,
                              lre + _philox_rows(rows, C, groups))
                fused('plain', 'bf16', '', dict(), bias, with_bias, same_as='bias')
            else:
                mult = ER.lrelu_bwd_multiplier(side['words'], C)
                fused('col', 'f32', '', dict(sums=hl.SUMS_COL, mask_in=mask_in), None, ref_rows * mult)
                fused('mask', 'f32', '', dict(mask_in=mask_in), None, ref_rows * mult)
                fused('plain', 'bf16', 'relu', dict(act=hl.ACT_RELU), bias, np.maximum(with_bias, 0.0))


def _params(pass_):
    return [pytest.param(c, p, id="%s-%s" % ("x".join(str(v) for v in c).replace(" ", ""), p))
            for c in ER.CASES for p in ER.PRECS if ER.tiles_of(pass_, p, c)]


@pytest.mark.parametrize("case,prec", _params('fprop'))
def test_fused_forward_launches_in_the_arena(hl, arena, case, prec):
    _run(hl, arena, 'fprop', case, prec)


@pytest.mark.parametrize("case,prec", _params('dgrad'))
def test_fused_input_gradient_launches_in_the_arena(hl, arena, case, prec):
    _run(hl, arena, 'dgrad', case, prec)


def test_the_whole_support_matrix_ran():
    """what ran fused above is exactly what SUPPORT says runs (and nothing it says is refused ran)"""
    runs = {k for k, v in ER.SUPPORT.items() if v}
    print("ran fused: %d combinations, refused: %d; largest |error| / bound per class: %s; module time %.1f s"
          % (len(RAN), len(REFUSED), {k: round(v, 4) for k, v in sorted(RATIO.items())}, time.time() - T0))
    for k in sorted(ER.SUPPORT):
        print("%-6s %-10s %-6s %-7s %-5s %s" % (k + ("ran" if k in RAN else "refused" if k in REFUSED else "not launched",)))
    assert RAN == runs, (sorted(runs - RAN), sorted(RAN - runs))
    # the issue's production combinations are among them
    assert ('fprop', 'reg', 'f32', 'bn_bwd', 'f32') in RAN and ('fprop', 'posmajor', 'f32x3', 'bn_bwd', 'f32') in RAN
