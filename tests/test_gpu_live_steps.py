"""Position-major rows and live K-steps in the dense MCG_PREC_SPLIT ('f32x3') forward -- tile codes 27 / 40 (tiles 7 / 10, one block
per tile, filter taps that read zero padding for every row of the tile left out of the K loop), 37 (27 with nothing left out) and
1027 / 2027 / 1040 / 2040 (the tiles cut into blocks of equal live work, partial tiles added with float atomics).

Yardstick: the float64 oracle at the tolerance of the split forms, err < 2e-6 and err < 2 * err32 + 1e-7, err32 the error of the
fp32-MFMA kernels on the same inputs.  Where ONE block writes an output element the skipping must not change a bit: a skipped
K-step multiplies zeros only, so 27 equals 37 exactly (and, in a 2-D layer, whose K axis the row-major form does not rotate, 17).
Outputs live in a guard-band arena: a wrong entry of the block table shows as a corrupted band or a NaN, not as a fault.

The weight gradient has a position-major PIXEL axis (27: 128x256/3 dense, 28: 256x256/2 padded; + 1000 / + 2000 double / halve
the pixel splits): held to the oracle where N To is a multiple of its K advance (64 / 16 pixels), refused elsewhere.  It has no
skipping-off twin and sums the pixels in another order than 17, so there is no bit-for-bit partner for it.  The input gradient has
no position-major form and refuses the codes."""
import numpy as np
import pytest
import torch

import guard
from oracle import functions as F

pytestmark = pytest.mark.gpu

# N, Ti, H, Ci, Co, kt
CASES = [(32, 7, 8, 64, 128, 4),       # 128 rows per position: uniform tiles, skipping fires
         (3, 7, 8, 64, 128, 4),        # 12 rows per position: tiles straddle many positions, OR-mask path
         (5, 1, 16, 128, 128, 1),      # ragged last tile, 2-D
         (64, 1, 8, 64, 128, 1),       # 2-D, uniform tiles
         (2, 7, 4, 64, 128, 4)]        # Ho = 2: every position is a border
ONE_BLOCK = [27, 40]                   # one block per tile
CHUNKED = [1027, 2027, 1040, 2040]     # tiles cut by live K-steps
NO_SKIP = 37                           # 27 without the skipping
SUM_TOL = 1e-5                         # tests/test_gpu_partials.py: statistics from per-tile partial sums
STRIDE, PAD = (1, 2, 2), (0, 1, 1)


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return guard.Arena(64 << 20)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def rel_l2(a, b):
    a = a.detach().cpu().double().numpy()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def within_oracle_tolerance(err, err32):
    return err < 2e-6 and err < 2 * err32 + 1e-7


class Operands:
    """full-mantissa fp32 inputs of one case, the float64 oracle's forward result, the split tensors and the fp32-MFMA kernel's
    error -- computed once per case and shared, read-only, by every test"""
    _made = {}

    def __init__(self, hl, case):
        import mocogan_chainer_amd.layout as lay
        N, Ti, H, Ci, Co, kt = case
        self.case, self.lay = case, lay
        rng = np.random.RandomState(4100 + sum(case))
        x = rng.uniform(-1, 1, (N, Ci, Ti, H, H)).astype(np.float32).astype(np.float64)
        W = (rng.randn(Co, Ci, kt, 4, 4) * 0.1).astype(np.float32).astype(np.float64)
        b = rng.randn(Co).astype(np.float32).astype(np.float64)
        self.b = b
        self.y_ref = F.conv3d_fwd(x, W, b, STRIDE, PAD)
        self.xd, self.wd, self.bd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b)
        self.xs, self.ws = hl.split_planes(self.xd), hl.split_planes(self.wd)
        g32 = hl.make_geom(N, Ti, H, H, Ci, Co, kt)
        self.shape = (N, g32.To, g32.Ho, g32.Wo, Co)
        y32 = torch.empty(self.shape, device="cuda")
        hl.conv_fprop(g32, self.xd, self.wd, self.bd, y32)
        self.err32 = self.err_y(y32)

    @classmethod
    def of(cls, hl, case):
        if case not in cls._made:
            cls._made[case] = cls(hl, case)
        return cls._made[case]

    def geom(self, hl, tile):
        N, Ti, H, Ci, Co, kt = self.case
        g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='f32x3')
        g.tile = tile
        return g

    def err_y(self, y, ref=None):
        return rel_l2(self.lay.act_from_dev(y, self.case[4]), self.y_ref if ref is None else ref)

    def fprop(self, hl, arena, tile, fill=3.0, bias=True, **kw):
        """the forward on the split operands into a pre-filled output inside the arena; the bands are checked after the launch"""
        arena.reset()
        y = arena.full(self.shape, fill)
        fused = hl.conv_fprop(self.geom(hl, tile), self.xs, self.ws, self.bd if bias else None, y, **kw)
        arena.check()
        return (y.clone(), fused) if kw else y.clone()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tile", ONE_BLOCK + CHUNKED)
def test_forward_matches_the_oracle(hl, arena, case, tile):
    """(a) one block per tile and tiles cut by live steps, against float64"""
    o = Operands.of(hl, case)
    err = o.err_y(o.fprop(hl, arena, tile))
    print("fprop", case, tile, "err", err, "err32", o.err32)
    assert within_oracle_tolerance(err, o.err32), (err, o.err32)


@pytest.mark.parametrize("case", CASES)
def test_skipping_removes_only_zero_steps(hl, arena, case):
    """(b) code 27 against code 37, the same rows, tiles and order of products with every K-step run: bit for bit"""
    o = Operands.of(hl, case)
    y, y_all = o.fprop(hl, arena, 27), o.fprop(hl, arena, NO_SKIP)
    err = o.err_y(y_all)
    print("fprop", case, NO_SKIP, "err", err, "err32", o.err32)
    assert within_oracle_tolerance(err, o.err32), (err, o.err32)
    assert torch.equal(y, y_all), guard.describe_diff(y, y_all, names=("27", "37"))
    if case[5] == 1:        # a 2-D layer: the row-major dense form visits K in the same order
        for code, same_tile in ((27, 17), (40, 20)):
            a, b = o.fprop(hl, arena, code), o.fprop(hl, arena, same_tile)
            assert torch.equal(a, b), guard.describe_diff(a, b, names=(str(code), str(same_tile)))


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tile", CHUNKED)
def test_chunked_forward_clears_the_output_and_adds_the_bias_once(hl, arena, case, tile):
    """(c) partial tiles are added onto y: whatever y held is gone, and exactly one block of a tile carries the bias"""
    o = Operands.of(hl, case)
    for fill in (3.0, -1e4):
        err = o.err_y(o.fprop(hl, arena, tile, fill=fill))
        assert within_oracle_tolerance(err, o.err32), (fill, err, o.err32)
    err = o.err_y(o.fprop(hl, arena, tile, bias=False), ref=o.y_ref - o.b.reshape(1, -1, 1, 1, 1))
    assert within_oracle_tolerance(err, o.err32), ("no bias", err, o.err32)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("tile", ONE_BLOCK)
def test_statistics_epilogue_on_position_major_rows(hl, arena, case, tile):
    """(d) the BatchNorm-statistics epilogue, two groups where the batch is even: the output bit for bit that of the plain launch,
    and each group's statistics from the partial sums against mcg_bn_stats of that group's rows"""
    o = Operands.of(hl, case)
    N, Ti, H, Ci, Co, kt = case
    groups = 2 if N % 2 == 0 else 1
    g = o.geom(hl, tile)
    y = o.fprop(hl, arena, tile)
    part = torch.zeros(hl.epilogue_part_floats(g, 'fprop', groups), device="cuda")
    ep = hl.epilogue(sums=hl.SUMS_STATS, groups=groups, part=part)
    y2, fused = o.fprop(hl, arena, tile, ep=ep, must_fuse=True)
    assert fused and torch.equal(y2, y)
    assert ep.n_slots > 0 and ep.slot_stride == groups * 2 * Co
    rng = np.random.RandomState(N + Co)
    gamma, beta = dev(1 + 0.1 * rng.randn(Co)), dev(0.1 * rng.randn(Co))
    ws = torch.empty(hl.bn_workspace_floats(Co), device="cuda")
    M = y2.numel() // Co // groups
    for gi in range(groups):
        rows = y2[gi * (N // groups):(gi + 1) * (N // groups)].contiguous()
        got, want = torch.empty(4 * Co, device="cuda"), torch.empty(4 * Co, device="cuda")
        hl.bn_stats_from_partials(M, Co, part[gi * 2 * Co:], ep.n_slots, ep.slot_stride, gamma, beta, got,
                                  torch.zeros(Co, device="cuda"), torch.ones(Co, device="cuda"), ws)
        hl.bn_stats(M, Co, rows, gamma, beta, want, torch.zeros(Co, device="cuda"), torch.ones(Co, device="cuda"), ws)
        for i, k in enumerate(('mean', 'inv_std', 'scale', 'shift')):
            err = rel_l2(got[i * Co:(i + 1) * Co], want[i * Co:(i + 1) * Co].double().cpu().numpy())
            print("stats", case, tile, "group", gi, k, err)
            assert err < SUM_TOL, (gi, k, err)


def test_chunked_codes_cannot_carry_an_epilogue(hl, arena):
    """a partial tile cannot carry an epilogue: must_fuse drops the cut (code % 1000), without it the plain launch runs"""
    o = Operands.of(hl, CASES[3])
    g = o.geom(hl, 1027)
    part = torch.zeros(hl.epilogue_part_floats(g, 'fprop', 1), device="cuda")
    ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part)
    y, fused = o.fprop(hl, arena, 1027, ep=ep, must_fuse=True)
    assert fused and torch.equal(y, o.fprop(hl, arena, 27))
    y, fused = o.fprop(hl, arena, 1027, ep=ep, must_fuse=False)
    assert not fused and within_oracle_tolerance(o.err_y(y), o.err32)


@pytest.mark.parametrize("tile", ONE_BLOCK + [NO_SKIP, 1027])
def test_the_other_passes_refuse_the_codes(hl, tile):
    """position-major rows exist for the forward only; 37 exists for tile 7 alone; the weight gradient refuses 27 where N To (5 here) is no multiple of its K advance; 29 is no code"""
    o = Operands.of(hl, CASES[2])
    N, Ti, H, Ci, Co, kt = o.case
    g = o.geom(hl, tile)
    gy = torch.randn(o.shape, device="cuda")
    gys = hl.split_planes(gy)
    dw = torch.ones_like(o.wd)
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        hl.conv_wgrad(g, o.xs, gys, dw)
    assert bool((dw == 1).all())
    gx = torch.full_like(o.xd, 7.0)
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        hl.conv_dgrad(g, gys, hl.split_planes(o.wd, run=16 * kt * 16 * Ci), None, gx)
    assert bool((gx == 7).all())
    y = torch.full(o.shape, 3.0, device="cuda")
    g.tile = 29
    with pytest.raises(hl.McgError, match="MCG_ERR_BAD_ARG"):
        hl.conv_fprop(g, o.xs, o.ws, None, y)
    g16 = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='bf16s')
    g16.tile = tile
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        hl.conv_fprop(g16, o.xd.bfloat16(), o.wd.bfloat16(), None, y)
    assert bool((y == 3).all())


def _shipped_live():
    import json
    import os
    import mocogan_chainer_amd.hiplib as hiplib
    pkg = os.path.dirname(hiplib.__file__)
    path = os.path.join(pkg, 'live_tiles_mi355x.json')
    dense = {tuple(k): v for k, v in json.load(open(os.path.join(pkg, 'dense_tiles_mi355x.json')))}
    return [(tuple(k), v, dense.get(tuple(k), 17)) for k, v in json.load(open(path))] if os.path.exists(path) else []


@pytest.mark.parametrize("entry", _shipped_live(), ids=lambda e: "%s-%s-%d" % (e[0][0], "x".join(str(v) for v in e[0][1:8]), e[1]))
def test_shipped_launches_at_their_production_geometry(hl, entry):
    """every launch the shipped list moves, at the batch it was measured at, against the dense row-major form of a code held to the
    oracle at the small shapes: both are within 2e-6 of the exact result there, hence within 4e-6 of each other (the bound
    tests/test_gpu_dense_split.py uses for forms that add partial tiles in another order)"""
    key, code, ref_code = entry
    kind, N, Ti, Hi, Wi, Ci, Co, kt = key[:8]
    g = hl.make_geom(N, Ti, Hi, Wi, Ci, Co, kt, precision='f32x3')
    gen = torch.Generator(device="cuda").manual_seed(N + Ti + Ci)
    x = torch.rand((N, Ti, Hi, Wi, Ci), device="cuda", generator=gen) * 2 - 1
    w = torch.randn((Co, kt, 4, 4, Ci), device="cuda", generator=gen) * 0.05
    b = torch.randn((Co,), device="cuda", generator=gen)
    gy = torch.randn((N, g.To, g.Ho, g.Wo, Co), device="cuda", generator=gen)
    ref_code = ref_code % 1000 if kind == "fprop" else 17       # (a weight gradient: the dense row-major 128x256 tile)
    out = {}
    if kind == "fprop":
        xs, ws = hl.split_planes(x), hl.split_planes(w)
        for c in (code, ref_code):
            g.tile = c
            out[c] = torch.full_like(gy, 3.0)
            hl.conv_fprop(g, xs, ws, b, out[c])
    else:
        assert kind == "wgrad"
        xs, gys = hl.split_planes(x), hl.split_planes(gy)
        for c in (code, ref_code):
            g.tile = c
            out[c] = torch.zeros_like(w)
            hl.conv_wgrad(g, xs, gys, out[c])
    a, r = out[code].double(), out[ref_code].double()
    d = float((a - r).norm() / r.norm())
    print(key, code, "rel-L2 to code", ref_code, d)
    assert d < 4e-6, d


# ---- the weight gradient: the issue's cases whose N To is a multiple of 64, and one more for the padded 256x256 tile (Co >= 256,
# N To = 32: a multiple of 16 but not of 64 -- 28 runs, 27 is refused)
WGRAD_CASES = [c for c in CASES if (c[0] * (c[1] - c[5] + 1)) % 64 == 0]
WGRAD_PADDED_CASE = (32, 1, 8, 64, 256, 1)


class WgradOperands:
    _made = {}

    def __init__(self, hl, case):
        import mocogan_chainer_amd.layout as lay
        N, Ti, H, Ci, Co, kt = case
        self.case, self.lay = case, lay
        rng = np.random.RandomState(5200 + sum(case))
        x = rng.uniform(-1, 1, (N, Ci, Ti, H, H)).astype(np.float32).astype(np.float64)
        gy = rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2).astype(np.float32).astype(np.float64)
        W0 = np.zeros((Co, Ci, kt, 4, 4))
        _, self.gW_ref, _ = F.conv3d_bwd(x, W0, gy, STRIDE, PAD, need_gx=False)
        self.xd, self.gyd = lay.act_to_dev(dev(x)), lay.act_to_dev(dev(gy))
        self.wshape = tuple(lay.conv_w_to_dev(dev(W0)).shape)
        self.xs, self.gys = hl.split_planes(self.xd), hl.split_planes(self.gyd)
        dw32 = torch.ones(self.wshape, device="cuda")
        hl.conv_wgrad(hl.make_geom(N, Ti, H, H, Ci, Co, kt), self.xd, self.gyd, dw32)
        self.err32 = self.err_dw(dw32)

    @classmethod
    def of(cls, hl, case):
        if case not in cls._made:
            cls._made[case] = cls(hl, case)
        return cls._made[case]

    def err_dw(self, dw):                              # (dw starts from ones: the kernels add onto it)
        return rel_l2(self.lay.conv_w_from_dev(dw, self.case[3], 3), self.gW_ref + 1)

    def wgrad(self, hl, arena, tile):
        N, Ti, H, Ci, Co, kt = self.case
        g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='f32x3')
        g.tile = tile
        arena.reset()
        dw = arena.full(self.wshape, 1.0)
        hl.conv_wgrad(g, self.xs, self.gys, dw)
        arena.check()
        return dw.clone()


@pytest.mark.parametrize("case", WGRAD_CASES)
@pytest.mark.parametrize("tile", [27, 1027, 2027])
def test_weight_gradient_matches_the_oracle(hl, arena, case, tile):
    """(a) the dense 128x256 tile with a position-major pixel axis, one or more pixel splits, against float64"""
    o = WgradOperands.of(hl, case)
    err = o.err_dw(o.wgrad(hl, arena, tile))
    print("wgrad", case, tile, "err", err, "err32", o.err32)
    assert within_oracle_tolerance(err, o.err32), (err, o.err32)


@pytest.mark.parametrize("tile", [28, 1028, 2028])
def test_padded_weight_gradient_matches_the_oracle_and_the_dense_code_is_refused(hl, arena, tile):
    """N To = 32: whole advances of 16 pixels per position, not of 64"""
    o = WgradOperands.of(hl, WGRAD_PADDED_CASE)
    err = o.err_dw(o.wgrad(hl, arena, tile))
    print("wgrad", WGRAD_PADDED_CASE, tile, "err", err, "err32", o.err32)
    assert within_oracle_tolerance(err, o.err32), (err, o.err32)
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        o.wgrad(hl, arena, tile - 1)


def test_weight_gradient_is_refused_without_whole_advances_per_position(hl, arena):
    """(3, 7, 8, 64, 128, 4): N To = 12 -- the library's error, and dw untouched"""
    N, Ti, H, Ci, Co, kt = CASES[1]
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='f32x3')
    g.tile = 27
    xs = torch.zeros((N, Ti, H, H, 4 * Ci), device="cuda", dtype=torch.bfloat16)
    gys = torch.zeros((N, g.To, g.Ho, g.Wo, 4 * Co), device="cuda", dtype=torch.bfloat16)
    dw = torch.ones((Co, kt, 4, 4, Ci), device="cuda")
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        hl.conv_wgrad(g, xs, gys, dw)
    assert bool((dw == 1).all())
