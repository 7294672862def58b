"""The dense LDS form of the MCG_PREC_SPLIT ('f32x3') GEMMs -- tile codes 17 / 20 = tiles 7 / 10 without the padding plane in LDS.

The form changes where the loads fetch from and how the K loop is cut into steps, not the order of the products per accumulator:
wherever ONE block writes an output element (no K split, a weight gradient with one pixel split) the result must be bit for bit
that of the padded form of the same tile.  Where partial tiles are added with float atomics the order is free, and the yardstick
is the float64 oracle at the tolerance of test_split_fp32_products_match_the_oracle: err < 2e-6 and err < 2 * err32 + 1e-7, err32
the error of the fp32-MFMA kernels on the same inputs."""
import numpy as np
import pytest
import torch

import guard
from oracle import functions as F

pytestmark = pytest.mark.gpu

# N, Ti, H, Ci, Co, kt
CASES = [(2, 7, 16, 64, 128, 4),       # one triple per tap in forward; dgrad's 256x64 tile; To = 4: dead temporal taps (next_valid, idle split blocks)
         (3, 1, 16, 128, 64, 1),       # ragged row tile; dgrad K = 64 channels: one triple per sub-filter tap
         (1, 5, 8, 256, 256, 4),       # long K
         (5, 1, 8, 128, 512, 1),       # wide Co
         (3, 1, 8, 64, 128, 1)]        # weight gradient with 48 pixels: a last (only) triple with out-of-range pixels
PIXSPLIT_CASE = (4, 7, 16, 64, 128, 4)  # 1024 output pixels: the dense weight gradient runs two pixel splits of 8 triples
DENSE = {17: 7, 20: 10}                # dense code -> the padded code of the same tile
STRIDE, PAD = (1, 2, 2), (0, 1, 1)


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def rel_l2(a, b):
    a = a.detach().cpu().double().numpy()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def within_oracle_tolerance(err, err32):
    return err < 2e-6 and err < 2 * err32 + 1e-7


class Operands:
    """full-mantissa fp32 inputs of one case, the float64 oracle's three results, the split tensors and the fp32-MFMA kernels'
    errors -- computed once per case and shared, read-only, by every test"""
    _made = {}

    def __init__(self, hl, case):
        import mocogan_chainer_amd.layout as lay
        N, Ti, H, Ci, Co, kt = case
        self.case, self.lay = case, lay
        rng = np.random.RandomState(9700 + sum(case))
        x = rng.uniform(-1, 1, (N, Ci, Ti, H, H)).astype(np.float32).astype(np.float64)
        W = (rng.randn(Co, Ci, kt, 4, 4) * 0.1).astype(np.float32).astype(np.float64)
        b = rng.randn(Co).astype(np.float32).astype(np.float64)
        gy = rng.randn(N, Co, Ti - kt + 1, H // 2, H // 2).astype(np.float32).astype(np.float64)
        self.y_ref = F.conv3d_fwd(x, W, b, STRIDE, PAD)
        self.gx_ref, self.gW_ref, _ = F.conv3d_bwd(x, W, gy, STRIDE, PAD)
        self.xd, self.wd, self.bd, self.gyd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W)), dev(b), lay.act_to_dev(dev(gy))
        self.xs, self.ws, self.gys = hl.split_planes(self.xd), hl.split_planes(self.wd), hl.split_planes(self.gyd)
        self.wsd = hl.split_planes(self.wd, run=16 * kt * 16 * Ci)
        self.mpix = N * (Ti - kt + 1) * (H // 2) ** 2
        self.has_dgrad = Ci >= 64                      # the LDS-DMA dgrad tiles need >= 64 output columns
        self.has_wgrad = Co >= 128 and Ci >= 64        # ... and the weight-gradient tiles Co >= 128
        g32 = hl.make_geom(N, Ti, H, H, Ci, Co, kt)
        y32, gx32, dw32 = torch.empty_like(self.y_like(hl)), torch.empty_like(self.xd), torch.ones_like(self.wd)
        hl.conv_fprop(g32, self.xd, self.wd, self.bd, y32)
        hl.conv_dgrad(g32, self.gyd, self.wd, None, gx32)
        hl.conv_wgrad(g32, self.xd, self.gyd, dw32)
        self.err32 = {"y": self.err_y(y32), "gx": self.err_gx(gx32), "dw": self.err_dw(dw32)}

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

    def y_like(self, hl, fill=3.0):
        g = self.geom(hl, 0)
        return torch.full((g.N, g.To, g.Ho, g.Wo, g.Co), fill, device="cuda")

    def err_y(self, y):
        return rel_l2(self.lay.act_from_dev(y, self.case[4]), self.y_ref)

    def err_gx(self, gx):
        return rel_l2(self.lay.act_from_dev(gx, self.case[3]), self.gx_ref)

    def err_dw(self, dw):                              # (dw starts from ones: the kernels add onto it)
        return rel_l2(self.lay.conv_w_from_dev(dw, self.case[3], 3), self.gW_ref + 1)

    # the three passes on the split operands
    def fprop(self, hl, tile, **kw):
        y = self.y_like(hl)
        hl.conv_fprop(self.geom(hl, tile), self.xs, self.ws, self.bd, y, **kw)
        return y

    def dgrad(self, hl, tile, bias=None, **kw):
        gx = torch.full_like(self.xd, 7.0)
        hl.conv_dgrad(self.geom(hl, tile), self.gys, self.wsd, bias, gx, **kw)
        return gx

    def wgrad(self, hl, tile):
        dw = torch.ones_like(self.wd)
        hl.conv_wgrad(self.geom(hl, tile), self.xs, self.gys, dw)
        return dw


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dense", sorted(DENSE))
def test_dense_form_is_bit_for_bit_the_padded_form(hl, case, dense):
    """forward, input gradient and weight gradient, one block per output element: torch.equal with the padded form of the same
    tile (and, so that the pair cannot be wrong together, the oracle tolerance)"""
    o = Operands.of(hl, case)
    g = o.geom(hl, dense)
    assert hl.dense_split_ok("fprop", g)
    y, yp = o.fprop(hl, dense), o.fprop(hl, DENSE[dense])
    err = o.err_y(y)
    print("fprop", case, dense, "err", err, "err32", o.err32["y"])
    assert within_oracle_tolerance(err, o.err32["y"]), (err, o.err32["y"])
    assert torch.equal(y, yp), guard.describe_diff(y, yp, names=("dense", "padded"))
    if o.has_dgrad:
        assert hl.dense_split_ok("dgrad", g)
        gx, gxp = o.dgrad(hl, dense), o.dgrad(hl, DENSE[dense])
        err = o.err_gx(gx)
        print("dgrad", case, dense, "err", err, "err32", o.err32["gx"])
        assert within_oracle_tolerance(err, o.err32["gx"]), (err, o.err32["gx"])
        assert torch.equal(gx, gxp), guard.describe_diff(gx, gxp, names=("dense", "padded"))
    if o.has_wgrad:
        assert hl.dense_split_ok("wgrad", g)
        # <= 512 pixels: one pixel split in either form (the padded form keeps >= 32 K-steps of 16 pixels per block, the dense
        # one >= 8 triples of 64), so every element of dw receives exactly one atomic add
        assert o.mpix <= 512 and hl.dense_split_chunk("wgrad", g) >= o.mpix
        dw, dwp = o.wgrad(hl, dense), o.wgrad(hl, DENSE[dense])
        err = o.err_dw(dw)
        print("wgrad", case, dense, "err", err, "err32", o.err32["dw"])
        assert within_oracle_tolerance(err, o.err32["dw"]), (err, o.err32["dw"])
        assert torch.equal(dw, dwp), guard.describe_diff(dw, dwp, names=("dense", "padded"))
    else:
        assert not hl.dense_split_ok("wgrad", g)
        with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
            o.wgrad(hl, dense)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dense", sorted(DENSE))
@pytest.mark.parametrize("ksplit", [1000, 2000])
def test_dense_form_with_k_split_matches_the_oracle(hl, case, dense, ksplit):
    """the K range of a tile over 2 / 4 blocks (whole triples each), partial tiles added with float atomics"""
    o = Operands.of(hl, case)
    g = o.geom(hl, dense + ksplit)
    for kind in ("fprop", "dgrad"):
        chunk = hl.dense_split_chunk(kind, g)
        assert chunk > 0 and chunk % 256 == 0, (kind, chunk)
    err = o.err_y(o.fprop(hl, dense + ksplit))
    print("fprop", case, dense + ksplit, "err", err, "err32", o.err32["y"])
    assert within_oracle_tolerance(err, o.err32["y"]), (err, o.err32["y"])
    if o.has_dgrad:
        err = o.err_gx(o.dgrad(hl, dense + ksplit))
        print("dgrad", case, dense + ksplit, "err", err, "err32", o.err32["gx"])
        assert within_oracle_tolerance(err, o.err32["gx"]), (err, o.err32["gx"])


@pytest.mark.parametrize("tile", [17, 20, 1020, 2017])
def test_dense_weight_gradient_with_pixel_splits_matches_the_oracle(hl, tile):
    """more than one pixel split (whole triples of 64 pixels each; + 1000 / + 2000 doubles / halves the block target)"""
    o = Operands.of(hl, PIXSPLIT_CASE)
    g = o.geom(hl, tile)
    chunk = hl.dense_split_chunk("wgrad", g)
    assert chunk % 64 == 0
    if tile < 2000:
        assert 0 < chunk < o.mpix, chunk                  # (the case is there for this: the sum really is split)
    err = o.err_dw(o.wgrad(hl, tile))
    print("wgrad", tile, "chunk", chunk, "err", err, "err32", o.err32["dw"])
    assert within_oracle_tolerance(err, o.err32["dw"]), (err, o.err32["dw"])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dense", sorted(DENSE))
def test_dense_form_under_the_fused_epilogues(hl, case, dense):
    """the statistics epilogue (forward) and the first layer's mask multiply + column sums (input gradient) on a dense launch:
    the dense plain launch's output bit for bit, and the sums of it at the tolerances of the padded form's tests"""
    o = Operands.of(hl, case)
    N, Ti, H, Ci, Co, kt = case
    g = o.geom(hl, dense)
    y = o.fprop(hl, dense)
    part = torch.zeros(hl.epilogue_part_floats(g, 'fprop', 1), device="cuda")
    ep = hl.epilogue(sums=hl.SUMS_STATS, groups=1, part=part)
    y2 = torch.empty_like(y)
    assert hl.conv_fprop(g, o.xs, o.ws, o.bd, y2, ep=ep, must_fuse=True)
    assert torch.equal(y2, y)
    sums = part[:ep.n_slots * ep.slot_stride].view(ep.n_slots, ep.slot_stride).double().sum(0)
    v = y2.double().view(-1, Co)
    assert torch.allclose(sums[:Co], v.sum(0), rtol=1e-5, atol=1e-3) and torch.allclose(sums[Co:2 * Co], (v * v).sum(0), rtol=1e-5, atol=1e-3)
    if not o.has_dgrad:
        return
    gx = o.dgrad(hl, dense)
    torch.manual_seed(sum(case))
    bits = torch.randint(0, 2, (N * Ti * H * H, Ci), device="cuda", dtype=torch.int64)
    words = (bits.view(-1, Ci // 32, 32) << torch.arange(32, device="cuda")).sum(-1)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()
    part = torch.zeros(hl.epilogue_part_floats(g, 'dgrad', 1), device="cuda")
    ep = hl.epilogue(mask_in=words, sums=hl.SUMS_COL, groups=1, part=part)
    gxm = torch.empty_like(gx)
    assert hl.conv_dgrad(g, o.gys, o.wsd, None, gxm, ep=ep, must_fuse=True)
    want = gx.view(-1, Ci) * torch.where(bits.bool(), 1.0, 0.2).float()
    assert torch.equal(gxm.view(-1, Ci), want)
    sums = part[:ep.n_slots * ep.slot_stride].view(ep.n_slots, ep.slot_stride).double().sum(0)
    assert torch.allclose(sums[:Ci], want.double().sum(0), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dense", sorted(DENSE))
def test_dense_form_stays_inside_its_tensors(hl, case, dense):
    """operands and sentinel-filled outputs carved from one poisoned arena: the ragged rows and columns of the last tiles, the
    out-of-range pixels of a weight gradient's last triple and the dummy loads past the K range neither store outside the outputs
    nor feed anything from outside the operands into them (the poison is a NaN in fp32 and in bf16)"""
    o = Operands.of(hl, case)
    g = o.geom(hl, dense)
    held = [o.xs, o.ws, o.wsd, o.gys, o.bd, o.y_like(hl), o.xd, o.wd]               # what is carved below
    arena = guard.Arena(nbytes=sum(t.numel() * t.element_size() for t in held) + (len(held) + 2) * (guard.MARGIN + 256))
    xs, ws, wsd, gys, bd = arena.put(o.xs), arena.put(o.ws), arena.put(o.wsd), arena.put(o.gys), arena.put(o.bd)
    y = arena.full(tuple(o.y_like(hl).shape), 3.0)
    hl.conv_fprop(g, xs, ws, bd, y)
    assert torch.equal(y, o.fprop(hl, dense))
    if o.has_dgrad:
        gx = arena.full(tuple(o.xd.shape), 7.0)
        hl.conv_dgrad(g, gys, wsd, None, gx)
        assert torch.equal(gx, o.dgrad(hl, dense))
    if o.has_wgrad:
        dw = arena.full(tuple(o.wd.shape), 1.0)
        hl.conv_wgrad(g, xs, gys, dw)
        assert torch.equal(dw, o.wgrad(hl, dense))
    arena.check()


@pytest.mark.parametrize("dense", sorted(DENSE))
def test_a_geometry_without_whole_triples_keeps_the_padded_form(hl, dense):
    """Ci = 16 (one group of 16 channels per tap): the dense code is refused with MCG_ERR_UNSUPPORTED, code 0 is the padded form;
    so is the dense code with another precision; a code between the tiles is a bad argument"""
    N, Ti, H, Ci, Co, kt = 2, 1, 32, 16, 32, 1
    import mocogan_chainer_amd.layout as lay
    rng = np.random.RandomState(11)
    x = rng.uniform(-1, 1, (N, Ci, Ti, H, H)).astype(np.float32).astype(np.float64)
    W = (rng.randn(Co, Ci, kt, 4, 4) * 0.1).astype(np.float32).astype(np.float64)
    xd, wd = lay.act_to_dev(dev(x)), lay.conv_w_to_dev(dev(W))
    xs, ws = hl.split_planes(xd), hl.split_planes(wd)
    g = hl.make_geom(N, Ti, H, H, Ci, Co, kt, precision='f32x3')
    y = torch.full((N, g.To, g.Ho, g.Wo, Co), 3.0, device="cuda")
    assert not hl.dense_split_ok("fprop", g)
    g.tile = dense
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        hl.conv_fprop(g, xs, ws, None, y)
    assert bool((y == 3.0).all())
    g.tile = 0
    hl.conv_fprop(g, xs, ws, None, y)
    y7 = torch.empty_like(y)
    g.tile = 7
    hl.conv_fprop(g, xs, ws, None, y7)
    assert torch.equal(y, y7)
    assert rel_l2(lay.act_from_dev(y, Co), F.conv3d_fwd(x, W, None, STRIDE, PAD)) < 2e-6
    g16 = hl.make_geom(2, 1, 16, 16, 64, 128, 1, precision='bf16s')
    g16.tile = dense
    with pytest.raises(hl.McgError, match="MCG_ERR_UNSUPPORTED"):
        hl.conv_fprop(g16, torch.zeros((2, 1, 16, 16, 64), device="cuda", dtype=torch.bfloat16),
                      torch.zeros((128, 1, 4, 4, 64), device="cuda", dtype=torch.bfloat16), None, torch.zeros((2, 1, 8, 8, 128), device="cuda"))
    g.tile = 18
    with pytest.raises(hl.McgError, match="MCG_ERR_BAD_ARG"):
        hl.conv_fprop(g, xs, ws, None, y)


def _shipped_dense():
    import json
    import os
    import mocogan_chainer_amd.hiplib as hiplib
    pkg = os.path.dirname(hiplib.__file__)
    main = {tuple(k): v for k, v in json.load(open(os.path.join(pkg, 'tuned_tiles_mi355x.json')))}
    return [(tuple(k), v, main[tuple(k)]) for k, v in json.load(open(os.path.join(pkg, 'dense_tiles_mi355x.json')))]


@pytest.mark.parametrize("entry", _shipped_dense(), ids=lambda e: "%s-%s-%d" % (e[0][0], "x".join(str(v) for v in e[0][1:8]), e[1]))
def test_shipped_dense_launches_equal_the_padded_form_at_their_production_geometry(hl, entry):
    """every launch the shipped list moves to the dense form, at the batch it was tuned at, against the padded form of ITS tile
    (code - 10 without the split digit): bit for bit where one block writes an output element; with a K split, or a weight
    gradient (pixel splits at these sizes), both results are within 2e-6 of the exact one (the oracle tolerance the small-shape
    tests hold either form to), hence within 4e-6 of each other"""
    key, code, _ = entry
    kind, N, Ti, Hi, Wi, Ci, Co, kt = key[:8]
    g = hl.make_geom(N, Ti, Hi, Wi, Ci, Co, kt, precision='f32x3')
    gen = torch.Generator(device="cuda").manual_seed(N + Ti + Ci)
    x = torch.rand((N, Ti, Hi, Wi, Ci), device="cuda", generator=gen) * 2 - 1
    y = torch.randn((N, g.To, g.Ho, g.Wo, Co), device="cuda", generator=gen)
    w = torch.randn((Co, kt, 4, 4, Ci), device="cuda", generator=gen) * 0.05
    if kind == "fprop":
        a, b = hl.split_planes(x), hl.split_planes(w)
        def run(tile):
            g.tile = tile
            out = torch.full_like(y, 3.0)
            hl.conv_fprop(g, a, b, None, out)
            return out
    elif kind == "dgrad":
        a, b = hl.split_planes(y), hl.split_planes(w, run=16 * kt * 16 * Ci)
        def run(tile):
            g.tile = tile
            out = torch.full_like(x, 7.0)
            hl.conv_dgrad(g, a, b, None, out)
            return out
    else:
        a, b = hl.split_planes(x), hl.split_planes(y)
        def run(tile):
            g.tile = tile
            out = torch.zeros_like(w)
            hl.conv_wgrad(g, a, b, out)
            return out
    dense, padded = run(code), run(code % 1000 - 10)
    if code < 1000 and kind != "wgrad":
        assert torch.equal(dense, padded), guard.describe_diff(dense, padded, names=("dense", "padded"))
    else:
        d = float((dense.double() - padded.double()).norm() / padded.double().norm())
        print(key, code, "rel-L2 dense - padded", d)
        assert d < 4e-6, d
