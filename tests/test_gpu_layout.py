"""The layout and data-movement kernels of csrc/small_ops.hip -- pack_clip, pack_clip_u8, unpack_clip, tanh_bwd_to_frames,
concat_label_planes, clip_to_u8, bn_fold_deconv, randn, randn_rowquad, split_planes -- against the NumPy statements of
tests/layout_ref.py (which tests/test_layout_ref_cpu.py holds to layout.py, model/updater.py and the reference's formulas).

Every one of these kernels is a grid-stride loop of at most EW = 2048 * 256 threads.  The shapes are the smallest that reach: one
item; odd extents; a channel pad of one, of two and of none; N != T (a frame index transposed the wrong way lands elsewhere); a
label plane inside the input's own quad, across a quad boundary, in front of a quad of zeros; and EW + a few hundred items, where a
thread takes a SECOND trip of its loop (at the workload's own size, 32 clips x 16 frames x 64 x 64, it takes four).

Copies, (x - 128) / 128 and a single fp32 addition are exact or identically rounded in NumPy: those results must match bit for
bit.  The toleranced ones: noise against oracle.philox at the bounds tests/test_gpu_ops.py::test_philox_noise_matches_oracle_stream
uses (4e-6 for the draw, 5e-6 for value + draw); tanh backward at |got - ref64| <= 3 * 2^-24 |g| (two roundings in 1 - x^2 with
|x| <= 1 cost at most 2^-24 (1 + 2^-24) absolute, fused or not; the product one more); the BatchNorm fold at FWD_TOL of
tests/test_gpu_sampler.py.  Run with -s: the PARITY lines are what profiles/layout_partials_parity.md records.

All operands and outputs are carved from one guard.Arena: outputs are poison (NaN) until written, the margins are checked after
every launch, inputs are compared bit for bit with a snapshot afterwards."""
import functools

import numpy as np
import pytest
import torch

import layout_ref as LR
from guard import Arena
from oracle import philox

pytestmark = pytest.mark.gpu

EW = 2048 * 256                         # threads of the largest element-wise grid (small_ops.hip: EW_GRID * NT)
FWD_TOL = 1e-5                          # tests/test_gpu_sampler.py::test_fold_kernel_matches_the_float64_formula
DRAW_TOL, SUM_DRAW_TOL = 4e-6, 5e-6     # tests/test_gpu_ops.py::test_philox_noise_matches_oracle_stream (sigma = 0.2)
SIGMA, SEED, STREAM = 0.2, 0x1234567887654321, 42
U = 2.0 ** -24
F32, BF, U8, I32 = torch.float32, torch.bfloat16, torch.uint8, torch.int32
POISON_BYTES = np.array([0xc0, 0x7f, 0xc0, 0x7f], np.uint8)


@pytest.fixture(scope="module")
def hl():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


@pytest.fixture(scope="module")
def arena():
    return Arena(128 << 20)


def raw(t):
    """the bytes of a tensor as a NumPy array of its own element type (fp32 as uint32: NaN poison compares equal to itself)"""
    t = t.detach().contiguous()
    if t.dtype == F32:
        return t.view(I32).cpu().numpy().view(np.uint32)
    if t.dtype == BF:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def f32bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same(case, what, got, want):
    """the device tensor `got` equals the fp32 / uint8 array `want` bit for bit"""
    g = raw(got)
    w = f32bits(want) if got.dtype == F32 else np.asarray(want)
    assert g.shape == w.shape, (case, what, g.shape, w.shape)
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    first = tuple(int(v) for v in bad[0])
    shown = (got.detach().cpu().numpy()[first], np.asarray(want)[first])
    raise AssertionError("%s %s: %d of %d elements differ, first at %s: got %r, want %r" % (case, what, len(bad), g.size, first, *shown))


def held(case, what, err, tol):
    print("PARITY %-34s %-30s %.2e  (bound %.0e)" % (case, what, err, tol))
    assert err < tol, (case, what, err, tol)


class Launch:
    """The tensors of one case: inputs are copies inside the arena with a snapshot outside it, outputs are poison."""

    def __init__(self, arena):
        arena.reset()
        self.arena, self.inputs = arena, []

    def put(self, a, dtype=F32):
        t = self.arena.put(torch.from_numpy(np.array(a, copy=True)).to(dtype).cuda())
        self.inputs.append((t, t.clone()))
        return t

    def put_padded(self, a, Cp):
        """[..][C] values into a poisoned [..][Cp] tensor: channels >= C hold NaN, nothing of which may reach an output"""
        a = np.asarray(a, np.float32)
        t = self.arena.empty(a.shape[:-1] + (Cp,))
        t[..., :a.shape[-1]] = torch.as_tensor(a).cuda()
        self.inputs.append((t, t.clone()))
        return t

    def keep(self, t):
        """an output of an earlier launch of the case that a later one reads"""
        self.inputs.append((t, t.clone()))
        return t

    def out(self, shape, dtype=F32):
        return self.arena.empty(shape, dtype)

    def done(self):
        self.arena.check()
        for t, snap in self.inputs:
            assert np.array_equal(raw(t), raw(snap)), "a launch wrote to one of its inputs"


# ---- pack_clip / pack_clip_u8 ------------------------------------------------------------------------------------------------
PACK_CASES = [(1, 1, 4, 1, 1),           # one pixel
              (3, 3, 4, 5, 63),          # odd HW, N != T
              (2, 6, 8, 3, 50),          # two quads, the second with two live channels
              (1, 4, 4, 2, 7),           # C == Cp
              (2, 3, 4, 2, 131147)]      # npix = EW + 300: the second trip
NOISE_CASES = [PACK_CASES[1], PACK_CASES[2], PACK_CASES[4]]
assert 2 * 2 * 131147 == EW + 300
FRAME_CASES = [(3, 3, 4, 5, 63, 2), (3, 3, 4, 5, 63, 4), (2, 3, 4, 3, 262200, 1), (2, 3, 4, 3, 262200, 2)]       # .., T of the clip, HW, frame
assert 2 * 262200 > EW


@functools.lru_cache(maxsize=None)
def _clips(case):
    """(float clip (N,C,T,HW), uint8 clip (N,T,HW,C), its normalised float form, an addend with zero padded channels)"""
    N, C, Cp, T, HW = case
    rng = np.random.RandomState(N * 1000 + C * 100 + T * 10 + HW % 7)
    x = rng.randn(N, C, T, HW).astype(np.float32)
    x.flat[0] = -0.0
    u8 = rng.randint(0, 256, (N, T, HW, C)).astype(np.uint8)
    u8.reshape(-1)[:2] = np.uint8([0, 255])[:u8.size]
    xu = np.ascontiguousarray(((u8.astype(np.float32) - 128.) / 128.).transpose(0, 3, 1, 2))
    add = np.zeros((N, T, HW, Cp), np.float32)
    add[..., :C] = rng.randn(N, T, HW, C)
    for a in (x, u8, xu, add):
        a.setflags(write=False)
    return x, u8, xu, add


def _zero_pad(case, what, out, C):
    assert not raw(out[..., C:]).any(), "%s %s: a padded channel is not +0.0" % (case, what)


@pytest.mark.parametrize("case", PACK_CASES, ids=str)
def test_pack_clip_without_noise_and_with_addend(hl, arena, case):
    N, C, Cp, T, HW = case
    x, u8, xu, add = _clips(case)
    for tag, addend in (("plain", None), ("addend", add)):
        L = Launch(arena)
        xd, ud = L.put(x), L.put(u8, U8)
        ad = None if addend is None else L.put(addend)
        o, o8 = L.out((N, T, HW, Cp)), L.out((N, T, HW, Cp))
        hl.pack_clip(N, C, Cp, T, HW, xd, o, addend=ad)
        L.done()
        hl.pack_clip_u8(N, C, Cp, T, HW, ud, o8, addend=ad)
        L.done()
        same(case, "pack_clip " + tag, o, LR.pack(x, Cp, addend))
        same(case, "pack_clip_u8 " + tag, o8, LR.pack_u8(u8, Cp, addend))
        _zero_pad(case, tag, o, C)
        _zero_pad(case, tag + " u8", o8, C)
    print("PARITY %-34s pack_clip / pack_clip_u8 == NumPy: bit for bit" % (case,))


@pytest.mark.parametrize("case", NOISE_CASES, ids=str)
def test_pack_clip_noise_is_the_oracle_stream(hl, arena, case):
    N, C, Cp, T, HW = case
    _, u8, xu, _ = _clips(case)
    L = Launch(arena)
    xd, ud = L.put(xu), L.put(u8, U8)
    o, o8 = L.out((N, T, HW, Cp)), L.out((N, T, HW, Cp))
    hl.pack_clip(N, C, Cp, T, HW, xd, o, sigma=SIGMA, seed=SEED, stream_id=STREAM)
    L.done()
    hl.pack_clip_u8(N, C, Cp, T, HW, ud, o8, sigma=SIGMA, seed=SEED, stream_id=STREAM)
    L.done()
    npix = N * T * HW
    want = LR.pack(xu, Cp).astype(np.float64) + LR.pack_noise(npix, C, Cp, SIGMA, SEED, STREAM).reshape(N, T, HW, Cp)
    got = o.cpu().numpy()
    assert np.isfinite(got).all()
    held(case, "pack_clip value + noise", np.abs(got - want).max(), SUM_DRAW_TOL)
    assert np.abs(got[..., :C] - LR.pack(xu, Cp)[..., :C]).max() > 0.1          # (noise was drawn at all)
    _zero_pad(case, "noise", o, C)
    assert np.array_equal(raw(o8), raw(o)), "pack_clip_u8 and pack_clip differ with in-kernel noise"


@pytest.mark.parametrize("case", FRAME_CASES, ids=str)
def test_pack_clip_frame_view(hl, arena, case):
    """frame t of every clip: T = 1 with the clip's strides, against the reference's slice of the clip -- plain, with an addend
    and with noise (whose counters are those of the FRAME's pixels)"""
    N, C, Cp, T, HW, t = case
    x, u8, xu, add = _clips((N, C, Cp, T, HW))
    add1 = np.ascontiguousarray(add[:, t:t + 1])
    for tag in ("plain", "addend", "noise"):
        L = Launch(arena)
        xd, ud = L.put(xu if tag == "noise" else x), L.put(u8, U8)
        ad = L.put(add1) if tag == "addend" else None
        kw = dict(sigma=SIGMA, seed=SEED, stream_id=STREAM) if tag == "noise" else {}
        o, o8 = L.out((N, 1, HW, Cp)), L.out((N, 1, HW, Cp))
        hl.pack_clip(N, C, Cp, 1, HW, xd[:, :, t], o, addend=ad, stride_n=C * T * HW, stride_c=T * HW, **kw)
        L.done()
        hl.pack_clip_u8(N, C, Cp, 1, HW, ud[:, t], o8, addend=ad, stride_n=T * HW * C, **kw)
        L.done()
        if tag == "noise":
            want = LR.pack(xu[:, :, t:t + 1], Cp).astype(np.float64) + LR.pack_noise(N * HW, C, Cp, SIGMA, SEED, STREAM).reshape(N, 1, HW, Cp)
            held(case, "frame view value + noise", np.abs(o.cpu().numpy() - want).max(), SUM_DRAW_TOL)
            assert np.array_equal(raw(o8), raw(o))
        else:
            same(case, "pack_clip frame " + tag, o, LR.pack(x[:, :, t:t + 1], Cp, None if ad is None else add1))
            same(case, "pack_clip_u8 frame " + tag, o8, LR.pack_u8(u8[:, t:t + 1], Cp, None if ad is None else add1))
        _zero_pad(case, tag, o, C)
        _zero_pad(case, tag + " u8", o8, C)


# ---- unpack_clip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PACK_CASES + [(2, 3, 8, 3, 50)], ids=str)
def test_unpack_clip(hl, arena, case):
    N, C, Cp, T, HW = case
    rng = np.random.RandomState(HW + Cp)
    v = rng.randn(N, T, HW, C).astype(np.float32)
    v.flat[0] = -0.0
    L = Launch(arena)
    ind = L.put_padded(v, Cp)
    x = L.out((N, C, T, HW))
    hl.unpack_clip(N, C, Cp, T, HW, ind, x)
    L.done()
    same(case, "unpack_clip", x, LR.unpack(ind.cpu().numpy(), C))
    assert np.array_equal(LR.unpack(ind.cpu().numpy(), C), v.transpose(0, 3, 1, 2))


# ---- tanh_bwd_to_frames --------------------------------------------------------------------------------------------------------
TANH_CASES = [(1, 1, 4), (3, 5, 4), (5, 3, 256), (2, 16, 4 * 8 * 8), (3, 5, 4 * 34973)]
assert 3 * 5 * 34973 == EW + 307


@pytest.mark.parametrize("case", TANH_CASES, ids=str)
def test_tanh_bwd_to_frames(hl, arena, case):
    N, T, fe = case
    rng = np.random.RandomState(N * 100 + T)
    g = rng.randn(N, T, fe).astype(np.float32)
    x = np.tanh(3 * rng.randn(N, T, fe)).astype(np.float32)
    assert np.abs(x).max() <= 1.0
    x[..., 0], x[..., 1], x[..., 2] = 0.0, 1.0, -1.0                      # in every frame
    L = Launch(arena)
    gd, xd = L.put(g), L.put(x)
    out = L.out((T * N, fe))
    hl.tanh_bwd_to_frames(N, T, fe, gd, xd, out)
    L.done()
    got = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    ref = LR.tanh_bwd_to_frames(g, x)
    gf = np.abs(LR.frames_order(g).astype(np.float64))
    excess = np.abs(got - ref) - 3 * U * gf
    worst = (np.abs(got - ref) / (U * np.maximum(gf, 1e-300))).max()
    print("PARITY %-34s %-30s %.3f x 2^-24 |g|  (bound 3)" % (case, "tanh_bwd_to_frames", worst))
    assert excess.max() <= 0, (case, int((excess > 0).sum()), worst)
    assert not got[:, 1].any() and not got[:, 2].any(), "x = +-1 must give exactly 0"
    assert np.array_equal(got[:, 0], LR.frames_order(g)[:, 0].astype(np.float64)), "x = 0 must give exactly g"


# ---- concat_label_planes -------------------------------------------------------------------------------------------------------
CONCAT_CASES = [(3, 128, 3, 4, 6, 12),
                (2, 1, 3, 4, 6, 12),         # P = 1
                (4, 50, 1, 4, 6, 8),         # one-channel clips
                (3, 50, 3, 4, 1, 4),         # the label plane inside the input's own quad
                (2, 50, 3, 4, 2, 8),         # planes straddling the quad boundary
                (3, 50, 3, 4, 6, 16),        # a whole quad of zero padding
                (2, 87432, 3, 4, 6, 12)]     # npix * Cq / 4 = EW + 304
assert 2 * 87432 * 3 == EW + 304


@pytest.mark.parametrize("case", CONCAT_CASES, ids=str)
def test_concat_label_planes_and_the_way_back(hl, arena, case):
    N, P, C, Cp, dl, Cq = case
    rng = np.random.RandomState(P % 1000 + dl + Cq)
    labels = np.array(([0, dl - 1] + [dl // 2] * N)[:N])
    assert 0 in labels and dl - 1 in labels
    v = rng.randn(N, P, C).astype(np.float32)
    L = Launch(arena)
    xd = L.put_padded(v, Cp)
    lab = L.put(labels, I32)
    out = L.out((N, P, Cq))
    hl.concat_label_planes(xd, C, dl, lab, out)
    L.done()
    want = LR.concat_label_planes(xd.cpu().numpy(), C, dl, Cq, labels)
    same(case, "concat_label_planes", out, want)
    # the way back (dl = 0) from this row width: into 4 channels always, into 8 once, and at the large size into 16 as well --
    # 2 * 87432 * 4 quads, a second trip of the slice itself
    L.keep(out)
    widths = [4] + ([8] if case == CONCAT_CASES[0] else []) + ([16] if P > 1000 else [])
    for Cb in widths:
        back = L.out((N, P, Cb))
        hl.concat_label_planes(out, C, 0, None, back)
        L.done()
        same(case, "way back into %d" % Cb, back, LR.concat_label_planes(want, C, 0, Cb))
        assert np.array_equal(back[..., :C].cpu().numpy(), v) and not raw(back[..., C:]).any()
    print("PARITY %-34s concat_label_planes, way back into %s: bit for bit" % (case, widths))


# ---- clip_to_u8 ----------------------------------------------------------------------------------------------------------------
def _byte_edge_values():
    """for every byte value k the fp32 nearest k / 127.5 - 1 and its two neighbours; then values that saturate"""
    k = (np.arange(256, dtype=np.float64) / 127.5 - 1).astype(np.float32)
    sat = np.float32([1.0000001, -1.0000001, 3, -3, np.inf, -np.inf])
    return np.concatenate([k, np.nextafter(k, np.float32(4)), np.nextafter(k, np.float32(-4)), sat])


def _clip_input(N, T, HW, C, seed):
    rng = np.random.RandomState(seed)
    live = rng.uniform(-1, 1, (N, T, HW, C)).astype(np.float32)
    ev = _byte_edge_values()
    assert live.size >= ev.size
    live.reshape(-1)[:ev.size] = ev
    return live


# name: N, T, HW, C, what makes the packed (12 bytes per 4 pixels) kernel unusable, if anything
CLIP_CASES = {
    "packed-second-trip": (2, 3, 349528, 3, None),
    "bytewise-second-trip": (2, 3, 87383, 3, None),
    "declined-out-unaligned": (3, 5, 64, 3, "out+1"),
    "declined-stride-t": (3, 2, 64, 3, "stride_t"),
    "declined-one-channel": (3, 5, 64, 1, None),
}
assert 2 * 3 * 349528 // 4 > EW and 349528 % 4 == 0 and 2 * 3 * 87383 > EW


@pytest.mark.parametrize("name", list(CLIP_CASES))
def test_clip_to_u8(hl, arena, name):
    N, T, HW, C, twist = CLIP_CASES[name]
    live = _clip_input(N, T, HW, C, len(name))
    L = Launch(arena)
    ind = L.put_padded(live, 4)
    frame = HW * C
    stride_t = frame + 2 if twist == "stride_t" else frame             # 194: no multiple of 4, while stride_n = 2 * 194 is one
    stride_n = T * stride_t
    assert twist != "stride_t" or (stride_t % 4 != 0 and stride_n % 4 == 0)
    buf = L.out((N * stride_n + 4,), U8)
    out = buf[1:] if twist == "out+1" else buf
    assert (out.data_ptr() % 4 == 1) == (twist == "out+1")
    before = buf.cpu().numpy().copy()
    hl.clip_to_u8(N, C, 4, T, HW, ind, out, stride_n=stride_n, stride_t=stride_t)
    L.done()
    got = out.cpu().numpy()[:N * stride_n].reshape(N, T, stride_t)
    want = LR.clip_bytes(live).reshape(N, T, frame)
    same(name, "bytes", torch.as_tensor(np.ascontiguousarray(got[..., :frame])), want)
    # everything outside the frames is as it was (the arena's poison)
    mask = np.ones(buf.numel(), bool)
    off = 1 if twist == "out+1" else 0
    for n in range(N):
        for t in range(T):
            b = off + n * stride_n + t * stride_t
            mask[b:b + frame] = False
    assert np.array_equal(buf.cpu().numpy()[mask], before[mask]), "%s: a byte outside the frames was written" % name
    print("PARITY %-34s clip_to_u8 == NumPy: bit for bit" % name)


# ---- bn_fold_deconv ------------------------------------------------------------------------------------------------------------
FOLD_CASES = [(5, 6, 8), (262145, 8, 8), (524290, 3, 4)]       # rows, C, Cp: 12, EW + 4 and EW + 3 items (the bias quads come last)
assert 262145 * 2 + 2 == EW + 4 and 524290 + 1 == EW + 3


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize("case", FOLD_CASES, ids=str)
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_bn_fold_deconv(hl, arena, case, with_bias):
    rows, C, Cp = case
    rng = np.random.RandomState(rows % 1000 + C)
    w = (rng.randn(rows, Cp) * 0.05).astype(np.float32)
    b = (rng.randn(Cp) * 0.1).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.normal(0, 0.2, C).astype(np.float32)
    mean, var = rng.normal(0, 0.05, C).astype(np.float32), rng.uniform(0.02, 0.2, C).astype(np.float32)
    L = Launch(arena)
    wd, bd = L.put(w), (L.put(b) if with_bias else None)
    gd, btd, md, vd = L.put(gamma), L.put(beta), L.put(mean), L.put(var)
    w_out, b_out = L.out((rows, Cp)), L.out((Cp,))
    hl.bn_fold_deconv(wd, bd, C, gd, btd, md, vd, w_out, b_out)
    L.done()
    w_ref, b_ref = LR.fold_deconv(w, b if with_bias else None, C, gamma, beta, mean, var)
    gw, gb = w_out.cpu().numpy(), b_out.cpu().numpy()
    assert np.isfinite(gw).all() and np.isfinite(gb).all()
    tag = "%s %s" % (case, "bias" if with_bias else "no bias")
    held(tag, "folded filter", rel_l2(gw[:, :C], w_ref[:, :C]), FWD_TOL)
    held(tag, "folded bias", rel_l2(gb[:C], b_ref[:C]), FWD_TOL)
    if Cp > C:                                                          # padded channels are copied
        same(tag, "padded filter channels", w_out[:, C:], w[:, C:])
        same(tag, "padded bias channels", b_out[C:], b[C:] if with_bias else np.zeros(Cp - C, np.float32))


# ---- randn, randn_rowquad, split_planes at a second trip -----------------------------------------------------------------------
def test_randn_second_trip(hl, arena):
    n = 4 * EW + 5
    L = Launch(arena)
    out = L.out((n,))
    hl.randn(out, SIGMA, SEED, STREAM)
    L.done()
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    held("n = 4 EW + 5", "randn", np.abs(got - philox.randn(n, SIGMA, SEED, STREAM)).max(), DRAW_TOL)


@pytest.mark.parametrize("M,C", [(4 * (EW // 4 + 3), 4), (4 * (EW // 64 + 1), 64)])
def test_randn_rowquad_second_trip(hl, arena, M, C):
    assert M // 4 * C > EW
    L = Launch(arena)
    out = L.out((M, C))
    hl.randn_rowquad(out, C, SIGMA, SEED, STREAM + 1)
    L.done()
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    held("M = %d, C = %d" % (M, C), "randn_rowquad", np.abs(got - philox.randn_rowquad(M, C, SIGMA, SEED, STREAM + 1)).max(), DRAW_TOL)


def test_split_planes_second_trip(hl, arena):
    """n / 8 = EW + 4 eight-value groups with run = 16, against the bit-exact statement of
    tests/test_gpu_ops.py::test_split_planes_are_an_exact_expansion; the padding plane is left as it was (the arena's poison)"""
    n8 = EW + 4
    n = 8 * n8
    torch.manual_seed(11)
    v = (torch.randn(n // 48, 48) * torch.logspace(-6, 6, 48)).view(-1)
    assert v.numel() == n
    L = Launch(arena)
    src = L.put(v.numpy())
    dst = L.out((n // 16, 4, 16), BF)
    hl.split_planes(src, run=16, out=dst)
    L.done()
    s = src.view(n // 16, 16)
    hi, mid, lo, pad = (dst[:, i] for i in range(4))
    assert torch.equal(hi, s.to(BF))
    r1 = s - hi.float()
    assert torch.equal(mid, r1.to(BF))
    r2 = r1 - mid.float()
    assert torch.equal(lo, r2.to(BF))
    big = s.abs() > 1e-30
    assert torch.equal((hi.double() + mid.double() + lo.double())[big], s.double()[big])
    assert bool((pad.contiguous().view(torch.int16) == 0x7fc0).all()), "the padding plane was written"
    print("PARITY %-34s split_planes (run 16): bit for bit, padding plane untouched" % ("n / 8 = EW + 4",))
