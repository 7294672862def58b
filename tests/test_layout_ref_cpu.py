"""tests/layout_ref.py held to what the repository states elsewhere: the NumPy statements of the layout entry points are only worth
comparing a kernel with if they agree with layout.act_to_dev / act_from_dev (the API boundary's own transposes), with
model/updater.py's label planes, with the reference's byte formula and with the float64 fold formula of tests/test_gpu_sampler.py.
No GPU, no library call."""
import types

import numpy as np
import pytest
import torch

import layout_ref as LR
from oracle import philox

SHAPES = [(1, 1, 4, 1, 1), (3, 3, 4, 5, 63), (2, 6, 8, 3, 50), (1, 4, 4, 2, 7), (2, 3, 8, 3, 50)]      # N, C, Cp, T, HW


def _lay():
    import mocogan_chainer_amd.layout as lay
    return lay


@pytest.mark.parametrize("shape", SHAPES)
def test_pack_and_unpack_are_the_api_boundary_transposes(shape):
    N, C, Cp, T, HW = shape
    lay = _lay()
    rng = np.random.RandomState(N + C + T + HW)
    x = rng.randn(N, C, T, HW).astype(np.float32)
    x.flat[0] = -0.0
    got = LR.pack(x, Cp)
    assert got.shape == (N, T, HW, Cp) and got.dtype == np.float32
    if Cp == lay.pad4(C):                                               # (act_to_dev pads to the next multiple of 4 only)
        want = lay.act_to_dev(torch.tensor(x).view(N, C, T, HW, 1)).numpy().reshape(N, T, HW, Cp)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not got[..., C:].view(np.uint32).any()                         # +0.0, not -0.0
    assert got[1 % N, T - 1, HW // 2, C - 1] == x[1 % N, C - 1, T - 1, HW // 2]
    # the way back, from a tensor whose padded channels hold anything
    dirty = got.copy()
    dirty[..., C:] = np.nan
    back = LR.unpack(dirty, C)
    want = lay.act_from_dev(torch.tensor(dirty).view(N, T, HW, 1, Cp), C).numpy().reshape(N, C, T, HW)
    assert np.array_equal(back.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(back.view(np.uint32), x.view(np.uint32))        # round trip, bit for bit
    # addend: one fp32 addition per live element, padded channels stay zero
    noise = LR.pack(rng.randn(N, C, T, HW).astype(np.float32), Cp)
    both = LR.pack(x, Cp, noise)
    assert np.array_equal(LR.unpack(both, C), x + LR.unpack(noise, C)) and not both[..., C:].view(np.uint32).any()


def test_pack_u8_is_the_loaders_normalisation():
    rng = np.random.RandomState(4)
    N, C, Cp, T, HW = 2, 3, 4, 3, 10
    u8 = rng.randint(0, 256, (N, T, HW, C)).astype(np.uint8)
    u8[0, 0, 0], u8[0, 0, 1] = 0, 255
    ref = ((u8.astype(np.float64) - 128.) / 128.).transpose(0, 3, 1, 2)        # datasets.py:95 and updater.py:87-92, in double
    got = LR.pack_u8(u8, Cp)
    assert np.array_equal(LR.unpack(got, C).astype(np.float64), ref)             # exact: k / 128 is an fp32 number
    assert np.array_equal(got, LR.pack(ref.astype(np.float32), Cp))
    assert got.min() == -1.0 and got.max() == 127. / 128.


def test_tanh_backward_goes_to_frame_order():
    rng = np.random.RandomState(5)
    N, T, fe = 3, 5, 8
    g, x = rng.randn(N, T, fe).astype(np.float32), np.tanh(3 * rng.randn(N, T, fe)).astype(np.float32)
    out = LR.tanh_bwd_to_frames(g, x)
    assert out.shape == (T * N, fe) and out.dtype == np.float64
    for n in range(N):
        for t in range(T):
            for e in range(fe):
                assert out[t * N + n, e] == float(g[n, t, e]) * (1.0 - float(x[n, t, e]) ** 2)
    assert np.array_equal(LR.frames_order(g)[2 * N + 1], g[1, 2])
    # autograd's statement of the same gradient: d tanh(a) = 1 - tanh(a)^2 at x = tanh(a)
    a = torch.tensor(rng.randn(N, T, fe), dtype=torch.float64, requires_grad=True)
    xt = torch.tanh(a)
    xt.backward(torch.tensor(g, dtype=torch.float64))
    want = a.grad.numpy().transpose(1, 0, 2).reshape(T * N, fe)
    assert np.allclose(LR.tanh_bwd_to_frames(g, xt.detach().numpy()), want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", [(3, 16, 3, 4, 6, 12), (2, 1, 3, 4, 6, 12), (4, 10, 1, 4, 6, 8), (3, 10, 3, 4, 1, 4),
                                  (2, 10, 3, 4, 2, 8), (3, 10, 3, 4, 6, 16)])
def test_label_planes_are_the_updaters(case):
    """model/updater.py's concat_label_video on the (N,C,T,H,W) clip, taken to the device layout, as
    tests/test_gpu_ops.py::test_concat_label_planes restates it: the clip's channels, -1 planes with +1 on the item's label, zeros"""
    from model.updater import Updater
    N, P, C, Cp, dl, Cq = case
    rng = np.random.RandomState(P + dl)
    labels = np.array(([0, dl - 1] + [dl // 2] * N)[:N])
    x = np.full((N, P, Cp), np.nan, np.float32)
    x[..., :C] = rng.randn(N, P, C)
    got = LR.concat_label_planes(x, C, dl, Cq, labels)
    video = torch.tensor(x[..., :C].transpose(0, 2, 1).reshape(N, C, 1, P, 1))
    cat = Updater.concat_label_video(types.SimpleNamespace(dim_zl=dl), video, labels)      # (N, C + dl, 1, P, 1)
    want = np.zeros((N, P, Cq), np.float32)
    want[..., :C + dl] = cat.numpy().reshape(N, C + dl, P).transpose(0, 2, 1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    restated = np.zeros((N, P, Cq), np.float32)
    restated[..., :C] = x[..., :C]
    restated[..., C:C + dl] = -1.0
    for i, lab in enumerate(labels):
        restated[i, :, C + lab] = 1.0
    assert np.array_equal(got, restated)
    # the way back: a channel slice, label planes dropped
    back = LR.concat_label_planes(got, C, 0, 4)
    assert np.array_equal(back[..., :C], x[..., :C]) and not back[..., C:].view(np.uint32).any()


def test_clip_bytes_are_the_references():
    rng = np.random.RandomState(6)
    x = rng.uniform(-1, 1, 4096).astype(np.float32)
    k = (np.arange(256) / 127.5 - 1).astype(np.float32)
    x = np.concatenate([x, k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-2)), np.float32([1, -1, 0, -0.0])])
    x = np.clip(x, -1, 1)
    assert np.array_equal(LR.clip_bytes(x), ((x / 2. + 0.5) * 255).astype(np.uint8))        # generate_samples.py:39 on in-range x
    in_double = np.floor((x.astype(np.float64) / 2 + 0.5) * 255)
    assert np.abs(LR.clip_bytes(x).astype(np.float64) - in_double).max() <= 1                # (fp32 rounding moves a boundary value by one)
    sat = np.float32([1.0000001, -1.0000001, 3, -3, np.inf, -np.inf])
    assert LR.clip_bytes(sat).tolist() == [255, 0, 255, 0, 255, 0]
    with pytest.raises(AssertionError):
        LR.clip_bytes(np.float32([np.nan]))


def test_fold_is_the_float64_formula():
    rng = np.random.RandomState(7)
    rows, C, Cp = 5, 6, 8
    w, b = rng.randn(rows, Cp), rng.randn(Cp)
    gamma, beta = rng.uniform(0.5, 1.5, C), rng.normal(0, 0.2, C)
    mean, var = rng.normal(0, 0.05, C), rng.uniform(0.02, 0.2, C)
    s = gamma / np.sqrt(var + np.float64(np.float32(2e-5)))
    w_out, b_out = LR.fold_deconv(w, b, C, gamma, beta, mean, var)
    assert np.allclose(w_out[:, :C], w[:, :C] * s, rtol=1e-15) and np.array_equal(w_out[:, C:], w[:, C:])
    assert np.allclose(b_out[:C], b[:C] * s + beta - mean * s, rtol=1e-13) and np.array_equal(b_out[C:], b[C:])
    _, b0 = LR.fold_deconv(w, None, C, gamma, beta, mean, var)
    assert np.allclose(b0[:C], beta - mean * s, rtol=1e-13) and not b0[C:].any()
    # the property the fold exists for: bn(v + b) == v' + b' with v' the folded product, per channel
    v = rng.randn(C)
    bn = gamma * ((v * w[0, :C] + b[:C]) - mean) / np.sqrt(var + np.float64(np.float32(2e-5))) + beta
    assert np.allclose(v * w_out[0, :C] + b_out[:C], bn, rtol=1e-12)


@pytest.mark.parametrize("M,C", [(8, 4), (12, 3), (4, 64)])
def test_rowquad_order_is_the_headers_sentence(M, C):
    """include/mocogan_hip.h, mcg_randn_rowquad: "element (m, c) is normal m & 3 of Philox counter (m >> 2) * C + c" -- with
    oracle.philox.randn's "one counter per group of 4 consecutive elements": normal j of counter k is element 4 k + j of the stream"""
    z = philox.randn(M * C, 0.2, 99, 7)
    got = philox.randn_rowquad(M, C, 0.2, 99, 7)
    assert got.shape == (M, C)
    for m in range(M):
        for c in range(C):
            assert got[m, c] == z[4 * ((m >> 2) * C + c) + (m & 3)]


@pytest.mark.parametrize("C,Cp", [(3, 4), (6, 8), (4, 4)])
def test_pack_noise_placement(C, Cp):
    """mcg_pack_clip's draw: counter p * Cp/4 + c4, four normals per counter, padded channels masked"""
    npix = 11
    z = philox.randn(npix * Cp, 0.2, 5, 3)
    got = LR.pack_noise(npix, C, Cp, 0.2, 5, 3)
    for p in range(npix):
        for c in range(Cp):
            want = z[4 * (p * (Cp // 4) + c // 4) + (c & 3)] if c < C else 0.0
            assert got[p, c] == want
    assert np.abs(got[:, :C]).min() > 0
