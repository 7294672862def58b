"""The layout and data-movement entry points of include/mocogan_hip.h stated in plain NumPy, one function per sentence of the
header (TEST INFRASTRUCTURE).  Written from the header's words -- "out[N][T][H][W][Cp] = x[N][C][T][H][W]", "padded channels = 0",
"+1 at channel C + labels[n], -1 at the others -- then zeros" -- not from the kernels: no grid, no stride, no loop of
csrc/small_ops.hip appears here.  tests/test_layout_ref_cpu.py holds every function to what the repository already states elsewhere
(layout.act_to_dev / act_from_dev, model/updater.py's label planes, the reference's byte formula, the float64 fold formula).

Copies, the uint8 normalisation and a single fp32 addition are exact or identically rounded in NumPy, so those functions return
fp32 arrays a kernel has to match bit for bit; the arithmetic ones (tanh backward, the BatchNorm fold, noise) return float64."""
import numpy as np

from oracle import philox

F32 = np.float32


def pack(x, Cp, addend=None):
    """mcg_pack_clip: x (N, C, T, HW) fp32 -> [N][T][HW][Cp] fp32, channels >= C zero; `addend` [N][T][HW][Cp] (zero in its own
    padded channels, as the callers' noise tensors are) is added with one fp32 addition."""
    x = np.asarray(x, F32)
    N, C, T, HW = x.shape
    assert Cp >= C and Cp % 4 == 0
    out = np.zeros((N, T, HW, Cp), F32)
    out[..., :C] = x.transpose(0, 2, 3, 1)
    if addend is not None:
        addend = np.asarray(addend, F32)
        assert addend.shape == out.shape and not addend[..., C:].any()
        out[..., :C] = out[..., :C] + addend[..., :C]
    return out


def pack_u8(x, Cp, addend=None):
    """mcg_pack_clip_u8: x (N, T, HW, C) uint8 -> [N][T][HW][Cp] = (x - 128) / 128 (exact in fp32), then as pack"""
    x = np.asarray(x)
    assert x.dtype == np.uint8
    f = (x.astype(F32) - F32(128)) / F32(128)
    return pack(f.transpose(0, 3, 1, 2), Cp, addend)


def unpack(inp, C):
    """mcg_unpack_clip: in [N][T][HW][Cp] -> x (N, C, T, HW), the first C channels"""
    inp = np.asarray(inp, F32)
    return np.ascontiguousarray(inp[..., :C].transpose(0, 3, 1, 2))


def tanh_bwd_to_frames(g_clip, x_clip):
    """mcg_tanh_bwd_to_frames: g_clip, x_clip [N][T][frame_elems] -> float64 [(t * N + n)][frame_elems] = g * (1 - x^2)"""
    g, x = np.asarray(g_clip, np.float64), np.asarray(x_clip, np.float64)
    N, T, fe = g.shape
    return np.ascontiguousarray((g * (1.0 - x * x)).transpose(1, 0, 2)).reshape(T * N, fe)


def frames_order(a):
    """[N][T][..] -> [(t * N + n)][..]: where tanh_bwd_to_frames puts frame (n, t), values untouched"""
    a = np.asarray(a)
    return np.ascontiguousarray(np.swapaxes(a, 0, 1)).reshape((a.shape[0] * a.shape[1],) + a.shape[2:])


def concat_label_planes(x, C, dl, Cq, labels=None):
    """mcg_concat_label_planes: x [N][P][Cp] -> [N][P][Cq]: the first C channels, then dl planes (+1 at C + labels[n], -1 at the
    others), then zeros.  dl == 0: the channel slice into another row width."""
    x = np.asarray(x, F32)
    N, P, Cp = x.shape
    assert Cp >= C and Cq >= C + dl and Cq % 4 == 0
    out = np.zeros((N, P, Cq), F32)
    out[..., :C] = x[..., :C]
    if dl:
        labels = np.asarray(labels)
        assert labels.shape == (N,) and labels.min() >= 0 and labels.max() < dl
        out[..., C:C + dl] = -1.0
        out[np.arange(N), :, C + labels] = 1.0
    return out


def clip_bytes(x):
    """mcg_clip_to_u8 with act = NONE on fp32 x: the reference's ((x / 2. + 0.5) * 255).astype(np.uint8) -- three separately
    rounded fp32 operations and a truncating cast; "values outside [0, 255] saturate" (NumPy's own cast of those is undefined).
    No NaN."""
    x = np.asarray(x, F32)
    assert not np.isnan(x).any()
    with np.errstate(over='ignore'):
        v = (x / F32(2.) + F32(0.5)) * F32(255)
    assert v.dtype == F32
    return np.clip(v, F32(0), F32(255)).astype(np.uint8)


def fold_deconv(w, bias, C, gamma, beta, avg_mean, avg_var, eps=2e-5):
    """mcg_bn_fold_deconv in float64: w [rows][Cp], bias [Cp] or None (= 0); s_c = gamma_c / sqrt(avg_var_c + eps);
    w_out[r][c] = w[r][c] * s_c, bias_out[c] = (bias[c] - avg_mean_c) * s_c + beta_c for c < C; channels C .. Cp are copied.
    eps is the fp32 value the device receives."""
    w = np.asarray(w, np.float64)
    Cp = w.shape[-1]
    b = np.zeros(Cp) if bias is None else np.asarray(bias, np.float64)
    s = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(avg_var, np.float64) + np.float64(F32(eps)))
    w_out, b_out = w.copy(), b.copy()
    w_out[..., :C] = w[..., :C] * s
    b_out[:C] = (b[:C] - np.asarray(avg_mean, np.float64)) * s + np.asarray(beta, np.float64)
    return w_out, b_out


def pack_noise(npix, C, Cp, sigma, seed, stream_id):
    """The noise mcg_pack_clip / mcg_pack_clip_u8 add when sigma > 0, float64 [npix][Cp]: pixel p's channel quad c4 takes Philox
    counter p * Cp/4 + c4 of (seed, stream_id), the four normals of a counter go to its four channels, padded channels take none."""
    z = philox.randn(npix * Cp, sigma, seed, stream_id).reshape(npix, Cp).copy()
    z[:, C:] = 0.0
    return z
