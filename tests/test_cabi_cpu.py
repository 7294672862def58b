"""CPU-only checks of the C-ABI boundary and the host logic around it: the shared library builds and
loads here (hipcc cross-compiles without a GPU), exports every symbol include/mocogan_hip.h declares,
validates its arguments before touching the device, and the layout / parameter plumbing round-trips.
No compute entry point is called with real work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def declared_symbols():
    src = open(os.path.join(ROOT, 'include', 'mocogan_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(mcg_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol(hl):
    names = declared_symbols()
    assert len(names) >= 20
    lib = hl.load()
    for n in names:
        assert hasattr(lib, n), "libmocogan_hip.so does not export %s" % n
        assert n in hl.SIGNATURES, "hiplib.SIGNATURES has no ctypes prototype for %s" % n
    assert set(hl.SIGNATURES) == set(names)
    assert lib.mcg_version() == hl.ABI_VERSION
    assert 'define MCG_ABI_VERSION %d' % hl.ABI_VERSION in open(os.path.join(ROOT, 'include', 'mocogan_hip.h')).read()


def test_library_exports_nothing_the_header_does_not_declare(hl):
    """the dynamic symbol table holds exactly the declared mcg_* entry points: helpers shared between the library's translation
    units have hidden visibility (round 5's review)."""
    import subprocess
    import mocogan_chainer_amd as build
    tool = '/opt/rocm/lib/llvm/bin/llvm-readelf'
    if not os.path.exists(tool):
        pytest.skip('llvm-readelf not found')
    out = subprocess.run([tool, '--dyn-syms', '-W', build.lib_path()], capture_output=True, text=True, check=True).stdout
    out = '\n'.join(l for l in out.splitlines() if ' UND ' not in l)                 # defined symbols only
    exported = sorted(set(re.findall(r'\b(mcg_[A-Za-z0-9_]+)\b', out)))
    assert exported == declared_symbols(), sorted(set(exported) ^ set(declared_symbols()))


def test_header_cites_reference_call_sites():
    src = open(os.path.join(ROOT, 'include', 'mocogan_hip.h')).read()
    for cite in ('model/net.py', 'model/updater.py', 'train.py:93-101'):
        assert cite in src


def test_argument_validation_happens_on_the_host(hl):
    lib = hl.load()
    g = hl.make_geom(1, 4, 12, 12, 4, 64, 4)                 # Ho = 6: not a power of two
    assert lib.mcg_conv_fprop(ctypes.byref(g), None, None, None, None, None) == -1
    g = hl.make_geom(1, 4, 16, 16, 3, 64, 4)                 # unpadded channels
    assert lib.mcg_conv_dgrad(ctypes.byref(g), None, None, None, None, 0, 0, None) == -1
    g = hl.make_geom(1, 2, 16, 16, 4, 64, 4)                 # To = Ti - kt + 1 <= 0
    assert lib.mcg_conv_wgrad(ctypes.byref(g), None, None, None, None) == -2
    g = hl.make_geom(1, 4, 16, 16, 4, 64, 4)                 # good geometry, null pointers
    assert lib.mcg_conv_fprop(ctypes.byref(g), None, None, None, None, None) == -1
    assert lib.mcg_fc_fprop(4, 30, 1, None, None, None, None, None) == -1
    assert lib.mcg_gru_seq_fwd(4, 16, 64, 0, 50, None, None, None, None, None, None, None, None) == -1
    assert lib.mcg_adam_wd(0, None, None, None, None, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, None, None) == -1
    assert int(lib.mcg_bn_workspace_bytes(0, 512)) == (512 * 2 * 512 + 3 * 512) * 4


def test_generator_head_entry_points_refuse_on_the_host(hl):
    """The GRU, the full-window layers and the losses pick their kernels from sizes the user sets (--dim_zm, the label count): what
    no kernel covers is refused before anything is launched.  `one` is a non-null pointer that is never dereferenced; no call
    below passes an acceptable argument set."""
    lib = hl.load()
    one = ctypes.c_void_p(16)
    BAD, UNSUPPORTED = -1, -2

    def gru(N, T, dz, dl, dc, labels=one, hole=None):
        ptr = lambda name: None if name == hole else one
        fwd = lib.mcg_gru_seq_fwd(N, T, dz, dl, dc, ptr('params'), ptr('h0'), ptr('e'), labels, ptr('zc'), ptr('z'), ptr('saved'), None)
        bwd = lib.mcg_gru_seq_bwd(N, T, dz, dl, dc, ptr('params'), ptr('e'), labels, ptr('saved'), ptr('gz'), ptr('dparams'), None)
        return fwd, bwd

    for dz, dl, dc in ((0, 0, 50), (65, 0, 50), (64, 65, 50), (10, 119, 50), (1, 128, 50), (10, -1, 50), (10, 6, -1), (-3, 6, 50)):
        assert gru(4, 16, dz, dl, dc) == (UNSUPPORTED, UNSUPPORTED), (dz, dl, dc)
    assert gru(4, 16, 10, 6, 50, labels=None) == (BAD, BAD)                 # a one-hot without labels
    assert gru(4, 16, 12, 6, 50, labels=None) == (BAD, BAD)
    assert gru(4, 16, 64, 64, 50, labels=None) == (BAD, BAD)
    for N, T in ((0, 16), (4, 0), (-1, 16), (4, -1)):
        assert gru(N, T, 10, 0, 50) == (BAD, BAD), (N, T)
    for hole in ('params', 'e', 'saved'):                                   # pointers BOTH entry points take (any other would leave one call acceptable)
        assert gru(4, 16, 10, 0, 50, hole=hole) == (BAD, BAD), hole

    fc = (lambda M, K, Co: lib.mcg_fc_fprop(M, K, Co, one, one, one, one, None),
          lambda M, K, Co: lib.mcg_fc_dgrad(M, K, Co, one, one, one, 4, one, None),
          lambda M, K, Co: lib.mcg_fc_dgrad(M, K, Co, one, one, None, 0, one, None),
          lambda M, K, Co: lib.mcg_fc_wgrad(M, K, Co, one, one, one, one, None),
          lambda M, K, Co: lib.mcg_fc_wgrad(M, K, Co, one, one, one, None, None))
    for M, K, Co in ((64, 30, 60), (64, 1022, 62), (4, 2, 1), (0, 1024, 60), (64, 0, 60), (64, 1024, 0), (-8, 1024, 60), (64, -4, 60)):
        for f in fc:
            assert f(M, K, Co) == BAD, (M, K, Co)
    for period in (0, -64, 6, 62, 48, 2048):                                # zero, negative, no multiple of 4 (twice), no divisor of K (twice)
        assert lib.mcg_fc_dgrad(64, 1024, 62, one, one, one, period, one, None) == BAD, period

    for N, C in ((0, 1), (19, 0), (0, 7), (-1, 7)):
        for ce in (0, 1):
            assert lib.mcg_loss_dis(N, C, one, one, one, one, ce, one, one, one, None) == BAD, (N, C, ce)
            assert lib.mcg_loss_gen(N, C, one, one, one, ce, one, one, one, None) == BAD, (N, C, ce)
    assert lib.mcg_loss_dis(19, 1, one, one, one, one, 1, one, one, one, None) == BAD         # no class columns beside the GAN logit
    assert lib.mcg_loss_gen(19, 1, one, one, one, 1, one, one, one, None) == BAD
    assert lib.mcg_loss_dis(19, 7, one, one, None, one, 1, one, one, one, None) == BAD        # classes without labels
    assert lib.mcg_loss_dis(19, 7, one, one, one, None, 1, one, one, one, None) == BAD
    assert lib.mcg_loss_gen(19, 7, one, one, None, 1, one, one, one, None) == BAD


def test_layout_and_partial_sum_entry_points_refuse_on_the_host(hl):
    """The layout kernels and the consumers of per-tile partial sums index with whatever extents and strides they are given: what
    they cannot take is refused before anything is launched.  `one` is a non-null pointer that is never dereferenced, the outputs
    are small host buffers that must come back untouched; no call below passes an acceptable argument set."""
    lib = hl.load()
    one = ctypes.c_void_p(16)
    BAD, UNSUPPORTED = -1, -2
    bufs = [(ctypes.c_float * 16)(*([3.0] * 16)) for _ in range(5)]
    o1, o2, o3, o4, o5 = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    calls = []

    def refused(code, rc, *what):
        calls.append(what)
        assert rc == code, (what, rc)
        assert all(list(b) == [3.0] * 16 for b in bufs), what

    pack = lambda N, C, Cp, T, HW, sn=1, sc=1, x=one, out=o1: lib.mcg_pack_clip(N, C, Cp, T, HW, x, sn, sc, None, 0.0, 0, 0, out, None)
    pack8 = lambda N, C, Cp, T, HW, sn=1, st=1, x=one, out=o1: lib.mcg_pack_clip_u8(N, C, Cp, T, HW, x, sn, st, None, 0.0, 0, 0, out, None)
    for name, f in (("mcg_pack_clip", pack), ("mcg_pack_clip_u8", pack8)):
        refused(BAD, f(2, 5, 4, 3, 8), name, "Cp < C")
        refused(BAD, f(2, 3, 6, 3, 8), name, "Cp % 4")
        refused(BAD, f(2, 3, 0, 3, 8), name, "Cp = 0")
        for ext in ((0, 3, 4, 3, 8), (2, 0, 4, 3, 8), (2, 3, 4, 0, 8), (2, 3, 4, 3, 0), (-2, 3, 4, 3, 8), (2, 3, 4, -3, 8), (2, 3, 4, 3, -8)):
            refused(BAD, f(*ext), name, ext)
        refused(BAD, f(2, 3, 4, 3, 8, sn=-72), name, "negative item stride")
        refused(BAD, f(2, 3, 4, 3, 8, 72, -24), name, "negative channel / frame stride")
        refused(BAD, f(2, 3, 4, 3, 8, x=None), name, "no x")
        refused(BAD, f(2, 3, 4, 3, 8, out=None), name, "no out")

    unpack = lambda N, C, Cp, T, HW, inp=one, x=o1: lib.mcg_unpack_clip(N, C, Cp, T, HW, inp, x, None)
    refused(BAD, unpack(2, 5, 4, 3, 8), "mcg_unpack_clip", "Cp < C")
    for ext in ((0, 3, 4, 3, 8), (2, 0, 4, 3, 8), (2, 3, 4, 0, 8), (2, 3, 4, 3, 0), (2, 3, 4, 3, -8)):
        refused(BAD, unpack(*ext), "mcg_unpack_clip", ext)
    refused(BAD, unpack(2, 3, 4, 3, 8, inp=None), "mcg_unpack_clip", "no in")
    refused(BAD, unpack(2, 3, 4, 3, 8, x=None), "mcg_unpack_clip", "no x")

    tanh = lambda N, T, fe, g=one, x=one, out=o1: lib.mcg_tanh_bwd_to_frames(N, T, fe, g, x, out, None)
    for fe in (1, 2, 3, 6, 257, 0, -4):
        refused(BAD, tanh(3, 5, fe), "mcg_tanh_bwd_to_frames", "frame_elems", fe)
    refused(BAD, tanh(0, 5, 256), "mcg_tanh_bwd_to_frames", "N = 0")
    refused(BAD, tanh(3, 0, 256), "mcg_tanh_bwd_to_frames", "T = 0")
    for hole in range(3):
        ptrs = [None if k == hole else p for k, p in enumerate((one, one, o1))]
        refused(BAD, tanh(3, 5, 256, *ptrs), "mcg_tanh_bwd_to_frames", "null pointer", hole)

    concat = lambda N, P, C, Cp, dl, Cq, x=one, labels=one, out=o1: lib.mcg_concat_label_planes(N, P, C, Cp, dl, Cq, x, labels, out, None)
    refused(BAD, concat(3, 64, 3, 4, 6, 8), "mcg_concat_label_planes", "Cq < C + dl")
    refused(BAD, concat(3, 64, 3, 4, 0, 0), "mcg_concat_label_planes", "Cq < C")
    refused(BAD, concat(3, 64, 3, 4, 6, 10), "mcg_concat_label_planes", "Cq % 4")
    refused(BAD, concat(3, 64, 3, 4, 6, 12, labels=None), "mcg_concat_label_planes", "label planes without labels")
    refused(BAD, concat(3, 64, 5, 4, 6, 12), "mcg_concat_label_planes", "Cp < C")
    refused(BAD, concat(3, 64, 3, 4, -1, 12), "mcg_concat_label_planes", "dl < 0")
    refused(BAD, concat(0, 64, 3, 4, 6, 12), "mcg_concat_label_planes", "N = 0")
    refused(BAD, concat(3, 0, 3, 4, 6, 12), "mcg_concat_label_planes", "P = 0")
    refused(BAD, concat(3, 64, 0, 4, 6, 12), "mcg_concat_label_planes", "C = 0")
    refused(BAD, concat(3, 64, 3, 4, 6, 12, x=None), "mcg_concat_label_planes", "no x")
    refused(BAD, concat(3, 64, 3, 4, 6, 12, out=None), "mcg_concat_label_planes", "no out")

    # the consumers of partial sums: stats (o1), running averages (o2, o3), gx (o1), dgamma / dbeta (o2, o3), db (o1), workspace (o4)
    def stats(M, C, n, stride, part=one, am=o2, av=o3, ws=o4):
        return lib.mcg_bn_stats_from_partials(M, C, part, n, stride, one, one, o1, am, av, 2e-5, 0.9, ws, None)

    def bwd(M, C, n, stride, part=one, ws=o4, flags=0, gx=o1):
        return lib.mcg_bn_act_bwd_from_partials(M, C, one, one, one, one, 2, part, n, stride, gx, flags, o2, o3, ws, None)

    def colsum(M, C, n, stride, part=one, ws=o4):
        return lib.mcg_colsum_from_partials(C, part, n, stride, o1, ws, None)

    for name, f in (("mcg_bn_stats_from_partials", stats), ("mcg_bn_act_bwd_from_partials", bwd), ("mcg_colsum_from_partials", colsum)):
        refused(BAD, f(64, 8, 0, 16), name, "n_slots = 0")
        refused(BAD, f(64, 8, -3, 16), name, "n_slots < 0")
        refused(BAD, f(64, 8, 5, 15), name, "slot_stride < 2 C")
        refused(BAD, f(64, 8, 5, 8), name, "slot_stride = C")
        refused(BAD, f(64, 8, 5, 0), name, "slot_stride = 0")
        refused(BAD, f(64, 6, 5, 16), name, "C % 4")
        refused(BAD, f(64, 0, 5, 16), name, "C = 0")
        refused(BAD, f(64, 8, 5, 16, part=None), name, "no partials")
    refused(BAD, stats(0, 8, 5, 16), "mcg_bn_stats_from_partials", "M = 0")
    refused(BAD, bwd(0, 8, 5, 16), "mcg_bn_act_bwd_from_partials", "M = 0")
    refused(BAD, stats(64, 8, 5, 16, av=None), "mcg_bn_stats_from_partials", "avg_mean without avg_var")
    refused(BAD, stats(64, 8, 5, 16, am=None), "mcg_bn_stats_from_partials", "avg_var without avg_mean")
    refused(BAD, bwd(64, 8, 5, 16, ws=None), "mcg_bn_act_bwd_from_partials", "no workspace")
    refused(BAD, bwd(64, 8, 5, 16, gx=None), "mcg_bn_act_bwd_from_partials", "no gx")
    refused(BAD, bwd(64, 8, 5, 16, flags=hl.IO_OUT_BF16, gx=one), "mcg_bn_act_bwd_from_partials", "in place across element types")
    refused(UNSUPPORTED, bwd(64, 8, 5, 16, flags=hl.IO_OUT_SPLIT), "mcg_bn_act_bwd_from_partials", "split output of 8 channels")

    acc = lambda M, C, g=one, db=o1, ws=o4: lib.mcg_colsum_acc(M, C, g, db, ws, None)
    refused(BAD, acc(0, 8), "mcg_colsum_acc", "M = 0")
    refused(BAD, acc(-5, 8), "mcg_colsum_acc", "M < 0")
    refused(BAD, acc(64, 6), "mcg_colsum_acc", "C % 4")
    refused(BAD, acc(64, 0), "mcg_colsum_acc", "C = 0")
    refused(UNSUPPORTED, acc(64, 24), "mcg_colsum_acc", "6 channel quads do not divide a block")
    refused(UNSUPPORTED, acc(64, 2048), "mcg_colsum_acc", "more channel quads than threads")
    refused(BAD, acc(64, 8, g=None), "mcg_colsum_acc", "no g")
    refused(BAD, acc(64, 8, db=None), "mcg_colsum_acc", "no db")
    refused(BAD, acc(64, 8, ws=None), "mcg_colsum_acc", "no workspace")

    quad = lambda M, C, out=o1: lib.mcg_randn_rowquad(M, C, 0.2, 1, 2, out, None)
    for M in (1, 2, 3, 5, 6, 1023, 0, -4):
        refused(BAD, quad(M, 64), "mcg_randn_rowquad", "M", M)
    refused(BAD, quad(64, 0), "mcg_randn_rowquad", "C = 0")
    refused(BAD, quad(64, 64, out=None), "mcg_randn_rowquad", "no out")
    assert len(calls) > 100


def test_product_path_refuses_host_tensors(hl):
    g = hl.make_geom(1, 4, 16, 16, 4, 64, 4)
    x = torch.zeros(16)
    with pytest.raises(hl.McgError):
        hl.conv_fprop(g, x, x, None, x)
    with pytest.raises(hl.McgError):
        hl.adam_wd(x, x, x, x, 1e-3, 0.9, 0.999, 1e-8, 0.0)


def test_layout_round_trips():
    import mocogan_chainer_amd.layout as lay
    rng = np.random.RandomState(0)
    x = torch.tensor(rng.randn(2, 3, 5, 8, 8), dtype=torch.float32)
    xd = lay.act_to_dev(x)
    assert xd.shape == (2, 5, 8, 8, 4) and float(xd[..., 3].abs().max()) == 0
    assert torch.equal(lay.act_from_dev(xd, 3), x)
    x2 = torch.tensor(rng.randn(2, 3, 8, 8), dtype=torch.float32)
    assert torch.equal(lay.act_from_dev(lay.act_to_dev(x2), 3, 2), x2)
    w = torch.tensor(rng.randn(8, 3, 4, 4, 4), dtype=torch.float32)
    wd = lay.conv_w_to_dev(w)
    assert wd.shape == (8, 4, 4, 4, 4)
    assert torch.equal(lay.conv_w_from_dev(wd, 3, 3), w)
    # w_dev[co][kt][kh][kw][ci] == W[co][ci][kt][kh][kw]
    assert float(wd[5, 1, 2, 3, 2]) == float(w[5, 2, 1, 2, 3])
    dw = torch.tensor(rng.randn(60, 512, 4, 4), dtype=torch.float32)
    dd = lay.deconv_w_to_dev(dw)
    assert dd.shape == (60, 1, 4, 4, 512) and torch.equal(lay.deconv_w_from_dev(dd, 512), dw)
    params = {'g0/%s/%s' % (k, s): torch.tensor(rng.randn(*((10, 16 if k[0] == 'W' else 10) if s == 'W' else (10,))), dtype=torch.float32)
              for k in lay.GRU_LINKS for s in ('W', 'b')}
    flat = lay.gru_to_dev(params)
    assert flat.numel() == 3 * (160 + 10) + 3 * (100 + 10)
    back = lay.gru_from_dev(flat, 10, 6)
    for k in params:
        assert torch.equal(back[k], params[k])


def test_adam_hyper_matches_reference_settings():
    """train.py:93-101: Adam(alpha=2e-4, beta1=5e-5) (beta2 never forwarded) + WeightDecay(1e-5)."""
    import mocogan_chainer_amd.step as step
    from oracle import updater as oupd
    h = step.AdamHyper()
    assert (h.alpha, h.beta1, h.beta2, h.eps, h.weight_decay) == (2e-4, 5e-5, 0.999, 1e-8, 1e-5)
    for t in (1, 2, 10):
        assert np.isclose(h.lr(t), oupd.ADAM_ALPHA * np.sqrt(1 - oupd.ADAM_BETA2 ** t) / (1 - oupd.ADAM_BETA1 ** t), rtol=1e-15)
    with pytest.raises(ValueError):
        step.make_models('cgan', num_labels=0, device='cpu')


def test_missing_library_fails_loudly():
    """No CPU fallback: with the shared library absent the binding raises instead of computing something else."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import mocogan_chainer_amd.hiplib as hl\n"
            "try:\n    hl.load()\nexcept hl.McgError as e:\n    print('RAISED', 'no CPU fallback' in str(e))\n" % ROOT)
    env = dict(os.environ, MCG_LIB_PATH='/nonexistent/libmocogan_hip.so')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, timeout=300)
    assert 'RAISED True' in r.stdout, r.stdout + r.stderr
