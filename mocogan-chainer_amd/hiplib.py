"""ctypes binding of libmocogan_hip.so (declared in include/mocogan_hip.h).

PyTorch-ROCm supplies device memory and the HIP stream only; every call below hands raw
device pointers to a hand-written gfx950 kernel.  There is no fallback: if the library is
missing or a status is non-zero this module raises.
"""
import ctypes as C
import os

import torch

from . import tiles
from .build import lib_path
from .tiles import (PREC_F32, PREC_BF16, PREC_BF16_STORE, PREC_SPLIT, PREC_BF16_Y16, TILE_CANDIDATES, FPROP_SPLIT_CANDIDATES,  # noqa: F401
                    WGRAD_SPLIT_CANDIDATES, V2_CANDIDATES, DENSE_CANDIDATES, LIVE_CANDIDATES, LIVE_WGRAD_CANDIDATES, split_covers)

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3

_STATUS = {0: "MCG_OK", -1: "MCG_ERR_BAD_ARG", -2: "MCG_ERR_UNSUPPORTED", -3: "MCG_ERR_LAUNCH",
           -4: "MCG_ERR_WORKSPACE"}


class McgError(RuntimeError):
    pass


class ConvGeom(C.Structure):
    """mcg_conv_geom"""
    _fields_ = [("N", C.c_int32), ("Ti", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32), ("Ci", C.c_int32),
                ("To", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("Co", C.c_int32),
                ("kt", C.c_int32), ("x_perm_n", C.c_int32), ("precision", C.c_int32),
                ("tile", C.c_int32), ("ci_valid", C.c_int32),
                ("x_stride0", C.c_int64), ("x_stride1", C.c_int64)]


SUMS_NONE, SUMS_STATS, SUMS_BN_BWD, SUMS_COL = 0, 1, 2, 3
IO_OUT_BF16, IO_Y_BF16, IO_G_BF16, IO_OUT_SPLIT = 1, 2, 4, 8          # MCG_IO_*: which tensors of an element-wise call are bf16


class ConvEpilogue(C.Structure):
    """mcg_conv_epilogue: what the conv's epilogue fuses (include/mocogan_hip.h)."""
    _fields_ = [("sums", C.c_int32), ("groups", C.c_int32), ("part", C.c_void_p), ("bn_y", C.c_void_p),
                ("bn_stats", C.c_void_p * 2), ("bn_act", C.c_int32), ("act", C.c_int32), ("addend", C.c_void_p * 2),
                ("sigma", C.c_float), ("seed", C.c_uint64), ("stream_id", C.c_uint64 * 2),
                ("mask_out", C.c_void_p), ("out_bf16", C.c_int32), ("mask_in", C.c_void_p), ("n_slots", C.c_int32),
                ("slot_stride", C.c_int32), ("bn_y_bf16", C.c_int32)]


_P, _I, _I64, _U64, _F, _D = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double
_GP = C.POINTER(ConvGeom)
_EP = C.POINTER(ConvEpilogue)

# name -> (restype, argtypes); mirrors include/mocogan_hip.h one to one
SIGNATURES = {
    "mcg_version": (_I, []),
    "mcg_conv_fprop": (_I, [_GP, _P, _P, _P, _P, _P]),
    "mcg_conv_dgrad": (_I, [_GP, _P, _P, _P, _P, _I, _I, _P]),
    "mcg_conv_wgrad": (_I, [_GP, _P, _P, _P, _P]),
    "mcg_conv_fprop_ex": (_I, [_GP, _P, _P, _P, _P, _EP, _P]),
    "mcg_conv_dgrad_ex": (_I, [_GP, _P, _P, _P, _P, _EP, _P]),
    "mcg_conv_epilogue_part_bytes": (_I64, [_GP, _I, _I]),
    "mcg_conv_dense_split_ok": (_I, [_GP, _I]),
    "mcg_conv_dense_split_chunk": (_I, [_GP, _I]),
    "mcg_bn_stats_from_partials": (_I, [_I64, _I, _P, _I, _I, _P, _P, _P, _P, _P, _F, _F, _P, _P]),
    "mcg_bn_act_bwd_from_partials": (_I, [_I64, _I, _P, _P, _P, _P, _I, _P, _I, _I, _P, _I, _P, _P, _P, _P]),
    "mcg_colsum_from_partials": (_I, [_I, _P, _I, _I, _P, _P, _P]),
    "mcg_randn_rowquad": (_I, [_I64, _I, _F, _U64, _U64, _P, _P]),
    "mcg_fc_fprop": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "mcg_fc_dgrad": (_I, [_I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "mcg_fc_wgrad": (_I, [_I, _I, _I, _P, _P, _P, _P, _P]),
    "mcg_bn_workspace_bytes": (_I64, [_I64, _I]),
    "mcg_bn_stats": (_I, [_I64, _I, _P, _P, _P, _P, _P, _P, _F, _F, _P, _P]),
    "mcg_bn_act_fwd": (_I, [_I64, _I, _I, _P, _I64, _I64, _P, _I, _P, _F, _U64, _U64, _P, _I, _P]),
    "mcg_bn_act_bwd": (_I, [_I64, _I, _P, _P, _P, _P, _I, _P, _I, _P, _P, _P, _P]),
    "mcg_bn_sums": (_I, [_I64, _I, _P, _P, _P, _P]),
    "mcg_bn_stats_from_sums": (_I, [_I64, _I, _P, _P, _P, _P, _P, _P, _F, _F, _P]),
    "mcg_bn_bwd_sums": (_I, [_I64, _I, _P, _P, _P, _I, _I, _P, _P, _P]),
    "mcg_bn_act_bwd_from_sums": (_I, [_I64, _I64, _I, _P, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "mcg_colsum_acc": (_I, [_I64, _I, _P, _P, _P, _P]),
    "mcg_pack_clip": (_I, [_I, _I, _I, _I, _I, _P, _I64, _I64, _P, _F, _U64, _U64, _P, _P]),
    "mcg_unpack_clip": (_I, [_I, _I, _I, _I, _I, _P, _P, _P]),
    "mcg_pack_clip_u8": (_I, [_I, _I, _I, _I, _I, _P, _I64, _I64, _P, _F, _U64, _U64, _P, _P]),
    "mcg_clip_to_u8": (_I, [_I, _I, _I, _I, _I, _P, _P, _I, _P, _I64, _I64, _P]),
    "mcg_bn_fold_deconv": (_I, [_I64, _I, _I, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P]),
    "mcg_concat_label_planes": (_I, [_I, _I64, _I, _I, _I, _I, _P, _P, _P, _P]),
    "mcg_tanh_bwd_to_frames": (_I, [_I, _I, _I64, _P, _P, _P, _P]),
    "mcg_gru_seq_fwd": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcg_gru_seq_bwd": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "mcg_loss_dis": (_I, [_I, _I, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "mcg_loss_gen": (_I, [_I, _I, _P, _P, _P, _I, _P, _P, _P, _P]),
    "mcg_adam_wd": (_I, [_I64, _P, _P, _P, _P, _D, _D, _D, _D, _D, _D, _P, _P]),
    "mcg_adam_wd_ema": (_I, [_I64, _P, _P, _P, _P, _D, _D, _D, _D, _D, _D, _P, _P, _F, _P]),
    "mcg_ema_multi": (_I, [_I, _P, _F, _P]),
    "mcg_grad_stats_workspace_bytes": (_I64, [_I]),
    "mcg_grad_stats_span": (_I, []),
    "mcg_grad_stats": (_I, [_I, _P, _P, _D, _D, _P, _P, _P, _P]),
    "mcg_adam_wd_ctl": (_I, [_I64, _P, _P, _P, _P, _D, _D, _D, _D, _D, _P, _P, _P, _F, _P]),
    "mcg_randn": (_I, [_I64, _F, _U64, _U64, _P, _P]),
    "mcg_randint": (_I, [_I64, _I, _U64, _U64, _P, _P]),
    "mcg_split_planes": (_I, [_I64, _I64, _P, _P, _P]),
    "mcg_split_planes_multi": (_I, [_I, _P, _P]),
    "mcg_augment_workspace_bytes": (_I64, [_I]),
    "mcg_augment_draw": (_I, [_I, _I, _I, _I, _U64, _U64, _P, _P, _P]),
    "mcg_augment_draw_gated": (_I, [_I, _I, _I, _I, _U64, _U64, _U64, _P, _P, _P, _P]),
    "mcg_ada_update": (_I, [_I, _I, _P, _P, _D, _D, _I, _P, _P]),
    "mcg_augment_fwd": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "mcg_augment_bwd": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "mcg_warp_fwd": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "mcg_warp_bwd": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "mcg_warp_draw": (_I, [_I, _I, _I, _I, _U64, _U64, _P, _P]),
    "mcg_warp_draw_gated": (_I, [_I, _I, _I, _I, _U64, _U64, _U64, _P, _P, _P]),
    "mcg_swd_workspace_bytes": (_I64, [_I64, _I, _I]),
    "mcg_swd_pyramid": (_I, [_I, _I, _I, _I, _I, _P, _P, _P, _P, _P]),
    "mcg_swd_gather": (_I, [_I, _I, _I, _I, _P, _I64, _I, _I, _U64, _U64, _P, _P]),
    "mcg_swd_channel_sums": (_I, [_I64, _I, _I, _P, _P, _P, _P]),
    "mcg_swd_normalize": (_I, [_I64, _I, _I, _P, _P, _P]),
    "mcg_swd_unit_columns": (_I, [_I, _I, _P, _P]),
    "mcg_swd_project": (_I, [_I64, _I, _I, _P, _P, _P, _I64, _P]),
    "mcg_sort_local_span": (_I, []),
    "mcg_sort_rows": (_I, [_I, _I64, _P, _I64, _P, _P]),
    "mcg_swd_distance": (_I, [_I, _I64, _I64, _P, _I64, _P, _I64, _P, _P, _P]),
    "mcg_knn_descriptors": (_I, [_I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "mcg_knn_sqdist": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _I64, _P]),
    "mcg_knn_smallest": (_I, [_I, _I, _P, _I64, _I, _I, _I64, _P, _P, _P]),
    "mcg_knn_ball_counts": (_I, [_I, _I, _P, _I64, _P, _P, _P]),
    "mcg_mc_frame_sqdist": (_I, [_I, _I, _I, _P, _P, _P]),
    "mcg_mc_clip_stats": (_I, [_I, _I, _P, _P, _P, _P]),
    "mcg_mc_motion_descriptors": (_I, [_I, _I, _I, _P, _P, _P, _P]),
}

ABI_VERSION = 8          # MCG_ABI_VERSION of include/mocogan_hip.h these prototypes were written against

_lib = None


def load():
    """dlopen the in-tree library (never a site-packages copy) and type every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise McgError("libmocogan_hip.so not built (%s): run __graft_entry__.build(); "
                       "there is no CPU fallback for the product path" % path)
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.mcg_version() != ABI_VERSION:
        raise McgError("%s is ABI revision %d, this binding expects %d: rebuild it (__graft_entry__.build())"
                       % (path, lib.mcg_version(), ABI_VERSION))
    _lib = lib
    return lib


_SYNC_EVERY_CALL = os.environ.get("MCG_SYNC", "0") == "1"     # debugging aid: serialise host and device


def _check(status, name):
    if status != 0:
        raise McgError("%s failed: %s" % (name, _STATUS.get(status, status)))
    if _SYNC_EVERY_CALL:
        torch.cuda.synchronize()


def _p(t, dtype=torch.float32):
    """device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise McgError("the HIP path needs device tensors (got a %s tensor)" % t.device)
    if t.dtype != dtype:
        raise McgError("expected %s, got %s" % (dtype, t.dtype))
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dense(t):
    if t is not None and not t.is_contiguous():
        raise McgError("tensor must be dense")
    return t


PRECISIONS = {"f32": PREC_F32, "fp32": PREC_F32, "bf16": PREC_BF16, "bf16s": PREC_BF16_STORE, "f32x3": PREC_SPLIT, "bf16y": PREC_BF16_Y16,
              PREC_F32: PREC_F32, PREC_BF16: PREC_BF16, PREC_BF16_STORE: PREC_BF16_STORE, PREC_SPLIT: PREC_SPLIT,
              PREC_BF16_Y16: PREC_BF16_Y16}


def _pin(g, t, side='x'):
    """device pointer of an INPUT operand of a conv launch (side: 'x' | 'y' | 'w'): bf16 tensors for MCG_PREC_BF16_STORE / split
    geometries, and for the y side of MCG_PREC_BF16_Y16"""
    if g.precision == PREC_BF16_Y16:
        return _p(t, torch.bfloat16 if side == 'y' else torch.float32)
    return _p(t, torch.bfloat16 if g.precision in (PREC_BF16_STORE, PREC_SPLIT) else torch.float32)


def _pany(t):
    """device pointer of a tensor that may be fp32 or bf16 (outputs of the element-wise passes) -> (pointer, is_bf16)"""
    if t.dtype == torch.bfloat16:
        return _p(t, torch.bfloat16), 1
    return _p(t), 0


def make_geom(N, Ti, Hi, Wi, Ci, Co, kt, x_stride0=None, x_perm_n=0, x_stride1=0, precision=PREC_F32, ci_valid=0):
    """Geometry of one k4 s(1,2,2) p(0,1,1) layer; x side [N][Ti][Hi][Wi][Ci], y side dense.  ci_valid: channels of x
    that carry data (0 = all Ci): 3 for the RGB clip stored with Ci = 4."""
    g = ConvGeom()
    g.precision = PRECISIONS[precision]
    g.ci_valid = ci_valid
    g.N, g.Ti, g.Hi, g.Wi, g.Ci = N, Ti, Hi, Wi, Ci
    g.To, g.Ho, g.Wo, g.Co, g.kt = Ti - kt + 1, Hi // 2, Wi // 2, Co, kt
    g.x_perm_n = x_perm_n
    g.x_stride0 = Ti * Hi * Wi * Ci if x_stride0 is None else x_stride0
    g.x_stride1 = x_stride1
    return g


# ------------------------------------------------------------------------------------------
# optional per-launch timing of the conv kernels with HIP events on the launch stream (bench.py's
# roofline leg).  Off by default; costs two event records per conv launch when on.
# ------------------------------------------------------------------------------------------
_timing = None
_tag = ""


def set_tag(tag):
    """Label (network name) attached to the conv launches that follow."""
    global _tag
    _tag = tag


def get_tag():
    return _tag


def timing_begin():
    global _timing
    _timing = {}


def timing_end():
    """-> {"<tag>.<pass>": (launches, total_ms)}; synchronises the device."""
    global _timing
    t, _timing = _timing, None
    torch.cuda.synchronize()
    return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in (t or {}).items()}


split_launches = 0          # conv launches in the MCG_PREC_SPLIT form so far (tests assert that the form really ran)
split_only_outputs = 0      # element-wise launches that wrote their output in the split layout only


def _timed(call, *keys):
    """call(), bracketed by two events on the current stream that are filed under every key while timing_begin() is on"""
    if _timing is None:
        return call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = call()
    e1.record()
    for k in keys:
        _timing.setdefault(k, []).append((e0, e1))
    return r


def _best_ms(call):
    """How the tuners time a candidate: one warm-up call (its McgError reaches the caller: an impossible candidate), then the best
    of three timings of two calls each, in ms.  Tuning launches are not part of any measurement: timing is suspended meanwhile."""
    global _timing
    saved, _timing = _timing, None
    try:
        call()
        best = None
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            call()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            best = ms if best is None or ms < best else best
        return best
    finally:
        _timing = saved


def _launch(kind, fn, *args):
    g = args[0]
    if g.precision == PREC_SPLIT:
        global split_launches
        split_launches += 1
    if _timing is None:                                         # (the per-geometry key is only built when it is used)
        return fn(*args)
    return _timed(lambda: fn(*args), _tag + "." + kind,        # per-geometry detail: "<tag>.<pass> N T H Ci Co"
                  "%s.%s N=%d T=%d H=%d Ci=%d Co=%d" % (_tag, kind, g.N, g.Ti, g.Hi, g.Ci, g.Co))


def with_precision(g, precision):
    """a copy of the geometry for another operand form of the same layer (its tile is chosen afresh)"""
    h = ConvGeom.from_buffer_copy(g)
    h.precision = PRECISIONS[precision]
    h.tile = 0
    return h


_PASS = {"fprop": 0, "dgrad": 1, "wgrad": 2}


def dense_split_ok(kind, g):
    """does the dense LDS form of the MCG_PREC_SPLIT launch (tile codes 17 / 20) exist for this pass and geometry?  The library's own
    answer (mcg_conv_dense_split_ok); launches nothing."""
    return bool(load().mcg_conv_dense_split_ok(C.byref(g), _PASS[kind]))


def dense_split_chunk(kind, g):
    """the part of the summed dimension one block of a dense split launch covers (g.tile: its K-split digit) -- split elements
    (256 per triple of K-steps) in fprop / dgrad, pixels (64 per triple) in wgrad; 0 when the form does not apply"""
    return int(load().mcg_conv_dense_split_chunk(C.byref(g), _PASS[kind]))


# ------------------------------------------------------------------------------------------
# which tile a conv launch takes: tiles.py holds the candidate rules, the table, the shipped lists and the timing loop;
# here are its public names (one table per process); _measure below is the measurement it is handed
# ------------------------------------------------------------------------------------------
_table = tiles.table
set_autotune, autotune_on, reset_tuning, set_tile_override = _table.set_autotune, _table.autotune_on, _table.reset, _table.set_override
use_pretuned_table, use_dense_list, use_live_list = _table.use_pretuned, _table.use_dense, _table.use_live
tile_choices, save_tile_choices, load_tile_choices, replace_tile_choices = _table.as_dict, _table.save, _table.load, _table.replace
table_tile, split_decided, _with_override = _table.tile, _table.split_decided, _table.with_override


def live_list(path=None):
    """{key: code} of live_tiles_mi355x.json (or of `path`), checked (tiles.live_list)"""
    return tiles.live_list(path or _table.live)


def split_pays(kind, g, run_plain, run_split):
    """_table.split_pays with the tuners' timing: does the split form of this launch beat the fp32 form?  Timed once per geometry."""
    return _table.split_pays(kind, g, run_plain, run_split, _best_ms)


def _scratch_like(g, which):
    """dense scratch tensors with the extents of the geometry's x / y / w sides"""
    if which == 'x':
        if g.x_perm_n:
            n = (g.x_perm_n - 1) * g.x_stride0 + (g.N // g.x_perm_n - 1) * g.x_stride1 + g.Ti * g.Hi * g.Wi * g.Ci
        else:
            n = (g.N - 1) * g.x_stride0 + g.Ti * g.Hi * g.Wi * g.Ci
        return torch.zeros(n, device='cuda')
    if which == 'y':
        return torch.zeros(g.N * g.To * g.Ho * g.Wo * g.Co, device='cuda')
    return torch.zeros(g.Co * g.kt * 16 * g.Ci, device='cuda')


# ------------------------------------------------------------------------------------------
# thin typed wrappers (tensors in; nothing allocated here except the one-off tuning scratch)
# ------------------------------------------------------------------------------------------
def _fprop(g, x, w, bias, y):
    if y.dtype == torch.bfloat16:                     # bf16 output: the flag travels in an (otherwise empty) epilogue
        return _fprop_ex(g, x, w, bias, y, epilogue(out_bf16=True), split_ok=True)
    g = _with_override(g)
    _check(load().mcg_conv_fprop(C.byref(g), _pin(g, x), _pin(g, _dense(w), 'w'), _p(bias), _p(_dense(y)), _stream()), "mcg_conv_fprop")


def _dgrad(g, y, w, bias, x, act, accumulate):
    if x.dtype == torch.bfloat16:
        assert act in (ACT_NONE, ACT_RELU) and not accumulate       # (ReLU in the store travels in the epilogue's act field)
        return _dgrad_ex(g, y, w, bias, x, epilogue(out_bf16=True, act=act), split_ok=True)
    g = _with_override(g)
    _check(load().mcg_conv_dgrad(C.byref(g), _pin(g, _dense(y), 'y'), _pin(g, _dense(w), 'w'), _p(bias), _p(x), act, int(accumulate), _stream()),
           "mcg_conv_dgrad")


def _wgrad(g, x, y, dw):
    g = _with_override(g)
    _check(load().mcg_conv_wgrad(C.byref(g), _pin(g, x), _pin(g, _dense(y), 'y'), _p(_dense(dw)), _stream()), "mcg_conv_wgrad")


# ---- fused epilogues (mcg_conv_epilogue) ---------------------------------------------------------
def _vp(t, dtype=torch.float32):
    """raw device address (0 for None) for the pointer fields of ConvEpilogue"""
    p = _p(t, dtype)
    return None if p is None else p.value


def epilogue(sums=SUMS_NONE, groups=1, part=None, bn_y=None, bn_stats=(None, None), bn_act=ACT_NONE, act=ACT_NONE,
             addend=(None, None), sigma=0.0, seed=0, stream_id=(0, 0), mask_out=None, mask_in=None, out_bf16=False, out_split=False):
    """Builds a ConvEpilogue; the tensors must stay alive until the launch has been queued (they are the caller's)."""
    ep = ConvEpilogue()
    y16 = bn_y is not None and bn_y.dtype == torch.bfloat16
    ep.sums, ep.groups, ep.part, ep.bn_y = sums, groups, _vp(part), _vp(_dense(bn_y), torch.bfloat16 if y16 else torch.float32)
    ep.bn_y_bf16 = int(y16)
    ep.bn_stats[0], ep.bn_stats[1] = _vp(bn_stats[0]), _vp(bn_stats[1] if len(bn_stats) > 1 else None)
    ep.bn_act, ep.act = bn_act, act
    ep.addend[0], ep.addend[1] = _vp(_dense(addend[0])), _vp(_dense(addend[1] if len(addend) > 1 else None))
    ep.sigma, ep.seed = float(sigma), int(seed)
    ep.stream_id[0], ep.stream_id[1] = int(stream_id[0]), int(stream_id[1] if len(stream_id) > 1 else 0)
    ep.mask_out, ep.mask_in = _vp(_dense(mask_out), torch.int32), _vp(_dense(mask_in), torch.int32)
    ep.out_bf16 = IO_OUT_SPLIT if out_split else int(bool(out_bf16))      # (out_split: the MCG_PREC_SPLIT layout, a bf16 tensor of 4 * Co columns)
    return ep


def epilogue_part_floats(g, kind, groups):
    """floats the per-tile partial sums of a fused epilogue can need for geometry g ('fprop' | 'dgrad')"""
    return int(load().mcg_conv_epilogue_part_bytes(C.byref(g), 0 if kind == "fprop" else 1, groups)) // 4


def _no_split(g):
    """the tile code without its split-K part: partial tiles cannot carry an epilogue"""
    if g.tile < 1000:
        return g
    gg = ConvGeom.from_buffer_copy(g)
    gg.tile = g.tile % 1000
    return gg


def _fprop_ex(g, x, w, bias, y, ep, split_ok=False):
    """split_ok: leave a split-K tile code in place (the library then refuses it for a bf16 output: the caller asked
    fprop_tile / dgrad_tile first)"""
    g = _with_override(g) if split_ok else _no_split(_with_override(g))
    assert bool(ep.out_bf16) == (y.dtype == torch.bfloat16)
    yp = _p(_dense(y), torch.bfloat16) if ep.out_bf16 else _p(_dense(y))
    _check(load().mcg_conv_fprop_ex(C.byref(g), _pin(g, x), _pin(g, _dense(w), 'w'), _p(bias), yp, C.byref(ep), _stream()), "mcg_conv_fprop_ex")


def _dgrad_ex(g, y, w, bias, x, ep, split_ok=False):
    g = _with_override(g) if split_ok else _no_split(_with_override(g))
    assert bool(ep.out_bf16) == (x.dtype == torch.bfloat16)
    xp = _p(_dense(x), torch.bfloat16) if ep.out_bf16 else _p(_dense(x))
    _check(load().mcg_conv_dgrad_ex(C.byref(g), _pin(g, _dense(y), 'y'), _pin(g, _dense(w), 'w'), _p(bias), xp, C.byref(ep), _stream()),
           "mcg_conv_dgrad_ex")


def dgrad_c4_mfma_covers(g):
    """True when conv_dgrad(g, ..., bias=None, act=ACT_NONE) runs the MFMA col2im kernel of the Ci = 4 layers (the library's
    own condition, restated for callers that split bias + tanh off into an element-wise pass to reach that kernel)."""
    frame = g.Ti * g.Hi * g.Wi * g.Ci
    whole = (g.x_stride1 == frame and g.x_stride0 == (g.N // g.x_perm_n) * frame) if g.x_perm_n else g.x_stride0 == frame
    return (g.Ci == 4 and 0 < g.ci_valid <= 3 and g.Co == 64 and g.Wo in (16, 32) and g.Ho % (128 // g.Wo) == 0 and whole
            and g.precision not in (PREC_BF16_STORE, PREC_SPLIT) and _with_override(g).tile in (0, 6))


def fprop_tile(g, x, w, bias):
    """the tile code the PLAIN conv_fprop uses for this geometry (tuned now if it has to be): codes >= 1000 split K, and a
    split launch can neither carry an epilogue nor write a bf16 output -- callers that want either ask before they allocate.
    (bf16 networks: the fused / bf16-output form is tuned separately and only over the tiles that admit it.)"""
    if _table.autotune and not g.tile:
        probe = torch.empty(0, device='cuda')
        g = _table.tuned("fprop", g, tiles.ep_key(g, None, False), _measure("fprop", g, x, w, bias, probe))
    return _with_override(g).tile


def dgrad_tile(g, y, w, bias, act=ACT_NONE, accumulate=False):
    if _table.autotune and not g.tile:
        probe = torch.empty(0, device='cuda')
        g = _table.tuned("dgrad", g, (act, int(accumulate)) + tiles.ep_key(g, None, False), _measure("dgrad", g, y, w, bias, probe, None, act, accumulate))
    return _with_override(g).tile


def _measure(kind, g, a, b, bias=None, out_like=None, ep=None, act=ACT_NONE, accumulate=False):
    """The measurement _table.tuned is handed: measure(geom) -> ms of the caller's form of the launch (epilogue, output type) with
    that geometry's tile code, None when the library refuses it.  The OUTPUT goes to scratch of its extent, allocated at the first
    candidate: tuning never touches the caller's output or accumulators.  (a, b) = (x, w) forward, (y, w) dgrad, (x, y) wgrad."""
    scratch = None

    def measure(gg):
        nonlocal scratch
        if scratch is None:
            scratch = _scratch_like(g, {"fprop": 'y', "dgrad": 'x', "wgrad": 'w'}[kind])

        def run():
            if kind == "wgrad":
                return _wgrad(gg, a, b, scratch)
            out = scratch.view(torch.bfloat16)[:scratch.numel()] if out_like.dtype == torch.bfloat16 else scratch
            if g.precision == PREC_BF16_STORE and (ep is not None or out_like.dtype == torch.bfloat16) and gg.tile < 1000:
                e2 = ep if ep is not None else epilogue(out_bf16=True)
                (_fprop_ex if kind == "fprop" else _dgrad_ex)(gg, a, b, bias, out, e2, split_ok=True)
            elif out_like.dtype == torch.bfloat16:
                raise McgError("a split-K tile cannot write a bf16 output")
            elif kind == "fprop":
                _fprop(gg, a, b, bias, scratch)
            else:
                _dgrad(gg, a, b, bias, scratch, act, accumulate)
        try:
            return _best_ms(run)                # (the warm-up rejects impossible candidates)
        except McgError:
            return None
    return measure


def conv_fprop(g, x, w, bias, y, ep=None, must_fuse=False):
    """ep: a ConvEpilogue to fuse into the launch.  Returns True when it was fused; False when the tile tuned for this
    geometry splits K (partial tiles cannot carry an epilogue) and must_fuse is off: then the PLAIN convolution ran and
    the caller does the epilogue's work with the stand-alone passes.  must_fuse drops the split instead."""
    if _table.autotune and not g.tile:
        g = _table.tuned("fprop", g, tiles.ep_key(g, ep, y.dtype == torch.bfloat16), _measure("fprop", g, x, w, bias, y, ep))   # x, w are only read
    if ep is not None and (must_fuse or _with_override(g).tile < 1000):
        _launch("fprop", _fprop_ex, g, x, w, bias, y, ep)
        return True
    _launch("fprop", _fprop, g, x, w, bias, y)
    return False


def conv_dgrad(g, y, w, bias, x, act=ACT_NONE, accumulate=False, ep=None, must_fuse=False, tune=True):
    """ep / return value as in conv_fprop (ep needs act == ACT_NONE, no accumulate, dense x).  tune=False: never time candidates
    from this call (the sampling path), whatever set_autotune says."""
    if _table.autotune and tune and not g.tile:
        g = _table.tuned("dgrad", g, (act, int(accumulate)) + tiles.ep_key(g, ep, x.dtype == torch.bfloat16), _measure("dgrad", g, y, w, bias, x, ep, act, accumulate))
    if ep is not None and (must_fuse or _with_override(g).tile < 1000):
        assert act == ACT_NONE and not accumulate
        _launch("dgrad", _dgrad_ex, g, y, w, bias, x, ep)
        return True
    _launch("dgrad", _dgrad, g, y, w, bias, x, act, accumulate)
    return False


def conv_dgrad_relu(g, y, w, bias, x):
    """x = max(conv_transpose(y, w) + bias, 0): the sampling path's deconvolution with test-mode BatchNorm folded into w and bias
    (bn_fold_deconv) and ReLU in the store; x fp32 or bf16.  Takes the tile the table holds for the PLAIN launch of this geometry
    and output type with its split-K part dropped (code % 1000: partial tiles cannot carry an activation), else the library's
    heuristic; the tuner is never run from here."""
    if not g.tile:
        code = table_tile("dgrad", g, (ACT_NONE, 0) + tiles.ep_key(g, None, x.dtype == torch.bfloat16)) % 1000
        if code:
            g = ConvGeom.from_buffer_copy(g)
            g.tile = code
    _launch("dgrad", _dgrad, g, y, w, bias, x, ACT_RELU, False)


def conv_wgrad(g, x, y, dw):
    if _table.autotune and not g.tile:
        g = _table.tuned("wgrad", g, (), _measure("wgrad", g, x, y))
    _launch("wgrad", _wgrad, g, x, y, dw)


def fc_fprop(M, K, Co, x, w, bias, y):
    _check(load().mcg_fc_fprop(M, K, Co, _p(_dense(x)), _p(_dense(w)), _p(bias), _p(_dense(y)), _stream()), "mcg_fc_fprop")


def fc_dgrad(M, K, Co, y, w, bias, bias_period, x):
    _check(load().mcg_fc_dgrad(M, K, Co, _p(_dense(y)), _p(_dense(w)), _p(bias), bias_period, _p(_dense(x)), _stream()), "mcg_fc_dgrad")


def fc_wgrad(M, K, Co, x, y, dw, db=None):
    _check(load().mcg_fc_wgrad(M, K, Co, _p(_dense(x)), _p(_dense(y)), _p(_dense(dw)), _p(db), _stream()), "mcg_fc_wgrad")


def bn_workspace_floats(C_max):
    return int(load().mcg_bn_workspace_bytes(0, C_max)) // 4


def bn_sums(M, Cn, y, sums, ws):
    """sums (float64)[2 Cn] = [sum y | sum y^2] over the M rows this rank holds (first half of synchronised BatchNorm's forward)"""
    _check(load().mcg_bn_sums(M, Cn, _p(_dense(y)), _p(sums, torch.float64), _p(ws), _stream()), "mcg_bn_sums")


def bn_stats_from_sums(M_total, Cn, sums, gamma, beta, stats, avg_mean, avg_var, eps=2e-5, decay=0.9):
    """bn_stats' outputs from the sums of the M_total rows of the global batch (bn_sums of every rank, added)"""
    _check(load().mcg_bn_stats_from_sums(M_total, Cn, _p(sums, torch.float64), _p(gamma), _p(beta), _p(stats), _p(avg_mean),
                                         _p(avg_var), eps, decay, _stream()), "mcg_bn_stats_from_sums")


def bn_stats(M, Cn, y, gamma, beta, stats, avg_mean, avg_var, ws, eps=2e-5, decay=0.9, sync=None):
    """sync: None, or an object with .world and .all_reduce_sum(tensor) (step.GradExchange): the statistics are then
    those of the global batch (every rank holds M rows)."""
    if sync is None or sync.world == 1:
        _check(load().mcg_bn_stats(M, Cn, _p(_dense(y)), _p(gamma), _p(beta), _p(stats), _p(avg_mean), _p(avg_var),
                                   eps, decay, _p(ws), _stream()), "mcg_bn_stats")
        return
    sums = torch.empty(2 * Cn, dtype=torch.float64, device=y.device)
    bn_sums(M, Cn, y, sums, ws)
    sync.all_reduce_sum(sums)
    bn_stats_from_sums(M * sync.world, Cn, sums, gamma, beta, stats, avg_mean, avg_var, eps, decay)


def _pout(out, split_out):
    """(pointer, MCG_IO_OUT_* flag) of an element-wise output: fp32, bf16, or (split_out) the split layout of PREC_SPLIT"""
    if split_out:
        global split_only_outputs
        split_only_outputs += 1
        return _p(_dense(out), torch.bfloat16), IO_OUT_SPLIT
    op, o16 = _pany(_dense(out))
    return op, IO_OUT_BF16 * o16


def bn_act_fwd(M, Cn, y, scale_shift, act, out, addend=None, sigma=0.0, seed=0, stream_id=0, c_valid=None,
               rows_per_item=0, item_stride=0, split_out=False):
    """y dense [M][Cn], or (rows_per_item > 0) a view whose items are item_stride elements apart.
    split_out: `out` is [M][4 Cn] bf16 and receives the split layout (split_planes' form) instead of fp32 values."""
    if rows_per_item == 0:
        _dense(y)
    op, oflag = _pout(out, split_out)
    yp, y16 = _pany(y)
    _check(load().mcg_bn_act_fwd(M, Cn, Cn if c_valid is None else c_valid, yp, rows_per_item, item_stride, _p(scale_shift), act,
                                 _p(_dense(addend)), sigma, seed, stream_id, op, oflag + IO_Y_BF16 * y16, _stream()),
           "mcg_bn_act_fwd")


def bn_bwd_sums(M, Cn, g_out, y, stats, act, sums, ws):
    """sums (float64)[2 Cn] = [sum g' | sum g' x_hat] over this rank's M rows, g' = g_out * act'(y * scale + shift); g_out and y
    fp32 or bf16 (first half of synchronised BatchNorm's backward)"""
    ip, i16 = _pany(_dense(g_out))
    yp, y16 = _pany(_dense(y))
    _check(load().mcg_bn_bwd_sums(M, Cn, ip, yp, _p(stats), act, IO_Y_BF16 * y16 + IO_G_BF16 * i16, _p(sums, torch.float64), _p(ws),
                                  _stream()), "mcg_bn_bwd_sums")


def bn_act_bwd_from_sums(M, M_total, Cn, g_out, y, stats, gamma, act, local_sums, global_sums, gx, dgamma, dbeta, ws):
    """bn_act_bwd's second half: gx of this rank's M rows from the sums of the M_total rows of the global batch; dgamma / dbeta
    accumulate this rank's own sums (the gradient exchange adds the ranks')"""
    gp, g16 = _pany(_dense(gx))
    ip, i16 = _pany(_dense(g_out))
    yp, y16 = _pany(_dense(y))
    _check(load().mcg_bn_act_bwd_from_sums(M, M_total, Cn, ip, yp, _p(stats), _p(gamma), act, _p(local_sums, torch.float64),
                                           _p(global_sums, torch.float64), gp, IO_OUT_BF16 * g16 + IO_Y_BF16 * y16 + IO_G_BF16 * i16,
                                           _p(dgamma), _p(dbeta), _p(ws), _stream()), "mcg_bn_act_bwd_from_sums")


def bn_act_bwd(M, Cn, g_out, y, stats, gamma, act, gx, dgamma, dbeta, ws, sync=None, split_out=False):
    if sync is None or sync.world == 1 or stats is None:
        gp, gflag = _pout(gx, split_out)
        ip, i16 = _pany(_dense(g_out))
        yp, y16 = _pany(_dense(y))
        _check(load().mcg_bn_act_bwd(M, Cn, ip, yp, _p(stats), _p(gamma), act, gp, gflag + IO_Y_BF16 * y16 + IO_G_BF16 * i16,
                                     _p(dgamma), _p(dbeta), _p(ws), _stream()), "mcg_bn_act_bwd")
        return
    assert not split_out
    local = torch.empty(2 * Cn, dtype=torch.float64, device=y.device)
    bn_bwd_sums(M, Cn, g_out, y, stats, act, local, ws)
    glob = local.clone()
    sync.all_reduce_sum(glob)
    bn_act_bwd_from_sums(M, M * sync.world, Cn, g_out, y, stats, gamma, act, local, glob, gx, dgamma, dbeta, ws)


def bn_stats_from_partials(M, Cn, part, n_slots, slot_stride, gamma, beta, stats, avg_mean, avg_var, ws, eps=2e-5, decay=0.9):
    """part: the (group's) partial sums a fused conv epilogue wrote (SUMS_STATS)."""
    _check(load().mcg_bn_stats_from_partials(M, Cn, _p(part), n_slots, slot_stride, _p(gamma), _p(beta), _p(stats), _p(avg_mean),
                                             _p(avg_var), eps, decay, _p(ws), _stream()), "mcg_bn_stats_from_partials")


def bn_act_bwd_from_partials(M, Cn, g_out, y, stats, gamma, act, part, n_slots, slot_stride, gx, dgamma, dbeta, ws, split_out=False):
    gp, gflag = _pout(gx, split_out)
    ip, i16 = _pany(_dense(g_out))
    yp, y16 = _pany(_dense(y))
    _check(load().mcg_bn_act_bwd_from_partials(M, Cn, ip, yp, _p(stats), _p(gamma), act, _p(part), n_slots, slot_stride, gp,
                                               gflag + IO_Y_BF16 * y16 + IO_G_BF16 * i16, _p(dgamma), _p(dbeta), _p(ws),
                                               _stream()), "mcg_bn_act_bwd_from_partials")


def colsum_from_partials(Cn, part, n_slots, slot_stride, db, ws):
    _check(load().mcg_colsum_from_partials(Cn, _p(part), n_slots, slot_stride, _p(db), _p(ws), _stream()), "mcg_colsum_from_partials")


def randn_rowquad(out, Cn, sigma, seed, stream_id):
    """out [M][Cn] in the element order of the fused first-layer epilogue"""
    _check(load().mcg_randn_rowquad(out.numel() // Cn, Cn, sigma, seed, stream_id, _p(_dense(out)), _stream()), "mcg_randn_rowquad")


def colsum_acc(M, Cn, g, db, ws):
    _check(load().mcg_colsum_acc(M, Cn, _p(_dense(g)), _p(db), _p(ws), _stream()), "mcg_colsum_acc")


def pack_clip(N, Cn, Cp, T, HW, x, out, addend=None, sigma=0.0, seed=0, stream_id=0, stride_n=None, stride_c=None):
    """x: reference-layout (N,C,T,H,W) tensor, or a frame view of one with explicit strides."""
    if stride_n is None and stride_c is None:
        _dense(x)                                          # (default strides are those of a dense tensor: a permuted view would be misread)
    stride_n = Cn * T * HW if stride_n is None else stride_n
    stride_c = T * HW if stride_c is None else stride_c
    _check(load().mcg_pack_clip(N, Cn, Cp, T, HW, _p(x), stride_n, stride_c, _p(_dense(addend)), sigma, seed, stream_id,
                                _p(_dense(out)), _stream()), "mcg_pack_clip")


def pack_clip_u8(N, Cn, Cp, T, HW, x, out, addend=None, sigma=0.0, seed=0, stream_id=0, stride_n=None, stride_t=None):
    """x: the loader's uint8 clips (N,T,H,W,C), or frame x[:, t] of them (T = 1, the clip's stride_n): -> (x - 128) / 128 in the
    device layout [N][T][HW][Cp] (+ noise as pack_clip)."""
    if stride_n is None and stride_t is None:
        _dense(x)
    stride_t = HW * Cn if stride_t is None else stride_t
    stride_n = T * stride_t if stride_n is None else stride_n
    _check(load().mcg_pack_clip_u8(N, Cn, Cp, T, HW, _p(x, torch.uint8), stride_n, stride_t, _p(_dense(addend)), sigma, seed, stream_id,
                                   _p(_dense(out)), _stream()), "mcg_pack_clip_u8")


def clip_to_u8(N, Cn, Cp, T, HW, inp, out, bias=None, act=ACT_NONE, stride_n=None, stride_t=None):
    """inp [N][T][HW][Cp] fp32 -> uint8 out[n * stride_n + t * stride_t + hw * Cn + c] = ((x / 2 + 0.5) * 255) truncated
    (generate_samples.py:39); default strides: dense (N,T,H,W,C).  act = ACT_TANH: inp is the pre-activation, x = tanh(inp + bias)."""
    stride_t = HW * Cn if stride_t is None else stride_t
    stride_n = T * stride_t if stride_n is None else stride_n
    need = (N - 1) * stride_n + (T - 1) * stride_t + HW * Cn
    if out.numel() < need or inp.numel() < N * T * HW * Cp or (bias is not None and bias.numel() < Cp):
        raise McgError("clip_to_u8: a tensor is smaller than the extents passed")
    _check(load().mcg_clip_to_u8(N, Cn, Cp, T, HW, _p(_dense(inp)), _p(bias), act, _p(_dense(out), torch.uint8), stride_n, stride_t,
                                 _stream()), "mcg_clip_to_u8")


def bn_fold_deconv(w, bias, c, gamma, beta, avg_mean, avg_var, w_out, bias_out, eps=2e-5):
    """w [..][Cp] (device-layout deconvolution filter, innermost axis = its output channels), bias [Cp] -> the filter and bias with
    test-mode BatchNorm (the running averages) folded in: mcg_bn_fold_deconv."""
    cp = w.shape[-1]
    for t, n in ((gamma, c), (beta, c), (avg_mean, c), (avg_var, c), (bias_out, cp), (w_out, w.numel())):
        if t.numel() < n:
            raise McgError("bn_fold_deconv: a tensor is smaller than the extents passed")
    if bias is not None and bias.numel() < cp:
        raise McgError("bn_fold_deconv: bias shorter than the padded channel count")
    _check(load().mcg_bn_fold_deconv(w.numel() // cp, c, cp, _p(_dense(w)), _p(bias), _p(gamma), _p(beta), _p(avg_mean), _p(avg_var),
                                     eps, _p(_dense(w_out)), _p(bias_out), _stream()), "mcg_bn_fold_deconv")


def concat_label_planes(x, c, dl, labels, out):
    """x [N][..][Cp] -> out [N][..][Cq]: the first c channels, dl label planes (+1 / -1), zero padding (model/updater.py:65-76);
    dl = 0: a channel slice into another row width."""
    N = x.shape[0]
    P = x[0].numel() // x.shape[-1]
    assert out.shape[:-1] == x.shape[:-1]
    _check(load().mcg_concat_label_planes(N, P, c, x.shape[-1], dl, out.shape[-1], _p(_dense(x)), _p(labels, torch.int32) if dl else None,
                                          _p(_dense(out)), _stream()), "mcg_concat_label_planes")
    return out


def unpack_clip(N, Cn, Cp, T, HW, inp, x):
    _check(load().mcg_unpack_clip(N, Cn, Cp, T, HW, _p(_dense(inp)), _p(_dense(x)), _stream()), "mcg_unpack_clip")


def tanh_bwd_to_frames(N, T, frame_elems, g_clip, x_clip, g_frames):
    _check(load().mcg_tanh_bwd_to_frames(N, T, frame_elems, _p(_dense(g_clip)), _p(_dense(x_clip)), _p(_dense(g_frames)),
                                         _stream()), "mcg_tanh_bwd_to_frames")


def gru_seq_fwd(N, T, dz, dl, dc, params, h0, e, labels, zc, z, saved):
    _check(load().mcg_gru_seq_fwd(N, T, dz, dl, dc, _p(params), _p(_dense(h0)), _p(_dense(e)), _p(labels, torch.int32),
                                  _p(_dense(zc)), _p(_dense(z)), _p(_dense(saved)), _stream()), "mcg_gru_seq_fwd")


def gru_seq_bwd(N, T, dz, dl, dc, params, e, labels, saved, gz, dparams):
    _check(load().mcg_gru_seq_bwd(N, T, dz, dl, dc, _p(params), _p(_dense(e)), _p(labels, torch.int32), _p(_dense(saved)),
                                  _p(_dense(gz)), _p(dparams), _stream()), "mcg_gru_seq_bwd")


def loss_dis(N, Cn, y_real, y_fake, t_real, t_fake, with_ce, loss_out, g_real, g_fake):
    _check(load().mcg_loss_dis(N, Cn, _p(_dense(y_real)), _p(_dense(y_fake)), _p(t_real, torch.int32), _p(t_fake, torch.int32),
                               int(with_ce), _p(loss_out), _p(_dense(g_real)), _p(_dense(g_fake)), _stream()), "mcg_loss_dis")


def loss_gen(N, Cn, y_i, y_v, t_fake, with_ce, loss_out, g_i, g_v):
    _check(load().mcg_loss_gen(N, Cn, _p(_dense(y_i)), _p(_dense(y_v)), _p(t_fake, torch.int32), int(with_ce), _p(loss_out),
                               _p(_dense(g_i)), _p(_dense(g_v)), _stream()), "mcg_loss_gen")


def adam_wd(p, g, m, v, lr_t, beta1, beta2, eps, wd, grad_scale=1.0, p16=None):
    """p16: optional bf16 buffer of p's size that receives a copy of the updated parameters"""
    _check(load().mcg_adam_wd(p.numel(), _p(_dense(p)), _p(_dense(g)), _p(_dense(m)), _p(_dense(v)), lr_t, beta1, beta2, eps, wd,
                              grad_scale, _p(_dense(p16), torch.bfloat16), _stream()), "mcg_adam_wd")


def adam_wd_ema(p, g, m, v, lr_t, beta1, beta2, eps, wd, ema, ema_rate, grad_scale=1.0, p16=None):
    """adam_wd, and in the same launch ema <- ema + ema_rate * (p - ema) with the parameter just written (ema_rate == 1: ema = p)"""
    for name, t in (('g', g), ('m', m), ('v', v), ('ema', ema), ('p16', p16)):
        if t is not None and t.numel() != p.numel():
            raise McgError("%s has %d elements, p has %d" % (name, t.numel(), p.numel()))
    _check(load().mcg_adam_wd_ema(p.numel(), _p(_dense(p)), _p(_dense(g)), _p(_dense(m)), _p(_dense(v)), lr_t, beta1, beta2, eps, wd,
                                  grad_scale, _p(_dense(p16), torch.bfloat16), _p(_dense(ema)), ema_rate, _stream()), "mcg_adam_wd_ema")


class EmaSeg(C.Structure):                                         # mcg_ema_seg
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("n", C.c_int64)]


def ema_multi(pairs, rate):
    """pairs: [(fp32 source tensor, fp32 average of the same size), ...], at most 32 -- dst <- dst + rate * (src - dst) for every
    pair in ONE launch (the generator's running statistics right after its Adam update)"""
    segs = (EmaSeg * len(pairs))()
    for q, (src, dst) in zip(segs, pairs):
        if src.numel() != dst.numel():
            raise McgError("an average and its source differ in size")
        _p(_dense(src)), _p(_dense(dst))                           # (device, dtype and density are checked here)
        q.src, q.dst, q.n = src.data_ptr(), dst.data_ptr(), src.numel()
    _check(load().mcg_ema_multi(len(pairs), C.cast(segs, C.c_void_p), rate, _stream()), "mcg_ema_multi")


class StatSeg(C.Structure):                                        # mcg_stat_seg
    _fields_ = [("offset", C.c_int64), ("n", C.c_int64)]


STAT_COLS, CTL_FLOATS, MAX_STAT_SEGS = 4, 8, 32                    # a stats row; the control block; segments of one call


def grad_stats_span():
    """the elements of a segment one block of mcg_grad_stats covers per loop trip (tests sit on its edges)"""
    return int(load().mcg_grad_stats_span())


def stat_segs(items):
    """[(offset, n), ...] in elements of the flat gradient -> the host array mcg_grad_stats reads (built once, reused every call)"""
    segs = (StatSeg * len(items))()
    for q, (off, n) in zip(segs, items):
        q.offset, q.n = int(off), int(n)
    return segs


def grad_stats_workspace(nseg, device):
    """the partial-sum workspace of grad_stats for up to nseg segments (float64)"""
    return torch.empty(max(int(load().mcg_grad_stats_workspace_bytes(nseg)) // 8, 1), dtype=torch.float64, device=device)


def grad_stats(segs, g, grad_scale, threshold, stats, ctl, ws):
    """segs: stat_segs(...) over the flat fp32 gradient g.  stats (float64)[(len(segs) + 1) * 4]: per segment and, last, in total
    {sum of squares, max |g|, non-finite count, 0}; ctl (float32)[8]: the control block adam_wd_ctl reads (include/mocogan_hip.h:
    mcg_grad_stats).  threshold: the L2 norm to clip to, math.inf for none.  Two launches on the current stream, no host sync."""
    nseg = len(segs)
    if stats.numel() < (nseg + 1) * STAT_COLS or ctl.numel() < CTL_FLOATS or ws.numel() * 8 < int(load().mcg_grad_stats_workspace_bytes(nseg)):
        raise McgError("grad_stats: stats, ctl or workspace too small for %d segments" % nseg)
    _check(load().mcg_grad_stats(nseg, C.cast(segs, C.c_void_p), _p(_dense(g)), grad_scale, threshold, _p(_dense(stats), torch.float64),
                                 _p(_dense(ctl)), _p(ws, torch.float64), _stream()), "mcg_grad_stats")


def adam_wd_ctl(p, g, m, v, lr_t, beta1, beta2, eps, wd, ctl, ema=None, ema_rate=0.0, p16=None):
    """adam_wd / adam_wd_ema (ema given) with the gradient scale read from ctl[0] on the device; nothing is written when
    ctl[1] != 0 (grad_stats found a non-finite gradient)"""
    for name, t in (('g', g), ('m', m), ('v', v), ('ema', ema), ('p16', p16)):
        if t is not None and t.numel() != p.numel():
            raise McgError("%s has %d elements, p has %d" % (name, t.numel(), p.numel()))
    if ctl.numel() < CTL_FLOATS:
        raise McgError("ctl holds %d floats, %d are needed" % (ctl.numel(), CTL_FLOATS))
    _check(load().mcg_adam_wd_ctl(p.numel(), _p(_dense(p)), _p(_dense(g)), _p(_dense(m)), _p(_dense(v)), lr_t, beta1, beta2, eps, wd,
                                  _p(_dense(ctl)), _p(_dense(p16), torch.bfloat16), _p(_dense(ema)), ema_rate, _stream()), "mcg_adam_wd_ctl")


def randint(out, modulus, seed, stream_id):
    """out (int32)[i] = Philox word i of the stream, modulo `modulus` (oracle.philox.randint states the same draw)"""
    _check(load().mcg_randint(out.numel(), int(modulus), seed, stream_id, _p(_dense(out), torch.int32), _stream()), "mcg_randint")


class SplitSeg(C.Structure):                                       # mcg_split_seg
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("n", C.c_int64), ("run", C.c_int64)]


split_multi_launches = 0                                       # (tests assert that the one-launch refresh really ran)


def split_planes_multi(items):
    """items: [(fp32 source tensor, run, bf16 destination tensor of 4x the elements), ...] -- mcg_split_planes of every item in ONE
    launch (an 'f32x3' network's filters right after its Adam update).  The split operands count as GEMM time in bench.py's
    roofline leg, as split_planes' do."""
    global split_multi_launches
    split_multi_launches += 1
    segs = (SplitSeg * len(items))()
    for q, (src, run, dst) in zip(segs, items):
        assert src.is_contiguous() and dst.is_contiguous() and dst.dtype == torch.bfloat16 and dst.numel() == 4 * src.numel()
        q.src, q.dst, q.n, q.run = src.data_ptr(), dst.data_ptr(), src.numel(), int(run)
    _timed(lambda: _check(load().mcg_split_planes_multi(len(items), C.cast(segs, C.c_void_p), _stream()), "mcg_split_planes_multi"),
           _tag + ".split")


def split_planes(src, run=16, out=None):
    """fp32 tensor -> its MCG_PREC_SPLIT form (include/mocogan_hip.h: mcg_split_planes): per run of `run` values four runs of
    bf16 (hi, mid, lo, padding).  run = 16: channels-last tensors (last dimension a multiple of 16) -> last dimension x 4."""
    src = _dense(src)
    n = src.numel()
    if out is None:
        out = torch.empty(src.shape[:-1] + (4 * src.shape[-1],), device=src.device, dtype=torch.bfloat16)
    assert out.numel() == 4 * n and out.dtype == torch.bfloat16
    _timed(lambda: _check(load().mcg_split_planes(n, int(run), _p(src), _p(out, torch.bfloat16), _stream()), "mcg_split_planes"),
           _tag + ".split")                                      # (bench.py's roofline leg charges the pass to the network's GEMMs)
    return out


def randn(out, sigma, seed, stream_id):
    _check(load().mcg_randn(out.numel(), sigma, seed, stream_id, _p(_dense(out)), _stream()), "mcg_randn")


# ---- differentiable augmentation of the discriminators' inputs (include/mocogan_hip.h: mcg_augment_*) ----------------------------
AUG_COLOR, AUG_TRANSLATION, AUG_CUTOUT = 1, 2, 4
AUG_NAMES = {'color': AUG_COLOR, 'translation': AUG_TRANSLATION, 'cutout': AUG_CUTOUT}


def _parse_policy(policy, names, top, noun, a_noun):
    """a comma-separated string of `names` (any subset, any order), a mask in 0..top, or None / '' / 0 (off) -> the mask (0 = off)"""
    if policy is None:
        return 0
    if isinstance(policy, bool) or not isinstance(policy, (int, str)):
        raise ValueError('%s policy is a string of names or a mask, got %r' % (a_noun, policy))
    if isinstance(policy, int):
        if not 0 <= policy <= top:
            raise ValueError('%s mask lies in 0..%d, got %r' % (a_noun, top, policy))
        return policy
    mask = 0
    for name in policy.split(','):
        name = name.strip()
        if not name:
            continue
        if name not in names:
            raise ValueError('unknown %s %r (known: %s)' % (noun, name, ', '.join(sorted(names))))
        mask |= names[name]
    return mask


def parse_augment(policy):
    """'color,translation,cutout' (any subset, any order), a mask of AUG_* flags, or None / '' / 0 (off) -> the mask (0 = off)"""
    return _parse_policy(policy, AUG_NAMES, 7, 'augmentation', 'an augmentation')


def augment_workspace(n, device):
    """the caller-owned scratch of augment_fwd / augment_bwd on n clips (mcg_augment_workspace_bytes)"""
    return torch.empty(load().mcg_augment_workspace_bytes(n) // 8, dtype=torch.float64, device=device)


def augment_draw(n, H, W, policy, seed, stream_id, geo=None, col=None, device=None):
    """the parameters of n clips from Philox stream (seed, stream_id): geo int32 [n][8], col float [n][4]"""
    if geo is None:
        geo = torch.empty((n, 8), dtype=torch.int32, device=device)
        col = torch.empty((n, 4), dtype=torch.float32, device=device)
    if geo.numel() < 8 * n or col.numel() < 4 * n:
        raise McgError("augment_draw: a parameter tensor is smaller than the clip count")
    _check(load().mcg_augment_draw(n, H, W, policy, seed, stream_id, _p(_dense(geo), torch.int32), _p(_dense(col)), _stream()),
           "mcg_augment_draw")
    return geo, col


ADA_DOUBLES = 8                                                    # the state block of the adaptive augmentation (mcg_ada_update)
ADA_P, ADA_SUM_V, ADA_SUM_I, ADA_COUNT, ADA_CALLS, ADA_RT_V, ADA_RT_I, ADA_ADJUSTMENTS = range(8)


def ada_state(p, device):
    """a fresh state block: probability p, every counter zero"""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError('the augmentation probability lies in [0, 1], got %r' % (p,))
    return torch.tensor([p] + [0.0] * (ADA_DOUBLES - 1), dtype=torch.float64, device=device)


def _ada_block(ada, name):
    if ada.dtype != torch.float64 or ada.numel() < ADA_DOUBLES:
        raise McgError("%s: the state block is %d doubles" % (name, ADA_DOUBLES))
    return _p(_dense(ada), torch.float64)


def augment_draw_gated(n, H, W, policy, seed, stream_id, gate_stream_id, ada, geo=None, col=None, device=None):
    """augment_draw with every component of the policy kept with probability ada[0] (device memory; gates from Philox stream
    (seed, gate_stream_id)); geo[:, 6] holds the flags that were applied"""
    if geo is None:
        geo = torch.empty((n, 8), dtype=torch.int32, device=device)
        col = torch.empty((n, 4), dtype=torch.float32, device=device)
    if geo.numel() < 8 * n or col.numel() < 4 * n:
        raise McgError("augment_draw_gated: a parameter tensor is smaller than the clip count")
    _check(load().mcg_augment_draw_gated(n, H, W, policy, seed, stream_id, gate_stream_id, _ada_block(ada, "augment_draw_gated"),
                                         _p(_dense(geo), torch.int32), _p(_dense(col)), _stream()), "mcg_augment_draw_gated")
    return geo, col


def ada_update(y_video, y_image, target, step, interval, ada):
    """one step of the controller on the real clips' logits [n][c] (column 0 is read); one launch on the current stream"""
    n, c = y_video.shape
    if tuple(y_image.shape) != (n, c):
        raise McgError("ada_update: the two discriminators' logits differ in shape")
    _check(load().mcg_ada_update(n, c, _p(_dense(y_video)), _p(_dense(y_image)), target, step, interval, _ada_block(ada, "ada_update"),
                                 _stream()), "mcg_ada_update")
    return ada


def _augment(fn, name, x, c, geo, col, ws, out):
    n, T, H, W, cp = x.shape
    if out.shape != x.shape or geo.numel() < 8 * n or col.numel() < 4 * n or ws.numel() * ws.element_size() < load().mcg_augment_workspace_bytes(n):
        raise McgError("%s: a tensor is smaller than the extents passed" % name)
    _check(fn(n, c, cp, T, H, W, _p(_dense(x)), _p(_dense(geo), torch.int32), _p(_dense(col)), _p(ws, ws.dtype), _p(_dense(out)), _stream()), name)
    return out


def augment_fwd(x, c, geo, col, ws, out):
    """x [n][T][H][W][4] with c valid channels -> out, the augmented clips (parameters geo / col, one set per clip)"""
    return _augment(load().mcg_augment_fwd, "mcg_augment_fwd", x, c, geo, col, ws, out)


def augment_bwd(g_out, c, geo, col, ws, g_in):
    """the adjoint of augment_fwd's linear part: gradient w.r.t. the augmented clips -> gradient w.r.t. the clips"""
    return _augment(load().mcg_augment_bwd, "mcg_augment_bwd", g_out, c, geo, col, ws, g_in)


# ---- geometric augmentation: a per-clip affine warp (include/mocogan_hip.h: mcg_warp_*) -----------------------------------------
WARP_FLIP, WARP_ROT90, WARP_SCALE, WARP_ROTATE = 1, 2, 4, 8
WARP_NAMES = {'flip': WARP_FLIP, 'rot90': WARP_ROT90, 'scale': WARP_SCALE, 'rotate': WARP_ROTATE}


def parse_warp(policy):
    """'flip,rot90,scale,rotate' (any subset, any order), a mask of WARP_* flags, or None / '' / 0 (off) -> the mask (0 = off)"""
    return _parse_policy(policy, WARP_NAMES, 15, 'warp', 'a warp')


def _warp_mat(n, mat, device, name):
    if mat is None:
        mat = torch.empty((n, 8), dtype=torch.float32, device=device)
    if mat.numel() < 8 * n:
        raise McgError("%s: the matrix tensor is smaller than the clip count" % name)
    return mat


def warp_draw(n, H, W, policy, seed, stream_id, mat=None, device=None):
    """the matrices of n clips from Philox stream (seed, stream_id): float [n][8] = m00 m01 m02 m10 m11 m12 flags 0"""
    mat = _warp_mat(n, mat, device, "warp_draw")
    _check(load().mcg_warp_draw(n, H, W, policy, seed, stream_id, _p(_dense(mat)), _stream()), "mcg_warp_draw")
    return mat


def warp_draw_gated(n, H, W, policy, seed, stream_id, gate_stream_id, ada, mat=None, device=None):
    """warp_draw with every component of the policy kept with probability ada[0] (device memory; gates from Philox stream
    (seed, gate_stream_id)); mat[:, 6] holds the flags that were applied"""
    mat = _warp_mat(n, mat, device, "warp_draw_gated")
    _check(load().mcg_warp_draw_gated(n, H, W, policy, seed, stream_id, gate_stream_id, _ada_block(ada, "warp_draw_gated"),
                                      _p(_dense(mat)), _stream()), "mcg_warp_draw_gated")
    return mat


def _warp(fn, name, x, c, mat, out):
    n, T, H, W, cp = x.shape
    if out.shape != x.shape or mat.numel() < 8 * n:
        raise McgError("%s: a tensor is smaller than the extents passed" % name)
    _check(fn(n, c, cp, T, H, W, _p(_dense(x)), _p(_dense(mat)), _p(_dense(out)), _stream()), name)
    return out


def warp_fwd(x, c, mat, out):
    """x [n][T][H][W][4] -> out, every clip warped by its matrix (mat [n][8], output position -> source; bilinear, zero padding)"""
    return _warp(load().mcg_warp_fwd, "mcg_warp_fwd", x, c, mat, out)


def warp_bwd(g_out, c, mat, g_in):
    """the adjoint of warp_fwd: gradient w.r.t. the warped clips -> gradient w.r.t. the clips (a gather: bit-reproducible)"""
    return _warp(load().mcg_warp_bwd, "mcg_warp_bwd", g_out, c, mat, g_in)


# ---- sliced Wasserstein distance (include/mocogan_hip.h: mcg_swd_*, mcg_sort_rows; composed by metrics.py) -------------------------
SWD_LEVELS = (64, 32, 16)                                          # frame sizes of the pyramid levels l64, l32, l16


def sort_local_span():
    """the row length up to which mcg_sort_rows needs one launch and no workspace (mcg_sort_local_span)"""
    return int(load().mcg_sort_local_span())


def swd_workspace(n, d, rows, device):
    """the caller-owned scratch of every swd_* stage on n x d descriptor matrices and `rows` sorted rows (mcg_swd_workspace_bytes)"""
    nbytes = load().mcg_swd_workspace_bytes(n, d, rows)
    if nbytes <= 0:
        raise McgError("swd_workspace: bad sizes n=%r d=%r rows=%r" % (n, d, rows))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def _ws_ok(ws, n, d, rows):
    return ws.numel() * ws.element_size() >= load().mcg_swd_workspace_bytes(n, d, rows)


def swd_pyramid(clips):
    """uint8 clips (N,T,64,64,C) -> the levels (l64, l32, l16), fp32 [N][T][h][h][4] with zero pad channels"""
    if clips.dtype != torch.uint8 or clips.dim() != 5:
        raise McgError("swd_pyramid: uint8 clips (N,T,H,W,C), got %s %s" % (clips.dtype, tuple(clips.shape)))
    n, t, h, w, c = clips.shape
    levels = [torch.empty(n, t, s, s, 4, dtype=torch.float32, device=clips.device) for s in SWD_LEVELS]
    _check(load().mcg_swd_pyramid(n, c, t, h, w, _p(_dense(clips), torch.uint8), _p(levels[0]), _p(levels[1]), _p(levels[2]), _stream()),
           "mcg_swd_pyramid")
    return levels


def swd_gather(level, c, first_clip, patches, patch_frames, seed, stream_id, out):
    """the patches * N descriptor rows of the N clips of `level` ([N][T][h][h][4], c valid channels, global clip indices from
    first_clip) into out [N * patches][patch_frames * 49 * c] (a view of the set's matrix at row first_clip * patches)"""
    n, t, h = level.shape[0], level.shape[1], level.shape[2]
    d = patch_frames * 49 * c
    if level.dim() != 5 or level.shape[3] != h or level.shape[4] != 4 or out.numel() != n * patches * d:
        raise McgError("swd_gather: level %s / out %s do not fit" % (tuple(level.shape), tuple(out.shape)))
    _check(load().mcg_swd_gather(n, c, t, h, _p(_dense(level)), first_clip, patches, patch_frames, seed, stream_id, _p(_dense(out)), _stream()),
           "mcg_swd_gather")
    return out


def swd_channel_sums(desc, c, ws, sums=None):
    """[sum | sum of squares] per channel of desc [n][D] as 2 * c doubles"""
    n, d = desc.shape
    sums = torch.empty(2 * c, dtype=torch.float64, device=desc.device) if sums is None else sums
    if sums.numel() < 2 * c or not _ws_ok(ws, n, d, 1):
        raise McgError("swd_channel_sums: sums or workspace too small")
    _check(load().mcg_swd_channel_sums(n, d, c, _p(_dense(desc)), _p(sums, torch.float64), _p(ws, torch.float64), _stream()), "mcg_swd_channel_sums")
    return sums


def swd_normalize(desc, c, sums):
    """desc <- (desc - mean_c) / std_c in place (a constant channel -> zeros)"""
    n, d = desc.shape
    _check(load().mcg_swd_normalize(n, d, c, _p(_dense(desc)), _p(sums, torch.float64), _stream()), "mcg_swd_normalize")
    return desc


def swd_unit_columns(dirs):
    """every column of dirs [D][K] to unit L2 norm, in place"""
    d, k = dirs.shape
    _check(load().mcg_swd_unit_columns(d, k, _p(_dense(dirs)), _stream()), "mcg_swd_unit_columns")
    return dirs


def swd_project(desc, dirs, out):
    """out [K][n_stride] (direction-major) = (desc [n][D] @ dirs [D][K])^T"""
    n, d = desc.shape
    k = dirs.shape[1]
    if dirs.shape[0] != d or out.dim() != 2 or out.shape[0] != k or out.shape[1] < n:
        raise McgError("swd_project: desc %s, dirs %s, out %s do not fit" % (tuple(desc.shape), tuple(dirs.shape), tuple(out.shape)))
    _check(load().mcg_swd_project(n, d, k, _p(_dense(desc)), _p(_dense(dirs)), _p(_dense(out)), out.shape[1], _stream()), "mcg_swd_project")
    return out


def sort_rows(data, n=None, ws=None):
    """sorts the first n (default: all) elements of every row of data [rows][row_stride] ascending, in place"""
    rows, stride = data.shape
    n = stride if n is None else n
    if n > sort_local_span() and (ws is None or not _ws_ok(ws, n, 1, rows)):
        raise McgError("sort_rows: rows of %d elements need a workspace (swd_workspace)" % n)
    _check(load().mcg_sort_rows(rows, n, _p(_dense(data)), stride, None if ws is None else _p(ws, torch.float64), _stream()), "mcg_sort_rows")
    return data


def swd_distance(a, b, n, ws, out):
    """out (one double) = mean |a - b| over the first n elements of every row of two sorted [K][stride] sets"""
    if a.shape[0] != b.shape[0] or not _ws_ok(ws, n, 1, 1):
        raise McgError("swd_distance: direction counts differ or workspace too small")
    _check(load().mcg_swd_distance(a.shape[0], n, n, _p(_dense(a)), a.shape[1], _p(_dense(b)), b.shape[1], _p(out, torch.float64),
                                   _p(ws, torch.float64), _stream()), "mcg_swd_distance")
    return out


# ---- nearest-neighbour metrics on the int8 matrix pipe (include/mocogan_hip.h: mcg_knn_*; composed by metrics.py) ------------------
KNN_POOLS = (2, 4, 8)
KNN_MAX_D, KNN_MAX_K = 32768, 16


def knn_descriptors(clips, pool, desc=None, norms=None):
    """uint8 clips (N,T,64,64,C) -> (desc [N][D] int8, norms [N] int32): box means over pool x pool, rounded half up, minus 128;
    D = T * (64 / pool)^2 * C.  desc / norms may be views of a set's matrices at the chunk's rows."""
    if clips.dtype != torch.uint8 or clips.dim() != 5:
        raise McgError("knn_descriptors: uint8 clips (N,T,H,W,C), got %s %s" % (clips.dtype, tuple(clips.shape)))
    n, t, h, w, c = clips.shape
    if pool not in KNN_POOLS:
        raise McgError("knn_descriptors: pool is one of %s, got %r" % (KNN_POOLS, pool))
    d = t * (h // pool) * (w // pool) * c
    desc = torch.empty(n, d, dtype=torch.int8, device=clips.device) if desc is None else desc
    norms = torch.empty(n, dtype=torch.int32, device=clips.device) if norms is None else norms
    if desc.numel() != n * d or norms.numel() != n:
        raise McgError("knn_descriptors: desc %s / norms %s do not fit %d x %d" % (tuple(desc.shape), tuple(norms.shape), n, d))
    _check(load().mcg_knn_descriptors(n, c, t, h, w, pool, _p(_dense(clips), torch.uint8), _p(_dense(desc), torch.int8),
                                      _p(_dense(norms), torch.int32), _stream()), "mcg_knn_descriptors")
    return desc, norms


def knn_sqdist(a, na, b, nb, out):
    """out [M][ld >= N] int32: out[i][j] = na[i] + nb[j] - 2 a[i].b[j] for int8 a [M][D], b [N][D] (exact); columns N.. untouched"""
    (m, d), n = a.shape, b.shape[0]
    if b.shape[1] != d or na.numel() != m or nb.numel() != n or out.dim() != 2 or out.shape[0] != m or out.shape[1] < n:
        raise McgError("knn_sqdist: a %s, b %s, out %s do not fit" % (tuple(a.shape), tuple(b.shape), tuple(out.shape)))
    _check(load().mcg_knn_sqdist(m, n, d, _p(_dense(a), torch.int8), _p(_dense(na), torch.int32), _p(_dense(b), torch.int8),
                                 _p(_dense(nb), torch.int32), _p(_dense(out), torch.int32), out.shape[1], _stream()), "mcg_knn_sqdist")
    return out


def knn_smallest(dist, k, n=None, exclude_self=False, self_col0=0, val=None, idx=None):
    """(val, idx) [M][k] int32: the k smallest of the first n (default: all) entries of every row of dist [M][ld] in ascending
    (value, column) order; with exclude_self row i skips column self_col0 + i; missing neighbours are (INT32_MAX, -1)"""
    m, ld = dist.shape
    n = ld if n is None else n
    val = torch.empty(m, k, dtype=torch.int32, device=dist.device) if val is None else val
    idx = torch.empty(m, k, dtype=torch.int32, device=dist.device) if idx is None else idx
    if val.numel() != m * k or idx.numel() != m * k:
        raise McgError("knn_smallest: val %s / idx %s do not fit %d x %d" % (tuple(val.shape), tuple(idx.shape), m, k))
    _check(load().mcg_knn_smallest(m, n, _p(_dense(dist), torch.int32), ld, k, int(bool(exclude_self)), self_col0,
                                   _p(_dense(val), torch.int32), _p(_dense(idx), torch.int32), _stream()), "mcg_knn_smallest")
    return val, idx


def knn_ball_counts(dist, radius, n=None, counts=None):
    """counts [M] int32: how many of the first n (default: all) entries j of row i of dist [M][ld] lie within radius[j]"""
    m, ld = dist.shape
    n = ld if n is None else n
    counts = torch.empty(m, dtype=torch.int32, device=dist.device) if counts is None else counts
    if radius.numel() < n or counts.numel() != m:
        raise McgError("knn_ball_counts: radius %s / counts %s do not fit %d x %d" % (tuple(radius.shape), tuple(counts.shape), m, n))
    _check(load().mcg_knn_ball_counts(m, n, _p(_dense(dist), torch.int32), ld, _p(_dense(radius), torch.int32),
                                      _p(_dense(counts), torch.int32), _stream()), "mcg_knn_ball_counts")
    return counts


# ---- motion and content metrics (include/mocogan_hip.h: mcg_mc_*; composed by metrics.py) -----------------------------------------
MC_MAX_T, MC_MAX_DF = 64, 3072


def _frames(desc, name):
    if desc.dim() != 3:
        raise McgError("%s: int8 per-frame descriptors (N,T,Df), got %s" % (name, tuple(desc.shape)))
    return desc.shape


def mc_frame_sqdist(desc, dist=None):
    """int8 desc (N,T,Df) -> dist [N][T][T] int32: the exact squared distances between the frames of every clip"""
    n, t, df = _frames(desc, "mc_frame_sqdist")
    dist = torch.empty(n, t, t, dtype=torch.int32, device=desc.device) if dist is None else dist
    if dist.numel() != n * t * t:
        raise McgError("mc_frame_sqdist: dist %s does not fit %d x %d x %d" % (tuple(dist.shape), n, t, t))
    _check(load().mcg_mc_frame_sqdist(n, t, df, _p(_dense(desc), torch.int8), _p(_dense(dist), torch.int32), _stream()), "mcg_mc_frame_sqdist")
    return dist


def mc_clip_stats(dist, pair_sum=None, lag_sum=None):
    """int32 dist (N,T,T) -> (pair_sum [N] float64: the sum over s < t of sqrt(dist[n][s][t]) in a fixed order, lag_sum [N][T] int64:
    the sums of the diagonals)"""
    if dist.dim() != 3 or dist.shape[1] != dist.shape[2]:
        raise McgError("mc_clip_stats: int32 dist (N,T,T), got %s" % (tuple(dist.shape),))
    n, t = dist.shape[:2]
    pair_sum = torch.empty(n, dtype=torch.float64, device=dist.device) if pair_sum is None else pair_sum
    lag_sum = torch.empty(n, t, dtype=torch.int64, device=dist.device) if lag_sum is None else lag_sum
    if pair_sum.numel() != n or lag_sum.numel() != n * t:
        raise McgError("mc_clip_stats: pair_sum %s / lag_sum %s do not fit %d x %d" % (tuple(pair_sum.shape), tuple(lag_sum.shape), n, t))
    _check(load().mcg_mc_clip_stats(n, t, _p(_dense(dist), torch.int32), _p(_dense(pair_sum), torch.float64), _p(_dense(lag_sum), torch.int64),
                                    _stream()), "mcg_mc_clip_stats")
    return pair_sum, lag_sum


def mc_motion_descriptors(desc, mdesc=None, mnorms=None):
    """int8 desc (N,T,Df) -> (mdesc [N][(T-1) Df] int8: the halved differences of consecutive frames (floor), mnorms [N] int32: the
    rows' sums of squares): operands of knn_sqdist.  mdesc / mnorms may be views of a set's matrices at the chunk's rows."""
    n, t, df = _frames(desc, "mc_motion_descriptors")
    d = (t - 1) * df
    mdesc = torch.empty(n, d, dtype=torch.int8, device=desc.device) if mdesc is None else mdesc
    mnorms = torch.empty(n, dtype=torch.int32, device=desc.device) if mnorms is None else mnorms
    if mdesc.numel() != n * d or mnorms.numel() != n:
        raise McgError("mc_motion_descriptors: mdesc %s / mnorms %s do not fit %d x %d" % (tuple(mdesc.shape), tuple(mnorms.shape), n, d))
    _check(load().mcg_mc_motion_descriptors(n, t, df, _p(_dense(desc), torch.int8), _p(_dense(mdesc), torch.int8),
                                            _p(_dense(mnorms), torch.int32), _stream()), "mcg_mc_motion_descriptors")
    return mdesc, mnorms
