"""NumPy statement of the adaptive augmentation (TEST INFRASTRUCTURE; include/mocogan_hip.h: mcg_augment_draw_gated and
mcg_ada_update are the specification): the gate in front of augment_ref.draw, and the controller of its probability in Python
floats and integers (a Python float is the kernel's double; the sign sums are integers on both sides)."""
import numpy as np

import augment_ref as ar
from oracle.philox import philox4x32_10

ADA_P, ADA_SUM_V, ADA_SUM_I, ADA_COUNT, ADA_CALLS, ADA_RT_V, ADA_RT_I, ADA_ADJUSTMENTS = range(8)
COMPONENTS = (ar.AUG_COLOR, ar.AUG_TRANSLATION, ar.AUG_CUTOUT)


def gate_units(n, seed, gate_sid):
    """u(g0), u(g1), u(g2) of clips 0..n-1 as float64 [n][3]: clip i takes Philox counter i of (seed, gate_sid)"""
    idx = np.arange(n, dtype=np.uint64)
    z = np.zeros(n, np.uint32)
    r = philox4x32_10((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                      z + np.uint32(gate_sid & 0xFFFFFFFF), z + np.uint32(gate_sid >> 32), seed & 0xFFFFFFFF, seed >> 32)
    g = np.stack(r[:3], axis=1).astype(np.int64)
    return (g >> 9).astype(np.float64) * 2.0 ** -23


def gated_draw(n, H, W, policy, seed, sid, gate_sid, p):
    """mcg_augment_draw_gated: (geo, col, mask) -- mask[i] = the flags that are in the policy and passed their gate; a component
    outside it has its identity values; geo[:, 6] = mask"""
    assert sid != gate_sid
    passed = gate_units(n, seed, gate_sid) < float(p)
    mask = np.zeros(n, np.int32)
    for k, flag in enumerate(COMPONENTS):
        if policy & flag:
            mask |= np.where(passed[:, k], flag, 0).astype(np.int32)
    full_geo, full_col = ar.draw(n, H, W, policy, seed, sid)
    geo, col = ar.identity_params(n)
    c, t, o = ((mask & f) != 0 for f in COMPONENTS)
    col[c, :3] = full_col[c, :3]
    geo[t, 0:2] = full_geo[t, 0:2]
    geo[o, 2:6] = full_geo[o, 2:6]
    geo[:, 6] = mask
    return geo, col, mask


def sign(y):
    """+1 for y > 0 (+inf too), -1 for y < 0 (-inf too), 0 for +-0 and NaN"""
    y = float(y)
    return (1 if y > 0.0 else 0) - (1 if y < 0.0 else 0)


def new_state(p=0.0):
    return [float(p)] + [0.0] * 7


def controller(state, logits_v, logits_i, target, step, interval):
    """mcg_ada_update: state (eight floats) and the real clips' logits (column 0 of [N][C], or [N]) -> the new state"""
    lv, li = (np.asarray(y, np.float32).reshape(len(y), -1)[:, 0] for y in (logits_v, logits_i))
    assert len(lv) == len(li) and len(lv) >= 1
    s = [float(v) for v in state]
    sum_v = s[ADA_SUM_V] + float(sum(sign(y) for y in lv))
    sum_i = s[ADA_SUM_I] + float(sum(sign(y) for y in li))
    count = s[ADA_COUNT] + float(len(lv))
    calls = s[ADA_CALLS] + 1.0
    if calls >= interval:
        r_v, r_i = sum_v / count, sum_i / count
        r = max(r_v, r_i)
        d = (1 if r > target else 0) - (1 if r < target else 0)
        p = min(1.0, max(0.0, s[ADA_P] + d * float(step)))
        return [p, 0.0, 0.0, 0.0, 0.0, r_v, r_i, s[ADA_ADJUSTMENTS] + 1.0]
    return [s[ADA_P], sum_v, sum_i, count, calls, s[ADA_RT_V], s[ADA_RT_I], s[ADA_ADJUSTMENTS]]


def stats(state):
    """TrainStep.ada_stats() of a state"""
    return {'p': float(state[ADA_P]), 'rt_video': float(state[ADA_RT_V]), 'rt_image': float(state[ADA_RT_I]),
            'adjustments': int(state[ADA_ADJUSTMENTS])}


def step_size(interval, n, kimg):
    return interval * n / (kimg * 1000.0)


def perf_mode_params(seed, it, rank, n, p, policy=ar.FULL, H=64, W=64):
    """the gated parameters iteration `it` of rank `rank` draws in perf mode at probability p (ids base + 40 /
    41 for the parameters, base + 42 / 43 for the gates) -- and the masks"""
    base = (it * 64 + rank + 1) * 64
    out, masks = {}, {}
    for which, sid in (('real', 40), ('fake', 41)):
        geo, col, mask = gated_draw(n, H, W, policy, seed, base + sid, base + sid + 2, p)
        out[which], masks[which] = (geo, col), mask
    return out, masks

