"""NumPy statement of the geometric augmentation (TEST INFRASTRUCTURE; include/mocogan_hip.h: mcg_warp_* is the specification): the
source coordinates and the Philox draw in float32 with the header's operation order (bit for bit what the kernels compute), the
bilinear weights and every sum in float64; the forward map as a gather, its adjoint as the SCATTER (the kernel gathers: it is
checked against the other statement); one training iteration with the warp, then the colour / translation / cutout augmentation of
tests/augment_ref.py, in front of both discriminators.  Clips are in the reference layout (N,C,T,H,W), valid channels only."""
import numpy as np

import augment_ref as ar
from oracle import net
from oracle import updater as oupd
from oracle.philox import philox4x32_10

WARP_FLIP, WARP_ROT90, WARP_SCALE, WARP_ROTATE = 1, 2, 4, 8
COMPONENTS = (WARP_FLIP, WARP_ROT90, WARP_SCALE, WARP_ROTATE)
FULL = 15
F32 = np.float32


def identity_mats(n):
    mat = np.zeros((n, 8), F32)
    mat[:, 0] = mat[:, 4] = 1.0
    return mat


def rotation(t):
    """c, sn of the draw's rotation at parameter t (float32, one rounding per operation)"""
    t = F32(t)
    tt = t * t
    den = F32(1) + tt
    return (F32(1) - tt) / den, (F32(2) * t) / den


# ---- source coordinates (float32, bit for bit) and taps -----------------------------------------------------------------------
def source(mat, H, W):
    """sx, sy [n][H][W] float32 of every output pixel: ((m00 xc) + (m01 yc)) + (cx + m02), each operation rounded on its own,
    clamped to [-2, extent + 1] (np.fmax drops a NaN, as fmaxf does)"""
    m = np.asarray(mat, F32)
    n = len(m)
    cx, cy = F32(W - 1) * F32(0.5), F32(H - 1) * F32(0.5)
    xc = (np.arange(W, dtype=F32) - cx).reshape(1, 1, W)
    yc = (np.arange(H, dtype=F32) - cy).reshape(1, H, 1)
    e = [m[:, k].reshape(n, 1, 1) for k in range(6)]
    with np.errstate(all='ignore'):
        sx = ((e[0] * xc) + (e[1] * yc)) + (cx + e[2])
        sy = ((e[3] * xc) + (e[4] * yc)) + (cy + e[5])
        assert sx.dtype == F32 and sy.dtype == F32
        sx = np.fmin(np.fmax(sx, F32(-2)), F32(W + 1))
        sy = np.fmin(np.fmax(sy, F32(-2)), F32(H + 1))
    return sx, sy


def taps(mat, H, W):
    """the four taps of every output pixel: a list of (yy, xx, w, inside) with integer positions [n][H][W], float64 weights and
    whether the tap lies inside the frame"""
    sx, sy = source(mat, H, W)
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0).astype(np.float64), (sy - y0).astype(np.float64)
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    out = []
    for j, wy in ((0, 1.0 - fy), (1, fy)):
        for i, wx in ((0, 1.0 - fx), (1, fx)):
            yy, xx = y0 + j, x0 + i
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            out.append((np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1), np.where(inside, wx * wy, 0.0), inside))
    return out


def forward(x, mat, with_terms=False):
    """out(t, y, x) = sum of the four taps' weights times the clip at the taps (zero outside the frame), float64.  with_terms: also
    S = the sum of |w| |value| over each element's terms (what a rounding bound scales with)"""
    x = np.asarray(x, np.float64)
    n, _, _, H, W = x.shape
    out = np.zeros((n, H, W) + x.shape[1:3])                          # [n][y][x][C][T]
    mag = np.zeros_like(out)
    rows = np.arange(n).reshape(-1, 1, 1)
    for yy, xx, w, _ in taps(mat, H, W):
        v = x[rows, :, :, yy, xx]
        out += w[..., None, None] * v
        mag += w[..., None, None] * np.abs(v)
    out, mag = (np.ascontiguousarray(a.transpose(0, 3, 4, 1, 2)) for a in (out, mag))
    return (out, mag) if with_terms else out


def adjoint(g, mat, with_terms=False):
    """the adjoint of forward as a scatter: every output pixel adds w g to its four taps"""
    g = np.asarray(g, np.float64)
    n, _, _, H, W = g.shape
    gt = g.transpose(0, 3, 4, 1, 2)                                    # [n][y][x][C][T]
    out = np.zeros(gt.shape)
    mag = np.zeros(gt.shape)
    for yy, xx, w, inside in taps(mat, H, W):
        nn, y, x = np.nonzero(inside & (w != 0.0))
        np.add.at(out, (nn, yy[nn, y, x], xx[nn, y, x]), w[nn, y, x, None, None] * gt[nn, y, x])
        np.add.at(mag, (nn, yy[nn, y, x], xx[nn, y, x]), w[nn, y, x, None, None] * np.abs(gt[nn, y, x]))
    out, mag = (np.ascontiguousarray(a.transpose(0, 3, 4, 1, 2)) for a in (out, mag))
    return (out, mag) if with_terms else out


# ---- the draws ----------------------------------------------------------------------------------------------------------------
def _words(n, seed, stream_id):
    idx = np.arange(n, dtype=np.uint64)
    z = np.zeros(n, np.uint32)
    r = philox4x32_10((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                      z + np.uint32(stream_id & 0xFFFFFFFF), z + np.uint32(stream_id >> 32), seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(r, axis=1).astype(np.int64)


def _unit(w):
    return (w >> 9).astype(F32) * F32(2.0 ** -23)


def components(n, policy, seed, stream_id):
    """f, k, s, c, sn of n clips, policy a mask or an [n] array of masks (the gated draw's); float32 with the header's roundings"""
    w = _words(n, seed, stream_id)
    pol = np.broadcast_to(np.asarray(policy, np.int64), (n,))
    one = np.ones(n, F32)
    f = np.where((pol & WARP_FLIP) != 0, np.where(w[:, 0] & 1, F32(-1), F32(1)), one).astype(F32)
    k = np.where((pol & WARP_ROT90) != 0, w[:, 1] & 3, 0)
    a = (F32(2) * _unit(w[:, 2]) - F32(1)) / F32(6)
    s = np.where((pol & WARP_SCALE) != 0, (F32(1) + a) / (F32(1) - a), one).astype(F32)
    t = F32(2) * _unit(w[:, 3]) - F32(1)
    tt = t * t
    den = F32(1) + tt
    c = np.where((pol & WARP_ROTATE) != 0, (F32(1) - tt) / den, one).astype(F32)
    sn = np.where((pol & WARP_ROTATE) != 0, (F32(2) * t) / den, F32(0)).astype(F32)
    return f, k, s, c, sn


def compose(f, k, s, c, sn):
    """L = (1 / s) [[c, sn], [-sn, c]] Q_k diag(f, 1) as mat [n][8]: one division, four products, then signs and a permutation"""
    f, s, c, sn = (np.atleast_1d(np.asarray(v, F32)) for v in (f, s, c, sn))
    k = np.atleast_1d(np.asarray(k, np.int64))
    r = F32(1) / s
    rc, rs = r * c, r * sn
    assert rc.dtype == F32 and rs.dtype == F32
    a00, a01, a10, a11 = rc, rs, -rs, rc
    for j in range(3):                                                  # times Q_1 = [[0, -1], [1, 0]], k times
        turn = k > j
        a00, a01, a10, a11 = (np.where(turn, p, q) for p, q in ((a01, a00), (-a00, a01), (a11, a10), (-a10, a11)))
    mat = np.zeros((len(f), 8), F32)
    mat[:, 0], mat[:, 1], mat[:, 3], mat[:, 4] = f * a00, a01, f * a10, a11
    mat[mat == 0] = 0.0                                                 # (-0 -> +0)
    return mat


def draw(n, H, W, policy, seed, stream_id):
    """mcg_warp_draw: clip i takes Philox counter i of the stream, words w0..w3; flags = 0"""
    assert 0 <= policy <= 15 and not (policy & WARP_ROT90 and H != W)
    return compose(*components(n, policy, seed, stream_id))


def gate_units(n, seed, gate_sid):
    return _unit(_words(n, seed, gate_sid)).astype(np.float64)


def draw_gated(n, H, W, policy, seed, stream_id, gate_sid, p):
    """mcg_warp_draw_gated: (mat, mask) -- mask[i] = the flags that are in the policy and passed their gate; mat[:, 6] = mask"""
    assert stream_id != gate_sid and 0 <= policy <= 15 and not (policy & WARP_ROT90 and H != W)
    passed = gate_units(n, seed, gate_sid) < float(p)
    mask = np.zeros(n, np.int64)
    for j, flag in enumerate(COMPONENTS):
        if policy & flag:
            mask |= np.where(passed[:, j], flag, 0)
    mat = compose(*components(n, mask, seed, stream_id))
    mat[:, 6] = mask
    return mat, mask.astype(np.int32)


def perf_mode_mats(seed, it, rank, n, policy=FULL, p=None, H=64, W=64):
    """the matrices iteration `it` of rank `rank` draws in perf mode (ids base + 44 real, base + 45 generated,
    and with a probability p the gates on base + 46 / 47)"""
    base = (it * 64 + rank + 1) * 64
    if p is None:
        return {'real': draw(n, H, W, policy, seed, base + 44), 'fake': draw(n, H, W, policy, seed, base + 45)}
    return {'real': draw_gated(n, H, W, policy, seed, base + 44, base + 46, p)[0],
            'fake': draw_gated(n, H, W, policy, seed, base + 45, base + 47, p)[0]}


# ---- hand-placed matrices -----------------------------------------------------------------------------------------------------
def hand_placed_sets(H, W):
    """matrices that hit every edge (rows of six floats): identity; flip; the three quarter turns; the scale's two ends; the
    rotation's two ends t = +-(1 - 2^-23); all four components together; an offset of half a pixel (every tap pair at weight one
    half); an offset that moves every source outside the frame; the all-zero matrix (every output reads the centre taps, the
    backward box is the whole frame); a scale of 1e6.  The last three are where a kernel can go wrong with nothing but indexing."""
    t1 = 1.0 - 2.0 ** -23
    c_p, s_p = rotation(t1)
    c_m, s_m = rotation(-t1)
    combo = compose(-1.0, 3, F32(1.25), *rotation(0.3))[0]
    sets = [[1, 0, 0, 0, 1, 0],
            [-1, 0, 0, 0, 1, 0],
            [0, -1, 0, 1, 0, 0], [-1, 0, 0, 0, -1, 0], [0, 1, 0, -1, 0, 0],
            [F32(7) / F32(5), 0, 0, 0, F32(7) / F32(5), 0], [F32(5) / F32(7), 0, 0, 0, F32(5) / F32(7), 0],
            [c_p, s_p, 0, -s_p, c_p, 0], [c_m, s_m, 0, -s_m, c_m, 0],
            [combo[0], combo[1], 0, combo[3], combo[4], 0],
            [1, 0, 0.5, 0, 1, -0.5],
            [1, 0, 3.0 * W + 0.25, 0, 1, -2.0 * H],
            [0, 0, 0, 0, 0, 0],
            [1e6, 0, 0, 0, 1e6, 0]]
    return np.asarray(sets, F32)


N_HAND_PLACED = 14


def hand_placed(n, H, W, first=0):
    """n matrices [n][8]: hand_placed_sets, starting at set `first`, cyclically"""
    sets = hand_placed_sets(H, W)
    assert len(sets) == N_HAND_PLACED
    mat = np.zeros((n, 8), F32)
    for i in range(n):
        mat[i, :6] = sets[(first + i) % len(sets)]
    return mat


# ---- one training iteration ---------------------------------------------------------------------------------------------------
def update_core(model, gen, dis_i, dis_v, opt_g, opt_i, opt_v, x_real, t_real, rnd, dim_zl=0, video_len=16):
    """augment_ref.update_core with rnd['warp'] = {'real': mat, 'fake': mat} applied FIRST: warp, then augment_ref.forward when
    rnd['augment'] is there, then the label planes and the discriminators; on the way back augment_ref.adjoint, then adjoint.
    x_real_aug / x_fake_aug are what the discriminators saw, gx_aug the gradient with respect to x_fake_aug; x_fake and gx_fake
    keep their meaning (the generated clip, the gradient with respect to it)."""
    warp, aug = rnd['warp'], rnd.get('augment')
    cgan = model == 'cgan'
    t = rnd['t']

    def both(x, which):
        x = forward(x, warp[which])
        return ar.forward(x, *aug[which]) if aug is not None else x

    x_real_aug = both(x_real, 'real')
    xr = oupd.concat_label_video(x_real_aug, t_real, dim_zl) if cgan else x_real_aug
    y_real_i, c_real_i = net.dis_forward(dis_i, xr[:, :, t], rnd['noise_i_real'])
    y_real_v, c_real_v = net.dis_forward(dis_v, xr, rnd['noise_v_real'])

    x_fake_tn, t_fake, c_gen = net.gen_forward(gen, rnd['gen'], video_len)
    x_fake = x_fake_tn.transpose(1, 2, 0, 3, 4)
    x_fake_aug = both(x_fake, 'fake')
    xf = oupd.concat_label_video(x_fake_aug, t_fake, dim_zl) if cgan else x_fake_aug
    y_fake_i, c_fake_i = net.dis_forward(dis_i, xf[:, :, t], rnd['noise_i_fake'])
    y_fake_v, c_fake_v = net.dis_forward(dis_v, xf, rnd['noise_v_fake'])

    out = {}
    l_i, gr, gf = oupd.loss_dis(model, False, y_real_i, y_fake_i, t_real, t_fake)
    g_i = oupd.zero_grads(dis_i)
    net.dis_backward(dis_i, c_real_i, gr, g_i)
    net.dis_backward(dis_i, c_fake_i, gf, g_i)
    out['grads_dis_i'] = {k: v.copy() for k, v in g_i.items()}
    oupd.adam_wd_update(dis_i, g_i, opt_i)
    l_v, gr, gf = oupd.loss_dis(model, True, y_real_v, y_fake_v, t_real, t_fake)
    g_v = oupd.zero_grads(dis_v)
    net.dis_backward(dis_v, c_real_v, gr, g_v)
    net.dis_backward(dis_v, c_fake_v, gf, g_v)
    out['grads_dis_v'] = {k: v.copy() for k, v in g_v.items()}
    oupd.adam_wd_update(dis_v, g_v, opt_v)
    l_g, gi, gv = oupd.loss_gen(model, y_fake_i, y_fake_v, t_fake)
    gx_i = net.dis_backward(dis_i, c_fake_i, gi, None, need_gx=True)
    gx_v = net.dis_backward(dis_v, c_fake_v, gv, None, need_gx=True)
    c_img = x_fake_tn.shape[2]
    gx_aug = np.array(gx_v[:, :c_img])
    gx_aug[:, :, t] += gx_i[:, :c_img]
    gx = ar.adjoint(gx_aug, *aug['fake']) if aug is not None else gx_aug
    gx = adjoint(gx, warp['fake'])
    g_g = oupd.zero_grads(gen)
    net.gen_backward(gen, c_gen, gx.transpose(2, 0, 1, 3, 4), g_g)
    out['grads_gen'] = {k: v.copy() for k, v in g_g.items()}
    oupd.adam_wd_update(gen, g_g, opt_g)
    out.update(x_fake=x_fake, x_fake_aug=x_fake_aug, x_real_aug=x_real_aug, gx_fake=gx, gx_aug=gx_aug,
               y_real_i=y_real_i, y_real_v=y_real_v, y_fake_i=y_fake_i, y_fake_v=y_fake_v,
               loss_dis_i=float(l_i), loss_dis_v=float(l_v), loss_gen=float(l_g), t_fake=t_fake,
               min_margin=min(c['min_margin'] for c in (c_real_i, c_real_v, c_fake_i, c_fake_v, c_gen)))
    return out


class Case(ar.Case):
    """augment_ref.Case with the warp in front: `warp` the warp's policy, `policy` the augmentation's (0: none).  perf = (philox
    seed, rank): everything is drawn on perf mode's stream ids -- with p, a probability, through the gated draws of both stages;
    else the matrices come from draw() on stream ids 44 / 45 of `seed` (the augmentation's from 40 / 41, as augment_ref.Case)."""

    def __init__(self, model, dim_zl, nf, n, seed, warp=FULL, policy=ar.FULL, perf=None, p=None):
        super().__init__(model, dim_zl, nf, n, seed, policy=policy, perf=perf)
        self.warp, self.p = warp, p
        assert p is None or perf is not None

    def next(self):
        from oracle.philox import perf_mode_randomness
        before = (self.copy(self.nets), self.copy(self.opts))
        x_real = self.rng.uniform(-1, 1, (self.n, 3, 16, 64, 64))
        t_real = self.rng.randint(0, 6, self.n)
        if self.perf:
            seed, rank = self.perf
            rnd = perf_mode_randomness(seed, self.it, rank, self.model, self.n, self.nf, self.dim_zl)
            rnd['warp'] = perf_mode_mats(seed, self.it, rank, self.n, self.warp, self.p)
            if self.policy:
                if self.p is None:
                    rnd['augment'] = ar.perf_mode_params(seed, self.it, rank, self.n, self.policy)
                else:
                    import ada_ref
                    rnd['augment'] = ada_ref.perf_mode_params(seed, self.it, rank, self.n, self.p, self.policy)[0]
        else:
            rnd = oupd.draw_step_randomness(self.rng, self.model, self.n, 3, self.nf, dim_zl=self.dim_zl, dtype=np.float64)
            rnd['warp'] = {'real': draw(self.n, 64, 64, self.warp, self.seed, 44 + 64 * self.it),
                           'fake': draw(self.n, 64, 64, self.warp, self.seed, 45 + 64 * self.it)}
            if self.policy:
                rnd['augment'] = {'real': ar.draw(self.n, 64, 64, self.policy, self.seed, 40 + 64 * self.it),
                                  'fake': ar.draw(self.n, 64, 64, self.policy, self.seed, 41 + 64 * self.it)}
        ref = update_core(self.model, *self.nets, *self.opts, x_real, t_real, rnd, dim_zl=self.dim_zl)
        self.it += 1
        return before, x_real, t_real, rnd, ref
