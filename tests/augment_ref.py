"""Float64 statement of the differentiable augmentation (TEST INFRASTRUCTURE; include/mocogan_hip.h: mcg_augment_* is the
specification): the forward map, the adjoint of its linear part, the Philox parameter draw, and one training iteration with the
augmentation in front of both discriminators.  Clips are in the reference layout (N,C,T,H,W), valid channels only."""
import numpy as np

from oracle import net
from oracle import updater as oupd
from oracle.philox import philox4x32_10

AUG_COLOR, AUG_TRANSLATION, AUG_CUTOUT = 1, 2, 4
FULL = AUG_COLOR | AUG_TRANSLATION | AUG_CUTOUT


def identity_params(n):
    geo = np.zeros((n, 8), np.int32)
    col = np.zeros((n, 4), np.float32)
    col[:, 1:3] = 1.0
    return geo, col


def hand_placed(n, H, W):
    """parameter sets that hit every edge: shifts +-W/8, +-H/8 and 0; the rectangle at cx = 0, cx = W, the centre and empty;
    s = 0 and near 2, c = 0.5 and near 1.5, b = +-0.5, identity"""
    def rect(cx, cy):
        return [max(cx - W // 4, 0), min(cx - W // 4 + W // 2, W), max(cy - H // 4, 0), min(cy - H // 4 + H // 2, H)]
    near2, near15 = 2.0 - 2.0 ** -22, 1.5 - 2.0 ** -23
    sets = [([W // 8, H // 8] + rect(0, 0), [0.5, 0.0, 0.5]),
            ([-(W // 8), -(H // 8)] + rect(W, H), [-0.5, near2, near15]),
            ([0, 0] + rect(W // 2, H // 2), [0.25, 1.0, 1.0]),
            ([W // 8, -(H // 8), 0, 0, 0, 0], [0.0, 0.625, 1.25]),
            ([-(W // 8), H // 8] + rect(W, 0), [-0.5, 0.0, near15]),
            ([0, 0, 0, 0, 0, 0], [0.0, 1.0, 1.0])]
    geo = np.zeros((n, 8), np.int32)
    col = np.zeros((n, 4), np.float32)
    for i in range(n):
        g, c = sets[i % len(sets)]
        geo[i, :6], col[i, :3] = g, c
    return geo, col


def _col(col, dtype):
    col = np.asarray(col).astype(dtype)
    return (col[:, k].reshape(-1, 1, 1, 1, 1) for k in range(3))


def _kept(geo, H, W):
    """keep[n][y][x]: output position (y, x) lies outside the cutout rectangle; (sy, sx, inside): its source and whether the
    source lies inside the frame"""
    geo = np.asarray(geo, np.int64)
    dx, dy, x0, x1, y0, y1 = (geo[:, k].reshape(-1, 1, 1) for k in range(6))
    ys, xs = np.arange(H).reshape(1, H, 1), np.arange(W).reshape(1, 1, W)
    rect = (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    sy, sx = ys - dy + 0 * xs, xs - dx + 0 * ys
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    return ~rect & inside, np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)


def forward(x, geo, col, dtype=np.float64):
    """colour, translation, cutout on x (N,C,T,H,W); geo (N,8) = dx, dy, x0, x1, y0, y1, -, -; col (N,4) = b, s, c, -"""
    x = np.asarray(x).astype(dtype)
    n, _, _, H, W = x.shape
    b, s, c = _col(col, dtype)
    one = dtype(1)
    v = x + b
    v = s * v + (one - s) * v.mean(axis=1, keepdims=True)
    m = x.mean(axis=(1, 2, 3, 4), keepdims=True) + b
    v = c * v + (one - c) * m
    keep, sy, sx = _kept(geo, H, W)
    src = v[np.arange(n).reshape(-1, 1, 1), :, :, sy, sx]            # [n][y][x][C][T]: v(t, y - dy, x - dx)
    out = np.where(keep[..., None, None], src, dtype(0))
    return np.ascontiguousarray(out.transpose(0, 3, 4, 1, 2))


def adjoint(g, geo, col, dtype=np.float64):
    """the adjoint of forward's linear part: gradient w.r.t. the augmented clips (N,C,T,H,W) -> gradient w.r.t. the clips"""
    g = np.asarray(g).astype(dtype)
    n, _, _, H, W = g.shape
    _, s, c = _col(col, dtype)
    one = dtype(1)
    keep, sy, sx = _kept(geo, H, W)
    # scatter of the kept positions onto their sources == gather at (sy + dy, sx + dx): written as the scatter here, so that
    # the kernel's gather is checked against the other statement
    g1 = np.zeros_like(g)
    nn, yy, xx = np.nonzero(keep)
    g1[nn, :, :, sy[nn, yy, xx], sx[nn, yy, xx]] = g[nn, :, :, yy, xx]
    g2 = c * g1 + (one - c) * g1.mean(axis=(1, 2, 3, 4), keepdims=True)
    return s * g2 + (one - s) * g2.mean(axis=1, keepdims=True)


def draw(n, H, W, policy, seed, stream_id):
    """mcg_augment_draw: clip i takes Philox counters 2i, 2i + 1 of the stream, words w0..w7"""
    idx = np.arange(2 * n, dtype=np.uint64)
    z = np.zeros(2 * n, np.uint32)
    r = philox4x32_10((idx & np.uint64(0xFFFFFFFF)).astype(np.uint32), (idx >> np.uint64(32)).astype(np.uint32),
                      z + np.uint32(stream_id & 0xFFFFFFFF), z + np.uint32(stream_id >> 32), seed & 0xFFFFFFFF, seed >> 32)
    w = np.stack(r, axis=1).reshape(n, 8).astype(np.int64)

    def u(v):
        return (v >> 9).astype(np.float64) * 2.0 ** -23

    geo, col = identity_params(n)
    if policy & AUG_COLOR:
        col[:, 0], col[:, 1], col[:, 2] = u(w[:, 0]) - 0.5, 2 * u(w[:, 1]), u(w[:, 2]) + 0.5
    if policy & AUG_TRANSLATION:
        geo[:, 0] = w[:, 3] % (2 * (W // 8) + 1) - W // 8
        geo[:, 1] = w[:, 4] % (2 * (H // 8) + 1) - H // 8
    if policy & AUG_CUTOUT:
        cx, cy = w[:, 5] % (W + 1), w[:, 6] % (H + 1)
        geo[:, 2], geo[:, 3] = np.clip(cx - W // 4, 0, W), np.clip(cx - W // 4 + W // 2, 0, W)
        geo[:, 4], geo[:, 5] = np.clip(cy - H // 4, 0, H), np.clip(cy - H // 4 + H // 2, 0, H)
    return geo, col


def perf_mode_params(seed, it, rank, n, policy=FULL, H=64, W=64):
    """the parameters iteration `it` of rank `rank` draws in perf mode (ids base + 40 real, base + 41 generated)"""
    base = (it * 64 + rank + 1) * 64
    return {'real': draw(n, H, W, policy, seed, base + 40), 'fake': draw(n, H, W, policy, seed, base + 41)}


def update_core(model, gen, dis_i, dis_v, opt_g, opt_i, opt_v, x_real, t_real, rnd, dim_zl=0, video_len=16):
    """oracle.updater.update_core's composition (model/updater.py:78-113) with rnd['augment'] = {'real': (geo, col), 'fake': (geo, col)}
    applied to the real and the generated clips in front of concat_label_video, and its adjoint on the clip gradient in front of
    the generator's backward pass.  Returns the oracle's `keep=True` dict plus x_real_aug, x_fake_aug and gx_aug; x_fake and
    gx_fake keep their meaning (the un-augmented clip, the gradient with respect to it)."""
    aug = rnd['augment']
    cgan = model == 'cgan'
    t = rnd['t']
    x_real_aug = forward(x_real, *aug['real'])
    xr = oupd.concat_label_video(x_real_aug, t_real, dim_zl) if cgan else x_real_aug
    y_real_i, c_real_i = net.dis_forward(dis_i, xr[:, :, t], rnd['noise_i_real'])
    y_real_v, c_real_v = net.dis_forward(dis_v, xr, rnd['noise_v_real'])

    x_fake_tn, t_fake, c_gen = net.gen_forward(gen, rnd['gen'], video_len)
    x_fake = x_fake_tn.transpose(1, 2, 0, 3, 4)
    x_fake_aug = forward(x_fake, *aug['fake'])
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
    gx = adjoint(gx_aug, *aug['fake'])
    g_g = oupd.zero_grads(gen)
    net.gen_backward(gen, c_gen, gx.transpose(2, 0, 1, 3, 4), g_g)
    out['grads_gen'] = {k: v.copy() for k, v in g_g.items()}
    oupd.adam_wd_update(gen, g_g, opt_g)
    out.update(x_fake=x_fake, x_fake_aug=x_fake_aug, x_real_aug=x_real_aug, gx_fake=gx, gx_aug=gx_aug,
               y_real_i=y_real_i, y_real_v=y_real_v, y_fake_i=y_fake_i, y_fake_v=y_fake_v,
               loss_dis_i=float(l_i), loss_dis_v=float(l_v), loss_gen=float(l_g), t_fake=t_fake,
               min_margin=min(c['min_margin'] for c in (c_real_i, c_real_v, c_fake_i, c_fake_v, c_gen)))
    return out


class Case:
    """The oracle side of a teacher-forced run (tests/test_gpu_step.py:_run_steps' set-up): three float64 networks with their Adam
    states from `seed`; every next() draws a batch and the iteration's randomness, returns the state BEFORE the iteration (what
    the device is loaded with) and the augmented oracle's result of it.  perf = (philox seed, rank): the randomness and the
    augmentation parameters are those of perf mode's stream ids; else everything comes from the NumPy generator, and the
    augmentation parameters from draw() on stream ids 40 / 41 of `seed`."""

    def __init__(self, model, dim_zl, nf, n, seed, policy=FULL, perf=None):
        import copy
        self.copy = copy.deepcopy
        self.model, self.dim_zl, self.nf, self.n, self.seed, self.policy, self.perf = model, dim_zl, nf, n, seed, policy, perf
        self.rng = rng = np.random.RandomState(seed)
        out_c = 7 if model == 'infogan' else 1
        c_d = 3 + (dim_zl if model == 'cgan' else 0)
        f64 = lambda p: {k: (v.astype(np.float64) if v.dtype.kind == 'f' else v) for k, v in p.items()}      # noqa: E731
        self.nets = [f64(net.init_generator(rng, dim_zl=dim_zl, n_filters=nf)), f64(net.init_discriminator(rng, 2, c_d, out_c, nf)),
                     f64(net.init_discriminator(rng, 3, c_d, out_c, nf))]
        self.opts = [oupd.new_adam_state(q) for q in self.nets]
        self.it = 0

    def next(self):
        from oracle.philox import perf_mode_randomness
        before = (self.copy(self.nets), self.copy(self.opts))
        x_real = self.rng.uniform(-1, 1, (self.n, 3, 16, 64, 64))
        t_real = self.rng.randint(0, 6, self.n)
        if self.perf:
            rnd = perf_mode_randomness(self.perf[0], self.it, self.perf[1], self.model, self.n, self.nf, self.dim_zl)
            rnd['augment'] = perf_mode_params(self.perf[0], self.it, self.perf[1], self.n, self.policy)
        else:
            rnd = oupd.draw_step_randomness(self.rng, self.model, self.n, 3, self.nf, dim_zl=self.dim_zl, dtype=np.float64)
            rnd['augment'] = {'real': draw(self.n, 64, 64, self.policy, self.seed, 40 + 64 * self.it),
                              'fake': draw(self.n, 64, 64, self.policy, self.seed, 41 + 64 * self.it)}
        ref = update_core(self.model, *self.nets, *self.opts, x_real, t_real, rnd, dim_zl=self.dim_zl)
        self.it += 1
        return before, x_real, t_real, rnd, ref
