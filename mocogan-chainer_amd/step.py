"""One MoCoGAN training iteration on the device (reference model/updater.py:78-113) and the
data-parallel gradient exchange.

The kernel schedule reproduces the reference's observable ordering:
  forwards with the OLD parameters: D_I(real), D_V(real), G, D_I(fake), D_V(fake)      (:97-108)
  D_I: loss_dis -> backward(real)+backward(fake) -> [all-reduce] -> Adam              (:111)
  D_V: the same                                                                         (:112)
  G  : loss_gen -> gradient through the ALREADY UPDATED D_V and D_I (saved activations,
       new weights / gamma: quirk Q5) -> G backward -> [all-reduce] -> Adam             (:113)
Gradients Chainer computes into the other networks and then discards (Q6) are not computed.
"""
import math
import os

import torch

from . import hiplib as hl
from . import layout as lay
from . import nets

CHAINS = os.environ.get('MCG_CHAINS', '1') == '1'          # the VideoDiscriminator's real / fake calls as two chains on two streams (A/B switch)
CHAINS_MIN_N = int(os.environ.get('MCG_CHAINS_MIN_N', '64'))  # ... from this many clips per call on (measured on one MI355X, clips/s with / without:
                                                              # fp32 batch 32 2120 / 2138, 64 2206 / 2140, 128 2284 / 2257; bf16 128 11.89 / 11.80 k, 256 12.19 / 11.94 k)
chain_iterations = 0                                          # iterations that took the two-chain schedule (tests assert that it really ran)


_STREAMS = {}


def _side_streams(device):
    """the process's six side streams on `device`: [D_I's, three weight-gradient streams (G, D_I, D_V), D_V's chain, its weight-gradient]"""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _STREAMS:
        # (MCG_STREAM_MAP="a,b,c,d,e,f": tuning aid -- which of twelve streams, in creation order, plays each role)
        m = [int(v) for v in os.environ.get('MCG_STREAM_MAP', '0,1,2,3,4,5').split(',')]
        pool = [torch.cuda.Stream(device=device) for _ in range(max(m) + 1)]
        _STREAMS[key] = [pool[i] for i in m]
    return _STREAMS[key]


class AdamHyper:
    """train.py:93-101 -- Chainer Adam(alpha=2e-4, beta1=5e-5) (beta2 0.999 / eps 1e-8 defaults)
    plus the WeightDecay(1e-5) hook."""

    def __init__(self, alpha=2e-4, beta1=5e-5, beta2=0.999, eps=1e-8, weight_decay=1e-5, clip=None):
        self.alpha, self.beta1, self.beta2, self.eps, self.weight_decay = alpha, beta1, beta2, eps, weight_decay
        # clip: None = off; T > 0 (math.inf allowed): chainer.optimizer.GradientClipping(T) -- the loss gradient of ALL of this
        # optimizer's parameters is scaled by min(1, T / its L2 norm) before weight decay, and an update whose gradient holds a
        # non-finite element is skipped (math.inf: that alone).  No reference counterpart (train.py:93-101 adds WeightDecay only).
        self.clip = check_clip(clip)

    def lr(self, t):
        return self.alpha * math.sqrt(1.0 - self.beta2 ** t) / (1.0 - self.beta1 ** t)


def check_clip(threshold):
    """a clipping threshold as AdamHyper carries it: None, or a float > 0 that is finite or +inf"""
    if threshold is None:
        return None
    t = float(threshold)
    if not t > 0.0:                                               # (a NaN fails too)
        raise ValueError('the gradient-clipping threshold must be > 0 (math.inf: skip non-finite steps only), got %r' % (threshold,))
    return t


ADA_DEFAULTS = {'target': 0.6, 'interval': 4, 'kimg': 500}        # Karras et al. 2020, section 3 and appendix D


def check_ada(ada):
    """the `ada` option of TrainStep as a dict of target / interval / kimg, or None (off): True = the paper's values, a dict
    overrides any of them"""
    if ada is None or ada is False:
        return None
    if ada is True:
        ada = {}
    if not isinstance(ada, dict):
        raise ValueError("ada is True or a dict with any of 'target', 'interval', 'kimg', got %r" % (ada,))
    unknown = sorted(set(ada) - set(ADA_DEFAULTS))
    if unknown:
        raise ValueError('unknown ada settings %s (known: %s)' % (unknown, ', '.join(sorted(ADA_DEFAULTS))))
    cfg = dict(ADA_DEFAULTS, **ada)
    target, interval, kimg = float(cfg['target']), cfg['interval'], float(cfg['kimg'])
    if not -1.0 < target < 1.0:                                   # (a NaN fails too)
        raise ValueError('the ada target is a mean of signs: it lies in (-1, 1), got %r' % (cfg['target'],))
    if isinstance(interval, bool) or int(interval) != interval or interval < 1:
        raise ValueError('the ada interval is a whole number of iterations >= 1, got %r' % (interval,))
    if not 0.0 < kimg < math.inf:
        raise ValueError('ada kimg (thousands of real clips in which p may cross [0, 1]) must be > 0 and finite, got %r' % (cfg['kimg'],))
    return {'target': target, 'interval': int(interval), 'kimg': kimg}


def check_augment_gate(augment, augment_p, ada, exchange=None, warp=None):
    """TrainStep's augment_p / ada options -> (the starting probability, or None when both are off; check_ada's dict or None).
    They gate the components of `augment` and of `warp` alike: one of the two has to be there."""
    cfg = check_ada(ada)
    if augment_p is None and cfg is None:
        return None, None
    if not hl.parse_augment(augment) and not hl.parse_warp(warp):
        raise ValueError('augment_p / ada set how often the augmentation is applied: they need a non-empty augment policy')
    if exchange is not None and exchange.active:
        raise ValueError('augment_p / ada with a gradient exchange: the ranks would need an all-reduce of the sign sums to keep '
                         'p equal (not implemented)')
    p0 = 0.0 if augment_p is None else float(augment_p)
    if not 0.0 <= p0 <= 1.0:                                      # (a NaN fails too)
        raise ValueError('augment_p lies in [0, 1], got %r' % (augment_p,))
    return p0, cfg


def ema_rate(decay, k):
    """r_k = 1 - d_k of the averaged generator's k-th update (k = 0, 1, ...: updates already done): d_k = min(decay, (1 + k) / (10 + k)),
    a warm-up that lets the average forget its starting point (rates 0.9, 0.82, 0.75, ... until the decay takes over).  In double,
    like AdamHyper.lr; the kernels take it as a float.  No reference counterpart: the reference samples the last iterate."""
    if not 0.0 <= decay < 1.0:
        raise ValueError('the decay of the averaged generator must lie in [0, 1), got %r' % (decay,))
    return 1.0 - min(float(decay), (1.0 + k) / (10.0 + k))


def adam_update(net, hyper, grad_scale=1.0):
    """optimizer.update() tail: hooks, t += 1, per-parameter Adam -- one launch over the flat buffers.
    grad_scale: 1 / world under data parallelism (the flat gradient then holds the SUM over the ranks).
    A net with an averaged twin (nets.GenNet.enable_ema): the same launch advances the average of the parameters (fp.e), one more
    launch behind it on the same stream the average of the running statistics.
    A net with gradient statistics (nets._Net.enable_grad_stats): their two launches go first, on this stream, over the gradient as
    it stands (after the exchange: with grad_scale the norm is the mean gradient's).  hyper.clip set: the update then reads its
    gradient scale from the control block they left (hl.adam_wd_ctl) and writes nothing when the gradient held a non-finite
    element.  The host never waits for a norm, so on a skipped update everything the host does here happens all the same: t, the
    averaged twin's k and its running statistics advance, the split filters are refreshed (to what they were)."""
    net.t += 1
    fp = net.fp
    ema = net.ema
    gst = net.gstats
    clip = getattr(hyper, 'clip', None)
    if clip is not None and gst is None:
        raise RuntimeError('a clipping threshold needs the gradient statistics of the network: net.enable_grad_stats() '
                           '(TrainStep does it for every optimizer that carries one)')
    if gst is not None:
        gst.launch(fp, grad_scale, clip)
    r = ema_rate(ema.decay, ema.k) if ema is not None else 0.0
    if clip is not None:
        hl.adam_wd_ctl(fp.p, fp.g, fp.m, fp.v, hyper.lr(net.t), hyper.beta1, hyper.beta2, hyper.eps, hyper.weight_decay, gst.ctl,
                       ema=fp.e if ema is not None else None, ema_rate=r, p16=fp.p16 if net.precision == 'bf16' else None)
    elif ema is None:
        hl.adam_wd(fp.p, fp.g, fp.m, fp.v, hyper.lr(net.t), hyper.beta1, hyper.beta2, hyper.eps, hyper.weight_decay, grad_scale,
                   p16=fp.p16 if net.precision == 'bf16' else None)
    else:
        hl.adam_wd_ema(fp.p, fp.g, fp.m, fp.v, hyper.lr(net.t), hyper.beta1, hyper.beta2, hyper.eps, hyper.weight_decay, fp.e, r, grad_scale,
                       p16=fp.p16 if net.precision == 'bf16' else None)
    if ema is not None:
        hl.ema_multi([(net.running[key], ema.running[key]) for key in sorted(net.running)], r)
        ema.k += 1
        ema.written(net)
    fp.touch()
    net.refresh_wsplits()                                         # ('f32x3': the split forms of the filters follow in one launch)


class GradExchange:
    """Data-parallel averaging of one network's flat gradient over the ranks of `group`
    (RCCL over xGMI on the GPU box, gloo in the CPU tests).  No reference counterpart: the
    reference is single-device (train.py:87-91).  Each rank runs the step on its own shard of
    the batch with its own BatchNorm statistics; gradients are averaged, so every rank applies
    the same Adam update and the replicas stay bit-identical.  The collective SUMS; the division by the world
    size happens inside the Adam kernel (``grad_scale``), not in a pass of its own."""

    def __init__(self, group=None, force=False):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.grad_scale = 1.0 / self.world
        # force: a world of ONE still goes through the collectives (a one-GPU rehearsal of the RCCL path: bench.py MCG_DP_REHEARSE_NCCL)
        self.active = self.world > 1 or (force and dist.is_available() and dist.is_initialized())

    def start(self, flat_grad):
        """Asynchronous SUM all-reduce of a (slice of a) flat gradient; returns a handle for finish()."""
        if not self.active:
            return None
        return (self.dist.all_reduce(flat_grad, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True), flat_grad)

    def finish(self, handle):
        """Wait for the collective start() returned the handle of (stream-ordered on RCCL: the current stream waits, the host
        does not).  Its buffer then holds the SUM over the ranks; adam_update(..., grad_scale=self.grad_scale) makes it the mean."""
        if handle is None:
            return
        work, _ = handle
        work.wait()

    def all_reduce_sum(self, t):
        """In-place SUM over the ranks, ordered on the current stream (synchronised BatchNorm's per-channel sums)."""
        if self.active:
            self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM, group=self.group)

    def broadcast_params(self, tensors, src=0):
        if not self.active:
            return
        for t in tensors:
            self.dist.broadcast(t, src=src, group=self.group)

    def broadcast_replica(self, net, src=0):
        """rank src's copy of everything a replica of `net` holds (replica_tensors, replica_counters) replaces everyone's"""
        if not self.active:
            return
        self.broadcast_params(replica_tensors(net), src)
        cnt = torch.tensor(replica_counters(net), dtype=torch.int64, device=net.fp.p.device)
        self.broadcast_params([cnt], src)
        set_replica_counters(net, cnt.tolist())


def replica_tensors(net):
    """What makes two replicas of a network equal, as the tensors a data-parallel run broadcasts after construction / resume:
    parameters, Adam moments, running statistics -- and, with an averaged twin, its parameters and running statistics."""
    tensors = [net.fp.p, net.fp.m, net.fp.v] + list(net.running.values())
    if net.ema is not None:
        tensors += [net.fp.e] + list(net.ema.running.values())
    return tensors


def replica_counters(net):
    """... and as integers: the Adam step counter (it sets lr_t), the BatchNorm call counts, the averaged twin's update count"""
    return [net.t] + [net.bn_count[k] for k in sorted(net.bn_count)] + ([net.ema.k] if net.ema is not None else [])


def set_replica_counters(net, values):
    """replica_counters' list back into the net; what is derived from the tensors that arrived with it is rebuilt"""
    names = sorted(net.bn_count)
    net.t = int(values[0])
    for k, v in zip(names, values[1:]):
        net.bn_count[k] = int(v)
    net.fp.touch()
    if net.precision == 'bf16':
        net.fp.refresh16()
    if net.ema is not None:
        net.ema.written(net)
        net.ema.k = int(values[1 + len(names)])


class ClipStage:
    """One differentiable stage on [n][T][H][W][4] clips in front of BOTH discriminators, one parameter set per clip."""
    # It is applied to the real and to the generated clips, and the generator's gradient goes back through its adjoint.
    # name: 'warp' | 'augment', also the key of its parameters in run()'s inject and result; mask: the enabled components
    # ids: {'real' | 'fake': (Philox stream id of the parameters, ... of the gates)}, relative to the iteration's base
    # gate: the state block of augment_p / ada, or None; draw, draw_gated: hl.*_draw (no gate) / hl.*_draw_gated
    # fwd, bwd: hl.*_fwd / hl.*_bwd, called as fn(clip, valid channels, *operands(parameters, clip), a new clip) -- what differs
    # between the stages (two parameter tensors and a workspace, or one matrix tensor) is in `operands` and nowhere else
    # missing: the error text when parity mode lacks inject[name]

    def __init__(self, name, mask, ids, gate, draw, draw_gated, fwd, bwd, operands, missing):
        self.name, self.mask, self.ids, self.gate, self.missing = name, mask, ids, gate, missing
        self.draw, self.draw_gated, self.fwd, self.bwd, self.operands = draw, draw_gated, fwd, bwd, operands

    def forward(self, x, which, it):
        """x -> its staged copy with the parameters of `which` ('real' | 'fake'), drawn first if need be: on the current stream"""
        par = it.par[self.name]
        if which not in par:
            sid, gate_sid = (it.base + i for i in self.ids[which])
            if self.gate is None:
                par[which] = self.draw(it.n, it.H, it.W, self.mask, it.seed, sid, device=x.device)
            else:
                par[which] = self.draw_gated(it.n, it.H, it.W, self.mask, it.seed, sid, gate_sid, self.gate, device=x.device)
        return self.fwd(x, it.c_img, *self.operands(par[which], x), torch.empty_like(x))

    def adjoint(self, g, which, it):
        """the gradient w.r.t. the staged clips of `which` -> the gradient w.r.t. the clips: on the current stream"""
        return self.bwd(g, it.c_img, *self.operands(it.par[self.name][which], g), torch.empty_like(g))


class _Iteration:
    """What the phases of one TrainStep.run share."""
    # Set here: the call's arguments, the shape, the frame index t, the first Philox stream id, the model's flags, the stages'
    # parameters (the caller's in parity mode, else drawn where the clips are staged), the two streams.  Added by the phases as
    # they produce them: the built clips (x_real_aug, real_clip, x_fake, x_fake_aug, xf), the first_input writers (first_real,
    # first_fake: D_V's, D_I's), logits, loss gradients, saved activations.

    def __init__(self, ts, x_real, t_real, inject, input_event):
        self.x_real, self.t_real, self.inject, self.input_event = x_real, t_real, inject, input_event
        self.u8 = x_real.dtype == torch.uint8
        if self.u8:
            self.n, self.T, self.H, self.W, self.c_img = x_real.shape
            if not x_real.is_contiguous():
                raise hl.McgError("uint8 clips must be dense (N,T,H,W,C)")
        else:
            self.n, self.c_img, self.T, self.H, self.W = x_real.shape
        self.hw = self.H * self.W
        self.seed, self.base = ts.seed, ts.stream_base(ts.iteration, ts.rank)
        self.t = int(inject['t']) if inject is not None else ts.frame_index(ts.iteration, self.T)
        self.cgan, self.with_ce = ts.model == 'cgan', ts.model == 'infogan'
        self.c_valid = self.c_img + (ts.gen.dim_zl if self.cgan else 0)
        self.par = {}
        for stage in ts._stages:
            if inject is not None and stage.name not in inject:
                raise ValueError(stage.missing)
            self.par[stage.name] = dict(inject[stage.name]) if inject is not None else {}
        self.main = torch.cuda.current_stream()
        self.side = ts.side if ts.side is not None else self.main

    def noise(self, key):
        return self.inject[key] if self.inject is not None else None

    def rng(self, k):
        return None if self.inject is not None else (self.seed, self.base + 8 * k)


class TrainStep:
    """Holds the three networks, their Adam hyper-parameters and runs update_core on device data."""

    def __init__(self, model, gen, dis_i, dis_v, hyper=None, exchange=None, seed=0, rank=0, precision=None, overlap=False, sync_bn=False,
                 input_ready_early=False, ema_decay=None, augment=None, grad_stats=False, augment_p=None, ada=None, warp=None):
        assert model in ('normal', 'cgan', 'infogan')
        p0, ada_cfg = check_augment_gate(augment, augment_p, ada, exchange, warp)      # (refused before anything is touched)
        self.model, self.gen, self.dis_i, self.dis_v = model, gen, dis_i, dis_v
        if precision is not None:                                 # 'f32' | 'bf16': MFMA operand type of every conv GEMM
            assert precision in ('f32', 'bf16', 'f32x3')
            for net in (gen, dis_i, dis_v):
                net.set_precision(precision)
        if hl.autotune_on():
            # the training step's forward launches that take position-major rows / live K-steps (hiplib.use_live_list = tiles.table.use_live: only where the
            # table still holds the shipped or the dense code; MCG_LIVE_STEPS=0 leaves it).  set_autotune() itself loads the shipped
            # table and the dense list, nothing else.
            hl.use_live_list()
        # ema_decay: None = off (nothing allocated, the launches of before); D in [0, 1): the generator keeps an exponential moving
        # average of its parameters and running statistics (gen.ema; ema_rate is the schedule), advanced by its Adam launch
        if ema_decay is not None:
            gen.enable_ema(ema_decay)
        # augment: None = off (no launch, no allocation, no stream id more); 'color,translation,cutout' (any subset) or a mask of
        # hl.AUG_* flags: differentiable augmentation (Zhao et al. 2020) of the real and the generated clips in front of BOTH
        # discriminators, one parameter set per clip; the generator's gradient goes back through its adjoint.  No reference counterpart.
        self.augment = hl.parse_augment(augment)
        # warp: None = off (no launch, no allocation, no stream id more); 'flip,rot90,scale,rotate' (any subset) or a mask of
        # hl.WARP_* flags: the geometric family of Karras et al. 2020 as a second differentiable stage IN FRONT of `augment` -- one
        # affine matrix per clip, bilinear taps, zero padding (hl.warp_fwd); the generator's gradient goes back through its exact
        # adjoint (hl.warp_bwd).  With augment_p / ada its components share the one probability of the state block.
        self.warp = hl.parse_warp(warp)
        # augment_p, ada: both None = the draws of before (no launch, allocation, stream id or event more).  augment_p = P in [0, 1]:
        # every component of the policy is applied to a clip with probability P (Karras et al. 2020: below about 0.8 the
        # augmentation does not leak into the generated clips) -- hl.augment_draw_gated reads P from a state block in device memory.
        # ada = True or {'target', 'interval', 'kimg'} (ADA_DEFAULTS): P starts at augment_p (or 0) and one launch per iteration
        # (hl.ada_update, on the real halves of the logits the step has anyway) moves it every `interval` iterations by
        # interval n / (1000 kimg) towards r_t = E[sign(D(real))] = target, r_t that of the discriminator that overfits more.
        # The host never reads the block; ada_stats() does, for the log.  No reference counterpart.
        self.ada = ada_cfg
        self._ada = hl.ada_state(p0, gen.device) if p0 is not None else None
        self._ev_ada = None
        # the enabled stages in application order -- the warp, then the augmentation: cutout and the zero border of a translation
        # stay axis-aligned.  The augmentation has two parameter tensors and a workspace, the warp one matrix tensor.  With a state
        # block both draw gated by it.
        self._stages = [stage for stage in (
            ClipStage('warp', self.warp, {'real': (self.WARP_STREAM_REAL, self.WARP_GATE_REAL), 'fake': (self.WARP_STREAM_FAKE, self.WARP_GATE_FAKE)},
                      self._ada, hl.warp_draw, hl.warp_draw_gated, hl.warp_fwd, hl.warp_bwd, lambda mat, x: (mat,),
                      "the warp is on: parity mode needs inject['warp'] = {'real': mat, 'fake': mat}"),
            ClipStage('augment', self.augment, {'real': (self.AUG_STREAM_REAL, self.AUG_GATE_REAL), 'fake': (self.AUG_STREAM_FAKE, self.AUG_GATE_FAKE)},
                      self._ada, hl.augment_draw, hl.augment_draw_gated, hl.augment_fwd, hl.augment_bwd,
                      lambda par, x: (*par, hl.augment_workspace(x.shape[0], x.device)),
                      "augmentation is on: parity mode needs inject['augment'] = {'real': (geo, col), 'fake': (geo, col)}"),
        ) if stage.mask]
        self.hyper = hyper or {'image_gen': AdamHyper(), 'image_dis': AdamHyper(), 'video_dis': AdamHyper()}
        self.exchange = exchange
        self._grad_scale = exchange.grad_scale if exchange else 1.0   # (the collectives SUM: 1 / world goes into the Adam launches)
        # grad_stats: False = off (nothing allocated, the launches of before).  True: every network's Adam update is preceded by the
        # two launches of hl.grad_stats over its flat gradient -- norm, peak, largest element, non-finite count, per-tensor norms,
        # read with grad_stats() -- and stays on the launch it had.  A clipping threshold on an optimizer (AdamHyper.clip) implies the
        # statistics for that network, whose update then goes through hl.adam_wd_ctl (adam_update).
        self._nets = {'image_gen': gen, 'image_dis': dis_i, 'video_dis': dis_v}
        for name, net in self._nets.items():
            if grad_stats or getattr(self.hyper[name], 'clip', None) is not None:
                net.enable_grad_stats()
        # sync_bn (opt-in): BatchNorm statistics and their backward sums are all-reduced over the ranks, i.e.
        # taken over the GLOBAL batch; without it every rank normalises with the statistics of its own shard.
        for net in (gen, dis_i, dis_v):
            net.sync_bn = exchange if (sync_bn and exchange is not None) else None
        self.seed, self.rank = seed, rank
        # input_ready_early (two-chain schedule only): the caller guarantees that x_real / t_real of run() were complete BEFORE the
        # previous run() was queued (resident synthetic data; a loader that stays one batch ahead).  The real chain of the
        # VideoDiscriminator then waits only for what it really needs -- the VideoDiscriminator's Adam update of the previous
        # iteration -- instead of for everything queued so far, and runs beside the END of the previous iteration (G's backward pass):
        # the host is several milliseconds ahead of the GPU, so the launches are there to overlap.  Off by default: a caller that
        # writes parameters or inputs on the current stream between two iterations (the teacher-forced tests do) needs the full wait.
        self.input_ready_early = bool(input_ready_early)
        self._ev_dv_updated = None
        self.iteration = 0
        self.device = gen.device
        self.loss = torch.zeros(3, device=self.device)            # loss_dis_i, loss_dis_v, loss_gen
        # overlap: independent work goes to side HIP streams -- the whole ImageDiscriminator update (small
        # kernels that cannot fill 256 CUs) beside the VideoDiscriminator's, and every weight-gradient GEMM
        # beside the input-gradient GEMM of the same layer.  Same kernels, same results; only placement in time.
        self.side = None
        self._wstreams = None
        self._chain_stream = None
        self._dv_chains = None
        self.set_overlap(overlap)

    def set_overlap(self, on):
        """Switch the side-stream placement on or off (between iterations)."""
        if on and self._wstreams is None:
            # ONE set of side streams per process and device (not per TrainStep): the runtime deals hardware queues to streams in
            # creation order (four queues by default), and which streams share a queue decides what really overlaps -- a second
            # TrainStep with fresh streams got another assignment and ran 4-5 % slower than the first (bench.py's secondary
            # workloads against the same workloads run alone).  (More hardware queues are not better: GPU_MAX_HW_QUEUES=8 cost
            # the batch-32 iteration 22 %.)
            st = _side_streams(self.device)
            self._side = st[0]
            self._wstreams = st[1:4]
            # the VideoDiscriminator's real and fake calls as two chains (nets._Net.chain): a second compute stream and a
            # weight-gradient stream of its own for the real chain
            self._chain_stream = st[4]
            self._dv_chains = self.dis_v.make_chains([st[5], self._wstreams[2]])
        self.side = self._side if on else None
        for i, net in enumerate((self.gen, self.dis_i, self.dis_v)):
            net.wgrad_stream = self._wstreams[i] if on else None

    # ---- cgan label planes (model/updater.py:65-76) -------------------------------------------------
    def _concat_label_clip(self, x_dev, labels):
        """x_dev [n][T][H][W][4] with C=3 -> [n][T][H][W][pad4(3+dim_zl)] with -1/+1 label planes (one launch)."""
        n, T, H, W, _ = x_dev.shape
        c, dl = self.gen.out_channels, self.gen.dim_zl
        out = torch.empty((n, T, H, W, lay.pad4(c + dl)), device=x_dev.device)
        return hl.concat_label_planes(x_dev, c, dl, labels, out)

    # ---- perf-mode randomness bookkeeping ----------------------------------------------------------
    STREAMS_PER_RANK = 64        # Philox stream ids one rank may consume per iteration (uses 5 x 8, 40 / 41 with augmentation, 42 / 43 with its gates,
    #                              44 / 45 with the warp, 46 / 47 with its gates)
    AUG_STREAM_REAL, AUG_STREAM_FAKE = 40, 41     # ... the augmentation parameters of the real / the generated clips
    AUG_GATE_REAL, AUG_GATE_FAKE = 42, 43         # ... and, with augment_p / ada, the gates of their components
    WARP_STREAM_REAL, WARP_STREAM_FAKE = 44, 45   # ... the warp's matrices of the real / the generated clips
    WARP_GATE_REAL, WARP_GATE_FAKE = 46, 47       # ... and the gates of their components
    MAX_RANKS = 64

    def frame_index(self, it, T):
        """The frame D_I looks at (model/updater.py:96).  One draw per iteration, shared by the whole
        batch (quirk Q7) -- and, under data parallelism, by every rank: seeded by (seed, iteration) only."""
        g = torch.Generator()
        g.manual_seed(self.seed * 7919 + it)
        return int(torch.randint(0, T, (1,), generator=g))

    @classmethod
    def stream_base(cls, it, rank):
        """First Philox stream id of (iteration, rank): disjoint across both, so every rank adds
        independent noise / latent codes while sharing the seed."""
        assert 0 <= rank < cls.MAX_RANKS
        return (it * cls.MAX_RANKS + rank + 1) * cls.STREAMS_PER_RANK

    # ---- one iteration -------------------------------------------------------------------------
    def run(self, x_real, t_real=None, inject=None, input_event=None):
        """x_real: device tensor in the reference layout (N,C,T,H,W) float32 (model/updater.py:89-90) -- or the loader's own
        form, uint8 (N,T,H,W,C) as datasets.py decodes it: the first kernel of each discriminator then normalises (v - 128) / 128
        while it writes the device layout (mcg_pack_clip_u8), and no float copy of the batch is ever made.
        t_real: int32 device tensor (N,) or None.
        input_event: an event recorded (on whatever stream produced x_real -- a loader's copy stream) when x_real was complete; the
        caller's current stream must be ordered behind it as well.  With it the two-chain schedule starts the VideoDiscriminator's
        real chain as soon as that event and the previous iteration's Adam(D_V) have happened, beside the end of the previous
        iteration (what `input_ready_early` promises for resident data, here per call and checked by the hardware).
        inject: parity mode -- dict with 't', 'noise_{i,v}_{real,fake}' (lists of 4 device tensors in
        device layout, pre-scaled) and 'gen' (latent draw dict); None = perf mode (Philox in-kernel,
        frame index from a seeded host generator shared by all ranks, quirk Q7).  With augmentation on, parity mode also needs
        'augment': {'real': (geo, col), 'fake': (geo, col)} -- int32 [n][8] and float [n][4] device tensors (mcg_augment_draw's
        form); perf mode draws them in-kernel on stream ids base + 40 / 41.  The result then also holds 'x_real_aug', 'x_fake_aug'
        (what the discriminators saw, without label planes), 'gx_aug' (the gradient w.r.t. x_fake_aug) and 'augment' (the
        parameters); 'x_fake' / 'gx_fake' stay the un-augmented clip and the gradient w.r.t. it.
        With augment_p / ada, perf mode draws the gates on stream ids base + 42 / 43 (geo[:, 6] then says what was applied); parity
        mode takes inject['augment'] as it is -- the caller gates it -- and the controller's update runs all the same.
        With the warp on, parity mode needs 'warp': {'real': mat, 'fake': mat} -- float [n][8] device tensors (mcg_warp_draw's form);
        perf mode draws them on stream ids base + 44 / 45 (gates: base + 46 / 47).  The clips are warped first, then augmented;
        the result holds 'warp' (the matrices) and 'x_real_aug' / 'x_fake_aug' / 'gx_aug' with the meaning above: what the
        discriminators saw after BOTH stages, and the gradient with respect to it."""
        it = _Iteration(self, x_real, t_real, inject, input_event)
        self._real_input(it)
        if it.two_chains:
            self._start_real_chain(it)
        self._fake_input(it)
        self._dis_i_gradient(it)
        if it.two_chains:
            self._dis_v_gradient_two_chains(it)
        else:
            self._dis_v_gradient_one_batch(it)
        self._dis_updates(it)
        if self.ada is not None:
            self._controller_step(it)
        self._gen_update(it)
        self.iteration += 1
        # (it.par: the enabled stages' parameters under their names, 'warp' / 'augment')
        res = dict(it.par, x_real_aug=it.x_real_aug, x_fake_aug=it.x_fake_aug, gx_aug=it.gx_aug) if self._stages else {}
        return {**res, 'x_fake': it.x_fake, 't_fake': it.t_fake, 't': it.t, 'gx_fake': it.gx_fake, 'saved_gen': it.s_gen,
                'saved_fake_i': it.s_fake_i, 'saved_fake_v': it.s_fake_v, 'saved_i': it.s_i, 'saved_v': it.s_v,
                'y_real_i': it.y_real_i, 'y_real_v': it.y_real_v, 'y_fake_i': it.y_fake_i, 'y_fake_v': it.y_fake_v}

    # ---- the phases of run(), in its order: each takes the iteration's record and says where it enqueues ---------------------
    def _built_input(self, it, x, which, labels):
        """A real or generated clip -> (staged, that with label planes, D_V's and D_I's first_input writers for it): current stream"""
        n, T, hw, t, cp, c_valid = it.n, it.T, it.hw, it.t, self.dis_v.cp0, it.c_valid
        for stage in self._stages:
            x = stage.forward(x, which, it)
        clip = self._concat_label_clip(x, labels) if it.cgan else x

        def first_v(out, na):
            hl.bn_act_fwd(n * T * hw, cp, clip, None, hl.ACT_NONE, out, c_valid=c_valid, **na)

        def first_i(out, na):                                        # frame t of every clip: the clip's item stride, one frame
            hl.bn_act_fwd(n * hw, cp, clip[:, t], None, hl.ACT_NONE, out, c_valid=c_valid, rows_per_item=hw,
                          item_stride=T * hw * cp, **na)
        return x, clip, (first_v, first_i)

    def _build_real_clip(self, it):
        """The real clips in the device layout, staged, with label planes, and the writers that read them: on the current stream"""
        # label planes (cgan) are part of D's input, and a stage reads whole clips: the clip is built once -- packed without
        # noise, warped, augmented, label planes appended (they are neither) -- and the discriminators' first kernels add the noise
        x = torch.empty((it.n, it.T, it.H, it.W, lay.pad4(it.c_img)), device=self.device)
        (hl.pack_clip_u8 if it.u8 else hl.pack_clip)(it.n, it.c_img, lay.pad4(it.c_img), it.T, it.hw, it.x_real, x)
        it.x_real_aug, it.real_clip, it.first_real = self._built_input(it, x, 'real', it.t_real)

    def _real_input(self, it):
        """Decides the schedule, once, and sets it.first_real.  A clip that is built is built on the main stream, where every reader
        is ordered behind it -- except with stages under the two-chain schedule: _start_real_chain builds it."""
        dv = self.dis_v
        # (not for 'f32x3': measured 2-3 % SLOWER at 32 / 64 / 128 clips -- its launches are tuned, form by form, at the 2n batch)
        it.two_chains = (CHAINS and self.side is not None and self.exchange is None and dv.sync_bn is None
                         and dv.precision != 'f32x3' and it.n >= CHAINS_MIN_N)
        if it.cgan or self._stages:
            if not (self._stages and it.two_chains):
                self._build_real_clip(it)
            return
        n, c_img, T, hw, t, x_real, u8, cp = it.n, it.c_img, it.T, it.hw, it.t, it.x_real, it.u8, dv.cp0

        def first_v(out, na):
            (hl.pack_clip_u8 if u8 else hl.pack_clip)(n, c_img, cp, T, hw, x_real, out, **na)

        def first_i(out, na):
            if u8:                                                   # frame t of every clip: the clip's item stride, one frame
                hl.pack_clip_u8(n, c_img, cp, 1, hw, x_real[:, t], out, stride_n=T * hw * c_img, **na)
            else:
                hl.pack_clip(n, c_img, cp, 1, hw, x_real[:, :, t], out, stride_n=c_img * T * hw, stride_c=T * hw, **na)
        it.first_real = first_v, first_i

    def _start_real_chain(self, it):
        """Two-chain schedule only: D_V's forward on the real clips (it.real_chain) on the chain stream, beside G's forward.  That
        stream waits for the main stream -- or, when the caller vouches for x_real, only for the events of the previous iteration."""
        cs, main = self._chain_stream, it.main
        if (self.input_ready_early or it.input_event is not None) and self._ev_dv_updated is not None and not it.cgan:
            cs.wait_event(self._ev_dv_updated)                       # the previous iteration's Adam(D_V)
            if self._ev_ada is not None:
                cs.wait_event(self._ev_ada)                          # ... and its controller step: the gates below read the p it left
            if it.input_event is not None:
                cs.wait_event(it.input_event)                        # x_real (otherwise ready by contract)
        else:
            cs.wait_stream(main)                                     # x_real (and whatever produced it)
        if self._stages:
            # the augmented real clips are made on the chain stream, which may run ahead of the main stream (input_event /
            # input_ready_early): its own reader follows in stream order; the main stream -- D_I's side stream and the
            # one-batch readers are ordered behind it -- waits for the event
            with torch.cuda.stream(cs):
                self._build_real_clip(it)
                ev = cs.record_event()
            main.wait_event(ev)
            for x in ([it.x_real_aug] if it.real_clip is it.x_real_aug else [it.x_real_aug, it.real_clip]):
                x.record_stream(main)
                x.record_stream(self.side)                           # (the two-chain schedule has side streams)
        with torch.cuda.stream(cs), self._dv_chains[0]:
            it.real_chain = self.dis_v.forward(it.n, it.first_real[0], noise=it.noise('noise_v_real'), rng=it.rng(1))
        it.x_real.record_stream(cs)

    def _fake_input(self, it):
        """G's forward (it needs nothing from D), the stages, the label planes, the writers: main stream, waits for nothing"""
        draw = it.inject['gen'] if it.inject is not None else self.gen.draw(it.n, it.rng(2))
        it.x_fake, it.s_gen = self.gen.forward(it.n, draw)
        it.t_fake = draw['labels']
        it.x_fake_aug, it.xf, it.first_fake = self._built_input(it, it.x_fake, 'fake', it.t_fake)

    def _dis_loss(self, it, net, slot, y_real, y_fake, with_ce):
        """[d loss / d logits] of (real | fake) for one discriminator, its gradient buffer cleared in front: current stream"""
        n, cd = it.n, net.out_channels
        g = torch.empty((2 * n, cd), device=self.device)
        net.zero_grad()
        hl.loss_dis(n, cd, y_real, y_fake, it.t_real, it.t_fake, with_ce, self.loss[slot:slot + 1], g[:n], g[n:])
        return g

    def _bucketed_exchange(self, net):
        """A network's gradient exchange in two buckets -> (on_late_bucket for its backward pass, finish); no exchange: (None, no-op)"""
        # finish() sends the two remaining slices and makes the current stream wait for all three;
        # the late bucket (D_V: dc4/W..dc5/b, 76 % of the bytes) is final after the first two layers of the backward pass and
        # travels while the rest is still being computed
        ex = self.exchange
        if ex is None:
            return None, lambda: None
        lo, hi = net.grad_bucket_late()
        late = []

        def finish():
            rest = [ex.start(net.fp.g[:lo]), ex.start(net.fp.g[hi:])]
            for h in late + rest:
                ex.finish(h)
        return (lambda: late.append(ex.start(net.fp.g[lo:hi]))), finish

    def _dis_i_gradient(self, it):
        """D_I's forward, loss, backward, and its exchange started: on the side stream, which first waits for the main stream"""
        # image_dis_optimizer.update(loss_dis, ...) (model/updater.py:111) with D_I on [real | fake] as one 2n batch (:97,107;
        # per-call BatchNorm statistics, real first)
        di, n = self.dis_i, it.n
        it.side.wait_stream(it.main)                                 # x_fake is ready
        with torch.cuda.stream(it.side):
            y_i, it.s_i = di.forward_groups(n, [dict(first_input=it.first_real[1], noise=it.noise('noise_i_real'), rng=it.rng(0)),
                                                dict(first_input=it.first_fake[1], noise=it.noise('noise_i_fake'), rng=it.rng(3))])
            it.y_real_i, it.y_fake_i = y_i[:n], y_i[n:]
            it.g_i = self._dis_loss(it, di, 0, it.y_real_i, it.y_fake_i, False)
            di.backward(it.s_i, it.g_i, True)
            it.work_i = self.exchange.start(di.fp.g) if self.exchange else None

    def _dis_v_gradient_one_batch(self, it):
        """D_V's forward, loss, backward with its late bucket sent, one-batch form: on the main stream, waits for nothing more"""
        # video_dis_optimizer.update(loss_dis, ...) (:112) with D_V on [real | fake] as one 2n batch (:98,108)
        dv, n = self.dis_v, it.n
        y_v, it.s_v = dv.forward_groups(n, [dict(first_input=it.first_real[0], noise=it.noise('noise_v_real'), rng=it.rng(1)),
                                            dict(first_input=it.first_fake[0], noise=it.noise('noise_v_fake'), rng=it.rng(4))])
        it.y_real_v, it.y_fake_v = y_v[:n], y_v[n:]
        it.g_v = self._dis_loss(it, dv, 1, it.y_real_v, it.y_fake_v, it.with_ce)
        on_late, it.finish_v = self._bucketed_exchange(dv)
        dv.backward(it.s_v, it.g_v, True, on_late_bucket=on_late)

    def _dis_v_gradient_two_chains(self, it):
        """The same, two-chain form: the fake call on the main stream, the real half's backward on the chain stream.  The main stream
        waits for the chain stream twice (the real logits; that backward), the chain stream once for the main stream (the loss)."""
        # The real and the fake call as TWO CHAINS on two streams (round 4): the real call needs nothing from G and was queued on
        # the chain stream BEFORE G's forward (_start_real_chain); the fake call follows G on the main stream.  One chain's
        # BatchNorm / activation passes (HBM-bound, 3.3 of 21.5 ms exposed at batch 256 in the one-batch schedule) run beside the
        # other's GEMMs.  Same kernels on n instead of 2n samples; what the calls share is kept in the reference's order by events
        # (nets._Net._ordered: running statistics real -> fake, gradient accumulators real -> fake).
        global chain_iterations
        chain_iterations += 1
        dv, n, main = self.dis_v, it.n, it.main
        cs, (ch_r, ch_f) = self._chain_stream, self._dv_chains
        it.y_real_v, s_real = it.real_chain
        with ch_f:
            it.y_fake_v, s_fake = dv.forward(n, it.first_fake[0], noise=it.noise('noise_v_fake'), rng=it.rng(4))
        main.wait_stream(cs)                                         # the real logits
        it.y_real_v.record_stream(main)
        it.g_v = self._dis_loss(it, dv, 1, it.y_real_v, it.y_fake_v, it.with_ce)
        cs.wait_stream(main)                                         # the loss gradients (and the cleared gradient buffer)
        it.g_v.record_stream(cs)
        with torch.cuda.stream(cs), ch_r:
            dv.backward(s_real, it.g_v[:n], True)
        with ch_f:
            dv.backward(s_fake, it.g_v[n:], True)
        main.wait_stream(cs)
        it.s_v = {'n': n, 'G': 2, 'chains': [s_real, s_fake]}

    def _record_for_next(self, name, stream):
        """record on `stream` the event self.<name> that the NEXT iteration's real chain waits for: made at first use, with chains only"""
        if self._dv_chains is not None:
            if getattr(self, name) is None:
                setattr(self, name, torch.cuda.Event())
            getattr(self, name).record(stream)

    def _dis_updates(self, it):
        """Adam(D_I) on the side stream, Adam(D_V) on the main stream, each behind its exchange; then main waits for the side stream"""
        with torch.cuda.stream(it.side):
            if self.exchange:
                self.exchange.finish(it.work_i)                      # D_I's exchange overlapped D_V's backward
            adam_update(self.dis_i, self.hyper['image_dis'], self._grad_scale)
        if not it.two_chains:                                        # (that schedule is taken without an exchange only)
            it.finish_v()
        adam_update(self.dis_v, self.hyper['video_dis'], self._grad_scale)
        self._record_for_next('_ev_dv_updated', it.main)
        it.main.wait_stream(it.side)                                 # D_I's logits and updated weights (Q5)

    def _controller_step(self, it):
        """With `ada`: the controller's launch on the main stream, where both discriminators' real logits are visible"""
        # every draw of this iteration is behind it (the chain stream's through main.wait_event in _start_real_chain), the next
        # iteration's follow in stream order or wait for the event recorded here
        cfg = self.ada
        hl.ada_update(it.y_real_v, it.y_real_i, cfg['target'], cfg['interval'] * it.n / (cfg['kimg'] * 1000.0), cfg['interval'], self._ada)
        self._record_for_next('_ev_ada', it.main)

    def _gen_update(self, it):
        """image_gen_optimizer.update(loss_gen, ...) (:113), through the ALREADY UPDATED discriminators (Q5) and the stages' adjoints.
        Main stream; with overlap D_I's layers run on the side stream, which waits for the main stream and is waited for."""
        gen, di, dv = self.gen, self.dis_i, self.dis_v
        n, T, H, W, hw, t, cp = it.n, it.T, it.H, it.W, it.hw, it.t, dv.cp0
        gen.zero_grad()
        gi, gv = it.g_i[:n], it.g_v[:n]                              # buffers reused: D's backward has consumed them
        hl.loss_gen(n, di.out_channels, it.y_fake_i, it.y_fake_v, it.t_fake, it.with_ce, self.loss[2:3], gi, gv)
        gx = torch.empty_like(it.xf)
        it.s_fake_v, it.s_fake_i = dv.select_group(it.s_v, 1), di.select_group(it.s_i, 1)
        gi_geom = hl.make_geom(n, 1, H, W, cp, di.chans[1], 1, x_stride0=T * hw * cp, precision=di.gemm_precision, ci_valid=di.chans[0])
        if self.side is not None:
            # the two discriminators' input gradients are independent until they meet in frame t of the clip gradient:
            # D_I's layers 5..2 (small kernels) run on the side stream beside D_V's; its LAST launch -- the input gradient of
            # dc1, accumulated onto frame t of what D_V's pass wrote -- follows on the main stream once both are done
            self.side.wait_stream(it.main)                           # loss_gen's gradients
            with torch.cuda.stream(self.side):
                last_i = di.backward(it.s_fake_i, gi, False, gx=gx[:, t], gx_geom=gi_geom, gx_accumulate=True, defer_gx=True)
            gi.record_stream(self.side)
            dv.backward(it.s_fake_v, gv, False, gx=gx)               # new D_V weights, old activations (Q5)
            it.main.wait_stream(self.side)
            last_i()
        else:
            dv.backward(it.s_fake_v, gv, False, gx=gx)               # new D_V weights, old activations (Q5)
            di.backward(it.s_fake_i, gi, False, gx=gx[:, t], gx_geom=gi_geom, gx_accumulate=True)
        if it.cgan:                                                  # label planes carry no gradient to G: the clip's channels alone
            gx = hl.concat_label_planes(gx, it.c_img, 0, None, torch.empty_like(it.x_fake))
        it.gx_aug = gx
        for stage in reversed(self._stages):                         # the adjoints of the generated clips' stages, last stage first
            gx = stage.adjoint(gx, 'fake', it)
        it.gx_fake = gx
        on_late, finish = self._bucketed_exchange(gen)
        gen.backward(it.s_gen, gx, on_late_bucket=on_late)
        finish()
        adam_update(gen, self.hyper['image_gen'], self._grad_scale)

    def grad_stats(self):
        """{network: {'grad_norm', 'grad_norm_peak' (since the last read; zeroed behind it), 'grad_max', 'nonfinite', 'clip_rate',
        'skipped' (updates so far), 'tensors': {parameter: norm}}} of the last iteration, for every network that keeps the
        statistics -- forces a host sync, like losses().  Norms are those of the gradient the update saw (the mean over the ranks)."""
        return {name: net.gstats.read() for name, net in self._nets.items() if net.gstats is not None}

    @property
    def has_ada_state(self):
        """does the step hold an augmentation state block (augment_p / ada): is there something for ada_stats() to report?"""
        return self._ada is not None

    def ada_state(self):
        """the eight doubles of the augmentation's state block (hl.ADA_*) as a float64 array, or None without augment_p / ada --
        forces a host sync"""
        return None if self._ada is None else self._ada.cpu().numpy()

    def load_ada_state(self, values):
        """ada_state()'s array back into the block (a resumed run); the host waits for the copy"""
        if self._ada is None:
            raise ValueError('this step has no augmentation state: augment_p / ada are off')
        v = torch.as_tensor(values, dtype=torch.float64).reshape(-1)
        if v.numel() != hl.ADA_DOUBLES:
            raise ValueError('the augmentation state is %d doubles, got %d' % (hl.ADA_DOUBLES, v.numel()))
        self._ada.copy_(v)
        torch.cuda.synchronize(self.device)

    def ada_stats(self):
        """{'p', 'rt_video', 'rt_image' (r_t = E[sign(D(real))] at the last adjustment), 'adjustments'} of the augmentation's state
        block -- forces a host sync, like losses()"""
        st = self.ada_state()
        if st is None:
            raise ValueError('this step has no augmentation state: augment_p / ada are off')
        return {'p': float(st[hl.ADA_P]), 'rt_video': float(st[hl.ADA_RT_V]), 'rt_image': float(st[hl.ADA_RT_I]),
                'adjustments': int(st[hl.ADA_ADJUSTMENTS])}

    def losses(self):
        """(loss_dis_i, loss_dis_v, loss_gen) of the last iteration -- forces a host sync."""
        l = self.loss.cpu().tolist()
        return {'image_dis/loss': l[0], 'video_dis/loss': l[1], 'image_gen/loss': l[2]}


def make_models(model='normal', num_labels=6, channel=3, dim_zc=50, dim_zm=10, n_filters=64, video_length=16,
                use_noise=True, noise_sigma=0.2, device='cuda', seed=0):
    """The three networks exactly as train.py:69-85 configures them for --model normal|cgan|infogan
    (note: n_filters_gen is used for all three nets there, and on MUG num_labels = 6 makes the GRU
    label-conditioned even for 'normal': quirk Q9)."""
    if model not in ('normal', 'cgan', 'infogan'):
        raise ValueError('unknown model %r' % model)
    if model in ('cgan', 'infogan') and num_labels == 0:
        raise ValueError('Called %s model, but dataset has no label.' % model)       # train.py:75,81
    c_d = channel + (num_labels if model == 'cgan' else 0)
    out_d = 1 + (num_labels if model == 'infogan' else 0)
    gen = nets.GenNet(dim_zc, dim_zm, num_labels, channel, n_filters, video_length, device=device, seed=seed)
    dis_i = nets.DisNet(2, c_d, out_d, n_filters, use_noise, noise_sigma, video_length, device=device, seed=seed + 1)
    dis_v = nets.DisNet(3, c_d, out_d, n_filters, use_noise, noise_sigma, video_length, device=device, seed=seed + 2)
    return gen, dis_i, dis_v


def pretune_and_share_tiles(exchange, model, precision, batch, rank, **model_kw):
    """Data parallel: make every rank run the SAME GEMM tile codes.  With autotune on, a geometry the table
    (tiles.table) does not hold is timed at its first launch -- per rank, so two ranks may keep different winners (results stay identical:
    Adam consumes the all-reduced gradient; but a rank with a slower choice sets the step time).  Here every rank runs ONE
    local iteration (no exchange) on throw-away networks, which tunes whatever is missing, then rank 0's table replaces
    everyone's.  No reference counterpart (the reference is single-device, train.py:87-91)."""
    if exchange is None or not exchange.active:
        return
    if hl.autotune_on():
        model_kw.setdefault('num_labels', 6)
        gen, di, dv = make_models(model, seed=0, **model_kw)           # (same widths / channels as the run: same geometries)
        ts = TrainStep(model, gen, di, dv, seed=0, rank=rank, precision=precision)
        x = torch.zeros((batch, gen.out_channels, gen.video_len, nets.IMG, nets.IMG), device=gen.device)
        t = torch.zeros(batch, dtype=torch.int32, device=gen.device)
        ts.run(x, t)
        torch.cuda.synchronize()
        del ts, gen, di, dv, x
    table = [[[list(k), v] for k, v in hl.tile_choices().items()]] if rank == 0 else [None]
    exchange.dist.broadcast_object_list(table, src=0, group=exchange.group)
    hl.replace_tile_choices(table[0])
