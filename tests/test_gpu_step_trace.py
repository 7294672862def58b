"""What TrainStep.run enqueues and how it orders its streams, entry for entry against a trace recorded from the commit before
run() was split into phases (tests/golden/step_launch_trace.json; tests/golden/make_step_launch_trace.py says how).

The step tests compare numbers with the float64 oracle, and a dropped wait_stream / wait_event / record_stream can pass them by
luck of timing.  Here nothing is compared but the sequence itself (tests/launch_trace.py): every library call with its stream, every
stream-ordering call with its streams and events, every slice a gradient exchange would send -- over two iterations in perf mode,
the second of which meets the events the first one left.  The trace does not show that results are unchanged: that stays with the
oracle tests."""
import contextlib
import os

import pytest
import torch

import launch_trace

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_launch_trace.json')
N, T, HW, NF = 2, 16, 64, 4                                         # (the smallest nets the step tests use: test_gpu_augment._nets)
WARP, AUG = 'flip,rot90,scale,rotate', 'color,translation,cutout'

# name -> (model, dim_zl, TrainStep options, what else the case sets: 'chains' = CHAINS_MIN_N patched to 1, 'event' = an input_event
# per call, 'u8' = uint8 (N,T,H,W,C) input, 'exchange' = the exchange stub with a clip threshold on one optimizer)
CONFIGS = {
    'normal': ('normal', 0, {}, ()),
    'cgan': ('cgan', 6, {}, ()),
    'infogan': ('infogan', 6, {}, ()),
    'overlap_one_batch': ('normal', 0, dict(overlap=True), ()),
    'chains_ready_early': ('normal', 0, dict(overlap=True, input_ready_early=True), ('chains',)),
    'chains_input_event': ('normal', 0, dict(overlap=True, input_ready_early=True), ('chains', 'event')),
    'stages_ada': ('normal', 0, dict(warp=WARP, augment=AUG, ada=True), ()),
    'stages_ada_chains': ('normal', 0, dict(warp=WARP, augment=AUG, ada=True, overlap=True, input_ready_early=True), ('chains',)),
    'cgan_augment_chains': ('cgan', 6, dict(augment=AUG, overlap=True), ('chains',)),
    'u8': ('normal', 0, {}, ('u8',)),
    'u8_augment': ('normal', 0, dict(augment=AUG), ('u8',)),
    'exchange_ema_stats_clip': ('normal', 0, dict(ema_decay=0.999, grad_stats=True), ('exchange',)),
}


@contextlib.contextmanager
def _chains_from(step, n):
    old = step.CHAINS_MIN_N
    step.CHAINS_MIN_N = n
    try:
        yield
    finally:
        step.CHAINS_MIN_N = old


def record(name, iterations=2):
    """the trace of `iterations` perf-mode iterations of configuration `name`"""
    import mocogan_chainer_amd.hiplib as hl
    import mocogan_chainer_amd.nets as nets
    import mocogan_chainer_amd.step as step
    hl.load()
    assert not hl.autotune_on()
    model, dim_zl, opts, flags = CONFIGS[name]
    c_d = 3 + (dim_zl if model == 'cgan' else 0)
    out_d = 1 + (dim_zl if model == 'infogan' else 0)
    devnets = (nets.GenNet(dim_zl=dim_zl, n_filters=NF), nets.DisNet(2, c_d, out_d, NF, use_noise=True),
               nets.DisNet(3, c_d, out_d, NF, use_noise=True))
    opts = dict(opts)
    if 'exchange' in flags:
        opts['exchange'] = launch_trace.ExchangeStub()
        opts['hyper'] = {'image_gen': step.AdamHyper(), 'image_dis': step.AdamHyper(clip=1.0), 'video_dis': step.AdamHyper()}
    ts = step.TrainStep(model, *devnets, seed=11, **opts)
    g = torch.Generator().manual_seed(5)
    if 'u8' in flags:
        x = torch.randint(0, 256, (N, T, HW, HW, 3), generator=g, dtype=torch.uint8).cuda()
    else:
        x = (torch.rand((N, 3, T, HW, HW), generator=g) * 2 - 1).cuda()
    t_real = torch.randint(0, 6, (N,), generator=g, dtype=torch.int32).cuda() if dim_zl else None
    torch.cuda.synchronize()
    with _chains_from(step, 1 if 'chains' in flags else step.CHAINS_MIN_N), launch_trace.Recorder() as tr:
        for _ in range(iterations):
            kw = {}
            if 'event' in flags:
                kw['input_event'] = torch.cuda.Event()
                kw['input_event'].record()
            ts.run(x, t_real, **kw)
    torch.cuda.synchronize()
    return launch_trace.normalise(tr.entries)


@pytest.fixture(scope="module")
def golden():
    assert torch.cuda.is_available()
    return launch_trace.load(GOLDEN)


def test_the_golden_holds_these_configurations(golden):
    assert sorted(golden) == sorted(CONFIGS)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_trace_equals_the_parent_commits(golden, name):
    got, want = record(name), golden[name]
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, "entry %d of %d: %r, recorded %r (before it: %r)" % (i, len(want), a, b, got[max(0, i - 3):i])
    assert len(got) == len(want)
