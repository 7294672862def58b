"""CPU-only checks of the averaged generator: the two entry points validate their arguments on the host, the decay schedule, the
flag and keyword plumbing (off by default, a decay outside [0, 1) refused), the snapshot keys and their round trip on
host-resident networks, and the list of tensors a data-parallel run broadcasts."""
import ctypes

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def hl():
    import mocogan_chainer_amd as pkg
    pkg.build()
    import mocogan_chainer_amd.hiplib as hiplib
    hiplib.load()
    return hiplib


def _ptr(addr):
    return ctypes.c_void_p(addr)       # non-null and never dereferenced: every call below fails before a launch


def test_adam_wd_ema_validates_on_the_host(hl):
    lib = hl.load()
    assert lib.mcg_version() == 8 and hl.ABI_VERSION == 8            # two entry points more, no argument list changed
    n = 1024
    p, g, m, v, e = (_ptr(0x100000 * (i + 1)) for i in range(5))      # five disjoint ranges of n floats

    def call(n=n, p=p, g=g, m=m, v=v, e=e, rate=0.5):
        return lib.mcg_adam_wd_ema(n, p, g, m, v, 1e-3, 5e-5, 0.999, 1e-8, 1e-5, 1.0, None, e, rate, None)
    for null in ('p', 'g', 'm', 'v', 'e'):
        assert call(**{null: None}) == -1, null
    assert call(n=0) == -1 and call(n=-4) == -1
    for rate in (0.0, -0.5, 1.0000001, 2.0, float('nan'), float('inf')):
        assert call(rate=rate) == -1, rate
    for other in (p, g, m, v):                                         # the average may not be any of the optimizer's buffers
        assert call(e=other) == -1
        assert call(e=_ptr(other.value + 4 * (n - 1))) == -1           # ... nor overlap one by a single element
        assert call(e=_ptr(other.value - 4 * (n - 1))) == -1


def test_ema_multi_validates_on_the_host(hl):
    lib = hl.load()

    def segs(k, n=8, src=0x1000, dst=0x2000):
        a = (hl.EmaSeg * max(k, 1))()
        for q in a:
            q.src, q.dst, q.n = src, dst, n
        return ctypes.cast(a, ctypes.c_void_p)
    assert lib.mcg_ema_multi(1, None, 0.5, None) == -1
    assert lib.mcg_ema_multi(0, segs(0), 0.5, None) == -1
    assert lib.mcg_ema_multi(-1, segs(1), 0.5, None) == -1
    assert lib.mcg_ema_multi(33, segs(33), 0.5, None) == -1
    assert lib.mcg_ema_multi(2, segs(2, n=0), 0.5, None) == -1
    assert lib.mcg_ema_multi(2, segs(2, n=-3), 0.5, None) == -1
    assert lib.mcg_ema_multi(2, segs(2, src=None), 0.5, None) == -1
    assert lib.mcg_ema_multi(2, segs(2, dst=None), 0.5, None) == -1
    for rate in (0.0, -1.0, 1.5, float('nan')):
        assert lib.mcg_ema_multi(2, segs(2), rate, None) == -1, rate


def test_binding_refuses_host_tensors(hl):
    x = torch.zeros(16)
    with pytest.raises(hl.McgError):
        hl.adam_wd_ema(x, x, x, x, 1e-3, 0.9, 0.999, 1e-8, 0.0, torch.zeros(16), 0.5)
    with pytest.raises(hl.McgError):
        hl.adam_wd_ema(x, x, x, x, 1e-3, 0.9, 0.999, 1e-8, 0.0, torch.zeros(15), 0.5)        # a shorter average would be overrun
    with pytest.raises(hl.McgError):
        hl.ema_multi([(x, torch.zeros(16))], 0.5)
    with pytest.raises(hl.McgError):
        hl.ema_multi([(x, torch.zeros(8))], 0.5)


def test_schedule():
    from mocogan_chainer_amd.step import ema_rate
    assert ema_rate(0.999, 0) == 1.0 - 0.1                              # k = 0: d_0 = 1 / 10
    assert ema_rate(0.05, 0) == 1.0 - 0.05                              # ... unless the decay is smaller still
    assert ema_rate(0.5, 0) == 1.0 - 1.0 / 10.0 and ema_rate(0.5, 1) == 1.0 - 2.0 / 11.0        # the rates 0.9, 0.82 of D = 0.5
    assert ema_rate(0.5, 8) == 0.5 and ema_rate(0.5, 7) == 1.0 - 8.0 / 17.0                     # (1 + k) / (10 + k) reaches 1 / 2 at k = 8
    assert all(ema_rate(0.0, k) == 1.0 for k in (0, 1, 10, 10 ** 6))    # D = 0: the average IS the parameters
    for D in (0.5, 0.99, 0.999):
        r = [ema_rate(D, k) for k in range(20000)]
        assert all(a >= b for a, b in zip(r, r[1:])) and r[-1] == 1.0 - D and all(0.0 < x <= 1.0 for x in r)
        assert all(x == 1.0 - min(D, (1.0 + k) / (10.0 + k)) for k, x in enumerate(r))
        assert all(0.0 < float(np.float32(x)) <= 1.0 for x in r)         # ... and as the float the kernels are given
    for bad in (1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            ema_rate(bad, 0)


def test_flag_defaults_to_off_and_refuses_a_decay_outside_the_unit_interval():
    import train
    assert train.parse_args([]).ema_decay == 0
    assert train.parse_args(['--ema_decay', '0.999']).ema_decay == 0.999
    for bad in ('1', '1.5', '-0.1', 'nan'):
        with pytest.raises(SystemExit):
            train.parse_args(['--ema_decay', bad])


def _models(**kw):
    import mocogan_chainer_amd.step as step
    return step.make_models('normal', n_filters=8, device='cpu', **kw)


def test_off_allocates_nothing_and_a_bad_decay_is_refused():
    import mocogan_chainer_amd.step as step
    gen, di, dv = _models(seed=0)
    step.TrainStep('normal', gen, di, dv)
    assert gen.ema is None and gen.fp.e is None and di.ema is None and dv.ema is None
    for bad in (1.0, -0.5, 2.0, float('nan')):
        with pytest.raises(ValueError):
            step.TrainStep('normal', gen, di, dv, ema_decay=bad)
        with pytest.raises(ValueError):
            gen.enable_ema(bad)
    assert gen.ema is None and gen.fp.e is None
    step.TrainStep('normal', gen, di, dv, ema_decay=0.0)                 # 0 is a decay (the average tracks the parameters); None is off
    assert gen.ema is not None and di.ema is None and dv.ema is None


def test_enabling_starts_from_the_live_values_and_shares_the_buffer():
    import mocogan_chainer_amd.step as step
    gen, di, dv = _models(seed=1)
    gen.running['bn2/avg_mean'].normal_()
    gen.bn_count['bn1'] = 7
    step.TrainStep('normal', gen, di, dv, ema_decay=0.99)
    e = gen.ema
    assert (e.decay, e.k) == (0.99, 0)
    assert e.fp.p is gen.fp.e and e.fp.p.data_ptr() != gen.fp.p.data_ptr()          # the buffer the Adam launch writes, no copy of it
    assert e.fp.g is None and e.fp.m is None and e.fp.v is None                      # nothing an optimizer needs
    assert torch.equal(e.fp.p, gen.fp.p)
    live, avg = gen.export_reference_params(), e.export_reference_params()
    assert list(live) == list(avg) and all(np.array_equal(live[k], avg[k]) for k in live)
    assert all(e.running[k].data_ptr() != gen.running[k].data_ptr() for k in gen.running)
    v0 = e.fp.version
    assert e.to('cpu') is e and gen.ema is e and e.fp.p is gen.fp.e and e.fp.version > v0     # a move keeps the buffer shared
    assert torch.equal(e.fp.p, gen.fp.p) and e.k == 0
    with pytest.raises(Exception):
        e.backward(None, None)
    with pytest.raises(Exception):
        e.forward(2, None)                                                # (config.train is True: the averaged net is test-mode only)


class _Link:
    def __init__(self, impl):
        self.impl = impl


class _Updater:
    """what Trainer.state / load_state need of model.updater.Updater"""

    def __init__(self, nets, **step_kw):
        import mocogan_chainer_amd.step as step
        from mocogan_chainer_amd import trainer as T
        from datasets import SyntheticDataset
        self.iteration = 0
        self._it = T.SerialIterator(SyntheticDataset(8, 6), 4)
        self._step = step.TrainStep('normal', *nets, **step_kw)
        self._links = dict(zip(('image_gen', 'image_dis', 'video_dis'), (_Link(n) for n in nets)))

    def get_iterator(self, name):
        return self._it

    def links(self):
        return self._links


def test_updater_passes_the_decay_on_and_still_refuses_unknown_arguments():
    import model.updater as mu
    from model.net import ImageGenerator, ImageDiscriminator, VideoDiscriminator
    from mocogan_chainer_amd import trainer as T
    from datasets import SyntheticDataset

    def updater(**kw):
        np.random.seed(0)
        nets = (ImageGenerator(50, 10, 0, 3, 8, 16, device='cpu'), ImageDiscriminator(3, 1, 8, True, 0.2, device='cpu'),
                VideoDiscriminator(3, 1, 8, True, 0.2, device='cpu'))
        opts = {}
        for k, n in zip(('image_gen', 'image_dis', 'video_dis'), nets):
            opts[k] = T.Adam(alpha=2e-4, beta1=5e-5)
            opts[k].setup(n)
        u = mu.Updater(model='normal', models=nets, video_length=16, img_size=64, channel=3, dim_zl=0,
                       iterator=T.SerialIterator(SyntheticDataset(8, 6), 4), tensorboard_writer=T.NullWriter(), optimizer=opts, **kw)
        return u, nets[0]
    u, gen = updater()
    assert gen.ema is None
    u, gen = updater(ema_decay=0.9)
    assert gen.ema is not None and gen.ema.impl is gen.impl.ema and gen.ema is gen.ema and gen.impl.ema.decay == 0.9
    assert gen.ema.ema is None
    assert [k for k, _ in gen.ema.namedparams()] == [k for k, _ in gen.namedparams()]
    assert set(gen.ema.serialize_dict()) == set(gen.serialize_dict())
    with pytest.raises(TypeError):
        updater(ema_decay=0.9, ema_warmup=10)


def test_snapshot_keys_exist_only_when_on_and_round_trip():
    from mocogan_chainer_amd import trainer as T
    off = T.Trainer(_Updater(_models(seed=2)), (1, 'epoch')).state()
    assert not [k for k in off if 'ema' in k]
    nets = _models(seed=2)
    u = _Updater(nets, ema_decay=0.9)
    gen = nets[0]
    gen.fp.e.normal_()                                                   # an average that differs from the parameters
    for t in gen.ema.running.values():
        t.uniform_(0.5, 2.0)
    gen.ema.k = 41
    d = T.Trainer(u, (1, 'epoch')).state()
    keys = sorted(k for k in d if k.startswith('updater/ema:'))
    assert keys == sorted(['updater/ema:image_gen/' + k for k in gen.ref_shapes] + ['updater/ema:image_gen/k'])
    assert not [k for k in d if k.startswith(('updater/ema:image_dis', 'updater/ema:video_dis'))]
    assert {k: v for k, v in d.items() if not k.startswith('updater/ema:')}.keys() == off.keys()
    assert int(d['updater/ema:image_gen/k']) == 41
    assert not np.array_equal(d['updater/ema:image_gen/dc3/W'], d['updater/model:image_gen/dc3/W'])
    nets2 = _models(seed=3)
    u2 = _Updater(nets2, ema_decay=0.9)
    v0 = nets2[0].ema.fp.version
    T.Trainer(u2, (1, 'epoch')).load_state(d)
    e2 = nets2[0].ema
    assert e2.k == 41 and e2.fp.version > v0                             # (what is derived from the average is rebuilt)
    assert e2.fp.p is nets2[0].fp.e
    want, got = gen.ema.export_reference_params(), e2.export_reference_params()      # (the flat buffer's padding is not part of a snapshot)
    assert list(want) == list(got) and all(np.array_equal(want[k], got[k]) for k in want)
    assert all(torch.equal(e2.running[k], gen.ema.running[k]) for k in gen.running)
    assert torch.equal(nets2[0].fp.p, gen.fp.p) and not torch.equal(nets2[0].fp.p, e2.fp.p)


def test_resuming_a_snapshot_without_an_average_starts_it_from_the_loaded_parameters():
    from mocogan_chainer_amd import trainer as T
    src = _models(seed=4)
    src[0].running['bn3/avg_var'].uniform_(0.5, 2.0)
    d = T.Trainer(_Updater(src), (1, 'epoch')).state()                   # written by a run without averaging
    nets = _models(seed=5)
    u = _Updater(nets, ema_decay=0.99)
    gen = nets[0]
    gen.ema.k = 17
    gen.fp.e.zero_()
    T.Trainer(u, (1, 'epoch')).load_state(d)
    assert gen.ema.k == 0 and gen.ema.decay == 0.99
    assert torch.equal(gen.fp.p, src[0].fp.p) and torch.equal(gen.fp.e, src[0].fp.p)
    assert all(torch.equal(gen.ema.running[k], src[0].running[k]) for k in src[0].running)
    # ... and a run without averaging reads a snapshot that holds one
    d_on = T.Trainer(u, (1, 'epoch')).state()
    plain = _models(seed=6)
    T.Trainer(_Updater(plain), (1, 'epoch')).load_state(d_on)
    assert plain[0].ema is None and torch.equal(plain[0].fp.p, gen.fp.p)


def test_broadcast_list_holds_the_average_when_on_and_is_unchanged_when_off():
    import mocogan_chainer_amd.step as step
    for net in _models(seed=7):
        today = [net.fp.p, net.fp.m, net.fp.v] + list(net.running.values())          # what train.py broadcast before the average existed
        got = step.replica_tensors(net)
        assert len(got) == len(today) and all(a is b for a, b in zip(got, today))
        assert step.replica_counters(net) == [net.t] + [net.bn_count[k] for k in sorted(net.bn_count)]
    gen, di, dv = _models(seed=7)
    step.TrainStep('normal', gen, di, dv, ema_decay=0.9)
    got = step.replica_tensors(gen)
    today = [gen.fp.p, gen.fp.m, gen.fp.v] + list(gen.running.values())
    assert all(a is b for a, b in zip(got, today))
    rest = got[len(today):]
    assert rest[0] is gen.fp.e and len(rest) == 1 + len(gen.running)
    assert all(a is b for a, b in zip(rest[1:], gen.ema.running.values()))
    gen.t, gen.ema.k = 5, 3
    cnt = step.replica_counters(gen)
    assert cnt[0] == 5 and cnt[-1] == 3 and len(cnt) == 2 + len(gen.bn_count)
    other = _models(seed=8)[0]
    other.enable_ema(0.9)
    v0 = other.ema.fp.version
    step.set_replica_counters(other, cnt)
    assert (other.t, other.ema.k) == (5, 3) and other.ema.fp.version > v0
    # a world of one: the collective path is inactive and leaves everything as it is
    step.GradExchange().broadcast_replica(gen)
    assert (gen.t, gen.ema.k) == (5, 3)
