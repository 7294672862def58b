"""What a piece of host code enqueues, and how it orders its streams -- recorded, not timed.

    with launch_trace.Recorder() as tr:
        ts.run(x, t)
    tr.entries            # [('mcg_pack_clip', 'main'), ('wait_stream', 's1', 'main'), ('record', 'e0', 's1'), ...]

For the duration of the block every entry point of the library that is reached through hiplib.load() is logged with the stream that
is current at the call, and every outermost Stream.wait_stream / Stream.wait_event / Event.record / Tensor.record_stream with its
streams and events.  Streams and events are named by their ordinal of first appearance ('s1', 's2', ...; 'e0', 'e1', ...), the
stream that is current on entry is 'main': no pointer and no object id enters a trace, so two runs of the same host code give the
same trace.  ExchangeStub stands in for step.GradExchange (no process group) and logs which slices of a flat gradient travel.

The numerical tests can pass by luck of timing when a wait is dropped; a trace cannot.  It touches only public seams (hiplib._lib,
the torch.cuda classes), so it records any revision of the package alike."""
import json

import torch

_active = None


def _log(*entry):
    if _active is not None:
        _active.entries.append(tuple(entry))


class _LibProxy:
    """hiplib's typed library with every mcg_* entry point logged as (name, current stream) before it runs"""

    def __init__(self, lib, rec):
        self._lib, self._rec = lib, rec

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('mcg_'):
            return fn
        rec = self._rec

        def call(*args):
            rec.entries.append((name, rec.stream(torch.cuda.current_stream())))
            return fn(*args)
        return call


class ExchangeStub:
    """step.GradExchange's surface as TrainStep.run uses it: start() logs (storage offset, element count) of the slice and returns
    a handle, finish() logs the handle"""
    active = True
    grad_scale = 1.0

    def __init__(self):
        self.started = 0

    def start(self, flat_grad):
        _log('start', flat_grad.storage_offset(), flat_grad.numel())
        self.started += 1
        return 'h%d' % (self.started - 1)

    def finish(self, handle):
        _log('finish', handle)


class Recorder:
    def __init__(self):
        self.entries = []
        self._streams, self._events, self._keep = {}, {}, []
        self._depth = 0

    def stream(self, s):
        return self._streams.setdefault(s.cuda_stream, 's%d' % len(self._streams))

    def event(self, e):
        if id(e) not in self._events:
            self._keep.append(e)                                  # (alive until the trace ends: its id names no other event)
            self._events[id(e)] = 'e%d' % len(self._events)
        return self._events[id(e)]

    def _outermost(self, orig, describe):
        rec = self

        def method(this, *args, **kw):
            if rec._depth == 0:
                rec.entries.append(describe(this, *args, **kw))
            rec._depth += 1
            try:
                return orig(this, *args, **kw)
            finally:
                rec._depth -= 1
        return method

    def __enter__(self):
        global _active
        import mocogan_chainer_amd.hiplib as hl
        assert _active is None, "one trace at a time"
        self._hl, self._lib = hl, hl.load()
        self._streams[torch.cuda.current_stream().cuda_stream] = 'main'
        S, E, T = torch.cuda.Stream, torch.cuda.Event, torch.Tensor
        cur = torch.cuda.current_stream
        patches = [
            (S, 'wait_stream', lambda this, other: ('wait_stream', self.stream(this), self.stream(other))),
            (S, 'wait_event', lambda this, ev: ('wait_event', self.stream(this), self.event(ev))),
            (E, 'record', lambda this, stream=None: ('record', self.event(this), self.stream(stream if stream is not None else cur()))),
            (T, 'record_stream', lambda this, stream: ('record_stream', self.stream(stream), this.numel())),
        ]
        self._saved = []
        for cls, name, describe in patches:
            self._saved.append((cls, name, cls.__dict__.get(name)))
            setattr(cls, name, self._outermost(getattr(cls, name), describe))
        hl._lib = _LibProxy(self._lib, self)
        _active = self
        return self

    def __exit__(self, *exc):
        global _active
        _active = None
        self._hl._lib = self._lib
        for cls, name, own in self._saved:
            if own is None:
                delattr(cls, name)                                # (inherited, e.g. Tensor.record_stream: the base's shows again)
            else:
                setattr(cls, name, own)
        self._keep = []
        return False


# ---- a set of traces as a small file: one table of the strings, entries as lists of indices into it ---------------------------
def encode(traces):
    names, index = [], {}

    def ix(v):
        v = str(v)
        if v not in index:
            index[v] = len(names)
            names.append(v)
        return index[v]
    body = {key: [[ix(v) for v in entry] for entry in entries] for key, entries in traces.items()}
    return {'names': names, 'traces': body}


def decode(doc):
    names = doc['names']
    return {key: [tuple(names[i] for i in entry) for entry in entries] for key, entries in doc['traces'].items()}


def normalise(entries):
    """a recorded trace in the form decode() gives: every field a string"""
    return [tuple(str(v) for v in entry) for entry in entries]


def save(path, traces, **header):
    with open(path, 'w') as f:
        json.dump(dict(header, **encode(traces)), f, separators=(',', ':'))
        f.write('\n')


def load(path):
    with open(path) as f:
        return decode(json.load(f))
