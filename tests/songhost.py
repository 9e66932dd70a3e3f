"""The fake native layer of the compiled song's host tests (tests/test_*_host.py; no GPU): device buffers, ``N.Sequence`` and
``N.SeqAutomation`` as the mixer sees them, the library by entry point, the small songs the tests compile and the ways a keyword reaches a
render.  A helper module: it holds no test."""
import numpy as np

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample

RATE = 8000


def _mono(n=1000, width=2):
    return Sample.from_raw_frames(bytes(width * n), width, RATE, 1)


def _stereo(n=1000, width=2):
    return Sample.from_raw_frames(bytes(2 * width * n), width, RATE, 2)


class _Buf:
    handle = None

    def __init__(self, nbytes=0):
        self.nbytes = nbytes

    @classmethod
    def from_bytes(cls, data):
        return cls(len(data))

    def zero(self, *_a):
        pass


class _StemBuf(_Buf):
    """a device buffer as the mixer sees it: every one that was made, and every view that was cut from it"""
    made = []

    def __init__(self, nbytes=0):
        _Buf.__init__(self, nbytes)
        self.views, self.parent = [], None
        _StemBuf.made.append(self)

    def view(self, offset, nbytes):
        v = _StemBuf.__new__(_StemBuf)
        v.nbytes, v.views, v.parent = nbytes, [], self
        self.views.append((offset, nbytes))
        return v


def _fake(monkeypatch):
    from tests.test_channels_host import _ChanLib            # (the library of mix_at_many's host tests, which import this module)
    lib = _ChanLib()
    monkeypatch.setattr(N, "lib", lambda: lib)
    monkeypatch.setattr(N, "DeviceBuffer", _Buf)
    return lib


class _Seq:
    """N.Sequence as the mixer sees it: what each render was handed"""

    def __init__(self, sources, table, segments, width, nchannels, track_samples, track_first=None):
        self.rendered = []

    def info(self):
        return {"level": 0, "device_bytes": 0}

    def render(self, first_sample, nsamples, out, out_sample=0, **kw):
        self.rendered.append((first_sample, nsamples, out_sample, kw))
        if kw.get("meters"):
            return [((0, 0), (0, 0))] * 4

    def free(self):
        pass


class _ClipSeq(_Seq):
    """_Seq, whose history is the array N.Sequence.render hands back -- with the field ``clipped`` where clips=True"""

    def render(self, first_sample, nsamples, out, out_sample=0, **kw):
        if kw.get("meters") == "history":
            self.rendered.append((first_sample, nsamples, out_sample, kw))
            nblocks = (first_sample + nsamples - 1) // 2048 - first_sample // 2048 + 1
            blocks = np.zeros((nblocks, 4 + len(kw.get("groups") or ())), dtype=N.SEQ_METER_CLIPS_DTYPE if kw.get("clips") else N.SEQ_METER_DTYPE)
            blocks["peak"][:, :, 0] = np.arange(nblocks)[:, None] + first_sample // 2048
            if kw.get("clips"):
                blocks["clipped"][:, :, 0] = 10 * (np.arange(nblocks)[:, None] + first_sample // 2048) + np.arange(blocks.shape[1])[None, :]
                blocks["clipped"][:, :, 1] = 1
            return blocks
        return _Seq.render(self, first_sample, nsamples, out, out_sample, **kw)


class _Lib:
    """the entry points N.Sequence.render reaches, by name, with their arguments"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            if name == "sh_seq_get_tracks":
                args[1]._obj.value = 3
            return 0
        return entry


class _Auto:
    """N.SeqAutomation as the mixer sees it: what it was handed, the arguments behind the third as well"""
    made = []

    def __init__(self, seq, segments, seg_first, *rest):
        self.seq, self.segments, self.seg_first, self.rest, self.freed = seq, segments, seg_first, rest, False
        _Auto.made.append(self)

    def free(self):
        self.freed = True


def _calls(cs, **kw):
    """the ways a keyword reaches a render"""
    return (lambda: cs.render(**kw), lambda: cs.render(3, 0, **kw), lambda: cs.render_into(N.DeviceBuffer(100), 0, 0, 10, **kw),
            lambda: next(cs.chunks(100, **kw)))


def _song(monkeypatch, nch=2, width=2):
    _fake(monkeypatch)
    monkeypatch.setattr(N, "Sequence", _Seq)
    monkeypatch.setattr(N, "SeqAutomation", _Auto)
    del _Auto.made[:]
    a = _stereo(1000, width) if nch == 2 else _mono(1000, width)
    return mixer.compile_tracks([[(0.0, a), (0.5, a, 0.5)], [], [(0.25, a)]], RATE, nch, width)


def _rows(g):
    return [tuple(g[k][f] for f in ("end", "origin", "mul", "slope", "numsamples", "offset", "kind", "reserved")) for k in range(len(g))]


def _piece(v, n, v0, v1):
    """the chain's step on one clip of n samples: Python ints and floats"""
    return [int(x * (k * (v1 - v0) / float(n) + v0)) for k, x in enumerate(v)]


def _clip(rng, width, n):
    bits = 8 * width
    v = rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), n, dtype=np.int64)
    edge = [-(1 << (bits - 1)), (1 << (bits - 1)) - 1, -1][:n]
    v[:len(edge)] = edge
    return v
