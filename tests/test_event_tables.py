"""The host side of the placed-sample mixer, characterised (no GPU): for event lists built from a fixed seed, which entry point
Sample.mix_at_many calls, the bytes of the table and of the segment table it hands over, the track's final byte count and the order of
the source slots; the same lists through Sample._compile_events and CompiledSequence._check_tracks; and every refusal's type and text,
alone and wrapped by compile_tracks.  The expected values are tests/golden/event_tables.json, written by this file's own writer
(``python tests/test_event_tables.py --write``) at the commit the fixture names; the code that packs the tables may be rearranged, the
bytes may not move.

Under the fake library every entry point answers 0 and copies nothing, so an event whose ``other`` is the track itself runs its chain
(copy, clip, reverse, the unrolled loop, speed, envelope, balance, volume, mix_at) as library calls whose NAMES are recorded, in order, beside the
tables of the batches in front of and behind it -- what those calls compute is tests/test_gpu_sequence.py's and its siblings'.

An AssertionError carries no text, so the refusals that are assertions are told apart by their case alone; every other refusal's text
must come from a case of its own."""
import ctypes as C
import hashlib
import itertools
import json
import random
import sys
from pathlib import Path

import pytest

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from synthesizer_amd import _native as N
from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample

GOLDEN = Path(__file__).resolve().parent / "golden" / "event_tables.json"
RATE = 8000
nan, inf = float("nan"), float("inf")
ROW_BYTES = {"sh_mix_events": 40, "sh_mix_events_rate": 56, "sh_mix_events_pan": 80, "sh_mix_events_env": 88, "sh_mix_events_loop": 104,
             "sh_mix_events_rev": 112, "sh_mix_events_chan": 112}          # include/synthhip.h; N.SEQ_LEVELS' order
ENTRIES = list(ROW_BYTES)
SEGMENTED = set(ENTRIES[3:])                                # these take (segments, nsegments) behind the table, and nchannels
SEGMENT_BYTES = 56
PLAIN, RATE_, PAN, ENV, LOOP, REV, CHAN = range(7)


def _sha(raw) -> str:
    return hashlib.sha256(bytes(raw)).hexdigest()


class _Buf:
    """N.DeviceBuffer without a device: a size and a handle that names it"""
    ids = itertools.count(1)

    def __init__(self, nbytes=0):
        self.nbytes = nbytes
        self.handle = next(self.ids)

    @classmethod
    def from_bytes(cls, data):
        return cls(len(data))

    def zero(self, *_a):
        pass


class _Lib:
    """Every entry point answers 0; the names of the calls are kept, and of a sh_mix_events* call what it was handed"""

    def __init__(self):
        self.calls = []
        self.mixes = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name in ROW_BYTES:
                srcs, nsrcs, table, nrows = args[:4]
                rest = args[4:]
                segments = None
                if name in SEGMENTED:
                    segments = bytes((C.c_char * (rest[1] * SEGMENT_BYTES)).from_address(rest[0])) if rest[1] else b""
                    rest = rest[2:]
                self.mixes.append({"entry": name, "rows": nrows, "table": _sha((C.c_char * (nrows * ROW_BYTES[name])).from_address(table)),
                                   "segments": None if segments is None else _sha(segments),
                                   "nsegments": None if segments is None else len(segments) // SEGMENT_BYTES,
                                   "scalars": [int(v) for v in rest[:-2]] + [int(rest[-1])],       # width (, nchannels), the track's samples
                                   "slots": [int(srcs[i]) for i in range(nsrcs)]})
            return 0
        return call


class _faked:
    """N.lib and N.DeviceBuffer replaced for the length of a ``with`` block"""

    def __enter__(self):
        self.patch = pytest.MonkeyPatch()
        lib = _Lib()
        self.patch.setattr(N, "lib", lambda: lib)
        self.patch.setattr(N, "DeviceBuffer", _Buf)
        return lib

    def __exit__(self, *_exc):
        self.patch.undo()


def _track(width, nch, frames=0, rate=RATE):
    return Sample.from_raw_frames(bytes(width * nch * frames), width, rate, nch, name="track")


def _instruments(width):
    """three mono and three stereo instruments of 0.1 s and more: m0 m1 m2, s0 s1 s2"""
    return {"%s%d" % ("ms"[nch - 1], k): Sample.from_raw_frames(bytes(width * nch * n), width, RATE, nch, name="%s%d" % ("ms"[nch - 1], k))
            for nch in (1, 2) for k, n in enumerate((1000, 801, 933))}


# ---- the lists -----------------------------------------------------------------------------------------------------------------------------
def _event(rng, level, width, tnch, inst):
    """one event whose highest attribute is ``level``, the attributes below it by chance, with values that pass every check"""
    pick = lambda values: values[int(rng.random() * len(values))]
    has = {level} | {k for k in range(1, level) if rng.random() < 0.4}
    if CHAN in has or tnch == 1:
        has.discard(PAN)
    if width == 3:
        has.discard(ENV)
    other = inst[("m" if PAN in has or (tnch == 1 and CHAN not in has) else "s") + str(int(rng.random() * 3))]
    seconds = round(rng.random(), 4)
    volume = pick([None, None, 0.5, 1.0, -0.75, 1.5])
    other_seconds = pick([None, None, None, 0.004, 0.0131, 0.05, 0.5])
    speed = pick([0.5, 0.75, 1.5, 2.0, 2 ** (5 / 12), 2 ** (-7 / 12)]) if RATE_ in has else pick([None, None, 1.0, 1.00001])
    pan = pick([-1.0, -0.3, 0.0, 0.45, 1, (1.0, 0.0), [0.25, 0.75], (0.0, 1.0)]) if PAN in has else None
    envelope = None
    if ENV in has:
        envelope = (round(0.001 + 0.004 * rng.random(), 4), pick([0.0, 0.002, 0.004]), pick([0.3, 0.5, 1.0, 0.0]), pick([0.0, 0.001, 0.004]))
        if rng.random() < 0.5:
            envelope += (pick([0.025, 0.0301, 0.04]),)
    loop = None
    if LOOP in has:
        first = pick([0.005, 0.0101, 0.02])
        last = first + pick([0.005, 0.0123, 0.03])
        loop = (first, last, pick([0.05, 0.1234, 0.3, 0.03, 0.03]))
    region = None
    if rng.random() < 0.35:
        first = pick([0.0, 0.0101, 0.03])
        region = (first, pick([None, first + 0.06, first + 0.0899]))
    reverse = pick([True, 1]) if REV in has else pick([None, False, 0])
    channels = pick([(0.5, 0.5), (1.0, 0.0), [0.25, 1.5], (-1.0, 1.0), (1.0, 1.0)]) if CHAN in has else None
    ev = (seconds, other, volume, other_seconds, speed, pan, envelope, loop, region, reverse, channels)
    used = max(k for k, v in enumerate(ev) if k < 2 or v is not None) + 1
    return ev[:used] if rng.random() < 0.5 else ev                 # (the short forms of an event as well as the full one)


def _levelled_lists():
    """for each level, width and channel count that can hold it, two lists of 5 .. 12 events: one or two rows of that level, the rest lower"""
    out = {}
    for level, width, tnch, variant in itertools.product(range(7), (1, 2, 3, 4), (1, 2), (0, 1)):
        if (level == PAN and tnch == 1) or (level == ENV and width == 3):
            continue
        rng = random.Random(1000 * level + 100 * width + 10 * tnch + variant)
        inst = _instruments(width)
        n = 5 + int(rng.random() * 8)
        top = {int(rng.random() * n) for _ in range(1 + variant)}
        events = [_event(rng, level if k in top else int(rng.random() * level), width, tnch, inst) for k in range(n)]
        out["level %s, width %d, %s, %d" % (N.SEQ_LEVELS[level], width, ("mono", "stereo")[tnch - 1], variant)] = (
            width, tnch, (0, 4000)[variant], inst, events)
    return out


def _attribute_lists():
    """per attribute, the variants the packing branches on"""
    out = {}
    env4, env5 = (0.008, 0.008, 0.5, 0.004), (0.008, 0.008, 0.5, 0.004, 0.03)
    for width in (2, 4):
        i = _instruments(width)
        m, s, m1, s1 = i["m0"], i["s0"], i["m1"], i["s1"]

        def add(name, tnch, frames, events):
            out["%s, width %d" % (name, width)] = (width, tnch, frames, i, events)
        add("pan as a float and as a pair", 2, 0, [(0.1, m, None, None, None, 0.3), (0.2, m, 0.5, None, None, (1.0, 0.0)), (0.0, s),
                                                   (0.3, m1, None, None, None, -1.0), (0.3, m1, None, None, None, [0.25, 0.75]), (0.05, m, None, 0.01, None, 1)])
        add("envelopes cut inside a segment, mono", 1, 0, [(0.1, m, None, cut, None, None, env) for env in (env4, env5)
                                                          for cut in (None, 0.004, 0.012, 0.05, 0.028, 0.5)])
        add("envelopes cut inside a segment, stereo and panned", 2, 4000, [(0.1, o, 0.5, cut, speed, pan, env) for env in (env4, env5)
                                                                          for cut in (0.004, 0.0121, 0.028) for o, pan in ((s, None), (m, 0.25))
                                                                          for speed in (None, 1.5)])
        add("an envelope without a ramp and one of sustain level 1", 1, 0, [(0.0, m, None, None, None, None, (0.0, 0.0, 0.5, 0.0)),
                                                                        (0.0, m, None, None, None, None, (0.0, 0.0, 1.0, 0.0)),
                                                                        (0.0, m, None, 0.0001, None, None, (0.01, 0.0, 1.0, 0.0))])
        add("regions alone: the plain entry point", 2, 0, [(0.1, s, None, None, None, None, None, None, (0.01, None)), (0.0, s1),
                                                           (0.2, s, 0.5, None, None, None, None, None, (0.05, 0.05)),
                                                           (0.25, s1, None, None, None, None, None, None, (0.2, 0.5)),
                                                           (0.3, s, None, 0.01, None, None, None, None, (0.0, 0.06), False)])
        add("regions beside a speed", 1, 0, [(0.1, m, None, None, 1.5, None, None, None, (0.01, None)), (0.0, m1, None, None, None, None, None, None, (0.02, 0.09)),
                                             (0.2, m, None, None, 0.5, None, None, None, (0.05, 0.05))])
        add("an empty region alone in an empty track", 1, 0, [(0.0, m, None, None, None, None, None, None, (0.05, 0.05))])
        add("region, reverse and loop: the region moves back", 2, 4000, [(0.1, s, None, None, speed, None, None, loop, region, True)
                                                                         for speed in (None, 2.0) for loop in (None, (0.01, 0.03, 0.2), (0.01, 0.05, 0.03))
                                                                         for region in (None, (0.01, 0.09), (0.02, None))])
        add("reverse beside a pan", 2, 0, [(0.1, m, None, None, None, 0.5, None, (0.01, 0.02, 0.1), (0.01, 0.08), True), (0.0, s, None, None, None, None, None, None, None, True)])
        add("loops with V <= E beside loops that run", 1, 4000, [(0.1, m, None, None, None, None, None, (0.01, 0.05, 0.03)), (0.2, m1, 0.5, None, 1.5, None, None, (0.01, 0.05, 0.05)),
                                                                 (0.0, m, None, 0.01, None, None, env5, (0.005, 0.5, 0.4)), (0.3, m)])
        add("a downmix with and without an envelope", 1, 0, [(0.1, s, None, None, None, None, None, None, None, None, (0.5, 0.5)),
                                                             (0.2, s, 0.5, 0.012, 1.5, None, env5, None, None, None, (1.0, 0.0)),
                                                             (0.0, s1, None, None, None, None, env4, (0.01, 0.03, 0.2), (0.01, 0.09), True, [0.25, 0.75]), (0.3, m)])
        add("a balance with and without an envelope", 2, 0, [(0.1, s, None, None, None, None, None, None, None, None, (0.5, 0.25)),
                                                             (0.2, s, 0.5, 0.012, 1.5, None, env5, None, None, None, (1.0, 0.0)),
                                                             (0.0, s1, None, None, None, None, env4, (0.01, 0.03, 0.2), (0.01, 0.09), True, (1.0, 1.0)),
                                                             (0.3, m, None, None, None, -0.5, env4), (0.35, s)])
        add("speeds that are none", 2, 0, [(0.1, s, None, None, 1.00001), (0.2, s, None, None, 1.0), (0.0, s1, 0.5, None, None)])
        add("speeds that are none beside one that is", 2, 0, [(0.1, s, None, None, 1.00001), (0.2, s, None, None, 1.0), (0.0, s1, 0.5, None, 1.0001)])
        add("nothing grows: in place", 1, 4000, [(0.0, m), (0.3, m1, 0.5)])
        add("an empty list", 1, 4000, [])
        add("an empty other into an empty track", 1, 0, [(0.0, _track(width, 1))])
        add("the sources' slots, in order of first use", 1, 0, [(0.0, i["m2"]), (0.1, m), (0.2, i["m2"]), (0.3, m1), (0.4, m)])
    return out


def _self_lists():
    """lists with events whose ``other`` is the track: the batch is cut there.  (name, width, channels, frames, builder(track, instruments))"""
    env4 = (0.008, 0.008, 0.5, 0.004)
    return {
        "the track itself, plain": (2, 1, 4000, lambda t, i: [(0.0, i["m0"]), (0.1, t), (0.2, i["m1"], 0.5), (0.7, t, 0.5, 0.1)]),
        "the track itself: region, reverse, loop": (2, 2, 4000, lambda t, i: [(0.0, i["s0"], None, None, 1.5), (0.6, t, None, None, None, None, None, (0.01, 0.05, 0.3), (0.1, 0.4), True),
                                                                            (0.2, i["m0"], None, None, None, 0.5), (1.0, t, None, None, None, None, None, None, (0.2, None))]),
        "the track itself: speed, envelope, balance, volume": (2, 2, 4000, lambda t, i: [(0.0, i["s0"]), (0.5, t, 0.5, 0.2, 1.5, None, env4 + (0.1,), None, None, None, (0.5, 1.0)), (0.1, i["s1"], None, None, None, None, env4)]),
        "the track itself first and last": (4, 1, 800, lambda t, i: [(0.05, t), (0.0, i["m0"], None, None, None, None, None, None, None, True), (0.3, t, None, None, None, None, None, None, None, True)]),
    }


def _names(inst, events):
    """handle -> name of every sample the list can have taken a buffer of"""
    return {o._device().handle: o.name for o in list(inst.values()) + [ev[1] for ev in events]}


def _mixed(width, tnch, frames, inst, events, track=None):
    """the list through Sample.mix_at_many under the fake library"""
    with _faked() as lib:
        track = track if track is not None else _track(width, tnch, frames)
        track.mix_at_many(events)
        names = _names(inst, events)
        for mix in lib.mixes:
            mix["slots"] = [names[h] for h in mix["slots"]]
        return {"calls": lib.calls, "mixes": lib.mixes, "nbytes": len(track) * width * tnch}


def _compiled(width, tnch, inst, events):
    """the list through Sample._compile_events: the top layout, whatever the list holds"""
    with _faked():
        bufs, table, segtab, nbytes = _track(width, tnch)._compile_events(events)
        names = _names(inst, events)
        return {"rows": len(table), "row_bytes": table.dtype.itemsize, "table": _sha(table.tobytes()),
                "segments": None if segtab is None else _sha(segtab.tobytes()), "nsegments": None if segtab is None else len(segtab),
                "nbytes": nbytes, "slots": [names[b.handle] for b in bufs]}


def _tracked(width, tnch, inst, tracks):
    with _faked():
        bufs, table, segtab, nbytes, track_first = mixer.CompiledSequence._check_tracks(_track(width, tnch), tracks)
        names = _names(inst, [ev for events in tracks for ev in events])
        return {"rows": len(table), "row_bytes": table.dtype.itemsize, "table": _sha(table.tobytes()),
                "segments": None if segtab is None else _sha(segtab.tobytes()), "nsegments": None if segtab is None else len(segtab),
                "nbytes": nbytes, "slots": [names[b.handle] for b in bufs], "track_first": track_first}


def _dealt(events, ntracks):
    """the list dealt into ``ntracks`` tracks, the second of several left empty"""
    tracks = [[] for _ in range(ntracks)]
    live = [t for t in range(ntracks) if t != 1 or ntracks == 1]
    for k, ev in enumerate(events):
        tracks[live[k * 7 % len(live)]].append(ev)
    return tracks


def cases() -> dict:
    out = {}
    lists = dict(_levelled_lists(), **_attribute_lists())
    for name, (width, tnch, frames, inst, events) in lists.items():
        out["mix: " + name] = _mixed(width, tnch, frames, inst, events)
        out["compile: " + name] = _compiled(width, tnch, inst, events)
    for k, (name, (width, tnch, frames, inst, events)) in enumerate(lists.items()):
        if k % 9 == 0 or name.startswith(("a downmix", "a balance", "envelopes cut")):
            for ntracks in (1, 3, 32):
                out["tracks (%d): %s" % (ntracks, name)] = _tracked(width, tnch, inst, _dealt(events, ntracks))
    for name, (width, tnch, frames, build) in _self_lists().items():
        inst = _instruments(width)
        with _faked():
            track = _track(width, tnch, frames)
        out["mix: " + name] = _mixed(width, tnch, frames, inst, build(track, inst), track=track)
    return out


# ---- the refusals --------------------------------------------------------------------------------------------------------------------------
def _refusal_events():
    """name -> (width, channels, rate of the track, event): one fault each, then two faults each (the first check in _check_events'
    order wins)"""
    i2, i3, i1 = _instruments(2), _instruments(3), _instruments(1)
    m, s = i2["m0"], i2["s0"]
    env = (0.008, 0.008, 0.5, 0.004)
    slow_m, slow_s = Sample.from_raw_frames(bytes(2 * 100), 2, 2, 1), Sample.from_raw_frames(bytes(4 * 100), 2, 2, 2)
    fast_s = Sample.from_raw_frames(bytes(4 * 100), 2, 2 ** 20, 2)
    E = lambda seconds, other, volume=None, other_seconds=None, speed=None, pan=None, envelope=None, loop=None, region=None, reverse=None, channels=None: (
        seconds, other, volume, other_seconds, speed, pan, envelope, loop, region, reverse, channels)
    one = {
        "another sample width": (2, 1, RATE, E(0.1, i1["m0"])),
        "another sample rate": (2, 1, RATE, E(0.1, slow_m)),
        "a stereo other in a mono track": (2, 1, RATE, E(0.1, s)),
        "pan and channels": (2, 2, RATE, E(0.1, s, pan=0.3, channels=(0.5, 0.5))),
        "channels: a number": (2, 1, RATE, E(0.1, s, channels=0.5)),
        "channels: a pair of strings": (2, 1, RATE, E(0.1, s, channels=("a", "b"))),
        "channels: a factor that is no number": (2, 1, RATE, E(0.1, s, channels=(nan, 0.5))),
        "channels on a mono sample": (2, 1, RATE, E(0.1, m, channels=(0.5, 0.5))),
        "channels into four channels": (2, 4, RATE, E(0.1, s, channels=(1.0, 1.0))),
        "pan on a stereo sample": (2, 2, RATE, E(0.1, s, pan=0.3)),
        "pan into a mono track": (2, 1, RATE, E(0.1, m, pan=0.3)),
        "pan: three numbers": (2, 2, RATE, E(0.1, m, pan=(0.1, 0.2, 0.3))),
        "pan beyond 1": (2, 2, RATE, E(0.1, m, pan=1.5)),
        "pan: an infinite factor": (2, 2, RATE, E(0.1, m, pan=(inf, 0.5))),
        "a negative time": (2, 1, RATE, E(-0.1, m)),
        "a negative other_seconds": (2, 1, RATE, (0.1, m, None, -0.01)),
        "a volume that is no number": (2, 1, RATE, (0.1, m, nan)),
        "a speed beyond 10": (2, 1, RATE, E(0.1, m, speed=11.0)),
        "a speed that leaves no sample rate": (2, 1, 2, E(0.1, slow_m, speed=0.1)),
        "an envelope on 24-bit samples": (3, 1, RATE, E(0.1, i3["m0"], envelope=env)),
        "envelope: three numbers": (2, 1, RATE, E(0.1, m, envelope=env[:3])),
        "envelope: a negative attack": (2, 1, RATE, E(0.1, m, envelope=(-0.01,) + env[1:])),
        "envelope: a sustain level above 1": (2, 1, RATE, E(0.1, m, envelope=(0.01, 0.01, 1.5, 0.01))),
        "envelope: a release longer than the sustain": (2, 1, RATE, E(0.1, m, envelope=(0.05, 0.05, 0.5, 0.45))),
        "a downmix beyond what the kernels address": (2, 1, 2 ** 20, E((2 ** 31 - 32768 - 99) / 2 ** 20, fast_s, channels=(0.5, 0.5))),
        "loop: two numbers": (2, 1, RATE, E(0.1, m, loop=(0.01, 0.02))),
        "loop: a negative length": (2, 1, RATE, E(0.1, m, loop=(0.01, 0.02, -1.0))),
        "loop: a string": (2, 1, RATE, E(0.1, m, loop=(0.01, "a", 1.0))),
        "loop: no frame between": (2, 1, RATE, E(0.1, m, loop=(0.05, 0.05, 1.0))),
        "loop: more than one call can address": (2, 2, RATE, E(0.1, s, loop=(0.01, 0.02, 2 ** 31 / RATE))),
        "region: a number": (2, 1, RATE, E(0.1, m, region=0.5)),
        "region: an infinite start": (2, 1, RATE, E(0.1, m, region=(inf, None))),
        "region: an end before the start": (2, 1, RATE, E(0.1, m, region=(0.03, 0.02))),
        "region: a start behind the sample and no end": (2, 1, RATE, E(0.1, m, region=(0.2, None))),
        "an empty region with a loop": (2, 1, RATE, E(0.1, m, loop=(0.0, 0.01, 0.1), region=(0.05, 0.05))),
    }
    two = {
        "pan and channels, and a negative time": (2, 2, RATE, E(-0.1, s, pan=0.3, channels=(0.5, 0.5))),
        "channels that are no pair, on a mono sample": (2, 1, RATE, E(0.1, m, channels=(0.5,))),
        "pan beyond 1 and a negative time": (2, 2, RATE, E(-0.1, m, pan=-1.5)),
        "a negative time and a volume that is no number": (2, 1, RATE, E(-0.1, m, volume=inf)),
        "a volume that is no number and a speed beyond 10": (2, 1, RATE, E(0.1, m, volume=nan, speed=11.0)),
        "a speed below 0.1 and a region that is no pair": (2, 1, RATE, E(0.1, m, speed=0.05, region=(0.1,))),
        "a region that ends before it starts and a loop of two numbers": (2, 1, RATE, E(0.1, m, loop=(0.1, 0.2), region=(0.03, 0.02))),
        "a loop without a frame and an envelope of three numbers": (2, 1, RATE, E(0.1, m, envelope=env[:3], loop=(0.05, 0.05, 1.0))),
        "a loop of two numbers and an envelope, 24-bit": (3, 1, RATE, E(0.1, i3["m0"], envelope=env, loop=(0.1, 0.2))),
        "an envelope on 24-bit samples that is no envelope": (3, 1, RATE, E(0.1, i3["m0"], envelope=0.5)),
        "a sustain level above 1 and a release too long": (2, 1, RATE, E(0.1, m, envelope=(0.05, 0.05, 1.5, 0.45))),
        "a release too long on a downmix too far": (2, 1, 2 ** 20, E((2 ** 31 - 32768 - 99) / 2 ** 20, fast_s, envelope=(0.0, 0.0, 0.5, 1.0), channels=(0.5, 0.5))),
        "another sample rate and a negative time": (2, 2, RATE, E(-0.1, slow_s)),
    }
    return one, two


def _raised(fn):
    try:
        fn()
    except (ValueError, NotImplementedError, AssertionError) as e:
        return {"type": type(e).__name__, "message": str(e)}
    return {"type": None, "message": None}


def refusals() -> dict:
    """every refusal before anything is mixed: alone in a list, behind a good event, and as compile_tracks words it; then the two that
    the track as its own source raises only when that event runs"""
    out = {}
    one, two = _refusal_events()

    def refuse(*_a, **_k):
        raise RuntimeError("the native library was reached")
    patch = pytest.MonkeyPatch()
    patch.setattr(N, "lib", refuse)
    patch.setattr(N, "DeviceBuffer", refuse)
    try:
        for faults, group in ((1, one), (2, two)):
            for name, (width, tnch, rate, ev) in group.items():
                good = (0.0, Sample.from_raw_frames(bytes(width * tnch * 100), width, rate, tnch))
                out["%d: %s" % (faults, name)] = {
                    "alone": _raised(lambda: _track(width, tnch, 4000, rate).mix_at_many([ev])),
                    "behind a good event": _raised(lambda: _track(width, tnch, 0, rate).mix_at_many([good, ev])),
                    "compile_tracks": _raised(lambda: mixer.compile_tracks([[good], [], [good, ev, ev]], rate, tnch, width))}
    finally:
        patch.undo()
    i = _instruments(2)
    with _faked() as lib:
        t = _track(2, 1, 4000)
        out["late: the track's own region ends before it starts"] = dict(
            _raised(lambda: t.mix_at_many([(0.0, i["m0"]), (0.1, t, None, None, None, None, None, None, (0.75, None)), (0.2, i["m1"])])), calls=list(lib.calls))
    with _faked() as lib:
        t = _track(2, 1, 4000)
        out["late: the track's own loop has no frame"] = dict(
            _raised(lambda: t.mix_at_many([(0.0, i["m0"]), (0.1, t, None, None, None, None, None, (0.6, 0.7, 1.0)), (0.2, i["m1"])])), calls=list(lib.calls))
    return out


# ---- the tests -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


@pytest.fixture(scope="module")
def got():
    return {"cases": cases(), "refusals": refusals()}


def test_every_case_reproduces_byte_for_byte(golden, got):
    assert sorted(got["cases"]) == sorted(golden["cases"])
    wrong = [name for name in golden["cases"] if got["cases"][name] != golden["cases"][name]]
    assert not wrong, (len(wrong), wrong[0], got["cases"][wrong[0]], golden["cases"][wrong[0]])


def test_every_refusal_reproduces_type_and_text(golden, got):
    assert sorted(got["refusals"]) == sorted(golden["refusals"])
    wrong = [name for name in golden["refusals"] if got["refusals"][name] != golden["refusals"][name]]
    assert not wrong, (len(wrong), wrong[0], got["refusals"][wrong[0]], golden["refusals"][wrong[0]])


def test_the_fixture_has_no_hole(golden):
    """every entry point in at least 8 cases; every case of every layer a call; every refusal a refusal, its text from a case of its own"""
    seen = {entry: 0 for entry in ENTRIES}
    for name, case in golden["cases"].items():
        if name.startswith("mix: "):
            for entry in {m["entry"] for m in case["mixes"]}:
                seen[entry] += 1
        else:
            assert case["row_bytes"] == ROW_BYTES["sh_mix_events_chan"]
    assert all(n >= 8 for n in seen.values()), seen
    assert sum(name.startswith("compile: ") for name in golden["cases"]) >= 100
    firsts = [case["track_first"] for name, case in golden["cases"].items() if name.startswith("tracks")]
    assert {len(f) - 1 for f in firsts} == {1, 3, 32} and any(f[1] == f[2] for f in firsts if len(f) > 2)
    assert any(len(case["mixes"]) > 1 and "sh_pcm_reverse" in case["calls"] for case in golden["cases"].values() if "mixes" in case)
    texts = {}
    for name, r in golden["refusals"].items():
        if name.startswith("late: "):
            assert r["type"] == "ValueError" and "as the events before left it" in r["message"] or "the track as the events before" in r["message"]
            assert any(c.startswith("sh_mix_events") for c in r["calls"])              # the events in front of it were mixed
            texts.setdefault(r["message"], []).append(name)
            continue
        assert r["alone"]["type"] in ("ValueError", "NotImplementedError", "AssertionError"), name
        assert r["behind a good event"] == r["alone"], name
        if r["alone"]["type"] == "AssertionError":
            assert r["compile_tracks"] == r["alone"], name                              # mix_at's assertions stay assertions, unwrapped
        else:
            assert r["compile_tracks"] == {"type": r["alone"]["type"], "message": "compile_tracks: track 2, event 1: " + r["alone"]["message"]}, name
        if name.startswith("1: ") and r["alone"]["type"] != "AssertionError":
            texts.setdefault(r["alone"]["message"], []).append(name)
    assert all(len(names) <= 2 for names in texts.values()), [n for n in texts.values() if len(n) > 2]
    assert len(texts) >= 30, len(texts)
    assert sum(r["alone"]["type"] == "AssertionError" for n, r in golden["refusals"].items() if n.startswith("1: ")) == 3
    assert sum(name.startswith("2: ") for name in golden["refusals"]) >= 6
    single = {r["alone"]["message"].split("(")[0] for n, r in golden["refusals"].items() if n.startswith("1: ")}
    assert all(r["alone"]["message"].split("(")[0] in single for n, r in golden["refusals"].items() if n.startswith("2: "))    # the winner is a known text


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_event_tables.py --write")
    import subprocess
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=str(GOLDEN.parent), capture_output=True, text=True).stdout.strip()
    rows = lambda d: "{\n%s\n}" % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"), sort_keys=True)) for k, v in sorted(d.items()))
    GOLDEN.write_text('{"generated_at": "%s",\n"cases": %s,\n"refusals": %s}\n' % (commit, rows(cases()), rows(refusals())))
    print("wrote %s: %d bytes" % (GOLDEN, GOLDEN.stat().st_size))
