"""The reference of the placed-sample mixer (Sample.mix_at_many, mixer.sequence, sh_mix_events*, sh_seq_*), on the CPU alone: live
``audioop`` on byte slices and upstream's ``array`` fades written out.  Nothing here comes from the product.

``source`` is what ``mix_at`` is handed for one event: the documented chain, stated once as STEPS, and every WRONG order as a named
departure from it, so that a test can show that its expected bytes tell the right chain from each of them (``discriminates``).  ``mix`` is
the one placement loop: ``add`` with saturation at every event, in list order, like the loop of ``Sample.mix_at`` calls the product
replaces.  tests/golden/seq_oracle_digests.json pins both to the bytes of the per-file oracles they replaced (tests/test_seq_oracle.py).

There is no rate here: the files use 8000, 8192 and 48000 on purpose and pass their own."""
import array
import audioop
import math

import numpy as np

TILE = {1: 1024, 2: 2048, 3: 1024, 4: 1024}                 # track samples per workgroup
LANE = {1: 4, 2: 8, 3: 4, 4: 4}                             # track samples per lane
OTHER_SCHEME = "1"                                          # SYNTHHIP_SEQ_ALIGN of the scheme that is not the default (include/synthhip.h)
SELF = object()                                             # an event whose source is the track itself, as earlier events left it
TYPECODE = {1: "b", 2: "h", 4: "i"}

# ---- the orders: the right one and, level by level, the wrong ones ---------------------------------------------------------------------
RIGHT = "right"
MUL_BEFORE_RATECV = "mul before ratecv"
MUL_BEFORE_TOSTEREO, FOLDED, STEREO_BEFORE_RATECV = "mul before tostereo", "volume folded into the factors", "tostereo before ratecv"
ENVELOPE_AFTER_MUL, ENVELOPE_AFTER_STEREO = "envelope after mul", "envelope after tostereo"
RAMPS_FLOORED, SUSTAIN_TRUNCATED, K_FRAMES = "ramps floored", "sustain truncated", "k counts frames"
LOOP_AFTER_RATECV, LOOP_AFTER_ENVELOPE = "loop after ratecv", "loop after the envelope"
UNREVERSED, REVERSE_AFTER_LOOP, REVERSE_AFTER_RATECV, REGION_AFTER_REVERSAL = \
    "not reversed", "reverse after the loop", "reverse after ratecv", "the region cut after the reversal"
CHANNELS_BEFORE_ENVELOPE, CHANNELS_BEFORE_REVERSAL, CHANNELS_AFTER_MUL, SWAPPED, N_IN_STEREO = \
    "channels before the envelope", "channels before the reversal", "channels after the mul", "factors swapped", \
    "a downmix's n counted in stereo samples"
ENVELOPE_VARIANTS = (RAMPS_FLOORED, SUSTAIN_TRUNCATED, K_FRAMES)
WRONG = {
    "plain": (),
    "rate": (MUL_BEFORE_RATECV,),
    "pan": (MUL_BEFORE_TOSTEREO, FOLDED, STEREO_BEFORE_RATECV),
    "env": (ENVELOPE_AFTER_MUL, ENVELOPE_AFTER_STEREO) + ENVELOPE_VARIANTS,
    "loop": (LOOP_AFTER_RATECV, LOOP_AFTER_ENVELOPE),
    "rev": (UNREVERSED, REVERSE_AFTER_LOOP, REVERSE_AFTER_RATECV, REGION_AFTER_REVERSAL),
    "chan": (CHANNELS_BEFORE_ENVELOPE, CHANNELS_BEFORE_REVERSAL, CHANNELS_AFTER_MUL, SWAPPED, N_IN_STEREO),
}


def wrong_orders(level, width, nch):
    """the wrong orders of a level that a list of this width and channel count can show: 24-bit samples have no envelope, so no order
    against it; swapped factors are a balance's, a count in stereo samples a downmix's"""
    orders = WRONG[level]
    if level == "chan":
        orders = tuple(o for o in orders if o != (SWAPPED if nch == 1 else N_IN_STEREO) and not (o == CHANNELS_BEFORE_ENVELOPE and width == 3))
    return orders


# ---- the building blocks ----------------------------------------------------------------------------------------------------------------
def pcm(rng, width, nsamples, scale=1.0) -> bytes:
    if width == 3:
        v = rng.integers(int(-8388608 * scale), int(8388607 * scale) + 1, nsamples, dtype=np.int64)
        return (v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    hi = 2 ** (8 * width - 1)
    return rng.integers(int(-hi * scale), int((hi - 1) * scale) + 1, nsamples, dtype=np.int64).astype({1: np.int8, 2: "<i2", 4: "<i4"}[width]).tobytes()


def differs(a: bytes, b: bytes) -> int:
    assert len(a) == len(b)
    return int(np.count_nonzero(np.frombuffer(a, dtype=np.uint8) != np.frombuffer(b, dtype=np.uint8)))


def out_frames(n, inrate, rate):
    return (n - 1) * rate // inrate + 1 if n else 0


def factors(pan):
    if isinstance(pan, tuple):
        return float(pan[0]), float(pan[1])
    return (1.0 - pan) / 2.0, (1.0 + pan) / 2.0           # Sample.pan upstream


def envelope_bytes(frames: bytes, width, nch, rate, attack, decay, sustainlevel, release, variant=RIGHT) -> bytes:
    """upstream's Sample.envelope on a byte string (split, amplify, fadein, fadeout, join as they stand), or one of the WRONG readings
    of its rounding"""
    fb = width * nch

    def frame_idx(seconds):
        return fb * int(rate * seconds)

    def duration(b):
        return len(b) / rate / width / nch

    def split(b, seconds):
        end = frame_idx(seconds)
        return (b[:end], b[end:]) if end != len(b) else (b, b"")

    def amplify(b, factor):
        if variant != SUSTAIN_TRUNCATED:
            return audioop.mul(b, width, factor)            # clamp, then floor
        a = array.array(TYPECODE[width], b)
        for k in range(len(a)):
            a[k] = int(a[k] * factor)
        return a.tobytes()

    def ramped(b, f):
        a = array.array(TYPECODE[width], b)
        numsamples = len(b) / width
        for k in range(int(numsamples)):
            v = a[k] * (f(k // nch, numsamples / nch) if variant == K_FRAMES else f(k, numsamples))
            a[k] = math.floor(v) if variant == RAMPS_FLOORED else int(v)
        return a.tobytes()

    def fadeout(b, seconds, target_volume):
        seconds = min(seconds, duration(b))
        i = frame_idx(duration(b) - seconds)
        decrease = 1.0 - target_volume
        return b[:i] + ramped(b[i:], lambda k, n: 1.0 - k * decrease / n)

    def fadein(b, seconds, start_volume=0.0):
        seconds = min(seconds, duration(b))
        i = frame_idx(seconds)
        increase = 1.0 - start_volume
        return ramped(b[:i], lambda k, n: k * increase / n + start_volume) + b[i:]

    A, D = split(frames, attack)
    D, S = split(D, decay)
    if sustainlevel < 1:
        S = amplify(S, sustainlevel)
    assert duration(S) - release >= 0, "upstream slices from the wrong end here; the product refuses it"
    S, R = split(S, duration(S) - release)
    if attack > 0:
        A = fadein(A, attack)
    if decay > 0:
        D = fadeout(D, decay, sustainlevel)
    if release > 0:
        R = fadeout(R, release, 0.0)
    return A + D + S + R


def loop_frames(loop, rate, frames):
    S, E, V = int(rate * loop[0]), min(int(rate * loop[1]), frames), int(rate * loop[2])
    assert S < E
    return S, E, V


def unroll_frames(data: bytes, fb, S, E, V) -> bytes:
    """the V virtual frames of a looped note, by the frame formula"""
    idx = [v if v < E else S + (v - E) % (E - S) for v in range(V)]
    return np.frombuffer(data, dtype=np.uint8).reshape(-1, fb)[idx].tobytes() if V else b""


def unroll(data: bytes, width, snch, rate, loop) -> bytes:
    fb = width * snch
    return unroll_frames(data, fb, *loop_frames(loop, rate, len(data) // fb))


def cut(data: bytes, width, snch, rate, region) -> bytes:
    """other.copy().clip(region[0], other.duration if region[1] is None else region[1]): byte slicing"""
    fb = width * snch
    end = len(data) / rate / width / snch if region[1] is None else region[1]
    assert end >= region[0]
    return data[fb * int(rate * region[0]):fb * int(rate * end)]


def balance(data: bytes, width, lf, rf) -> bytes:
    """Sample.stereo of a stereo sample: left().amplify(lf).stereo(1, 0) mixed with right().amplify(rf).stereo(0, 1); a last sample
    without its frame is the left one of a frame whose right one is cut off again"""
    odd = len(data) // width % 2
    if odd:
        data = data + bytes(width)
    left = audioop.tostereo(audioop.mul(audioop.tomono(data, width, 1, 0), width, lf), width, 1, 0)
    right = audioop.tostereo(audioop.mul(audioop.tomono(data, width, 0, 1), width, rf), width, 0, 1)
    out = audioop.add(left, right, width)
    return out[:len(out) - width] if odd else out


def weigh(data: bytes, width, nch, lf, rf) -> bytes:
    return audioop.tomono(data, width, lf, rf) if nch == 1 else balance(data, width, lf, rf)


# ---- one event ----------------------------------------------------------------------------------------------------------------------------
# the chain the product documents, in its order: the region cut; the reversal; the loop unrolled; ratecv; the clip to the note's length and
# then the envelope; tostereo for a pan, tomono or the balance for channels; mul; the cut of other_seconds, in track samples
STEPS = ("region", "reverse", "loop", "ratecv", "envelope", "place", "mul", "cut")
# a wrong order that only moves a step: (the step, where it goes, the events it is about -- those with a pan, with channels, or all)
MOVED = {
    MUL_BEFORE_RATECV: ("mul", "before", "ratecv", None),
    MUL_BEFORE_TOSTEREO: ("mul", "before", "place", "pan"),
    STEREO_BEFORE_RATECV: ("place", "before", "ratecv", "pan"),
    ENVELOPE_AFTER_MUL: ("envelope", "after", "mul", None),
    ENVELOPE_AFTER_STEREO: ("envelope", "after", "place", None),
    LOOP_AFTER_RATECV: ("loop", "after", "ratecv", None),
    LOOP_AFTER_ENVELOPE: ("loop", "after", "envelope", None),
    REVERSE_AFTER_LOOP: ("reverse", "after", "loop", None),
    REVERSE_AFTER_RATECV: ("reverse", "after", "ratecv", None),
    REGION_AFTER_REVERSAL: ("region", "after", "reverse", None),
    CHANNELS_BEFORE_ENVELOPE: ("place", "before", "envelope", "channels"),
    CHANNELS_AFTER_MUL: ("mul", "before", "place", "channels"),
}


def source(data, width, rate, nch, *, volume=None, other_seconds=None, speed=None, pan=None, env=None, loop=None, region=None, reverse=None,
           channels=None, order=RIGHT) -> bytes:
    """what mix_at is handed for one event of a track of nch channels -- a source with a pan is mono, one with channels stereo, any other
    has the track's channels -- or, under a WRONG order, what it would be handed if the chain ran that way"""
    assert pan is None or channels is None
    inrate = rate if speed is None else int(rate * speed)
    about = {"pan": pan is not None, "channels": channels is not None, None: True}
    steps = list(STEPS)
    if order in MOVED and about[MOVED[order][3]]:
        step, where, anchor, _about = MOVED[order]
        steps.remove(step)
        steps.insert(steps.index(anchor) + (where == "after"), step)
    if order == UNREVERSED:
        steps.remove("reverse")
    if channels is not None and (order == SWAPPED or (order == CHANNELS_BEFORE_REVERSAL and reverse)):
        channels = channels[::-1]                           # (weighed first and turned round after: lf stays with the stored left)
    c = 1 if pan is not None else 2 if channels is not None else nch        # the channels of the frames as they stand
    for step in steps:
        if step == "region" and region is not None:
            data = cut(data, width, c, rate, region)
        elif step == "reverse" and reverse:
            data = audioop.reverse(data, width)             # the order of the SAMPLES
        elif step == "loop" and loop is not None:
            data = unroll(data, width, c, rate, loop)
        elif step == "ratecv" and inrate != rate:
            data = audioop.ratecv(data, width, c, inrate, rate, None)[0]
        elif step == "envelope" and env is not None:
            if len(env) == 5:
                data = data[:width * c * int(rate * env[4])]                    # clip(0.0, length)
            data = envelope_bytes(data, width, c, rate, *env[:4], variant=order if order in ENVELOPE_VARIANTS else RIGHT)
        elif step == "place" and pan is not None:
            left, right = factors(pan)
            if order == FOLDED:
                v = 1.0 if volume is None else volume
                left, right, volume = left * v, right * v, None
            data, c = audioop.tostereo(data, width, left, right), 2
        elif step == "place" and channels is not None:
            data, c = weigh(data, width, nch, *channels), nch
        elif step == "mul" and volume is not None:
            data = audioop.mul(data, width, volume)
        elif step == "cut" and other_seconds:
            data = data[:width * (2 if order == N_IN_STEREO and channels is not None else nch) * int(rate * other_seconds)]
    return data


# ---- a list -------------------------------------------------------------------------------------------------------------------------------
FIELDS = ("volume", "other_seconds", "speed", "pan", "env", "loop", "region", "reverse", "channels")


def mix(track: bytes, events, width, rate, nch, order=RIGHT) -> bytes:
    """events: (seconds, source bytes | SELF, volume, other_seconds, speed, pan, envelope, loop, region, reverse, channels), the tail from
    `speed` on may be left out; applied one after another like upstream's mix_at"""
    fb = width * nch
    t = bytearray(track)
    for seconds, data, *rest in events:
        frames = source(bytes(t) if data is SELF else data, width, rate, nch, order=order, **dict(zip(FIELDS, rest)))
        start = fb * int(rate * seconds)
        end = start + len(frames)
        if end > len(t):
            t.extend(bytes(end - len(t)))
        t[start:end] = audioop.add(bytes(t[start:end]), frames, width)
    return bytes(t)


def discriminates(want, events, width, rate, nch, level, base=b""):
    """the expected bytes differ from each wrong order's of the level: on the CPU, with audioop alone, before the GPU is asked"""
    found = {}
    for order in wrong_orders(level, width, nch):
        b = mix(base, events, width, rate, nch, order)
        m = min(len(want), len(b))
        found[order] = differs(want[:m], b[:m]) + abs(len(want) - len(b))
    print("width %d, %d channels: bytes of %d that differ from the wrong orders: %s" % (width, nch, len(want), found))
    assert all(n > 0 for n in found.values()), found
