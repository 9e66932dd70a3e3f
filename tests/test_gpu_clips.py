"""GPU parity of the OVERS of a compiled song's level history -- CompiledSequence.render(meters="history", clips=True) /
N.Sequence.render(meters="history", clips=True) / sh_seq_render_clips -- against an INTEGER restatement of the chain.  An over is a sample
at which a bus's own arithmetic was clamped (csrc/seqclip.hpp has the contract); saturation destroys that information, so the reference
cannot be read off ``audioop``'s bytes: ``chain`` below restates the whole chain in numpy int64 with the exact value of every step in
hand -- the events' samples AS PLACED come from tests/seqref.source (live ``audioop``), every saturating add is an exact integer sum and
its clip, every multiply the float64 product, its floor and fbound's clamp -- keeps one sticky flag per bus and sample, and holds every
stage's bytes to live ``audioop`` (``audioop.add``, ``audioop.mul``, tests/seqref.balance) before its counts are trusted.  Expected counts
never come from the product; where the issue asks for the product against itself -- the bytes against the render without ``clips``, the
peaks and sums against ``meters="history"`` of the same call -- that is said.

Songs of about 2.2 tiles at rate 8192, six tracks: a group of two, a loose track, a group of two, a loose track.  Widths 1, 2, 3, 4, mono
and stereo, all events plain (the PLAIN kernels) or some resampled (the RATE kernels); track 0 holds ten events in one tile, more than the
plain 16-bit schedule keeps in flight (four) plus a remainder: its batch loop twice and its tail twice."""
import audioop
import ctypes as C
import functools

import numpy as np
import pytest

from tests.seqcases import RATE, _ev, as_samples, ints, named, raw_tracks, with_samples
from tests.seqref import FIELDS, LANE, TILE, balance, mix, pcm, source
from tests.test_gpu_automation import native_auto, ride
from tests.test_gpu_groups import six
from tests.test_gpu_history import blocks_of
from tests.test_gpu_meters import to_bytes

gpu_test = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4]
NTRACKS = 6
CASES = [(width, nch, level) for width in WIDTHS for nch in (1, 2) for level in ("plain", "rate")]


# ---- the songs -------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def the_song(width, nch, level):
    """(instruments as (bytes, channels), six tracks of events, total samples).  Frames below; w0 is where the pile-up starts, in tile 1."""
    T, L = TILE[width], LANE[width]
    F = T // nch
    rng = np.random.default_rng(4000 + 100 * width + 10 * nch + (level == "rate"))
    instruments = [(pcm(rng, width, 600 * nch, 1.0), nch), (pcm(rng, width, 300 * nch, 0.6), nch), (pcm(rng, width, 97 * nch, 0.1), nch)]
    w0, tail = (T + 3 * L) // nch, (61 * L + 3) // nch
    fast, slow = (2.5, 0.37) if level == "rate" else (None, None)
    tracks = [
        # 0 (group A): two loud notes on one another, then eight more notes over them: ten events in tile 1; clips inside itself on both rails
        [_ev(w0 + 10, 0, 1.7, 200), _ev(w0 + 13, 0, 1.7, 200)] +
        [_ev(w0 + 20 + 7 * k, 1, 0.9 if k % 2 else -0.9, 250, slow if k == 0 else None) for k in range(8)],
        # 1 (group A): one loud note where track 0 piles up: nothing clips inside it, the group's bus does
        [_ev(w0 + 10, 0, None, 200, fast)],
        # 2 (loose): three notes that do not touch one another: no add of an event clamps; a gain above 1.0 does
        [_ev(5, 0, None, 300), _ev(w0 + 10, 0, None, 200), _ev(2 * F, 0, 1.2, tail)],
        # 3 (group B): one loud note: only a pan factor above 1.0 clamps it
        [_ev(w0 + 10, 0, None, 200)],
        # 4 (group B): a note clamped by its OWN volume (the event's chain: not counted) and a quiet one: signal, full scale, no over
        [_ev(3, 2, None), _ev(w0 + 12, 0, 1.7, 200, fast)],
        # 5 (loose): clips inside itself; muted in the first setting
        [_ev(w0 + 10, 0, 1.7, 200), _ev(w0 + 11, 0, 1.7, 200)],
    ]
    total = max(nch * int(RATE * e[0]) + len(source(instruments[e[1]][0], width, RATE, nch, **dict(zip(FIELDS, e[2:])))) // width for t in tracks for e in t)
    assert 2 * T < total < 3 * T and total % L != 0 and total % nch == 0, (total, T, L)
    assert sum(1 for e in tracks[0] if T <= nch * int(RATE * e[0]) < 2 * T) == 10
    return instruments, tracks, total


def settings(nch):
    """(gains, pans as (left, right) pairs or None, groups as (first, end, gain, left, right), the master's gain): the desk at work; a group
    at gain 0.0 with everything else at rest and a master gain that clamps"""
    pans = [None, None, None, (1.5, 1.0), None, None] if nch == 2 else None
    a_pan, b_pan = ((0.999, 0.37), (1.0, 1.0)) if nch == 2 else ((1.0, 1.0), (1.0, 1.0))
    return [((0.5, 1.0, 1.9, 1.0, 1.0, 0.0), pans, [(0, 2, 1.3) + a_pan, (3, 5, 0.8) + b_pan], 0.7),
            (None, None, [(0, 2, 0.0, 1.0, 1.0), (3, 5, 1.0, 1.0, 1.0)], -1.3)]


def flat(pans):
    return None if pans is None else [f for p in pans for f in ((1.0, 1.0) if p is None else p)]


# ---- the reference: the chain in integers, a sticky flag per bus, every stage pinned to live audioop --------------------------------------------
_CHAIN = {}


def chain(width, nch, level, gains, pans, groups, master_gain, lanes=None):
    """(flags: ntracks + 1 + ngroups bool arrays over the song's samples, rows in table order; the master's bytes; post: what each row's
    bus holds where its levels are read, int64; the rails that a clamp hit).  lanes: the tracks' fader moves (tests/test_gpu_automation.ride),
    between a track's gain and its pan: they change the samples and set no flag"""
    key = (width, nch, level, gains, None if pans is None else tuple(pans), tuple(groups), master_gain, lanes)
    if key in _CHAIN:
        return _CHAIN[key]
    instruments, tracks, total = the_song(width, nch, level)
    HI = 2 ** (8 * width - 1) - 1
    LO = -HI - 1
    rails = set()

    def add(acc, x, flag):                                     # audioop.add: the exact sum, its clip
        exact = acc + x
        if (exact > HI).any():
            rails.add("hi")
        if (exact < LO).any():
            rails.add("lo")
        out = np.clip(exact, LO, HI)
        assert to_bytes(out, width) == audioop.add(to_bytes(acc, width), to_bytes(x, width), width)
        return out, flag | (exact > HI) | (exact < LO)

    def mul(x, f, flag, at=slice(None)):                        # audioop.mul on the samples `at`: the float64 product, its floor, fbound's clamp
        if f == 1.0:
            return x, flag
        p = x[at].astype(np.float64) * f
        floor = np.floor(p)
        if (floor > HI).any():
            rails.add("hi")
        if (floor < LO).any():
            rails.add("lo")
        out, flag = x.copy(), flag.copy()
        out[at] = np.floor(np.clip(p, LO, HI)).astype(np.int64)
        flag[at] |= (floor > HI) | (floor < LO)
        assert to_bytes(out[at], width) == audioop.mul(to_bytes(x[at], width), width, f)
        return out, flag

    def pan(x, left, right, flag):                              # a stereo sample's Sample.stereo: even samples by left, odd ones by right
        if (left, right) == (1.0, 1.0):
            return x, flag
        out, flag = mul(x, left, flag, slice(0, None, 2))
        out, flag = mul(out, right, flag, slice(1, None, 2))
        assert to_bytes(out, width) == balance(to_bytes(x, width), width, left, right)
        return out, flag

    none = np.zeros(total, dtype=bool)
    of = {t: k for k, g in enumerate(groups) for t in range(g[0], g[1])}
    quiet = [g[2] == 0.0 or (g[3], g[4]) == (0.0, 0.0) for g in groups]
    flags, post = [none] * (NTRACKS + 1 + len(groups)), [np.zeros(total, dtype=np.int64)] * (NTRACKS + 1 + len(groups))
    master, mflag, bus, bflag = np.zeros(total, dtype=np.int64), none, None, None
    for t, events in enumerate(tracks):
        k = of.get(t)
        g = 1.0 if gains is None else gains[t]
        lr = (1.0, 1.0) if pans is None or pans[t] is None else pans[t]
        if k is not None and t == groups[k][0]:
            bus, bflag = np.zeros(total, dtype=np.int64), none
        if not (g == 0.0 or lr == (0.0, 0.0) or (k is not None and quiet[k])):       # (a muted or skipped track: its events are not read, it reads 0)
            sub, flag = np.zeros(total, dtype=np.int64), none
            for seconds, data, *rest in named(instruments, events):                  # mix_at: every event's samples as placed, added saturating
                placed = np.zeros(total, dtype=np.int64)
                x = ints(source(data, width, RATE, nch, **dict(zip(FIELDS, rest))), width)
                start = nch * int(RATE * seconds)
                placed[start:start + len(x)] = x
                sub, flag = add(sub, placed, flag)
            want = mix(b"", named(instruments, events), width, RATE, nch)
            assert to_bytes(sub, width) == want + bytes(total * width - len(want))
            sub, flag = mul(sub, g, flag)
            if lanes is not None and lanes[t]:
                sub = ints(ride(to_bytes(sub, width), width, nch, lanes[t]), width)      # volumes of at most 1.0, truncated toward zero: inside the range
            sub, flag = pan(sub, lr[0], lr[1], flag)
            flags[t], post[t] = flag, sub
            if k is None:
                master, mflag = add(master, sub, mflag)
            else:
                bus, bflag = add(bus, sub, bflag)
        if k is not None and t == groups[k][1] - 1 and not quiet[k]:                  # the group closes where its last track stands
            bus, bflag = mul(bus, groups[k][2], bflag)
            bus, bflag = pan(bus, groups[k][3], groups[k][4], bflag)
            flags[NTRACKS + 1 + k], post[NTRACKS + 1 + k] = bflag, bus
            master, mflag = add(master, bus, mflag)
    master, mflag = mul(master, 1.0 if master_gain is None else master_gain, mflag)
    flags[NTRACKS], post[NTRACKS] = mflag, master
    _CHAIN[key] = (flags, to_bytes(master, width), post, rails)
    return _CHAIN[key]


def counts(flags, a, b, nch):
    """[row] = (left, right): the flagged samples of song samples [a, b); song sample s is channel s & 1 of a stereo song, 0 of a mono one"""
    s = np.arange(a, b)
    return [(int(f[a:b][s % 2 == 0].sum()), int(f[a:b][s % 2 == 1].sum())) if nch == 2 else (int(f[a:b].sum()), 0) for f in flags]


def want_blocks(width, nch, level, setting, a, b):
    flags = chain(width, nch, level, *setting)[0]
    return [counts(flags, x, y, nch) for x, y in blocks_of(a, b, TILE[width])]


def windows(width, total):
    """the whole song; mid-tile on an odd sample to mid-tile; tile 1 whole with a few samples on either side"""
    T, L = TILE[width], LANE[width]
    return [(0, total), (T // 2 + L + 1, 2 * T - 3 * L - 2), (T - 5, 2 * T + 9)]


# ---- 0: the cases are not vacuous (the reference alone: no GPU) -----------------------------------------------------------------------------------
def test_the_cases_hold_every_kind_of_over():
    kinds, rails, below_the_rail, clean_signal, full_scale_clean = set(), set(), 0, 0, 0
    only_gain = only_pan = 0
    for width, nch, level in CASES:
        _instruments, _tracks, total = the_song(width, nch, level)
        HI = 2 ** (8 * width - 1) - 1
        for setting in settings(nch):
            gains, pans, groups, master_gain = setting
            flags, _bytes, post, hit = chain(width, nch, level, *setting)
            rails |= hit
            whole = counts(flags, 0, total, nch)
            for r, c in enumerate(whole):
                kind = "track" if r < NTRACKS else "master" if r == NTRACKS else "group"
                if sum(c):
                    kinds.add(kind)
                    if kind == "track" and np.abs(post[r]).max() < HI:
                        below_the_rail += 1                     # it clipped inside itself and sits under its fader: its peak looks healthy
                elif np.abs(post[r]).max() > 0:
                    clean_signal += 1
                    full_scale_clean += int(np.abs(post[r]).max() >= HI)
            assert sum(whole[4]) == 0 and np.abs(post[4]).max() >= HI      # track 4: clamped by its own event's volume alone: at the rail, no over
            if gains is not None:                               # track 2: its count comes from its gain of 1.9 alone
                rest = chain(width, nch, level, gains[:2] + (1.0,) + gains[3:], pans, groups, master_gain)[0]
                assert gains[2] > 1.0 and sum(whole[2]) > 0 and sum(counts(rest, 0, total, nch)[2]) == 0
                only_gain += 1
                assert sum(whole[5]) == 0 and gains[5] == 0.0   # the muted track
                assert sum(counts(chain(width, nch, level, None, pans, groups, master_gain)[0], 0, total, nch)[5]) > 0      # which clips when it sounds
            if pans is not None:                                # track 3: its count comes from its left pan factor of 1.5 alone
                rest = chain(width, nch, level, gains, None, groups, master_gain)[0]
                assert pans[3][0] > 1.0 and whole[3][0] > 0 and whole[3][1] == 0 and sum(counts(rest, 0, total, nch)[3]) == 0
                only_pan += 1
            for k, g in enumerate(groups):
                if g[2] == 0.0:                                 # a group at gain 0.0: it and its tracks read 0
                    assert all(sum(whole[r]) == 0 for r in [NTRACKS + 1 + k] + list(range(g[0], g[1])))
            # in the plain 16-bit schedule's batches: track 0's overs in tile 1 come from adds of its ten events
            if gains is not None and gains[0] == 0.5:
                assert sum(whole[0]) > 0 and np.abs(post[0]).max() < HI
            # a sample counts once however many steps clamped at it: no count passes the samples of its channel
            assert all(c[0] <= (total + 1) // nch and c[1] <= total // 2 for c in whole)
    assert kinds == {"track", "group", "master"} and rails == {"hi", "lo"}
    assert only_gain and only_pan and below_the_rail and clean_signal and full_scale_clean


# ---- the product's side -------------------------------------------------------------------------------------------------------------------------------
def render(N, seq, width, a, b, setting, out_sample=0, clips=True, auto=None):
    """(the array of blocks, the rendered bytes, the guards intact) of a history render into a 0x5A-filled buffer"""
    gains, pans, groups, master_gain = setting
    n = b - a
    inner = (out_sample + n) * width
    parent = N.DeviceBuffer.from_bytes(b"\x5a" * (64 + inner + 64))
    kw = dict(clips=True) if clips else {}
    if auto is not None:
        kw["automation"] = auto
    blocks = seq.render(a, n, parent.view(64, inner), out_sample, gains=gains, meters="history", pans=flat(pans), master=master_gain, groups=groups, **kw)
    got = parent.download_bytes(64 + inner + 64)
    at = 64 + out_sample * width
    return blocks, got[at:at + n * width], got[:at] == b"\x5a" * at and got[at + n * width:] == b"\x5a" * 64


# ---- 1: counts, levels and bytes, window by window ------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width, nch, level", CASES)
def test_counts_equal_the_reference_per_block_row_and_channel(gpu, width, nch, level):
    N = gpu
    instruments, tracks, total = the_song(width, nch, level)
    T = TILE[width]
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    assert N.SEQ_LEVELS[seq.info()["level"]] == level and seq.tracks()[0] == NTRACKS
    for setting in settings(nch):
        want_bytes = chain(width, nch, level, *setting)[1]
        seen = {}
        for a, b in windows(width, total):
            ranges = blocks_of(a, b, T)
            want = want_blocks(width, nch, level, setting, a, b)
            for out_sample in (0, 1):                           # the output buffer on and one sample off the window's place
                blocks, got, guards = render(N, seq, width, a, b, setting, out_sample)
                assert blocks.dtype == N.SEQ_METER_CLIPS_DTYPE and blocks.shape == (len(ranges), NTRACKS + 3)
                have = [[(int(r["clipped"][0]), int(r["clipped"][1])) for r in block] for block in blocks]
                print("width %d, %d ch, %s, window [%d, %d) at %d: counts %s" % (width, nch, level, a, b, out_sample, have))
                for j, rows in enumerate(have):
                    assert rows == want[j], "setting %s, window [%d, %d) at out_sample %d, block %d = [%d, %d):\n%s\n%s" % (
                        (setting, a, b, out_sample, j) + ranges[j] + (rows, want[j]))
                assert got == want_bytes[a * width:b * width] and guards, (setting, a, b, out_sample)
            # the product against itself: the bytes of the render without clips, the peaks and sums of meters="history" of the same call
            levels, plain_bytes, _g = render(N, seq, width, a, b, setting, 1, clips=False)
            assert levels.dtype == N.SEQ_METER_DTYPE and got == plain_bytes
            for field in ("peak", "sq_hi", "sq_lo"):
                assert np.array_equal(blocks[field], levels[field]), (field, setting, a, b)
            # the total is the sum over the blocks, and what the reference counts in the window as a whole
            assert blocks["clipped"].sum(axis=0).tolist() == [list(c) for c in counts(chain(width, nch, level, *setting)[0], a, b, nch)]
            for (x, y), rows in zip(ranges, have):
                if y - x == T:
                    assert seen.setdefault(x, rows) == rows    # a song block whole inside two windows reads the same from both
        assert T in seen
        whole = render(N, seq, width, 0, total, setting)[0]["clipped"].sum(axis=0).tolist()
        gains, _pans, groups, _master = setting
        if gains is not None:
            assert whole[5] == [0, 0] and gains[5] == 0.0 and sum(whole[0]) > 0      # a muted track reads 0
        for k, g in enumerate(groups):
            if g[2] == 0.0:                                     # a group at gain 0.0 and its tracks read 0
                assert all(whole[r] == [0, 0] for r in [NTRACKS + 1 + k] + list(range(g[0], g[1])))
        if nch == 1:
            assert all(c[1] == 0 for c in whole)                # a mono song fills channel 0
    seq.free()


# ---- 1b: with the tracks' fader moves, which are not counted and change what the steps behind them clamp ------------------------------------------
@gpu_test
@pytest.mark.parametrize("width, nch", [(2, 2), (2, 1), (1, 2), (4, 1)])
def test_fader_moves_are_not_counted_and_shape_what_the_buses_behind_them_take(gpu, width, nch):
    N = gpu
    instruments, tracks, total = the_song(width, nch, "plain")
    T, L = TILE[width], LANE[width]
    w = (T + 3 * L) // nch
    # in song frames: track 0 fades across the pile-up, track 2 (the gain of 1.9) is held at 0.4 over its second note, track 3 fades out
    lanes = (((w - 40, w + 60, 0.2, 0.9), (w + 60, w + 150, 0.9, 0.1)), (), ((w, w + 300, 0.4, 0.4),), ((0, total // nch, 1.0, 0.25),), (), ())
    seq, _samples = raw_tracks(N, instruments, tracks, nch, width)
    auto = native_auto(N, seq, lanes, nch)
    setting = settings(nch)[0]
    flags, want_bytes, _post, _rails = chain(width, nch, "plain", *setting, lanes=lanes)
    still = chain(width, nch, "plain", *setting)[0]
    whole, unmoved = counts(flags, 0, total, nch), counts(still, 0, total, nch)
    assert whole[0] == unmoved[0] and sum(whole[0]) > 0         # a track's own count does not see its moves: they stand behind its adds and its gain
    assert whole[NTRACKS] != unmoved[NTRACKS] or whole[NTRACKS + 1] != unmoved[NTRACKS + 1]      # what the buses behind them take does
    for a, b in windows(width, total):
        blocks, got, guards = render(N, seq, width, a, b, setting, 1, auto=auto)
        have = [[(int(r["clipped"][0]), int(r["clipped"][1])) for r in block] for block in blocks]
        assert have == [counts(flags, x, y, nch) for x, y in blocks_of(a, b, T)], (a, b)
        assert got == want_bytes[a * width:b * width] and guards, (a, b)
        levels = render(N, seq, width, a, b, setting, 1, clips=False, auto=auto)[0]
        assert all(np.array_equal(blocks[f], levels[f]) for f in ("peak", "sq_hi", "sq_lo"))
    auto.free()
    seq.free()


# ---- 2: through the mixer: render, chunks that are no multiple of the block, total and fold ------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width, nch, level", [(2, 2, "plain"), (2, 1, "rate"), (1, 1, "plain"), (3, 2, "rate"), (4, 2, "plain")])
def test_the_mixer_hands_the_counts_on(gpu, width, nch, level):
    from synthesizer_amd import mixer
    instruments, tracks, total = the_song(width, nch, level)
    T = TILE[width]
    samples = as_samples(instruments, width, RATE)
    setting = settings(nch)[0]
    gains, pans, groups, master_gain = setting
    flags, want_bytes, _post, _rails = chain(width, nch, level, *setting)
    both = (lambda c: tuple(c)) if nch == 2 else (lambda c: (c[0], c[0]))      # the mono rule of peak
    desk = dict(gains=gains, pans=pans, master=master_gain, groups=[(f, e, g, None if (lf, rf) == (1.0, 1.0) else (lf, rf)) for f, e, g, lf, rf in groups])
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, nch, width) as cs:
        sample, h = cs.render(meters="history", clips=True, **desk)
        assert bytes(sample.view_frame_data()) == want_bytes and isinstance(h, mixer.SongHistory)
        want = want_blocks(width, nch, level, setting, 0, total)
        assert h.clipped().shape == (len(want), NTRACKS + 3, 2) and h.clipped().tolist() == [[list(both(c)) for c in rows] for rows in want]
        whole = counts(flags, 0, total, nch)
        levels = h.total()
        assert [lv.clipped for lv in levels.tracks + [levels.master] + levels.groups] == [both(c) for c in whole]
        assert h.clipped().sum(axis=0).tolist() == [list(both(c)) for c in whole] and h.fold(2).clipped().sum(axis=0).tolist() == [list(both(c)) for c in whole]
        assert [lv.clipped for lv in h[1].tracks] == [both(c) for c in want[1][:NTRACKS]]
        _s, plain = cs.render(meters="history", **desk)          # the levels there were: equal with and without counts, no counts without clips
        assert plain.clipped() is None and plain.total() == levels and all(plain[j] == h[j] for j in range(len(want)))
        assert levels == cs.render(meters=True, **desk)[1]
        chunk = T // nch + 3                                    # frames: no multiple of the block
        at, joined = 0, b""
        for part, hist in cs.chunks(chunk, meters="history", clips=True, **desk):
            n = len(part)
            assert hist.clipped().tolist() == [[list(both(c)) for c in rows] for rows in want_blocks(width, nch, level, setting, at * nch, (at + n) * nch)], at
            joined += bytes(part.view_frame_data())
            at += n
        assert at * nch == total and joined == want_bytes
        buf = gpu.DeviceBuffer.from_bytes(b"\x5a" * 64)
        for meters in (False, True):
            with pytest.raises(ValueError, match="clips=True counts the overs per block of a level history"):
                cs.render_into(buf, 0, 0, 8, meters=meters, clips=True)
        if width != 3:                                          # (a fade has no 24-bit form: no automation there at all)
            ride = cs.automation([None] * NTRACKS, master=[(0, 50, 0.5, 1.0)])
            with pytest.raises(NotImplementedError, match="overs are not counted through rides of buses and pans yet"):
                cs.render_into(buf, 0, 0, 8, meters="history", clips=True, automation=ride)
            ride.close()
        assert buf.download_bytes(64) == b"\x5a" * 64
    with mixer.compile_sequence(with_samples(samples, tracks[0]), RATE, nch, width) as flat_song:
        with pytest.raises(ValueError, match="meters need a song of tracks"):
            flat_song.render(meters="history", clips=True)


# ---- 3: what the entry point refuses ----------------------------------------------------------------------------------------------------------------
@gpu_test
def test_the_entry_point_refuses_on_the_host_and_leaves_out_and_rows(gpu):
    N = gpu
    lib = N.lib()
    from synthesizer_amd import mixer
    from synthesizer_amd.sample import Sample
    instruments, tracks, _subs, total = six("pile", 2)
    T = TILE[2]
    seq, samples = raw_tracks(N, instruments, tracks, 2, 2)
    bufs, table, segtab, nbytes = Sample(samplerate=RATE, nchannels=2, samplewidth=2)._compile_events(with_samples(samples, [e for t in tracks for e in t]))
    flat_song = N.Sequence(bufs, table, segtab, 2, 2, nbytes // 2)
    pack = mixer.CompiledSequence._pack_lanes
    none6 = ((),) * 6
    segments, first = pack(none6, 2, master=((0, 50, 0.5, 1.0),), groups=((), ()), buses=True)
    master_ride = N.SeqAutomation(seq, segments, first, 2)
    segments, first = pack(none6, 2, master=(), groups=((), ((0, 50, 0.5, 0.5),)), buses=True)
    group_ride = N.SeqAutomation(seq, segments, first, 2)
    segments, first = pack(none6, 2, master=(), groups=((), ()), buses=True)
    pan_segments, pan_first = mixer.CompiledSequence._pack_pan_lanes((((0, 50, 0.5, -1.0),),) + ((),) * 5, ((), ()))
    pan_ride = N.SeqAutomation(seq, segments, first, 2, pan_segments, pan_first)
    out = N.DeviceBuffer.from_bytes(b"\x5a" * 4000)
    rows = (N.SeqMeterClips * 20)()
    C.memset(rows, 0xAB, C.sizeof(rows))
    untouched = bytes(rows)
    dbl = lambda *v: (C.c_double * len(v))(*v)                 # noqa: E731
    grp = lambda *g: (N.SeqGroup * max(1, len(g)))(*[N.SeqGroup(*x) for x in g])      # noqa: E731
    ones, twelve = dbl(*[1.0] * 6), dbl(*[0.5, 0.5] * 6)
    good = grp((0, 2, 0.8, 1.0, 1.0), (3, 5, 1.3, 0.5, 0.25))

    def call(song=seq, a=0, n=100, o=out.handle, at=0, gains=ones, ngains=6, pans=twelve, npans=12, master_gain=1.0, meters=rows, nrows=9, nblocks=1,
             automation=None, groups=good, ngroups=2):
        return (song.handle if song is not None else None, a, n, o, at, gains, ngains, pans, npans, master_gain, meters, nrows, nblocks, automation, groups,
                ngroups)
    for what, args, message in (
        ("a master ride", call(automation=master_ride.handle), b"the automation rides a bus: overs are not counted through rides of buses and pans yet"),
        ("a group ride", call(automation=group_ride.handle), b"the automation rides a bus: overs are not counted through rides of buses and pans yet"),
        ("a pan ride", call(automation=pan_ride.handle), b"the automation rides a pan: overs are not counted through rides of buses and pans yet"),
        ("rows for the tracks and the master alone", call(nrows=7), b"7 rows for 6 tracks, the master and 2 groups"),
        ("a row too many", call(nrows=10), b"10 rows for 6 tracks, the master and 2 groups"),
        ("the groups' rows without groups", call(groups=None, ngroups=0), b"9 rows for 6 tracks, the master and 0 groups"),
        ("a block too few", call(a=T - 1, n=2), b"1 blocks for a window of 2"),
        ("a block too many", call(nblocks=2), b"2 blocks for a window of 1"),
        ("no block for a window", call(nblocks=0), b"0 blocks for a window of 1"),
        ("a block for an empty window", call(n=0), b"1 blocks for a window of 0"),
        ("NULL rows with a window", call(meters=None), b"NULL argument"),
        ("a flat song", call(song=flat_song, gains=None, ngains=0, pans=None, npans=0), b"the song has no tracks"),
        ("a range past the song", call(a=total - 10, n=11), b"range outside the song"),
        ("too few gains", call(ngains=5), b"5 gains for 6 tracks"),
    ):
        assert lib.sh_seq_render_clips(*args) == N.SH_ERR_INVALID, what
        err = lib.sh_last_error()
        assert err.startswith(b"sh_seq_render_clips") and message in err, (what, err)
        assert bytes(rows) == untouched, what
    assert out.download_bytes(4000) == b"\x5a" * 4000           # nothing was launched
    # an empty window: SH_OK with no block, NULL rows or not; nothing is written
    assert lib.sh_seq_render_clips(*call(a=50, n=0, nblocks=0)) == N.SH_OK and lib.sh_seq_render_clips(*call(a=50, n=0, nblocks=0, meters=None)) == N.SH_OK
    assert bytes(rows) == untouched and out.download_bytes(4000) == b"\x5a" * 4000
    # and a call it takes writes exactly its rows, 48 bytes each, the levels those of sh_seq_render_history
    assert lib.sh_seq_render_clips(*call(n=1000)) == N.SH_OK
    raw = bytes(rows)
    assert raw[9 * 48:] == untouched[9 * 48:] and all(raw[r * 48:(r + 1) * 48] != untouched[:48] for r in range(9))
    levels = (N.SeqMeter * 9)()
    assert lib.sh_seq_render_history(*call(n=1000, meters=levels)) == N.SH_OK
    got = np.frombuffer(raw[:9 * 48], dtype=N.SEQ_METER_CLIPS_DTYPE)
    for field in ("peak", "sq_hi", "sq_lo"):
        assert np.array_equal(got[field], np.frombuffer(bytes(levels), dtype=N.SEQ_METER_DTYPE)[field])
    for a in (master_ride, group_ride, pan_ride):
        a.free()
    for s in (seq, flat_song):
        s.free()
