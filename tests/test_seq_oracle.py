"""tests/seqref.py returns the bytes of the seven per-file oracles it replaced (no GPU).  tests/golden/seq_oracle_digests.json holds the
SHA-256 of what those oracles -- and the case generators around them -- returned at the commit its "parent" entry names, for the right
order and for every wrong order a test forms, list by list; every key is recomputed here through seqref.source / seqref.mix and the
generators where they live now.  The fixture is a record: a digest that differs means the reference changed, never that the fixture is
to be made again."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from tests import test_gpu_channels as CH, test_gpu_enveloped as EN, test_gpu_looped as LP, test_gpu_mix_views as MV
from tests import test_gpu_panned as PA, test_gpu_reversed as RV, test_gpu_sampler as SA, test_gpu_sequence as SQ
from tests.seqcases import GAINS, LEVELS, bus_song, lists, master, named, song
from tests.seqref import ENVELOPE_VARIANTS, RIGHT, SELF, TILE, WRONG, envelope_bytes, mix, pcm, wrong_orders

RECORDED = json.loads((Path(__file__).parent / "golden" / "seq_oracle_digests.json").read_text())
ENTRIES = {}                                                # key -> a function that returns the bytes


def put(key, make):
    assert key not in ENTRIES, key
    ENTRIES[key] = make


def orders(key, events, width, rate, nch, wrong, base=b""):
    """the list under the right order and under each of `wrong`"""
    for order in (RIGHT,) + tuple(wrong):
        put("%s/%s" % (key, order), lambda order=order: mix(base, events(), width, rate, nch, order))


def both_ways(key, events, width, rate, nch):
    put(key + "/right", lambda: mix(b"", events(), width, rate, nch))
    put(key + "/backwards", lambda: mix(b"", events()[::-1], width, rate, nch))


def _entries():
    W4, W3, R = (1, 2, 3, 4), (1, 2, 4), 8192
    # the plain file, the sampler's, the panned one
    def plain_song(*a):
        instruments, events = SQ.song(*a)
        return [(s, instruments[i], v, None) for s, i, v in events]

    def listed(made):
        instruments, events = made
        return [(e[0], instruments[e[1]]) + tuple(e[2:]) for e in events]
    both_ways("sequence/song", plain_song, 2, SQ.RATE, SQ.NCH)
    put("sequence/song(400, 2.0) twice/right", lambda: mix(bytes(2 * SQ.NCH * SQ.RATE * 3), plain_song(400, 2.0) * 2, 2, SQ.RATE, SQ.NCH))
    a, b, c = (pcm(np.random.default_rng(5), 2, n, 0.6) for n in (8192, 3000, 500))
    put("sequence/the track as a source/right", lambda: mix(a, [(0.1, b, 0.9, None), (0.05, SELF, 0.5, 0.2), (0.3, c, None, None), (0.0, SELF, None, None),
                                                                (0.7, c, 1.5, None)], 2, R, 1))
    put("sampler/the track as a source/right", lambda: mix(a, [(0.1, b, 0.9, None, 1.25), (0.05, SELF, 0.5, 0.2, 0.8), (0.3, c, None, None, None),
                                                               (0.0, SELF, None, None, 2.0), (0.7, c, 1.5, None, 0.6)], 2, R, 1))

    def placed(made):
        sources, base, events = made[0], made[-2], made[-1]         # (the panned file's has the number of mono sources between them)
        return base, [(e[0], sources[e[1]]) + tuple(e[2:]) for e in events]
    for w in W4:
        for n in (1, 2):
            put("sequence/every offset/%d-%d/right" % (w, n), lambda w=w, n=n: mix(*placed(SQ._every_offset(w, n, R)), w, R, n))
            put("sampler/every offset/%d-%d/right" % (w, n), lambda w=w, n=n: mix(*placed(SA._every_offset(w, n, R, 100 * w + n)), w, R, n))
        put("panned/every offset/%d/right" % w, lambda w=w: mix(*placed(PA._every_offset(w, R, 300 + w)), w, R, 2))
    sampler, panned = listed(SA.sampler_song()), listed(PA.panned_song())
    orders("sampler/song", lambda: sampler, 2, SA.RATE, SA.NCH, WRONG["rate"])
    orders("panned/song", lambda: panned, 2, PA.RATE, 2, WRONG["pan"])
    # the envelope file
    for w in W3:
        for n in (1, 2):
            orders("enveloped/notes/%d-%d" % (w, n), lambda w=w, n=n: named(*EN.notes(w, n)), w, EN.RATE, n, WRONG["env"] if n == 2 else ())
            put("enveloped/notes on a base/%d-%d/right" % (w, n), lambda w=w, n=n: mix(pcm(np.random.default_rng(w + n), w, 4 * TILE[w], 0.3),
                                                                                       named(*EN.notes(w, n)), w, EN.RATE, n))
            data = pcm(np.random.default_rng(5), w, 1500 * n)
            for variant in (RIGHT,) + ENVELOPE_VARIANTS:
                put("envelope_bytes/%d-%d/%s" % (w, n, variant), lambda w=w, n=n, data=data, variant=variant:
                    envelope_bytes(data, w, n, EN.RATE, 0.0113, 0.0171, 0.5, 0.0233, variant=variant))
            put("envelope_bytes/%d-%d/an unfaded frame" % (w, n), lambda w=w, n=n, data=data: envelope_bytes(data, w, n, EN.RATE, 1001.5 / EN.RATE, 0.01, 0.7, 0.02))

        def loud(w=w):
            instruments, events = EN.notes(w, 2, seed=4, scale=1.0)
            return named(instruments, [(s, i, (1.9 if k % 2 else -1.9), o, sp, p, e) for k, (s, i, _v, o, sp, p, e) in enumerate(events) if e is not None])
        both_ways("enveloped/loud notes/%d" % w, loud, w, EN.RATE, 2)
    # the loop file, the reversed one, the channels one
    for w in W4:
        quiet = pcm(np.random.default_rng(w), w, 3 * TILE[w] - 6, 0.3)
        for n in (1, 2):
            put("looped/plain/%d-%d" % (w, n), lambda w=w, n=n, quiet=quiet: LP.plain_want(quiet, *LP.plain_cases(w, n), w, n))
            put("reversed/plain/%d-%d" % (w, n), lambda w=w, n=n, quiet=quiet: RV.plain_want(quiet, *RV.plain_cases(w, n), w, n))
            put("reversed/plain forwards/%d-%d" % (w, n), lambda w=w, n=n, quiet=quiet: RV.plain_want(quiet, *RV.plain_cases(w, n), w, n, reverse=False))
            put("channels/plain/%d-%d" % (w, n), lambda w=w, n=n: CH.plain_cases(w, n)[3])
            orders("looped/notes/%d-%d" % (w, n), lambda w=w, n=n: named(*LP.notes(w, n)), w, LP.RATE, n, ())
            orders("reversed/notes/%d-%d" % (w, n), lambda w=w, n=n: named(*RV.notes(w, n)), w, RV.RATE, n, WRONG["rev"] if n == 2 else ())
            orders("channels/notes/%d-%d" % (w, n), lambda w=w, n=n: named(*CH.notes(w, n)), w, CH.RATE, n, wrong_orders("chan", w, n))
            if w in (2, 3):
                orders("channels/notes on a base/%d-%d" % (w, n), lambda w=w, n=n: named(*CH.notes(w, n, seed=1)), w, CH.RATE, n, wrong_orders("chan", w, n),
                       pcm(np.random.default_rng(5), w, 3 * TILE[w], 0.3))
        both_ways("looped/loud notes/%d" % w, lambda w=w: named(*LP.notes(w, 2, seed=4, scale=1.0, loud=True)), w, LP.RATE, 2)
        both_ways("reversed/loud notes/%d" % w, lambda w=w: named(*RV.notes(w, 2, seed=4, scale=1.0, loud=True)), w, RV.RATE, 2)
        if w != 3:
            orders("looped/order notes/%d" % w, lambda w=w: named(*LP.order_notes(w)), w, LP.RATE, 2, WRONG["loop"])
        orders("reversed/order notes/%d" % w, lambda w=w: named(*RV.order_notes(w)), w, RV.RATE, 2, WRONG["rev"])
    # the compiled songs, the bus song, the lists of the levels file and of the views file
    for w in W4:
        for level in LEVELS:
            if (level, w) != ("env", 3):
                put("compiled/song/%s-%d" % (level, w), lambda level=level, w=w: song(level, w)[3])
        for t in range(3):
            put("tracks/bus song/%d/track %d" % (w, t), lambda w=w, t=t: bus_song(w)[2][t])
        put("tracks/bus song/%d/master %s" % (w, GAINS[0]), lambda w=w: master(bus_song(w)[2], GAINS[0], w))
        for k, name in enumerate("ABC"):
            put("levels/list %s/%d" % (name, w), lambda w=w, k=k: lists(w)[5 + k])
        for kind in ("loop", "rev"):
            put("mix views/shaped %s/%d" % (kind, w), lambda w=w, kind=kind: MV.shaped(kind, w)[3])


_entries()


def test_every_recorded_key_is_recomputed_and_nothing_else():
    assert set(ENTRIES) == set(RECORDED) - {"parent"} and len(RECORDED["parent"]) == 40


@pytest.mark.parametrize("family", sorted({key.split("/")[0] for key in ENTRIES}))
def test_the_bytes_are_those_of_the_oracles_that_were_replaced(family):
    for key in sorted(k for k in ENTRIES if k.split("/")[0] == family):
        assert hashlib.sha256(ENTRIES[key]()).hexdigest() == RECORDED[key], key


def test_every_list_tells_the_right_order_from_each_of_its_wrong_ones():
    """what the `discriminates` checks of the GPU files rely on, on the recorded digests: under a wrong order a list gives other bytes"""
    every = [o for level in WRONG.values() for o in level]
    judged = 0
    for key in RECORDED:
        head, _, order = key.rpartition("/")
        if order in every and not (key.startswith("envelope_bytes/") and head.endswith("-1")):      # (one channel: k counts frames either way)
            assert RECORDED[key] != RECORDED[head + "/right"], key
            judged += 1
    assert judged >= len(every) and {key.rpartition("/")[2] for key in RECORDED} >= set(every)
