"""csrc/seqbus.hpp -- which bus a render of a compiled song gets: the table of the 22 routes, the width rule and route(), built for the
host with g++ and held to the ladder they replace, written out here by bus name.  tests/cpu_seqroute.cpp also builds as a program of its
own (-DSEQROUTE_MAIN), which is built and run once here without a sanitizer.  No GPU."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
FIELDS = ("tracks", "meters", "desk", "automation", "groups", "rides", "pans", "history", "clips", "stems")      # shb::Call's, in order
BITS = ("METERS", "DESK", "AUTO", "GROUPS", "RIDES", "PANS", "HISTORY", "CLIPS", "STEMS")

# The bus each call shape took BEFORE there was a route: the struct the ladder in seq_render named, its features read off its bases
# (SeqBusM : SeqBus + meters; SeqBusDM : SeqBusM, SeqDesk; ... SeqBusGC : SeqBusGH, SeqClips), and one call that reached it.
LADDER = {
    "SeqBus":    ("", "tracks", (1, 2, 3, 4)),
    "SeqBusM":   ("METERS", "tracks meters", (1, 2, 3, 4)),
    "SeqBusD":   ("DESK", "tracks desk", (1, 2, 3, 4)),
    "SeqBusDM":  ("METERS DESK", "tracks desk meters", (1, 2, 3, 4)),
    "SeqBusA":   ("DESK AUTO", "tracks desk automation", (1, 2, 4)),
    "SeqBusAM":  ("METERS DESK AUTO", "tracks desk automation meters", (1, 2, 4)),
    "SeqBusG":   ("DESK AUTO GROUPS", "tracks desk groups", (1, 2, 4)),
    "SeqBusG3":  ("DESK GROUPS", "tracks desk groups", (3,)),
    "SeqBusR":   ("DESK AUTO GROUPS RIDES", "tracks desk automation groups rides", (1, 2, 4)),
    "SeqBusP":   ("DESK AUTO GROUPS RIDES PANS", "tracks desk automation groups rides pans", (1, 2, 4)),
    "SeqBusGS":  ("DESK AUTO GROUPS STEMS", "tracks desk automation groups stems", (1, 2, 4)),
    "SeqBusRS":  ("DESK AUTO GROUPS RIDES STEMS", "tracks desk automation groups rides stems", (1, 2, 4)),
    "SeqBusPS":  ("DESK AUTO GROUPS RIDES PANS STEMS", "tracks desk automation groups rides pans stems", (1, 2, 4)),
    "SeqBusGS3": ("DESK GROUPS STEMS", "tracks desk groups stems", (3,)),
    "SeqBusGM":  ("METERS DESK AUTO GROUPS", "tracks desk groups meters", (1, 2, 4)),
    "SeqBusGM3": ("METERS DESK GROUPS", "tracks desk groups meters", (3,)),
    "SeqBusRM":  ("METERS DESK AUTO GROUPS RIDES", "tracks desk automation groups rides meters", (1, 2, 4)),
    "SeqBusPM":  ("METERS DESK AUTO GROUPS RIDES PANS", "tracks desk automation groups rides pans meters", (1, 2, 4)),
    "SeqBusGH":  ("METERS DESK AUTO GROUPS HISTORY", "tracks desk groups meters history", (1, 2, 4)),
    "SeqBusGH3": ("METERS DESK GROUPS HISTORY", "tracks desk groups meters history", (3,)),
    "SeqBusGC":  ("METERS DESK AUTO GROUPS HISTORY CLIPS", "tracks desk automation groups meters history clips", (1, 2, 4)),
    "SeqBusGC3": ("METERS DESK GROUPS HISTORY CLIPS", "tracks desk groups meters history clips", (3,)),
}


@pytest.fixture(scope="module")
def sr(tmp_path_factory):
    out = tmp_path_factory.mktemp("seqroute") / "libseqroute.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", str(ROOT / "tests" / "cpu_seqroute.cpp"), "-o", str(out)], check=True)
    lib = C.CDLL(str(out))
    u32 = C.c_uint32
    for name, args, res in (("sr_nroutes", [], u32), ("sr_route_at", [u32], u32), ("sr_no_bus", [], u32), ("sr_bit", [u32], u32), ("sr_known", [u32], C.c_int),
                            ("sr_valid_at", [u32, C.c_int], C.c_int), ("sr_route", [u32, C.c_int], u32)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    lib.bit = {name: lib.sr_bit(i) for i, name in enumerate(BITS)}
    lib.mask = lambda names: sum(lib.bit[n] for n in names.split())
    lib.routes = [lib.sr_route_at(i) for i in range(lib.sr_nroutes())]
    return lib


def flags_of(call):
    return sum(1 << FIELDS.index(f) for f in call)


def every_call():
    for width in (1, 2, 3, 4):
        for n in range(len(FIELDS) + 1):
            for call in itertools.combinations(FIELDS, n):
                yield set(call), width


def makeable(c, width):
    """What the entry points of sequence.hip can ask of seq_render: their refusals, as a predicate."""
    if "tracks" not in c:
        return not c                                         # a flat song: sh_seq_render alone, every other entry point refuses it
    return ((("clips" not in c) or "history" in c)           # sh_seq_render_clips is a history
            and (("history" not in c) or ({"meters", "groups"} <= c and "rides" not in c))      # blocks of rows, group table (maybe empty); no rides yet
            and (not ({"automation", "groups"} & c) or "desk" in c)
            and (("automation" not in c) or width != 3)      # a fade has no 24-bit form
            and (("pans" not in c) or "rides" in c)          # rides = buses or pans
            and (("rides" not in c) or {"automation", "groups"} <= c)      # the handle says so; sh_seq_render_auto hands an empty group table
            and (("stems" not in c) or ("groups" in c and "meters" not in c)))


def test_the_bits_are_nine_and_the_table_holds_the_22_buses_of_the_ladder(sr):
    assert sorted(sr.bit.values()) == [1 << i for i in range(9)] and sr.sr_no_bus() not in sr.routes
    assert len(sr.routes) == 22 == len(set(sr.routes)) == len(LADDER)
    assert set(sr.routes) == {sr.mask(features) for features, _call, _widths in LADDER.values()}
    assert all(sr.sr_known(m) for m in sr.routes) and sum(sr.sr_known(m) for m in range(512)) == 22


def test_each_bus_of_the_ladder_is_reached_by_its_call_at_its_widths(sr):
    for name, (features, call, widths) in LADDER.items():
        for width in (1, 2, 3, 4):
            got = sr.sr_route(flags_of(call.split()), width)
            if width in widths:
                assert got == sr.mask(features), (name, width)
                assert sr.sr_valid_at(got, width), (name, width)
            elif makeable(set(call.split()), width):         # the same call at the other widths is another bus's (SeqBusG / SeqBusG3)
                assert got != sr.mask(features) and sr.sr_valid_at(got, width), (name, width)
        assert [w for w in (1, 2, 3, 4) if sr.sr_valid_at(sr.mask(features), w)] == list(widths), name


def test_the_width_rule(sr):
    for m in range(512):
        for width in range(0, 6):
            want = m in sr.routes and 1 <= width <= 4 and (width != 3 if m & sr.bit["AUTO"] else width == 3 if m & sr.bit["GROUPS"] else True)
            assert bool(sr.sr_valid_at(m, width)) == want, (m, width)


def test_the_calls_that_can_be_made_take_exactly_the_22_routes(sr):
    image, flat = set(), 0
    for c, width in every_call():
        got = sr.sr_route(flags_of(c), width)
        assert (got == sr.sr_no_bus()) == ("tracks" not in c)           # whatever else a call says
        if not makeable(c, width):
            continue
        if "tracks" not in c:
            flat += 1
            continue
        image.add(got)
        assert sr.sr_valid_at(got, width), (sorted(c), width)
        # a kernel that reads bus lanes or pan lanes of the automation's table is reached only where the handle holds them
        assert not (got & sr.bit["RIDES"]) or "rides" in c, (sorted(c), width)
        assert not (got & sr.bit["PANS"]) or "pans" in c, (sorted(c), width)
        # a part is neither lost nor invented: the rows, their kind and the planes are what the call asked for
        for bit, field in (("METERS", "meters"), ("HISTORY", "history"), ("CLIPS", "clips"), ("STEMS", "stems"), ("DESK", "desk")):
            assert bool(got & sr.bit[bit]) == (field in c), (bit, sorted(c), width)
        assert bool(got & sr.bit["GROUPS"]) == ("groups" in c)
        # with a desk and groups the whole desk rides on the group bus: AUTO with or without automation, except at width 3
        assert bool(got & sr.bit["AUTO"]) == ("automation" in c or ("groups" in c and width != 3)), (sorted(c), width)
    assert image == set(sr.routes) and flat == 4


def test_the_quirks_of_the_ladder(sr):
    r = lambda call, width: sr.sr_route(flags_of(call.split()), width)
    m = sr.mask
    # without a desk nothing but the meters counts, and without groups rides and pans choose nothing (the ladder never looked)
    assert r("tracks automation groups rides stems", 2) == m("") and r("tracks meters history", 2) == m("METERS")
    assert r("tracks desk automation rides pans", 2) == m("DESK AUTO") and r("tracks desk rides history meters", 1) == m("METERS DESK")
    # pans imply the bus that rides as well; stems come in front of the rows, overs in front of a history, and neither rides
    assert r("tracks desk groups pans", 4) == m("DESK AUTO GROUPS RIDES PANS")
    assert r("tracks desk groups stems meters history clips", 2) == m("DESK AUTO GROUPS STEMS")
    assert r("tracks desk groups clips rides pans", 2) == m("METERS DESK AUTO GROUPS HISTORY CLIPS")
    assert r("tracks desk groups history rides", 1) == m("METERS DESK AUTO GROUPS HISTORY")
    # width 3 never rides
    assert r("tracks desk groups rides pans meters", 3) == m("METERS DESK GROUPS") and r("tracks desk groups pans stems", 3) == m("DESK GROUPS STEMS")


def test_the_file_is_a_program_of_its_own_as_well(tmp_path):
    exe = tmp_path / "cpu_seqroute"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-DSEQROUTE_MAIN", str(ROOT / "tests" / "cpu_seqroute.cpp"), "-o", str(exe)], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("seqroute: ") and p.stdout.strip().endswith("ok"), p.stdout + p.stderr
