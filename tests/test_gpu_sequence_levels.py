"""The four entry points of the placed-sample mixer agree with each other: a list that a lower feature level can express gives the same
track bytes through every level above it -- sh_mix_events, sh_mix_events_rate, sh_mix_events_pan (src_channels 2) and sh_mix_events_env
(seg_count 0) -- and those bytes are live ``audioop``'s (tests/seqref.py: ratecv, tostereo, mul, add with
saturation at every event, in list order).  Small on purpose: a stereo track of two tiles and a tail, sources of a few hundred frames."""
import pytest

from tests.seqcases import call_level, in_a_child_under_the_other_alignment_scheme, lists, rows_of

pytestmark = pytest.mark.gpu


def _run(N, level, rows, bufs, base, width):
    """the track bytes after one call of the entry point of `level` on a fresh copy of base"""
    track = N.DeviceBuffer.from_bytes(base)
    assert call_level(N, level, rows, bufs, width, track, len(base) // width) == N.SH_OK, (level, N.lib().sh_last_error())
    return track.download_bytes(len(base))


@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_the_levels_agree(gpu, width):
    N = gpu
    sources, base, A, B, C_, want_a, want_b, want_c = lists(width)
    bufs = [N.DeviceBuffer.from_bytes(b) for b in sources]
    env = [] if width == 3 else ["env"]                    # an envelope's fades have no 24-bit form
    for name, lst, want, levels in (("A", A, want_a, ["plain", "rate", "pan"] + env), ("B", B, want_b, ["rate", "pan"] + env),
                                    ("C", C_, want_c, ["pan"] + env)):
        rows = rows_of(lst, sources, width)
        got = {level: _run(N, level, rows, bufs, base, width) for level in levels}
        for level in levels:
            assert got[level] == got[levels[0]], "list %s, width %d: %s differs from %s" % (name, width, level, levels[0])
            assert got[level] == want, "list %s, width %d: %s differs from audioop" % (name, width, level)
    assert want_a != base and want_b != want_a and want_c != want_b


def test_the_levels_agree_under_the_other_alignment_scheme(gpu):
    """SYNTHHIP_SEQ_ALIGN is read once per process (sh_init): the 16-bit case again in a child under the scheme that is not the default"""
    in_a_child_under_the_other_alignment_scheme(__file__, ["test_the_levels_agree[2]"])
