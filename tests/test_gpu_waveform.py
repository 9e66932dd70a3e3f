"""GPU tests of the waveform EXTREMES per block of PCM in device memory -- sh_pcm_extent_blocks, N.pcm_extent_blocks, mixer.waveform /
Sample.waveform, SongStems.waveform and CompiledSequence.waveform -- against the live ``audioop.minmax`` on each channel's samples,
de-interleaved in Python, at widths 1 to 4; every comparison exact equality of ``lo`` and ``hi``.  The shapes are the smallest at which
the kernel can go wrong: a window that is no multiple of any block or vector, blocks of one frame and blocks longer than the window,
planes of one sign (an accumulator that starts at 0), a stereo plane whose sides differ in sign behind an even and an odd head, every
start within a 16-byte vector with the two rails in turn in front and behind, planes with rails between them, blocks of more than one
part whose extremes stand in the scalar head and tail, and the song of tests/test_gpu_level_blocks.py with its rides."""
import audioop
import ctypes as C
import random

import numpy as np
import pytest

from tests.test_gpu_level_blocks import LISTS, RATE, SETTINGS, TILE, as_samples, blocks_of, pack, seeded, six, with_samples

gpu_test = pytest.mark.gpu
WIDTHS = [1, 2, 3, 4]


# ---- the reference: audioop.minmax ---------------------------------------------------------------------------------------------------------
def rails(width):
    return -(1 << (8 * width - 1)), (1 << (8 * width - 1)) - 1


def between(seed, n, width, low=None, high=None):
    """n seeded samples in [low, high], by default every value but the two rails, which then mark a read outside"""
    lo, hi = rails(width)
    rng = random.Random(seed)
    low, high = lo + 1 if low is None else low, hi - 1 if high is None else high
    return [rng.randrange(low, high + 1) for _ in range(n)]


def turns(width, count, first=0):
    """`count` samples that alternate the lower and the upper rail"""
    return pack([rails(width)[(first + k) & 1] for k in range(count)], width)


def want_rows(values, width, nch, origin, n, B):
    """[(lo pair, hi pair)] per block of one plane's samples; a mono input's channel 1 reads (0, 0)"""
    chans = [pack(values[c:n * nch:nch], width) for c in range(nch)]
    out = []
    for a, b in blocks_of(origin, n, B):
        lo, hi = [0, 0], [0, 0]
        for c in range(nch):
            lo[c], hi[c] = audioop.minmax(chans[c][(a - origin) * width:(b - origin) * width], width)
        out.append((tuple(lo), tuple(hi)))
    return out


def got_rows(blocks, r=0):
    return [((int(row["lo"][0]), int(row["lo"][1])), (int(row["hi"][0]), int(row["hi"][1]))) for row in blocks[:, r]]


# ---- 1: the grid ---------------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", WIDTHS)
def test_every_block_of_a_window_of_4097_frames(gpu, width, nch):
    N = gpu
    n = 4097
    values = seeded(10 * width + nch, n * nch, width)
    assert (min(values), max(values)) == rails(width)           # both rails among the samples
    buf = N.DeviceBuffer.from_bytes(pack(values, width))
    for B in (1, 7, 64, 1000, 5000):
        for origin in (0, 5, 999):
            blocks = N.pcm_extent_blocks(buf, 0, n, nch, width, n * nch, 1, origin, B)
            want = want_rows(values, width, nch, origin, n, B)
            assert blocks.shape == (len(want), 1) and blocks.dtype == N.PCM_EXTENT_DTYPE and got_rows(blocks) == want, (B, origin)
            assert nch == 2 or not (blocks["lo"][:, :, 1].any() or blocks["hi"][:, :, 1].any())      # a mono input's channel 1 is (0, 0)
    assert min(row[0][0] for row in want) == rails(width)[0] and max(max(row[1]) for row in want) == rails(width)[1]


# ---- 2: signs ------------------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", WIDTHS)
def test_planes_of_one_sign_and_planes_constant_at_a_rail(gpu, width, nch):
    N = gpu
    n, B, origin = 301, 64, 5
    lo, hi = rails(width)
    for name, values in (("negative", between(40 * width + nch, n * nch, width, lo, -1)), ("positive", between(41 * width + nch, n * nch, width, 1, hi)),
                         ("the lower rail", [lo] * (n * nch)), ("the upper rail", [hi] * (n * nch))):
        buf = N.DeviceBuffer.from_bytes(pack(values, width))
        got, want = got_rows(N.pcm_extent_blocks(buf, 0, n, nch, width, n * nch, 1, origin, B)), want_rows(values, width, nch, origin, n, B)
        assert got == want, name
        if name == "negative":
            assert all(row[1][c] < 0 for row in got for c in range(nch))      # hi < 0: no accumulator started at 0
        if name == "positive":
            assert all(row[0][c] > 0 for row in got for c in range(nch))      # lo > 0
        if name == "the lower rail":
            assert all(row[0][0] == row[1][0] == lo for row in got) and (width < 4 or lo == -2 ** 31)


@gpu_test
@pytest.mark.parametrize("width", WIDTHS)
def test_a_stereo_plane_whose_left_is_negative_and_right_positive_behind_an_even_and_an_odd_head(gpu, width):
    N = gpu
    n, B, origin = 203, 48, 7
    lo, hi = rails(width)
    left, right = between(50 + width, n, width, lo, -1), between(60 + width, n, width, 1, hi)
    values = [x for pair in zip(left, right) for x in pair]
    want = want_rows(values, width, 2, origin, n, B)
    assert all(row[1][0] < 0 < row[0][1] for row in want)
    for off in (8, 9, 16, 17, 3):                               # the plane's first sample on an even and on an odd sample of the buffer
        buf = N.DeviceBuffer.from_bytes(bytes(off * width) + pack(values, width) + bytes(8 * width))
        assert got_rows(N.pcm_extent_blocks(buf, off, n, 2, width, 2 * n, 1, origin, B)) == want, off
        view = buf.view(off * width, 2 * n * width)
        assert got_rows(N.pcm_extent_blocks(view, 0, n, 2, width, 2 * n, 1, origin, B)) == want, off


# ---- 3: alignment: every start within a 16-byte vector, the rails in turn in front and behind --------------------------------------------
@gpu_test
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", WIDTHS)
def test_every_start_within_a_vector_reads_its_window_and_nothing_beside_it(gpu, width, nch):
    N = gpu
    n, B, origin = 203, 48, 7
    values = between(20 * width + nch, n * nch, width)
    lo, hi = rails(width)
    want = want_rows(values, width, nch, origin, n, B)
    assert all(lo < row[0][c] and row[1][c] < hi for row in want for c in range(nch))      # one sample read outside shows in lo or in hi
    for off in range(16 if width == 3 else 16 // width):       # in samples: each of the offsets of a 16-byte vector
        for first in (0, 1):                                    # either rail next to the window, on either side
            data = turns(width, 32 + off, first) + pack(values, width) + turns(width, 40, first)
            buf = N.DeviceBuffer.from_bytes(data)
            assert got_rows(N.pcm_extent_blocks(buf, 32 + off, n, nch, width, n * nch, 1, origin, B)) == want, (off, first)
            # the same bytes behind a view cut at that sample: the base itself off the 16-byte grid
            view = buf.view((32 + off) * width, len(data) - (32 + off) * width)
            assert got_rows(N.pcm_extent_blocks(view, 0, n, nch, width, n * nch, 1, origin, B)) == want, (off, first)
    if width > 1:                                               # a view cut at an odd BYTE: off the sample grid
        for first in (0, 1):
            buf = N.DeviceBuffer.from_bytes(turns(width, 8, first) + b"\x80" + pack(values, width) + turns(width, 8, first))
            view = buf.view(8 * width + 1, n * nch * width)
            assert got_rows(N.pcm_extent_blocks(view, 0, n, nch, width, n * nch, 1, origin, B)) == want, first


# ---- 4: planes, with rails between them ---------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("width", WIDTHS)
def test_three_planes_with_the_rails_in_the_gaps(gpu, width, nch):
    N = gpu
    n, B, origin = 333, 100, 250
    plane = n * nch + 3
    planes = [between(30 * width + nch + 100 * r, n * nch, width) for r in range(3)]
    lo, hi = rails(width)
    data = turns(width, 5) + b"".join(pack(p, width) + turns(width, 3, r) for r, p in enumerate(planes)) + turns(width, 16)
    buf = N.DeviceBuffer.from_bytes(data)
    blocks = N.pcm_extent_blocks(buf, 5, n, nch, width, plane, 3, origin, B)
    nb = len(blocks_of(origin, n, B))
    assert blocks.shape == (nb, 3) and nb == 4
    wants = [want_rows(planes[r], width, nch, origin, n, B) for r in range(3)]
    for r in range(3):
        assert got_rows(blocks, r) == wants[r] and all(lo < row[0][0] and row[1][0] < hi for row in wants[r]), r
    flat = np.frombuffer(blocks.tobytes(), dtype=N.PCM_EXTENT_DTYPE)      # block-major: row r of block j at j * nplanes + r
    for j in range(nb):
        for r in range(3):
            assert (tuple(flat[j * 3 + r]["lo"].tolist()), tuple(flat[j * 3 + r]["hi"].tolist())) == wants[r][j], (j, r)


# ---- 5: blocks of more than one part ---------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width", [2, 4])
@pytest.mark.parametrize("nch, extra", [(1, 5), (1, 6), (2, 8)])
def test_blocks_of_three_parts_and_a_few_samples_with_their_extremes_in_head_and_tail(gpu, width, nch, extra):
    from synthesizer_amd.sample import Sample
    N = gpu
    P = N.PCM_PART_SAMPLES
    B = (3 * P + extra) // nch                                  # blocks of 3 * PART_SAMPLES + extra samples
    assert B * nch == 3 * P + extra
    n, origin = 2 * B + 1000, 0                                 # two whole blocks and a partial one
    lo, hi = rails(width)
    values = between(50 * width + nch + extra, n * nch, width)
    for a, b in blocks_of(origin, n, B):                        # the block's maximum in its first sample, its minimum in its last
        values[a * nch], values[b * nch - 1] = hi, lo
    want = want_rows(values, width, nch, origin, n, B)
    assert all(row[0][nch - 1] == lo and row[1][0] == hi for row in want)
    # behind one sample of padding the plane starts off the 16-byte grid: a block's first sample is scalar head, its last scalar tail
    buf = N.DeviceBuffer.from_bytes(bytes(width) + pack(values, width) + bytes(width))
    blocks = N.pcm_extent_blocks(buf, 1, n, nch, width, n * nch, 1, origin, B)
    assert blocks.shape == (3, 1) and got_rows(blocks) == want
    shifted = N.pcm_extent_blocks(buf, 1, n, nch, width, n * nch, 1, B - 77, B)      # a window that starts mid-block
    assert got_rows(shifted) == want_rows(values, width, nch, B - 77, n, B)
    # the same table from a call whose blocks are one part each, folded in Python
    small = max(d for d in range(1, P // nch + 1) if B % d == 0)
    assert small * nch <= P and 1 < small < B
    sample = Sample.from_raw_frames(pack(values, width), width, RATE, nch)
    whole, fine = sample.waveform(B), sample.waveform(small)
    folded = fine.fold(B // small)
    assert len(whole) == 3 and len(fine) > len(whole) and np.array_equal(folded.lo, whole.lo) and np.array_equal(folded.hi, whole.hi)
    assert [((int(l[0]), int(l[1])), (int(h[0]), int(h[1]))) for l, h in zip(whole.lo[:, 0], whole.hi[:, 0])] == want
    assert folded.starts == whole.starts and folded.block_counts == whole.block_counts


# ---- 6: edge sizes and repetition ------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("width", WIDTHS)
def test_no_frame_one_frame_a_block_longer_than_the_window_and_the_same_table_twice(gpu, width):
    from synthesizer_amd import mixer
    from synthesizer_amd.sample import Sample
    N = gpu
    values = seeded(60 + width, 2 * 500, width)
    buf = N.DeviceBuffer.from_bytes(pack(values, width))
    assert N.pcm_extent_blocks(buf, 0, 0, 2, width, 0, 1, 17, 10).shape == (0, 1)
    assert N.lib().sh_pcm_extent_blocks(buf.handle, 0, 0, 2, width, 0, 1, 17, 10, None, 0) == N.SH_OK
    for nch in (1, 2):
        one = N.pcm_extent_blocks(buf, 3, 1, nch, width, nch, 1, 2 ** 40 + 1, 64)
        assert got_rows(one) == want_rows(values[3:3 + nch], width, nch, 2 ** 40 + 1, 1, 64)
        wide = N.pcm_extent_blocks(buf, 0, 500, nch, width, 500 * nch, 1, 100, 10 ** 9)
        assert wide.shape == (1, 1) and got_rows(wide) == want_rows(values, width, nch, 100, 500, 10 ** 9)
        across = N.pcm_extent_blocks(buf, 0, 500, nch, width, 500 * nch, 1, 10 ** 9 - 100, 10 ** 9)      # two partial blocks of a long grid
        assert across.shape == (2, 1) and got_rows(across) == want_rows(values, width, nch, 10 ** 9 - 100, 500, 10 ** 9)
    first = N.pcm_extent_blocks(buf, 0, 500, 2, width, 1000, 1, 5, 7)
    again = N.pcm_extent_blocks(buf, 0, 500, 2, width, 1000, 1, 5, 7)
    assert first.tobytes() == again.tobytes() and len(first) == 73
    # through the mixer: an empty Sample has an empty Waveform; a mono Sample draws channel 0 twice
    empty = Sample(samplerate=RATE, nchannels=2, samplewidth=width).waveform(64, 5)
    assert isinstance(empty, mixer.Waveform) and len(empty) == 0 and empty.extents().shape == (0, 1, 2, 2) and empty.peaks().shape == (0, 1, 2)
    mono = Sample.from_raw_frames(pack(values[:333], width), width, RATE, 1)
    w = mixer.waveform(mono, 100, origin_frame=250)
    want = want_rows(values[:333], width, 1, 250, 333, 100)
    assert w.starts == [250, 300, 400, 500] and w.block_counts == [50, 100, 100, 83] and w.first_block == 2 and w.ngroups == 0
    assert [[list(pair) for pair in block[0]] for block in w.extents()] == [[[l[0], h[0]]] * 2 for l, h in want]
    assert [a.tolist() for a in w.total()] == [[[min(values[:333]), 0]], [[max(values[:333]), 0]]]
    assert w.peaks()[:, 0, 0].tolist() == mono.level_history(100, 250).peaks()[:, 0, 0].tolist()


# ---- 7: the song ---------------------------------------------------------------------------------------------------------------------------
def extremes_of(sample, a, b, width):
    """audioop.minmax per channel of frames [a, b) of a stereo Sample's own bytes"""
    data = bytes(sample.view_frame_data())[2 * a * width:2 * b * width]
    sides = [b"".join(data[k + c * width:k + (c + 1) * width] for k in range(0, len(data), 2 * width)) for c in range(2)]
    pairs = [audioop.minmax(side, width) for side in sides]
    return (pairs[0][0], pairs[1][0]), (pairs[0][1], pairs[1][1])


@gpu_test
@pytest.mark.parametrize("width", [2, 4])
def test_the_waveform_of_a_desk_that_rides_its_buses_and_pans(gpu, width):
    from synthesizer_amd import mixer
    instruments, tracks, _subs, _total = six("pile", width)
    samples = as_samples(instruments, width, RATE)
    F = TILE[width] // 2
    gains, pans, master_gain, name = SETTINGS[0]
    gains = tuple(gains[:5]) + (0.0,)                           # track 5, loose behind the groups, is muted
    groups = LISTS[name]
    with mixer.compile_tracks([with_samples(samples, t) for t in tracks], RATE, 2, width) as cs:
        frames = cs.frames
        auto = cs.automation([[(10, F + 40, 0.2, 0.9)]] + [None] * 5, master=[(F // 2, frames, 1.0, 0.0)],      # the desk of tests/test_gpu_level_blocks.py
                             groups=[[(0, F + 7, 0.5, 0.8)]] + [None] * (len(groups) - 1),
                             pans=[None, [(3, 2 * F + 9, -1.0, 1.0)]] + [None] * 4, group_pans=[[(F - 20, F + 300, 0.8, -0.6)]])
        kw = dict(gains=gains, pans=pans, master=master_gain, groups=groups, automation=auto)
        a, n = F // 2 + 3, frames - F
        st = cs.stems(a, n, **kw)
        rows = st.rows()
        for B in (None, 300):
            w = st.waveform(B)
            size = F if B is None else B
            assert isinstance(w, mixer.Waveform) and w.block_frames == size and len(w) == (a + n - 1) // size - a // size + 1
            assert w.ngroups == len(groups) and w.lo.shape == (len(w), len(rows), 2) and (w.start_frame, w.frames) == (a, n)
            for j, (lo, count) in enumerate(zip(w.starts, w.block_counts)):
                for r, sample in enumerate(rows):
                    got = (tuple(w.lo[j, r].tolist()), tuple(w.hi[j, r].tolist()))
                    assert got == extremes_of(sample, lo - a, lo - a + count, width), (B, j, r)
            h = st.level_history(B)
            assert np.array_equal(w.peaks(), h.peaks()) and w.starts == h.starts and w.block_counts == h.block_counts, B      # block for block
            whole = cs.waveform(a, n, block_frames=B, **kw)     # stems, then their extremes: the same table
            assert np.array_equal(whole.lo, w.lo) and np.array_equal(whole.hi, w.hi) and whole.starts == w.starts and whole.ngroups == w.ngroups
            assert not w.lo[:, 5].any() and not w.hi[:, 5].any()      # the muted track reads (0, 0) in every block
            by_hand = mixer.SongStems(st.tracks, st.master, st.groups, a, n).waveform(size)      # one launch per row: the same table
            assert np.array_equal(by_hand.lo, w.lo) and np.array_equal(by_hand.hi, w.hi)
        assert (w.lo[:, 6] < 0).any() and (w.hi[:, 6] > 0).any() and any(w.hi[:, 7 + g].max() > 0 for g in range(len(groups)))      # the desk sounds
        e = cs.waveform(7, 0, groups=groups)
        assert len(e) == 0 and e.lo.shape == (0, 7 + len(groups), 2)
        auto.close()


# ---- 8: what the entry point refuses ----------------------------------------------------------------------------------------------------------
@gpu_test
def test_the_entry_point_refuses_on_the_host_and_writes_nothing(gpu):
    N = gpu
    lib = N.lib()
    buf = N.DeviceBuffer.from_bytes(bytes(4000))                # 2000 samples of 16 bits
    rows = (N.PcmExtent * 64)()
    C.memset(rows, 0x5A, C.sizeof(rows))
    untouched = bytes(rows)

    def call(b=buf.handle, off=0, n=100, nch=2, width=2, plane=200, nplanes=3, origin=5, B=50, out=rows, nblocks=3):
        return b, off, n, nch, width, plane, nplanes, origin, B, out, nblocks
    for what, args, message in (
        ("three channels", call(nch=3), b"3 channels (1 or 2)"),
        ("no channel", call(nch=0), b"0 channels (1 or 2)"),
        ("a width of five", call(width=5), b"sample width 5 not in {1,2,3,4}"),
        ("a width of zero", call(width=0), b"sample width 0 not in {1,2,3,4}"),
        ("blocks of no frame", call(B=0), b"blocks of 0 frames"),
        ("no plane", call(nplanes=0), b"0 planes"),
        ("planes closer than the window", call(plane=199), b"planes 199 samples apart for a window of 200: they would overlap"),
        ("a last plane that ends one sample past in", call(off=1401), b"the last of 3 planes ends outside in"),
        ("one plane past in", call(off=1801, nplanes=1), b"the last of 1 planes ends outside in"),
        ("a window past 2^64 frames", call(origin=2 ** 64 - 50), b"the window ends past 2^64 frames"),
        ("a block too many", call(nblocks=4), b"4 blocks for a window of 3"),
        ("a block too few", call(nblocks=2), b"2 blocks for a window of 3"),
        ("blocks for an empty window", call(n=0, plane=0, nblocks=1), b"1 blocks for a window of 0"),
        ("no rows", call(out=None), b"NULL rows"),
        ("no buffer", call(b=None), b"NULL buffer"),
    ):
        assert lib.sh_pcm_extent_blocks(*args) == N.SH_ERR_INVALID, what
        err = lib.sh_last_error()
        assert err.startswith(b"sh_pcm_extent_blocks: ") and message in err, (what, err)
        assert bytes(rows) == untouched, what
    # what it takes: the call as it stands, its last plane ending with in, and one plane whose stride says nothing
    assert lib.sh_pcm_extent_blocks(*call()) == N.SH_OK and bytes(rows)[:9 * 16] == bytes(9 * 16) and bytes(rows)[9 * 16:] == untouched[9 * 16:]
    assert lib.sh_pcm_extent_blocks(*call(off=1400)) == N.SH_OK
    assert lib.sh_pcm_extent_blocks(*call(nplanes=1, plane=0, off=1800)) == N.SH_OK
    assert lib.sh_pcm_extent_blocks(*call(n=0, plane=0, nblocks=0, out=None)) == N.SH_OK
