"""sh_pcm_limit / ``mixer.limit`` / ``mixer.limit_into`` / ``mixer.limit_gain`` / ``Sample.limit`` on the GPU, held to byte equality
throughout.  Expected bytes never come from the code under test: the reference is tests/limitref.py's numpy form (two prefix minima
in int64, which tests/test_pcmlimit.py holds to the definition by brute force), and a closed form, min(ONE, g + s * distance), for the
single peaks.

The shapes are sized from the kernels' own division, T = N.PCM_LIMIT_TILE_FRAMES frames per workgroup on the sample's own grid:
samples of {1, 2, T - 1, T, T + 1, 3 T + 5} frames under attacks and releases from {0, 1, 2, 7, T - 1, T, T + 1, 2 T + 3}, widths
1, 2 and 4, mono and stereo, the input quiet noise with sparse peaks; single peaks at frame 0, at the last frame, at a tile's last
frame and at the next one's first; 2^20 frames of release and of attack, which is the whole carry; windows that begin and end inside
a tile, of one frame, with peaks just outside them, and the whole result assembled from windows of 1000 frames; the call in place;
every operand as a DeviceBuffer.view at residues 0, 2 and 15 mod 16 inside sentinel-filled parents; the wall, unity and the slopes on
the GPU's own output; the rails; every refusal of the C entry point with the destination left untouched."""
import ctypes as C

import numpy as np
import pytest

from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample
from tests import limitref
from tests.helpers import pcm_view_call

pytestmark = pytest.mark.gpu
RATE = 48000
ONE = limitref.ONE
CASES = [(w, nch) for w in (1, 2, 4) for nch in (1, 2)]


def sample_of(values, width):
    return Sample.from_raw_frames(limitref.pcm(values, width), width, RATE, values.shape[1])


def frames_of(sample):
    """a Sample's bytes as int64 (frames, nch)"""
    raw = bytes(sample.view_frame_data())
    return np.frombuffer(raw, dtype=limitref.DTYPES[sample.samplewidth]).astype(np.int64).reshape(-1, sample.nchannels)


def spans(T):
    return (0, 1, 2, 7, T - 1, T, T + 1, 2 * T + 3)


@pytest.mark.parametrize("width,nch", CASES)
def test_every_length_against_the_reference(gpu, width, nch):
    """Every length under eight pairs of attack and release, each of the eight values on either side.  From T - 1 frames on every case
    must hold frames at unity AND frames below it (asserted on the reference's G): the peaks are mild where a ramp is longer than 7
    frames -- about a tenth above the ceiling, so the gain is back at unity within an eighth of 2 T + 3 frames, some 500 -- and lie
    in the sample's second half, T / 2 - 1 > 1000 frames from its start.  One or two frames cannot hold both under every ramp; those
    cases together must."""
    T = gpu.PCM_LIMIT_TILE_FRAMES
    rng = np.random.default_rng(1000 * width + nch)
    S = spans(T)
    ceiling = limitref.hi_of(width) // 2
    seen = set()
    for n in (1, 2, T - 1, T, T + 1, 3 * T + 5):
        for k in range(8):
            attack, release = S[k], S[(k + 3) % 8]
            peaks = [0] if n <= 2 else np.unique(rng.integers(n // 2, n, 4))
            x = limitref.noise_with_peaks(rng, width, n, nch, ceiling, peaks=peaks, mild=max(attack, release) > 7)
            wy, wG = limitref.limit(x, ceiling, attack, release)
            if n > 2:
                assert (wG == ONE).any() and (wG < ONE).any(), (n, attack, release)
            seen |= {bool(v) for v in (wG == ONE)} if n <= 2 else set()
            xs = sample_of(x, width).to_device().lock()
            got = mixer.limit(xs, ceiling, attack, release)
            assert len(got) == n and (got.nchannels, got.samplewidth, got.samplerate) == (nch, width, RATE)
            assert np.array_equal(frames_of(got), wy), (n, attack, release)
            G = mixer.limit_gain(xs, ceiling, attack, release)
            assert G.dtype == np.uint32 and np.array_equal(G.astype(np.int64), wG), (n, attack, release)
            assert np.array_equal(frames_of(xs), x)             # the input is read only
    assert seen == {True, False}


@pytest.mark.parametrize("width,nch", [(2, 1), (4, 2), (1, 2)])
def test_a_single_peak_against_the_closed_form(gpu, width, nch):
    """one peak at frame 0, at the last frame, at a tile's last frame, at the next tile's first: G[i] = min(ONE, g + s * |i - p|), s the
    attack's slope in front of the peak and the release's behind it"""
    T = gpu.PCM_LIMIT_TILE_FRAMES
    n = 2 * T + 3
    hi = limitref.hi_of(width)
    ceiling = hi // 3
    i = np.arange(n, dtype=np.int64)
    for p in (0, n - 1, T - 1, T):
        for attack, release in ((0, 0), (7, 2), (T + 1, 2 * T + 3), (2 * T + 3, T - 1), (1, T)):
            x = np.full((n, nch), ceiling // 5, dtype=np.int64)
            x[::2] *= -1
            x[p, nch - 1] = -hi - 1
            g = (ceiling * ONE) // (hi + 1)
            want = np.minimum(ONE, g + np.where(i < p, (p - i) * limitref.slope(attack), (i - p) * limitref.slope(release)))
            xs = sample_of(x, width).to_device()
            assert np.array_equal(mixer.limit_gain(xs, ceiling, attack, release).astype(np.int64), want), (p, attack, release)
            assert np.array_equal(frames_of(mixer.limit(xs, ceiling, attack, release)), (x * want[:, None]) >> 30), (p, attack, release)


def test_the_full_lookback_two_to_the_20_frames(gpu):
    """n = 2^20 + 2 T + 3 at width 1, mono: a peak at frame 0 under a release of 2^20 frames and a peak at the last frame under an
    attack of 2^20 frames; every tile folds the carry over as many summaries as the sample holds on that side, up to the bound.  The
    expected gains come from the closed form.  A peak beyond the reach changes nothing: the frames 2^20 and more away are the bytes
    of the sample without the peak."""
    T = gpu.PCM_LIMIT_TILE_FRAMES
    M = gpu.PCM_LIMIT_MAX_FRAMES
    n = M + 2 * T + 3
    rng = np.random.default_rng(9)
    quiet = rng.integers(-3, 4, (n, 1), dtype=np.int64)
    i = np.arange(n, dtype=np.int64)
    g = (12 * ONE) // 128
    assert limitref.slope(M) == 1024 and limitref.reach(M) == M and g + (M - 1) * 1024 >= ONE
    for p, attack, release in ((0, 0, M), (n - 1, M, 0), (0, M, M), (n - 1, M, M)):
        x = quiet.copy()
        x[p] = -128
        want = np.minimum(ONE, g + np.abs(i - p) * 1024)
        xs = sample_of(x, 1).to_device()
        G = mixer.limit_gain(xs, 12, attack, release).astype(np.int64)
        assert np.array_equal(G, want), (p, int(np.flatnonzero(G != want)[0]))
        assert np.array_equal(frames_of(mixer.limit(xs, 12, attack, release)), (x * want[:, None]) >> 30)
        far = i[np.abs(i - p) >= M]
        assert far.size == 2 * T + 3 and (want[far] == ONE).all() and (want[np.abs(i - p) < M - 2 ** 17] < ONE).all()
        first = int(far[0])
        assert bytes(mixer.limit(xs, 12, attack, release, first, far.size).view_frame_data()) == limitref.pcm(quiet[far], 1)
    # the lowest gain a width admits at the far end of the ramp: g = 2^23 (x = -128 under a ceiling of 1), unity 2^20 - 2^13 frames on
    x = np.clip(quiet, -1, 1)
    x[0] = -128
    want = np.minimum(ONE, 2 ** 23 + i * 1024)
    assert want[M - 2 ** 13 - 1] < ONE == want[M - 2 ** 13]
    assert np.array_equal(mixer.limit_gain(sample_of(x, 1).to_device(), 1, 0, M, M - 2 ** 13 - T, 2 * T).astype(np.int64), want[M - 2 ** 13 - T:M - 2 ** 13 + T])


@pytest.mark.parametrize("width", [1, 2, 4])
def test_a_window_is_that_slice_of_the_whole_result(gpu, width):
    T = gpu.PCM_LIMIT_TILE_FRAMES
    rng = np.random.default_rng(50 + width)
    n, nch, attack, release = 3 * T + 300, 2, 300, T + 1
    ceiling = limitref.hi_of(width) // 3
    # peaks just outside the windows below on either side, and at the tiles' edges
    x = limitref.noise_with_peaks(rng, width, n, nch, ceiling, peaks=[4, T - 3, T - 1, T, T + 517, 2 * T + 99, 2 * T + 111, n - 1])
    wy, wG = limitref.limit(x, ceiling, attack, release)
    assert (wG == ONE).any() and (wG < ONE).any()
    xs = sample_of(x, width).to_device()
    assert np.array_equal(frames_of(mixer.limit(xs, ceiling, attack, release)), wy)
    pairs = [(0, 1), (0, T), (0, T + 1), (5, 100), (5, T), (T - 2, 1), (T - 1, 2), (T, 1), (T + 17, T + 500), (2 * T + 100, 11), (n - 3, 3), (n - 1, 1), (3, n - 3)]
    for first, count in pairs:
        got = mixer.limit(xs, ceiling, attack, release, start_frame=first, nframes=count)
        assert len(got) == count and np.array_equal(frames_of(got), wy[first:first + count]), (first, count)
        assert np.array_equal(mixer.limit_gain(xs, ceiling, attack, release, first, count).astype(np.int64), wG[first:first + count]), (first, count)
    assert len(mixer.limit(xs, ceiling, attack, release, start_frame=n)) == 0 and len(mixer.limit(xs, ceiling, attack, release, 7, 0)) == 0
    # the whole result assembled from windows of 1000 frames, each written into its place of one buffer
    fb = nch * width
    buf = gpu.DeviceBuffer(n * fb)
    for first in range(0, n, 1000):
        assert mixer.limit_into(buf, first * fb, xs, ceiling, attack, release, first, min(1000, n - first)) == min(1000, n - first)
    assert buf.download_bytes(n * fb) == limitref.pcm(wy, width)
    # and in place, window by window: a window's own bytes are written, the frames outside it still shape it as they were
    own = sample_of(x, width).to_device()
    L = gpu.lib()
    for first in range(0, n, 1000):
        count = min(1000, n - first)
        assert L.sh_pcm_limit(own._device().handle, 0, n, nch, width, ceiling, attack, release, first, count, own._device().handle, first * fb, None, 0) == 0
        gpu.sync()
        want = x.copy()
        want[first:first + count] = limitref.limit(x, ceiling, attack, release)[0][first:first + count]
        assert own._device().download_bytes(n * fb) == limitref.pcm(want, width), first
        own._device().upload(np.frombuffer(limitref.pcm(x, width), dtype=np.uint8))


@pytest.mark.parametrize("width,nch", CASES)
def test_in_place_is_the_copying_form(gpu, width, nch):
    """Sample.limit equals mixer.limit, by its seconds and by ceiling_db; in its own buffer"""
    T = gpu.PCM_LIMIT_TILE_FRAMES
    rng = np.random.default_rng(70 + 10 * width + nch)
    hi = limitref.hi_of(width)
    n = 2 * T + 77
    x = limitref.noise_with_peaks(rng, width, n, nch, hi // 2, peaks=[0, 900, T - 1, T, T + 1000, n - 1])
    for kw, ceiling, attack, release in ((dict(ceiling=hi // 2), hi // 2, 240, 9600), (dict(ceiling_db=-6.0, attack=0.001, release=0.01), int(hi * 10 ** (-6.0 / 20)), 48, 480),
                                         (dict(ceiling=hi // 2, attack=0, release=0), hi // 2, 0, 0)):
        s = sample_of(x, width).to_device()
        buf = s._device()
        assert s.limit(**kw) is s and s._device() is buf and len(s) == n
        want = limitref.limit(x, ceiling, attack, release)[0]
        assert np.array_equal(frames_of(s), want), kw
        assert np.array_equal(frames_of(mixer.limit(sample_of(x, width), ceiling, attack, release)), want), kw
        assert int(np.abs(want).max()) <= ceiling


@pytest.mark.parametrize("width", [1, 2, 4])
def test_every_operand_as_a_view_at_residues_0_2_and_15(gpu, width):
    """in, out and the gain plane each as a DeviceBuffer.view at residues 0, 2 and 15 mod 16 inside sentinel-filled parents, and the call
    in place on such a view: pcm_view_call asserts that no byte outside the destination changed and that the inputs are untouched.  The
    sentinels around the input are loud samples: a kernel that read a frame outside [0, n) would lower the gains at the edges."""
    L = gpu.lib()
    T = gpu.PCM_LIMIT_TILE_FRAMES
    rng = np.random.default_rng(90 + width)
    residues = (0, 2, 15)
    for nch in (1, 2):
        n, attack, release = T + 9, 40, 700
        ceiling = limitref.hi_of(width) // 4
        x = limitref.noise_with_peaks(rng, width, n, nch, ceiling, peaks=[3, 777, 1200])
        x[3, 0] = limitref.hi_of(width)                         # (loud: the gain at frame 0 is below unity; at the last frame it is back)
        raw = limitref.pcm(x, width)
        wy, wG = limitref.limit(x, ceiling, attack, release)
        assert wG[0] < ONE and wG[n - 1] == ONE
        fb = nch * width
        for first, count in ((0, n), (3, n - 8)):
            want = limitref.pcm(wy[first:first + count], width)
            want_gain = wG[first:first + count].astype(np.uint32).tobytes()
            for a_in, a_out in [(a, 0) for a in residues] + [(0, a) for a in residues[1:]] + [(2, 15), (15, 2), (15, 15)]:
                rc, got = pcm_view_call(gpu, [(raw, a_in)], len(want), a_out,
                                        lambda iv, ov: L.sh_pcm_limit(iv[0].handle, 0, n, nch, width, ceiling, attack, release, first, count, ov.handle, 0, None, 0))
                assert rc == 0 and got == want, (nch, first, a_in, a_out, rc)
                rc, got = pcm_view_call(gpu, [(raw, a_in)], len(want_gain), a_out,
                                        lambda iv, ov: L.sh_pcm_limit(iv[0].handle, 0, n, nch, width, ceiling, attack, release, first, count, None, 0, ov.handle, 0))
                assert rc == 0 and got == want_gain, (nch, first, a_in, a_out, rc)
            for a in residues:
                def in_place(_iv, ov):
                    ov.upload(np.frombuffer(raw, dtype=np.uint8))
                    return L.sh_pcm_limit(ov.handle, 0, n, nch, width, ceiling, attack, release, first, count, ov.handle, first * fb, None, 0)
                rc, got = pcm_view_call(gpu, [], len(raw), a, in_place)
                assert rc == 0 and got == raw[:first * fb] + want + raw[(first + count) * fb:], (nch, first, a, rc)


@pytest.mark.parametrize("width,nch", CASES)
def test_the_wall_unity_and_the_slopes_on_the_gpus_own_output(gpu, width, nch):
    T = gpu.PCM_LIMIT_TILE_FRAMES
    rng = np.random.default_rng(200 + 10 * width + nch)
    hi = limitref.hi_of(width)
    n = 4 * T + 123
    for ceiling, attack, release in ((hi // 2, 7, 300), (max(hi // 50, 1), T + 1, 2 * T + 3), (hi - 1, 0, T), (1, 3, 0)):
        x = limitref.noise_with_peaks(rng, width, n, nch, max(ceiling, 8), peaks=np.unique(rng.integers(n // 2, n, 6)) if attack > 7 else None, mild=attack > 7)
        if ceiling == 1:
            x[T:3 * T] = rng.integers(-1, 2, (2 * T, nch))       # (frames that need no gain under a ceiling of 1)
        xs = sample_of(x, width).to_device()
        y = frames_of(mixer.limit(xs, ceiling, attack, release))
        G = mixer.limit_gain(xs, ceiling, attack, release).astype(np.int64)
        wG = limitref.gain(x, ceiling, attack, release)
        assert (wG == ONE).any() and (wG < ONE).any(), (ceiling, attack, release)
        assert int(np.abs(y).max()) <= ceiling                                          # the wall
        assert np.array_equal(y[wG == ONE], x[wG == ONE])                               # untouched at unity
        d = np.diff(G)
        assert int((-d).max()) <= limitref.slope(attack) and int(d.max()) <= limitref.slope(release)
        assert np.array_equal(G, wG) and int(G.max()) <= ONE
    x = np.clip(x, -1000 if width > 1 else -100, 1000 if width > 1 else 100)
    back = mixer.limit(sample_of(x, width), int(np.abs(x).max()), 5, 50)               # a sample under the ceiling comes back byte for byte
    assert bytes(back.view_frame_data()) == limitref.pcm(x, width)


@pytest.mark.parametrize("width", [1, 2, 4])
def test_the_rails(gpu, width):
    """x = -2^(8w-1) on every sample under a ceiling of 1 and of HI; and the rails beside silence"""
    hi = limitref.hi_of(width)
    T = gpu.PCM_LIMIT_TILE_FRAMES
    for nch in (1, 2):
        low = np.full((T + 5, nch), -hi - 1, dtype=np.int64)
        mixed = np.array([[-hi - 1, 0], [hi, -hi - 1], [0, 0], [-1, 1], [hi, hi], [1, -hi]], dtype=np.int64)[:, :nch]
        for x in (low, mixed):
            for ceiling in (1, hi):
                for attack, release in ((0, 0), (2, 3)):
                    wy, wG = limitref.limit(x, ceiling, attack, release)
                    assert int(np.abs(wy).max()) <= ceiling
                    xs = sample_of(x, width).to_device()
                    assert np.array_equal(frames_of(mixer.limit(xs, ceiling, attack, release)), wy), (nch, ceiling, attack)
                    assert np.array_equal(mixer.limit_gain(xs, ceiling, attack, release).astype(np.int64), wG), (nch, ceiling, attack)
        g = (hi * ONE) // (hi + 1)
        assert limitref.gain(low, hi, 0, 0).tolist() == [g] * (T + 5) and limitref.gain(low, 1, 0, 0).tolist() == [ONE // (hi + 1)] * (T + 5)


def test_every_refusal_of_the_entry_point_leaves_the_destination_alone(gpu):
    L = gpu.lib()
    rng = np.random.default_rng(3)
    n = 100
    x = limitref.pcm(limitref.noise_with_peaks(rng, 2, n, 2, 5000), 2)
    out_bytes = n * 4

    def call(width=2, nch=2, in_frames=n, ceiling=5000, attack=10, release=100, first=0, count=n, in_off=0, out_off=0, gain=False, gain_off=0):
        if gain:
            return lambda iv, ov: L.sh_pcm_limit(iv[0].handle, in_off, in_frames, nch, width, ceiling, attack, release, first, count, None, 0, ov.handle, gain_off)
        return lambda iv, ov: L.sh_pcm_limit(iv[0].handle, in_off, in_frames, nch, width, ceiling, attack, release, first, count, ov.handle, out_off, None, 0)
    refusals = [
        (call(width=3), "width 3 is not built"), (call(width=0), "not in {1,2,4}"), (call(width=8), "not in {1,2,4}"),
        (call(nch=3), "3 channels"), (call(nch=0), "0 channels"),
        (call(ceiling=0), "a ceiling of 0 is not in [1, 32767]"), (call(ceiling=32768), "a ceiling of 32768"), (call(width=1, ceiling=128), "not in [1, 127]"),
        (call(attack=2 ** 20 + 1), "an attack of 1048577 frames"), (call(release=2 ** 20 + 1), "a release of 1048577 frames"),
        (call(count=n + 1), "reach past the sample's 100"), (call(first=1), "reach past the sample's 100"), (call(first=101, count=0), "reach past the sample's 100"),
        (call(in_frames=n + 1, count=1), "input range outside buffer"), (call(in_off=4), "input range outside buffer"),
        (call(out_off=4), "output range outside buffer"), (call(out_off=out_bytes + 1, count=0), "output range outside buffer"),
        (call(gain=True, gain_off=4), "gain range outside buffer"), (call(gain=True, gain_off=out_bytes + 1, count=0), "gain range outside buffer"),
    ]
    for how, text in refusals:
        rc, _ = pcm_view_call(gpu, [(x, 0)], out_bytes, 0, how, untouched=True)
        assert rc == gpu.SH_ERR_INVALID and text in L.sh_last_error().decode() and "sh_pcm_limit: " in L.sh_last_error().decode(), (text, rc, L.sh_last_error())
    # the overlaps: the views are cut from ONE parent
    img = np.full(4096, 0x5A, dtype=np.uint8)
    parent = gpu.DeviceBuffer.from_array(img)
    try:
        a = parent.view(0, len(x))
        args = (0, n, 2, 2, 5000, 10, 100)
        for dst, first, count in ((parent.view(len(x) - 2, out_bytes), 0, n), (parent.view(2, out_bytes), 0, n), (parent.view(40, 360), 9, 90),
                                  (parent.view(44, 356), 10, 89), (parent.view(0, 40), 90, 10)):
            assert L.sh_pcm_limit(a.handle, *args, first, count, dst.handle, 0, None, 0) == gpu.SH_ERR_INVALID
            assert "out overlaps the input and is not the window's own bytes" in L.sh_last_error().decode()
        far = parent.view(2048, out_bytes)
        for plane in (parent.view(len(x) - 1, 400), parent.view(396, 400), parent.view(2048 + out_bytes - 1, 400), parent.view(2048 - 399, 400)):
            assert L.sh_pcm_limit(a.handle, *args, 0, n, far.handle, 0, plane.handle, 0) == gpu.SH_ERR_INVALID and "gain overlaps the input or out" in L.sh_last_error().decode()
        assert L.sh_pcm_limit(a.handle, *args, 0, 10, None, 0, parent.view(300, 40).handle, 0) == gpu.SH_ERR_INVALID            # the WHOLE input counts
        assert "gain overlaps the input or out" in L.sh_last_error().decode()
        assert L.sh_pcm_limit(a.handle, *args, 0, n, None, 0, None, 0) == gpu.SH_ERR_INVALID and "neither out nor gain" in L.sh_last_error().decode()
        assert L.sh_pcm_limit(a.handle, *args, 5, 0, parent.view(2, 400).handle, 0, None, 0) == 0                               # an empty window writes nothing
        assert L.sh_pcm_limit(a.handle, *args, 5, 0, None, 0, None, 0) == gpu.SH_ERR_INVALID                                    # (but names a destination)
        gpu.sync()
        assert parent.download(np.uint8, img.size).tobytes() == img.tobytes()
        # side by side is no overlap; exactly the window's own bytes is the call in place
        parent.upload(np.frombuffer(x, dtype=np.uint8))
        assert L.sh_pcm_limit(a.handle, *args, 0, n, parent.view(len(x), out_bytes).handle, 0, parent.view(2 * len(x), 4 * n).handle, 0) == 0
        assert L.sh_pcm_limit(a.handle, *args, 10, 90, parent.view(40, 360).handle, 0, None, 0) == 0
        gpu.sync()
        got = parent.download(np.uint8, img.size)
        xv = np.frombuffer(x, dtype=np.int16).astype(np.int64).reshape(n, 2)
        wy, wG = limitref.limit(xv, 5000, 10, 100)
        assert got[len(x):2 * len(x)].tobytes() == limitref.pcm(wy, 2) and got[2 * len(x):2 * len(x) + 4 * n].tobytes() == wG.astype(np.uint32).tobytes()
        assert got[:len(x)].tobytes() == x[:40] + limitref.pcm(wy[10:], 2) and (got[2 * len(x) + 4 * n:] == 0x5A).all()
    finally:
        parent.free()
    args = [None, 0, n, 2, 2, 5000, 10, 100, 0, 1, C.c_void_p(1), 0, None, 0]
    assert L.sh_pcm_limit(*args) == gpu.SH_ERR_INVALID and "NULL buffer" in L.sh_last_error().decode()
