"""sh_pcm_resample_fir / ``mixer.resample_fir`` / ``mixer.resample_fir_into`` / ``Sample.resample_fir`` on the GPU, held to byte
equality throughout.  Expected bytes never come from the code under test: the reference is tests/resampleref.py (``numpy.convolve``
over int64 per phase, audioop's fbound written out), the live ``audioop`` and the package's own convolution for the ties, and a closed
form for the bound.

The shapes are sized from the kernel's own division (N.PCM_RESAMPLE_*): a group is P = copies * up outputs from copies * down input
frames, a wave owns B = 64 groups, a chunk of steps is K = 1024: inputs of 1 and 2 frames and of B - 1, B, B + 1, 2 B and 3 B groups'
worth, under 1, 2, L - 1, L, L + 1 and 8 L + 3 taps at delays 0, (m - 1) // 2 and m - 1, for thirteen ratios on both sides of one --
small ups, where a workgroup owns several blocks, among them -- and rows longer than K through L = 1 with 2 K + 5 taps; both widths,
mono and stereo; windows; every operand as a DeviceBuffer.view at residues 0, 2 and 15 mod 16 inside sentinel-filled parents; 2^22 taps
at the rails; every refusal of the C entry point with the destination left untouched."""
import audioop
import ctypes as C

import numpy as np
import pytest

from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample
from tests import firref, resampleref
from tests.helpers import pcm_view_call

pytestmark = pytest.mark.gpu
RATE = 48000
RATIOS = [(1, 1), (2, 1), (1, 2), (3, 2), (2, 3), (7, 8), (8, 1), (1, 8), (5, 3), (4, 6), (160, 147), (147, 160), (80, 441)]
FORMATS = [(1, 1), (1, 2), (2, 1), (2, 2)]                       # (width, channels)


def sample_of(values, width, rate=RATE):
    return Sample.from_raw_frames(firref.pcm(values, width), width, rate, values.shape[1])


def frames_of(sample):
    """a Sample's bytes as int64 (frames, nch)"""
    raw = bytes(sample.view_frame_data())
    return np.frombuffer(raw, dtype=firref.DTYPES[sample.samplewidth]).astype(np.int64).reshape(-1, sample.nchannels)


def taps_of(h):
    return np.asarray(h).astype(np.int16)


def convert(xs, L, M, h, factor, delay, **kw):
    """mixer.resample_fir of a Sample at 100 M Hz to 100 L Hz (L and M coprime: the mixer reduces the rates by their gcd)"""
    return mixer.resample_fir(xs, xs.samplerate // M * L, taps_of(h), factor, delay, **kw)


def tap_counts(L):
    return sorted({1, 2, max(L - 1, 1), L, L + 1, 8 * L + 3})


@pytest.mark.parametrize("width,nch", FORMATS)
def test_the_grid_of_ratios_taps_delays_and_lengths(gpu, width, nch):
    """the unreduced ratio through the entry point itself (4/6 stays 4/6); every length under every ratio, tap count and delay where the
    ratio is small, two of the seven in turn where it is large (160/147, 147/160, 80/441: a reference of some milliseconds a case)"""
    Lb = gpu.lib()
    B = gpu.PCM_RESAMPLE_BLOCK_GROUPS
    rng = np.random.default_rng(1000 * width + nch)
    factors = (2.0 ** -14, 2.0 ** -(8 * width + 10), 1.0)
    k, seen = 0, set()
    for L, M in RATIOS:
        per = gpu.pcm_resample_copies(L) * M                     # input frames of one group
        lengths = [1, 2, (B - 1) * per, B * per, (B + 1) * per, 2 * B * per, 3 * B * per]
        xs = {n: firref.rand_frames(rng, width, n, nch) for n in lengths}
        dev = {n: gpu.DeviceBuffer.from_bytes(firref.pcm(x, width)) for n, x in xs.items()}
        for m in tap_counts(L):
            h = resampleref.rand_taps(rng, m)
            hb = gpu.DeviceBuffer.from_bytes(taps_of(h).tobytes())
            for delay in sorted({0, (m - 1) // 2, m - 1}):
                mine = lengths if L * M < 1000 else [lengths[(k + i) % 7] for i in (0, 3)]
                for n in mine:
                    factor = factors[k % 3]
                    k += 1
                    want = resampleref.resample(xs[n], h, L, M, delay, factor, width)
                    total = len(want)
                    assert Lb.sh_pcm_resample_fir_frames(n, L, M) == total == -(-n * L // M)
                    out = gpu.DeviceBuffer(total * nch * width)
                    gpu.check(Lb.sh_pcm_resample_fir(dev[n].handle, 0, n, nch, width, hb.handle, 0, m, L, M, delay, factor, 0, total, out.handle, 0))
                    assert out.download_bytes(total * nch * width) == firref.pcm(want, width), (L, M, m, delay, n, factor)
                    seen |= {int(want.min()), int(want.max())}
        for n, x in xs.items():
            assert dev[n].download_bytes(len(x) * nch * width) == firref.pcm(x, width)            # the input is read only
    assert set(firref.lo_hi(width)) <= seen                      # both rails were reached


@pytest.mark.parametrize("width,nch", FORMATS)
def test_rows_longer_than_a_chunk_of_steps(gpu, width, nch):
    K, B = gpu.PCM_RESAMPLE_STEP_CHUNK, gpu.PCM_RESAMPLE_BLOCK_GROUPS
    rng = np.random.default_rng(40 + 10 * width + nch)
    for L, M, m, n in ((1, 1, 2 * K + 5, 8 * B + 77), (1, 1, 2 * K + 5, 700), (2, 3, 2 * K + 1, 1000), (3, 2, 3 * K + 7, 333), (160, 147, 160 * K + 9, 401)):
        x, h = firref.rand_frames(rng, width, n, nch), resampleref.rand_taps(rng, m)
        xs = sample_of(x, width, 100 * M).lock()
        for delay in (0, (m - 1) // 2, m - 1):
            want = resampleref.resample(x, h, L, M, delay, 2.0 ** -17, width)
            got = convert(xs, L, M, h, 2.0 ** -17, delay)
            assert (got.samplerate, got.nchannels, got.samplewidth) == (100 * L, nch, width)
            assert np.array_equal(frames_of(got), want), (L, M, m, delay)


@pytest.mark.parametrize("width,nch", FORMATS)
def test_a_window_is_that_slice_of_the_whole_result(gpu, width, nch):
    B = gpu.PCM_RESAMPLE_BLOCK_GROUPS
    rng = np.random.default_rng(50 + 10 * width + nch)
    for L, M in ((160, 147), (1, 6), (3, 2)):
        P = gpu.pcm_resample_copies(L) * L
        block = B * P                                            # the outputs of one block of groups
        n = -(-(4 * block + 300) * M // L) if L < 8 else -(-(block + 300) * M // L)
        x, h = firref.rand_frames(rng, width, n, nch), resampleref.rand_taps(rng, 77)
        whole = resampleref.resample(x, h, L, M, 30, 2.0 ** -15, width)
        total = len(whole)
        xs = sample_of(x, width, 100 * M).to_device()
        assert np.array_equal(frames_of(convert(xs, L, M, h, 2.0 ** -15, 30)), whole)
        pairs = [(0, 1), (7, 1), (total - 1, 1), (0, block), (5, block), (block - 1, 2), (P + 3, 2 * P), (block // 2, 3), (3, total - 3), (block + 11, 250)]
        for first, count in pairs:                                # begins and ends inside a block, one frame, across blocks
            got = convert(xs, L, M, h, 2.0 ** -15, 30, start_frame=first, nframes=count)
            assert len(got) == count and np.array_equal(frames_of(got), whole[first:first + count]), (L, M, first, count)
        assert len(convert(xs, L, M, h, 2.0 ** -15, 30, start_frame=total)) == 0 and len(convert(xs, L, M, h, 2.0 ** -15, 30, start_frame=7, nframes=0)) == 0
        # the whole result assembled from windows of 1000 frames, each written into its place of one buffer
        fb = nch * width
        buf = gpu.DeviceBuffer(total * fb)
        for first in range(0, total, 1000):
            count = min(1000, total - first)
            assert mixer.resample_fir_into(buf, first * fb, xs, 100 * L, taps_of(h), 2.0 ** -15, 30, first, count) == count
        assert buf.download_bytes(total * fb) == firref.pcm(whole, width)


@pytest.mark.parametrize("width", [1, 2])
def test_every_operand_as_a_view_at_residues_0_2_and_15(gpu, width):
    """in, taps and out each as a DeviceBuffer.view at residues 0, 2 and 15 mod 16 inside sentinel-filled parents: pcm_view_call asserts
    that no byte outside the destination changed and that the inputs are untouched"""
    Lb = gpu.lib()
    rng = np.random.default_rng(90 + width)
    residues = (0, 2, 15)
    for nch in (1, 2):
        for L, M in ((160, 147), (3, 2)):
            n, m, delay = 70 * gpu.pcm_resample_copies(L) * M + 9, 3 * L + 5, L + 1
            x, h = firref.rand_frames(rng, width, n, nch), resampleref.rand_taps(rng, m)
            whole = resampleref.resample(x, h, L, M, delay, 2.0 ** -16, width)
            first, count = 3, len(whole) - 8
            want = firref.pcm(whole[first:first + count], width)
            cases = [(a, 0, 0) for a in residues] + [(0, a, 0) for a in residues[1:]] + [(0, 0, a) for a in residues[1:]] + [(2, 15, 15), (15, 2, 2), (15, 15, 15)]
            for a_in, a_h, a_out in cases:
                rc, got = pcm_view_call(gpu, [(firref.pcm(x, width), a_in), (taps_of(h).tobytes(), a_h)], len(want), a_out,
                                        lambda iv, ov: Lb.sh_pcm_resample_fir(iv[0].handle, 0, n, nch, width, iv[1].handle, 0, m, L, M, delay, 2.0 ** -16, first, count,
                                                                              ov.handle, 0))
                assert rc == 0 and got == want, (nch, L, M, a_in, a_h, a_out, rc)


@pytest.mark.parametrize("nch", [1, 2])
def test_the_ties_that_need_no_numpy(gpu, nch):
    rng = np.random.default_rng(30 + nch)
    n = 64 * 8 * 3 + 77
    x = firref.rand_frames(rng, 2, n, nch)
    raw = firref.pcm(x, 2)
    # L = M = 1 is the package's own convolution, shifted by the delay
    h = resampleref.rand_taps(rng, 45)
    for delay in (0, 22, 44):
        got = mixer.resample_fir(sample_of(x, 2), RATE, taps_of(h), 2.0 ** -16, delay)
        want = mixer.convolve(sample_of(x, 2), Sample.from_raw_frames(taps_of(h).tobytes(), 2, RATE, 1), 2.0 ** -16, delay, n)
        assert len(got) == n and bytes(got.view_frame_data()) == bytes(want.view_frame_data()), delay
    one = np.array([1], dtype=np.int16)
    for width in (1, 2):
        xw = firref.rand_frames(rng, width, n, nch)
        dt = firref.DTYPES[width]
        arr = xw.astype(dt)
        for k in (2, 3, 8, 9):
            # taps [1] at factor 1.0: down by k keeps every k-th frame, up by k puts k - 1 zeros behind each
            got = mixer.resample_fir(sample_of(xw, width, k * 8000), 8000, one, 1.0, 0)
            assert bytes(got.view_frame_data()) == arr[::k].tobytes(), (width, k)
            got = mixer.resample_fir(sample_of(xw, width, 8000), k * 8000, one, 1.0, 0)
            stuffed = np.zeros((n * k, nch), dtype=dt)
            stuffed[::k] = arr
            assert bytes(got.view_frame_data()) == stuffed.tobytes(), (width, k)
            # k ones with up = k: each frame k times
            got = mixer.resample_fir(sample_of(xw, width, 8000), k * 8000, np.ones(k, dtype=np.int16), 1.0, 0)
            assert bytes(got.view_frame_data()) == np.repeat(arr, k, axis=0).tobytes(), (width, k)
        # one tap a with L = M = 1 is audioop.mul by a * factor, wherever that product is a float64 exactly
        for a, f in ((3, 0.25), (-5, 0.125), (7, 1.0), (-32768, 2.0 ** -15), (32767, 2.0 ** -16), (1, -1.5)):
            got = mixer.resample_fir(sample_of(xw, width), RATE, np.array([a], dtype=np.int16), f, 0)
            assert bytes(got.view_frame_data()) == audioop.mul(firref.pcm(xw, width), width, a * f), (width, a, f)
    assert raw == firref.pcm(x, 2)


def counted(sign_h, m, L, delay, n, factor):
    """x of n frames, all -32768, under m taps, all sign_h, up by L: output j sums one product for every frame i with
    0 <= j + delay - L i < m -- counted here, in integers -- and fbound follows: the closed form, no numpy.convolve"""
    j = np.arange(n * L, dtype=np.int64)[:, None] + delay - L * np.arange(n, dtype=np.int64)[None, :]
    acc = ((j >= 0) & (j < m)).sum(axis=1) * (-32768 * sign_h)
    assert int(np.abs(acc).max()) <= 2 ** 52
    return firref.fbound(acc.astype(np.float64) * factor, 2)


def test_the_bound_two_to_the_22_taps_at_the_rails(gpu):
    m, n = 2 ** 22, 64
    x = Sample.from_raw_frames(np.full(n, -32768, dtype=np.int16).tobytes(), 2, 8000, 1).to_device()
    for sign_h in (-32768, 32767):
        h = np.full(m, sign_h, dtype=np.int16)
        for L in (1, 4):
            for delay, factor in ((m - 11, 2.0 ** -22), (m - 11, 2.0 ** -20), (5, 2.0 ** -22), (m // 2, 2.0 ** -21)):
                want = counted(sign_h, m, L, delay, n, factor)
                got = frames_of(mixer.resample_fir(x, 8000 * L, h, factor, delay))[:, 0]
                assert np.array_equal(got, want), (sign_h, L, delay, got.tolist()[:20], want.tolist()[:20])
        # 64 products of 2^30 at 2^-20 pass the upper rail (65536) or reach the lower one: both were clamped above
        assert set(counted(sign_h, m, 1, m - 11, n, 2.0 ** -20).tolist()) >= ({32767} if sign_h < 0 else {-32768})


def test_every_refusal_of_the_entry_point_leaves_the_destination_alone(gpu):
    Lb = gpu.lib()
    rng = np.random.default_rng(3)
    n, m, up, down = 147, 10, 160, 147
    total = 160
    x, h = firref.pcm(firref.rand_frames(rng, 2, n, 2), 2), taps_of(resampleref.rand_taps(rng, m)).tobytes()
    out_bytes = total * 4

    def call(width=2, nch=2, in_frames=n, ntaps=m, up=up, down=down, delay=4, factor=0.5, first=0, count=total, in_off=0, taps_off=0, out_off=0):
        return lambda iv, ov: Lb.sh_pcm_resample_fir(iv[0].handle, in_off, in_frames, nch, width, iv[1].handle, taps_off, ntaps, up, down, delay, factor, first,
                                                     count, ov.handle, out_off)
    refusals = [
        (call(width=3), "widths 3 and 4 are not built"), (call(width=4), "widths 3 and 4 are not built"),
        (call(nch=3), "3 channels"), (call(nch=0), "0 channels"),
        (call(ntaps=0), "no taps"),
        (call(ntaps=2 ** 22 + 1), "taps are more than 4194304"),
        (call(up=0), "both at least 1"), (call(down=0), "both at least 1"),
        (call(up=4097), "up 4097 is more than 4096"),
        (call(up=1, down=63), "convert in two steps"), (call(up=8, down=504), "convert in two steps"),
        (call(delay=10), "a delay of 10 with 10 taps"),
        (call(factor=float("inf")), "not finite"), (call(factor=float("nan")), "not finite"),
        (call(count=total + 1), "reach past the result's 160"), (call(first=1), "reach past the result's 160"), (call(first=161, count=0), "reach past the result's 160"),
        (call(in_frames=n + 1, count=1), "input range outside buffer"), (call(in_off=4), "input range outside buffer"),
        (call(ntaps=m + 1, count=1), "taps range outside buffer"), (call(taps_off=2), "taps range outside buffer"),
        (call(out_off=4), "output range outside buffer"), (call(out_off=out_bytes + 1, count=0), "output range outside buffer"),
    ]
    for how, text in refusals:
        rc, _ = pcm_view_call(gpu, [(x, 0), (h, 0)], out_bytes, 0, how, untouched=True)
        assert rc == gpu.SH_ERR_INVALID and text in Lb.sh_last_error().decode() and "sh_pcm_resample_fir: " in Lb.sh_last_error().decode(), (text, rc, Lb.sh_last_error())
    # out over in, out over the taps: the views are cut from ONE parent
    img = np.full(4096, 0x5A, dtype=np.uint8)
    parent = gpu.DeviceBuffer.from_array(img)
    try:
        a, b, o = parent.view(0, len(x)), parent.view(2048, len(h)), parent.view(len(x) - 2, out_bytes)
        o2, o3 = parent.view(2048 + len(h) - 1, out_bytes), parent.view(len(x), out_bytes)
        for dst in (o, o2, a):
            rc = Lb.sh_pcm_resample_fir(a.handle, 0, n, 2, 2, b.handle, 0, m, up, down, 4, 0.5, 0, total if dst is not a else n, dst.handle, 0)
            assert rc == gpu.SH_ERR_INVALID and "out overlaps an input" in Lb.sh_last_error().decode()
        assert Lb.sh_pcm_resample_fir(a.handle, 0, n, 2, 2, b.handle, 0, m, up, down, 4, 0.5, 5, 0, a.handle, 0) == 0       # an empty window writes nothing
        gpu.sync()
        assert parent.download(np.uint8, img.size).tobytes() == img.tobytes()
        assert Lb.sh_pcm_resample_fir(a.handle, 0, n, 2, 2, b.handle, 0, m, up, down, 4, 0.5, 0, total, o3.handle, 0) == 0   # side by side is no overlap
        gpu.sync()
        got = parent.download(np.uint8, img.size)
        assert got[:len(x)].tobytes() == img[:len(x)].tobytes() and (got[len(x) + out_bytes:] == 0x5A).all()
    finally:
        parent.free()
    for null in (0, 5, 14):
        args = [None if k == null else v for k, v in enumerate([C.c_void_p(1), 0, n, 2, 2, C.c_void_p(1), 0, m, up, down, 4, 0.5, 0, 1, C.c_void_p(1), 0])]
        assert Lb.sh_pcm_resample_fir(*args) == gpu.SH_ERR_INVALID and "NULL buffer" in Lb.sh_last_error().decode()


@pytest.mark.parametrize("rate_in,rate_out,width,nch", [(44100, 48000, 2, 2), (48000, 44100, 2, 1), (44100, 96000, 1, 2), (48000, 8000, 2, 2), (44100, 8000, 1, 1)])
def test_a_samples_resample_fir_in_place_with_the_default_taps(gpu, rate_in, rate_out, width, nch):
    rng = np.random.default_rng(rate_in + rate_out + width)
    g = int(np.gcd(rate_in, rate_out))
    up, down = rate_out // g, rate_in // g
    x = firref.rand_frames(rng, width, 5000, nch)
    h = resampleref.lowpass_taps(up, down).astype(np.int64)
    want = resampleref.resample(x, h, up, down, (len(h) - 1) // 2, 2.0 ** -14, width)
    s = sample_of(x, width, rate_in)
    assert s.resample_fir(rate_out) is s and s.samplerate == rate_out and len(s) == -(-5000 * up // down)
    assert np.array_equal(frames_of(s), want)
    before = bytes(s.view_frame_data())
    assert s.resample_fir(rate_out) is s and bytes(s.view_frame_data()) == before                # the same rate: untouched
    locked = sample_of(x, width, rate_in).lock()
    out = mixer.resample_fir(locked, rate_out)
    assert np.array_equal(frames_of(out), want) and np.array_equal(frames_of(locked), x)
