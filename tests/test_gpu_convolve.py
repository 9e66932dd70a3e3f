"""sh_pcm_convolve / ``mixer.convolve`` / ``mixer.convolve_into`` / ``Sample.convolve`` on the GPU, held to byte equality throughout.
Expected bytes never come from the code under test: the reference is ``numpy.convolve`` of each channel's samples as int64 and
audioop's fbound written out (tests/firref.py), the live ``audioop`` for the three ties, and a closed form for the bound.

The shapes are sized from the kernel's own division, T = N.PCM_FIR_TILE_FRAMES output frames per workgroup and K =
N.PCM_FIR_TAP_CHUNK taps per staged span: inputs of {1, 2, T - 1, T, T + 1, 2 T + 3} frames under responses of {1, 2, 3, K - 1, K,
K + 1, 2 K + 5} taps (so m > n and m much smaller than n meet in one run), the three channel layouts, both widths; windows that begin
and end inside a tile, in the tail, of one frame, and the whole result assembled from windows of 1000 frames; every operand as a
DeviceBuffer.view at residues 0, 2 and 15 mod 16 inside sentinel-filled parents; 2^22 taps at both rails; every refusal of the C
entry point with the destination left untouched."""
import audioop
import ctypes as C

import numpy as np
import pytest

from synthesizer_amd import mixer
from synthesizer_amd.sample import Sample
from tests import firref
from tests.helpers import pcm_view_call

pytestmark = pytest.mark.gpu
RATE = 48000
LAYOUTS = [(1, 1), (2, 1), (2, 2)]                              # (channels, channels of the response)


def sample_of(values, width):
    return Sample.from_raw_frames(firref.pcm(values, width), width, RATE, values.shape[1])


def frames_of(sample):
    """a Sample's bytes as int64 (frames, nch)"""
    raw = bytes(sample.view_frame_data())
    return np.frombuffer(raw, dtype=firref.DTYPES[sample.samplewidth]).astype(np.int64).reshape(-1, sample.nchannels)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("nch,hch", LAYOUTS)
def test_every_length_against_numpy_convolve(gpu, width, nch, hch):
    T, K = gpu.PCM_FIR_TILE_FRAMES, gpu.PCM_FIR_TAP_CHUNK
    rng = np.random.default_rng(1000 * width + 10 * nch + hch)
    factors = (1.0 / (1 << (8 * width - 1)), 1.0 / (1 << (8 * width + 3)), 1.0)
    irs = {m: firref.rand_frames(rng, width, m, hch) for m in (1, 2, 3, K - 1, K, K + 1, 2 * K + 5)}
    k = 0
    for n in (1, 2, T - 1, T, T + 1, 2 * T + 3):
        x = firref.rand_frames(rng, width, n, nch)
        xs = sample_of(x, width).to_device().lock()
        for m, h in irs.items():
            factor = factors[k % 3]
            k += 1
            got = mixer.convolve(xs, sample_of(h, width), factor)
            assert len(got) == n + m - 1 and (got.nchannels, got.samplewidth, got.samplerate) == (nch, width, RATE)
            assert np.array_equal(frames_of(got), firref.convolve(x, h, factor, width)), (n, m, factor)
    assert np.array_equal(frames_of(xs), x)                     # the input is read only


@pytest.mark.parametrize("width", [1, 2])
def test_a_long_sample_under_a_long_response_and_the_default_factor(gpu, width):
    """the largest case: 20 000 frames by 3 000 taps, stereo under a stereo response, in place, with and without the tail"""
    rng = np.random.default_rng(77 + width)
    x, h = firref.rand_frames(rng, width, 20000, 2), firref.rand_frames(rng, width, 3000, 2)
    want = firref.convolve(x, h, 1.0 / (1 << (8 * width - 1)), width)
    s = sample_of(x, width)
    assert s.convolve(sample_of(h, width)) is s and np.array_equal(frames_of(s), want)
    lo, hi = firref.lo_hi(width)
    assert want.min() == lo and want.max() == hi                # (a full-scale response over full-scale noise: both rails are hit)
    s = sample_of(x, width)
    s.convolve(sample_of(h, width), tail=False)
    assert len(s) == 20000 and np.array_equal(frames_of(s), want[:20000])
    quiet = sample_of(x, width).convolve(sample_of(h, width), 1.0 / (1 << (8 * width + 6)))
    want = firref.convolve(x, h, 1.0 / (1 << (8 * width + 6)), width)
    assert np.array_equal(frames_of(quiet), want) and lo < want.min() and want.max() < hi       # and none where nothing clips


@pytest.mark.parametrize("width", [1, 2])
def test_the_three_ties_to_audioop(gpu, width):
    """one tap is audioop.mul; a 1 at tap k is k frames of silence in front (add_silence at the start); two taps of 1 are audioop.add
    of the sample and its delayed copy: one clamp of a two-term sum"""
    rng = np.random.default_rng(30 + width)
    T = gpu.PCM_FIR_TILE_FRAMES
    for nch in (1, 2):
        x = firref.rand_frames(rng, width, T + 77, nch)
        raw = firref.pcm(x, width)
        one = np.array([[1]], dtype=np.int64)
        for f in (1.0, 0.5, -0.75, 1.9, -2.0, 1.0 / 3.0):
            got = mixer.convolve(sample_of(x, width), sample_of(one, width), f)
            assert bytes(got.view_frame_data()) == audioop.mul(raw, width, f), (nch, f)
        for k in (1, 9, 2050):
            h = np.zeros((k + 1, 1), dtype=np.int64)
            h[k] = 1
            got = mixer.convolve(sample_of(x, width), sample_of(h, width), 1.0)
            silent = sample_of(x, width).add_silence((k + 0.5) / RATE, at_start=True)      # (int(RATE * seconds) == k for certain)
            assert len(silent) == len(x) + k and bytes(got.view_frame_data()) == bytes(k * nch * width) + raw == bytes(silent.view_frame_data())
            h[0] = 1
            got = mixer.convolve(sample_of(x, width), sample_of(h, width), 1.0)
            assert bytes(got.view_frame_data()) == audioop.add(raw + bytes(k * nch * width), bytes(k * nch * width) + raw, width), (nch, k)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("nch,hch", LAYOUTS)
def test_a_window_is_that_slice_of_the_whole_result(gpu, width, nch, hch):
    T, K = gpu.PCM_FIR_TILE_FRAMES, gpu.PCM_FIR_TAP_CHUNK
    rng = np.random.default_rng(50 + 10 * width + nch + hch)
    n, m = 2 * T + 300, K + 77
    x, h = firref.rand_frames(rng, width, n, nch), firref.rand_frames(rng, width, m, hch)
    factor = 1.0 / (1 << (8 * width + 2))
    whole = firref.convolve(x, h, factor, width)
    xs, hs = sample_of(x, width).to_device(), sample_of(h, width).to_device()
    assert np.array_equal(frames_of(mixer.convolve(xs, hs, factor)), whole)
    total = n + m - 1
    pairs = [(0, 1), (0, T), (0, T + 1), (5, 100), (5, T), (T - 1, 2), (T + 17, T + 500),(n - 3, 10), (n, m - 1), (n + 5, 1), (total - 1, 1), (3, total - 3)]
    for first, count in pairs:
        got = mixer.convolve(xs, hs, factor, start_frame=first, nframes=count)
        assert len(got) == count and np.array_equal(frames_of(got), whole[first:first + count]), (first, count)
    assert len(mixer.convolve(xs, hs, factor, start_frame=total)) == 0 and len(mixer.convolve(xs, hs, factor, 7, 0)) == 0
    # the whole result assembled from windows of 1000 frames, each written into its place of one buffer
    fb = nch * width
    buf = gpu.DeviceBuffer(total * fb)
    for first in range(0, total, 1000):
        assert mixer.convolve_into(buf, first * fb, xs, hs, factor, first, min(1000, total - first)) == min(1000, total - first)
    assert buf.download_bytes(total * fb) == firref.pcm(whole, width)


@pytest.mark.parametrize("width", [1, 2])
def test_every_operand_as_a_view_at_residues_0_2_and_15(gpu, width):
    """in, ir and out each as a DeviceBuffer.view at residues 0, 2 and 15 mod 16 inside sentinel-filled parents: pcm_view_call asserts
    that no byte outside the destination changed and that the inputs are untouched"""
    L = gpu.lib()
    T = gpu.PCM_FIR_TILE_FRAMES
    rng = np.random.default_rng(90 + width)
    residues = (0, 2, 15)
    for nch, hch in LAYOUTS:
        n, m = T + 9, 37
        x, h = firref.rand_frames(rng, width, n, nch), firref.rand_frames(rng, width, m, hch)
        factor = 1.0 / (1 << (8 * width + 1))
        whole = firref.convolve(x, h, factor, width)
        first, count = 3, n + m - 1 - 5
        want = firref.pcm(whole[first:first + count], width)
        cases = [(a, 0, 0) for a in residues] + [(0, a, 0) for a in residues[1:]] + [(0, 0, a) for a in residues[1:]] + [(2, 15, 15), (15, 2, 2), (15, 15, 15)]
        for a_in, a_ir, a_out in cases:
            rc, got = pcm_view_call(gpu, [(firref.pcm(x, width), a_in), (firref.pcm(h, width), a_ir)], len(want), a_out,
                                    lambda iv, ov: L.sh_pcm_convolve(iv[0].handle, 0, n, nch, width, iv[1].handle, 0, m, hch, factor, first, count, ov.handle, 0))
            assert rc == 0 and got == want, (nch, hch, a_in, a_ir, a_out, rc)


def closed_form(sign_h, first, count, taps, width=2):
    """x all -32768 under `taps` taps all sign_h: acc = min(i + 1, taps) * (-32768 * sign_h), p = acc * 2^-37 (both exact), fbound"""
    i = np.arange(first, first + count, dtype=np.int64)
    acc = np.minimum(i + 1, taps) * (-32768 * sign_h)
    assert int(np.abs(acc).max()) <= 2 ** 52
    return firref.fbound(acc.astype(np.float64) * 2.0 ** -37, width)


def test_the_bound_two_to_the_22_taps_at_the_rails(gpu):
    """x of 2^22 + 63 frames, all -32768, under 2^22 taps, all -32768: the sum reaches 2^52, the largest the contract admits, and
    frame 2^22 - 1 reads HI only if no partial sum on the way was rounded; the same under taps of 32767 for the negative side.  The
    expected samples come from the closed form, not from numpy."""
    taps = 2 ** 22
    n = taps + 63
    x = Sample.from_raw_frames(np.full(n, -32768, dtype=np.int16).tobytes(), 2, RATE, 1).to_device()
    first = taps - 32
    for sign_h in (-32768, 32767):
        h = Sample.from_raw_frames(np.full(taps, sign_h, dtype=np.int16).tobytes(), 2, RATE, 1).to_device()
        want = closed_form(sign_h, first, 64, taps)
        got = frames_of(mixer.convolve(x, h, 2.0 ** -37, start_frame=first, nframes=64))[:, 0]
        assert np.array_equal(got, want), (sign_h, got.tolist(), want.tolist())
        if sign_h < 0:
            assert int(np.minimum(first + 31 + 1, taps)) * 2 ** 30 == 2 ** 52 and got[31] == 32767      # acc = 2^52 at frame first + 31
            # and a window that crosses the upper rail: p = (i + 1) / 128 passes 32767 at i + 1 = 2^22 - 128
            early = taps - 128 - 32
            want = closed_form(sign_h, early, 64, taps)
            assert want[0] < 32767 and want[-1] == 32767 and len(set(want.tolist())) > 1
            assert np.array_equal(frames_of(mixer.convolve(x, h, 2.0 ** -37, start_frame=early, nframes=64))[:, 0], want)
        else:
            assert want.min() == -32767 and got[31] == -32767    # p = -32768 (1 - 2^-15) = -32767.0 exactly: not below LO + 1, so its floor
            # the lower rail itself: twice the factor puts p below LO + 1.0
            want = firref.fbound(np.minimum(np.arange(first, first + 64, dtype=np.int64) + 1, taps).astype(np.float64) * (-32768.0 * 32767.0) * 2.0 ** -36, 2)
            assert (want == -32768).all()
            assert np.array_equal(frames_of(mixer.convolve(x, h, 2.0 ** -36, start_frame=first, nframes=64))[:, 0], want)


def test_every_refusal_of_the_entry_point_leaves_the_destination_alone(gpu):
    L = gpu.lib()
    rng = np.random.default_rng(3)
    n, m = 100, 10
    x, h = firref.pcm(firref.rand_frames(rng, 2, n, 2), 2), firref.pcm(firref.rand_frames(rng, 2, m, 2), 2)
    out_bytes = (n + m - 1) * 4

    def call(width=2, nch=2, ir_nch=1, in_frames=n, ir_frames=m, factor=0.5, first=0, count=n + m - 1, in_off=0, ir_off=0, out_off=0):
        return lambda iv, ov: L.sh_pcm_convolve(iv[0].handle, in_off, in_frames, nch, width, iv[1].handle, ir_off, ir_frames, ir_nch, factor, first, count,
                                                ov.handle, out_off)
    refusals = [
        (call(width=3), "widths 3 and 4 are not built"), (call(width=4), "widths 3 and 4 are not built"),
        (call(nch=3), "3 channels"), (call(nch=0), "0 channels"),
        (call(nch=1, ir_nch=2), "a response of 2 channels over 1"), (call(ir_nch=3), "a response of 3 channels over 2"),
        (call(ir_frames=0), "an empty response"),
        (call(ir_frames=2 ** 22 + 1), "taps are more than 4194304"),
        (call(factor=float("inf")), "not finite"), (call(factor=float("nan")), "not finite"),
        (call(count=n + m), "reach past the result's 109"), (call(first=1), "reach past the result's 109"), (call(first=110, count=0), "reach past the result's 109"),
        (call(in_frames=n + 1, count=1), "input range outside buffer"), (call(in_off=4), "input range outside buffer"),
        (call(ir_nch=2, ir_frames=m + 1, count=1), "response range outside buffer"), (call(ir_off=2, ir_nch=2), "response range outside buffer"),
        (call(out_off=4), "output range outside buffer"), (call(out_off=out_bytes + 1, count=0), "output range outside buffer"),
    ]
    for how, text in refusals:
        rc, _ = pcm_view_call(gpu, [(x, 0), (h, 0)], out_bytes, 0, how, untouched=True)
        assert rc == gpu.SH_ERR_INVALID and text in L.sh_last_error().decode() and "sh_pcm_convolve: " in L.sh_last_error().decode(), (text, rc, L.sh_last_error())
    # out over in, out over ir: the views are cut from ONE parent
    img = np.full(4096, 0x5A, dtype=np.uint8)
    parent = gpu.DeviceBuffer.from_array(img)
    try:
        a, b, o = parent.view(0, len(x)), parent.view(1024, len(h)), parent.view(len(x) - 2, out_bytes)
        o2, o3 = parent.view(1024 + len(h) - 1, out_bytes), parent.view(len(x), out_bytes)
        for dst in (o, o2, a):
            rc = L.sh_pcm_convolve(a.handle, 0, n, 2, 2, b.handle, 0, m, 2, 0.5, 0, n + m - 1 if dst is not a else n, dst.handle, 0)
            assert rc == gpu.SH_ERR_INVALID and "out overlaps an input" in L.sh_last_error().decode()
        assert L.sh_pcm_convolve(a.handle, 0, n, 2, 2, b.handle, 0, m, 2, 0.5, 5, 0, a.handle, 0) == 0          # an empty window writes nothing
        gpu.sync()
        assert parent.download(np.uint8, img.size).tobytes() == img.tobytes()
        assert L.sh_pcm_convolve(a.handle, 0, n, 2, 2, b.handle, 0, m, 2, 0.5, 0, n + m - 1, o3.handle, 0) == 0 # side by side is no overlap
        gpu.sync()
        got = parent.download(np.uint8, img.size)
        assert got[:len(x)].tobytes() == img[:len(x)].tobytes() and (got[len(x) + out_bytes:] == 0x5A).all()
    finally:
        parent.free()
    for null in (0, 5, 12):
        args = [None if k == null else v for k, v in enumerate([C.c_void_p(1), 0, n, 2, 2, C.c_void_p(1), 0, m, 1, 0.5, 0, 1, C.c_void_p(1), 0])]
        assert L.sh_pcm_convolve(*args) == gpu.SH_ERR_INVALID and "NULL buffer" in L.sh_last_error().decode()
