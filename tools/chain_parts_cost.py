#!/usr/bin/env python
"""What the chain maps cost (GPU box, repo root): per 48 000-frame block of the 1024-voice additive table on its plateau (the fused
fold), ``mixdown_i16_device`` against ``mixdown_i16_parts_device`` + the apply of its one plane, and the apply of 8 planes alone
(what root does after an 8-rank gather).  Reported, not gated.

    python tools/chain_parts_cost.py
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def steady(N, call, min_seconds=0.2, reps=10):
    call()
    N.sync()
    loops, total = [], 0.0
    while total < min_seconds or len(loops) < 5:
        N.timer_start()
        for _ in range(reps):
            call()
        ms = N.timer_stop()
        loops.append(ms / reps)
        total += ms / 1e3
    return statistics.median(loops)


def main():
    from synthesizer_amd import _native as N
    from synthesizer_amd import oscillators as G
    from synthesizer_amd.mixer import VoiceBank
    from synthesizer_amd.workloads import additive_voices
    N.ensure_init(0)
    L = N.lib()
    SR, n, start = 48000, 48000, 3 * 48000
    gv, gains = additive_voices(G, 1024, SR, seed=0, partials=16, adsr={"sustain": 1.0e6})
    bank = VoiceBank(gv, gains=gains)
    out = N.DeviceBuffer(n * 2)
    parts = N.DeviceBuffer(8 * n * 8)
    plane0 = parts.view(0, n * 8)
    want = bank.mixdown_i16_device(n, start).download_bytes(n * 2)
    bank.mixdown_i16_parts_device(n, start, out=plane0)
    N.check(L.sh_chain_parts_apply(plane0.handle, 1, n, n, None, out.handle))
    assert out.download_bytes(n * 2) == want
    fused = L.sh_get_option(N.SH_INFO_LAST_MIXDOWN_FUSED)
    for k in range(1, 8):                                       # eight planes (as after an 8-rank gather)
        N.check(L.sh_buf_copy(parts.handle, k * n * 8, parts.handle, 0, n * 8))

    def whole():
        N.check(L.sh_bank_mixdown_i16_async(bank._bank.handle, start, n, 32767.0, out.handle))

    def parts_then_apply():
        N.check(L.sh_bank_mixdown_i16_parts_async(bank._bank.handle, start, n, 32767.0, plane0.handle))
        N.check(L.sh_chain_parts_apply(plane0.handle, 1, n, n, None, out.handle))

    def parts_only():
        N.check(L.sh_bank_mixdown_i16_parts_async(bank._bank.handle, start, n, 32767.0, plane0.handle))

    def apply8():
        N.check(L.sh_chain_parts_apply(parts.handle, 8, n, n, None, out.handle))

    print("1024-voice additive table, %d frames per block, fused stretches: %d" % (n, fused))
    rows = [("mixdown_i16_device", whole), ("mixdown_i16_parts_device + apply (1 plane)", parts_then_apply),
            ("mixdown_i16_parts_device alone", parts_only), ("apply of 8 planes alone", apply8)]
    base = None
    for name, fn in rows:
        us = steady(N, fn) * 1e3
        base = base or us
        print("%-44s %10.1f us per block  (%.3f x)" % (name, us, us / base))
    N.check(L.sh_overflow_check())


if __name__ == "__main__":
    main()
