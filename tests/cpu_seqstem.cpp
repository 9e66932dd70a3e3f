// csrc/seqstem.hpp built for the host behind a few C functions (tests/test_seqstem.py drives them through ctypes): the row order of the
// planes, the 64-bit address of a plane's sample, the refusals of a call's geometry, the all-planes-aligned predicate, the span of all
// planes and the stride that keeps the store's fast path.  With SEQSTEM_MAIN it is a program of its own (its own main: generated
// geometries against restatements in place, in 128-bit integers where a product could pass 2^64), which a sanitizer build can run as it
// stands.
#include "../synthesizer_amd/csrc/seqstem.hpp"

extern "C" {

uint32_t st_nrows(uint32_t ntracks, uint32_t ngroups) { return shst::nrows(ntracks, ngroups); }
uint32_t st_track_row(uint32_t t) { return shst::track_row(t); }
uint32_t st_master_row(uint32_t ntracks) { return shst::master_row(ntracks); }
uint32_t st_group_row(uint32_t ntracks, uint32_t g) { return shst::group_row(ntracks, g); }
uint32_t st_max_rows() { return shst::MAX_ROWS; }
uint64_t st_stride_bytes(uint64_t plane_samples, uint32_t width) { return shst::stride_bytes(plane_samples, width); }
uint64_t st_plane_offset(uint32_t r, uint64_t stride) { return shst::plane_offset(r, stride); }
uint64_t st_address(uint64_t biased, uint32_t r, uint64_t stride, uint64_t s, uint32_t width) { return shst::address(biased, r, stride, s, width); }
int st_check(uint32_t nplanes, uint32_t ntracks, uint32_t ngroups, uint64_t plane_samples, uint64_t nsamples, uint64_t out_sample, uint64_t have) {
    return (int)shst::check(nplanes, ntracks, ngroups, plane_samples, nsamples, out_sample, have);
}
uint64_t st_span(uint32_t nplanes, uint64_t plane_samples, uint64_t nsamples) { return shst::span(nplanes, plane_samples, nsamples); }
int st_overlaps(uint64_t a0, uint64_t a1, uint64_t b0, uint64_t b1) { return shst::overlaps(a0, a1, b0, b1); }
int st_aligned(uint64_t biased, uint64_t stride) { return shst::aligned(biased, stride); }
uint64_t st_plane_samples_for(uint64_t nsamples, uint32_t width) { return shst::plane_samples_for(nsamples, width); }

}  // extern "C"

#ifdef SEQSTEM_MAIN
#include <cstdio>
int main() {
    uint64_t state = 88172645463325252ull;
    auto rnd = [&](uint64_t m) { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return state % m; };
    typedef unsigned __int128 u128;
    unsigned calls = 0;
    for (int k = 0; k < 200000; ++k) {
        const uint32_t ntracks = 1 + (uint32_t)rnd(32), ngroups = (uint32_t)rnd(9), width = 1 + (uint32_t)rnd(4);
        const uint32_t nplanes = rnd(8) ? ntracks + 1 + ngroups : (uint32_t)rnd(50);
        // sizes up to the longest song and far past it, and small ones, so that every refusal and the boundary between them is met
        const uint64_t big = rnd(2) ? (1ull << (1 + rnd(62))) : 1 + rnd(5000);
        const uint64_t nsamples = rnd(big + 1), plane_samples = rnd(3) ? nsamples + rnd(40) : rnd(big + 1);
        const uint64_t out_sample = rnd(4) ? rnd(100) : rnd(big + 1);
        const u128 need = (u128)out_sample + (u128)(nplanes ? nplanes - 1 : 0) * plane_samples + nsamples;
        const uint64_t have = rnd(3) ? (uint64_t)(need > ~0ull ? ~0ull : (uint64_t)need) + rnd(3) - (need && rnd(2) ? 1 : 0) : rnd(big + 1);
        shst::Refusal want = shst::OK;
        if (nplanes != ntracks + 1 + ngroups) want = shst::PLANES;
        else if (plane_samples < nsamples) want = shst::STRIDE;
        else if (need > (u128)have) want = shst::EXTENT;
        const shst::Refusal got = shst::check(nplanes, ntracks, ngroups, plane_samples, nsamples, out_sample, have);
        if (got != want) { printf("check %d: got %d, want %d\n", k, (int)got, (int)want); return 1; }
        if (got == shst::OK && nsamples) {
            // a checked call: the span is the distance from plane 0's first sample to the last plane's last, and every plane's window
            // lies inside the buffer, in rows' order, without touching its neighbour's
            if ((u128)shst::span(nplanes, plane_samples, nsamples) != need - out_sample) { printf("span %d\n", k); return 1; }
            const uint64_t stride = shst::stride_bytes(plane_samples, width), base = 4096 + rnd(1ull << 40);
            for (uint32_t r = 0; r < nplanes; ++r) {
                const u128 first = (u128)base + (u128)r * stride, last = first + (u128)nsamples * width;
                if ((u128)have * width < (u128)~0ull - base && (uint64_t)first != shst::address(base, r, stride, 0, width)) { printf("address %d\n", k); return 1; }
                if (r && first < (u128)base + (u128)(r - 1) * stride + (u128)nsamples * width) { printf("planes %d overlap\n", k); return 1; }
                if (last > (u128)base + (u128)(have - out_sample) * width) { printf("plane %u of %d past the buffer\n", r, k); return 1; }
            }
            // aligned: every plane's first lane-aligned address is a multiple of 16 exactly where the predicate says so
            bool all = true;
            for (uint32_t r = 0; r < nplanes; ++r) all = all && (shst::address(base, r, stride, 0, width) % 16 == 0);
            if (shst::aligned(base, stride) && !all) { printf("aligned %d\n", k); return 1; }
            if (!shst::aligned(base, stride) && all && nplanes > 1) { printf("not aligned %d, yet every plane is\n", k); return 1; }
        }
        const uint64_t n = rnd(1ull << 33), p = shst::plane_samples_for(n, width);
        if (p < n || p - n >= 16 || (p * width) % 16) { printf("plane_samples_for %d\n", k); return 1; }
        ++calls;
    }
    // the address wraps as the biased base wraps: a window far into the song, stored at the buffer's start
    const uint64_t buffer = 0x7f0000001000ull, first_sample = 3000000000ull;
    for (uint32_t width = 1; width <= 4; ++width) {
        const uint64_t biased = buffer - first_sample * width, stride = shst::stride_bytes(1ull << 31, width);
        for (uint32_t r = 0; r < 41; ++r)
            if (shst::address(biased, r, stride, first_sample + 5, width) != buffer + (uint64_t)r * stride + 5 * width) { printf("biased\n"); return 1; }
    }
    printf("seqstem: %u geometries: ok\n", calls);
    return 0;
}
#endif
