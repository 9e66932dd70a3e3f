// Host build of synthesizer_amd/csrc/seqenv.hpp for tests/test_seqenv.py (g++ -ffp-contract=off, no GPU): a buffer shaped the way the
// envelope kernels of sequence.hip shape an event -- the event placed at track sample dst, the track cut into tiles of `tile` samples,
// every lane taking `lane` consecutive samples (zeros where they lie outside the event), she::shape_lane with what the lane's tile takes
// of the event.
#include "../synthesizer_amd/csrc/seqenv.hpp"
#include <string.h>

namespace {

int get(const unsigned char* p, int width, uint64_t i) {
    if (width == 1) return (int)(signed char)p[i];
    if (width == 2) { int16_t v; memcpy(&v, p + 2 * i, 2); return v; }
    int32_t v;
    memcpy(&v, p + 4 * i, 4);
    return v;
}

void put(unsigned char* p, int width, uint64_t i, int x) {
    for (int b = 0; b < width; ++b) p[(uint64_t)width * i + b] = (unsigned char)(((unsigned)x >> (8 * b)) & 0xFF);
}

template <int N>
void run(const unsigned char* in, int width, uint32_t n, const she::Seg* segs, uint32_t nseg, uint32_t dst, uint32_t tile, unsigned char* out) {
    const double hi = width == 1 ? 127.0 : (width == 2 ? 32767.0 : 2147483647.0), lo = -hi - 1.0;
    for (uint32_t t0 = dst / tile * tile; t0 < dst + n; t0 += tile) {
        const uint32_t tlo = t0 > dst ? t0 - dst : 0u, thi = (t0 + tile < dst + n ? t0 + tile : dst + n) - dst;
        for (uint32_t s0 = t0; s0 < t0 + tile; s0 += N) {
            const long long p0 = (long long)s0 - (long long)dst;
            int x[N];
            for (int k = 0; k < N; ++k) x[k] = (p0 + k >= 0 && p0 + k < (long long)n) ? get(in, width, (uint64_t)(p0 + k)) : 0;
            she::shape_lane<N>(segs, nseg, tlo, thi, p0, x, lo, hi);
            for (int k = 0; k < N; ++k) {
                if (p0 + k >= 0 && p0 + k < (long long)n) put(out, width, (uint64_t)(p0 + k), x[k]);
                else if (x[k] != 0) out[(uint64_t)width * n] = 1;                // a zero outside the event must stay zero
            }
        }
    }
}

}  // namespace

extern "C" {

unsigned se_seg_bytes() { return (unsigned)sizeof(she::Seg); }
unsigned se_max_segments() { return she::MAX_SEGMENTS; }

// out[0 .. n) = the n samples of `in` shaped by segs; out[n * width] (one byte more) is set when a sample outside the event left zero.
// lane: 2, 4 or 8 (the kernels' shape_lane<N>); tile: a multiple of lane.  Returns 0, or -1 for a shape it does not have.
int se_shape(const unsigned char* in, int width, uint32_t n, const void* segs, uint32_t nseg, uint32_t dst, uint32_t tile, int lane, unsigned char* out) {
    const she::Seg* g = (const she::Seg*)segs;
    if (tile % (uint32_t)lane) return -1;
    if (lane == 8) run<8>(in, width, n, g, nseg, dst, tile, out);
    else if (lane == 4) run<4>(in, width, n, g, nseg, dst, tile, out);
    else if (lane == 2) run<2>(in, width, n, g, nseg, dst, tile, out);
    else return -1;
    return 0;
}

}
