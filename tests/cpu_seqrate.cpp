// Host build of synthesizer_amd/csrc/ratecv.hpp for tests/test_seqrate.py (g++ -ffp-contract=off, no GPU): a buffer resampled the way a lane
// of sequence.hip's resampled events forms its samples -- shr::position for the first frame of a run of `run` output frames, shr::step
// between them, shr::index, prev = frame j - 1 (zero when j == 0 or d == 0), cur = frame j, then shr::small_int or shr::shifted_int.
#include "../synthesizer_amd/csrc/ratecv.hpp"
#include <string.h>

namespace {

int get(const unsigned char* p, int width, uint64_t i) {
    if (width == 1) return (int)(signed char)p[i];
    if (width == 2) { int16_t v; memcpy(&v, p + 2 * i, 2); return v; }
    if (width == 3) return (int)p[3 * i] | ((int)p[3 * i + 1] << 8) | ((int)(signed char)p[3 * i + 2] << 16);
    int32_t v;
    memcpy(&v, p + 4 * i, 4);
    return v;
}

void put(unsigned char* p, int width, uint64_t i, int x) {
    for (int b = 0; b < width; ++b) p[(uint64_t)width * i + b] = (unsigned char)(((unsigned)x >> (8 * b)) & 0xFF);
}

}  // namespace

extern "C" {

uint64_t sr_out_frames(uint64_t in_frames, uint64_t inrate, uint64_t outrate) { return shr::out_frames(in_frames, shr::reduce(inrate, outrate)); }

// 1 when sequence.hip takes shr::small_int for this width and these rates
int sr_small(int width, uint64_t inrate, uint64_t outrate) { return width <= 2 && shr::reduce(inrate, outrate).outr < 65536u; }

// out[0 .. out_frames * nch) = ratecv(in); use_small: shr::small_int (allowed where sr_small says so), else shr::shifted_int
void sr_resample(const unsigned char* in, int width, int nch, uint64_t inrate, uint64_t outrate, unsigned char* out, uint64_t out_frames, int run,
                 int use_small) {
    const shr::Rates R = shr::reduce(inrate, outrate);
    const double inv_outr = 1.0 / (double)R.outr;
    for (uint64_t m0 = 0; m0 < out_frames; m0 += (uint64_t)run) {
        shr::Pos p = shr::position(m0, R.inr, R.outr, inv_outr);
        for (uint64_t m = m0; m < m0 + (uint64_t)run && m < out_frames; ++m) {
            uint64_t j;
            uint32_t d;
            shr::index(p, R.outr, j, d);
            for (int c = 0; c < nch; ++c) {
                const int cur = get(in, width, j * nch + c);
                const int prev = (j && d) ? get(in, width, (j - 1) * nch + c) : 0;
                int x;
                if (use_small && width == 1) x = shr::small_int<signed char>((signed char)prev, (signed char)cur, d, R.outr, inv_outr);
                else if (use_small) x = shr::small_int<short>((short)prev, (short)cur, d, R.outr, inv_outr);
                else x = shr::shifted_int(prev, cur, d, R.outr, inv_outr, 32 - 8 * width);
                put(out, width, m * nch + c, x);
            }
            shr::step<uint64_t>(p.q, p.r, R.inr / R.outr, R.inr % R.outr, R.outr);
        }
    }
}

}
