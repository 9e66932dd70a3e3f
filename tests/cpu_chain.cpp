// Host build of synthesizer_amd/csrc/chain.hpp for tests/test_chain_maps.py (g++, no GPU): the scalar map algebra over arrays of
// stored maps (int32 add, uint32 lo | hi << 16) and of int16 rows.
#include "../synthesizer_amd/csrc/chain.hpp"

static shc::Map at(const int32_t* add, const uint32_t* b, long i, bool stored) {
    return stored ? shc::unpack<shc::STORED>(add[i], b[i]) : shc::unpack<shc::RANGE>(add[i], b[i]);
}
static void put(shc::Map m, int32_t* add, uint32_t* b, long i) { add[i] = shc::packed_add(m); b[i] = shc::packed_bounds(m); }

extern "C" {
// stored-map rule: f then g, per value (chainmaps.compose)
void ch_compose_stored(const int32_t* fa, const uint32_t* fb, const int32_t* ga, const uint32_t* gb, long n, int32_t* oa, uint32_t* ob) {
    for (long i = 0; i < n; ++i) put(shc::compose<shc::STORED>(at(fa, fb, i, true), at(ga, gb, i, true)), oa, ob, i);
}
// stored maps applied to x (chainmaps.apply of one plane)
void ch_apply_stored(const int32_t* a, const uint32_t* b, const int16_t* x, long n, int16_t* out) {
    for (long i = 0; i < n; ++i) out[i] = (int16_t)shc::apply(at(a, b, i, true), x[i]);
}
// range rule: nv int16 rows of n values (row-major), each voice's map x -> clamp(x + s, -32768, 32767) composed in order from the
// identity, stored once at the end
void ch_range_rows(const int16_t* rows, long nv, long n, int32_t* oa, uint32_t* ob) {
    for (long i = 0; i < n; ++i) {
        shc::Map m = shc::identity();
        for (long v = 0; v < nv; ++v) m = shc::compose<shc::RANGE>(m, shc::Map{rows[v * n + i], -32768, 32767});
        put(m, oa, ob, i);
    }
}
}
