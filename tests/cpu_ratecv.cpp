// Host build of synthesizer_amd/csrc/ratecv.hpp for tests/test_ratecv_plan.py (g++, no GPU): positions and steps, floor_by_outr, the
// frame counts and the route plan.
#include "../synthesizer_amd/csrc/ratecv.hpp"

extern "C" {
// output frame m: its (j, d), and its position (q, r) after k steps
void rc_walk(uint64_t inrate, uint64_t outrate, uint64_t m, long k, uint64_t* out) {
    const shr::Rates R = shr::reduce(inrate, outrate);
    shr::Pos p = shr::position(m, R.inr, R.outr, 1.0 / (double)R.outr);
    uint64_t j;
    uint32_t d;
    shr::index(p, R.outr, j, d);
    for (long s = 0; s < k; ++s) shr::step<uint64_t>(p.q, p.r, R.inr / R.outr, R.inr % R.outr, R.outr);
    out[0] = j;
    out[1] = d;
    out[2] = p.q;
    out[3] = p.r;
}
void rc_floor_by_outr(const uint32_t* u, long n, uint32_t outr, uint32_t* out) {
    for (long i = 0; i < n; ++i) out[i] = shr::floor_by_outr(u[i], 1.0 / (double)outr);
}
uint64_t rc_out_frames(uint64_t in_frames, uint64_t inrate, uint64_t outrate) { return shr::out_frames(in_frames, shr::reduce(inrate, outrate)); }
void rc_reads(uint64_t m0, uint64_t n, uint64_t inrate, uint64_t outrate, uint64_t* out) {
    const shr::Span s = shr::reads(m0, n, shr::reduce(inrate, outrate));
    out[0] = s.lo;
    out[1] = s.hi;
}
// one launch's plan as 19 numbers: route, vec, fr, groups, mode, nv, grid, lds_bytes, span_vecs, m_base, m_end, n_out, c0, c1, L, kinr,
// per_wg, head_end, tail_begin
void rc_plan(int width, int is_float, int nch, uint64_t inrate, uint64_t outrate, int aligned, int no_period, uint64_t m_base, uint64_t m_end,
             uint64_t in_lo, uint64_t in_frames, uint64_t* out) {
    const shr::Plan p = shr::plan(width, is_float, (uint32_t)nch, shr::reduce(inrate, outrate), aligned, no_period, 0, m_base, m_end, in_lo, in_frames);
    const uint64_t v[19] = {(uint64_t)p.route, (uint64_t)p.vec, (uint64_t)p.fr, (uint64_t)p.groups, (uint64_t)p.mode, (uint64_t)p.nv, p.grid,
                            p.lds_bytes, p.span_vecs, p.m_base, p.m_end, p.n_out, p.P.c0, p.P.c1, p.P.L, p.P.kinr, p.P.per_wg, p.head_end,
                            p.tail_begin};
    for (int i = 0; i < 19; ++i) out[i] = v[i];
}
}
