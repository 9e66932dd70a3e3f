// sequence.hip -- a list of placed samples mixed into a track in one launch (sh_mix_events: Sample.mix_at_many, mixer.sequence).
//
// Per event audioop.mul (fbound: clamp, then floor) and audioop.add with saturation AT EVERY EVENT, IN LIST ORDER -- the loop of
// Sample.mix_at calls it replaces, byte for byte.  The track is cut into tiles (seqplan.hpp); one workgroup per tile that some event
// touches walks that tile's events in order, every lane keeping its own few track samples in registers from the one load of the base
// to the one store of the result.  Lanes own disjoint samples and read the track only there, so the fold is in place; a source may
// not be the track.  Built with -ffp-contract=off (the float64 product of audioop.mul stays one rounding).
#include "common.hpp"
#include "chain.hpp"
#include "pcmdev.hpp"
#include "seqplan.hpp"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

typedef int int4v __attribute__((ext_vector_type(4)));
typedef short short8u __attribute__((ext_vector_type(8), aligned(2)));      // eight samples at any sample offset
// A source pointer comes out of a record in memory, so the compiler cannot know its address space and would read through it with flat
// loads: the sources are device buffers, say so (global_load).
#define SH_SEQ_GLOBAL __attribute__((address_space(1)))
typedef const SH_SEQ_GLOBAL short* gshort_p;

// One event as the kernels read it: wave-uniform, so a record is fetched by scalar loads.
struct SeqEv {
    const void* src;          // the first sample taken from the source
    double      factor;       // audioop.mul's; exactly 1.0: none
    uint32_t    dst;          // where in the track its first sample lands (samples)
    uint32_t    n;            // samples, > 0 for every event a tile lists
    uint32_t    pad[2];
};
static_assert(sizeof(SeqEv) == 32, "SeqEv is read as one 32-byte scalar load");

// How a lane gets the eight samples of an event that start at sample `rel` of its source, when they sit at any 2-byte offset against
// the lane's aligned sixteen.  All lanes of a workgroup start on multiples of eight track samples, so that offset -- (src - 2 dst)
// mod 16 -- is the same for every lane: wave-uniform per event.
//   FUNNEL  two aligned 16-byte loads and a funnel shift by that byte count (v_alignbyte_b32); an aligned event takes one load.
//   VEC2    one load through a vector type of alignment 2: the compiler emits ONE global_load_dwordx4 at the odd address (read
//           in the ISA: no global_load_ushort), the memory pipeline splits what crosses a line.
// FUNNEL is the default and SYNTHHIP_SEQ_ALIGN=1 selects VEC2.  Measured (profiles/sequence_ab.txt; one call of Sample.mix_at_many on the
// 120-s song with 4096 / 32 768 events, 75 % of the starts misaligned): 3.36 / 30.6 ms against 3.48 / 31.5 ms -- within 4 %, and that call is
// still bound by the host's table packing, so the choice is not settled by it: FUNNEL stays because it asks nothing of how the memory
// pipeline treats a vector load that straddles a line.  Staging an event's span through LDS was not built.
// Lanes on the edges of an event (not all eight samples inside it; FUNNEL: not both aligned vectors inside the source) assemble
// their samples one by one, zeros outside: x + 0 is the identity of the saturating add and fbound(0 * factor) == 0.
enum Scheme { FUNNEL = 0, VEC2 = 1 };

__device__ __forceinline__ short8v seq_edge8(gshort_p src, long long rel, uint32_t n) {
    short8v x = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (rel + j >= 0 && rel + j < (long long)n) x[j] = src[rel + j];
    return x;
}

template <int SCHEME>
__device__ __forceinline__ short8v seq_load8(const SeqEv& c, uint32_t s0) {
    gshort_p src = (gshort_p)c.src;
    const long long rel = (long long)s0 - (long long)c.dst;
    if (rel + 8 <= 0 || rel >= (long long)c.n) return (short8v){0, 0, 0, 0, 0, 0, 0, 0};
    if constexpr (SCHEME == VEC2) {
        if (rel >= 0 && rel + 8 <= (long long)c.n) return *(const SH_SEQ_GLOBAL short8u*)(src + rel);
    } else {
        const uint32_t sh = (uint32_t)(((uintptr_t)c.src - 2 * (uintptr_t)c.dst) & 15);      // (uniform) 0, 2 .. 14
        if (sh == 0) {
            if (rel >= 0 && rel + 8 <= (long long)c.n) return *(const SH_SEQ_GLOBAL short8v*)(src + rel);
        } else if (rel >= 8 && rel + 16 <= (long long)c.n) {
            const SH_SEQ_GLOBAL int4v* q = (const SH_SEQ_GLOBAL int4v*)((uintptr_t)(src + rel) - sh);
            const int4v lo = q[0], hi = q[1];
            const uint32_t r = sh & 3;
            union { int4v v; short8v s; } o;
#define SH_FUNNEL(A_, B_, C_, D_, E_) o.v = (int4v){(int)__builtin_amdgcn_alignbyte(B_, A_, r), (int)__builtin_amdgcn_alignbyte(C_, B_, r), \
                                                    (int)__builtin_amdgcn_alignbyte(D_, C_, r), (int)__builtin_amdgcn_alignbyte(E_, D_, r)}
            switch (sh >> 2) {                              // (uniform)
            case 0: SH_FUNNEL(lo[0], lo[1], lo[2], lo[3], hi[0]); break;
            case 1: SH_FUNNEL(lo[1], lo[2], lo[3], hi[0], hi[1]); break;
            case 2: SH_FUNNEL(lo[2], lo[3], hi[0], hi[1], hi[2]); break;
            default: SH_FUNNEL(lo[3], hi[0], hi[1], hi[2], hi[3]); break;
            }
#undef SH_FUNNEL
            return o.s;
        }
    }
    return seq_edge8(src, rel, c.n);
}

__device__ __forceinline__ short8v seq_mul8(const short8v x, const double factor) {
    short8v r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (short)fbound((double)x[j] * factor, Lim<short>::lo, Lim<short>::hi);
    return r;
}

// The 16-bit kernel: workgroup k folds active tile tiles[k]; a lane owns LANE_SAMPLES_I16 = 8 consecutive track samples (one aligned
// 16-byte load of the base, one aligned 16-byte store).  INFLIGHT events' records (scalar loads, one batch ahead) and source vectors
// are in flight before their adds.  `aligned`: the track starts on a 16-byte boundary (a view that does not: sample by sample).
template <int SCHEME, int INFLIGHT>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_i16(const SeqEv* __restrict__ ev, const uint32_t* __restrict__ tiles,
                                                                      const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                                      uint32_t ntiles, short* track, uint32_t track_samples, int aligned) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t s0 = tiles[k] * shq::TILE_I16 + threadIdx.x * shq::LANE_SAMPLES_I16;
    if (s0 >= track_samples) return;
    const bool whole = aligned && s0 + 8 <= track_samples;
    short8v acc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (whole) acc = *reinterpret_cast<const short8v*>(track + s0);
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) acc[j] = track[s0 + j];
    uint32_t e = first[k];
    const uint32_t e1 = first[k + 1];
    auto fold = [&](const SeqEv& c, short8v x) {
        if (c.factor != 1.0) x = seq_mul8(x, c.factor);       // (uniform)
        acc = __builtin_elementwise_add_sat(acc, x);
    };
    if (e1 - e >= INFLIGHT) {
        SeqEv c[INFLIGHT], nx[INFLIGHT];
#pragma unroll
        for (int u = 0; u < INFLIGHT; ++u) c[u] = ev[idx[e + u]];
        for (; e + INFLIGHT <= e1; e += INFLIGHT) {
            const bool more = e + 2 * INFLIGHT <= e1;
            if (more) {
#pragma unroll
                for (int u = 0; u < INFLIGHT; ++u) nx[u] = ev[idx[e + INFLIGHT + u]];
            }
            short8v x[INFLIGHT];
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) x[u] = seq_load8<SCHEME>(c[u], s0);
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) fold(c[u], x[u]);
            if (more) {
#pragma unroll
                for (int u = 0; u < INFLIGHT; ++u) c[u] = nx[u];
            }
        }
    }
    for (; e < e1; ++e) {
        const SeqEv c = ev[idx[e]];
        fold(c, seq_load8<SCHEME>(c, s0));
    }
    if (whole) *reinterpret_cast<short8v*>(track + s0) = acc;
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) track[s0 + j] = acc[j];
}

// Widths 1, 3 and 4: the reference's loop as it stands, LANE_SAMPLES_W = 4 consecutive samples per thread, bytes assembled for 24-bit
// samples, 64-bit sums for 32-bit ones -- the shape of k_mix_chain_gather_w (pcm.hip), which says why these widths get the plain kernel.
template <int WIDTH>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_mix_events_w(const SeqEv* __restrict__ ev, const uint32_t* __restrict__ tiles,
                                                                    const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                                    uint32_t ntiles, unsigned char* track, uint32_t track_samples) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t s0 = tiles[k] * shq::TILE_W + threadIdx.x * shq::LANE_SAMPLES_W;
    if (s0 >= track_samples) return;
    constexpr long long HI = WIDTH == 1 ? 127LL : (WIDTH == 3 ? 8388607LL : 2147483647LL), LO = -HI - 1;
    long long acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) acc[j] = chain_get<WIDTH>(track, s0 + j);
    const uint32_t e1 = first[k + 1];
    for (uint32_t e = first[k]; e < e1; ++e) {
        const SeqEv c = ev[idx[e]];
        const unsigned char* src = (const unsigned char*)c.src;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long rel = (long long)s0 + j - (long long)c.dst;
            if (rel >= 0 && rel < (long long)c.n) {
                long long x = chain_get<WIDTH>(src, (size_t)rel);
                if (c.factor != 1.0) x = fbound((double)x * c.factor, (double)LO, (double)HI);
                const long long t = acc[j] + x;
                acc[j] = t > HI ? HI : (t < LO ? LO : t);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) chain_put<WIDTH>(track, s0 + j, acc[j]);
}

}  // namespace

extern "C" {

int sh_mix_events(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event* events, uint32_t nevents, int width, sh_buf* track,
                  size_t track_samples) {
    SH_REQUIRE_INIT();
    if (width < 1 || width > 4) return sh::set_error(SH_ERR_INVALID, "sh_mix_events: width %d not in {1, 2, 3, 4}", width);
    if (!track || (nevents && !events) || (nsrc && !srcs)) return sh::set_error(SH_ERR_INVALID, "sh_mix_events: NULL argument");
    const size_t w = (size_t)width;
    if (track_samples > track->bytes / w) return sh::set_error(SH_ERR_INVALID, "sh_mix_events: track range outside buffer");
    const char* t0 = (const char*)track->ptr;
    const char* t1 = t0 + track_samples * w;
    for (uint32_t v = 0; v < nsrc; ++v) {
        if (!srcs[v]) continue;
        const char* p = (const char*)srcs[v]->ptr;
        if (srcs[v] == track || (p < t1 && t0 < p + srcs[v]->bytes))
            return sh::set_error(SH_ERR_INVALID, "sh_mix_events: source %u is the track", v);
    }
    std::vector<shq::Event> pe(nevents);
    for (uint32_t e = 0; e < nevents; ++e) {
        const sh_mix_event& m = events[e];
        if (m.reserved != 0) return sh::set_error(SH_ERR_INVALID, "sh_mix_events: event %u: reserved must be 0", e);
        if (!isfinite(m.factor)) return sh::set_error(SH_ERR_INVALID, "sh_mix_events: event %u: factor is not finite", e);
        if (m.src >= nsrc || !srcs[m.src]) return sh::set_error(SH_ERR_INVALID, "sh_mix_events: event %u: no source %u", e, m.src);
        const size_t have = srcs[m.src]->bytes / w;
        if (m.src_sample > have || m.nsamples > have - m.src_sample)
            return sh::set_error(SH_ERR_INVALID, "sh_mix_events: event %u: range outside its source", e);
        pe[e] = shq::Event{m.dst_sample, m.nsamples};
    }
    const uint32_t tile = shq::tile_samples(width);
    const shq::Plan P = shq::plan(pe.data(), nevents, track_samples, tile);
    if (P.refused == shq::EVENT_BEYOND_TRACK) return sh::set_error(SH_ERR_INVALID, "sh_mix_events: event %u: range outside the track", P.bad_event);
    if (P.refused == shq::TRACK_TOO_LONG) return sh::set_error(SH_ERR_INVALID, "sh_mix_events: at most 2^32 - 65536 track samples per call");
    if (P.refused) return sh::set_error(SH_ERR_INVALID, "sh_mix_events: more than 2^28 (event, tile) overlaps in one call");
    if (P.tiles.empty()) return SH_OK;

    // one block on the library's grow-only scratch, one copy: records | tiles | first | idx
    const uint32_t nt = (uint32_t)P.tiles.size();
    const size_t b_ev = (size_t)nevents * sizeof(SeqEv), b_tiles = (size_t)nt * 4, b_first = ((size_t)nt + 1) * 4, b_idx = P.idx.size() * 4;
    std::vector<char> host(b_ev + b_tiles + b_first + b_idx);
    SeqEv* rec = reinterpret_cast<SeqEv*>(host.data());
    for (uint32_t e = 0; e < nevents; ++e) {
        const sh_mix_event& m = events[e];
        rec[e] = SeqEv{(const char*)srcs[m.src]->ptr + m.src_sample * w, m.factor, (uint32_t)m.dst_sample, (uint32_t)m.nsamples, {0, 0}};
    }
    memcpy(host.data() + b_ev, P.tiles.data(), b_tiles);
    memcpy(host.data() + b_ev + b_tiles, P.first.data(), b_first);
    memcpy(host.data() + b_ev + b_tiles + b_first, P.idx.data(), b_idx);
    int rc = sh::ensure_scratch(host.size());
    if (rc) return rc;
    hipStream_t st = sh::state().stream;
    char* dev = (char*)sh::state().scratch;
    // (pageable source: staged before the call returns, ordered after earlier kernels)
    SH_HIP(hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, st));
    const SeqEv* d_ev = (const SeqEv*)dev;
    const uint32_t* d_tiles = (const uint32_t*)(dev + b_ev);
    const uint32_t* d_first = (const uint32_t*)(dev + b_ev + b_tiles);
    const uint32_t* d_idx = (const uint32_t*)(dev + b_ev + b_tiles + b_first);
    const dim3 grid = sh::grid1d(nt, 1), block(shq::TILE_THREADS);
    const uint32_t ns = (uint32_t)track_samples;
    if (width == 2) {
        const int aligned = ((uintptr_t)track->ptr & 15) == 0;
        if (sh::knobs().seq_align == VEC2) hipLaunchKernelGGL((k_mix_events_i16<VEC2, 4>), grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
        else hipLaunchKernelGGL((k_mix_events_i16<FUNNEL, 4>), grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (short*)track->ptr, ns, aligned);
    }
    else if (width == 1) hipLaunchKernelGGL(k_mix_events_w<1>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
    else if (width == 3) hipLaunchKernelGGL(k_mix_events_w<3>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
    else hipLaunchKernelGGL(k_mix_events_w<4>, grid, block, 0, st, d_ev, d_tiles, d_first, d_idx, nt, (unsigned char*)track->ptr, ns);
    SH_CHECK_LAUNCH("k_mix_events");
    return SH_OK;
}

}  // extern "C"
