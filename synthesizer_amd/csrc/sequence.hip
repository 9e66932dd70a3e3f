// sequence.hip -- a list of placed samples mixed into a track in one launch (sh_mix_events, sh_mix_events_rate, sh_mix_events_pan,
// sh_mix_events_env, sh_mix_events_loop, sh_mix_events_rev, sh_mix_events_chan: Sample.mix_at_many, mixer.sequence).
//
// The track is cut into tiles (seqplan.hpp); one workgroup per tile that some event touches walks that tile's events IN LIST ORDER, every
// lane keeping its own few track samples in registers from the one load of the base to the one store of the result.  Lanes own disjoint
// samples and read the track only there, so the fold is in place; a source may not be the track.  Per event, in this order -- none of
// the steps commute, and the bytes are those of the loop of copy().speed().clip().envelope().stereo() or .mono() / at_volume / mix_at it
// replaces:
//
//   region     a slice of the recording: where the record's pointer stands and how many frames the steps below may count; reversed
//              (audioop.reverse: the order of the SAMPLES) the pointer stands behind the slice and sample i is ptr[-1 - i] (seqrev.hpp),
//              applied where a sample is fetched, behind the loop's map; everything below sees the reversed frames.
//   loop       a note longer than its recording: the event's frames are VIRTUAL ones, frame v of the source up to the loop's end and the
//              loop region again and again behind it (seqloop.hpp), mapped where they are fetched; everything below sees virtual frames.
//   fetch      the event's source samples that land on the lane's track samples, zeros outside the event (x + 0 is the identity of the
//              saturating add, fbound(0 * f) == 0).  A plain event (inr == outr): vector loads at 16 bits (seq_load), byte-assembled
//              samples at widths 1, 3, 4.  A resampled one: audioop.ratecv, output frame m formed by whichever lane owns the track
//              sample it lands on (seq_rate; ratecv.hpp: the position in closed form, the sample arithmetic), never materialised.
//   the cut    the event's n: the host has checked that the samples exist.
//   envelope   Sample.envelope's gain (she::shape_lane, seqenv.hpp) on the (resampled, cut) source samples.
//   tostereo   a mono source into a stereo track: audioop.tostereo, frame f -> (fbound(s * left), fbound(s * right)), in the same lane.
//   channels   a STEREO source weighed per channel, where tostereo stands (an event has one of the three or none).  Downmix, into a mono
//              track: audioop.tomono, frame f -> fbound(l * left + r * right), two products and a sum with three roundings (k_tomono's
//              statement) -- a lane's N track samples are 2 N source samples, fetched and shaped as two halves of N, so everything
//              above runs over the stereo samples with coordinates doubled (2 (dst + n) in 32 bits: the entry point refuses the rest).
//              Balance, in a stereo track: even samples fbound(x * left), odd ones fbound(x * right); a side of exactly 1.0: none.
//   mul        audioop.mul (fbound: clamp, then floor); a factor of exactly 1.0: none.
//   add        audioop.add, saturating AT EVERY EVENT.
//
// A feature LEVEL says how much of the chain a list may ask for, and with it which record a kernel reads: PLAIN (fetch of plain events,
// mul, add: sh_mix_events), RATE (+ ratecv: sh_mix_events_rate), PAN (+ tostereo: sh_mix_events_pan), ENV (+ envelope:
// sh_mix_events_env), LOOP (+ the sustain loop: sh_mix_events_loop), REV (+ reversed playback: sh_mix_events_rev; its five kernels are
// reached from that entry point alone), CHAN (+ downmix and balance: sh_mix_events_chan; five kernels again, reached from there
// alone).  seq_event is the chain up to the mul, written once: a stage above the level is removed by `if constexpr`, a stage of the
// level that an event does not use is skipped by a wave-uniform branch on its record (a row of sh_mix_events_loop without a loop is an
// event of ENV).  The loop around it -- events [e, e1) of a tile's index folded into a lane's accumulator in list order -- is a SCHEDULE,
// and there are three, each written once: seq_walk_plain16 (PLAIN at 16 bits: INFLIGHT records and source vectors in flight),
// seq_walk_16 (the other levels at 16 bits: one record ahead, from LOOP on the next record's index) and seq_walk_w (widths 1, 3, 4,
// event by event).  Three kernel templates, k_seq_plain16, k_seq_16 and k_seq_w, are a schedule between the load of a tile's track
// samples and their store.  Built with -ffp-contract=off (the float64 product of audioop.mul stays one rounding, ratecv's
// prev*d + cur*(outr-d) two, tomono's l*left + r*right three).
//
// A list that is KEPT (sh_seq_create: the checks, the records of the lowest level that covers every row, the segments and
// shq::plan_by_tile's index -- every tile of the song in song order -- uploaded once into a block the handle owns) is rendered window by
// window by three more templates, k_win_plain16, k_win_16 and k_win_w, which mirror the three above and call the same three schedules:
// one workgroup per song tile of the window (workgroup k takes tile lo / TILE + k; a window that is the WHOLE song takes
// tile order[k], the tiles heaviest first, a permutation the handle keeps -- song order lost to it when measured), lanes at SONG positions, the fold started from silence, every sample of the
// window stored (zeros in a tile no event touches) through a pointer the host has biased by out_sample - first_sample, one 16-byte
// vector per lane where the lane lies inside the window and the host found the biased base aligned.  sh_seq_render is that one launch and
// copies nothing; a window of the song holds the bytes of that slice of the whole song, since every track sample is its own fold.
// A song of TRACKS (sh_seq_create_tracks) is rendered by the BUS = true instantiations of the same three templates, a gain per track in
// the kernel arguments (sh_seq_render_gains): seq_runs, written once, walks the runs of the tile -- the kernel's schedule over a run's
// events into a sub-mix, the sub-mix by its gain, a hook, the saturating add into the master.  With a metering bus (METERS) the hook
// reduces one row of levels per track, post-fader, and the same launch one for the master, into a table the handle owns
// (sh_seq_render_meters; seqmeter.hpp); seq_window_bus is what a window kernel does with either bus.  On the host one launcher,
// seq_window_launch, forwards the bus as the kernels' trailing pack: none, or a SeqBusOf<F> -- ONE bus type, F the set of FEATURES of
// seqbus.hpp, whose route() says which set a call takes; seq_with_level turns the level a handle holds into a template argument and
// seq_with_bus the set of features.  What each feature adds to this chain is stated once, above its part or its function: the DESK (a
// pan pot per track and a master fader: SeqDesk), AUTOMATION (fader moves per track: SeqAuto), GROUPS (a third accumulator between sub
// and acc, closed into the master: SeqGroups), RIDES and PANS (moves on the bus levels and of the pans, lanes of the automation's table
// and no kernel argument: seq_ride, seq_pan_ride), the HISTORY (the rows a workgroup reduced, kept per song tile: seq_hist_end), the
// OVERS (counting accumulators through the same schedules and the same seq_runs, which are generic in the accumulator's type) and the
// STEMS (the lanes STORE every bus where a metering bus reduces it: SeqStems, seq_stems_bus).
#include "common.hpp"
#include "chain.hpp"
#include "pcmdev.hpp"
#include "ratecv.hpp"
#include "seqauto.hpp"
#include "seqbus.hpp"
#include "seqclip.hpp"
#include "seqpan.hpp"
#include "seqenv.hpp"
#include "seqgroup.hpp"
#include "seqhist.hpp"
#include "seqloop.hpp"
#include "seqmeter.hpp"
#include "seqrev.hpp"
#include "seqplan.hpp"
#include "seqstem.hpp"
#include <math.h>
#include <string.h>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

// A source pointer comes out of a record in memory, so the compiler cannot know its address space and would read through it with flat
// loads: the sources are device buffers, say so (global_load).
#define SH_SEQ_GLOBAL __attribute__((address_space(1)))
typedef const SH_SEQ_GLOBAL short* gshort_p;
typedef const SH_SEQ_GLOBAL unsigned char* gbyte_p;
typedef int int_u1 __attribute__((aligned(1)));

enum Level { PLAIN = 0, RATE = 1, PAN = 2, ENV = 3, LOOP = 4, REV = 5, CHAN = 6 };

// ---- the records: one event as the kernels read it, wave-uniform, so fetched by scalar loads ------------------------------------------
struct SeqEv {                // PLAIN, 32 bytes
    const void* src;          // the first sample taken from the source
    double      factor;       // audioop.mul's; exactly 1.0: none
    uint32_t    dst;          // where in the track its first sample lands (samples)
    uint32_t    n;            // samples, > 0 for every event a tile lists
    uint32_t    pad[2];
};
// RATE, 64 bytes.  inr == outr: a plain event, src its first sample.  Otherwise src is input frame 0, and track sample dst + i is channel
// i % nch of output frame i / nch of audioop.ratecv(src, width, nch, inr, outr): the host has checked that the n samples exist
// (n <= out_frames(source frames) * nch), so every input frame a lane computes lies inside the source and the kernels test nothing but
// [0, n).
struct SeqEvR {
    const void* src;
    double      factor;       // audioop.mul's, after everything else; exactly 1.0: none
    double      inv_outr;     // 1.0 / outr
    uint32_t    dst, n;       // as SeqEv's, n counting RESAMPLED samples
    uint32_t    inr, outr;    // reduced rates
    uint32_t    step_q, step_r;   // inr / outr, inr % outr (shr::step)
    uint32_t    nch;          // the SOURCE's channel count
    uint32_t    small;        // 1: shr::small_int (8/16-bit samples, outr < 65536), 0: the float64 expression (shr::shifted_int)
    uint32_t    pad[2];
};
// PAN, 96 bytes.  tostereo == 0: an event of RATE.  tostereo == 1: a mono source into a stereo track -- dst and n count TRACK samples,
// both even, and track frame dst / 2 + f is frame f of the mono source (plain) or of audioop.ratecv(src, width, 1, inr, outr)
// (resampled) through audioop.tostereo's two factors.
struct SeqEvP : SeqEvR {
    double   left, right;
    uint32_t pad2[2];
    uint32_t tostereo;
    uint32_t pad3;
};
// ENV, 96 bytes: SeqEvP with its padding put to use.  nseg > 0: segs[seg0 .. seg0 + nseg) (she::Seg, seqenv.hpp) shape the event's source
// samples -- the samples of the mono frames for a tostereo event.
struct SeqEvE : SeqEvR {
    double   left, right;
    uint32_t seg0, nseg;
    uint32_t tostereo;
    uint32_t pad3;
};
// LOOP, 96 bytes: SeqEvE with the rest of its padding put to use (a fourth 32 bytes, held one record ahead as well, cost the 16-bit
// kernels scalar-register spills).  loop_len() == 0: an event of ENV.  Otherwise the event plays VIRTUAL frames (seqloop.hpp): virtual
// frame v is frame v of src while v < loop_end() and frame loop_end() - loop_len() + (v - loop_end()) % loop_len() after it; everything SeqEvR says
// of input frames it says of virtual ones, and the host has checked that the n samples exist among the V virtual frames (V * nch < 2^32:
// 32-bit indices).
struct SeqEvL : SeqEvE {
    SH_HD uint32_t loop_end() const { return pad[0]; }                    // E, frames from src
    SH_HD uint32_t loop_len() const { return pad[1]; }                    // E - S
    SH_HD uint32_t step_mod() const { return pad3; }                      // step_q % loop_len: what one ratecv step adds to a cursor's phase
    SH_HD uint32_t seam() const { return loop_end() * nch; }              // the first source SAMPLE behind the head
};
// REV, 96 bytes: SeqEvL, and bit 1 of `small` -- a word that held 0 or 1 -- says reversed.  reversed() == 0: an event of LOOP.  Otherwise
// src stands one sample BEHIND the event's region and sample i of what SeqEvL describes is src[-1 - i] (seqrev.hpp): dst, n, nch, the
// rates and the loop count reversed frames, and the host has checked that the region lies inside its source.
struct SeqEvV : SeqEvL {
    SH_HD uint32_t reversed() const { return small >> 1; }
    SH_HD uint32_t small_int() const { return small & 1u; }
};
// CHAN, 96 bytes: SeqEvV again, and the word `tostereo` -- 0 or 1 up to REV -- says which channel step the event takes (SeqMode).  NONE
// and TOSTEREO: an event of REV.  DOWNMIX: a stereo source into a mono track -- dst and n count TRACK (mono) samples, track sample dst + f
// is frame f of what SeqEvV describes with nch == 2 (region, reversal, loop, ratecv and envelope over the stereo samples) through
// audioop.tomono's two factors; the host has checked that 2 (dst + n) fits 32 bits.  BALANCE: a stereo source in a stereo track, its even
// samples through fbound(x * left) and its odd ones through fbound(x * right); dst is even.
enum SeqMode : uint32_t { SEQ_NONE = 0, SEQ_TOSTEREO = 1, SEQ_DOWNMIX = 2, SEQ_BALANCE = 3 };
static_assert(sizeof(SeqEv) == 32, "SeqEv is read as one 32-byte scalar load");
static_assert(sizeof(SeqEvR) == 64, "SeqEvR is read as one 64-byte scalar load");
static_assert(sizeof(SeqEvP) == 96 && sizeof(SeqEvE) == 96, "SeqEvP and SeqEvE are read as a 64-byte and a 32-byte scalar load");
static_assert(sizeof(SeqEvL) == 96 && sizeof(SeqEvL) % 32 == 0, "SeqEvL is read as a 64-byte and a 32-byte scalar load");
static_assert(sizeof(SeqEvV) == 96, "SeqEvV is SeqEvL: the flag rides in a word that is there");

template <int LEVEL> struct SeqRec;
template <> struct SeqRec<PLAIN> { typedef SeqEv type; };
template <> struct SeqRec<RATE> { typedef SeqEvR type; };
template <> struct SeqRec<PAN> { typedef SeqEvP type; };
template <> struct SeqRec<ENV> { typedef SeqEvE type; };
template <> struct SeqRec<LOOP> { typedef SeqEvL type; };
template <> struct SeqRec<REV> { typedef SeqEvV type; };
template <> struct SeqRec<CHAN> { typedef SeqEvV type; };

// ---- the lane shapes: eight 16-bit samples (one aligned 16-byte vector), four samples of widths 1, 3, 4 (bytes assembled for 24-bit
// samples, 64-bit sums for 32-bit ones -- the shape of k_mix_chain_gather_w, pcm.hip, which says why these widths get the plain loop) ----
template <int WIDTH> constexpr int SEQ_LANE = WIDTH == 2 ? (int)shq::LANE_SAMPLES_I16 : (int)shq::LANE_SAMPLES_W;
template <int WIDTH> constexpr uint32_t SEQ_TILE = WIDTH == 2 ? shq::TILE_I16 : shq::TILE_W;
template <int WIDTH> constexpr long long SEQ_HI = WIDTH == 1 ? 127LL : (WIDTH == 2 ? 32767LL : (WIDTH == 3 ? 8388607LL : 2147483647LL));
template <int WIDTH> constexpr long long SEQ_LO = -SEQ_HI<WIDTH> - 1;
// N samples in registers: packed at 16 bits, an int each at the other widths; x[j] reads and writes either
template <int WIDTH, int N> struct SeqVec { typedef int type[N]; };
template <int N> struct SeqVec<2, N> { typedef typename ShortVec<N>::type type; };

// ---- fetch ------------------------------------------------------------------------------------------------------------------------------
// How a lane gets the N (eight; four of a mono source, whose four frames are the lane's eight stereo samples) 16-bit samples of an event
// that start at sample `rel` of its source, when they sit at any 2-byte offset against the lane's aligned 2 N bytes.  All lanes of a
// workgroup start on multiples of N samples, so that offset -- (src - 2 dst) mod 2 N -- is the same for every lane: wave-uniform per event.
//   FUNNEL  two aligned 2 N-byte loads and a funnel shift by that byte count (v_alignbyte_b32); an aligned event takes one load.
//   VEC2    one load through a vector type of alignment 2: the compiler emits ONE global_load_dwordx4 / x2 at the odd address (read
//           in the ISA: no global_load_ushort), the memory pipeline splits what crosses a line.
// FUNNEL is the default and SYNTHHIP_SEQ_ALIGN=1 selects VEC2.  Measured (profiles/sequence_ab.txt; one call of Sample.mix_at_many on the
// 120-s song with 4096 / 32 768 events, 75 % of the starts misaligned): 3.36 / 30.6 ms against 3.48 / 31.5 ms -- within 4 %, and that call is
// still bound by the host's table packing, so the choice is not settled by it: FUNNEL stays because it asks nothing of how the memory
// pipeline treats a vector load that straddles a line.  Staging an event's span through LDS was not built.
// Lanes on the edges of an event (not all N samples inside it; FUNNEL: not both aligned vectors inside the source) assemble their samples
// one by one.
enum Scheme { FUNNEL = 0, VEC2 = 1 };

// FUNNEL: the N samples at p, which lies sh bytes (0 < sh < 2 N, even, uniform) behind an aligned 2 N bytes: that vector and the next
template <int N, typename P>
__device__ __forceinline__ typename ShortVec<N>::type seq_funnel(P p, uint32_t sh) {
    typedef typename ShortVec<N>::type vec;
    typedef int words __attribute__((ext_vector_type(N / 2)));
    constexpr int W = N / 2;
    const SH_SEQ_GLOBAL words* q = (const SH_SEQ_GLOBAL words*)((uintptr_t)p - sh);
    const words lo = q[0], hi = q[1];
    int w[2 * W];
#pragma unroll
    for (int i = 0; i < W; ++i) { w[i] = lo[i]; w[W + i] = hi[i]; }
    const uint32_t r = sh & 3;
    union { words v; vec s; } o;
    auto funnel = [&](auto K) {                       // from word K of the 2 N bytes on
        constexpr int k = decltype(K)::value;
#pragma unroll
        for (int i = 0; i < W; ++i) o.v[i] = (int)__builtin_amdgcn_alignbyte(w[k + i + 1], w[k + i], r);
    };
    if constexpr (W == 2) {
        if (sh < 4) funnel(std::integral_constant<int, 0>());
        else funnel(std::integral_constant<int, 1>());
    } else {
        switch (sh >> 2) {                              // (uniform)
        case 0: funnel(std::integral_constant<int, 0>()); break;
        case 1: funnel(std::integral_constant<int, 1>()); break;
        case 2: funnel(std::integral_constant<int, 2>()); break;
        default: funnel(std::integral_constant<int, 3>()); break;
        }
    }
    return o.s;
}

template <int N, int SCHEME>
__device__ __forceinline__ typename ShortVec<N>::type seq_load(gshort_p src, uint32_t dst, uint32_t n, uint32_t s0) {
    typedef typename ShortVec<N>::type vec;
    typedef short vecu __attribute__((ext_vector_type(N), aligned(2)));       // N samples at any sample offset
    const long long rel = (long long)s0 - (long long)dst;
    vec x = 0;
    if (rel + N <= 0 || rel >= (long long)n) return x;
    if constexpr (SCHEME == VEC2) {
        if (rel >= 0 && rel + N <= (long long)n) return *(const SH_SEQ_GLOBAL vecu*)(src + rel);
    } else {
        const uint32_t sh = (uint32_t)(((uintptr_t)src - 2 * (uintptr_t)dst) & (2 * N - 1));      // (uniform) 0, 2 .. 2 N - 2
        if (sh == 0) {
            if (rel >= 0 && rel + N <= (long long)n) return *(const SH_SEQ_GLOBAL vec*)(src + rel);
        } else if (rel >= N && rel + 2 * N <= (long long)n) {
            return seq_funnel<N>(src + rel, sh);
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (rel + j >= 0 && rel + j < (long long)n) x[j] = src[rel + j];
    return x;
}

// The same of a REVERSED event: `end` stands one sample behind its region, and the lane's N samples from event sample rel on are the N
// contiguous stored samples end[-rel - N .. -rel) in reverse order -- one vector load under either scheme (FUNNEL: those samples start
// (end + 2 dst) mod 2 N bytes behind an aligned vector, uniform again, since every lane starts on a multiple of N samples), then the N
// shorts turned round in registers.  The conditions are seq_load's, in event samples: a vector is read only where all of it holds samples
// of the event, so no load leaves the region, let alone the buffer; lanes on the edges assemble sample by sample.
template <int N, int SCHEME>
__device__ __forceinline__ typename ShortVec<N>::type seq_load_rev(gshort_p end, uint32_t dst, uint32_t n, uint32_t s0) {
    typedef typename ShortVec<N>::type vec;
    typedef short vecu __attribute__((ext_vector_type(N), aligned(2)));
    const long long rel = (long long)s0 - (long long)dst;
    vec x = 0;
    if (rel + N <= 0 || rel >= (long long)n) return x;
    gshort_p lo = end + shv::offset(1u, (uint64_t)(rel + N - 1));      // the lowest of the lane's stored samples: event sample rel + N - 1
    const bool inside = rel >= 0 && rel + N <= (long long)n;
    bool got = false;
    vec m = 0;
    if constexpr (SCHEME == VEC2) {
        if (inside) { m = *(const SH_SEQ_GLOBAL vecu*)lo; got = true; }
    } else {
        const uint32_t sh = (uint32_t)(((uintptr_t)end + 2 * (uintptr_t)dst) & (2 * N - 1));      // (uniform) 0, 2 .. 2 N - 2
        if (sh == 0) {
            if (inside) { m = *(const SH_SEQ_GLOBAL vec*)lo; got = true; }
        } else if (rel >= N && rel + 2 * N <= (long long)n) {
            m = seq_funnel<N>(lo, sh);
            got = true;
        }
    }
    if (got) {
#pragma unroll
        for (int j = 0; j < N; ++j) x[j] = m[N - 1 - j];
        return x;
    }
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (rel + j >= 0 && rel + j < (long long)n) x[j] = end[shv::offset(1u, (uint64_t)(rel + j))];
    return x;
}

// sample i of a source of WIDTH bytes per sample, sign-extended: chain_get (pcmdev.hpp) through a pointer that says where a source lives
template <int WIDTH>
__device__ __forceinline__ int seq_get(gbyte_p p, size_t i) {
    if (WIDTH == 1) return (int)(signed char)p[i];
    if (WIDTH == 2) return (int)((gshort_p)p)[i];
    if (WIDTH == 3) {
        gbyte_p q = p + 3 * i;
        return (int)q[0] | ((int)q[1] << 8) | ((int)(signed char)q[2] << 16);
    }
    return *(const SH_SEQ_GLOBAL int_u1*)(p + 4 * i);
}

// seq_get at an offset of either sign against the pointer (shv::offset: a reversed event's samples lie in front of it).  A copy of
// seq_get on purpose, for the REV kernels alone: giving seq_get itself a signed index changes the instructions of the kernels of the
// other levels, which are held to what they were (profiles/sequence_rev_ab.txt, section 1).
template <int WIDTH>
__device__ __forceinline__ int seq_get_at(gbyte_p p, int64_t i) {
    if (WIDTH == 1) return (int)(signed char)p[i];
    if (WIDTH == 2) return (int)((gshort_p)p)[i];
    if (WIDTH == 3) {
        gbyte_p q = p + 3 * i;
        return (int)q[0] | ((int)q[1] << 8) | ((int)(signed char)q[2] << 16);
    }
    return *(const SH_SEQ_GLOBAL int_u1*)(p + 4 * i);
}

// A lane's N consecutive samples from sample f0 on, as a plain event gives them
template <int WIDTH, int SCHEME, int N>
__device__ __forceinline__ void seq_plain(const void* src, uint32_t dst, uint32_t n, uint32_t f0, typename SeqVec<WIDTH, N>::type& x) {
    if constexpr (WIDTH == 2) {
        x = seq_load<N, SCHEME>((gshort_p)src, dst, n, f0);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const long long rel = (long long)f0 + j - (long long)dst;
            x[j] = rel >= 0 && rel < (long long)n ? seq_get<WIDTH>((gbyte_p)src, (size_t)rel) : 0;
        }
    }
}

// and as a plain REVERSED event gives them
template <int WIDTH, int SCHEME, int N>
__device__ __forceinline__ void seq_plain_rev(const void* end, uint32_t dst, uint32_t n, uint32_t f0, typename SeqVec<WIDTH, N>::type& x) {
    if constexpr (WIDTH == 2) {
        x = seq_load_rev<N, SCHEME>((gshort_p)end, dst, n, f0);
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const long long rel = (long long)f0 + j - (long long)dst;
            x[j] = rel >= 0 && rel < (long long)n ? seq_get_at<WIDTH>((gbyte_p)end, shv::offset(1u, (uint64_t)rel)) : 0;
        }
    }
}

// sample i of the frames that event c plays: of its source, or (SeqEvV, reversed) of its reversed region, mapped to memory here
template <int WIDTH, typename Rec>
__device__ __forceinline__ int seq_at(const Rec& c, gbyte_p src, size_t i) {
    if constexpr (std::is_same<Rec, SeqEvV>::value) return seq_get_at<WIDTH>(src, shv::offset(c.reversed(), i));
    else return seq_get<WIDTH>(src, i);
}

template <typename Rec>
__device__ __forceinline__ uint32_t seq_small(const Rec& c) {          // (SeqEvV: the word carries the reversed flag as well)
    if constexpr (std::is_same<Rec, SeqEvV>::value) return c.small_int();
    else return c.small;
}

// A lane's N consecutive track samples from s0 on, as a resampled event gives them: zeros outside the event (the identity of the fold,
// as seq_load's edges), inside it frame m = rel / nch and channel rel % nch -- the position of the lane's first frame once (shr::position),
// then shr::step per frame -- prev = frame j - 1 (zero when j == 0 or d == 0, as k_resample), cur = frame j, both straight from global
// memory: an instrument is a few tens of KB that every note re-reads (L2 / TCP hits), and a lane's samples span about
// N / nch * speed + 2 input frames.  get(i): sample i of the source, sign-extended.
// A looped event (SeqEvL, loop_len != 0): positions, j and d are those of the VIRTUAL frames, and cur and prev are mapped one by one
// (seqloop.hpp), so the interpolation runs across the seam, from frame E - 1 to frame S.  d != 0 exactly when r != 0: cur is virtual
// frame q + 1 and prev is q; d == 0: cur is q and there is no prev.  The lane keeps the cursor of q: one division where it starts,
// then step_mod and the carry per frame, by compare and subtract -- a step may be longer than the loop.
// A reversed event (SeqEvV): positions, j, d and the cursor are those of the REVERSED frames, and get maps an index to memory last.
template <int WIDTH, int N, typename Rec, typename Get>
__device__ __forceinline__ void seq_rate(const Rec& c, uint32_t s0, Get get, int (&x)[N]) {
    constexpr bool LOOPED = std::is_base_of<SeqEvL, Rec>::value;
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = 0;
    const long long rel = (long long)s0 - (long long)c.dst;
    if (rel + N <= 0 || rel >= (long long)c.n) return;
    const uint32_t r0 = rel > 0 ? (uint32_t)rel : 0u;                  // the first sample of the event that this lane owns
    uint32_t m, ch;                                                     // (nch is uniform)
    if (c.nch == 1) { m = r0; ch = 0; }
    else if (c.nch == 2) { m = r0 >> 1; ch = r0 & 1u; }
    else { m = r0 / c.nch; ch = r0 - m * c.nch; }
    shr::Pos p = shr::position(m, c.inr, c.outr, c.inv_outr);
    shl::Cur lc{0u, 0u};
    if constexpr (LOOPED)
        if (c.loop_len()) lc = shl::at((uint32_t)p.q, c.loop_end(), c.loop_len());       // (uniform branch; q < V < 2^32)
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const long long r = rel + k;
        if (r < 0 || r >= (long long)c.n) continue;
        uint64_t j;
        uint32_t d;
        shr::index(p, c.outr, j, d);
        int cur = 0, prev = 0;
        bool mapped = false;
        if constexpr (LOOPED) {
            if (c.loop_len()) {
                shl::Cur lj = lc;
                if (d) shl::step1(lj, c.loop_end(), c.loop_len());
                cur = get((size_t)shl::frame(lj, c.loop_end()) * c.nch + ch);
                prev = d ? get((size_t)shl::frame(lc, c.loop_end()) * c.nch + ch) : 0;
                mapped = true;
            }
        }
        if (!mapped) {
            const size_t at = (size_t)j * c.nch + ch;
            cur = get(at);
            prev = (j && d) ? get(at - c.nch) : 0;
        }
        if constexpr (WIDTH <= 2) {
            typedef typename std::conditional<WIDTH == 1, signed char, short>::type T;
            x[k] = seq_small(c) ? (int)shr::small_int<T>((T)prev, (T)cur, d, c.outr, c.inv_outr)
                           : shr::shifted_int(prev, cur, d, c.outr, c.inv_outr, 32 - 8 * WIDTH);
        } else {
            x[k] = shr::shifted_int(prev, cur, d, c.outr, c.inv_outr, 32 - 8 * WIDTH);
        }
        if (++ch == c.nch) {
            ch = 0;
            const uint64_t q0 = p.q;
            shr::step<uint64_t>(p.q, p.r, (uint64_t)c.step_q, c.step_r, c.outr);
            if constexpr (LOOPED) {
                if (c.loop_len()) {
                    shl::step(lc, c.step_q, c.step_mod(), c.loop_end(), c.loop_len());
                    if (p.q - q0 != (uint64_t)c.step_q) shl::step1(lc, c.loop_end(), c.loop_len());
                }
            }
        }
    }
}

// A lane's N consecutive samples from sample f0 on, as a plain LOOPED event gives them where its tile reaches the seam or lies behind it:
// sample by sample through seq_at (global loads; a reversed event's index is mapped to memory last) at mapped frames, the cursor of the
// lane's first frame from scratch, then one frame on per frame.  NOT built: a vector read inside one loop pass -- which pass, and so which alignment against the lane's vector, differs from
// lane to lane there, so it is not wave-uniform and FUNNEL does not apply; a later A/B.
template <int WIDTH, int N, typename Rec>
__device__ __forceinline__ void seq_looped(const Rec& c, uint32_t f0, int (&x)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = 0;
    const long long rel = (long long)f0 - (long long)c.dst;
    if (rel + N <= 0 || rel >= (long long)c.n) return;
    const uint32_t r0 = rel > 0 ? (uint32_t)rel : 0u;
    uint32_t v, ch;                                                     // (nch is uniform)
    if (c.nch == 1) { v = r0; ch = 0; }
    else if (c.nch == 2) { v = r0 >> 1; ch = r0 & 1u; }
    else { v = r0 / c.nch; ch = r0 - v * c.nch; }
    shl::Cur lc = shl::at(v, c.loop_end(), c.loop_len());
    gbyte_p src = (gbyte_p)c.src;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const long long r = rel + k;
        if (r < 0 || r >= (long long)c.n) continue;
        x[k] = seq_at<WIDTH>(c, src, (size_t)shl::frame(lc, c.loop_end()) * c.nch + ch);
        if (++ch == c.nch) {
            ch = 0;
            shl::step1(lc, c.loop_end(), c.loop_len());
        }
    }
}

// ---- one event, up to the mul -------------------------------------------------------------------------------------------------------------
// What the tile [t0, t0 + tile) of the track takes of an event, in the event's source samples (sh = 1: a tostereo event, whose source
// samples are track frames; dst, n, t0 and tile are even then): [tlo, thi), uniform.  The tile lists the event, so they overlap.
__device__ __forceinline__ void seq_env_span(const SeqEvE& c, uint32_t t0, uint32_t tile, uint32_t& tlo, uint32_t& thi) {
    const uint32_t sh = c.tostereo, d = c.dst >> sh, n = c.n >> sh, a = t0 >> sh, b = a + (tile >> sh);       // (no wrap: MAX_TRACK_SAMPLES)
    tlo = a > d ? a - d : 0u;
    thi = (b < d + n ? b : d + n) - d;
}

// The same of a CHAN record, whose word says more than 0 or 1: a downmix's source samples are two to a track sample (the opposite shift;
// no wrap: the host has checked 2 (dst + n), and the tile overlaps the event).
__device__ __forceinline__ void seq_env_span_chan(const SeqEvV& c, uint32_t t0, uint32_t tile, uint32_t& tlo, uint32_t& thi) {
    const uint32_t sh = c.tostereo == SEQ_TOSTEREO ? 1u : 0u, d = c.dst >> sh, n = c.n >> sh, a = t0 >> sh, b = a + (tile >> sh);
    const uint32_t up = c.tostereo == SEQ_DOWNMIX ? 1u : 0u;
    tlo = (a > d ? a - d : 0u) << up;
    thi = ((b < d + n ? b : d + n) - d) << up;
}

// fetch and envelope: the N source samples of event c from its sample f0 on -- c.dst, c.n and f0 count what the event resamples and
// shapes: track samples, or the frames of a tostereo event.  An enveloped event shapes them with she::shape_lane: float64 per sample only
// inside a ramp, one fbound multiply inside the sustain, nothing inside a plain stretch, a per-sample select only in a tile that
// straddles a boundary.
template <int LEVEL, int WIDTH, int SCHEME, int N>
__device__ __forceinline__ void seq_source(const typename SeqRec<LEVEL>::type& c, const she::Seg* __restrict__ segs, uint32_t tlo, uint32_t thi,
                                           uint32_t f0, typename SeqVec<WIDTH, N>::type& x) {
    if constexpr (LEVEL == PLAIN) {
        seq_plain<WIDTH, SCHEME, N>(c.src, c.dst, c.n, f0, x);
    } else {
        int v[N];                                             // (ENV: the join below carries ints, as she::shape_lane takes them)
        if (c.inr == c.outr) {                                // (uniform, as every branch on the record)
            bool gathered = false;
            if constexpr (LEVEL >= LOOP) {                        // what the tile takes lies wholly in the head: the plain path below
                if (c.loop_len() && thi > c.seam()) {
                    seq_looped<WIDTH, N>(c, f0, v);
                    gathered = true;
                }
            }
            if (!gathered) {
                uint32_t n = c.n;                                 // (a looped event's n may reach past the source: the head ends at the seam,
                if constexpr (LEVEL >= LOOP)                      // and seq_load's second vector must not be read behind it)
                    if (c.loop_len() && c.seam() < n) n = c.seam();
                bool turned = false;
                if constexpr (LEVEL >= REV) {
                    if (c.reversed()) {
                        seq_plain_rev<WIDTH, SCHEME, N>(c.src, c.dst, n, f0, x);
                        turned = true;
                    }
                }
                if (!turned) seq_plain<WIDTH, SCHEME, N>(c.src, c.dst, n, f0, x);
                if constexpr (LEVEL >= ENV) {
#pragma unroll
                    for (int j = 0; j < N; ++j) v[j] = (int)x[j];
                }
            }
        } else {
            gbyte_p src = (gbyte_p)c.src;
            seq_rate<WIDTH, N>(c, f0, [&](size_t i) { return seq_at<WIDTH>(c, src, i); }, v);
            if constexpr (LEVEL < ENV) {
#pragma unroll
                for (int j = 0; j < N; ++j) x[j] = v[j];
            }
        }
        if constexpr (LEVEL >= ENV) {
            if (c.nseg) she::shape_lane<N>(segs + c.seg0, c.nseg, tlo, thi, (long long)f0 - (long long)c.dst, v, (double)SEQ_LO<WIDTH>, (double)SEQ_HI<WIDTH>);
#pragma unroll
            for (int j = 0; j < N; ++j) x[j] = v[j];
        }
    }
}

// What event c gives the lane's track samples from s0 on, before the mul: fetch, the cut, envelope, tostereo.
template <int LEVEL, int WIDTH, int SCHEME>
__device__ __forceinline__ void seq_event(const typename SeqRec<LEVEL>::type& c, const she::Seg* __restrict__ segs, uint32_t t0, uint32_t s0,
                                          typename SeqVec<WIDTH, SEQ_LANE<WIDTH>>::type& x) {
    constexpr int N = SEQ_LANE<WIDTH>;
    uint32_t tlo = 0, thi = 0;
    if constexpr (LEVEL == ENV)
        if (c.nseg) seq_env_span(c, t0, SEQ_TILE<WIDTH>, tlo, thi);
    if constexpr (LEVEL == LOOP || LEVEL == REV)
        if (c.nseg || c.loop_len()) seq_env_span(c, t0, SEQ_TILE<WIDTH>, tlo, thi);
    if constexpr (LEVEL == CHAN) {
        if (c.nseg || c.loop_len()) seq_env_span_chan(c, t0, SEQ_TILE<WIDTH>, tlo, thi);
        if (c.tostereo == SEQ_DOWNMIX) {                      // the lane's N mono samples are N stereo frames, 2 N source samples
            typename SeqRec<LEVEL>::type f = c;
            f.dst = c.dst << 1;
            f.n = c.n << 1;
            f.nch = 2;                                        // (as the host wrote it: said again for the compiler)
            constexpr double LO = (double)SEQ_LO<WIDTH>, HI = (double)SEQ_HI<WIDTH>;
#pragma nounroll
            for (int h = 0; h < 2; ++h) {                     // one copy of the chain in the code, run on each half
                typename SeqVec<WIDTH, N>::type m;
                seq_source<LEVEL, WIDTH, SCHEME, N>(f, segs, tlo, thi, (s0 << 1) + (uint32_t)h * N, m);
                int r[N / 2];                                 // audioop.tomono as k_tomono: two products, a sum, three roundings
#pragma unroll
                for (int j = 0; j < N / 2; ++j) r[j] = fbound((double)m[2 * j] * c.left + (double)m[2 * j + 1] * c.right, LO, HI);
                if (h == 0) {
#pragma unroll
                    for (int j = 0; j < N / 2; ++j) x[j] = r[j];
                } else {
#pragma unroll
                    for (int j = 0; j < N / 2; ++j) x[N / 2 + j] = r[j];
                }
            }
            return;
        }
    }
    if constexpr (LEVEL >= PAN) {
        bool mono;                                            // (CHAN: the word carries the other modes as well)
        if constexpr (LEVEL == CHAN) mono = c.tostereo == SEQ_TOSTEREO;
        else mono = c.tostereo != 0;
        if (mono) {                                           // the lane's N track samples are N / 2 frames of the mono source
            typename SeqRec<LEVEL>::type f = c;
            f.dst = c.dst >> 1;
            f.n = c.n >> 1;
            f.nch = 1;                                        // (as the host wrote it: said again for the compiler, which drops seq_rate's other channel counts)
            typename SeqVec<WIDTH, N / 2>::type m;
            seq_source<LEVEL, WIDTH, SCHEME, N / 2>(f, segs, tlo, thi, s0 >> 1, m);
#pragma unroll
            for (int j = 0; j < N / 2; ++j) {
                const double s = (double)m[j];
                x[2 * j] = fbound(s * c.left, (double)SEQ_LO<WIDTH>, (double)SEQ_HI<WIDTH>);
                x[2 * j + 1] = fbound(s * c.right, (double)SEQ_LO<WIDTH>, (double)SEQ_HI<WIDTH>);
            }
            return;
        }
    }
    seq_source<LEVEL, WIDTH, SCHEME, N>(c, segs, tlo, thi, s0, x);
    if constexpr (LEVEL == CHAN) {
        if (c.tostereo == SEQ_BALANCE) {                      // lanes start on even samples, dst is even: even samples left, odd ones right
            constexpr double LO = (double)SEQ_LO<WIDTH>, HI = (double)SEQ_HI<WIDTH>;
            if (c.left != 1.0) {                              // (uniform; fbound(x * 1.0) == x: skipping changes no bytes)
#pragma unroll
                for (int j = 0; j < N; j += 2) x[j] = fbound((double)x[j] * c.left, LO, HI);
            }
            if (c.right != 1.0) {
#pragma unroll
                for (int j = 1; j < N; j += 2) x[j] = fbound((double)x[j] * c.right, LO, HI);
            }
        }
    }
}

// ---- 16-bit samples ---------------------------------------------------------------------------------------------------------------------
template <int LEVEL, int SCHEME>
__device__ __forceinline__ short8v seq_event8(const typename SeqRec<LEVEL>::type& c, const she::Seg* __restrict__ segs, uint32_t t0, uint32_t s0) {
    short8v x;
    seq_event<LEVEL, 2, SCHEME>(c, segs, t0, s0, x);
    return x;
}

// audioop.mul of a lane's samples: of an event's by its factor, of a folded track's by its gain
__device__ __forceinline__ short8v seq_scale8(short8v x, const double factor) {
    if (factor != 1.0) {                                      // (uniform)
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (short)fbound((double)x[j] * factor, Lim<short>::lo, Lim<short>::hi);
    }
    return x;
}

// mul and add
__device__ __forceinline__ void seq_fold8(short8v& acc, const short8v x, const double factor) {
    acc = __builtin_elementwise_add_sat(acc, seq_scale8(x, factor));
}

// A COUNTING accumulator (seqclip.hpp; the buses that count overs, shb::CLIPS): a lane's samples and one sticky over-flag per sample -- 0 or
// -1, a vector comparison's lanes, at 16 bits; bit j of a word at widths 1, 3, 4.  The schedules below are generic in the accumulator's
// type, so either kind passes through the same schedule text.
typedef unsigned short ushort8v __attribute__((ext_vector_type(8)));
struct SeqAccC8 { short8v v; short8v over; };
// seq_v: a lane's samples, of either kind of accumulator
__device__ __forceinline__ short8v& seq_v(short8v& a) { return a; }
__device__ __forceinline__ const short8v& seq_v(const short8v& a) { return a; }
__device__ __forceinline__ short8v& seq_v(SeqAccC8& a) { return a.v; }
__device__ __forceinline__ const short8v& seq_v(const SeqAccC8& a) { return a.v; }

// the saturating add of a lane's samples into a bus; counting: a packed add clamped exactly where the saturating and the WRAPPING packed
// sums differ (the wrapping one formed unsigned: tests/cpu_seqclip.cpp holds shcl::add_clamps16 to the exact sum) -- into's own step, so
// x's flags stay with x
__device__ __forceinline__ void seq_add8(short8v& into, const short8v& x) { into = __builtin_elementwise_add_sat(into, x); }
__device__ __forceinline__ void seq_add8(SeqAccC8& into, const short8v x) {
    const short8v sat = __builtin_elementwise_add_sat(into.v, x);
    into.over |= (ushort8v)sat != (ushort8v)into.v + (ushort8v)x;
    into.v = sat;
}
__device__ __forceinline__ void seq_add8(SeqAccC8& into, const SeqAccC8& x) { seq_add8(into, x.v); }

// mul and add, counting: the event's own mul is not counted (the sample as placed), the add is the track's
__device__ __forceinline__ void seq_fold8(SeqAccC8& acc, const short8v x, const double factor) { seq_add8(acc, seq_scale8(x, factor)); }

// audioop.mul of a bus's samples by its gain, counting: floor(p) against the range in front of fbound, then seq_scale8's bytes
__device__ __forceinline__ SeqAccC8 seq_scale8(SeqAccC8 a, const double factor) {
    if (factor != 1.0) {                                      // (uniform)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (shcl::mul_clamps<2>((double)a.v[j] * factor)) a.over[j] = (short)-1;
    }
    a.v = seq_scale8(a.v, factor);
    return a;
}

// A lane's eight track samples: one aligned 16-byte load of the base, one aligned 16-byte store.  whole: the track starts on a 16-byte
// boundary (a view that does not: sample by sample) and all eight samples exist.
__device__ __forceinline__ short8v seq_track_load8(const short* track, uint32_t s0, uint32_t track_samples, bool whole) {
    short8v acc = {0, 0, 0, 0, 0, 0, 0, 0};
    if (whole) acc = *reinterpret_cast<const short8v*>(track + s0);
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) acc[j] = track[s0 + j];
    return acc;
}

__device__ __forceinline__ void seq_track_store8(short* track, uint32_t s0, uint32_t track_samples, bool whole, const short8v acc) {
    if (whole) *reinterpret_cast<short8v*>(track + s0) = acc;
    else
        for (uint32_t j = 0; j < 8 && s0 + j < track_samples; ++j) track[s0 + j] = acc[j];
}

// ---- widths 1, 3 and 4 ------------------------------------------------------------------------------------------------------------------
// A lane's four 64-bit sums: a vector type, as short8v is, so that they pass through the schedule functions as one value in registers
typedef long long llong4v __attribute__((ext_vector_type(4)));

template <int WIDTH>
__device__ __forceinline__ void seq_track_load_w(const unsigned char* track, uint32_t s0, uint32_t track_samples, llong4v& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[j] = 0;
        if (s0 + j < track_samples) acc[j] = chain_get<WIDTH>(track, s0 + j);
    }
}

template <int WIDTH>
__device__ __forceinline__ void seq_track_store_w(unsigned char* track, uint32_t s0, uint32_t track_samples, const llong4v& acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (s0 + j < track_samples) chain_put<WIDTH>(track, s0 + j, acc[j]);
}

// mul and add of one sample, for an event (seq_fold_w) and for a track (seq_runs): x by the factor unless that is exactly 1.0 -- x is
// left scaled --, then the clamped 64-bit add; the sum
template <int WIDTH>
__device__ __forceinline__ long long seq_mul_add_w(const long long acc, long long& x, const double factor) {
    constexpr long long HI = SEQ_HI<WIDTH>, LO = SEQ_LO<WIDTH>;
    if (factor != 1.0) x = fbound((double)x * factor, (double)LO, (double)HI);
    const long long t = acc + x;
    return t > HI ? HI : (t < LO ? LO : t);
}

// the same, and whether each of its two steps clamped (seqclip.hpp): the scaling is a step of x's row -- a track's or a group's pan --,
// the add one of the destination's
template <int WIDTH>
__device__ __forceinline__ long long seq_mul_add_w(const long long acc, long long& x, const double factor, bool& scaled, bool& added) {
    scaled = factor != 1.0 && shcl::mul_clamps<WIDTH>((double)x * factor);
    const long long sum = seq_mul_add_w<WIDTH>(acc, x, factor);      // (x: scaled now)
    added = shcl::add_clamps<WIDTH>(acc, x);
    return sum;
}

// the counting accumulator of these widths: four sums and four sticky flags, bit j sample j's
struct SeqAccCW { llong4v v; uint32_t over; };
__device__ __forceinline__ llong4v& seq_v(llong4v& a) { return a; }
__device__ __forceinline__ const llong4v& seq_v(const llong4v& a) { return a; }
__device__ __forceinline__ llong4v& seq_v(SeqAccCW& a) { return a.v; }
__device__ __forceinline__ const llong4v& seq_v(const SeqAccCW& a) { return a.v; }
// a counting accumulator's flags as shcl::lane reads them
__device__ __forceinline__ const short8v& seq_flags(const SeqAccC8& a) { return a.over; }
__device__ __forceinline__ shcl::Bits seq_flags(const SeqAccCW& a) { return shcl::Bits{a.over}; }

// sample j of `from` (x: its value, left scaled) by the factor and into sample j of `into`: seq_mul_add_w; counting: the scaling's flag
// to `from`, the add's to `into`.  An EVENT's sample has no row: seq_add_w drops its scaling's flag (the sample as placed).
template <int WIDTH>
__device__ __forceinline__ void seq_into_w(llong4v& into, const int j, llong4v&, long long& x, const double factor) {
    into[j] = seq_mul_add_w<WIDTH>(into[j], x, factor);
}
template <int WIDTH>
__device__ __forceinline__ void seq_into_w(SeqAccCW& into, const int j, SeqAccCW& from, long long& x, const double factor) {
    bool scaled, added;
    into.v[j] = seq_mul_add_w<WIDTH>(into.v[j], x, factor, scaled, added);
    from.over |= (uint32_t)scaled << j;
    into.over |= (uint32_t)added << j;
}
template <int WIDTH>
__device__ __forceinline__ void seq_add_w(llong4v& acc, const int j, long long& x, const double factor) {
    acc[j] = seq_mul_add_w<WIDTH>(acc[j], x, factor);
}
template <int WIDTH>
__device__ __forceinline__ void seq_add_w(SeqAccCW& acc, const int j, long long& x, const double factor) {
    bool scaled, added;
    acc.v[j] = seq_mul_add_w<WIDTH>(acc.v[j], x, factor, scaled, added);
    acc.over |= (uint32_t)added << j;
}

// mul and add, where the event is; get(j, rel): what the event gives the lane's sample j, sample rel of the event
template <int WIDTH, typename Acc, typename Get>
__device__ __forceinline__ void seq_fold_w(Acc& acc, const double factor, uint32_t s0, uint32_t dst, uint32_t n, Get get) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long rel = (long long)s0 + j - (long long)dst;
        if (rel >= 0 && rel < (long long)n) {
            long long x = get(j, rel);
            seq_add_w<WIDTH>(acc, j, x, factor);
        }
    }
}

// ---- the schedules: events [e, e1) of idx folded into acc in list order, each written once -- the tile-list kernels call them over a
// tile's events into the track's samples, the window kernels over a tile's events from silence or over a RUN's events into a track's
// sub-mix (seq_runs) -----------------------------------------------------------------------------------------------------------------
// PLAIN at 16 bits.  INFLIGHT events' records (scalar loads, one batch ahead) and source vectors are in flight before their muls and
// adds, then a tail event by event -- a schedule of its own, measured (profiles/sequence_ab.txt).  [e, e1) may be empty.
template <int SCHEME, int INFLIGHT, typename Acc>
__device__ __forceinline__ void seq_walk_plain16(const SeqEv* __restrict__ ev, const she::Seg* __restrict__ segs, const uint32_t* __restrict__ idx,
                                                 uint32_t& e, const uint32_t e1, uint32_t t0, uint32_t s0, Acc& acc) {
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
            for (int u = 0; u < INFLIGHT; ++u) x[u] = seq_event8<PLAIN, SCHEME>(c[u], segs, t0, s0);
#pragma unroll
            for (int u = 0; u < INFLIGHT; ++u) seq_fold8(acc, x[u], c[u].factor);
            if (more) {
#pragma unroll
                for (int u = 0; u < INFLIGHT; ++u) c[u] = nx[u];
            }
        }
    }
    for (; e < e1; ++e) {
        const SeqEv c = ev[idx[e]];
        seq_fold8(acc, seq_event8<PLAIN, SCHEME>(c, segs, t0, s0), c.factor);
    }
}

// The other levels at 16 bits.  One record ahead instead of INFLIGHT: a resampled event is sixteen dependent-address loads and some forty
// instructions per sample, which is what there is to hide behind.  e < e1: behind the last event idx holds nothing.
template <int LEVEL, int SCHEME, typename Acc>
__device__ __forceinline__ void seq_walk_16(const typename SeqRec<LEVEL>::type* __restrict__ ev, const she::Seg* __restrict__ segs,
                                            const uint32_t* __restrict__ idx, uint32_t& e, const uint32_t e1, uint32_t t0, uint32_t s0, Acc& acc) {
    typedef typename SeqRec<LEVEL>::type Rec;
    if constexpr (LEVEL >= LOOP) {
        // LOOP is where the scalar registers run out: with a whole record held ahead the allocator spilled (read in the ISA).  The INDEX
        // of the next record is held ahead instead, so one scalar load of the two is still hidden.
        uint32_t ni = idx[e];
        while (e < e1) {
            const Rec c = ev[ni];
            if (++e < e1) ni = idx[e];
            seq_fold8(acc, seq_event8<LEVEL, SCHEME>(c, segs, t0, s0), c.factor);
        }
    } else {
        Rec nx = ev[idx[e]];
        while (e < e1) {
            const Rec c = nx;
            if (++e < e1) nx = ev[idx[e]];
            seq_fold8(acc, seq_event8<LEVEL, SCHEME>(c, segs, t0, s0), c.factor);
        }
    }
}

// Every level at widths 1, 3 and 4: the reference's loop as it stands, event by event.  [e, e1) may be empty.
template <int LEVEL, int WIDTH, typename Acc>
__device__ __forceinline__ void seq_walk_w(const typename SeqRec<LEVEL>::type* __restrict__ ev, const she::Seg* __restrict__ segs,
                                           const uint32_t* __restrict__ idx, uint32_t& e, const uint32_t e1, uint32_t t0, uint32_t s0, Acc& acc) {
    for (; e < e1; ++e) {
        const typename SeqRec<LEVEL>::type c = ev[idx[e]];
        if constexpr (LEVEL == PLAIN) {                        // fetched inside the fold, sample by sample, by chain_get on the generic pointer
            const unsigned char* src = (const unsigned char*)c.src;
            seq_fold_w<WIDTH>(acc, c.factor, s0, c.dst, c.n, [&](int, long long rel) { return chain_get<WIDTH>(src, (size_t)rel); });
        } else {
            int v[4];
            seq_event<LEVEL, WIDTH, FUNNEL>(c, segs, t0, s0, v);
            seq_fold_w<WIDTH>(acc, c.factor, s0, c.dst, c.n, [&](int j, long long) { return (long long)v[j]; });
        }
    }
}

// ---- the tile-list kernels (sh_mix_events*): workgroup k folds active tile tiles[k] into the track ------------------------------------------
// PLAIN at 16 bits
template <int SCHEME, int INFLIGHT>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_seq_plain16(const SeqEv* __restrict__ ev, const she::Seg* __restrict__ segs,
                                                                   const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ first,
                                                                   const uint32_t* __restrict__ idx, uint32_t ntiles, short* track,
                                                                   uint32_t track_samples, int aligned) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t t0 = tiles[k] * shq::TILE_I16, s0 = t0 + threadIdx.x * shq::LANE_SAMPLES_I16;
    if (s0 >= track_samples) return;
    const bool whole = aligned && s0 + 8 <= track_samples;
    short8v acc = seq_track_load8(track, s0, track_samples, whole);
    uint32_t e = first[k];
    seq_walk_plain16<SCHEME, INFLIGHT>(ev, segs, idx, e, first[k + 1], t0, s0, acc);
    seq_track_store8(track, s0, track_samples, whole, acc);
}

// RATE to CHAN at 16 bits: the same tile, lane and fold
template <int LEVEL, int SCHEME>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_seq_16(const typename SeqRec<LEVEL>::type* __restrict__ ev, const she::Seg* __restrict__ segs,
                                                              const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ first,
                                                              const uint32_t* __restrict__ idx, uint32_t ntiles, short* track,
                                                              uint32_t track_samples, int aligned) {
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t t0 = tiles[k] * shq::TILE_I16, s0 = t0 + threadIdx.x * shq::LANE_SAMPLES_I16;
    if (s0 >= track_samples) return;
    const bool whole = aligned && s0 + 8 <= track_samples;
    short8v acc = seq_track_load8(track, s0, track_samples, whole);
    uint32_t e = first[k];
    seq_walk_16<LEVEL, SCHEME>(ev, segs, idx, e, first[k + 1], t0, s0, acc);      // (an active tile lists at least one event)
    seq_track_store8(track, s0, track_samples, whole, acc);
}

// Every level at widths 1, 3 and 4.  An envelope has widths 1, 2 and 4 (upstream's fades have no 24-bit form).
template <int LEVEL, int WIDTH>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_seq_w(const typename SeqRec<LEVEL>::type* __restrict__ ev, const she::Seg* __restrict__ segs,
                                                             const uint32_t* __restrict__ tiles, const uint32_t* __restrict__ first,
                                                             const uint32_t* __restrict__ idx, uint32_t ntiles, unsigned char* track,
                                                             uint32_t track_samples) {
    static_assert(LEVEL != ENV || WIDTH == 1 || WIDTH == 4, "an envelope has widths 1, 2 and 4");
    const uint32_t k = (uint32_t)sh::block_id();
    if (k >= ntiles) return;
    const uint32_t t0 = tiles[k] * shq::TILE_W, s0 = t0 + threadIdx.x * shq::LANE_SAMPLES_W;
    if (s0 >= track_samples) return;
    llong4v acc;
    seq_track_load_w<WIDTH>(track, s0, track_samples, acc);
    uint32_t e = first[k];
    seq_walk_w<LEVEL, WIDTH>(ev, segs, idx, e, first[k + 1], t0, s0, acc);
    seq_track_store_w<WIDTH>(track, s0, track_samples, acc);
}

// ---- a window of a kept song (sh_seq_render) -------------------------------------------------------------------------------------------
// The three templates again for a list that is resident (sh_seq, below): the records, the segments and plan_by_tile's index -- EVERY tile
// of the song in song order -- were uploaded once, and a render of song samples [lo, hi) is one launch that copies nothing.  Workgroup k
// folds song tile lo / TILE + k -- or, where the window is the whole song, tile order[k] of the handle's heaviest-first permutation (the
// order of shq::plan: measured, profiles/sequence_plan_ab.txt); either way t0 and s0 stay SONG coordinates, so the resident index is used as it is, seq_event sees what it sees in
// the kernels above, and the steps that count parity (tostereo, balance, downmix) count the song's samples whatever sample the window
// starts on.  The fold starts from silence -- no load of a base -- and the lane stores to out + s0, `out` being the caller's buffer biased
// by (out_sample - first_sample) samples on the host.  A lane wholly inside the window stores one 16-byte vector where the host found the
// biased base on a 16-byte boundary; a lane on the window's edge, or any lane of a misaligned window, stores sample by sample inside
// [lo, hi) alone; a lane outside the window exits.  A tile that no event touches has an empty index range and stores zeros: every sample
// of the window is written, so the caller's buffer needs no memset.
// `out` is the BIASED base: an address formed with integers on the host, which may lie outside the caller's buffer (below it, even wrapped,
// when first_sample > out_sample).  It means something only as out + s for s in [lo, hi): nothing may be read or written through it
// elsewhere, and it carries no __restrict__ and no bounds of its own.
__device__ __forceinline__ void seq_window_store8(short* out, uint32_t s0, uint32_t lo, uint32_t hi, bool whole, const short8v acc) {
    if (whole) *reinterpret_cast<short8v*>(out + s0) = acc;
    else {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j)
            if (s0 + j >= lo && s0 + j < hi) out[s0 + j] = acc[j];
    }
}

template <int WIDTH>
__device__ __forceinline__ void seq_window_store_w(unsigned char* out, uint32_t s0, uint32_t lo, uint32_t hi, const llong4v& acc) {
    unsigned char* p = out + (size_t)WIDTH * s0;             // (the biased base, as seq_window_store8's: valid at samples [lo, hi) alone)
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (s0 + j >= lo && s0 + j < hi) chain_put<WIDTH>(p, j, acc[j]);
}

// the song tile of workgroup k of a window that starts at sample lo, or false: a workgroup beyond the window (a grid folded into two
// dimensions has some)
// order: NULL, or -- a window that is the whole song (lo == 0, hi the song's length) -- the song's tiles heaviest first, as shq::plan has
// them: workgroup k folds tile order[k], so that a pile-up is not the last workgroup to start.
template <int WIDTH>
__device__ __forceinline__ bool seq_window_tile(const uint32_t* __restrict__ order, uint32_t lo, uint32_t hi, uint32_t& tile, uint32_t& t0, uint32_t& s0) {
    uint64_t t = (uint64_t)(lo / SEQ_TILE<WIDTH>) + sh::block_id();
    if (t * SEQ_TILE<WIDTH> >= hi) return false;              // (uniform; the whole song: workgroup k of ceil(hi / TILE))
    if (order) t = order[t];                                  // (uniform)
    tile = (uint32_t)t;
    t0 = tile * SEQ_TILE<WIDTH>;
    s0 = t0 + threadIdx.x * SEQ_LANE<WIDTH>;
    return true;
}

// and false as well for a lane none of whose samples lie in [lo, hi)
template <int WIDTH>
__device__ __forceinline__ bool seq_window_lane(const uint32_t* __restrict__ order, uint32_t lo, uint32_t hi, uint32_t& tile, uint32_t& t0, uint32_t& s0) {
    return seq_window_tile<WIDTH>(order, lo, hi, tile, t0, s0) && s0 < hi && s0 + SEQ_LANE<WIDTH> > lo;       // (no wrap: MAX_TRACK_SAMPLES)
}

// ---- a song made of tracks (sh_seq_create_tracks, sh_seq_render_gains): BUS = true ------------------------------------------------------
// The reference chain is NOT the flat list: every track is folded on its own from silence (saturating at every event), scaled by a gain
// given at RENDER time (audioop.mul: clamp, then floor; exactly 1.0: none; exactly 0.0: the track's events are not even read, since
// fbound(x * 0.0) is 0 and adding 0 is the identity) and added, saturating, into the master in track order.  A bus lane keeps two
// accumulators: acc, the master, and sub, the current track.  Its tile's slice of idx is cut into RUNS (shq::plan_runs): one per track
// with events there, in track order, so the lane folds [e, run.end) into sub with the schedule of the kernel it mirrors and then sub into
// acc -- which is seq_fold8 / seq_mul_add_w's own mul and add again, one level up (seq_runs).  The gains come BY VALUE in the kernel
// arguments, read at a wave-uniform index by scalar loads from the kernel-argument segment (read in the ISA: no scratch): a render
// uploads nothing.
struct SeqGains { double g[shq::MAX_TRACKS]; };
struct SeqBus {
    const uint32_t* rfirst;               // ntiles + 1 offsets into runs
    const shq::Run* runs;
    SeqGains        gains;
};
// The window templates take the bus as a trailing parameter PACK -- empty for BUS = false, whose kernels so keep the argument list, the
// kernel-argument offsets and the instructions they had; one SeqBusOf<F> for BUS = true.
static_assert(sizeof(shq::Run) == 8 && sizeof(SeqGains) == 256, "a run is one 8-byte scalar load, the gains 256 bytes of kernel arguments");

// The METERS' part (shb::METERS; sh_seq_render_meters -- what the kernels do with it stands in front of seq_meter_begin): 16 bytes of
// kernel arguments behind the bus.
struct SeqMeters {
    shmt::Row* meters;                     // ntracks + 1 rows, zeroed on the stream in front of the launch; row ntracks: the master
    uint32_t  ntracks, nch;               // nch: the song's channels (2: sample s is channel s & 1; otherwise all are channel 0)
};

// The DESK (shb::DESK; sh_seq_render_desk): a pan pot per track and a master fader on either bus, by value in the kernel arguments as the gains
// are and read at wave-uniform indices as they are -- 520 more bytes of arguments, nothing uploaded.  pan[2 t] and pan[2 t + 1]: what
// Sample.stereo(left, right) of a STEREO sample takes, applied to track t's sub-mix BEHIND its gain (two roundings, not one product):
// even samples fbound(x * left), odd ones fbound(x * right); a factor of exactly 1.0: none; both exactly 0.0: the track's events are
// not read, as at a gain of 0.0.  master: audioop.mul of the saturated master, once, behind the last track; exactly 1.0: none.
struct SeqDesk {
    double pan[2 * shq::MAX_TRACKS];
    double master;
};

// AUTOMATION (shb::AUTO; sh_seq_render_auto): fader moves per track on a desk bus -- a table a handle of its own keeps on the device
// (sh_seq_auto), its two pointers by value in the kernel arguments: a render uploads nothing.  Track t's segments are
// asegs[afirst[t] .. afirst[t + 1]) (she::Seg in SONG samples, the ends ascending, plain segments in the gaps), applied to the track's
// sub-mix BEHIND its gain and IN FRONT of its pan: sample s of a segment becomes int(x * ((s - origin) * slope / numsamples + offset)),
// she::gain's fade-in, truncated toward zero.  Per run the first segment that ends past the tile's first sample is found by binary search
// (sha::find: uniform, scalar loads), and the lane's samples are shaped from there on (sha::shape_from).  Widths 1, 2 and 4: upstream's
// fades have no 24-bit form.
struct SeqAuto {
    const she::Seg* asegs;
    const uint32_t* afirst;               // ntracks + 1 offsets into asegs
};

// GROUP BUSES (shb::GROUPS; sh_seq_render_groups): runs of consecutive tracks mixed into a bus of their own between the track and the master -- the
// table of seqgroup.hpp by value in the kernel arguments, 232 more bytes, read at wave-uniform indices as the gains are; a render still
// uploads nothing.  A bus lane keeps a THIRD accumulator, grp, between sub and acc: a track of a group is added, saturating, into grp
// and not into acc; where the next run's track belongs to another group or to none, and behind the last run, the open group is CLOSED:
// grp by the group's gain (audioop.mul, one rounding over the saturated sum), by its pan factors, the hook for its meter row, the
// saturating add into acc -- seq_scale8 / seq_pan8 / seq_scale_w / seq_mul_add_w one level up.  The runs of a tile come in track
// order, so a group enters the master where its last track stands; tracks without a run in the tile add zeros, and a group without one
// never opens (fbound(0 * g) == 0).  A group at gain 0.0 or pan (0.0, 0.0) skips its tracks' events as a muted track does.  These
// buses carry the WHOLE desk so that the kernel count does not double: at widths 1, 2 and 4 the automation's two pointers as well,
// NULL meaning no moves (a uniform branch); width 3, which has no automation, goes without them (shb::valid_at).
struct SeqGroups { shg::Table groups; };

// BUS RIDES (shb::RIDES; sh_seq_auto_create_buses): fader moves on the two bus levels -- a group's bus shaped through a lane of its own BEHIND the
// group's gain and IN FRONT of its pan, the master through one BEHIND the master's gain, over the saturated sum in both places.  No new
// kernel argument: the lanes stand in the automation's table in the meter table's row order (seqauto.hpp), the master's at
// groups.row0 - 1 and group g's at groups.row0 + g, behind the tracks', and index the afirst / asegs that a group bus carries anyway.
// The table of such a handle always has an offset for every one of the MAX_GROUPS group lanes, so a render may name more groups than
// the handle rides.  A bit and nothing else, on the group buses of widths 1, 2 and 4, with and without meters; a handle without a segment
// on a bus lane never gets here (shb::route).

// PAN RIDES (shb::PANS; sh_seq_auto_create_pans): pan moves of a track and of a group's bus, Sample.pan(lfo=...)'s expression per frame (seqpan.hpp),
// where a pan lane has a move; elsewhere the static factors as ever.  No new kernel argument either: the pan lanes stand in the same
// table behind the fader lanes' offsets -- track t's at shp::track_lane(row0, t), group g's at shp::group_lane(row0, g) -- and their
// segments behind the fader lanes' segments.  A bit and nothing else, on top of the buses that ride; a handle without a pan move never
// gets here.

// The STEMS (shb::STEMS; sh_seq_render_stems; seqstem.hpp): the group buses, the buses that ride and the buses that pan again -- the whole desk,
// NULL pointers meaning no moves, the empty table no groups -- whose lanes STORE every bus where a metering bus reduces it: track t's
// samples as seq_runs' hook receives them into plane t, a group's into plane groups.row0 + g, the master's into plane groups.row0 - 1,
// plane r standing r * stride BYTES behind plane 0 (64-bit).  A part that carries the stride -- the one new kernel argument -- on the
// group bus, the bus that rides and the bus that pans (widths 1, 2 and 4: a table without bus lanes or without pan lanes must not reach a
// kernel that reads them) and on width 3's group bus.  They are NOT metering buses: no table, no barrier, lanes outside the window leave.
struct SeqStems { uint64_t stride; };

// ONE bus type for every set of features F (seqbus.hpp): the plain bus, then the parts F has in this one order -- the layout of the
// kernel arguments.  A part F lacks is an empty base of a type of its own, which takes no room, so the parts behind it stand where they
// stood; RIDES, PANS, HISTORY and CLIPS are bits and nothing else.  SEQ_DESK ... SEQ_CLIPS read the bits (an empty pack: none).
template <uint32_t BIT> struct SeqNoPart {};
template <uint32_t F, uint32_t BIT, typename Part> using SeqPart = typename std::conditional<(F & BIT) != 0, Part, SeqNoPart<BIT>>::type;
template <uint32_t F>
struct SeqBusOf : SeqBus, SeqPart<F, shb::METERS, SeqMeters>, SeqPart<F, shb::DESK, SeqDesk>, SeqPart<F, shb::AUTO, SeqAuto>,
                  SeqPart<F, shb::GROUPS, SeqGroups>, SeqPart<F, shb::STEMS, SeqStems> {
    static constexpr uint32_t FEATURES = F;
};
template <typename... Bus> constexpr uint32_t SEQ_MASK = (0u | ... | Bus::FEATURES);
template <typename... Bus> constexpr bool SEQ_METERS = (SEQ_MASK<Bus...> & shb::METERS) != 0;
template <typename... Bus> constexpr bool SEQ_DESK = (SEQ_MASK<Bus...> & shb::DESK) != 0;
template <typename... Bus> constexpr bool SEQ_AUTO = (SEQ_MASK<Bus...> & shb::AUTO) != 0;
template <typename... Bus> constexpr bool SEQ_GROUPS = (SEQ_MASK<Bus...> & shb::GROUPS) != 0;
template <typename... Bus> constexpr bool SEQ_RIDES = (SEQ_MASK<Bus...> & shb::RIDES) != 0;
template <typename... Bus> constexpr bool SEQ_PANS = (SEQ_MASK<Bus...> & shb::PANS) != 0;
template <typename... Bus> constexpr bool SEQ_HISTORY = (SEQ_MASK<Bus...> & shb::HISTORY) != 0;
template <typename... Bus> constexpr bool SEQ_CLIPS = (SEQ_MASK<Bus...> & shb::CLIPS) != 0;
template <typename... Bus> constexpr bool SEQ_STEMS = (SEQ_MASK<Bus...> & shb::STEMS) != 0;
// every route's kernel arguments: the 272 bytes of the plain bus, then the parts it has -- the meters' 16, the desk's 520, the automation's 16,
// the groups' 232, the stems' 8 -- each behind the one before it and nothing between them; rides, pan rides, a history and overs add none
constexpr size_t seq_bus_bytes(uint32_t f) {
    return 272 + (f & shb::METERS ? 16 : 0) + (f & shb::DESK ? 520 : 0) + (f & shb::AUTO ? 16 : 0) + (f & shb::GROUPS ? 232 : 0) + (f & shb::STEMS ? 8 : 0);
}
template <uint32_t... I> constexpr bool seq_bus_layouts(std::integer_sequence<uint32_t, I...>) { return ((sizeof(SeqBusOf<shb::ROUTES[I]>) == seq_bus_bytes(shb::ROUTES[I])) && ...); }
static_assert(seq_bus_layouts(std::make_integer_sequence<uint32_t, shb::NROUTES>()) && sizeof(SeqBus) == 272 && sizeof(SeqMeters) == 16 && sizeof(SeqDesk) == 520 &&
              sizeof(SeqAuto) == 16 && sizeof(SeqGroups) == 232 && sizeof(SeqStems) == 8, "every bus is its parts, in the one order, and nothing else");
static_assert(shg::MAX_TRACKS == shq::MAX_TRACKS && sha::MAX_GROUP_LANES == shg::MAX_GROUPS && SH_ENV_PAN == shp::PAN &&
              shst::MAX_ROWS == shq::MAX_TRACKS + 1 + shg::MAX_GROUPS && shst::MAX_ROWS <= 64, "the lanes of the rides; the stems: a bit of one 64-bit mask per plane");

// a lane's accumulator: eight packed samples at 16 bits, four 64-bit sums at the other widths
template <int WIDTH> struct SeqAcc { typedef llong4v type; };
template <> struct SeqAcc<2> { typedef short8v type; };

// a track's pan step and the master's gain on a lane's samples: seq_scale8's arithmetic at 16 bits, seq_mul_add_w's at widths 1, 3, 4.
// Lanes start on even song samples, so sample j of a lane is a left one where j is even, whatever sample the window starts on.
__device__ __forceinline__ short8v seq_pan8(short8v x, const double left, const double right) {
    if (left != 1.0) {                                        // (uniform)
#pragma unroll
        for (int j = 0; j < 8; j += 2) x[j] = (short)fbound((double)x[j] * left, Lim<short>::lo, Lim<short>::hi);
    }
    if (right != 1.0) {
#pragma unroll
        for (int j = 1; j < 8; j += 2) x[j] = (short)fbound((double)x[j] * right, Lim<short>::lo, Lim<short>::hi);
    }
    return x;
}

// counting: floor(p) against the range in front of fbound, then seq_pan8's bytes
__device__ __forceinline__ SeqAccC8 seq_pan8(SeqAccC8 a, const double left, const double right) {
    if (left != 1.0) {                                        // (uniform)
#pragma unroll
        for (int j = 0; j < 8; j += 2)
            if (shcl::mul_clamps<2>((double)a.v[j] * left)) a.over[j] = (short)-1;
    }
    if (right != 1.0) {
#pragma unroll
        for (int j = 1; j < 8; j += 2)
            if (shcl::mul_clamps<2>((double)a.v[j] * right)) a.over[j] = (short)-1;
    }
    a.v = seq_pan8(a.v, left, right);
    return a;
}

template <int WIDTH>
__device__ __forceinline__ long long seq_scale_w(const long long x, const double factor) {
    return factor != 1.0 ? (long long)fbound((double)x * factor, (double)SEQ_LO<WIDTH>, (double)SEQ_HI<WIDTH>) : x;
}

// sample j of a bus by its gain: seq_scale_w's value; counting: whether it clamped, into the bus's flag
template <int WIDTH>
__device__ __forceinline__ long long seq_gain_w(const llong4v& a, const int j, const double gain) { return seq_scale_w<WIDTH>(a[j], gain); }
template <int WIDTH>
__device__ __forceinline__ long long seq_gain_w(SeqAccCW& a, const int j, const double gain) {
    if (gain != 1.0 && shcl::mul_clamps<WIDTH>((double)a.v[j] * gain)) a.over |= 1u << j;
    return seq_scale_w<WIDTH>(a.v[j], gain);
}

template <int WIDTH>
__device__ __forceinline__ void seq_master(typename SeqAcc<WIDTH>::type& acc, const double gain) {
    if constexpr (WIDTH == 2) {
        acc = seq_scale8(acc, gain);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = seq_scale_w<WIDTH>(acc[j], gain);
    }
}
template <int WIDTH>
__device__ __forceinline__ void seq_master(SeqAccC8& acc, const double gain) { acc = seq_scale8(acc, gain); }
template <int WIDTH>
__device__ __forceinline__ void seq_master(SeqAccCW& acc, const double gain) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc.v[j] = seq_gain_w<WIDTH>(acc, j, gain);
}

// "Shape this accumulator through lane `lane` of the automation's table", stated once for the buses that ride (shb::RIDES) -- a
// track's sub-mix, a group's bus and the master: a lane's samples of tile k at their SONG positions, one binary search at the tile's first
// sample (sha::find) and one walk from there (sha::shape_from); everything but x and the lane's position is wave-uniform, and behind the
// lane's last segment nothing is shaped.  x holds saturated samples of the width, so they pass through int unchanged.
template <int WIDTH>
__device__ __forceinline__ void seq_ride(typename SeqAcc<WIDTH>::type& x, const SeqAuto& au, const uint32_t lane, const uint32_t k) {
    constexpr int N = SEQ_LANE<WIDTH>;
    const uint32_t t0 = k * SEQ_TILE<WIDTH>;
    const uint32_t a0 = au.afirst[lane];
    const she::Seg* segs = au.asegs + a0;
    const uint32_t n = au.afirst[lane + 1] - a0;
    const uint32_t i = sha::find(segs, n, t0);
    if (i >= n) return;                                       // (uniform)
    int v[N];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (int)x[j];
    sha::shape_from<N>(segs, n, i, t0, t0 + SEQ_TILE<WIDTH>, (long long)t0 + threadIdx.x * N, v, (double)SEQ_LO<WIDTH>, (double)SEQ_HI<WIDTH>);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if constexpr (WIDTH == 2) x[j] = (short)v[j];
        else x[j] = v[j];
    }
}

// "Pass this accumulator through pan lane `lane` of the automation's table", stated once for the buses that pan (shb::PANS) -- a
// track's sub-mix and a group's bus, where their static pan stands: one binary search at the tile's first sample, then one of
// shp::shape_from's uniform paths.  false: no move reaches into the tile and NOTHING was done -- the caller applies the static factors
// with the code it always had (seq_pan8, seq_mul_add_w); true: x is panned, by the move where one holds the frame and by left / right
// where none does.
template <int WIDTH>
__device__ __forceinline__ bool seq_pan_ride(typename SeqAcc<WIDTH>::type& x, const SeqAuto& au, const uint32_t lane, const uint32_t k, const double left,
                                             const double right) {
    constexpr int N = SEQ_LANE<WIDTH>;
    const uint32_t t0 = k * SEQ_TILE<WIDTH>;
    const uint32_t a0 = au.afirst[lane];
    const she::Seg* segs = au.asegs + a0;
    const uint32_t n = au.afirst[lane + 1] - a0;
    const uint32_t i = sha::find(segs, n, t0);
    if (shp::plain(segs, n, i, t0 + SEQ_TILE<WIDTH>)) return false;      // (uniform)
    int v[N];
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = (int)x[j];
    shp::shape_from<N>(segs, n, i, t0, t0 + SEQ_TILE<WIDTH>, (long long)t0 + threadIdx.x * N, v, left, right, (double)SEQ_LO<WIDTH>, (double)SEQ_HI<WIDTH>);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if constexpr (WIDTH == 2) x[j] = (short)v[j];
        else x[j] = v[j];
    }
    return true;
}

// The runs of tile k, written once for the three templates and every bus: the events from e on, run by run.  walk(e, e1, sub): the
// schedule of the kernel, events [e, e1) into sub; hook(sub, row): what else a bus does with a track's samples as its bus takes them,
// post-fader and (a desk bus) post-pan (the metering buses: its row).  Everything about a run is uniform, and a run lists at least one event.
// An automation bus: the track's fader moves between the gain and the pan, at the lane's SONG positions (tile k starts at k * TILE).
// A group bus: a track of a group goes into grp, the open group's bus, and a group is closed -- its gain, its pan, hook(grp, its row),
// into acc -- in front of the first run that is not of it and behind the last run; opening and closing are uniform.
// Acc: the accumulator's type, the same for sub, grp and acc -- a lane's samples, or (a bus that counts overs) a counting accumulator,
// whose flags each bus carries through its own steps and the hook receives next to the samples.
template <int WIDTH, typename Bus, typename Acc, typename Walk, typename Hook>
__device__ __forceinline__ void seq_runs(const Bus& bus, uint32_t k, uint32_t e, Acc& acc, Walk walk, Hook hook) {
    [[maybe_unused]] Acc grp = {};                            // (a group bus: the open group's samples)
    [[maybe_unused]] uint32_t open = shg::NONE, of = shg::NONE;
    [[maybe_unused]] auto close = [&] {                       // the open group into the master
        if constexpr (SEQ_GROUPS<Bus>) {
            const double gg = bus.groups.gain[open], gl = bus.groups.pan[2 * open], gr = bus.groups.pan[2 * open + 1];
            if constexpr (SEQ_PANS<Bus> && WIDTH == 2) {      // the group's pan ride: where its static pan stands
                grp = seq_scale8(grp, gg);
                seq_ride<2>(grp, bus, sha::group_lane(bus.groups.row0, open), k);
                if (!seq_pan_ride<2>(grp, bus, shp::group_lane(bus.groups.row0, open), k, gl, gr)) grp = seq_pan8(grp, gl, gr);
                hook(grp, bus.groups.row0 + open);
                acc = __builtin_elementwise_add_sat(acc, grp);
            } else if constexpr (SEQ_PANS<Bus>) {
#pragma unroll
                for (int j = 0; j < 4; ++j) grp[j] = seq_scale_w<WIDTH>(grp[j], gg);
                seq_ride<WIDTH>(grp, bus, sha::group_lane(bus.groups.row0, open), k);
                const bool rode = seq_pan_ride<WIDTH>(grp, bus, shp::group_lane(bus.groups.row0, open), k, gl, gr);      // (uniform)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    long long x = grp[j];
                    acc[j] = seq_mul_add_w<WIDTH>(acc[j], x, rode ? 1.0 : (j & 1 ? gr : gl));
                    grp[j] = x;
                }
                hook(grp, bus.groups.row0 + open);
            } else if constexpr (SEQ_RIDES<Bus> && WIDTH == 2) {     // the group's ride: behind its gain, in front of its pan
                grp = seq_scale8(grp, gg);
                seq_ride<2>(grp, bus, sha::group_lane(bus.groups.row0, open), k);
                grp = seq_pan8(grp, gl, gr);
                hook(grp, bus.groups.row0 + open);
                acc = __builtin_elementwise_add_sat(acc, grp);
            } else if constexpr (SEQ_RIDES<Bus>) {
#pragma unroll
                for (int j = 0; j < 4; ++j) grp[j] = seq_scale_w<WIDTH>(grp[j], gg);
                seq_ride<WIDTH>(grp, bus, sha::group_lane(bus.groups.row0, open), k);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    long long x = grp[j];
                    acc[j] = seq_mul_add_w<WIDTH>(acc[j], x, j & 1 ? gr : gl);
                    grp[j] = x;
                }
                hook(grp, bus.groups.row0 + open);
            } else if constexpr (WIDTH == 2) {
                grp = seq_pan8(seq_scale8(grp, gg), gl, gr);
                hook(grp, bus.groups.row0 + open);
                seq_add8(acc, grp);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    long long x = seq_gain_w<WIDTH>(grp, j, gg);
                    seq_into_w<WIDTH>(acc, j, grp, x, j & 1 ? gr : gl);
                    seq_v(grp)[j] = x;
                }
                hook(grp, bus.groups.row0 + open);
            }
            open = shg::NONE;
        }
    };
    const uint32_t r1 = bus.rfirst[k + 1];
    for (uint32_t r = bus.rfirst[k]; r < r1; ++r) {
        const shq::Run run = bus.runs[r];
        const double g = bus.gains.g[run.track];
        double left = 1.0, right = 1.0;
        bool silent = g == 0.0;
        if constexpr (SEQ_DESK<Bus>) {
            left = bus.pan[2 * run.track];
            right = bus.pan[2 * run.track + 1];
            silent = silent || (left == 0.0 && right == 0.0);
        }
        if constexpr (SEQ_GROUPS<Bus>) {
            of = shg::group_of(bus.groups, run.track);
            if (open != shg::NONE && of != open) close();
            if (of != shg::NONE)
                silent = silent || bus.groups.gain[of] == 0.0 || (bus.groups.pan[2 * of] == 0.0 && bus.groups.pan[2 * of + 1] == 0.0);
        }
        if (silent) {
            e = run.end;
            continue;
        }
        if constexpr (SEQ_GROUPS<Bus>) {
            if (of != shg::NONE && open == shg::NONE) {       // the group opens: from silence
                grp = Acc{};
                open = of;
            }
        }
        [[maybe_unused]] const she::Seg* asegs = nullptr;    // (an automation bus: the track's segments, from the first that ends past t0)
        [[maybe_unused]] uint32_t an = 0, ai = 0;
        [[maybe_unused]] const uint32_t t0 = k * SEQ_TILE<WIDTH>;
        if constexpr (SEQ_AUTO<Bus> && !SEQ_RIDES<Bus>) {       // (a bus that rides searches in seq_ride)
            bool moves = true;
            if constexpr (SEQ_GROUPS<Bus>) moves = bus.asegs != nullptr;      // (uniform: a group bus without automation)
            if (moves) {
                const uint32_t a0 = bus.afirst[run.track];
                asegs = bus.asegs + a0;
                an = bus.afirst[run.track + 1] - a0;
                ai = sha::find(asegs, an, t0);
            }
        }
        if constexpr (WIDTH == 2) {
            Acc sub = {};
            walk(e, run.end, sub);
            sub = seq_scale8(sub, g);                         // post-fader: what the master takes of the track
            if constexpr (SEQ_RIDES<Bus>) {
                seq_ride<2>(sub, bus, run.track, k);
            } else if constexpr (SEQ_AUTO<Bus>) {
                if (ai < an) {                                // (uniform: behind the track's last segment nothing is shaped)
                    int v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = (int)seq_v(sub)[j];
                    sha::shape_from<8>(asegs, an, ai, t0, t0 + SEQ_TILE<2>, (long long)t0 + threadIdx.x * SEQ_LANE<2>, v, (double)SEQ_LO<2>, (double)SEQ_HI<2>);
#pragma unroll
                    for (int j = 0; j < 8; ++j) seq_v(sub)[j] = (short)v[j];
                }
            }
            if constexpr (SEQ_PANS<Bus>) {                    // the track's pan ride: where its static pan stands
                if (!seq_pan_ride<2>(sub, bus, shp::track_lane(bus.groups.row0, run.track), k, left, right)) sub = seq_pan8(sub, left, right);
            } else if constexpr (SEQ_DESK<Bus>) sub = seq_pan8(sub, left, right);
            hook(sub, run.track);
            bool grouped = false;
            if constexpr (SEQ_GROUPS<Bus>) grouped = of != shg::NONE;
            if (grouped) seq_add8(grp, sub);
            else seq_add8(acc, sub);
        } else {
            Acc sub = {};
            walk(e, run.end, sub);
            if constexpr (SEQ_RIDES<Bus>) {
#pragma unroll
                for (int j = 0; j < 4; ++j) sub[j] = seq_scale_w<WIDTH>(sub[j], g);
                seq_ride<WIDTH>(sub, bus, run.track, k);
                if constexpr (SEQ_PANS<Bus>) {                // the track's pan ride; a tile it panned takes no static factor below
                    if (seq_pan_ride<WIDTH>(sub, bus, shp::track_lane(bus.groups.row0, run.track), k, left, right)) left = right = 1.0;
                }
            } else if constexpr (SEQ_AUTO<Bus>) {             // the gain over all four first, then the segments; the pan below
                int v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (int)seq_gain_w<WIDTH>(sub, j, g);
                sha::shape_from<4>(asegs, an, ai, t0, t0 + SEQ_TILE<WIDTH>, (long long)t0 + threadIdx.x * SEQ_LANE<WIDTH>, v, (double)SEQ_LO<WIDTH>,
                                   (double)SEQ_HI<WIDTH>);
#pragma unroll
                for (int j = 0; j < 4; ++j) seq_v(sub)[j] = v[j];
            }
            if constexpr (SEQ_GROUPS<Bus>) {                  // (the desk's steps into the bus that takes the track: whole values, uniform)
                Acc into = of != shg::NONE ? grp : acc;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    long long x = seq_v(sub)[j];
                    if constexpr (!SEQ_AUTO<Bus>) x = seq_gain_w<WIDTH>(sub, j, g);
                    seq_into_w<WIDTH>(into, j, sub, x, j & 1 ? right : left);
                    seq_v(sub)[j] = x;
                }
                if (of != shg::NONE) grp = into;
                else acc = into;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    long long x = sub[j];
                    if constexpr (SEQ_AUTO<Bus>) {            // (scaled and shaped above)
                        acc[j] = seq_mul_add_w<WIDTH>(acc[j], x, j & 1 ? right : left);
                    } else if constexpr (SEQ_DESK<Bus>) {     // the gain, then the pan: two roundings
                        x = seq_scale_w<WIDTH>(x, g);
                        acc[j] = seq_mul_add_w<WIDTH>(acc[j], x, j & 1 ? right : left);
                    } else {
                        acc[j] = seq_mul_add_w<WIDTH>(acc[j], x, g);
                    }
                    sub[j] = x;
                }
            }
            hook(sub, run.track);
        }
    }
    if constexpr (SEQ_GROUPS<Bus>) {
        if (open != shg::NONE) close();                       // (uniform)
    }
}

// ---- level meters from the same launch (sh_seq_render_meters): the buses with shb::METERS ---------------------------------------------
// A metered render stores the bytes of the render with gains and, from the values the lane holds anyway, one row of levels (seqmeter.hpp:
// per channel the peak and the exact sum of squares) per track, post-fader -- over mul(sub, gain), formed just before it is added into
// acc -- and one for the master, over acc at the store; only samples inside [lo, hi) count.  The reduction (the guide's: partials on chip,
// one atomic per workgroup and value): the lane's partial row; a wave reduction by __shfl_xor; the wave's first lane into a row table in
// LDS (33 rows, 1320 bytes) by LDS atomics -- integer max and add, so the order of arrival changes nothing; behind a barrier, lane
// 2 row + channel of the workgroup adds what its tile found for (row, channel) to the handle's device table: one atomicMax and one or two
// atomicAdd at agent scope, none where the peak is 0.  A barrier needs every lane, so the metering kernels do NOT leave with
// seq_window_lane's lanes outside the window: only a workgroup beyond the window leaves (seq_window_tile, uniform); a WAVE without a lane
// in the window skips the runs (uniform: the shuffles see whole waves), and inside a wave the lanes outside fold their samples like the
// others, count none of them (seqmeter's cut) and store none (seq_window_store8's).  Their fetches are the ones lanes beside an event
// make in any tile: nothing outside an event's samples is read.  A muted track's run is skipped as before: its row stays zero.
// With the desk a track's row is post-fader and post-pan and the master's over the stored bytes; with automation a track's row stands
// behind its fader moves as well.  With groups: ntracks + 1 + ngroups rows -- tracks and the master where they were, group g in row
// ntracks + 1 + g, over what the master takes of it (behind its gain and pan); a track's row stays what its bus takes of it; a table of
// their own size in LDS.  With rides a group's row stands behind its ride and pan and the master's behind its ride; with pan rides a
// track's row behind its pan ride, a group's behind its ride and its pan ride.
// The HISTORY (shb::HISTORY; sh_seq_render_history; seqhist.hpp): the metering group buses again -- the whole desk, NULL pointers meaning no
// moves, the empty table no groups -- whose workgroups KEEP their table instead of merging it: bus.meters points at a table of blocks, one
// per song tile of the window, and the workgroup that folds tile k stores its ntracks + 1 + groups.n rows as block k - lo / TILE.  No new
// kernel argument: the first tile and the row count are in the kernel already.  A bit and nothing else, at widths 1, 2 and 4 and at width
// 3; the buses that ride and pan have none.
// The OVERS (shb::CLIPS; sh_seq_render_clips; seqclip.hpp): a history again whose lanes keep counting accumulators -- sub, grp and acc each
// with a sticky flag per sample, set where one of the bus's own steps clamped -- and whose rows carry, behind the levels, the count of
// flagged samples per channel: a table of 48-byte rows in LDS and in the table of blocks.  A bit and no new kernel argument, at widths 1, 2
// and 4 and at width 3.
// what a window kernel's lane accumulates in: the samples, or with a bus that counts the counting accumulator
template <int WIDTH, typename... Bus> struct SeqWinAcc {
    typedef typename std::conditional<SEQ_CLIPS<Bus...>, typename std::conditional<WIDTH == 2, SeqAccC8, SeqAccCW>::type, typename SeqAcc<WIDTH>::type>::type type;
};

// the workgroup's row table, zeroed: every lane of the workgroup calls it (a barrier).  ROWS: 33, or 41 with the rows of the groups
template <uint32_t ROWS = shq::MAX_TRACKS + 1>
__device__ __forceinline__ shmt::Row* seq_meter_begin() {
    __shared__ shmt::Row table[ROWS];
    uint32_t* w = reinterpret_cast<uint32_t*>(table);
    for (uint32_t i = threadIdx.x; i < sizeof(table) / 4; i += shq::TILE_THREADS) w[i] = 0u;
    __syncthreads();
    return table;
}

// the lanes' partial rows of one WHOLE wave into row `slot` of the workgroup's table (every lane of the wave calls it; WIDE: widths 3, 4)
template <bool WIDE>
__device__ __forceinline__ void seq_meter_wave(shmt::Row r, const bool stereo, shmt::Row* slot) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        shmt::Row o = shmt::zero();
        o.peak[0] = __shfl_xor(r.peak[0], m, 64);
        o.sq_lo[0] = __shfl_xor((unsigned long long)r.sq_lo[0], m, 64);
        if (WIDE) o.sq_hi[0] = __shfl_xor((unsigned long long)r.sq_hi[0], m, 64);
        if (stereo) {                                         // (uniform)
            o.peak[1] = __shfl_xor(r.peak[1], m, 64);
            o.sq_lo[1] = __shfl_xor((unsigned long long)r.sq_lo[1], m, 64);
            if (WIDE) o.sq_hi[1] = __shfl_xor((unsigned long long)r.sq_hi[1], m, 64);
        }
        shmt::fold(r, o);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (r.peak[0]) {                                      // (a peak of 0: every sample 0, both sums 0)
            atomicMax(&slot->peak[0], r.peak[0]);
            atomicAdd(reinterpret_cast<unsigned long long*>(&slot->sq_lo[0]), (unsigned long long)r.sq_lo[0]);
            if (WIDE) atomicAdd(reinterpret_cast<unsigned long long*>(&slot->sq_hi[0]), (unsigned long long)r.sq_hi[0]);
        }
        if (stereo && r.peak[1]) {
            atomicMax(&slot->peak[1], r.peak[1]);
            atomicAdd(reinterpret_cast<unsigned long long*>(&slot->sq_lo[1]), (unsigned long long)r.sq_lo[1]);
            if (WIDE) atomicAdd(reinterpret_cast<unsigned long long*>(&slot->sq_hi[1]), (unsigned long long)r.sq_hi[1]);
        }
    }
}

// the same of a bus that counts: 41 rows of 48 bytes
__device__ __forceinline__ shcl::Row* seq_clip_begin() {
    __shared__ shcl::Row table[shq::MAX_TRACKS + 1 + shg::MAX_GROUPS];
    uint32_t* w = reinterpret_cast<uint32_t*>(table);
    for (uint32_t i = threadIdx.x; i < sizeof(table) / 4; i += shq::TILE_THREADS) w[i] = 0u;
    __syncthreads();
    return table;
}

// the lanes' partial counts of one WHOLE wave into row `slot` of the workgroup's table, beside seq_meter_wave: a wave reduction by
// __shfl_xor, then the wave's first lane by an LDS integer add (none where the count is 0)
__device__ __forceinline__ void seq_clip_wave(shcl::Count c, const bool stereo, shcl::Row* slot) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        shcl::Count o{{0u, 0u}};
        o.c[0] = __shfl_xor(c.c[0], m, 64);
        if (stereo) o.c[1] = __shfl_xor(c.c[1], m, 64);      // (uniform)
        shcl::fold(c, o);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (c.c[0]) atomicAdd(&slot->clipped[0], c.c[0]);
        if (stereo && c.c[1]) atomicAdd(&slot->clipped[1], c.c[1]);
    }
}

// the workgroup's table into the handle's: every lane of the workgroup calls it (a barrier), lane 2 row + channel carries one value each
// (groups: the rows of a group bus behind the master's; 2 * 41 lanes at the most, of TILE_THREADS)
template <bool WIDE>
__device__ __forceinline__ void seq_meter_end(const shmt::Row* table, const SeqMeters& bus, const uint32_t groups = 0) {
    static_assert(2 * (shq::MAX_TRACKS + 1 + shg::MAX_GROUPS) <= shq::TILE_THREADS, "a lane per row and channel");
    __syncthreads();
    const uint32_t row = threadIdx.x >> 1, c = threadIdx.x & 1u;
    if (row > bus.ntracks + groups) return;
    const uint32_t peak = table[row].peak[c];
    if (!peak) return;
    shmt::Row* g = bus.meters + row;
    atomicMax(&g->peak[c], peak);
    atomicAdd(reinterpret_cast<unsigned long long*>(&g->sq_lo[c]), (unsigned long long)table[row].sq_lo[c]);
    if (WIDE) atomicAdd(reinterpret_cast<unsigned long long*>(&g->sq_hi[c]), (unsigned long long)table[row].sq_hi[c]);
}

// the workgroup's table as block `tile - lo / TILE` of the history's: every lane of the workgroup calls it (a barrier), lane 2 row + channel
// STORES its three values of (row, channel), zeros as well -- the block has this one writer, so nothing merges and nothing was zeroed.
// R: the row, shmt::Row or (a bus that counts) shcl::Row, whose count is a fourth value; bus.meters is a table of R.
template <int WIDTH, typename R>
__device__ __forceinline__ void seq_hist_end(const R* table, const SeqMeters& bus, const uint32_t groups, const uint32_t tile, const uint32_t lo) {
    static_assert(2 * (shq::MAX_TRACKS + 1 + shg::MAX_GROUPS) <= shq::TILE_THREADS, "a lane per row and channel");
    __syncthreads();
    const uint32_t row = threadIdx.x >> 1, c = threadIdx.x & 1u, nrows = bus.ntracks + 1 + groups;
    if (row >= nrows) return;
    R* g = reinterpret_cast<R*>(bus.meters) + shhs::row_at(shhs::block_of(tile, lo, SEQ_TILE<WIDTH>), nrows, row);
    g->peak[c] = table[row].peak[c];
    g->sq_hi[c] = table[row].sq_hi[c];
    g->sq_lo[c] = table[row].sq_lo[c];
    if constexpr (std::is_same<R, shcl::Row>::value) g->clipped[c] = table[row].clipped[c];
}

// What a window kernel does where it has a STEMS bus (sh_seq_render_stems; seqstem.hpp), once for the three templates: a lane that
// seq_window_lane kept, as with a plain bus.  put(to, x): the kernel's window store of a lane's samples x at the lane's song position
// through the biased base `to` -- seq_window_store8 / seq_window_store_w with their cut to [lo, hi) and the aligned fast path --, stated
// once per template and used for every plane, the master's too.  seq_runs' hook puts a bus's samples into plane `row` and marks the row
// in a wave-uniform mask; the master, behind its gain and its ride, goes to plane groups.row0 - 1; behind the runs every row that no hook
// stored -- a muted or skipped track, a track or a group without a run in this tile, all of them in an idle tile -- gets the lane's samples
// as zeros, so that every sample of every plane has this one writer and nothing zeroes the planes in front of the launch.
// (A function and a store of their own, beside seq_window_bus and the kernels' store(): giving THAT lambda the destination and the samples
// as parameters changed the register allocation of 25 of the 508 existing kernels, which are held to what they were
// -- profiles/sequence_stems_ab.txt, section 1.)
template <int WIDTH, typename Bus, typename Walk, typename Put, typename Out>
__device__ __forceinline__ void seq_stems_bus(const Bus& bus, uint32_t k, uint32_t e, typename SeqAcc<WIDTH>::type& acc, Walk walk, Put put, Out* out) {
    typedef typename SeqAcc<WIDTH>::type V;
    auto plane = [&](uint32_t row) {                          // (the biased base of plane `row`: valid at samples [lo, hi) alone, as `out` is)
        return reinterpret_cast<Out*>(reinterpret_cast<unsigned char*>(out) + shst::plane_offset(row, bus.stride));
    };
    uint64_t stored = 0;                                      // (uniform: bit `row` set where a hook stored the row in this tile)
    seq_runs<WIDTH>(bus, k, e, acc, walk, [&](const V& x, uint32_t row) {
        put(plane(row), x);
        stored |= 1ull << row;
    });
    seq_master<WIDTH>(acc, bus.master);
    if constexpr (SEQ_RIDES<Bus>) seq_ride<WIDTH>(acc, bus, sha::master_lane(bus.groups.row0), k);      // the master's ride: behind its gain
    const uint32_t master = bus.groups.row0 - 1u, nrows = bus.groups.row0 + bus.groups.n;
    put(plane(master), acc);
    stored |= 1ull << master;
    const V zeros = {};
    for (uint32_t row = 0; row < nrows; ++row)
        if (!((stored >> row) & 1ull)) put(plane(row), zeros);      // (uniform)
}

// What a window kernel does where it has a bus, once for the three templates: the runs of tile k into acc, (a desk bus) the master's gain,
// then store().  A plain bus: a lane that seq_window_lane kept; s0, lo and hi, which only a metering bus needs, are ignored.
// A metering bus: EVERY lane of a workgroup that seq_window_tile kept, the rows of the tracks from seq_runs' hook and the master's row
// in front of the store, the table's barriers around everything.
// A bus that counts overs: acc is a counting accumulator, the table's rows are shcl::Row, and every row takes its bus's flags beside its
// samples -- the master's in front of the store.
template <int WIDTH, typename Bus, typename Acc, typename Walk, typename Store>
__device__ __forceinline__ void seq_window_bus(const Bus& bus, uint32_t k, uint32_t e, uint32_t s0, uint32_t lo, uint32_t hi, Acc& acc, Walk walk,
                                               Store store) {
    if constexpr (!SEQ_METERS<Bus>) {
        seq_runs<WIDTH>(bus, k, e, acc, walk, [](const typename SeqAcc<WIDTH>::type&, uint32_t) {});
        if constexpr (SEQ_DESK<Bus>) seq_master<WIDTH>(acc, bus.master);
        if constexpr (SEQ_RIDES<Bus>) seq_ride<WIDTH>(acc, bus, sha::master_lane(bus.groups.row0), k);      // the master's ride: behind its gain
        store();
    } else {
        constexpr bool WIDE = WIDTH >= 3;
        constexpr int N = SEQ_LANE<WIDTH>;
        constexpr bool CLIPS = SEQ_CLIPS<Bus>;
        typename std::conditional<CLIPS, shcl::Row, shmt::Row>::type* table;
        if constexpr (CLIPS) table = seq_clip_begin();
        else if constexpr (SEQ_GROUPS<Bus>) table = seq_meter_begin<shq::MAX_TRACKS + 1 + shg::MAX_GROUPS>();
        else table = seq_meter_begin();
        const bool stereo = bus.nch == 2;
        auto meter = [&](const Acc& x, uint32_t row) {         // a bus's samples (and flags) as they stand into its row
            seq_meter_wave<WIDE>(shmt::lane<WIDE, N>(seq_v(x), s0, lo, hi, bus.nch), stereo, table + row);
            if constexpr (CLIPS) seq_clip_wave(shcl::lane<N>(seq_flags(x), s0, lo, hi, bus.nch), stereo, table + row);
        };
        if (__builtin_amdgcn_ballot_w64(s0 < hi && s0 + N > lo)) {                    // (uniform: a wave with a lane in the window)
            seq_runs<WIDTH>(bus, k, e, acc, walk, meter);
            if constexpr (SEQ_DESK<Bus>) seq_master<WIDTH>(acc, bus.master);
            if constexpr (SEQ_RIDES<Bus>) seq_ride<WIDTH>(acc, bus, sha::master_lane(bus.groups.row0), k);      // (in front of the master's row: over the stored bytes)
            meter(acc, bus.ntracks);
            store();
        }
        if constexpr (SEQ_HISTORY<Bus>) seq_hist_end<WIDTH>(table, bus, bus.groups.n, k, lo);      // (k: the song tile, in song order whatever workgroup folds it)
        else if constexpr (SEQ_GROUPS<Bus>) seq_meter_end<WIDE>(table, bus, bus.groups.n);
        else seq_meter_end<WIDE>(table, bus);
    }
}

// PLAIN at 16 bits: k_seq_plain16's schedule
template <int SCHEME, int INFLIGHT, bool BUS = false, typename... Bus>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_win_plain16(const SeqEv* __restrict__ ev, const she::Seg* __restrict__ segs,
                                                                   const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                                   const uint32_t* __restrict__ order, uint32_t lo, uint32_t hi, short* out, int aligned,
                                                                   const Bus... bus) {
    static_assert(sizeof...(Bus) == (BUS ? 1 : 0), "the bus, and only with BUS");
    uint32_t k, t0, s0;
    if constexpr (SEQ_METERS<Bus...>) {
        if (!seq_window_tile<2>(order, lo, hi, k, t0, s0)) return;
    } else {
        if (!seq_window_lane<2>(order, lo, hi, k, t0, s0)) return;
    }
    const bool whole = aligned && s0 >= lo && s0 + 8 <= hi;
    typename SeqWinAcc<2, Bus...>::type acc = {};
    auto walk = [&](uint32_t& e, uint32_t e1, auto& into) { seq_walk_plain16<SCHEME, INFLIGHT>(ev, segs, idx, e, e1, t0, s0, into); };
    auto store = [&] { seq_window_store8(out, s0, lo, hi, whole, seq_v(acc)); };
    uint32_t e = first[k];
    if constexpr (SEQ_STEMS<Bus...>) {
        seq_stems_bus<2>(bus..., k, e, acc, walk, [&](short* to, const short8v& x) { seq_window_store8(to, s0, lo, hi, whole, x); }, out);
    } else if constexpr (BUS) {
        seq_window_bus<2>(bus..., k, e, s0, lo, hi, acc, walk, store);
    } else {
        walk(e, first[k + 1], acc);
        store();
    }
}

// The other levels at 16 bits: k_seq_16's schedule.  An idle tile reads neither record nor index: behind the last event idx holds nothing.
template <int LEVEL, int SCHEME, bool BUS = false, typename... Bus>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_win_16(const typename SeqRec<LEVEL>::type* __restrict__ ev, const she::Seg* __restrict__ segs,
                                                              const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                              const uint32_t* __restrict__ order, uint32_t lo, uint32_t hi, short* out, int aligned,
                                                              const Bus... bus) {
    static_assert(sizeof...(Bus) == (BUS ? 1 : 0), "the bus, and only with BUS");
    uint32_t k, t0, s0;
    if constexpr (SEQ_METERS<Bus...>) {
        if (!seq_window_tile<2>(order, lo, hi, k, t0, s0)) return;
    } else {
        if (!seq_window_lane<2>(order, lo, hi, k, t0, s0)) return;
    }
    const bool whole = aligned && s0 >= lo && s0 + 8 <= hi;
    typename SeqWinAcc<2, Bus...>::type acc = {};
    auto walk = [&](uint32_t& e, uint32_t e1, auto& into) { seq_walk_16<LEVEL, SCHEME>(ev, segs, idx, e, e1, t0, s0, into); };
    auto store = [&] { seq_window_store8(out, s0, lo, hi, whole, seq_v(acc)); };
    uint32_t e = first[k];
    if constexpr (SEQ_STEMS<Bus...>) {
        seq_stems_bus<2>(bus..., k, e, acc, walk, [&](short* to, const short8v& x) { seq_window_store8(to, s0, lo, hi, whole, x); }, out);
    } else if constexpr (BUS) {
        seq_window_bus<2>(bus..., k, e, s0, lo, hi, acc, walk, store);
    } else {
        const uint32_t e1 = first[k + 1];
        if (e < e1) walk(e, e1, acc);                         // (uniform)
        store();
    }
}

// Widths 1, 3 and 4: k_seq_w's loop from silence, every sample of the lane that lies in the window stored
template <int LEVEL, int WIDTH, bool BUS = false, typename... Bus>
__global__ __launch_bounds__(shq::TILE_THREADS) void k_win_w(const typename SeqRec<LEVEL>::type* __restrict__ ev, const she::Seg* __restrict__ segs,
                                                             const uint32_t* __restrict__ first, const uint32_t* __restrict__ idx,
                                                             const uint32_t* __restrict__ order, uint32_t lo, uint32_t hi, unsigned char* out,
                                                             const Bus... bus) {
    static_assert(sizeof...(Bus) == (BUS ? 1 : 0), "the bus, and only with BUS");
    static_assert(LEVEL != ENV || WIDTH == 1 || WIDTH == 4, "an envelope has widths 1, 2 and 4");
    uint32_t k, t0, s0;
    if constexpr (SEQ_METERS<Bus...>) {
        if (!seq_window_tile<WIDTH>(order, lo, hi, k, t0, s0)) return;
    } else {
        if (!seq_window_lane<WIDTH>(order, lo, hi, k, t0, s0)) return;
    }
    typename SeqWinAcc<WIDTH, Bus...>::type acc = {};
    auto walk = [&](uint32_t& e, uint32_t e1, auto& into) { seq_walk_w<LEVEL, WIDTH>(ev, segs, idx, e, e1, t0, s0, into); };
    auto store = [&] { seq_window_store_w<WIDTH>(out, s0, lo, hi, seq_v(acc)); };
    uint32_t e = first[k];
    if constexpr (SEQ_STEMS<Bus...>) {
        seq_stems_bus<WIDTH>(bus..., k, e, acc, walk, [&](unsigned char* to, const llong4v& x) { seq_window_store_w<WIDTH>(to, s0, lo, hi, x); }, out);
    } else if constexpr (BUS) {
        seq_window_bus<WIDTH>(bus..., k, e, s0, lo, hi, acc, walk, store);
    } else {
        walk(e, first[k + 1], acc);
        store();
    }
}

}  // namespace

// ---- host: what the entry points share ----------------------------------------------------------------------------------------------
namespace {

int seq_null(const char* fn) { return sh::set_error(SH_ERR_INVALID, "%s: NULL argument", fn); }

// the arguments in front of the events: width, pointers, the track's range, no source that is (or overlaps) the track
int seq_check_args(const char* fn, const sh_buf* const* srcs, uint32_t nsrc, const void* events, uint32_t nevents, int width,
                   const sh_buf* track, size_t track_samples) {
    if (width < 1 || width > 4) return sh::set_error(SH_ERR_INVALID, "%s: width %d not in {1, 2, 3, 4}", fn, width);
    if (!track || (nevents && !events) || (nsrc && !srcs)) return seq_null(fn);
    const size_t w = (size_t)width;
    if (track_samples > track->bytes / w) return sh::set_error(SH_ERR_INVALID, "%s: track range outside buffer", fn);
    const char* t0 = (const char*)track->ptr;
    const char* t1 = t0 + track_samples * w;
    for (uint32_t v = 0; v < nsrc; ++v) {
        if (!srcs[v]) continue;
        const char* p = (const char*)srcs[v]->ptr;
        if (srcs[v] == track || (p < t1 && t0 < p + srcs[v]->bytes)) return sh::set_error(SH_ERR_INVALID, "%s: source %u is the track", fn, v);
    }
    return SH_OK;
}

// The plan of the checked events (dst, n), then records | tiles | first | idx as one block on the library's grow-only scratch, one copy,
// one launch: fill(rec) writes the nevents records, launch(records, tiles, first, idx, ntiles, grid, block, stream) names the kernel.
// after_records: bytes of a second table (a multiple of 16) that fill writes behind the records and the kernel finds there.
template <typename Rec, typename Fill, typename Launch>
int seq_run(const char* fn, const std::vector<shq::Event>& pe, int width, size_t track_samples, Fill fill, Launch launch, size_t after_records = 0) {
    const uint32_t nevents = (uint32_t)pe.size();
    const uint32_t tile = shq::tile_samples(width);
    const shq::Plan P = shq::plan(pe.data(), nevents, track_samples, tile);
    if (P.refused == shq::EVENT_BEYOND_TRACK) return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside the track", fn, P.bad_event);
    if (P.refused == shq::TRACK_TOO_LONG) return sh::set_error(SH_ERR_INVALID, "%s: at most 2^32 - 65536 track samples per call", fn);
    if (P.refused) return sh::set_error(SH_ERR_INVALID, "%s: more than 2^28 (event, tile) overlaps in one call", fn);
    if (P.tiles.empty()) return SH_OK;
    const uint32_t nt = (uint32_t)P.tiles.size();
    const size_t b_ev = (size_t)nevents * sizeof(Rec) + after_records, b_tiles = (size_t)nt * 4, b_first = ((size_t)nt + 1) * 4, b_idx = P.idx.size() * 4;
    std::vector<char> host(b_ev + b_tiles + b_first + b_idx);
    fill(reinterpret_cast<Rec*>(host.data()));
    memcpy(host.data() + b_ev, P.tiles.data(), b_tiles);
    memcpy(host.data() + b_ev + b_tiles, P.first.data(), b_first);
    memcpy(host.data() + b_ev + b_tiles + b_first, P.idx.data(), b_idx);
    int rc = sh::ensure_scratch(host.size());
    if (rc) return rc;
    hipStream_t st = sh::state().stream;
    char* dev = (char*)sh::state().scratch;
    // (pageable source: staged before the call returns, ordered after earlier kernels)
    SH_HIP(hipMemcpyAsync(dev, host.data(), host.size(), hipMemcpyHostToDevice, st));
    launch((const Rec*)dev, (const uint32_t*)(dev + b_ev), (const uint32_t*)(dev + b_ev + b_tiles), (const uint32_t*)(dev + b_ev + b_tiles + b_first),
           nt, sh::grid1d(nt, 1), dim3(shq::TILE_THREADS), st);
    SH_CHECK_LAUNCH(fn);
    return SH_OK;
}

// One event as the entry points' adapters hand it on: sh_mix_event_env's fields and the call's nchannels (the track's).  What a lower
// level's struct does not have says "none": inrate == outrate, src_channels == nchannels, seg_count == 0.
struct SeqIn {
    uint64_t dst_sample, src_sample, nsamples, src_frames;
    double   factor, left, right;
    uint32_t src, inrate, outrate, src_channels, seg_first, seg_count, reserved;
    int      nchannels;
    uint64_t loop_start = 0, loop_frames = 0;               // sh_mix_event_loop's; loop_frames == 0: none, and src_frames is what it was
    uint32_t flags = 0;                                      // sh_mix_event_rev's; SH_MIX_EVENT_REVERSED: played backwards
    bool tostereo() const { return src_channels == 1 && nchannels == 2; }
    bool downmix() const { return (flags & SH_MIX_EVENT_DOWNMIX) != 0; }      // sh_mix_event_chan's; the six other entry points say none
    bool balance() const { return (flags & SH_MIX_EVENT_BALANCE) != 0; }
    uint32_t mode() const { return tostereo() ? SEQ_TOSTEREO : downmix() ? SEQ_DOWNMIX : balance() ? SEQ_BALANCE : SEQ_NONE; }
    bool reversed() const { return (flags & SH_MIX_EVENT_REVERSED) != 0; }
    // the frames of a reversed event's region, stored from src_sample on: nothing behind a loop's end is played, and a looped event's
    // src_frames counts virtual frames
    uint64_t region_frames() const { return loop_frames ? loop_start + loop_frames : src_frames; }
};

// sh_mix_event_chan as a SeqIn, and sh_mix_event_rev, _loop and _env, whose fields are its first ones, for the fields they have
template <typename Ev>
SeqIn seq_in(const Ev& m, int nchannels) {
    SeqIn v{m.dst_sample, m.src_sample, m.nsamples, m.src_frames, m.factor, m.left, m.right, m.src, m.inrate, m.outrate, m.src_channels,
            m.seg_first, m.seg_count, m.reserved, nchannels};
    if constexpr (!std::is_same<Ev, sh_mix_event_env>::value) {
        v.loop_start = m.loop_start;
        v.loop_frames = m.loop_frames;
        if constexpr (!std::is_same<Ev, sh_mix_event_loop>::value) v.flags = m.flags;
    }
    return v;
}

// 24-bit samples may loop, play backwards and be downmixed, every other step has a 24-bit form; an envelope has none: the first event
// of a width-3 list that has segments is refused
template <typename Ev>
int seq_check_width3(const char* fn, const Ev* events, uint32_t nevents, int width) {
    for (uint32_t e = 0; width == 3 && e < nevents; ++e)
        if (events[e].seg_count) return sh::set_error(SH_ERR_INVALID, "%s: event %u: width 3: an envelope's fades have no 24-bit form", fn, e);
    return SH_OK;
}

// the caller's segments as the kernels read them (a segment that no event names was not checked, and no kernel reads it)
void seq_segments(she::Seg* dst, const sh_env_segment* segments, uint32_t n) {
    for (uint32_t s = 0; s < n; ++s) {
        const sh_env_segment& g = segments[s];
        dst[s] = she::Seg{g.mul, g.slope, g.numsamples, g.offset, (uint32_t)g.end, (uint32_t)g.origin, g.kind, 0};
    }
}

// Every refusal of an event, in the order they are reported; in(e): event e as a SeqIn.  pe: the plan's view of the checked events.
template <typename In>
int seq_check_events(const char* fn, int level, In in, uint32_t nevents, const sh_buf* const* srcs, uint32_t nsrc, const sh_env_segment* segments,
                     uint32_t nsegments, int width, std::vector<shq::Event>& pe) {
    const size_t w = (size_t)width;
    for (uint32_t e = 0; e < nevents; ++e) {
        const SeqIn m = in(e);
        if (m.reserved != 0) return sh::set_error(SH_ERR_INVALID, "%s: event %u: reserved must be 0", fn, e);
        const uint32_t known = level == CHAN ? SH_MIX_EVENT_REVERSED | SH_MIX_EVENT_DOWNMIX | SH_MIX_EVENT_BALANCE : SH_MIX_EVENT_REVERSED;
        if (m.flags & ~known) return sh::set_error(SH_ERR_INVALID, "%s: event %u: unknown flags 0x%x", fn, e, m.flags);
        if (m.downmix() || m.balance()) {
            if (m.downmix() && m.balance()) return sh::set_error(SH_ERR_INVALID, "%s: event %u: downmix and balance on one event", fn, e);
            if (m.src_channels != 2) return sh::set_error(SH_ERR_INVALID, "%s: event %u: a downmix or balance needs a stereo source, src_channels is %u", fn, e, m.src_channels);
            if (m.downmix() && m.nchannels != 1) return sh::set_error(SH_ERR_INVALID, "%s: event %u: a downmix needs a mono track, this one has %d channels", fn, e, m.nchannels);
            if (m.balance() && m.nchannels != 2) return sh::set_error(SH_ERR_INVALID, "%s: event %u: a balance needs a stereo track, this one has %d channels", fn, e, m.nchannels);
            if (!isfinite(m.left) || !isfinite(m.right)) return sh::set_error(SH_ERR_INVALID, "%s: event %u: left / right is not finite", fn, e);
            if (m.balance() && m.dst_sample % 2) return sh::set_error(SH_ERR_INVALID, "%s: event %u: a balance starts on a whole stereo frame", fn, e);
            // the kernels form a downmix's source-sample coordinates, 2 dst and 2 n, in 32 bits
            if (m.downmix() && (m.nsamples > shq::MAX_TRACK_SAMPLES / 2 || m.dst_sample > shq::MAX_TRACK_SAMPLES / 2 - m.nsamples))
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: a downmix ends at most 2^31 - 32768 track samples in", fn, e);
        }
        if (!isfinite(m.factor)) return sh::set_error(SH_ERR_INVALID, "%s: event %u: factor is not finite", fn, e);
        if (m.src >= nsrc || !srcs[m.src]) return sh::set_error(SH_ERR_INVALID, "%s: event %u: no source %u", fn, e, m.src);
        if (!m.tostereo() && !m.downmix() && m.src_channels != (uint32_t)m.nchannels) {
            if (level == PAN) return sh::set_error(SH_ERR_INVALID, "%s: event %u: src_channels %u not 1 or 2", fn, e, m.src_channels);
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: src_channels %u is neither the track's %d nor a mono source of a stereo track", fn, e, m.src_channels, m.nchannels);
        }
        if (!m.inrate || !m.outrate || m.inrate >= (1u << 31) || m.outrate >= (1u << 31))
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: sampling rate not in [1, 2^31)", fn, e);
        const uint64_t nch = m.src_channels, have = srcs[m.src]->bytes / w;
        uint64_t nsrc_samples = m.nsamples;                   // what the event takes of its (resampled) source
        if (m.tostereo()) {
            if (!isfinite(m.left) || !isfinite(m.right)) return sh::set_error(SH_ERR_INVALID, "%s: event %u: left / right is not finite", fn, e);
            if (m.dst_sample % 2 || m.nsamples % 2)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: a mono source starts and ends on whole stereo frames", fn, e);
            nsrc_samples = m.nsamples / 2;
        }
        if (m.downmix()) nsrc_samples = m.nsamples * 2;
        const bool looped = m.loop_frames != 0;               // src_frames counts VIRTUAL frames then, and may exceed the source's
        if (m.src_sample > have || (!looped && m.inrate == m.outrate && nsrc_samples > have - m.src_sample))
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside its source", fn, e);
        if (looped) {
            if (m.src_sample % nch || nsrc_samples % nch)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: a looped event starts and ends on whole frames", fn, e);
            const uint64_t held = (have - m.src_sample) / nch;
            if (m.loop_start > held || m.loop_frames > held - m.loop_start)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: loop outside its source", fn, e);
            if (m.src_frames > shq::MAX_TRACK_SAMPLES / nch)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: at most 2^32 - 65536 looped samples per event", fn, e);
            if (m.inrate == m.outrate && nsrc_samples / nch > m.src_frames)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: more samples than src_frames hold", fn, e);
        }
        if (m.reversed()) {                                   // the region as stored: region_frames() whole frames from src_sample on
            if (m.src_sample % nch) return sh::set_error(SH_ERR_INVALID, "%s: event %u: a reversed event's region starts on a whole frame", fn, e);
            if (m.region_frames() > (have - m.src_sample) / nch)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: reversed region outside its source", fn, e);
            if (!looped && m.inrate == m.outrate && nsrc_samples > m.region_frames() * nch)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: more samples than src_frames hold", fn, e);
        }
        if (m.inrate != m.outrate) {
            if (m.src_sample % nch || nsrc_samples % nch)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: a resampled event starts and ends on whole frames", fn, e);
            if (!looped && m.src_frames > (have - m.src_sample) / nch) return sh::set_error(SH_ERR_INVALID, "%s: event %u: src_frames outside its source", fn, e);
            if (nsrc_samples / nch > shr::out_frames(m.src_frames, shr::reduce(m.inrate, m.outrate)))
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: more samples than src_frames resample to", fn, e);
        }
        if (m.seg_count > she::MAX_SEGMENTS) return sh::set_error(SH_ERR_INVALID, "%s: event %u: more than %u segments", fn, e, she::MAX_SEGMENTS);
        if (m.seg_count && (m.seg_first > nsegments || m.seg_count > nsegments - m.seg_first))
            return sh::set_error(SH_ERR_INVALID, "%s: event %u: segments outside the table", fn, e);
        uint64_t prev = 0;
        for (uint32_t s = 0; s < m.seg_count; ++s) {
            const sh_env_segment& g = segments[m.seg_first + s];
            if (g.reserved != 0) return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: reserved must be 0", fn, e, s);
            if (g.end < prev || g.end > nsrc_samples)
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: ends not ascending or beyond the event's source samples", fn, e, s);
            if (g.kind > she::FADE_OUT) return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: kind %u not 0, 1 or 2", fn, e, s, g.kind);
            if (!isfinite(g.mul) || !isfinite(g.slope) || !isfinite(g.numsamples) || !isfinite(g.offset))
                return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: a factor is not finite", fn, e, s);
            if (g.kind != she::NONE && !(g.numsamples > 0.0)) return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: a ramp needs numsamples > 0", fn, e, s);
            if (g.origin > nsrc_samples) return sh::set_error(SH_ERR_INVALID, "%s: event %u: segment %u: origin beyond the event's source samples", fn, e, s);
            prev = g.end;
        }
        pe[e] = shq::Event{m.dst_sample, m.nsamples};
    }
    return SH_OK;
}

// the records of the checked events
template <int LEVEL, typename In>
void seq_fill(typename SeqRec<LEVEL>::type* rec, In in, uint32_t nevents, const sh_buf* const* srcs, int width) {
    for (uint32_t e = 0; e < nevents; ++e) {
        const SeqIn m = in(e);
        const void* src = (const char*)srcs[m.src]->ptr + m.src_sample * (size_t)width;
        if constexpr (LEVEL == PLAIN) {
            rec[e] = SeqEv{src, m.factor, (uint32_t)m.dst_sample, (uint32_t)m.nsamples, {0, 0}};
        } else {
            const shr::Rates R = shr::reduce(m.inrate, m.outrate);
            const SeqEvR r{src, m.factor, 1.0 / (double)R.outr, (uint32_t)m.dst_sample, (uint32_t)m.nsamples, R.inr, R.outr, R.inr / R.outr, R.inr % R.outr,
                           m.src_channels, width <= 2 && R.outr < 65536u ? 1u : 0u, {0, 0}};
            if constexpr (LEVEL == RATE) rec[e] = r;
            else if constexpr (LEVEL == PAN) rec[e] = SeqEvP{r, m.left, m.right, {0, 0}, m.tostereo() ? 1u : 0u, 0};
            else {
                const SeqEvE v{r, m.left, m.right, m.seg_count ? m.seg_first : 0u, m.seg_count, m.mode(), 0};
                if constexpr (LEVEL == ENV) rec[e] = v;
                else {
                    // a note no longer than its head (V <= E) is a plain cut: no loop pass, an event of ENV
                    const uint64_t E = m.loop_start + m.loop_frames;
                    SeqEvL l{v};
                    if (m.loop_frames && m.src_frames > E) {
                        l.pad[0] = (uint32_t)E;
                        l.pad[1] = (uint32_t)m.loop_frames;
                        l.pad3 = (uint32_t)(r.step_q % m.loop_frames);
                    }
                    if constexpr (LEVEL == LOOP) rec[e] = l;
                    else {
                        SeqEvV t{l};
                        if (m.reversed()) {                   // one sample behind the region; played sample i is src[-1 - i]
                            t.src = (const char*)src + shv::origin(1u, m.region_frames() * m.src_channels) * (size_t)width;
                            t.small |= 2u;
                        }
                        rec[e] = t;
                    }
                }
            }
        }
    }
}

// which kernel: the width, at 16 bits the way misaligned event samples are read and whether the track starts on a 16-byte boundary
template <int LEVEL>
void seq_launch(const typename SeqRec<LEVEL>::type* ev, const she::Seg* segs, const uint32_t* tiles, const uint32_t* first, const uint32_t* idx, uint32_t nt,
                dim3 grid, dim3 block, hipStream_t st, int width, sh_buf* track, uint32_t ns) {
    if (width == 2) {
        const int aligned = ((uintptr_t)track->ptr & 15) == 0;
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, ev, segs, tiles, first, idx, nt, (short*)track->ptr, ns, aligned); };
        const bool vec2 = sh::knobs().seq_align == VEC2;
        if constexpr (LEVEL == PLAIN) vec2 ? go(k_seq_plain16<VEC2, 4>) : go(k_seq_plain16<FUNNEL, 4>);
        else vec2 ? go(k_seq_16<LEVEL, VEC2>) : go(k_seq_16<LEVEL, FUNNEL>);
    } else {
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, ev, segs, tiles, first, idx, nt, (unsigned char*)track->ptr, ns); };
        if (width == 1) go(k_seq_w<LEVEL, 1>);
        else if (width == 4) go(k_seq_w<LEVEL, 4>);
        else if constexpr (LEVEL != ENV) go(k_seq_w<LEVEL, 3>);       // (LOOP: the entry point refuses width 3 with segments)
    }
}

// What the seven entry points do behind their own arguments: check, plan, records (and the segments behind them), one launch.
template <int LEVEL, typename In>
int seq_mix(const char* fn, In in, const sh_buf* const* srcs, uint32_t nsrc, uint32_t nevents, const sh_env_segment* segments, uint32_t nsegments, int width,
            int nchannels, sh_buf* track, size_t track_samples) {
    typedef typename SeqRec<LEVEL>::type Rec;
    if (nchannels < 1) return sh::set_error(SH_ERR_INVALID, "%s: # of channels should be >= 1", fn);
    if (nsegments && !segments) return seq_null(fn);
    std::vector<shq::Event> pe(nevents);
    const int rc = seq_check_events(fn, LEVEL, in, nevents, srcs, nsrc, segments, nsegments, width, pe);
    if (rc) return rc;
    return seq_run<Rec>(fn, pe, width, track_samples,
        [&](Rec* rec) {
            seq_fill<LEVEL>(rec, in, nevents, srcs, width);
            seq_segments(reinterpret_cast<she::Seg*>(rec + nevents), segments, nsegments);
        },
        [&](const Rec* d_ev, const uint32_t* d_tiles, const uint32_t* d_first, const uint32_t* d_idx, uint32_t nt, dim3 grid, dim3 block, hipStream_t st) {
            seq_launch<LEVEL>(d_ev, reinterpret_cast<const she::Seg*>(d_ev + nevents), d_tiles, d_first, d_idx, nt, grid, block, st, width, track,
                              (uint32_t)track_samples);
        },
        (size_t)nsegments * sizeof(she::Seg));
}

}  // namespace

// ---- the entry points: their own arguments, and an adapter from their event struct to SeqIn ----------------------------------------------
extern "C" {

int sh_mix_events(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event* events, uint32_t nevents, int width, sh_buf* track,
                  size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events";
    const int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (rc) return rc;
    auto in = [=](uint32_t e) {
        const sh_mix_event& m = events[e];
        return SeqIn{m.dst_sample, m.src_sample, m.nsamples, 0, m.factor, 0.0, 0.0, m.src, 1, 1, 1, 0, 0, m.reserved, 1};
    };
    return seq_mix<PLAIN>(fn, in, srcs, nsrc, nevents, nullptr, 0, width, 1, track, track_samples);
}

int sh_mix_events_rate(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_rate* events, uint32_t nevents, int width, int nchannels,
                       sh_buf* track, size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events_rate";
    const int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (rc) return rc;
    auto in = [=](uint32_t e) {
        const sh_mix_event_rate& m = events[e];
        return SeqIn{m.dst_sample, m.src_sample, m.nsamples, m.src_frames, m.factor, 0.0, 0.0, m.src, m.inrate, m.outrate, (uint32_t)nchannels, 0, 0,
                     m.reserved, nchannels};
    };
    return seq_mix<RATE>(fn, in, srcs, nsrc, nevents, nullptr, 0, width, nchannels, track, track_samples);
}

int sh_mix_events_pan(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_pan* events, uint32_t nevents, int width, sh_buf* track,
                      size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events_pan";
    const int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (rc) return rc;
    auto in = [=](uint32_t e) {
        const sh_mix_event_pan& m = events[e];
        return SeqIn{m.dst_sample, m.src_sample, m.nsamples, m.src_frames, m.factor, m.left, m.right, m.src, m.inrate, m.outrate, m.src_channels, 0, 0,
                     m.reserved, 2};
    };
    return seq_mix<PAN>(fn, in, srcs, nsrc, nevents, nullptr, 0, width, 2, track, track_samples);
}

int sh_mix_events_env(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_env* events, uint32_t nevents,
                      const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, sh_buf* track, size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events_env";
    if (width == 3) return sh::set_error(SH_ERR_INVALID, "%s: width 3: an envelope's fades have no 24-bit form", fn);
    const int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (rc) return rc;
    auto in = [=](uint32_t e) { return seq_in(events[e], nchannels); };
    return seq_mix<ENV>(fn, in, srcs, nsrc, nevents, segments, nsegments, width, nchannels, track, track_samples);
}

int sh_mix_events_loop(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_loop* events, uint32_t nevents,
                       const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, sh_buf* track, size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events_loop";
    int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (!rc) rc = seq_check_width3(fn, events, nevents, width);
    if (rc) return rc;
    auto in = [=](uint32_t e) { return seq_in(events[e], nchannels); };
    return seq_mix<LOOP>(fn, in, srcs, nsrc, nevents, segments, nsegments, width, nchannels, track, track_samples);
}

int sh_mix_events_rev(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_rev* events, uint32_t nevents,
                      const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, sh_buf* track, size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events_rev";
    int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (!rc) rc = seq_check_width3(fn, events, nevents, width);
    if (rc) return rc;
    auto in = [=](uint32_t e) { return seq_in(events[e], nchannels); };
    return seq_mix<REV>(fn, in, srcs, nsrc, nevents, segments, nsegments, width, nchannels, track, track_samples);
}

int sh_mix_events_chan(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_chan* events, uint32_t nevents,
                       const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, sh_buf* track, size_t track_samples) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_mix_events_chan";
    int rc = seq_check_args(fn, srcs, nsrc, events, nevents, width, track, track_samples);
    if (!rc) rc = seq_check_width3(fn, events, nevents, width);
    if (rc) return rc;
    auto in = [=](uint32_t e) { return seq_in(events[e], nchannels); };
    return seq_mix<CHAN>(fn, in, srcs, nsrc, nevents, segments, nsegments, width, nchannels, track, track_samples);
}

}  // extern "C"

// ---- a kept song: sh_seq ---------------------------------------------------------------------------------------------------------------
// What sh_mix_events_chan does in front of its launch, done once: the checked events as records of the LOWEST level whose chain covers
// every row, the segments, and plan_by_tile's index, in one device block that the handle owns (the buffer pool's, as sh_buf_alloc's; not
// the grow-only scratch, which the next call overwrites).  The records point into the sources: the caller keeps those alive.
struct sh_seq {
    void*    block = nullptr;             // records | segments | first | idx | order | runs | rfirst | meters (the last three: a song of tracks)
    size_t   cap = 0, bytes = 0;
    size_t   at_segs = 0, at_first = 0, at_idx = 0, at_order = 0;     // order: the tiles heaviest first, for a render of the whole song
    size_t   at_rfirst = 0, at_runs = 0;  // shq::plan_runs' table, behind order
    size_t   at_meters = 0;               // a song of tracks: ntracks + 1 rows of levels (shmt::Row) behind rfirst, written by a metered render alone
    uint32_t ntracks = 0, nruns = 0;      // ntracks == 0: sh_seq_create's flat list, no bus
    int      width = 0, nchannels = 0, level = 0;
    uint32_t nevents = 0, ntiles = 0, active_tiles = 0;
    uint64_t track_samples = 0, pairs = 0;
    std::vector<const char*> src_lo, src_hi;      // the byte ranges of the sources: a render's `out` may overlap none
};

// Fader automation of a song of tracks (sh_seq_auto_create): the tracks' segments and where each track's start, uploaded once into a
// block this handle owns; what it says of the song it was made for is what sh_seq_render_auto holds a song to.
struct sh_seq_auto {
    void*    block = nullptr;             // segments (she::Seg) | first (ntracks + 1 offsets; sh_seq_auto_create_buses: ntracks + 1 + MAX_GROUPS + 1)
                                          // sh_seq_auto_create_pans: the pan lanes' segments behind the others, their ntracks + MAX_GROUPS + 1 offsets behind the others'
    size_t   cap = 0, bytes = 0, at_first = 0;
    uint32_t ntracks = 0, nsegments = 0;
    uint32_t ngroups = 0;                 // sh_seq_auto_create_buses: the group lanes it was given
    uint32_t ridden = 0;                  // one past the last group lane that has a segment; 0: no group rides
    bool     buses = false;               // a bus lane -- the master's or a group's -- has a segment: the kernels that ride
    uint32_t panned = 0;                  // sh_seq_auto_create_pans: one past the last group PAN lane that has a segment; 0: none
    bool     pans = false;                // a pan lane -- a track's or a group's -- has a segment: the kernels that pan
    int      width = 0, nchannels = 0;
    uint64_t track_samples = 0;
};

namespace {

// the lowest level whose chain covers the row
int seq_row_level(const SeqIn& m) {
    if (m.downmix() || m.balance()) return CHAN;
    if (m.reversed()) return REV;
    if (m.loop_frames && m.src_frames > m.loop_start + m.loop_frames) return LOOP;        // (no longer than its head: a plain cut, seq_fill)
    if (m.seg_count) return ENV;
    if (m.tostereo()) return PAN;
    if (m.inrate != m.outrate) return RATE;
    return PLAIN;
}

// f(std::integral_constant<int, L>()) for the level L that a handle holds as a number
template <int L = PLAIN, typename F>
void seq_with_level(int level, F f) {
    if constexpr (L == CHAN) f(std::integral_constant<int, CHAN>());
    else if (level == L) f(std::integral_constant<int, L>());
    else seq_with_level<L + 1>(level, f);
}

// f(std::integral_constant<uint32_t, F>()) for the route F (one of shb::ROUTES) that a call takes; any other number: nothing, so that the
// kernels of the 22 routes are the only ones there are
template <uint32_t I = 0, typename F>
void seq_with_bus(uint32_t route, F f) {
    if constexpr (I < shb::NROUTES) {
        if (route == shb::ROUTES[I]) f(std::integral_constant<uint32_t, shb::ROUTES[I]>());
        else seq_with_bus<I + 1>(route, f);
    }
}

// the bus of route F out of one that holds every part: the parts F has, part by part
template <uint32_t F>
SeqBusOf<F> seq_bus_parts(const SeqBusOf<shb::PARTS>& all) {
    SeqBusOf<F> bus{};
    static_cast<SeqBus&>(bus) = all;
    if constexpr ((F & shb::METERS) != 0) static_cast<SeqMeters&>(bus) = all;
    if constexpr ((F & shb::DESK) != 0) static_cast<SeqDesk&>(bus) = all;
    if constexpr ((F & shb::AUTO) != 0) static_cast<SeqAuto&>(bus) = all;
    if constexpr ((F & shb::GROUPS) != 0) static_cast<SeqGroups&>(bus) = all;
    if constexpr ((F & shb::STEMS) != 0) static_cast<SeqStems&>(bus) = all;
    return bus;
}

// Which window kernel: the width, at 16 bits the way misaligned event samples are read and whether the biased base lies on a 16-byte
// boundary.  bus: nothing (a flat list) or the SeqBusOf<F> of one of shb::ROUTES (a song of tracks: the same kernels with the bus, its
// parts by value), forwarded as the kernels' trailing pack; shb::valid_at says at which widths the kernels of F exist.
template <int LEVEL, typename... Bus>
void seq_window_launch(const sh_seq* q, dim3 grid, hipStream_t st, uint32_t lo, uint32_t hi, void* out, const Bus&... bus) {
    typedef typename SeqRec<LEVEL>::type Rec;
    constexpr bool BUS = sizeof...(Bus) != 0;
    const char* b = (const char*)q->block;
    const Rec* ev = (const Rec*)b;
    const she::Seg* segs = (const she::Seg*)(b + q->at_segs);
    const uint32_t* first = (const uint32_t*)(b + q->at_first);
    const uint32_t* idx = (const uint32_t*)(b + q->at_idx);
    // the whole song: heaviest tile first (measured: profiles/sequence_plan_ab.txt); any other window: its tiles in song order
    const uint32_t* order = lo == 0 && hi == q->track_samples ? (const uint32_t*)(b + q->at_order) : nullptr;
    const dim3 block(shq::TILE_THREADS);
    constexpr bool AT3 = !BUS || shb::valid_at(SEQ_MASK<Bus...>, 3), W3 = BUS && AT3 && !shb::valid_at(SEQ_MASK<Bus...>, 2);      // W3: a group bus without automation, width 3's and only width 3's
    if constexpr (W3) {
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, ev, segs, first, idx, order, lo, hi, (unsigned char*)out, bus...); };
        if constexpr (LEVEL != ENV) go(k_win_w<LEVEL, 3, BUS, Bus...>);
    } else if (q->width == 2) {
        int aligned = ((uintptr_t)out & 15) == 0;             // the BIASED base: song-anchored lanes start on multiples of eight samples
        if constexpr (SEQ_STEMS<Bus...>) aligned = (shst::aligned((uint64_t)(uintptr_t)out, bus.stride) && ...);      // (stems: of EVERY plane)
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, ev, segs, first, idx, order, lo, hi, (short*)out, aligned, bus...); };
        const bool vec2 = sh::knobs().seq_align == VEC2;
        if constexpr (LEVEL == PLAIN) vec2 ? go(k_win_plain16<VEC2, 4, BUS, Bus...>) : go(k_win_plain16<FUNNEL, 4, BUS, Bus...>);
        else vec2 ? go(k_win_16<LEVEL, VEC2, BUS, Bus...>) : go(k_win_16<LEVEL, FUNNEL, BUS, Bus...>);
    } else {
        auto go = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, ev, segs, first, idx, order, lo, hi, (unsigned char*)out, bus...); };
        if (q->width == 1) go(k_win_w<LEVEL, 1, BUS, Bus...>);
        else if (q->width == 4) go(k_win_w<LEVEL, 4, BUS, Bus...>);
        else if constexpr (LEVEL != ENV && AT3) go(k_win_w<LEVEL, 3, BUS, Bus...>);       // (sh_seq_create refuses width 3 with segments, sh_seq_render_auto width 3)
    }
}

// sh_seq_create (track_first NULL, ntracks 0) and sh_seq_create_tracks behind their names
int seq_create(const char* fn, const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_chan* events, uint32_t nevents, const uint32_t* track_first,
               uint32_t ntracks, bool tracks, const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, size_t track_samples, sh_seq** out) {
    // The refusals in front of the events, in the ORDER sh_mix_events_chan reports them (seq_check_args without its track, the width-3
    // refusal, then seq_mix's two), so that a call with two faults names the same one here and there.
    if (!out) return seq_null(fn);
    *out = nullptr;
    if (width < 1 || width > 4) return sh::set_error(SH_ERR_INVALID, "%s: width %d not in {1, 2, 3, 4}", fn, width);
    if ((nevents && !events) || (nsrc && !srcs)) return seq_null(fn);
    int rc = seq_check_width3(fn, events, nevents, width);
    if (rc) return rc;
    if (nchannels < 1) return sh::set_error(SH_ERR_INVALID, "%s: # of channels should be >= 1", fn);
    if (nsegments && !segments) return seq_null(fn);
    if (tracks) {                                             // the tracks' events, concatenated: track t holds events [track_first[t], track_first[t + 1])
        if (ntracks == 0) return sh::set_error(SH_ERR_INVALID, "%s: a song needs at least one track", fn);
        if (ntracks > shq::MAX_TRACKS) return sh::set_error(SH_ERR_INVALID, "%s: %u tracks, at most %u", fn, ntracks, shq::MAX_TRACKS);
        if (!track_first) return seq_null(fn);
        if (track_first[0] != 0 || track_first[ntracks] != nevents)
            return sh::set_error(SH_ERR_INVALID, "%s: track_first starts at 0 and ends at nevents", fn);
        for (uint32_t t = 0; t < ntracks; ++t)
            if (track_first[t] > track_first[t + 1]) return sh::set_error(SH_ERR_INVALID, "%s: track_first decreases at track %u", fn, t + 1);
    }
    auto in = [=](uint32_t e) { return seq_in(events[e], nchannels); };
    std::vector<shq::Event> pe(nevents);
    rc = seq_check_events(fn, CHAN, in, nevents, srcs, nsrc, segments, nsegments, width, pe);
    if (rc) return rc;
    const shq::TilePlan P = shq::plan_by_tile(pe.data(), nevents, track_samples, shq::tile_samples(width));
    if (P.refused == shq::EVENT_BEYOND_TRACK) return sh::set_error(SH_ERR_INVALID, "%s: event %u: range outside the track", fn, P.bad_event);
    if (P.refused == shq::TRACK_TOO_LONG) return sh::set_error(SH_ERR_INVALID, "%s: at most 2^32 - 65536 track samples per call", fn);
    if (P.refused) return sh::set_error(SH_ERR_INVALID, "%s: more than 2^28 (event, tile) overlaps in one call", fn);
    int level = PLAIN;
    for (uint32_t e = 0; e < nevents; ++e) level = std::max(level, seq_row_level(in(e)));
    const size_t rec = level == PLAIN ? sizeof(SeqEv) : level == RATE ? sizeof(SeqEvR) : sizeof(SeqEvV);       // (PAN .. CHAN: 96 bytes)
    sh_seq* q = new (std::nothrow) sh_seq;
    if (!q) return sh::set_error(SH_ERR_NOMEM, "host allocation failed");
    q->width = width;
    q->nchannels = nchannels;
    q->level = level;
    q->nevents = nevents;
    q->ntiles = P.ntiles;
    q->active_tiles = P.active;
    q->track_samples = track_samples;
    q->pairs = P.idx.size();
    q->at_segs = (size_t)nevents * rec;
    q->at_first = q->at_segs + (size_t)nsegments * sizeof(she::Seg);
    q->at_idx = q->at_first + P.first.size() * 4;
    q->at_order = q->at_idx + P.idx.size() * 4;
    q->bytes = q->at_order + (size_t)P.ntiles * 4;
    shq::RunPlan R;
    if (tracks) {                                             // the run table behind order, 8-byte aligned for its 8-byte rows
        std::vector<uint32_t> track_of(nevents);
        for (uint32_t t = 0; t < ntracks; ++t)
            for (uint32_t e = track_first[t]; e < track_first[t + 1]; ++e) track_of[e] = t;
        R = shq::plan_runs(P.first.data(), P.idx.data(), P.ntiles, track_of.data());
        q->ntracks = ntracks;
        q->nruns = (uint32_t)R.runs.size();
        q->at_runs = (q->bytes + 7) & ~(size_t)7;
        q->at_rfirst = q->at_runs + R.runs.size() * sizeof(shq::Run);
        q->at_meters = (q->at_rfirst + R.rfirst.size() * 4 + 7) & ~(size_t)7;
        q->bytes = q->at_meters + ((size_t)ntracks + 1) * sizeof(shmt::Row);
    }
    for (uint32_t v = 0; v < nsrc; ++v) {
        if (!srcs[v] || !srcs[v]->bytes) continue;
        q->src_lo.push_back((const char*)srcs[v]->ptr);
        q->src_hi.push_back((const char*)srcs[v]->ptr + srcs[v]->bytes);
    }
    std::vector<char> host(q->bytes);
    seq_with_level(level, [&](auto L) {
        constexpr int LEVEL = decltype(L)::value;
        seq_fill<LEVEL>(reinterpret_cast<typename SeqRec<LEVEL>::type*>(host.data()), in, nevents, srcs, width);
    });
    seq_segments(reinterpret_cast<she::Seg*>(host.data() + q->at_segs), segments, nsegments);
    memcpy(host.data() + q->at_first, P.first.data(), P.first.size() * 4);
    if (!P.idx.empty()) memcpy(host.data() + q->at_idx, P.idx.data(), P.idx.size() * 4);
    if (P.ntiles) {                                           // every tile, heaviest first, ties in song order (idle tiles last)
        std::vector<uint32_t> order(P.ntiles);
        for (uint32_t t = 0; t < P.ntiles; ++t) order[t] = t;
        std::stable_sort(order.begin(), order.end(),
                         [&](uint32_t a, uint32_t b) { return P.first[a + 1] - P.first[a] > P.first[b + 1] - P.first[b]; });
        memcpy(host.data() + q->at_order, order.data(), (size_t)P.ntiles * 4);
    }
    if (tracks) {
        if (!R.runs.empty()) memcpy(host.data() + q->at_runs, R.runs.data(), R.runs.size() * sizeof(shq::Run));
        memcpy(host.data() + q->at_rfirst, R.rfirst.data(), R.rfirst.size() * 4);
    }
    // (a song of tracks: behind the song's tables, which `bytes` counts, room for the rows of a metered render's groups)
    rc = sh::pool_alloc(q->bytes + (tracks ? shg::MAX_GROUPS * sizeof(shmt::Row) : 0), &q->block, &q->cap);
    if (rc) {
        delete q;
        return rc;
    }
    hipStream_t st = sh::state().stream;
    hipError_t e = hipMemcpyAsync(q->block, host.data(), host.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);        // once per song: the host copy goes when this returns
    if (e != hipSuccess) {
        sh::pool_free(q->block, q->cap);
        delete q;
        return sh::hip_error(e, fn);
    }
    *out = q;
    return SH_OK;
}

// the gains of a render as the kernels take them: the caller's ngains (NULL: none given), every finite; 1.0 for every other track
int seq_gains(const char* fn, const double* gains, uint32_t ngains, SeqGains& out) {
    for (uint32_t t = 0; t < shq::MAX_TRACKS; ++t) out.g[t] = 1.0;
    for (uint32_t t = 0; gains && t < ngains; ++t) {
        if (!isfinite(gains[t])) return sh::set_error(SH_ERR_INVALID, "%s: gain %u is not finite", fn, t);
        out.g[t] = gains[t];
    }
    return SH_OK;
}

// the desk of a render as the kernels take it: the caller's npans == 2 * ntracks factors (NULL: no pan), every one and the master's gain
// finite; (1.0, 1.0) for every other track
int seq_desk(const char* fn, const double* pans, uint32_t npans, double master_gain, SeqDesk& out) {
    for (uint32_t i = 0; i < 2 * shq::MAX_TRACKS; ++i) out.pan[i] = 1.0;
    for (uint32_t i = 0; pans && i < npans; ++i) {
        if (!isfinite(pans[i])) return sh::set_error(SH_ERR_INVALID, "%s: pan %u: %s factor is not finite", fn, i / 2, i % 2 ? "right" : "left");
        out.pan[i] = pans[i];
    }
    if (!isfinite(master_gain)) return sh::set_error(SH_ERR_INVALID, "%s: master gain is not finite", fn);
    out.master = master_gain;
    return SH_OK;
}

// The refusals that every render with a desk shares (seq_render_desk, seq_render_grouped), behind their own NULL checks and in the order
// both report them: no tracks; automation (where given) at width 3 or made for another song; pans on a
// mono song; the gains' count; the pans' count.
int seq_desk_args(const char* fn, const sh_seq* seq, const sh_seq_auto* automation, const double* gains, uint32_t ngains, const double* pans, uint32_t npans) {
    if (!seq->ntracks) return sh::set_error(SH_ERR_INVALID, "%s: the song has no tracks (sh_seq_create_tracks makes one that has)", fn);
    if (automation) {
        if (seq->width == 3) return sh::set_error(SH_ERR_INVALID, "%s: width 3: a fader move's fade has no 24-bit form", fn);
        if (automation->ntracks != seq->ntracks || automation->width != seq->width || automation->nchannels != seq->nchannels ||
            automation->track_samples != seq->track_samples)
            return sh::set_error(SH_ERR_INVALID, "%s: the automation was made for another song (%u tracks, width %d, %d channels, %llu samples)", fn,
                                 automation->ntracks, automation->width, automation->nchannels, (unsigned long long)automation->track_samples);
    }
    if (pans && seq->nchannels != 2) return sh::set_error(SH_ERR_INVALID, "%s: pans need a stereo song, this one has %d channels", fn, seq->nchannels);
    if (gains && ngains != seq->ntracks) return sh::set_error(SH_ERR_INVALID, "%s: %u gains for %u tracks", fn, ngains, seq->ntracks);
    if (pans && npans != 2 * seq->ntracks) return sh::set_error(SH_ERR_INVALID, "%s: %u pan factors for %u tracks (two each)", fn, npans, seq->ntracks);
    return SH_OK;
}

// the table of an automation's handle as the kernels take it (none: NULL pointers, no moves)
SeqAuto seq_auto_of(const sh_seq_auto* a) {
    if (!a) return SeqAuto{nullptr, nullptr};
    return SeqAuto{(const she::Seg*)a->block, (const uint32_t*)((const char*)a->block + a->at_first)};
}

// What a render is told beside the handle and the window (every entry point fills what it has; sh_seq_render nothing).  told: the entry
// point says rides, pans, history and clips; seq_render reads the rest off the handle and the pointers.
struct SeqCall {
    const SeqGains* gains = nullptr;      // NULL: every track at 1.0
    void* meters = nullptr;               // host rows: ntracks + 1 (+ ngroups with groups); told.history: a table of BLOCKS, nblocks * nrows rows -- the device
                                          // table is then the library's scratch, sized for the call, and needs no zeroing; told.clips: rows of 48 bytes
    const SeqDesk* desk = nullptr;        // the pans and the master's gain; the handle has tracks
    const SeqAuto* au = nullptr;          // with a desk; told.rides: its table has a segment on a bus lane, told.pans: on a pan lane
    const shg::Table* groups = nullptr;   // with a desk, with or without au; the empty table where au rides the master or tracks' pans alone
    uint64_t stride = 0; uint32_t nplanes = 0;      // stems (nplanes != 0): the planes' stride in bytes and their count, checked by the caller against
                                          // `out`; with groups, no meters; out_sample is plane 0's
    shb::Call told{};
};
int seq_render(const char* fn, const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const SeqCall& call = SeqCall()) {
    static_assert(sizeof(sh_seq_meter) == sizeof(shmt::Row) && offsetof(sh_seq_meter, sq_hi) == offsetof(shmt::Row, sq_hi) &&
                  offsetof(sh_seq_meter, sq_lo) == offsetof(shmt::Row, sq_lo), "sh_seq_meter is shmt::Row");
    static_assert(sizeof(sh_seq_meter_clips) == sizeof(shcl::Row) && offsetof(sh_seq_meter_clips, sq_hi) == offsetof(sh_seq_meter, sq_hi) &&
                  offsetof(sh_seq_meter_clips, sq_lo) == offsetof(sh_seq_meter, sq_lo) && offsetof(sh_seq_meter_clips, clipped) == sizeof(shmt::Row),
                  "sh_seq_meter_clips is shcl::Row: sh_seq_meter, then the counts");
    shb::Call told = call.told;
    told.tracks = seq->ntracks != 0, told.width = seq->width, told.stems = call.nplanes != 0;
    told.meters = call.meters != nullptr, told.desk = call.desk != nullptr, told.automation = call.au != nullptr, told.groups = call.groups != nullptr;
    void* const meters = call.meters;
    const shg::Table* const groups = call.groups;
    const bool history = told.history, clips = told.clips;
    const size_t b_rows = meters ? ((size_t)seq->ntracks + 1 + (groups ? groups->n : 0)) * (clips ? sizeof(shcl::Row) : sizeof(shmt::Row)) : 0;
    const size_t w = (size_t)seq->width;
    if (first_sample > seq->track_samples || nsamples > seq->track_samples - first_sample)
        return sh::set_error(SH_ERR_INVALID, "%s: range outside the song", fn);
    const size_t have = out->bytes / w;
    if (out_sample > have || nsamples > have - out_sample) return sh::set_error(SH_ERR_INVALID, "%s: range outside out", fn);
    if (!nsamples) {
        if (meters && !history) memset(meters, 0, b_rows);    // an empty window: every level 0 (a history: no block)
        return SH_OK;
    }
    const char* o0 = (const char*)out->ptr + out_sample * w;
    const char* o1 = o0 + nsamples * w;
    if (told.stems) {                                         // from the first sample of plane 0 to the last of the last plane, gaps included
        const char* s1 = o0 + shst::span(call.nplanes, call.stride / w, nsamples) * w;
        for (size_t v = 0; v < seq->src_lo.size(); ++v)
            if (shst::overlaps((uint64_t)(uintptr_t)o0, (uint64_t)(uintptr_t)s1, (uint64_t)(uintptr_t)seq->src_lo[v], (uint64_t)(uintptr_t)seq->src_hi[v]))
                return sh::set_error(SH_ERR_INVALID, "%s: the span of the %u planes overlaps a source of the song", fn, call.nplanes);
    }
    for (size_t v = 0; v < seq->src_lo.size(); ++v)
        if (seq->src_lo[v] < o1 && o0 < seq->src_hi[v]) return sh::set_error(SH_ERR_INVALID, "%s: out overlaps a source of the song", fn);
    const uint32_t lo = (uint32_t)first_sample, hi = (uint32_t)(first_sample + nsamples), tile = shq::tile_samples(seq->width);
    const uint32_t nt = shhs::nblocks(lo, hi, tile);          // the song tiles of the window: its workgroups, and a history's blocks
    // the store's base, biased so that song sample s lands on out[out_sample + s - first_sample]: integer address arithmetic
    void* biased = (void*)((uintptr_t)out->ptr + w * (uintptr_t)out_sample - w * (uintptr_t)first_sample);
    const dim3 grid = sh::grid1d(nt, 1);
    hipStream_t st = sh::state().stream;
    const size_t b_meters = history ? (size_t)nt * b_rows : b_rows;      // (a history: a block of rows per tile of the window, shhs::nblocks)
    char* table = (char*)seq->block + seq->at_meters;         // (the handle's: one metered render at a time)
    if (history) {                                            // the library's scratch, in front of the launch: every block has one writer, no memset
        const int rc = sh::ensure_scratch(b_meters);
        if (rc) return rc;
        table = (char*)sh::state().scratch;
    } else if (meters) SH_HIP(hipMemsetAsync(table, 0, b_meters, st));
    SeqBusOf<shb::PARTS> bus{};                               // every part a bus may carry (no automation: NULL pointers, no moves); the route takes its own
    if (call.desk) static_cast<SeqDesk&>(bus) = *call.desk;
    if (call.au) static_cast<SeqAuto&>(bus) = *call.au;
    if (groups) bus.groups = *groups;
    bus.stride = call.stride;
    if (seq->ntracks) {
        bus.rfirst = (const uint32_t*)((const char*)seq->block + seq->at_rfirst);
        bus.runs = (const shq::Run*)((const char*)seq->block + seq->at_runs);
        if (call.gains) bus.gains = *call.gains;
        else seq_gains(fn, nullptr, 0, bus.gains);
        bus.meters = (shmt::Row*)table;
        bus.ntracks = seq->ntracks;
        bus.nch = (uint32_t)seq->nchannels;
    }
    const uint32_t route = shb::route(told);
    seq_with_level(seq->level, [&](auto L) {
        constexpr int LEVEL = decltype(L)::value;
        if (route == shb::NO_BUS) seq_window_launch<LEVEL>(seq, grid, st, lo, hi, biased);
        else seq_with_bus(route, [&](auto F) { seq_window_launch<LEVEL>(seq, grid, st, lo, hi, biased, seq_bus_parts<decltype(F)::value>(bus)); });
    });
    SH_CHECK_LAUNCH(fn);
    if (meters) {                                             // synchronous, as sh_pcm_stats: one small copy, one wait
        SH_HIP(hipMemcpyAsync(meters, table, b_meters, hipMemcpyDeviceToHost, st));
        SH_HIP(hipStreamSynchronize(st));
    }
    return SH_OK;
}

}  // namespace

extern "C" {

int sh_seq_create(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_chan* events, uint32_t nevents,
                  const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, size_t track_samples, sh_seq** out) {
    SH_REQUIRE_INIT();
    return seq_create("sh_seq_create", srcs, nsrc, events, nevents, nullptr, 0, false, segments, nsegments, width, nchannels, track_samples, out);
}

int sh_seq_create_tracks(const sh_buf* const* srcs, uint32_t nsrc, const sh_mix_event_chan* events, uint32_t nevents, const uint32_t* track_first,
                         uint32_t ntracks, const sh_env_segment* segments, uint32_t nsegments, int width, int nchannels, size_t track_samples,
                         sh_seq** out) {
    SH_REQUIRE_INIT();
    return seq_create("sh_seq_create_tracks", srcs, nsrc, events, nevents, track_first, ntracks, true, segments, nsegments, width, nchannels,
                      track_samples, out);
}

int sh_seq_render(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_seq_render";
    if (!seq || !out) return seq_null(fn);
    return seq_render(fn, seq, first_sample, nsamples, out, out_sample);
}

int sh_seq_render_gains(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                        uint32_t ngains) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_seq_render_gains";
    if (!seq || !out || !gains) return seq_null(fn);
    if (!seq->ntracks) return sh::set_error(SH_ERR_INVALID, "%s: the song has no tracks (sh_seq_create_tracks makes one that has)", fn);
    if (ngains != seq->ntracks) return sh::set_error(SH_ERR_INVALID, "%s: %u gains for %u tracks", fn, ngains, seq->ntracks);
    SeqGains g;
    const int rc = seq_gains(fn, gains, ngains, g);
    if (rc) return rc;
    SeqCall call;
    call.gains = &g;
    return seq_render(fn, seq, first_sample, nsamples, out, out_sample, call);
}

int sh_seq_render_meters(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                         uint32_t ngains, sh_seq_meter* meters, uint32_t nmeters) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_seq_render_meters";
    if (!seq || !out || !meters || (!gains && ngains)) return seq_null(fn);
    if (!seq->ntracks) return sh::set_error(SH_ERR_INVALID, "%s: the song has no tracks (sh_seq_create_tracks makes one that has)", fn);
    if (gains && ngains != seq->ntracks) return sh::set_error(SH_ERR_INVALID, "%s: %u gains for %u tracks", fn, ngains, seq->ntracks);
    if (nmeters != seq->ntracks + 1) return sh::set_error(SH_ERR_INVALID, "%s: %u rows for %u tracks and the master", fn, nmeters, seq->ntracks);
    SeqGains g;
    const int rc = seq_gains(fn, gains, ngains, g);
    if (rc) return rc;
    SeqCall call;
    call.gains = &g, call.meters = meters;
    return seq_render(fn, seq, first_sample, nsamples, out, out_sample, call);
}

// sh_seq_auto_create (buses false: ntracks lanes) and sh_seq_auto_create_buses (ntracks + 1 + ngroups lanes in the meter table's row order)
// behind their names: sha::check's verdict in words, then the table on the device.  Who a lane is: a track, the master or a group.
// sh_seq_auto_create_pans (pans true): the bus lanes and, in pan_segments and pan_first, ntracks + ngroups pan lanes held to shp::check.
static int seq_auto_make(const char* fn, const sh_seq* seq, const sh_env_segment* segments, uint32_t nsegments, const uint32_t* seg_first,
                         uint32_t ntracks, uint32_t ngroups, bool buses, sh_seq_auto** out, bool pans = false,
                         const sh_env_segment* pan_segments = nullptr, uint32_t npan = 0, const uint32_t* pan_first = nullptr) {
    if (!out) return seq_null(fn);
    *out = nullptr;
    if (!seq || !seg_first || (nsegments && !segments)) return seq_null(fn);
    if (pans && (!pan_first || (npan && !pan_segments))) return seq_null(fn);
    if (!seq->ntracks) return sh::set_error(SH_ERR_INVALID, "%s: the song has no tracks (sh_seq_create_tracks makes one that has)", fn);
    if (seq->width == 3) return sh::set_error(SH_ERR_INVALID, "%s: width 3: a fader move's fade has no 24-bit form", fn);
    if (ntracks != seq->ntracks) return sh::set_error(SH_ERR_INVALID, "%s: %u lanes for %u tracks", fn, ntracks, seq->ntracks);
    if (buses && ngroups > shg::MAX_GROUPS) return sh::set_error(SH_ERR_INVALID, "%s: %u group lanes, 0 to %u", fn, ngroups, shg::MAX_GROUPS);
    if (pans && seq->nchannels != 2) return sh::set_error(SH_ERR_INVALID, "%s: a pan needs a stereo song, this one has %d channels", fn, seq->nchannels);
    const uint32_t nlanes = buses ? sha::lanes(ntracks, ngroups) : ntracks;
    const sha::Verdict v = sha::check(segments, nsegments, seg_first, nlanes, seq->track_samples);
    char who[32];
    if (v.lane < ntracks || !buses) snprintf(who, sizeof who, "track %u", v.lane);
    else if (v.lane == ntracks) snprintf(who, sizeof who, "master");
    else snprintf(who, sizeof who, "group %u", v.lane - ntracks - 1);
    const uint32_t k = v.segment;
    switch (v.why) {
    case sha::OK: break;
    case sha::FIRST_ENDS: return sh::set_error(SH_ERR_INVALID, "%s: seg_first starts at 0 and ends at nsegments", fn);
    case sha::FIRST_DECREASES: return sh::set_error(SH_ERR_INVALID, "%s: seg_first decreases at %s", fn, who);
    case sha::RESERVED: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: reserved must be 0", fn, who, k);
    case sha::ENDS: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: ends not ascending or beyond the song", fn, who, k);
    case sha::KIND: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: kind %u not 0 or 1", fn, who, k, segments[seg_first[v.lane] + k].kind);
    case sha::MUL: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: mul must be 1.0 (a track's gain is the render's)", fn, who, k);
    case sha::ORIGIN: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: a move's origin is its first sample", fn, who, k);
    case sha::NUMSAMPLES: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: numsamples shorter than the move", fn, who, k);
    default: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: a volume is not finite or outside 0 .. 1", fn, who, k);
    }
    if (pans) {                                               // the pan lanes: the tracks', then the groups'
        const shp::Verdict p = shp::check(pan_segments, npan, pan_first, shp::lanes(ntracks, ngroups), seq->track_samples);
        if (p.lane < ntracks) snprintf(who, sizeof who, "track %u pan", p.lane);
        else snprintf(who, sizeof who, "group %u pan", p.lane - ntracks);
        const uint32_t j = p.segment;
        switch (p.why) {
        case shp::OK: break;
        case shp::FIRST_ENDS: return sh::set_error(SH_ERR_INVALID, "%s: pan_first starts at 0 and ends at npan_segments", fn);
        case shp::FIRST_DECREASES: return sh::set_error(SH_ERR_INVALID, "%s: pan_first decreases at %s", fn, who);
        case shp::RESERVED: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: reserved must be 0", fn, who, j);
        case shp::ENDS: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: ends not ascending or beyond the song", fn, who, j);
        case shp::ODD: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: an odd end (a pan segment holds whole frames)", fn, who, j);
        case shp::KIND: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: kind %u not 0 or 3", fn, who, j, pan_segments[pan_first[p.lane] + j].kind);
        case shp::MUL: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: mul must be 1.0", fn, who, j);
        case shp::ORIGIN: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: a move's origin is its first sample", fn, who, j);
        case shp::NUMSAMPLES: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: numsamples smaller than the move's frames", fn, who, j);
        default: return sh::set_error(SH_ERR_INVALID, "%s: %s: segment %u: a pan is not finite or outside -1 .. 1", fn, who, j);
        }
    }
    sh_seq_auto* a = new (std::nothrow) sh_seq_auto;
    if (!a) return sh::set_error(SH_ERR_NOMEM, "host allocation failed");
    a->ntracks = ntracks;
    a->nsegments = nsegments;
    a->width = seq->width;
    a->nchannels = seq->nchannels;
    a->track_samples = seq->track_samples;
    // with bus lanes the table holds an offset for EVERY group lane a render may name (the kernels read afirst[row0 + g + 1] for g < the
    // render's groups): the lanes that were not given are empty, at nsegments
    const size_t noffsets = buses ? (size_t)sha::lanes(ntracks, shg::MAX_GROUPS) + 1 : (size_t)ntracks + 1;
    if (buses) {
        a->ngroups = ngroups;
        for (uint32_t g = 0; g < ngroups; ++g)
            if (seg_first[ntracks + 1 + g] < seg_first[ntracks + 2 + g]) a->ridden = g + 1;
        a->buses = a->ridden != 0 || seg_first[ntracks] < seg_first[ntracks + 1];
    }
    // with pan lanes the pan segments follow the others and their offsets the others', for every track and every group lane a render may
    // name (shp::track_lane, shp::group_lane), counted from the table's first segment as the others are
    const size_t npanoffsets = pans ? (size_t)shp::lanes(ntracks, shg::MAX_GROUPS) + 1 : 0;
    if (pans) {
        const uint32_t npanlanes = shp::lanes(ntracks, ngroups);
        for (uint32_t g = 0; g < ngroups; ++g)
            if (pan_first[ntracks + g] < pan_first[ntracks + g + 1]) a->panned = g + 1;
        a->pans = pan_first[npanlanes] != 0;
    }
    a->at_first = ((size_t)nsegments + npan) * sizeof(she::Seg);
    a->bytes = a->at_first + (noffsets + npanoffsets) * 4;
    std::vector<char> host(a->bytes);
    seq_segments(reinterpret_cast<she::Seg*>(host.data()), segments, nsegments);
    if (pans) seq_segments(reinterpret_cast<she::Seg*>(host.data()) + nsegments, pan_segments, npan);
    uint32_t* first = reinterpret_cast<uint32_t*>(host.data() + a->at_first);
    memcpy(first, seg_first, ((size_t)nlanes + 1) * 4);
    for (size_t i = (size_t)nlanes + 1; i < noffsets; ++i) first[i] = nsegments;
    if (pans) {
        const uint32_t npanlanes = shp::lanes(ntracks, ngroups);
        for (size_t i = 0; i < npanoffsets; ++i) first[noffsets + i] = nsegments + (i <= npanlanes ? pan_first[i] : npan);
    }
    int rc = sh::pool_alloc(a->bytes, &a->block, &a->cap);
    if (rc) {
        delete a;
        return rc;
    }
    hipStream_t st = sh::state().stream;
    hipError_t e = hipMemcpyAsync(a->block, host.data(), host.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);        // once per automation: the host copy goes when this returns
    if (e != hipSuccess) {
        sh::pool_free(a->block, a->cap);
        delete a;
        return sh::hip_error(e, fn);
    }
    *out = a;
    return SH_OK;
}

int sh_seq_auto_create(const sh_seq* seq, const sh_env_segment* segments, uint32_t nsegments, const uint32_t* seg_first, uint32_t ntracks,
                       sh_seq_auto** out) {
    SH_REQUIRE_INIT();
    return seq_auto_make("sh_seq_auto_create", seq, segments, nsegments, seg_first, ntracks, 0, false, out);
}

int sh_seq_auto_create_buses(const sh_seq* seq, const sh_env_segment* segments, uint32_t nsegments, const uint32_t* seg_first, uint32_t ntracks,
                             uint32_t ngroups, sh_seq_auto** out) {
    SH_REQUIRE_INIT();
    return seq_auto_make("sh_seq_auto_create_buses", seq, segments, nsegments, seg_first, ntracks, ngroups, true, out);
}

int sh_seq_auto_create_pans(const sh_seq* seq, const sh_env_segment* segments, uint32_t nsegments, const uint32_t* seg_first, uint32_t ntracks,
                            uint32_t ngroups, const sh_env_segment* pan_segments, uint32_t npan_segments, const uint32_t* pan_first,
                            sh_seq_auto** out) {
    SH_REQUIRE_INIT();
    return seq_auto_make("sh_seq_auto_create_pans", seq, segments, nsegments, seg_first, ntracks, ngroups, true, out, true, pan_segments, npan_segments,
                         pan_first);
}

int sh_seq_auto_destroy(sh_seq_auto* a) {
    if (!a) return SH_OK;
    SH_API_LOCK();
    if (a->block && sh::state().initialized) {
        if (sh::has_pending()) sh::flush_pending();
        sh::pool_free(a->block, a->cap);                      // (stream-ordered reuse: a render still in flight finishes first)
    }
    delete a;
    return SH_OK;
}

// sh_seq_render_desk (automation NULL) and sh_seq_render_auto behind their names
static int seq_render_desk(const char* fn, const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                           uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter* meters, uint32_t nmeters,
                           const sh_seq_auto* automation) {
    if (!seq || !out || (!gains && ngains) || (!pans && npans) || (!meters && nmeters)) return seq_null(fn);
    int rc = seq_desk_args(fn, seq, automation, gains, ngains, pans, npans);
    if (rc) return rc;
    if (meters && nmeters != seq->ntracks + 1) return sh::set_error(SH_ERR_INVALID, "%s: %u rows for %u tracks and the master", fn, nmeters, seq->ntracks);
    SeqGains g;
    SeqDesk d;
    rc = seq_gains(fn, gains, ngains, g);
    if (!rc) rc = seq_desk(fn, pans, npans, master_gain, d);
    if (rc) return rc;
    const SeqAuto au = seq_auto_of(automation);
    SeqCall call;
    call.gains = &g, call.meters = meters, call.desk = &d, call.au = automation ? &au : nullptr;
    shg::Table none;
    if (automation && automation->ridden)
        return sh::set_error(SH_ERR_INVALID, "%s: the automation rides group %u, which this call does not name (sh_seq_render_groups does)", fn,
                             automation->ridden - 1);
    if (automation && automation->panned)
        return sh::set_error(SH_ERR_INVALID, "%s: the automation rides the pan of group %u, which this call does not name (sh_seq_render_groups does)", fn,
                             automation->panned - 1);
    if (automation && (automation->buses || automation->pans)) {      // a master ride or tracks' pan rides alone: the kernels that ride, an empty group table
        shg::pack(nullptr, 0, seq->ntracks, none);
        call.groups = &none, call.told.rides = true, call.told.pans = automation->pans;
    }
    return seq_render(fn, seq, first_sample, nsamples, out, out_sample, call);
}

int sh_seq_render_desk(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                       uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter* meters, uint32_t nmeters) {
    SH_REQUIRE_INIT();
    return seq_render_desk("sh_seq_render_desk", seq, first_sample, nsamples, out, out_sample, gains, ngains, pans, npans, master_gain, meters, nmeters, nullptr);
}

int sh_seq_render_auto(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                       uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter* meters, uint32_t nmeters,
                       const sh_seq_auto* automation) {
    SH_REQUIRE_INIT();
    if (!automation) return seq_null("sh_seq_render_auto");
    return seq_render_desk("sh_seq_render_auto", seq, first_sample, nsamples, out, out_sample, gains, ngains, pans, npans, master_gain, meters, nmeters, automation);
}

// sh_seq_render_groups (history false: meters is NULL or nmeters == ntracks + 1 + ngroups rows, at least one group) and
// sh_seq_render_history (history true: meters is nblocks blocks of nmeters rows each, groups and automation may be none) and
// sh_seq_render_clips (history and clips true: the same, the rows sh_seq_meter_clips) and sh_seq_render_stems (stems: no meters, groups
// and automation may be none, any automation; the planes' geometry is checked here, behind the desk's refusals) behind their names
struct SeqStemsArgs { size_t plane_samples; uint32_t nplanes; };
static int seq_render_grouped(const char* fn, bool history, const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample,
                              const double* gains, uint32_t ngains, const double* pans, uint32_t npans, double master_gain, void* meters,
                              uint32_t nmeters, uint32_t nblocks, const sh_seq_auto* automation, const sh_seq_group* groups, uint32_t ngroups,
                              bool clips = false, const SeqStemsArgs* stems = nullptr) {
    static_assert(sizeof(sh_seq_group) == sizeof(shg::Group) && offsetof(sh_seq_group, gain) == offsetof(shg::Group, gain) &&
                  offsetof(sh_seq_group, right) == offsetof(shg::Group, right) && SH_SEQ_MAX_GROUPS == shg::MAX_GROUPS, "sh_seq_group is shg::Group");
    if (!seq || !out || (!gains && ngains) || (!pans && npans) || (!meters && nmeters && !history)) return seq_null(fn);
    int rc = seq_desk_args(fn, seq, automation, gains, ngains, pans, npans);
    if (rc) return rc;
    const bool nogroups = history || stems;                   // (a history and stems: ngroups may be 0)
    if ((ngroups == 0 && !nogroups) || ngroups > shg::MAX_GROUPS)
        return sh::set_error(SH_ERR_INVALID, "%s: %u groups, %u to %u", fn, ngroups, nogroups ? 0u : 1u, shg::MAX_GROUPS);
    if (!groups && ngroups) return seq_null(fn);
    const shg::Group* gs = reinterpret_cast<const shg::Group*>(groups);
    const shg::Verdict v = ngroups ? shg::check(gs, ngroups, seq->ntracks, seq->nchannels) : shg::Verdict{shg::OK, 0};
    static const sh_seq_group nogroup{};
    const sh_seq_group& b = ngroups ? groups[v.entry] : nogroup;
    switch (v.why) {
    case shg::OK: break;
    case shg::RANGE_EMPTY: return sh::set_error(SH_ERR_INVALID, "%s: group %u: tracks [%u, %u): an empty range", fn, v.entry, b.first, b.end);
    case shg::RANGE_BEYOND: return sh::set_error(SH_ERR_INVALID, "%s: group %u: tracks [%u, %u) of %u", fn, v.entry, b.first, b.end, seq->ntracks);
    case shg::RANGE_ORDER:
        return sh::set_error(SH_ERR_INVALID, "%s: group %u: starts at track %u, in front of the end of the group before it", fn, v.entry, b.first);
    case shg::GAIN_NOT_FINITE: return sh::set_error(SH_ERR_INVALID, "%s: group %u: gain is not finite", fn, v.entry);
    case shg::PAN_NOT_FINITE: return sh::set_error(SH_ERR_INVALID, "%s: group %u: left / right is not finite", fn, v.entry);
    case shg::PAN_NOT_STEREO:
        return sh::set_error(SH_ERR_INVALID, "%s: group %u: a pan needs a stereo song, this one has %d channels", fn, v.entry, seq->nchannels);
    default: return sh::set_error(SH_ERR_INVALID, "%s: %u groups, %u to %u", fn, ngroups, nogroups ? 0u : 1u, shg::MAX_GROUPS);
    }
    SeqCall call;
    if (stems) {                                              // the planes' geometry (seqstem.hpp), each refusal by a message of its own
        const size_t w = (size_t)seq->width;
        switch (shst::check(stems->nplanes, seq->ntracks, ngroups, stems->plane_samples, nsamples, out_sample, out->bytes / w)) {
        case shst::OK: break;
        case shst::PLANES:
            return sh::set_error(SH_ERR_INVALID, "%s: %u planes for %u tracks, the master and %u groups", fn, stems->nplanes, seq->ntracks, ngroups);
        case shst::STRIDE:
            return sh::set_error(SH_ERR_INVALID, "%s: planes %llu samples apart for a window of %llu: they would overlap", fn,
                                 (unsigned long long)stems->plane_samples, (unsigned long long)nsamples);
        default:
            return sh::set_error(SH_ERR_INVALID, "%s: the last of %u planes ends outside out (%llu samples from sample %llu on, planes %llu apart)", fn,
                                 stems->nplanes, (unsigned long long)(out->bytes / w), (unsigned long long)out_sample, (unsigned long long)stems->plane_samples);
        }
        call.stride = shst::stride_bytes(stems->plane_samples, (uint32_t)seq->width), call.nplanes = stems->nplanes;
    }
    if (clips && automation && (automation->buses || automation->pans))
        return sh::set_error(SH_ERR_INVALID, "%s: the automation rides a %s: overs are not counted through rides of buses and pans yet", fn,
                             automation->pans ? "pan" : "bus");
    if (history && automation && (automation->buses || automation->pans))
        return sh::set_error(SH_ERR_INVALID, "%s: the automation rides a %s: rides of buses and pans have no history yet", fn,
                             automation->pans ? "pan" : "bus");
    if (automation && automation->ridden > ngroups)
        return sh::set_error(SH_ERR_INVALID, "%s: the automation rides group %u, and this call names %u groups", fn, automation->ridden - 1, ngroups);
    if (automation && automation->panned > ngroups)
        return sh::set_error(SH_ERR_INVALID, "%s: the automation rides the pan of group %u, and this call names %u groups", fn, automation->panned - 1, ngroups);
    if ((meters || history) && nmeters != seq->ntracks + 1 + ngroups)
        return sh::set_error(SH_ERR_INVALID, "%s: %u rows for %u tracks, the master and %u groups", fn, nmeters, seq->ntracks, ngroups);
    if (history) {                                            // the window's blocks, counted as the kernels count them (a window outside the song: seq_render says so)
        const bool inside = first_sample <= seq->track_samples && nsamples <= seq->track_samples - first_sample;
        const uint32_t want = inside ? shhs::nblocks(first_sample, first_sample + nsamples, shq::tile_samples(seq->width)) : nblocks;
        if (nblocks != want)
            return sh::set_error(SH_ERR_INVALID, "%s: %u blocks for a window of %u (song tiles of %u samples)", fn, nblocks, want, shq::tile_samples(seq->width));
        if (!meters && nblocks) return seq_null(fn);
    }
    SeqGains g;
    SeqDesk d;
    rc = seq_gains(fn, gains, ngains, g);
    if (!rc) rc = seq_desk(fn, pans, npans, master_gain, d);
    if (rc) return rc;
    shg::Table table;
    shg::pack(gs, ngroups, seq->ntracks, table);
    const SeqAuto au = seq_auto_of(automation);
    call.gains = &g, call.meters = meters, call.desk = &d, call.au = automation ? &au : nullptr, call.groups = &table;
    call.told.rides = automation && (automation->buses || automation->pans), call.told.pans = automation && automation->pans;
    call.told.history = history, call.told.clips = clips;
    return seq_render(fn, seq, first_sample, nsamples, out, out_sample, call);
}

int sh_seq_render_groups(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                         uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter* meters, uint32_t nmeters,
                         const sh_seq_auto* automation, const sh_seq_group* groups, uint32_t ngroups) {
    SH_REQUIRE_INIT();
    return seq_render_grouped("sh_seq_render_groups", false, seq, first_sample, nsamples, out, out_sample, gains, ngains, pans, npans, master_gain, meters,
                              nmeters, 0, automation, groups, ngroups);
}

int sh_seq_render_history(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                          uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter* rows, uint32_t nrows,
                          uint32_t nblocks, const sh_seq_auto* automation, const sh_seq_group* groups, uint32_t ngroups) {
    SH_REQUIRE_INIT();
    return seq_render_grouped("sh_seq_render_history", true, seq, first_sample, nsamples, out, out_sample, gains, ngains, pans, npans, master_gain, rows,
                              nrows, nblocks, automation, groups, ngroups);
}

int sh_seq_render_clips(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, const double* gains,
                        uint32_t ngains, const double* pans, uint32_t npans, double master_gain, sh_seq_meter_clips* rows, uint32_t nrows,
                        uint32_t nblocks, const sh_seq_auto* automation, const sh_seq_group* groups, uint32_t ngroups) {
    SH_REQUIRE_INIT();
    return seq_render_grouped("sh_seq_render_clips", true, seq, first_sample, nsamples, out, out_sample, gains, ngains, pans, npans, master_gain, rows,
                              nrows, nblocks, automation, groups, ngroups, true);
}

int sh_seq_render_stems(const sh_seq* seq, size_t first_sample, size_t nsamples, sh_buf* out, size_t out_sample, size_t plane_samples,
                        uint32_t nplanes, const double* gains, uint32_t ngains, const double* pans, uint32_t npans, double master_gain,
                        const sh_seq_auto* automation, const sh_seq_group* groups, uint32_t ngroups) {
    SH_REQUIRE_INIT();
    static const char fn[] = "sh_seq_render_stems";
    if (seq && !seq->ntracks)
        return sh::set_error(SH_ERR_INVALID, "%s: a flat song has no stems: it has no tracks (sh_seq_create_tracks makes a song that has)", fn);
    const SeqStemsArgs stems{plane_samples, nplanes};
    return seq_render_grouped(fn, false, seq, first_sample, nsamples, out, out_sample, gains, ngains, pans, npans, master_gain, nullptr, 0, 0, automation,
                              groups, ngroups, false, &stems);
}

int sh_seq_get_tracks(const sh_seq* seq, uint32_t* ntracks, uint32_t* nruns) {
    SH_API_LOCK();
    if (!seq || !ntracks || !nruns) return seq_null("sh_seq_get_tracks");
    *ntracks = seq->ntracks;
    *nruns = seq->nruns;
    return SH_OK;
}

int sh_seq_get_info(const sh_seq* seq, sh_seq_info* out) {
    SH_API_LOCK();
    if (!seq || !out) return seq_null("sh_seq_get_info");
    out->track_samples = seq->track_samples;
    out->pairs = seq->pairs;
    out->device_bytes = seq->bytes;
    out->nevents = seq->nevents;
    out->ntiles = seq->ntiles;
    out->active_tiles = seq->active_tiles;
    out->level = (uint32_t)seq->level;
    return SH_OK;
}

int sh_seq_destroy(sh_seq* seq) {
    if (!seq) return SH_OK;
    SH_API_LOCK();
    if (seq->block && sh::state().initialized) {
        if (sh::has_pending()) sh::flush_pending();
        sh::pool_free(seq->block, seq->cap);                  // (stream-ordered reuse: a render still in flight finishes first)
    }
    delete seq;
    return SH_OK;
}

}  // extern "C"
