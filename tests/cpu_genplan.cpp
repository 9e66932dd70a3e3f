// csrc/genplan.hpp built for the host behind a few C functions (tests/test_genplan.py drives them through ctypes).
#include "../synthesizer_amd/csrc/genplan.hpp"
#include <cstdio>
#include <string>

using namespace shg;

namespace {
std::string tab_text(const SegTab& t) {
    std::string s = std::to_string(t.n) + "[";
    for (uint32_t i = 0; i < t.n; ++i)
        s += (i ? "," : "") + std::to_string(t.first[i]) + "+" + std::to_string(t.len[i]) + "@" + std::to_string(t.set[i]);
    return s + "]";
}
const char* out_name(Form f, Mix m) { return m != ROWS || f == ROWS_I16 ? "i16" : (f == ROWS_F64 ? "f64" : "f32"); }
int copy_out(const std::string& s, char* buf, size_t cap) {
    if (s.size() + 1 > cap) return -1;
    std::snprintf(buf, cap, "%s", s.c_str());
    return (int)s.size();
}
}  // namespace

extern "C" {

void* gp_facts(uint32_t nvoices, uint32_t lean, uint32_t lean_fm, int all_lean, int has_guard, uint64_t flat_from, uint64_t flat_until,
               const uint64_t* short_piece_end, const uint64_t* corners, uint32_t ncorners) {
    BankFacts* F = new BankFacts;
    F->nvoices = nvoices; F->lean_candidates = lean; F->lean_fm_candidates = lean_fm;
    F->all_lean = all_lean != 0; F->has_guard = has_guard != 0;
    F->env_flat_from = flat_from; F->env_flat_until = flat_until;
    for (int k = 0; k < 34; ++k) F->short_piece_end[k] = short_piece_end[k];
    F->env_corners.assign(corners, corners + ncorners);
    return F;
}
void gp_free(void* f) { delete (BankFacts*)f; }
int gp_seg_max(void) { return SEG_MAX; }
int gp_no_general_voice(const void* f, uint64_t start, uint32_t n) { return ((const BankFacts*)f)->no_general_voice(start, n); }
int gp_lean_bank(const void* f, int reads_rows, uint32_t n) { return lean_bank(*(const BankFacts*)f, reads_rows != 0, n); }
uint32_t gp_plan_segments(const void* f, uint64_t start, uint32_t n, uint64_t T, uint64_t max_len, int corners, uint32_t* seg_first) {
    return plan_segments(*(const BankFacts*)f, start, n, T, max_len, corners != 0, seg_first);
}

// The plan in the notation of the recorded route table (one line per record-set decision, launch, temporary and stretch), in the
// order the executor follows: a two-step stretch's rows are allocated before its first step's records, a fused stretch's planes behind them;
// returns the text's length, -1 when it does not fit, -2 when the plan refuses the call.
int gp_plan_routes(const void* f, uint64_t start, uint32_t nframes, int form, int reads_rows, int no_seg, char* buf, size_t cap) {
    const Call c{start, nframes, (Form)form, reads_rows != 0};
    const Plan p = plan(*(const BankFacts*)f, c, no_seg != 0);
    if (p.refused) return -2;
    std::string s;
    char line[512];
    for (const Step& st : p.steps) {
        const unsigned long long at = start + st.first;
        if (st.opens && st.mix != ROWS) {
            std::snprintf(line, sizeof line, "M %s %llu %u\n", st.mix == FUSED ? "fused" : "two", (unsigned long long)(start + st.stretch_first), st.stretch_n);
            s += line;
        }
        if (st.opens && st.mix == TWO_STEP) s += "T " + std::to_string(st.temp_bytes) + "\n";
        if (st.records == ONE_SET) std::snprintf(line, sizeof line, "R one %llu %u\n", at, st.n);
        else if (st.records == EQUAL_SETS) std::snprintf(line, sizeof line, "R eq %u %llu %u\n", st.nseg, at, st.n);
        else std::snprintf(line, sizeof line, "R var %u %llu ", st.nseg, at);
        s += line;
        if (st.records == TABLE_SETS) {
            for (uint32_t k = 0; k <= st.nseg; ++k) s += (k ? "," : "") + std::to_string(st.seg_first[k]);
            s += "\n";
        }
        if (st.mix == FUSED) s += "T " + std::to_string(st.temp_bytes) + "\n";
        const char* T = out_name(c.form, st.mix);
        for (const Launch& l : st.launches) {
            const unsigned long long lat = at + l.first;
            switch (l.kernel) {
            case LEAN_HARM:
                std::snprintf(line, sizeof line, "L lean<%d,%s,%d,%d> grid=%ux%u n=%u segf=%u split=%u tab=", l.fpl, T, (int)l.fold, (int)l.guard, l.gx, l.gy, l.n, l.seg_frames, l.split);
                s += line + tab_text(l.tab) + "\n";
                break;
            case LISTS:
                std::snprintf(line, sizeof line, "L lists<%d,%s> grid=%ux%u at=%llu n=%u split=%u seg=%u tab=", (int)l.lean, T, l.gx, l.gy, lat, l.n, l.split, l.set);
                s += line + tab_text(l.tab) + "\n";
                break;
            case GENERATE:
                std::snprintf(line, sizeof line, "L gen<%d> %s grid=%ux%u at=%llu n=%u vpg=%u\n", l.fpl, T, l.gx, l.gy, lat, l.n, l.split);
                s += line;
                break;
            default:
                std::snprintf(line, sizeof line, "L %s grid=%u n=%u planes=%u\n", l.kernel == COMBINE ? "combine" : "compose", l.gx, l.n, l.split);
                s += line;
            }
        }
        if (st.closes && st.mix == TWO_STEP) {
            std::snprintf(line, sizeof line, "C chain%s n=%u stride=%zu\n", c.form == MIXDOWN_MAPS ? "_parts" : "", st.stretch_n, ((size_t)st.stretch_n + 63) & ~(size_t)63);
            s += line;
        }
    }
    return copy_out(s, buf, cap);
}

// Every field of the plan, for the invariants: "S first n records nseg mix stretch_first stretch_n temp opens closes cut,cut,.."
// per step and "X kernel fpl lean fold guard gx gy first n set seg_frames split tab" per launch; "F fused" last.
int gp_plan_fields(const void* f, uint64_t start, uint32_t nframes, int form, int reads_rows, int no_seg, char* buf, size_t cap) {
    const Plan p = plan(*(const BankFacts*)f, Call{start, nframes, (Form)form, reads_rows != 0}, no_seg != 0);
    if (p.refused) return -2;
    std::string s;
    char line[512];
    for (const Step& st : p.steps) {
        std::snprintf(line, sizeof line, "S %u %u %d %u %d %u %u %zu %d %d ", st.first, st.n, (int)st.records, st.nseg, (int)st.mix, st.stretch_first, st.stretch_n,
                      st.temp_bytes, (int)st.opens, (int)st.closes);
        s += line;
        for (uint32_t k = 0; k <= (st.records == TABLE_SETS ? st.nseg : 0); ++k) s += (k ? "," : "") + std::to_string(st.seg_first[k]);
        s += "\n";
        for (const Launch& l : st.launches) {
            std::snprintf(line, sizeof line, "X %d %d %d %d %d %u %u %u %u %u %u %u ", (int)l.kernel, l.fpl, (int)l.lean, (int)l.fold, (int)l.guard, l.gx, l.gy, l.first, l.n,
                          l.set, l.seg_frames, l.split);
            s += line + tab_text(l.tab) + "\n";
        }
    }
    s += "F " + std::to_string(p.fused) + "\n";
    return copy_out(s, buf, cap);
}

}  // extern "C"
