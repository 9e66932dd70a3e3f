// csrc/seqbus.hpp built for the host behind a few C functions (tests/test_seqroute.py drives them through ctypes): the table of routes, the
// width rule and the route of a call.  With SEQROUTE_MAIN it is a program of its own (its own main: every call there is, against the
// properties restated in place), which a sanitizer build can run as it stands.
#include "../synthesizer_amd/csrc/seqbus.hpp"

// a call from its flags in the order of shb::Call's fields: bit 0 tracks, 1 meters, 2 desk, 3 automation, 4 groups, 5 rides, 6 pans,
// 7 history, 8 clips, 9 stems
static shb::Call call_of(uint32_t flags, int width) {
    auto bit = [&](int i) { return ((flags >> i) & 1u) != 0; };
    return shb::Call{bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8), bit(9), width};
}

extern "C" {

uint32_t sr_nroutes() { return shb::NROUTES; }
uint32_t sr_route_at(uint32_t i) { return shb::ROUTES[i]; }
uint32_t sr_no_bus() { return shb::NO_BUS; }
uint32_t sr_bit(uint32_t i) {
    const uint32_t bits[] = {shb::METERS, shb::DESK, shb::AUTO, shb::GROUPS, shb::RIDES, shb::PANS, shb::HISTORY, shb::CLIPS, shb::STEMS};
    return bits[i];
}
int sr_known(uint32_t mask) { return shb::known(mask); }
int sr_valid_at(uint32_t mask, int width) { return shb::valid_at(mask, width); }
uint32_t sr_route(uint32_t flags, int width) { return shb::route(call_of(flags, width)); }

}  // extern "C"

// the route is a constant expression: what sequence.hip's dispatch may name as a template argument
static_assert(shb::route(shb::Call{true, false, true, false, true, false, false, false, false, false, 2}) == (shb::DESK | shb::AUTO | shb::GROUPS) &&
              shb::valid_at(shb::DESK | shb::GROUPS, 3) && !shb::valid_at(shb::DESK | shb::GROUPS, 2) && !shb::valid_at(shb::DESK | shb::RIDES, 2), "constexpr");

#ifdef SEQROUTE_MAIN
#include <cstdio>
int main() {
    // what the entry points can ask of seq_render (sequence.hip: their refusals), restated
    auto reachable = [](const shb::Call& c) {
        if (!c.tracks) return !(c.meters || c.desk || c.automation || c.groups || c.rides || c.pans || c.history || c.clips || c.stems);
        if (c.clips && !c.history) return false;
        if (c.history && !(c.meters && c.groups) ) return false;
        if ((c.automation || c.groups) && !c.desk) return false;
        if (c.automation && c.width == 3) return false;
        if (c.pans && !c.rides) return false;
        if (c.rides && !(c.automation && c.groups)) return false;
        if (c.stems && (!c.groups || c.meters)) return false;
        if (c.history && c.rides) return false;
        return true;
    };
    unsigned calls = 0, made = 0, hit[shb::NROUTES] = {};
    for (int width = 1; width <= 4; ++width)
        for (uint32_t flags = 0; flags < 1024; ++flags, ++calls) {
            const shb::Call c = call_of(flags, width);
            const uint32_t m = shb::route(c);
            if ((m == shb::NO_BUS) != !c.tracks) { printf("flags %u width %d: no bus and tracks\n", flags, width); return 1; }
            if (!reachable(c)) continue;
            ++made;
            if (!c.tracks) continue;
            if (!shb::valid_at(m, width)) { printf("flags %u width %d: mask %u has no kernels at the width\n", flags, width, m); return 1; }
            if (((m & shb::RIDES) && !c.rides) || ((m & shb::PANS) && !c.pans)) { printf("flags %u width %d: mask %u reads lanes the handle lacks\n", flags, width, m); return 1; }
            if (((m & shb::METERS) != 0) != c.meters || ((m & shb::STEMS) != 0) != c.stems || ((m & shb::HISTORY) != 0) != c.history || ((m & shb::CLIPS) != 0) != c.clips) {
                printf("flags %u width %d: mask %u loses or invents a part\n", flags, width, m);
                return 1;
            }
            for (uint32_t i = 0; i < shb::NROUTES; ++i)
                if (shb::ROUTES[i] == m) ++hit[i];
        }
    for (uint32_t i = 0; i < shb::NROUTES; ++i)
        if (!hit[i]) { printf("route %u (mask %u) is never taken\n", i, shb::ROUTES[i]); return 1; }
    for (uint32_t m = 0; m < 512; ++m)
        for (int width = 0; width <= 5; ++width)
            if (shb::valid_at(m, width) && !(shb::known(m) && width >= 1 && width <= 4)) { printf("valid_at %u %d\n", m, width); return 1; }
    printf("seqroute: %u calls, %u of them makeable, %u routes: ok\n", calls, made, (unsigned)shb::NROUTES);
    return 0;
}
#endif
