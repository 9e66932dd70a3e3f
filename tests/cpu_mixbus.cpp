// Host build of synthesizer_amd/csrc/mixbus_plan.hpp for tests/test_mixbus_plan.py (g++, no GPU): the chunks of a call and the plan
// of every launch.
#include "../synthesizer_amd/csrc/mixbus_plan.hpp"

extern "C" {
uint32_t mb_chunks(uint32_t nframes) { return shm::chunks(nframes); }
// chunk c: out[0] = first frame, out[1] = frames
void mb_chunk(uint32_t nframes, uint32_t c, uint64_t* out) {
    const shm::Chunk k = shm::chunk(nframes, c);
    out[0] = k.off;
    out[1] = k.n;
}
// one launch's plan as 8 numbers: tiles, groups, voices_per_group, direct, stream, vec, part_stride, part_bytes
void mb_plan(uint32_t nvoices, uint64_t stride, uint32_t nframes, uint64_t voices, uint64_t bus, uint64_t* out) {
    const shm::Plan p = shm::plan(nvoices, (size_t)stride, nframes, (uintptr_t)voices, (uintptr_t)bus);
    const uint64_t v[8] = {p.tiles, p.groups, p.voices_per_group, p.direct, p.stream, p.vec, p.part_stride, p.part_bytes};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
}
}
