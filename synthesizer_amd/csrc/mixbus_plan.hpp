// mixbus_plan.hpp -- the launch plan of sh_mix_bus_f32 (osc_mixbus.hip), host only, plain C++17: the library's launch code and
// tests/cpu_mixbus.cpp compile the same statement, so a test case meant for a kernel route proves on the host that it reaches it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace shm {

constexpr uint32_t MAX_FRAMES = 1u << 24;               // per launch: tiles x 512 threads must stay below 2^32 work-items
constexpr uint32_t TILE_FRAMES = 256;                   // one wave of k_mix_bus_f32: 64 lanes x 4 frames
constexpr uint32_t WAVES = 8;                           // waves per workgroup, both kernels
constexpr uint32_t DIRECT_TILES = 1536;                 // from here on the frame range alone fills the chip: k_mix_bus_direct
constexpr uint32_t SPLIT_WORKGROUPS = 1024;             // below this many (tile, group) workgroups the voices are split further ...
constexpr uint32_t MIN_GROUP_VOICES = 4 * WAVES;        // ... while every group keeps at least this many voices
constexpr size_t STREAM_BYTES = (size_t)128 << 20;      // sh::STREAM_BYTES (common.hpp; osc_mixbus.hip asserts that they agree)

// A call of more than MAX_FRAMES frames is cut into chunks; chunk c covers the frames [off, off + n) of every row and of the bus.
inline uint32_t chunks(uint32_t nframes) { return nframes ? (uint32_t)(((uint64_t)nframes + MAX_FRAMES - 1) / MAX_FRAMES) : 0; }
struct Chunk {
    uint64_t off;
    uint32_t n;
};
inline Chunk chunk(uint32_t nframes, uint32_t c) {
    const uint64_t off = (uint64_t)c * MAX_FRAMES;
    const uint64_t left = nframes - off;
    return Chunk{off, left < MAX_FRAMES ? (uint32_t)left : MAX_FRAMES};
}

struct Plan {
    uint32_t tiles;                 // 256-frame tiles
    uint32_t groups;                // voice groups of the split kernel (a power of two); 1 under direct
    uint32_t voices_per_group;
    uint32_t direct;                // k_mix_bus_direct, else k_mix_bus_f32 (and k_bus_sum when groups > 1)
    uint32_t stream;                // direct only: non-temporal row loads
    uint32_t vec;                   // may the launch issue 16-byte accesses: voices and destination on the 16-byte grid
                                    // (the split kernel asks stride % 4 == 0 per launch as well; direct implies both)
    size_t part_stride;             // float2s between the partial buses of two groups: even, so that every group's row keeps
                                    // the 16-byte grid of the scratch block
    size_t part_bytes;              // scratch the partial buses need; 0 when groups == 1
};

// One launch: nframes <= MAX_FRAMES (a chunk).  voices / bus: the device addresses the launch reads rows from and writes the
// bus to.  The partial buses live in the library's scratch block, which is on the 16-byte grid.
inline Plan plan(uint32_t nvoices, size_t stride, uint32_t nframes, uintptr_t voices, uintptr_t bus) {
    Plan p{};
    p.tiles = (uint32_t)(((uint64_t)nframes + TILE_FRAMES - 1) / TILE_FRAMES);
    const bool on_grid = (voices & 15) == 0 && (bus & 15) == 0;
    p.direct = p.tiles >= DIRECT_TILES && (stride & 3) == 0 && on_grid;
    p.groups = 1;
    // enough workgroups to cover 256 CUs several times over: split the voices into groups when the frame range alone gives too few tiles
    // (DIRECT_TILES > SPLIT_WORKGROUPS: a direct launch has one group)
    while (p.tiles * p.groups < SPLIT_WORKGROUPS && nvoices / (p.groups * 2) >= MIN_GROUP_VOICES) p.groups *= 2;
    p.voices_per_group = (nvoices + p.groups - 1) / p.groups;
    p.stream = p.direct && (size_t)nvoices * nframes * 4 > STREAM_BYTES;      // rows beyond the Infinity Cache: streaming loads
    p.vec = p.groups > 1 ? (voices & 15) == 0 : on_grid;
    p.part_stride = ((size_t)nframes + 1) & ~(size_t)1;
    p.part_bytes = p.groups > 1 ? (size_t)p.groups * p.part_stride * 8 : 0;
    return p;
}

}  // namespace shm
