// pcmdev.hpp -- device helpers that more than one unit's PCM kernels share (every kernel lives in the unit that launches it, so
// what pcm.hip, pcm_ops.hip and sequence.hip all need is stated once, here): audioop's fbound and sample limits, and the
// byte-assembled sample access of the widths that are not 16 bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// audioop's fbound(): clamp, then round toward minus infinity
__device__ __forceinline__ int fbound(double val, double minval, double maxval) {
    if (val > maxval) val = maxval;
    else if (val < minval + 1.0) val = minval;
    return (int)floor(val);
}

template <typename T> struct Lim;
template <> struct Lim<signed char> { static constexpr double lo = -128.0, hi = 127.0; };
template <> struct Lim<short> { static constexpr double lo = -32768.0, hi = 32767.0; };
template <> struct Lim<int> { static constexpr double lo = -2147483648.0, hi = 2147483647.0; };

// sample i of a PCM buffer of WIDTH bytes per sample (1, 3, 4), sign-extended / its low bytes stored back (a 24-bit sample: GETINT24)
template <int WIDTH>
__device__ __forceinline__ long long chain_get(const unsigned char* p, size_t i) {
    if (WIDTH == 1) return (long long)(signed char)p[i];
    if (WIDTH == 3) {
        const unsigned char* q = p + 3 * i;
        return (long long)((int)q[0] | ((int)q[1] << 8) | ((int)(signed char)q[2] << 16));
    }
    int v;
    __builtin_memcpy(&v, p + 4 * i, 4);
    return (long long)v;
}

template <int WIDTH>
__device__ __forceinline__ void chain_put(unsigned char* p, size_t i, long long x) {
    if (WIDTH == 1) { p[i] = (unsigned char)(signed char)x; return; }
    if (WIDTH == 3) {
        unsigned char* q = p + 3 * i;
        const int v = (int)x;
        q[0] = (unsigned char)(v & 0xFF); q[1] = (unsigned char)((v >> 8) & 0xFF); q[2] = (unsigned char)((v >> 16) & 0xFF);
        return;
    }
    const int v = (int)x;
    __builtin_memcpy(p + 4 * i, &v, 4);
}
