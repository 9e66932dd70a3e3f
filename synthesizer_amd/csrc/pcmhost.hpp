// pcmhost.hpp -- host helpers that the PCM entry points of pcm.hip and pcm_ops.hip share, each stated once: the sample-width test,
// refusal and dispatch; the result of a launch; the overflow flag's readback; the split of a call into a 16-byte vector prefix and
// a scalar rest; the range check of one input and one output.  (Device helpers: pcmdev.hpp.)
#pragma once
#include "common.hpp"

inline bool valid_width(int width) { return width == 1 || width == 2 || width == 4; }      // (width 3 is diverted to the 32-bit kernels before this test)
inline bool valid_width3(int width) { return valid_width(width) || width == 3; }           // the entry points that take 24-bit samples as they are
inline int bad_width(const char* who, int width) { return sh::set_error(SH_ERR_INVALID, "%s: sample width %d not in {1,2,4}", who, width); }

// f(T()) with T the sample type of `width`
template <typename F>
int dispatch_width(int width, F&& f) {
    if (width == 1) return f((signed char)0);
    if (width == 2) return f((short)0);
    if (width == 4) return f((int)0);
    return bad_width("PCM", width);
}

// what the launches since the last look came to (for lambdas and value returns; SH_CHECK_LAUNCH returns from the enclosing function)
inline int launch_result(const char* kernel) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? (int)SH_OK : sh::hip_error(e, kernel);
}

// The overflow flag that k_quantize, k_modulate and k_pan_lfo raise: read back (one wait), and lowered again when it was up.
inline int take_overflow(int width) {
    sh::State& s = sh::state();
    SH_HIP(hipMemcpyAsync(s.flag_host, s.flag, sizeof(int), hipMemcpyDeviceToHost, s.stream));
    SH_HIP(hipStreamSynchronize(s.stream));
    if (!s.flag_host[0]) return SH_OK;
    SH_HIP(hipMemsetAsync(s.flag, 0, sizeof(int), s.stream));
    return sh::set_error(SH_ERR_OVERFLOW, "signed integer out of range for sample width %d", width);
}

// n units, `per` of them to a vector: nvec vectors cover the first `done` units where the caller found its pointers aligned (else
// none), `rest` units are left to the scalar kernel.
struct VecSplit { size_t nvec, done, rest; };
inline VecSplit vec_split(bool aligned, size_t n, size_t per) {
    const size_t nvec = aligned ? n / per : 0;
    return {nvec, nvec * per, n - nvec * per};
}

inline int check_io(const sh_buf* in, size_t in_off, size_t in_bytes, const sh_buf* out, size_t out_off, size_t out_bytes, const char* who) {
    if (!in || !out) return sh::set_error(SH_ERR_INVALID, "%s: NULL buffer", who);
    if (in_off > in->bytes || in_bytes > in->bytes - in_off) return sh::set_error(SH_ERR_INVALID, "%s: input range outside buffer", who);
    if (out_off > out->bytes || out_bytes > out->bytes - out_off) return sh::set_error(SH_ERR_INVALID, "%s: output range outside buffer", who);
    return SH_OK;
}
