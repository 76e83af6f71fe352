// opts_check.h -- what the checks of a caller's option structs share (compressor.cpp, limiter.cpp, true_peak.cpp, eq.cpp): the refusal, the range
// message and the size rules of a struct that carries its own size (include/ptts.h ptts_dsp_ext_opts).  Header only, no HIP header.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "eq.h"

namespace ptts {

inline int fail(const std::string& e) {
    set_last_error("ptts-hip: " + e);
    return PTTS_EINVAL;
}

// true, and the message in out: v is not a finite value from lo to hi.  stage: what the message starts with ("compressor", "eq: section 2")
inline bool range_error(const char* stage, const char* field, double v, double lo, double hi, std::string& out) {
    if (std::isfinite(v) && v >= lo && v <= hi) return false;
    out = strfmt("%s: %s %g is not a finite value from %g to %g", stage, field, v, lo, hi);
    return true;
}

// The size rules: `size`, as the struct at p states it, covers at least the first `least` bytes (least_covers names them in the message), and
// whatever a caller newer than this library says beyond the `known` bytes is "off": zero.  Empty: fine
inline std::string opts_size_error(const char* stage, const void* p, uint32_t size, size_t least, size_t known, const char* least_covers) {
    if (size < least) return strfmt("%s: size %u is smaller than %s (%zu bytes)", stage, size, least_covers, least);
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = known; i < size; i++)
        if (b[i]) return strfmt("%s: size %u: byte %zu is not 0, and this library knows %zu bytes", stage, size, i, known);
    return std::string();
}

}  // namespace ptts
