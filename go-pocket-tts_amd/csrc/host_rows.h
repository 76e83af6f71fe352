// host_rows.h -- how the rows of a host-rows entry point (ptts_dsp_rows and its kin, ptts_resample, ptts_pcm_encode) share one device buffer: every row
// starts on a 256-byte boundary, and a skipped row takes no bytes.  No HIP header: the planning is plain arithmetic (runtime.h PackedRows holds the buffer).
#pragma once
#include <cstddef>

namespace ptts {

constexpr size_t kRowAlign = 256;

// off[i]: where row i of bytes[i] bytes starts; skip (optional): rows that stay on the host.  Returns the bytes of the whole buffer
inline size_t pack_rows(const size_t* bytes, const bool* skip, int rows, size_t* off) {
    size_t total = 0;
    for (int i = 0; i < rows; i++) {
        off[i] = total;
        if (!(skip && skip[i])) total += (bytes[i] + kRowAlign - 1) & ~(kRowAlign - 1);
    }
    return total;
}

}  // namespace ptts
