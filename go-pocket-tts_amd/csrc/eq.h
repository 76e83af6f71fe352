// eq.h -- what eq.cpp (the host side of a request's equaliser, no HIP header) shares with the device side (dsp_device.cpp, capi_rows.cpp, generate.cpp).
#pragma once
#include <string>
#include <type_traits>

#include "../../include/ptts.h"
#include "scan_block.h"

struct ptts_eq { ptts::EqScan sc; };

namespace ptts {

std::string strfmt(const char* fmt, ...) __attribute__((format(printf, 1, 2)));   // (common.h's, restated: this header includes no HIP header)
void set_last_error(const std::string& m);

// empty: section `index` of a cascade is well formed
std::string eq_section_error(const ptts_eq_section& s, int index);
// the RBJ cookbook section, normalised by a0 (s: well formed)
DspBiquad eq_design(const ptts_eq_section& s);
// sections, the cascade's state matrix and its powers A^kDspRun, A^kDspTile (c: n = 1 .. kEqMaxSections sections)
EqScan eq_scan_coeffs(const DspBiquad* c, int n);
// the cascade over x[0, n) in place, in the blocked form of scan_block.h: what k_eq_summary, k_eq_carry and k_eq_apply compute for one row
void eq_apply_blocked(const EqScan& sc, float* x, int64_t n);
// the process-wide registry of live handles, one for every kind of per-request handle: an address is looked up under its mutex together with
// its kind (an equaliser is no ptts_dsp_ext) and never read
enum HandleKind : int { HANDLE_EQ = 1, HANDLE_DSP_EXT = 2 };
void handle_add(const void* h, HandleKind kind);
bool handle_take(const void* h, HandleKind kind);    // true: it was live, and is no more
bool handle_live(const void* h, HandleKind kind);
// f() under the registry's mutex if h is live (false: it is not, and f was not called): what reads or writes a handle whose owner may change it
bool handle_locked(const void* h, HandleKind kind, void (*f)(void* ctx), void* ctx);
template <class F>
inline bool handle_with(const void* h, HandleKind kind, F&& f) {   // (no type erasure: every delivered row's ext_lookup comes through here)
    return handle_locked(h, kind, [](void* ctx) { (*static_cast<std::remove_reference_t<F>*>(ctx))(); }, &f);
}
// the handle's system, or null when e is not one ptts_eq_create returned and ptts_eq_free has not
// yet taken (e itself is not read)
const EqScan* eq_lookup(const ptts_eq* e);

}  // namespace ptts
