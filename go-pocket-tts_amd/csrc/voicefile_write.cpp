// voicefile_write.cpp -- the two kinds of voice file the reader (voicefile.cpp; internal/safetensors/reader.go:69-155,219-308) accepts, written
// on the host.  safetensors layout: 8-byte little-endian header length, a JSON header mapping each tensor name (sorted) to its dtype, shape and
// [begin, end) byte range in the data section, then the data, tensor after tensor in header order.  The header is padded with spaces so that
// the data starts 8-byte aligned.
#include <cstdio>

#include "runtime.h"

namespace ptts {

namespace {

struct StOut {
    std::string dtype;
    std::vector<int64_t> shape;
    const void* data;
    size_t bytes;
};

std::vector<uint8_t> st_write(const std::map<std::string, StOut>& tensors) {   // (std::map: names in sorted order)
    std::string h = "{";
    size_t off = 0;
    for (const auto& kv : tensors) {
        if (h.size() > 1) h += ",";
        h += "\"" + kv.first + "\":{\"dtype\":\"" + kv.second.dtype + "\",\"shape\":[";
        for (size_t i = 0; i < kv.second.shape.size(); i++) h += (i ? "," : "") + std::to_string((long long)kv.second.shape[i]);
        h += "],\"data_offsets\":[" + std::to_string(off) + "," + std::to_string(off + kv.second.bytes) + "]}";
        off += kv.second.bytes;
    }
    h += "}";
    while ((8 + h.size()) % 8) h += ' ';
    std::vector<uint8_t> out(8 + h.size() + off);
    const uint64_t hl = h.size();
    for (int i = 0; i < 8; i++) out[(size_t)i] = (uint8_t)(hl >> (8 * i));
    std::memcpy(out.data() + 8, h.data(), h.size());
    uint8_t* p = out.data() + 8 + h.size();
    for (const auto& kv : tensors) {
        if (kv.second.bytes) std::memcpy(p, kv.second.data, kv.second.bytes);
        p += kv.second.bytes;
    }
    return out;
}

}  // namespace

std::vector<uint8_t> voice_state_file(const float* const* caches, int64_t offset, int n_layers, int heads, int head_dim) {
    if (n_layers < 1 || heads < 1 || head_dim < 1 || offset < 0)
        throw Error(PTTS_EINVAL, strfmt("ptts-hip: voice model state of %d layers, %d heads x %d, offset %lld", n_layers, heads, head_dim, (long long)offset));
    if (!caches) throw Error(PTTS_EINVAL, "native: voice model state is nil");
    const size_t cb = (size_t)2 * offset * heads * head_dim * sizeof(float);
    std::vector<int64_t> offs((size_t)n_layers, offset);
    std::map<std::string, StOut> t;
    for (int l = 0; l < n_layers; l++) {
        if (!caches[l] && cb) throw Error(PTTS_EINVAL, strfmt("native: voice model state module \"transformer.layers.%d.self_attn\" missing cache", l));
        const std::string mod = "transformer.layers." + std::to_string(l) + ".self_attn";
        t[mod + "/cache"] = StOut{"F32", {2, 1, offset, heads, head_dim}, caches[l], cb};
        t[mod + "/offset"] = StOut{"I64", {1}, &offs[(size_t)l], sizeof(int64_t)};
    }
    return st_write(t);
}

std::vector<uint8_t> voice_embedding_file(const float* emb, int64_t frames, int64_t dim) {
    if (frames < 1 || dim < 1) throw Error(PTTS_EINVAL, strfmt("ptts-hip: voice embedding shape [1 %lld %lld]", (long long)frames, (long long)dim));
    if (!emb) throw Error(PTTS_EINVAL, "ptts-hip: voice embedding is null");
    std::map<std::string, StOut> t;
    t["audio_prompt"] = StOut{"F32", {1, frames, dim}, emb, (size_t)frames * dim * sizeof(float)};
    return st_write(t);
}

void write_file(const std::string& path, const std::vector<uint8_t>& bytes) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) throw Error(PTTS_EIO, strfmt("ptts-hip: create %s: %s", path.c_str(), strerror(errno)));
    const bool ok = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    const bool closed = fclose(f) == 0;
    if (!ok || !closed) throw Error(PTTS_EIO, strfmt("ptts-hip: write %s failed", path.c_str()));
}

}  // namespace ptts
