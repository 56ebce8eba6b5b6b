// vba_host_arena.h -- the arena of a small-problem entry point (plain C++17, no HIP): an ordered list of 256-byte-aligned regions
// in three consecutive sections [upload | back | work].  The device arena holds all three; the pinned staging block `in` mirrors
// the upload section (one H2D copy) and `out` mirrors the back section (one D2H copy, offsets relative to its start).
#pragma once
#include <cstddef>

namespace vba_host {

struct ArenaLayout {
    size_t cur = 0, up_end = 0, back_end = 0;
    // offset of a new region of `bytes` (the caller's slack included); the next one starts at the next multiple of 256
    size_t take(size_t bytes) { const size_t o = cur; cur += (bytes + 255) / 256 * 256; return o; }
    void end_upload() { up_end = cur; }   // the regions so far go up, the next ones come back ...
    void end_back() { back_end = cur; }   // ... and the rest never leaves the device
    size_t upload_bytes() const { return up_end; }
    size_t back_bytes() const { return back_end - up_end; }
    size_t total_bytes() const { return cur; }
    size_t in_back(size_t offset) const { return offset - up_end; }   // a back region's offset inside the `out` staging block
};

template <typename T>
T* at(void* base, size_t offset) { return reinterpret_cast<T*>(static_cast<char*>(base) + offset); }

}  // namespace vba_host
