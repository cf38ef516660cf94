// oi_stage_layout.h -- one workspace carved into aligned parts.  No HIP here: a CPU program can include it.
#pragma once

#include <cstddef>
#include <cstdint>

// Parts are added front to back; add() returns the part's offset, every offset is a multiple of the granule (a power of two)
// and a part of 0 bytes -- an absent one -- takes no room: it shares the next part's offset.  total() is what the buffer needs.
struct StageLayout {
    size_t granule, end = 0;
    explicit StageLayout(size_t granule_) : granule(granule_) {}
    size_t add(size_t bytes) {
        const size_t off = end;
        end += (bytes + granule - 1) & ~(granule - 1);
        return off;
    }
    size_t total() const { return end; }
    template <class T> static T *at(void *base, size_t part) { return reinterpret_cast<T *>(static_cast<uint8_t *>(base) + part); }
};
