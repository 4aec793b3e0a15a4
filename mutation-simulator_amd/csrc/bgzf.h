// BGZF compression on the device (bgzf.hip): shared by the output channels (file_io.hip) and msim_bgzf_compress.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace msim {

constexpr uint32_t BGZF_BLOCK = 65280;         // uncompressed bytes per member (what bgzip uses)
constexpr uint32_t BGZF_SLOT = 65536;          // a member's deflate data is written into a slot of this size first
constexpr uint64_t BGZF_PIECE_BLOCKS = 1024;   // members per launch: the workspace is sized for this many
extern const uint8_t BGZF_EOF[28];             // the end-of-file marker member

struct BgzfWork {                              // per-launch device workspace (one per output channel / one-shot call)
    uint32_t *d_ws = nullptr;                  // 4 B per input byte: match candidates, then tokens
    uint8_t *d_slots = nullptr;                // deflate data per block
    uint32_t *d_meta = nullptr;                // {deflate bytes, CRC32, ISIZE} per block
    uint64_t *d_off = nullptr;                 // member offsets + total
    uint8_t *d_out = nullptr;                  // the members back to back
    uint64_t *h_total = nullptr;               // pinned
};

hipError_t bgzf_compress_device(const uint8_t *d_src, uint64_t n, BgzfWork &w, hipStream_t st, uint64_t *out_bytes,
                                hipEvent_t ev_start = nullptr, hipEvent_t ev_end = nullptr);
void bgzf_work_free(BgzfWork &w);

}  // namespace msim
