// BGZF on the device (bgzf.hip).  Compression: shared by the output channels (file_io.hip) and msim_bgzf_compress.
// Inflation: the member chain of an input file (host pass) and k_bgzf_inflate, behind msim_bgzf_probe / msim_bgzf_inflate.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <vector>

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

// ---- inflate
constexpr uint32_t BGZF_MAX_ISIZE = 65536;     // the format's limit on a member's uncompressed bytes (BGZF_BLOCK is bgzip's habit)

struct BgzfMember {                            // one non-empty member of a piece, as k_bgzf_inflate reads it
    uint32_t in_off, in_len;                   // its deflate data: offset from the piece's first byte, bytes
    uint32_t out_off, isize;                   // its place in the piece's uncompressed bytes (exclusive scan of ISIZE), ISIZE
    uint32_t crc;                              // the trailer's CRC32
};

// reason codes of the inflate kernel's error word ((member index in the launch) << 4 | reason; 0xffffffff: none)
enum BgzfInflateError : uint32_t {
    BGZF_E_BTYPE = 1, BGZF_E_LENS = 2, BGZF_E_CODE = 3, BGZF_E_DIST = 4, BGZF_E_PAST = 5, BGZF_E_TRUNC = 6, BGZF_E_STORED = 7,
    BGZF_E_CRC = 8, BGZF_E_ISIZE = 9, BGZF_E_STEPS = 10
};
const char *bgzf_inflate_reason(uint32_t code);

struct BgzfMemberHost {                        // the same member as the host pass finds it in the file
    uint64_t start, payload;                   // file offsets of the member and of its deflate data
    uint32_t payload_len, isize, crc;
};

// Host pass over the member chain of in[0, n): BSIZE from the 'BC' subfield, ISIZE and CRC32 from the trailer.  Empty members
// (ISIZE 0: the EOF marker, wherever it stands) are counted in *n_members and otherwise skipped; `members` (optional) gets
// the others in file order.  false + *why: not gzip, gzip without BGZF framing, a BSIZE past the end, a truncated member,
// ISIZE > 65 536.
bool bgzf_walk(const uint8_t *in, uint64_t n, uint64_t *uncompressed, uint64_t *n_members, std::vector<BgzfMemberHost> *members,
               std::string *why);

// n members of one piece: d_in the piece's bytes (in_len of them), d_out its uncompressed bytes, *d_err the error word
// (set to 0xffffffff on `st` first).  Asynchronous.
hipError_t bgzf_inflate_device(const uint8_t *d_in, uint32_t in_len, const BgzfMember *d_meta, uint32_t n, uint8_t *d_out,
                               uint32_t *d_err, hipStream_t st);

}  // namespace msim
