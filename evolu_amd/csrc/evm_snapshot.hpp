// The sync server's snapshot file (evm_sync_save / evm_sync_load): layout,
// checksum and the host-only verifier (evm_snapshot.cpp; no HIP in either).
//
// Little-endian, no padding, no pointers, times or capacities:
//
//   header (SNAP_HEADER_BYTES)
//     0   magic "EVMSNAP\0"
//     8   u32 version (1)            12  u32 sections (SNAP_SECTIONS)
//     16  u64 users   24 u64 rows   32 u64 content bytes   40 u64 key bytes   48 u64 blob bytes
//     56  per section: u64 length, u64 checksum
//     200 u64 checksum of bytes [0, 200)
//   sections, back to back, in this order:
//     KLEN    users x u32      each user's key length, slot order
//     KEYS    key bytes        the userIds, slot order
//     FLAGS   users x u8       hand-over flags (0 / 1)
//     OWNER   rows x u32       each log row's owner slot, id order
//     TS      rows x 48        the log's timestamp rows
//     COFF    (rows + 1) x u64 content offsets (from 0, ascending, last = content bytes)
//     CONTENT content bytes
//     ROOTS   users x i32 root hash, then users x u8 present (evm_tree_roots)
//     BLOB    the caller's bytes
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace evm {

constexpr uint32_t SNAP_VERSION = 1;
constexpr int SNAP_SECTIONS = 9;
constexpr size_t SNAP_HEADER_BYTES = 208;
enum SnapSection { SN_KLEN = 0, SN_KEYS, SN_FLAGS, SN_OWNER, SN_TS, SN_COFF, SN_CONTENT, SN_ROOTS, SN_BLOB };

struct SnapHeader {
  uint64_t users = 0, rows = 0, content_bytes = 0, key_bytes = 0, blob_bytes = 0;
  uint64_t len[SNAP_SECTIONS] = {};
  uint64_t sum[SNAP_SECTIONS] = {};
  // where each section starts in the file
  uint64_t at(int k) const {
    uint64_t a = SNAP_HEADER_BYTES;
    for (int j = 0; j < k; ++j) a += len[j];
    return a;
  }
};

// each section's length as the counts give it
inline void snap_lengths(SnapHeader* h) {
  h->len[SN_KLEN] = h->users * 4;
  h->len[SN_KEYS] = h->key_bytes;
  h->len[SN_FLAGS] = h->users;
  h->len[SN_OWNER] = h->rows * 4;
  h->len[SN_TS] = h->rows * 48;
  h->len[SN_COFF] = (h->rows + 1) * 8;
  h->len[SN_CONTENT] = h->content_bytes;
  h->len[SN_ROOTS] = h->users * 5;
  h->len[SN_BLOB] = h->blob_bytes;
}

// 64-bit checksum of a byte stream, fed in pieces of any size (the result
// does not depend on how the stream is cut).  Four multiply-rotate lanes over
// the stream's little-endian 8-byte words (word i in lane i % 4), the tail
// zero-padded, the length mixed in last.
class Sum64 {
 public:
  void update(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    total_ += n;
    if (fill_) {
      const size_t take = n < 32 - fill_ ? n : 32 - fill_;
      memcpy(buf_ + fill_, b, take);
      fill_ += take;
      b += take;
      n -= take;
      if (fill_ < 32) return;
      block(buf_);
      fill_ = 0;
    }
    for (; n >= 32; n -= 32, b += 32) block(b);
    if (n) {
      memcpy(buf_, b, n);
      fill_ = n;
    }
  }
  uint64_t digest() const {
    uint64_t l[4] = {l_[0], l_[1], l_[2], l_[3]};
    if (fill_) {
      uint8_t t[32] = {};
      memcpy(t, buf_, fill_);
      mix(l, t);
    }
    uint64_t h = total_ * K2;
    for (int k = 0; k < 4; ++k) h = rotl(h ^ l[k], 27) * K1 + 0x52dce729u;
    h ^= h >> 32;
    h *= K2;
    return h ^ (h >> 29);
  }

 private:
  static constexpr uint64_t K1 = 0x9e3779b185ebca87ull, K2 = 0xc2b2ae3d27d4eb4full;
  static uint64_t rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
  static uint64_t word(const uint8_t* p) {
    uint64_t w = 0;
    for (int k = 7; k >= 0; --k) w = (w << 8) | p[k];  // (little-endian on every host)
    return w;
  }
  static void mix(uint64_t* l, const uint8_t* p) {
    for (int k = 0; k < 4; ++k) l[k] = rotl(l[k] + word(p + 8 * k) * K2, 31) * K1;
  }
  void block(const uint8_t* p) { mix(l_, p); }
  uint64_t l_[4] = {0x60ea27eeadc0b5d6ull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull};
  uint8_t buf_[32] = {};
  size_t fill_ = 0;
  uint64_t total_ = 0;
};

void snap_header_write(const SnapHeader& h, uint8_t* out);  // out: SNAP_HEADER_BYTES
// The whole file checked on the host: header, lengths, every checksum, and
// what the device would otherwise have to trust (key lengths sum to the key
// bytes, flags 0 / 1, owners < users, content offsets ascending from 0 to the
// content bytes).  EVM_OK or EVM_ESNAPSHOT (EVM_EINVAL: no path / no output).
int snap_verify(const char* path, SnapHeader* out);

}  // namespace evm
