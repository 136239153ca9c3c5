// The snapshot file's host side: header codec and the verifier that reads a
// file from disk and trusts nothing in it (evm_snapshot.hpp has the layout).
// Host C++ only -- no HIP, no device: evm_snapshot_info runs anywhere.
#include "evm_snapshot.hpp"

#include <stdio.h>

#include <vector>

#include "../../include/evm.h"

namespace evm {

namespace {

const uint8_t MAGIC[8] = {'E', 'V', 'M', 'S', 'N', 'A', 'P', 0};

void put32(uint8_t* p, uint32_t v) {
  for (int k = 0; k < 4; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
void put64(uint8_t* p, uint64_t v) {
  for (int k = 0; k < 8; ++k) p[k] = (uint8_t)(v >> (8 * k));
}
uint32_t get32(const uint8_t* p) {
  uint32_t v = 0;
  for (int k = 3; k >= 0; --k) v = (v << 8) | p[k];
  return v;
}
uint64_t get64(const uint8_t* p) {
  uint64_t v = 0;
  for (int k = 7; k >= 0; --k) v = (v << 8) | p[k];
  return v;
}

// a * b + c without wrapping, or false
bool mul_add(uint64_t a, uint64_t b, uint64_t c, uint64_t* out) {
  if (b && a > (UINT64_MAX - c) / b) return false;
  *out = a * b + c;
  return true;
}

// Per-section checks of the values the device would otherwise trust, fed
// the section's bytes in pieces (an element may straddle two pieces).
struct Checker {
  const SnapHeader& h;
  int sec;
  uint8_t part[8];
  size_t fill = 0;
  uint64_t acc = 0, prev = 0, count = 0;
  bool ok = true;

  Checker(const SnapHeader& hd, int s) : h(hd), sec(s) {}
  size_t width() const { return sec == SN_KLEN || sec == SN_OWNER ? 4 : sec == SN_COFF ? 8 : 1; }
  void element(const uint8_t* p) {
    switch (sec) {
      case SN_KLEN: {
        const uint64_t v = get32(p);
        if (v > h.key_bytes - acc) ok = false;
        else acc += v;
        break;
      }
      case SN_OWNER:
        if (get32(p) >= h.users) ok = false;
        break;
      case SN_COFF: {
        const uint64_t v = get64(p);
        if (count == 0 ? v != 0 : v < prev) ok = false;
        if (v > h.content_bytes) ok = false;
        prev = v;
        break;
      }
      default: break;
    }
    ++count;
  }
  void update(const uint8_t* p, size_t n) {
    if (sec == SN_FLAGS) {
      for (size_t i = 0; i < n; ++i)
        if (p[i] > 1) ok = false;
      return;
    }
    const size_t w = width();
    if (w == 1) return;
    while (n) {
      if (fill || n < w) {
        const size_t take = n < w - fill ? n : w - fill;
        memcpy(part + fill, p, take);
        fill += take;
        p += take;
        n -= take;
        if (fill == w) {
          element(part);
          fill = 0;
        }
        continue;
      }
      element(p);
      p += w;
      n -= w;
    }
  }
  bool finish() const {
    if (!ok || fill) return false;
    if (sec == SN_KLEN) return acc == h.key_bytes;
    if (sec == SN_COFF) return count == h.rows + 1 && prev == h.content_bytes;
    return true;
  }
};

int parse_header(const uint8_t* b, SnapHeader* h) {
  if (memcmp(b, MAGIC, 8) != 0) return EVM_ESNAPSHOT;
  Sum64 s;
  s.update(b, SNAP_HEADER_BYTES - 8);
  if (s.digest() != get64(b + SNAP_HEADER_BYTES - 8)) return EVM_ESNAPSHOT;
  if (get32(b + 8) != SNAP_VERSION || get32(b + 12) != (uint32_t)SNAP_SECTIONS) return EVM_ESNAPSHOT;
  h->users = get64(b + 16);
  h->rows = get64(b + 24);
  h->content_bytes = get64(b + 32);
  h->key_bytes = get64(b + 40);
  h->blob_bytes = get64(b + 48);
  // (slots are 32-bit; every length below must be computable)
  uint64_t t;
  if (h->users > 0xfffffffeull || !mul_add(h->rows, 48, 0, &t) || !mul_add(h->rows, 8, 8, &t)) return EVM_ESNAPSHOT;
  SnapHeader want = *h;
  snap_lengths(&want);
  uint64_t total = SNAP_HEADER_BYTES;
  for (int k = 0; k < SNAP_SECTIONS; ++k) {
    h->len[k] = get64(b + 56 + 16 * k);
    h->sum[k] = get64(b + 64 + 16 * k);
    if (h->len[k] != want.len[k]) return EVM_ESNAPSHOT;
    if (h->len[k] > UINT64_MAX - total) return EVM_ESNAPSHOT;
    total += h->len[k];
  }
  return EVM_OK;
}

}  // namespace

void snap_header_write(const SnapHeader& h, uint8_t* out) {
  memset(out, 0, SNAP_HEADER_BYTES);
  memcpy(out, MAGIC, 8);
  put32(out + 8, SNAP_VERSION);
  put32(out + 12, (uint32_t)SNAP_SECTIONS);
  put64(out + 16, h.users);
  put64(out + 24, h.rows);
  put64(out + 32, h.content_bytes);
  put64(out + 40, h.key_bytes);
  put64(out + 48, h.blob_bytes);
  for (int k = 0; k < SNAP_SECTIONS; ++k) {
    put64(out + 56 + 16 * k, h.len[k]);
    put64(out + 64 + 16 * k, h.sum[k]);
  }
  Sum64 s;
  s.update(out, SNAP_HEADER_BYTES - 8);
  put64(out + SNAP_HEADER_BYTES - 8, s.digest());
}

int snap_verify(const char* path, SnapHeader* out) {
  if (!path || !out) return EVM_EINVAL;
  FILE* f = fopen(path, "rb");
  if (!f) return EVM_ESNAPSHOT;
  int st = EVM_OK;
  uint8_t hb[SNAP_HEADER_BYTES];
  SnapHeader h;
  if (fread(hb, 1, SNAP_HEADER_BYTES, f) != SNAP_HEADER_BYTES) st = EVM_ESNAPSHOT;
  if (!st) st = parse_header(hb, &h);
  std::vector<uint8_t> buf((size_t)1 << 20);
  for (int k = 0; !st && k < SNAP_SECTIONS; ++k) {
    Sum64 s;
    Checker c(h, k);
    for (uint64_t left = h.len[k]; left && !st;) {
      const size_t want = (size_t)(left < buf.size() ? left : buf.size());
      if (fread(buf.data(), 1, want, f) != want) {
        st = EVM_ESNAPSHOT;  // (truncated)
        break;
      }
      s.update(buf.data(), want);
      c.update(buf.data(), want);
      left -= want;
    }
    if (!st && (s.digest() != h.sum[k] || !c.finish())) st = EVM_ESNAPSHOT;
  }
  if (!st && fgetc(f) != EOF) st = EVM_ESNAPSHOT;  // (bytes after the last section)
  fclose(f);
  if (!st) *out = h;
  return st;
}

}  // namespace evm

extern "C" int evm_snapshot_info(const char* path, struct evm_snapshot_info* out) {
  if (!path || !out) return EVM_EINVAL;
  evm::SnapHeader h;
  const int st = evm::snap_verify(path, &h);
  if (st) return st;
  out->version = evm::SNAP_VERSION;
  out->users = h.users;
  out->rows = h.rows;
  out->content_bytes = h.content_bytes;
  out->blob_bytes = h.blob_bytes;
  return EVM_OK;
}
