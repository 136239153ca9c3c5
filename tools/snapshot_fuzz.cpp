// The snapshot reader under the CPU sanitizers: evm_snapshot_info over a good
// file and over seeded mutations of it.  Host code only (it links
// evolu_amd/csrc/evm_snapshot.cpp and nothing else; no HIP, no GPU):
//
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/snapshot_fuzz.cpp evolu_amd/csrc/evm_snapshot.cpp -o /tmp/snapshot_fuzz
//   /tmp/snapshot_fuzz tests/golden/sync_snapshot_v1.bin 4000
//
// Mutations: bytes flipped, the file cut or extended, header fields
// overwritten with the header re-summed (so the counts and lengths are what
// the reader sees, not the checksum), section bytes overwritten with the
// section re-summed (so the value checks run).  The good file must be
// accepted, every mutation must answer EVM_OK or EVM_ESNAPSHOT, and a mutation
// that changed a byte the file's checksums cover must not be accepted unless
// it was re-summed.  Exit status 0 and a one-line summary, or the sanitizer's
// report.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../evolu_amd/csrc/evm_snapshot.hpp"
#include "../include/evm.h"

namespace {

uint64_t rng_state = 1;
uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

uint64_t get64(const std::vector<uint8_t>& b, size_t at) {
  uint64_t v = 0;
  for (int k = 7; k >= 0; --k) v = (v << 8) | b[at + k];
  return v;
}
void put64(std::vector<uint8_t>& b, size_t at, uint64_t v) {
  for (int k = 0; k < 8; ++k) b[at + k] = (uint8_t)(v >> (8 * k));
}
void resum_header(std::vector<uint8_t>& b) {
  evm::Sum64 s;
  s.update(b.data(), evm::SNAP_HEADER_BYTES - 8);
  put64(b, evm::SNAP_HEADER_BYTES - 8, s.digest());
}

bool write_file(const std::string& path, const std::vector<uint8_t>& b) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = b.empty() || fwrite(b.data(), 1, b.size(), f) == b.size();
  return fclose(f) == 0 && ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s good-snapshot mutations [seed] [scratch-file]\n", argv[0]);
    return 2;
  }
  const long n_mut = atol(argv[2]);
  rng_state = argc > 3 ? strtoull(argv[3], nullptr, 10) : 1;
  const std::string tmp = argc > 4 ? argv[4] : std::string(argv[1]) + ".fuzz.tmp";
  std::vector<uint8_t> good;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint8_t buf[4096];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) good.insert(good.end(), buf, buf + k);
    fclose(f);
  }
  struct evm_snapshot_info si;
  if (evm_snapshot_info(argv[1], &si) != EVM_OK || good.size() < evm::SNAP_HEADER_BYTES) {
    fprintf(stderr, "the good file is not accepted\n");
    return 1;
  }
  if (evm_snapshot_info(nullptr, &si) != EVM_EINVAL || evm_snapshot_info(argv[1], nullptr) != EVM_EINVAL) return 1;
  // where the sections lie (from the good header)
  uint64_t at[evm::SNAP_SECTIONS + 1];
  at[0] = evm::SNAP_HEADER_BYTES;
  for (int k = 0; k < evm::SNAP_SECTIONS; ++k) at[k + 1] = at[k] + get64(good, 56 + 16 * k);
  long accepted = 0, rejected = 0, kinds[5] = {};
  for (long m = 0; m < n_mut; ++m) {
    std::vector<uint8_t> b = good;
    const int kind = (int)(rnd() % 5);
    bool must_reject = false;
    ++kinds[kind];
    switch (kind) {
      case 0: {  // flip 1-4 bytes anywhere
        const int flips = 1 + (int)(rnd() % 4);
        for (int j = 0; j < flips; ++j) b[rnd() % b.size()] ^= (uint8_t)(1u << (rnd() % 8));
        must_reject = b != good;
        break;
      }
      case 1:  // cut
        b.resize(rnd() % b.size());
        must_reject = true;
        break;
      case 2: {  // extend
        const int more = 1 + (int)(rnd() % 64);
        for (int j = 0; j < more; ++j) b.push_back((uint8_t)rnd());
        must_reject = true;
        break;
      }
      case 3: {  // a header field (version .. a section's length or sum) overwritten, header re-summed
        const size_t field = 8 + 8 * (rnd() % 24);
        uint64_t v = rnd();
        switch (rnd() % 4) {
          case 0: v &= 0xff; break;
          case 1: v = get64(b, field) + (rnd() % 5) - 2; break;
          case 2: v = ~0ull - (rnd() % 64); break;
          default: break;
        }
        put64(b, field, v);
        resum_header(b);
        must_reject = b != good;
        break;
      }
      default: {  // section bytes overwritten, the section and the header re-summed
        const int k = (int)(rnd() % evm::SNAP_SECTIONS);
        const uint64_t len = at[k + 1] - at[k];
        if (len) {
          const int writes = 1 + (int)(rnd() % 6);
          for (int j = 0; j < writes; ++j) {
            const uint64_t p = at[k] + rnd() % len;
            b[p] = (rnd() & 1) ? (uint8_t)rnd() : (uint8_t)(b[p] + 1);
          }
          evm::Sum64 s;
          s.update(b.data() + at[k], len);
          put64(b, 64 + 16 * k, s.digest());
          resum_header(b);
        }
        break;  // (may be accepted: contents, keys, roots and the blob are free bytes)
      }
    }
    if (!write_file(tmp, b)) return 2;
    const int st = evm_snapshot_info(tmp.c_str(), &si);
    if (st != EVM_OK && st != EVM_ESNAPSHOT) {
      fprintf(stderr, "mutation %ld (kind %d): status %d\n", m, kind, st);
      return 1;
    }
    if (st == EVM_OK && must_reject) {
      fprintf(stderr, "mutation %ld (kind %d): a damaged file was accepted\n", m, kind);
      return 1;
    }
    ++(st == EVM_OK ? accepted : rejected);
  }
  remove(tmp.c_str());
  printf("snapshot_fuzz: %ld mutations (flip %ld, cut %ld, extend %ld, header %ld, section %ld): %ld rejected, %ld accepted\n",
         n_mut, kinds[0], kinds[1], kinds[2], kinds[3], kinds[4], rejected, accepted);
  return 0;
}
