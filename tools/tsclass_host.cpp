// The timestamp classifier (evolu_amd/csrc/evm_tsclass.hpp, the arithmetic of
// evm_ts_classify and of the sync round's EVM_SYNC_OPT_DATE_500) on the host:
// no GPU, so it can run under ASan / UBSan.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ievolu_amd/csrc tools/tsclass_host.cpp -o tsclass_host
//   tsclass_host rows.bin     rows.bin: n rows of 46 bytes back to back
//
// Prints per row its class (0 ok, 1 range_error, 2 unsupported) and, for class
// 0, the canonical string.  Each row is classified from a heap copy of exactly
// 46 bytes, and canon is a heap block of exactly 46: a read or write past
// either is an ASan report.  tests/test_tsclass_host.py builds it plain and
// compares the output with evolu_amd/lenient.py over the V8-generated
// vectors, edge dates and damaged rows.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "evm_tsclass.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s rows.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> all;
  uint8_t buf[4096];
  for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) all.insert(all.end(), buf, buf + k);
  fclose(f);
  if (all.size() % 46) {
    fprintf(stderr, "%s: not a whole number of 46-byte rows\n", argv[1]);
    return 2;
  }
  for (size_t i = 0; i < all.size() / 46; ++i) {
    std::unique_ptr<uint8_t[]> row(new uint8_t[46]), canon(new uint8_t[46]);
    memcpy(row.get(), &all[i * 46], 46);
    const uint8_t c = evm::ts_classify(row.get(), canon.get());
    if (c != evm::ts_classify(row.get(), nullptr)) return 1;  // (the class does not depend on canon)
    if (c == evm::TS_OK) printf("0 %.46s\n", reinterpret_cast<const char*>(canon.get()));
    else printf("%d\n", (int)c);
  }
  return 0;
}
