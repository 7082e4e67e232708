/*
 * The host flush writer (reporter_amd/csrc/flush_host.cpp) as a stand-alone
 * program: linked with flush_host.cpp and json.cpp alone -- no HIP, no engine --
 * so that tests/test_flush_host.py can build it with AddressSanitizer and
 * UndefinedBehaviorSanitizer linked in and run it as an ordinary program.
 *
 *   flush_host_main CASE OUT
 *
 * CASE (little endian): int64 n_segments, rows, nbins, rank, world; float
 * bin_kph and 4 bytes of padding; u64 ids[n_segments]; u32 counts[rows * nbins];
 * u64 speed_sum[rows].  OUT receives the body; stdout
 * "rc n_records body_len terminator".
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "otmatch.h"

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s CASE OUT\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t hdr[5];
  float kph[2];
  if (fread(hdr, 8, 5, f) != 5 || fread(kph, 4, 2, f) != 2) return 2;
  const int64_t nseg = hdr[0], rows = hdr[1], nbins = hdr[2];
  if (nseg < 0 || rows < 0 || nbins < 0 || nseg > (1 << 24) || rows > (1 << 24) || nbins > 4096) return 2;
  const size_t nc = (size_t)rows * (size_t)nbins;
  /* exact-size heap blocks: a read past either end is an ASan report */
  uint64_t* ids = (uint64_t*)malloc(nseg ? (size_t)nseg * 8 : 1);
  uint32_t* counts = (uint32_t*)malloc(nc ? nc * 4 : 1);
  uint64_t* sums = (uint64_t*)malloc(rows ? (size_t)rows * 8 : 1);
  if (!ids || !counts || !sums) return 2;
  if (fread(ids, 8, (size_t)nseg, f) != (size_t)nseg || fread(counts, 4, nc, f) != nc ||
      fread(sums, 8, (size_t)rows, f) != (size_t)rows)
    return 2;
  fclose(f);
  char* body = NULL;
  size_t len = 0;
  int64_t nrec = -1;
  const int rc = otm_flush_body_host(counts, sums, ids, nseg, rows, (int)nbins, kph[0], (int)hdr[3], (int)hdr[4],
                                     &body, &len, &nrec);
  if (rc == 0) {
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(body, 1, len, o) != len) return 2;
    fclose(o);
  }
  printf("%d %lld %zu %d\n", rc, (long long)nrec, len, rc == 0 ? (int)body[len] : -1);
  free(body); /* (otm_free of a plain allocation: the library is not linked here) */
  free(ids);
  free(counts);
  free(sums);
  return 0;
}
