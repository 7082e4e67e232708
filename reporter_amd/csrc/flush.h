// flush.h -- the datastore flush body: the per-segment speed
// histogram of a window (counts u32[rows x nbins], speed sums u64[rows]) as the
// JSON body reporter_amd/datastore.py defines,
//   {"mode":"auto","bin_kph":B,"rank":R,"world":W,"segments":[
//    {"id":I,"count":C,"speed_sum_kph":F,"bins":[b0,...]},...]}
// written on the host (flush_host.cpp) or on the GPU (flush.hip).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

// (flush_host.cpp sees the host part alone: no HIP header, no engine)
#ifndef OTM_FLUSH_HOST_ONLY
#include <hip/hip_runtime.h>
#endif

struct otm_engine;

namespace otm {

// the device writer's limit on nbins (one lane per bin of a row: a wave)
constexpr int FLUSH_MAX_NBINS = 64;
// a record's literals: ,{"id": ,"count": ,"speed_sum_kph": ,"bins":[ ]}
constexpr int FLUSH_LIT_BYTES = 7 + 9 + 17 + 9 + 2;
// a record's slot: the literals, 20 bytes for the id, 20 for the count, 24
// for the float and 11 per bin (ten digits and a comma), in whole 8-byte words
constexpr int flush_slot_bytes(int nbins) { return (FLUSH_LIT_BYTES + 20 + 20 + 24 + 11 * nbins + 7) & ~7; }

// the body up to the records' '[' (flush_host.cpp)
std::string flush_head(float bin_kph, int rank, int world);
// the whole body on the host; 0 or OTM_EINVAL / OTM_ENOMEM with *err set
int flush_body_host(const uint32_t* counts, const uint64_t* speed_sum, const uint64_t* segment_ids,
                    int64_t n_segments, int64_t rows, int nbins, float bin_kph, int rank, int world, char** body,
                    size_t* body_len, int64_t* n_records, std::string* err);

#ifndef OTM_FLUSH_HOST_ONLY
struct FlushIn {
  const uint32_t* counts;            // [rows x nbins]
  const unsigned long long* sums;    // [rows]
  const uint64_t* ids;               // [n_segments] of the graph
  int64_t rows, row0, n_segments;    // slice rows; the slice's first global row
  int nbins;
};
struct FlushMeta {  // device counters of one call (zeroed before it)
  unsigned long long n_records;
  int32_t declined;  // a row whose float the device writer does not format
  int32_t pad;
};
// k_flush_rows: one streaming read of the slice; each row with a report is
// formatted into slot[row] (flush_slot_bytes) with a leading comma, len[row]
// its length (0: no record)
void launch_flush_rows(const FlushIn& in, char* slots, int64_t* len, FlushMeta* meta, hipStream_t s);
// k_flush_copy: the records back to back into dst (off: the scanned lengths,
// off[rows] the total); nothing when the total exceeds cap
void launch_flush_copy(int64_t rows, int slot_bytes, const char* slots, const int64_t* off, char* dst, int64_t cap,
                       hipStream_t s);
// k_flush_out: blob[0, *total) into page-locked host memory, 16 bytes a lane
// (both buffers hold cap + 16 bytes); nothing when the total exceeds cap
void launch_flush_out(const char* blob, const int64_t* total, char* dst, int64_t cap, hipStream_t s);
// dst += src over n32 counts and n64 sums (the member reduce of a window)
void launch_flush_add(uint32_t* dc, const uint32_t* sc, int64_t n32, unsigned long long* ds,
                      const unsigned long long* ss, int64_t n64, hipStream_t s);

// engine.cpp: the device writer over a slice in E's HBM (E a one-device
// engine or a clone); the caller holds E->mu.  stream null: E's own.
int engine_flush_body(otm_engine* E, const void* dev_counts, const void* dev_speed_sum, int64_t rows, int nbins,
                      float bin_kph, int rank, int world, hipStream_t stream, char** body, size_t* body_len,
                      int64_t* n_records, std::string* err);
// engine-owned windows (engine.cpp; E a parent engine or a multi-device engine)
int engine_window_begin(otm_engine* E, int nbins, float bin_kph, std::string* err);
int engine_window_flush(otm_engine* E, char** body, size_t* body_len, int64_t* n_records, std::string* err);
int engine_window_end(otm_engine* E, std::string* err);
#endif

}  // namespace otm
