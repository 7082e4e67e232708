// pairs.h -- the pair window: the datastore reports aggregated
// per (time bucket, segment, next segment) in a hash table in HBM that the
// report kernels fill as they write the reports, and its flush body
//   {"mode":"auto","bucket_s":B,"origin":O,"privacy":P,"pairs":[
//    {"id":I,"next_id":N,"bucket":O+k*B,"count":C,"duration_ms":D,"length":L,
//     "queue_length":Q,"t_min":a,"t_max":b},...]}
// as reporter_amd/datastore.py defines it (serialize(pair_records(...))),
// written on the GPU (pairs.hip).
//
// The table: open addressing, linear probing, a power-of-two number of slots
// (>= 2 x max_keys).  A key is ONE 64-bit word,
//   k << 52 | row(id) << 26 | (row(next) + 1)       (0: no next; ~0: EMPTY)
// so a slot is claimed and its key published by one 64-bit compare-and-swap
// and no lane ever waits for another; the word's integer order is the body's
// order.  Whether a slot is EMPTY, holds the lane's key or another's is
// decided from an agent-scope atomic load or from what the compare-and-swap
// returned, never from a plain load (another XCD's L2 may hold a stale EMPTY).
// The max_keys cap is kept EXACTLY and without a lane ever waiting, by ranks:
// the lane whose compare-and-swap claimed a slot (one lane per distinct key)
// draws the key's rank from a counter that only grows; a key of rank >=
// max_keys is marked `over`.  Reports of an over key are added to its slot
// like any other and counted as dropped at the flush, which leaves the slot
// out: the body holds exactly min(distinct keys, max_keys) keys, whichever
// way the lanes raced.  So that over keys do not fill the table, a lane that
// finds the counter at max_keys BEFORE it confirms (by a compare-and-swap
// that changes nothing, so the answer is the memory's) that its probe ended
// on an EMPTY slot drops its report at once: every kept key was published
// before the counter reached max_keys, so the key is not among them.  Over
// keys are therefore claimed only by lanes that raced the counter's last
// steps; a probe that went round a table they filled drops too (a full table
// holds more than max_keys keys), so every probe ends.  (A reservation
// counter given back by the loser of a race for one key, the textbook cap,
// drops reports of other keys while two lanes hold reservations for the same
// key: the table then ends below max_keys with reports dropped.)
// The values are integer atomics on fields the clear kernel initialised (add,
// min, max), so no sum depends on order; `length` and `over` are plain stores
// (every writer stores the same value).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "otmatch.h"

struct otm_engine;

namespace otm {

constexpr int PAIR_BUCKETS = 4096;                   // time buckets of a window (12 bits of the key)
constexpr int PAIR_ROW_BITS = 26;                    // bits of a segment row (and of row(next) + 1)
constexpr int64_t PAIR_MAX_SEGMENTS = (1ll << PAIR_ROW_BITS) - 2;
constexpr unsigned long long PAIR_EMPTY = ~0ull;
constexpr int64_t PAIR_MAX_KEYS = 1ll << 30;         // the table's limit (2^31 slots)
// a record's literals (",{"id": ,"next_id": ,"bucket": ,"count": ,"duration_ms":
// ,"length": ,"queue_length": ,"t_min": ,"t_max": }) and its nine integers'
// digits (20 each but count 10 and length 11), in whole 8-byte words
constexpr int PAIR_SLOT_BYTES = (97 + 7 * 20 + 10 + 11 + 7 + 8) & ~7;

struct PairVal {  // one key's aggregates (48 bytes)
  unsigned long long duration_ms;  // sum of int((t1 - t0) * 1000 + 0.5), two's complement
  unsigned long long queue;        // sum of queue_length, two's complement
  long long t_min, t_max;          // min floor(t0), max floor(t1)
  uint32_t count;
  int32_t length;
  uint32_t over;  // its key's rank is >= max_keys: its reports count as dropped
  uint32_t pad;
};
// the table's counters: keys claimed (the ranks; only grows), reports added to
// a slot, out of range, dropped at the upsert, and (written by the flush's
// compaction and by the merge) the reports of over keys
enum { PAIR_C_KEYS = 0, PAIR_C_REPORTS, PAIR_C_RANGE, PAIR_C_DROPPED, PAIR_C_OVER, PAIR_C_WORDS };

// The table as the kernels see it (DevOut::pairs; key null: no pair window)
struct PairTab {
  unsigned long long* key;  // [1 << log2]
  PairVal* val;             // [1 << log2]
  unsigned long long* ctr;  // [PAIR_C_WORDS]
  int64_t max_keys;
  int64_t origin_k;         // origin / bucket_s
  int32_t bucket_s;
  int32_t log2;
};

// one host record of otm_pairs_add_reports, its ids mapped to rows
struct PairIn {
  double t0, t1;
  int32_t gi, gn;  // row(id) (-1: not admitted), row(next_id) (-1: no next)
  int32_t length, queue;
  uint32_t flags, pad;
};

struct PairMeta {  // device counters of one flush (zeroed before it)
  unsigned long long keys, records, suppressed_keys, suppressed_reports;
};

#ifdef __HIPCC__
__device__ __forceinline__ int64_t pair_hash(unsigned long long key, int log2) {
  return (int64_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - log2));
}

// The slot of `key`, claimed if new; -1 when the key is new and the table
// holds max_keys keys (the caller's report is dropped).
__device__ __forceinline__ int64_t pair_slot(const PairTab& T, unsigned long long key) {
  const int64_t mask = ((int64_t)1 << T.log2) - 1;
  int64_t h = pair_hash(key, T.log2);
  for (int64_t step = 0; step <= mask; ++step) {
    unsigned long long cur = __hip_atomic_load(&T.key[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == PAIR_EMPTY) {
      // the counter first, the slot after it (the order the drop relies on)
      const unsigned long long claimed =
          __hip_atomic_load(&T.ctr[PAIR_C_KEYS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool full = (int64_t)claimed >= T.max_keys;
      cur = atomicCAS(&T.key[h], PAIR_EMPTY, full ? PAIR_EMPTY : key);
      if (cur == PAIR_EMPTY) {
        if (full) return -1;
        // claimed and published at once; this lane alone draws the key's rank
        if ((int64_t)atomicAdd(&T.ctr[PAIR_C_KEYS], 1ull) >= T.max_keys) T.val[h].over = 1u;
        return h;
      }
    }
    if (cur == key) return h;
    h = (h + 1) & mask;  // another key's slot
  }
  return -1;  // once round a full table: it holds more than max_keys keys, and not this one
}

// `n` reports' aggregates into the slot's values
__device__ __forceinline__ void pair_add(PairVal& v, uint32_t n, unsigned long long dur, unsigned long long queue,
                                         long long t_min, long long t_max, int32_t length) {
  atomicAdd(&v.count, n);
  atomicAdd(&v.duration_ms, dur);
  atomicAdd(&v.queue, queue);
  atomicMin(&v.t_min, t_min);
  atomicMax(&v.t_max, t_max);
  v.length = length;
}

// One report into the table: report_hist's admission (a t1 that is the int -1
// of a partial next segment gives no speed; a speed >= 0 in float64; a segment
// with a row), then the bucket of t0.
__device__ __forceinline__ void pair_report(const PairTab& T, int32_t gi, int32_t gn, double t0, double t1,
                                            int32_t length, int32_t queue, uint32_t flags) {
  const double speed = ((double)length / (t1 - t0)) * 3.6;
  const bool t1_minus1 = (flags & OTM_REP_T1_INT) && t1 == -1.0;
  if (t1_minus1 || !(speed >= 0.0) || gi < 0) return;
  const double kf = floor(t0 / (double)T.bucket_s) - (double)T.origin_k;
  if (!(kf >= 0.0 && kf < (double)PAIR_BUCKETS)) {
    atomicAdd(&T.ctr[PAIR_C_RANGE], 1ull);
    return;
  }
  const unsigned long long key = (unsigned long long)(long long)kf << (2 * PAIR_ROW_BITS) |
                                 (unsigned long long)(uint32_t)gi << PAIR_ROW_BITS |
                                 (unsigned long long)(uint32_t)(gn + 1);
  const int64_t h = pair_slot(T, key);
  if (h < 0) {
    atomicAdd(&T.ctr[PAIR_C_DROPPED], 1ull);
    return;
  }
  atomicAdd(&T.ctr[PAIR_C_REPORTS], 1ull);
  pair_add(T.val[h], 1u, (unsigned long long)(long long)((t1 - t0) * 1000.0 + 0.5),
           (unsigned long long)(long long)queue, (long long)floor(t0), (long long)floor(t1), length);
}
#endif

// ---- launches (pairs.hip)
// every slot EMPTY with initial values, the counters zero
void launch_pairs_clear(const PairTab& t, hipStream_t s);
// k_pairs_add: one lane per host record
void launch_pairs_add(const PairTab& t, const PairIn* in, int64_t n, hipStream_t s);
// k_pairs_merge: every occupied slot of src upserted into dst (dst sized so that nothing drops)
void launch_pairs_merge(const PairTab& dst, const unsigned long long* src_key, const PairVal* src_val,
                        int64_t src_slots, hipStream_t s);
// the occupied slots' keys and slot numbers, in any order, into ckey / cidx
// (ckey pre-filled with EMPTY over cap entries; *n zeroed: the count)
void launch_pairs_compact(const PairTab& t, unsigned long long* ckey, uint32_t* cidx, unsigned long long* n,
                          hipStream_t s);
// (key, slot) pairs sorted by key; tmp_bytes from pairs_sort_tmp_bytes(n)
size_t pairs_sort_tmp_bytes(int64_t n);
void pairs_sort(const unsigned long long* kin, unsigned long long* kout, const uint32_t* vin, uint32_t* vout,
                int64_t n, void* tmp, size_t tmp_bytes, hipStream_t s);
// k_pairs_rows: sorted entry i (EMPTY: none) with count >= privacy formatted
// into slots[i] (PAIR_SLOT_BYTES, a leading comma included), len[i] its length
// (0: no record; len[n] = 0), the counts into meta
void launch_pairs_rows(const PairTab& t, const unsigned long long* skey, const uint32_t* sidx, int64_t n,
                       const uint64_t* ids, int32_t privacy, int64_t origin, char* slots, int64_t* len,
                       PairMeta* meta, hipStream_t s);

// ---- engine.cpp: the pair window of E (a parent engine or a multi-device engine)
int pairs_cfg_check(const otm_pairs_cfg* cfg, std::string* err);
int engine_pairs_begin(otm_engine* E, const otm_pairs_cfg* cfg, std::string* err);
int engine_pairs_add(otm_engine* E, int64_t n, const otm_report_rec* recs, std::string* err);
int engine_pairs_flush(otm_engine* E, char** body, size_t* body_len, otm_pairs_stats* stats, std::string* err);
int engine_pairs_end(otm_engine* E, std::string* err);

}  // namespace otm
