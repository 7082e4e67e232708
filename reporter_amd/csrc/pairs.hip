// pairs.hip -- the pair window's kernels (pairs.h).
//
// The upsert itself (pair_slot / pair_add / pair_report, pairs.h) runs inside
// the report kernels (kernels.hip); here are the launches around it:
//   k_pairs_clear    every slot EMPTY, the values at their identities (begin,
//                    and after each flush)
//   k_pairs_add      one lane per host record (otm_pairs_add_reports)
//   k_pairs_merge    every occupied slot of one table upserted into another:
//                    the member reduce of a multi-device engine's window
// and the flush (engine.cpp engine_pairs_flush):
//   k_pairs_compact  the kept keys' (key, slot) pairs, in any order; the reports
//                    of the keys past max_keys (pairs.h) counted as dropped
//   (radix sort)     by key: the key's integer order is the body's order
//   k_pairs_rows     one lane per sorted entry: its values read, the privacy
//                    floor applied, the record formatted into a fixed slot
//   (scan_i64, k_flush_copy, k_flush_out: flush.hip)  packed and copied out
// Everything is an integer: no float writer, no host fallback.
#include <hipcub/hipcub.hpp>

#include "pairs.h"
#include "out8.h"
#include "pyrepr.h"

namespace otm {
namespace {

constexpr int PAIRS_TB = 256;

unsigned grid_for(int64_t items, int64_t per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > 16384) g = 16384;
  return (unsigned)g;
}

__global__ __launch_bounds__(PAIRS_TB) void k_pairs_clear(PairTab t) {
  const int64_t slots = (int64_t)1 << t.log2;
  const int64_t tid = (int64_t)blockIdx.x * PAIRS_TB + threadIdx.x, nt = (int64_t)gridDim.x * PAIRS_TB;
  if (tid < PAIR_C_WORDS) t.ctr[tid] = 0ull;
  for (int64_t i = tid; i < slots; i += nt) {
    t.key[i] = PAIR_EMPTY;
    t.val[i] = PairVal{0ull, 0ull, INT64_MAX, INT64_MIN, 0u, 0, 0u, 0u};
  }
}

__global__ __launch_bounds__(PAIRS_TB) void k_pairs_add(PairTab t, const PairIn* in, int64_t n) {
  const int64_t nt = (int64_t)gridDim.x * PAIRS_TB;
  for (int64_t i = (int64_t)blockIdx.x * PAIRS_TB + threadIdx.x; i < n; i += nt) {
    const PairIn r = in[i];
    pair_report(t, r.gi, r.gn, r.t0, r.t1, r.length, r.queue, r.flags);
  }
}

__global__ __launch_bounds__(PAIRS_TB) void k_pairs_merge(PairTab dst, const unsigned long long* src_key,
                                                          const PairVal* src_val, int64_t src_slots) {
  const int64_t nt = (int64_t)gridDim.x * PAIRS_TB;
  for (int64_t i = (int64_t)blockIdx.x * PAIRS_TB + threadIdx.x; i < src_slots; i += nt) {
    const unsigned long long key = src_key[i];
    if (key == PAIR_EMPTY) continue;
    const PairVal v = src_val[i];
    if (v.over) {  // a key past its member's max_keys: its reports were dropped
      atomicAdd(&dst.ctr[PAIR_C_OVER], (unsigned long long)v.count);
      continue;
    }
    const int64_t h = pair_slot(dst, key);
    if (h < 0) {  // (the host sized dst for every member's keys: not reached)
      atomicAdd(&dst.ctr[PAIR_C_DROPPED], (unsigned long long)v.count);
      continue;
    }
    pair_add(dst.val[h], v.count, v.duration_ms, v.queue, v.t_min, v.t_max, v.length);
  }
}

// the places come from one atomic per wave (the order is the sort's to make)
__global__ __launch_bounds__(PAIRS_TB) void k_pairs_compact(PairTab t, unsigned long long* ckey, uint32_t* cidx,
                                                            unsigned long long* n) {
  const int64_t slots = (int64_t)1 << t.log2;
  const int64_t nt = (int64_t)gridDim.x * PAIRS_TB;
  const int lane = threadIdx.x & 63;
  // (slots is a multiple of 64 and so is nt: a wave's lanes leave the loop together)
  for (int64_t i = (int64_t)blockIdx.x * PAIRS_TB + threadIdx.x; i < slots; i += nt) {
    const unsigned long long key = t.key[i];
    bool live = key != PAIR_EMPTY;
    if (live && t.val[i].over) {  // a key past max_keys: no record, its reports dropped
      atomicAdd(&t.ctr[PAIR_C_OVER], (unsigned long long)t.val[i].count);
      live = false;
    }
    const unsigned long long m = __ballot(live);
    if (!m) continue;
    unsigned long long base = 0;
    if (lane == __ffsll((long long)m) - 1) base = atomicAdd(n, (unsigned long long)__popcll(m));
    base = __shfl(base, __ffsll((long long)m) - 1, 64);
    if (live) {
      const unsigned long long at = base + __popcll(m & ((1ull << lane) - 1));
      if ((int64_t)at < t.max_keys) {  // (kept keys never exceed max_keys)
        ckey[at] = key;
        cidx[at] = (uint32_t)i;
      }
    }
  }
}

__global__ __launch_bounds__(PAIRS_TB) void k_pairs_rows(PairTab t, const unsigned long long* skey,
                                                         const uint32_t* sidx, int64_t n, const uint64_t* ids,
                                                         int32_t privacy, int64_t origin, char* slots, int64_t* len,
                                                         PairMeta* meta) {
  const int64_t nt = (int64_t)gridDim.x * PAIRS_TB;
  if (blockIdx.x == 0 && threadIdx.x == 0) len[n] = 0;
  constexpr unsigned long long RM = (1ull << PAIR_ROW_BITS) - 1;
  // (the loop runs to n rounded up to whole waves: every lane of a wave runs
  // the same iterations, so the ballots and the reduce are whole)
  const int64_t n64 = (n + 63) & ~(int64_t)63;
  for (int64_t i = (int64_t)blockIdx.x * PAIRS_TB + threadIdx.x; i < n64; i += nt) {
    const unsigned long long key = i < n ? skey[i] : PAIR_EMPTY;
    const bool live = key != PAIR_EMPTY;
    PairVal v{};
    if (live) v = t.val[sidx[i]];
    const bool emit = live && (int64_t)v.count >= (int64_t)privacy;
    const bool supp = live && !emit;
    if (emit) {
      Out o{slots + i * PAIR_SLOT_BYTES, 0, 0};
      const unsigned long long k = key >> (2 * PAIR_ROW_BITS), gi = (key >> PAIR_ROW_BITS) & RM, gn1 = key & RM;
      o.lit(",{\"id\":");
      pyrepr::put_u64(ids[gi], o);
      if (gn1) {
        o.lit(",\"next_id\":");
        pyrepr::put_u64(ids[gn1 - 1], o);
      }
      o.lit(",\"bucket\":");
      o.i64(origin + (int64_t)k * t.bucket_s);
      o.lit(",\"count\":");
      pyrepr::put_u64(v.count, o);
      o.lit(",\"duration_ms\":");
      o.i64((int64_t)v.duration_ms);
      o.lit(",\"length\":");
      o.i64(v.length);
      o.lit(",\"queue_length\":");
      o.i64((int64_t)v.queue);
      o.lit(",\"t_min\":");
      o.i64(v.t_min);
      o.lit(",\"t_max\":");
      o.i64(v.t_max);
      o.put('}');
      len[i] = o.done();
    } else if (i < n) {
      len[i] = 0;
    }
    // the call's counts: one atomic per wave and counter
    const unsigned long long ml = __ballot(live), me = __ballot(emit), ms = __ballot(supp);
    unsigned long long sr = supp ? v.count : 0ull;
    for (int d = 32; d; d >>= 1) sr += __shfl_xor(sr, d, 64);
    if ((threadIdx.x & 63) == 0 && ml) {
      atomicAdd(&meta->keys, (unsigned long long)__popcll(ml));
      if (me) atomicAdd(&meta->records, (unsigned long long)__popcll(me));
      if (ms) {
        atomicAdd(&meta->suppressed_keys, (unsigned long long)__popcll(ms));
        atomicAdd(&meta->suppressed_reports, sr);
      }
    }
  }
}

}  // namespace

void launch_pairs_clear(const PairTab& t, hipStream_t s) {
  hipLaunchKernelGGL(k_pairs_clear, dim3(grid_for((int64_t)1 << t.log2, PAIRS_TB * 4)), dim3(PAIRS_TB), 0, s, t);
}

void launch_pairs_add(const PairTab& t, const PairIn* in, int64_t n, hipStream_t s) {
  if (n < 1) return;
  hipLaunchKernelGGL(k_pairs_add, dim3(grid_for(n, PAIRS_TB)), dim3(PAIRS_TB), 0, s, t, in, n);
}

void launch_pairs_merge(const PairTab& dst, const unsigned long long* src_key, const PairVal* src_val,
                        int64_t src_slots, hipStream_t s) {
  hipLaunchKernelGGL(k_pairs_merge, dim3(grid_for(src_slots, PAIRS_TB * 4)), dim3(PAIRS_TB), 0, s, dst, src_key,
                     src_val, src_slots);
}

void launch_pairs_compact(const PairTab& t, unsigned long long* ckey, uint32_t* cidx, unsigned long long* n,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_pairs_compact, dim3(grid_for((int64_t)1 << t.log2, PAIRS_TB * 4)), dim3(PAIRS_TB), 0, s, t,
                     ckey, cidx, n);
}

size_t pairs_sort_tmp_bytes(int64_t n) {
  size_t b = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const unsigned long long*)nullptr,
                                           (unsigned long long*)nullptr, (const uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (int)n, 0, 64);
  return b;
}

void pairs_sort(const unsigned long long* kin, unsigned long long* kout, const uint32_t* vin, uint32_t* vout,
                int64_t n, void* tmp, size_t tmp_bytes, hipStream_t s) {
  (void)hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, kin, kout, vin, vout, (int)n, 0, 64, s);
}

void launch_pairs_rows(const PairTab& t, const unsigned long long* skey, const uint32_t* sidx, int64_t n,
                       const uint64_t* ids, int32_t privacy, int64_t origin, char* slots, int64_t* len,
                       PairMeta* meta, hipStream_t s) {
  hipLaunchKernelGGL(k_pairs_rows, dim3(grid_for(n, PAIRS_TB)), dim3(PAIRS_TB), 0, s, t, skey, sidx, n, ids, privacy,
                     origin, slots, len, meta);
}

}  // namespace otm
