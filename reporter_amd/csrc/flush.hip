// flush.hip -- the datastore flush body written on the GPU.
//
// flush_host.cpp's bytes (reporter_amd/datastore.py: serialize(flush_records))
// from a slice of the speed histogram in HBM.  Launches (engine.cpp
// engine_flush_body):
//   k_flush_rows  one streaming read of the slice: L lanes take a row (L the
//                 power of two >= nbins, a lane per bin, 64 / L rows to a
//                 wave), the row's total from a cross-lane reduce.  A row
//                 with total 0 costs its read and one length word; a row with
//                 a report is formatted by its first lane into a fixed-size
//                 slot (flush_slot_bytes), a leading comma included, with its
//                 length (its 64 B of bins read again by that lane: a cache
//                 hit).  A float outside pyrepr.h's range flags the call: the
//                 host writes that slice (flush_host.cpp).
//   (scan_i64)    the lengths into the records' places
//   k_flush_copy  the slots back to back into one dense blob
//   k_flush_out   the blob into page-locked host memory, 16 bytes a lane: the
//                 only bytes that cross the link are the body's
//   k_flush_add   dst += src over counts and sums: the member reduce of a
//                 multi-device engine's window
#include "flush.h"
#include "out8.h"
#include "pyrepr.h"

namespace otm {
namespace {

constexpr int FLUSH_TB = 256;

__global__ __launch_bounds__(FLUSH_TB) void k_flush_rows(FlushIn in, int lg, int slot_bytes, char* slots,
                                                         int64_t* len, FlushMeta* meta) {
  const int L = 1 << lg, rpb = FLUSH_TB >> lg;
  const int sub = threadIdx.x >> lg, j = threadIdx.x & (L - 1);
  const int64_t ngroups = (in.rows + rpb - 1) / rpb;
  if (blockIdx.x == 0 && threadIdx.x == 0) len[in.rows] = 0;
  for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {  // (uniform over the block)
    const int64_t row = g * rpb + sub;
    const bool live = row < in.rows;
    const uint32_t v = live && j < in.nbins ? in.counts[row * in.nbins + j] : 0u;
    unsigned long long tot = v;
    for (int o = L >> 1; o; o >>= 1) tot += __shfl_xor(tot, o, 64);
    const int64_t grow = in.row0 + row;
    // a row at or past n_segments is padding: it carries no id
    const bool emit = live && j == 0 && tot > 0 && grow < in.n_segments;
    const unsigned long long em = __ballot(emit);
    if (emit) {
      Out o{slots + row * slot_bytes, 0, 0};
      o.lit(",{\"id\":");
      pyrepr::put_u64(in.ids[grow], o);
      o.lit(",\"count\":");
      pyrepr::put_u64(tot, o);
      o.lit(",\"speed_sum_kph\":");
      // Python's int / float: the integer rounded to a double, one IEEE division
      const bool ok = o.f64((double)in.sums[row] / 1000.0);
      if (ok) {
        o.lit(",\"bins\":[");
        const uint32_t* c = in.counts + row * in.nbins;
        for (int b = 0; b < in.nbins; ++b) {
          if (b) o.put(',');
          pyrepr::put_u64(c[b], o);
        }
        o.lit("]}");
        len[row] = o.done();
      } else {
        len[row] = 0;
        meta->declined = 1;
      }
    } else if (live && j == 0) {
      len[row] = 0;
    }
    if ((threadIdx.x & 63) == 0 && em) atomicAdd(&meta->n_records, (unsigned long long)__popcll(em));
  }
}

// a wave per 64 rows: each lane its row's place and length, then the whole
// wave copies each record in turn
__global__ __launch_bounds__(FLUSH_TB) void k_flush_copy(int64_t rows, int slot_bytes, const char* slots,
                                                         const int64_t* off, char* dst, int64_t cap) {
  if (off[rows] > cap) return;  // (the host grows the blob and launches again)
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * FLUSH_TB + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * FLUSH_TB) >> 6;
  for (int64_t base = wave * 64; base < rows; base += nwaves * 64) {
    const int64_t row = base + lane;
    const int64_t a = row < rows ? off[row] : 0;
    const int l = row < rows ? (int)(off[row + 1] - a) : 0;
    unsigned long long m = __ballot(l > 0);
    while (m) {
      const int k = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int64_t ak = __shfl(a, k, 64);
      const int lk = __shfl(l, k, 64);
      const char* src = slots + (base + k) * slot_bytes;
      for (int i = lane; i < lk; i += 64) dst[ak + i] = src[i];
    }
  }
}

// blob[0, *total) into page-locked host memory (both 16-byte aligned; the
// last word may run past the total into the buffers' slack)
__global__ __launch_bounds__(FLUSH_TB) void k_flush_out(const uint4* blob, const int64_t* total, uint4* dst,
                                                        int64_t cap) {
  const int64_t n = *total;
  if (n > cap) return;
  const int64_t nw = (n + 15) >> 4;
  for (int64_t i = (int64_t)blockIdx.x * FLUSH_TB + threadIdx.x; i < nw; i += (int64_t)gridDim.x * FLUSH_TB)
    dst[i] = blob[i];
}

__global__ __launch_bounds__(FLUSH_TB) void k_flush_add(uint32_t* dc, const uint32_t* sc, int64_t n32,
                                                        unsigned long long* ds, const unsigned long long* ss,
                                                        int64_t n64) {
  const int64_t tid = (int64_t)blockIdx.x * FLUSH_TB + threadIdx.x, nt = (int64_t)gridDim.x * FLUSH_TB;
  const int64_t q32 = n32 >> 2, q64 = n64 >> 1;  // (the buffers are hipMalloc'd: 16-byte aligned)
  for (int64_t i = tid; i < q32; i += nt) {
    uint4 d = ((uint4*)dc)[i];
    const uint4 s = ((const uint4*)sc)[i];
    d.x += s.x;
    d.y += s.y;
    d.z += s.z;
    d.w += s.w;
    ((uint4*)dc)[i] = d;
  }
  for (int64_t i = (q32 << 2) + tid; i < n32; i += nt) dc[i] += sc[i];
  for (int64_t i = tid; i < q64; i += nt) {
    ulonglong2 d = ((ulonglong2*)ds)[i];
    const ulonglong2 s = ((const ulonglong2*)ss)[i];
    d.x += s.x;
    d.y += s.y;
    ((ulonglong2*)ds)[i] = d;
  }
  for (int64_t i = (q64 << 1) + tid; i < n64; i += nt) ds[i] += ss[i];
}

unsigned grid_for(int64_t items, int64_t per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > 16384) g = 16384;
  return (unsigned)g;
}

}  // namespace

void launch_flush_rows(const FlushIn& in, char* slots, int64_t* len, FlushMeta* meta, hipStream_t s) {
  int lg = 0;
  while ((1 << lg) < in.nbins) ++lg;  // (nbins <= FLUSH_MAX_NBINS = 64: lg <= 6)
  hipLaunchKernelGGL(k_flush_rows, dim3(grid_for(in.rows, FLUSH_TB >> lg)), dim3(FLUSH_TB), 0, s, in, lg,
                     flush_slot_bytes(in.nbins), slots, len, meta);
}

void launch_flush_copy(int64_t rows, int slot_bytes, const char* slots, const int64_t* off, char* dst, int64_t cap,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_flush_copy, dim3(grid_for(rows, FLUSH_TB)), dim3(FLUSH_TB), 0, s, rows, slot_bytes, slots,
                     off, dst, cap);
}

void launch_flush_out(const char* blob, const int64_t* total, char* dst, int64_t cap, hipStream_t s) {
  hipLaunchKernelGGL(k_flush_out, dim3(grid_for(cap >> 4, FLUSH_TB * 4)), dim3(FLUSH_TB), 0, s, (const uint4*)blob,
                     total, (uint4*)dst, cap);
}

void launch_flush_add(uint32_t* dc, const uint32_t* sc, int64_t n32, unsigned long long* ds,
                      const unsigned long long* ss, int64_t n64, hipStream_t s) {
  hipLaunchKernelGGL(k_flush_add, dim3(grid_for(n32 >> 2, FLUSH_TB * 2)), dim3(FLUSH_TB), 0, s, dc, sc, n32, ds, ss,
                     n64);
}

}  // namespace otm
