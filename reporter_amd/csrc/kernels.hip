// kernels.hip -- the map-matching hot path as HIP kernels for gfx950 (CDNA4).
//
// Replaces valhalla.SegmentMatcher().Match (py/reporter_service.py:112) and
// report() (:110-215).  Every float expression below follows the evaluation
// order of the written spec (oracle/otm_oracle.c) and the file
// is compiled with -ffp-contract=off, so results are bit-identical to the CPU
// oracle: no FMA contraction, IEEE division and sqrt, and order-independent
// fixed points (label-correcting search == Dijkstra, see K4).
//
// Execution model: wave64.  The irregular stages run one wavefront per unit
// of work (probe, column pair, trace) in 64-thread workgroups, grid-striding,
// with their working sets (edge hash, search labels, frontiers) in LDS.  No
// stage is a dense contraction; MFMA is deliberately unused.  Graph arrays are
// read-only and small enough (tens of MB at city scale) to live in L2 / the
// 256 MB Infinity Cache after first touch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include <hipcub/hipcub.hpp>

#include "kernels.h"
#include "otmatch.h"

namespace otm {

namespace {

// metres per degree of rules 1 and 2: one digit off (float)(20037581.187 / 180) =
// 111319.8954833 of Batch.java:33, kept so that results stay what they were; the oracle uses the same
#define MPD_F 111319.4954833f
constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr unsigned long long LAB_NONE = ~0ull;
constexpr int TB = 64;  // one wavefront per workgroup for the wave kernels
// A one-wavefront block's LDS operations execute in issue order, so its
// cross-lane LDS hand-offs need only the compiler kept from moving memory
// accesses across this point.  __syncthreads() would also wait for every
// global load and store in flight (s_waitcnt vmcnt(0)): the next chunks'
// prefetches, or the last item's result stores before the next item starts.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_wave_barrier();
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ float cos_deg(float deg) {
  const float x = deg * 0.017453292519943295f;
  const float x2 = x * x;
  float c = -1.1470745597729725e-11f;
  c = c * x2 + 2.08767569878681e-09f;
  c = c * x2 - 2.755731922398589e-07f;
  c = c * x2 + 2.48015873015873e-05f;
  c = c * x2 - 0.001388888888888889f;
  c = c * x2 + 0.041666666666666664f;
  c = c * x2 - 0.5f;
  c = c * x2 + 1.0f;
  return c;
}

__device__ __forceinline__ float gc_dist(float la, float lo, float lb, float lob) {
  const float ls = MPD_F * cos_deg((la + lb) * 0.5f);
  const float dx = (lob - lo) * ls;
  const float dy = (lb - la) * MPD_F;
  return sqrtf(dx * dx + dy * dy);
}

// squared distance from the probe to shape segment a-b: the sqd half of
// project() below, same float evaluation order
__device__ __forceinline__ float seg_sqdist(float alat, float alon, float blat, float blon, float lat, float lon,
                                            float ls) {
  const float ax = (alon - lon) * ls;
  const float ay = (alat - lat) * MPD_F;
  const float bx = (blon - lon) * ls;
  const float by = (blat - lat) * MPD_F;
  const float vx = bx - ax;
  const float vy = by - ay;
  const float l2 = vx * vx + vy * vy;
  // branch-free: the quotient of a zero-length segment (inf / nan) is
  // selected away, so the lanes of the scan never split here
  const float dot = ax * vx + ay * vy;
  float t = -dot / l2;
  t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
  t = l2 > 0.0f ? t : 0.0f;
  const float px = ax + t * vx;
  const float py = ay + t * vy;
  return px * px + py * py;
}

// seg_sqdist over an ent_geo word {alat, alon, blat, blon}, the two coordinates
// of a point as one pair: ll = {lat, lon}, sc = {MPD_F, ls}.  The same
// operations on the same operands as seg_sqdist (the sums of two products with
// their terms the other way round, which an IEEE sum does not see), so the same
// bits; written in pairs so that the lane tier's scan gets v_pk_* instructions
// without the register shuffles that the vectoriser's own pairing needs.
typedef float float2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float seg_sqdist_pk(const float4 G, float2_t ll, float2_t sc) {
  const float2_t a = (float2_t{G.x, G.y} - ll) * sc;  // {ay, ax}
  const float2_t b = (float2_t{G.z, G.w} - ll) * sc;
  const float2_t v = b - a;
  const float2_t vv = v * v;
  const float l2 = vv.y + vv.x;
  const float2_t av = a * v;
  const float dot = av.y + av.x;
  float t = -dot / l2;
  t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
  t = l2 > 0.0f ? t : 0.0f;
  const float2_t p = a + t * v;
  const float2_t pp = p * p;
  return pp.y + pp.x;
}

// (round 4 A/B, not kept: a division-free early out in the lane tier's scan
// for segments whose whole line lies beyond the radius measured slower --
// k_cand_lane 0.229 vs 0.221 ms on config 2, 1.89 vs 1.85 on config 4; the
// branch splits the wave where the division did not)

// A projection's inputs (the shape segment's two points and cumulative
// metres, the edge length and its last shape point), loaded apart from the
// arithmetic so a caller can issue several projections' loads at once.
// Two dependent trips, three loads: the edge's projection record, then the
// segment's two point records, 32 contiguous bytes (DevGraph::e_proj / s_pt,
// the floats of s_lat / s_lon / s_cum and e_len themselves).  rep_from and
// end are the node snap's answers, loaded with the operands: the start node's
// representative edge, and point b's end word -- PT_INNER unless b is its
// edge's last shape point, there the end node's representative edge, or -2
// when that node has no outgoing edge.
constexpr int32_t PT_INNER = -1;  // (engine.cpp writes the same value)
struct ProjIn {
  float alon, alat, blon, blat, ca, cb, len;
  int32_t rep_from, end;
};
__device__ __forceinline__ ProjIn proj_points(const DevGraph& g, const int4 er, int32_t k) {
  ProjIn in;
  const int32_t a = er.x + k;
  // (a's end word is not needed: twelve bytes, a register less in flight)
  typedef float float3_t __attribute__((ext_vector_type(3)));
  const float3_t pa = *(const float3_t*)(g.s_pt + a);
  const float4 pb = g.s_pt[a + 1];
  in.alat = pa.x;
  in.alon = pa.y;
  in.ca = pa.z;
  in.blat = pb.x;
  in.blon = pb.y;
  in.cb = pb.z;
  in.end = __float_as_int(pb.w);
  in.len = __int_as_float(er.z);
  in.rep_from = er.w;
  return in;
}
__device__ __forceinline__ ProjIn proj_load(const DevGraph& g, int32_t e, int32_t k) {
  return proj_points(g, g.e_proj[e], k);
}
__device__ __forceinline__ void proj_calc(const ProjIn& in, float lat, float lon, float ls, float& sqd,
                                          float& off_out, bool& at_end) {
  const float ax = (in.alon - lon) * ls;
  const float ay = (in.alat - lat) * MPD_F;
  const float bx = (in.blon - lon) * ls;
  const float by = (in.blat - lat) * MPD_F;
  const float vx = bx - ax;
  const float vy = by - ay;
  const float l2 = vx * vx + vy * vy;
  float t = 0.0f;
  if (l2 > 0.0f) {
    const float dot = ax * vx + ay * vy;
    t = -dot / l2;
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
  }
  const float px = ax + t * vx;
  const float py = ay + t * vy;
  sqd = px * px + py * py;
  float off = in.ca + t * (in.cb - in.ca);
  off_out = off > in.len ? in.len : off;
  // clamped to the edge's last shape point (b == last: b's end word is not
  // PT_INNER): the projection is its end node
  at_end = t == 1.0f && in.end != PT_INNER;
}
// node snap of a projection at offset off: the representative
// (first outgoing) edge of the node it snaps to -- the edge's start node at
// offset 0, its end node when clamped there and the node has an outgoing
// edge -- or a negative value.  The node candidate is carried as (that edge,
// offset 0).
__device__ __forceinline__ int32_t snap_rep(const ProjIn& in, float off, bool at_end) {
  return off == 0.0f ? in.rep_from : (at_end ? in.end : -1);
}
// The closest projection on the whole of an edge, from its projection record:
// every shape segment, ties to the lowest (the record's two shape indexes give
// the segment count, so the edge costs one load before its points).
__device__ __forceinline__ void project_edge(const DevGraph& g, const int4 er, float lat, float lon, float ls,
                                             float& bsq, float& boff) {
  bsq = INFINITY;
  boff = 0.0f;
  const int32_t nsh = er.y - er.x;
  for (int sg = 0; sg < nsh; ++sg) {
    float sqd, off;
    bool at_end;
    proj_calc(proj_points(g, er, sg), lat, lon, ls, sqd, off, at_end);
    if (sqd < bsq) {
      bsq = sqd;
      boff = off;
    }
  }
}
__device__ __forceinline__ void project(const DevGraph& g, int32_t e, int32_t k, float lat, float lon, float ls,
                                        float& sqd, float& off_out, bool& at_end) {
  proj_calc(proj_load(g, e, k), lat, lon, ls, sqd, off_out, at_end);
}
__device__ __forceinline__ void project(const DevGraph& g, int32_t e, int32_t k, float lat, float lon, float ls,
                                        float& sqd, float& off_out) {
  bool at_end;
  project(g, e, k, lat, lon, ls, sqd, off_out, at_end);
}
__device__ __forceinline__ float probe_radius(const DevParams& P, float acc) {
  const float a = acc > 0.0f ? acc : P.gps_accuracy;
  const float r = a > P.search_radius ? a : P.search_radius;
  return r < P.max_search_radius ? r : P.max_search_radius;
}

__device__ __forceinline__ uint32_t fbits(float f) { return __float_as_uint(f); }
__device__ __forceinline__ float bitsf(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t hash32(uint32_t x) { return x * 2654435761u; }

__device__ __forceinline__ void cadd(unsigned long long* c, unsigned long long v) {
  if (c && v) atomicAdd(c, v);
}

// candidate slot j of point p (DevWork: KIN inline slots, the rest overflow)
__device__ __forceinline__ int2 crec(const DevWork& w, int64_t p, int j) {
  return j < KIN ? w.cand_eo[p * KIN + j] : w.cand_xeo[p * KX + (j - KIN)];
}
__device__ __forceinline__ float cemis(const DevWork& w, int64_t p, int j) {
  return j < KIN ? w.cand_em[p * KIN + j] : w.cand_xem[p * KX + (j - KIN)];
}
__device__ __forceinline__ void cput(const DevWork& w, int64_t p, int j, int32_t e, float off, float em) {
  if (j < KIN) {
    w.cand_eo[p * KIN + j] = make_int2(e, __float_as_int(off));
    w.cand_em[p * KIN + j] = em;
  } else {
    w.cand_xeo[p * KX + (j - KIN)] = make_int2(e, __float_as_int(off));
    w.cand_xem[p * KX + (j - KIN)] = em;
  }
}

// ============================================================== turn costs
// deviation from straight on (0..180 degrees) of the turn from an edge whose
// end heading is hin into an edge whose start heading is hout
__device__ __forceinline__ uint32_t turn_deg(uint32_t hin, uint32_t hout) {
  int d = (int)hout - (int)hin;
  d += d < 0 ? 360 : 0;
  return (uint32_t)(d <= 180 ? d : 360 - d);
}
// transition cost (turn_cost + |r - gc|) / beta of DESIGN.md §3; the turn
// cost is integer 1/64 m units summed over the route's turns (order-free),
// exact in a float below 2^24
__device__ __forceinline__ float trans_cost(uint32_t units, float r, float gcv, float beta) {
  units = units > TURN_UNITS_MAX ? TURN_UNITS_MAX : units;
  const float tc = (float)units * 0.015625f;
  const float diff = fabsf(r - gcv);
  return (tc + diff) / beta;
}

// ============================================================== node candidates
// DESIGN.md §3 node snap: a candidate at offset 0 is the node candidate of its
// edge's start node (K2 snaps every end-of-edge projection to the node, so
// an edge candidate never sits at offset 0).  Its routes start at the node
// with nothing left to drive, and it has no heading on its side of a route.
constexpr uint32_t NO_HEAD = 0xFFFFu;
__device__ __forceinline__ bool cand_node(float off) { return off == 0.0f; }
__device__ __forceinline__ int32_t src_node(const DevGraph& g, int32_t e, float off) {
  return cand_node(off) ? g.e_from[e] : g.e_to[e];
}
__device__ __forceinline__ float src_start(const DevGraph& g, int32_t e, float off) {
  return cand_node(off) ? 0.0f : g.e_len[e] - off;
}
__device__ __forceinline__ uint32_t src_head(const DevGraph& g, int32_t e, float off) {
  return cand_node(off) ? NO_HEAD : (uint32_t)g.e_head_in[e];
}
__device__ __forceinline__ uint32_t dst_head(const DevGraph& g, int32_t e, float off) {
  return cand_node(off) ? NO_HEAD : (uint32_t)g.e_head_out[e];
}
// DESIGN.md §3 rule 4, same edge: from (e, oi) to (e, oj) the route is along
// the edge when oj is not before oi; when oj is behind oi and both are edge
// candidates the step is a stay (GPS noise moved the later probe back; a
// vehicle does not reverse along a directed edge): route distance 0, no
// turns, no traversal, the position on the edge staying at the largest offset
// reached.  oracle/otm_oracle.c same_edge_step / same_edge_dist.
__device__ __forceinline__ bool same_edge_step(int32_t ei, float oi, int32_t ej, float oj) {
  return ei == ej && (oj >= oi || (!cand_node(oj) && !cand_node(oi)));
}
__device__ __forceinline__ float same_edge_dist(float oi, float oj) { return oj >= oi ? oj - oi : 0.0f; }
// turn units of one turn (none when either side is a node candidate)
__device__ __forceinline__ uint32_t turn_units(const uint32_t* TU, uint32_t hin, uint32_t hout) {
  return (hin == NO_HEAD || hout == NO_HEAD) ? 0u : TU[turn_deg(hin, hout)];
}

// wave-wide inclusive scan of an int (64 lanes)
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  return v;
}

// The batch bookkeeping is folded into the stage kernels: each kernel boundary
// in a stream costs ~5-10 us, and it once ran as five one-wave launches per batch.
// one thread: spill snapshot k of the per-stage counters, optionally resetting them
__device__ __forceinline__ void fold_snap(DevWork& w, int k, bool reset) {
  for (int t = 0; t < CTR_STAGE_WORDS; ++t) {
    w.snap[CTR_STAGE_WORDS * k + t] = w.counters_i32[t];
    if (reset) w.counters_i32[t] = 0;
  }
}
// one lane, about to push onto a list that group G's kernels drain: when the
// group is dormant (kernels.h TierGroup) nothing will drain it this attempt,
// so the batch aborts and says which group it needs
template <int G>
__device__ __forceinline__ void tier_wake(const DevWork& w) {
  if (G != 0 && (w.dormant & G)) {
    atomicOr(&w.counters_i32[CTR_TIER_WAKE], G);
    *w.abort = 1;
  }
}
// one lane: p onto the list that slot C counts (G: the TierGroup that drains
// it when that group is launched on demand, 0: drained by a kernel that always runs)
template <CtrSlot C, int G = 0>
__device__ __forceinline__ void spill_push(const DevWork& w, int32_t p) {
  const SpillRef s = spill_of<C>(w);
  tier_wake<G>(w);
  s.list[atomicAdd(s.count, 1)] = p;
}
// every transition kernel's first test: the matrices' total against the
// buffer (the first kernel to run sets the abort flag for the rest)
__device__ __forceinline__ bool trans_over_cap(const DevBatch& b, const DevWork& w) {
  if (w.trans_off[b.n_points] <= w.trans_cap) return false;
  *w.abort = 1;
  return true;
}

// ============================================================== spatial work order
__device__ __forceinline__ int hilbert_d(int x, int y) {
  int d = 0;
  for (int sft = ORDER_SIDE / 2; sft > 0; sft >>= 1) {
    const int rx = (x & sft) > 0;
    const int ry = (y & sft) > 0;
    d += sft * sft * ((3 * rx) ^ ry);
    if (ry == 0) {
      if (rx == 1) {
        x = ORDER_SIDE - 1 - x;
        y = ORDER_SIDE - 1 - y;
      }
      const int tmp = x;
      x = y;
      y = tmp;
    }
  }
  return d;
}

__device__ __forceinline__ int tile_of(const DevGraph& g, float lat, float lon) {
  int ty = (int)((lat - g.bb_lat0) * g.bb_inv_h);
  int tx = (int)((lon - g.bb_lon0) * g.bb_inv_w);
  ty = ty < 0 ? 0 : (ty >= ORDER_SIDE ? ORDER_SIDE - 1 : ty);
  tx = tx < 0 ? 0 : (tx >= ORDER_SIDE ? ORDER_SIDE - 1 : tx);
  return hilbert_d(tx, ty);
}

// Wave-aggregated atomicAdd(&ctr[key], 1): one atomic per distinct key in
// the wave; returns this lane's slot.  64 consecutive points of a config-2
// trace cross about 15 tiles, so the lanes are first matched by key in
// registers (agg_match: one round per distinct key, no memory operation in
// it); then every key's first lane adds its count in ONE atomic instruction,
// and the wave waits for one round trip, not for one per key in turn.  All 64
// lanes call these.
struct AggMatch {
  int leader;  // the first lane with this lane's key
  int rank;    // lanes with the key below this one
  int count;   // lanes with the key
};
__device__ __forceinline__ AggMatch agg_match(int key, bool active) {
  const int lane = threadIdx.x & 63;
  unsigned long long pending = __ballot(active);
  AggMatch m{lane, 0, 0};
  while (pending) {
    const int leader = __ffsll((long long)pending) - 1;
    const int k = __shfl(key, leader, 64);
    const unsigned long long grp = __ballot(((pending >> lane) & 1ull) && key == k);
    if ((grp >> lane) & 1ull) {
      m.leader = leader;
      m.rank = (int)__popcll(grp & ((1ull << lane) - 1ull));
      m.count = (int)__popcll(grp);
    }
    pending &= ~grp;
  }
  return m;
}
__device__ __forceinline__ int wave_agg_slot(int32_t* ctr, int key, bool active) {
  const AggMatch m = agg_match(key, active);
  int base = 0;
  if (active && m.leader == (int)(threadIdx.x & 63)) base = atomicAdd(&ctr[key], m.count);
  return __shfl(base, m.leader, 64) + m.rank;
}
// ... counting only (K1): the atomics return nothing, so the wave does not wait at all
__device__ __forceinline__ void wave_agg_count(int32_t* ctr, int key, bool active) {
  const AggMatch m = agg_match(key, active);
  if (active && m.leader == (int)(threadIdx.x & 63)) atomicAdd(&ctr[key], m.count);
}

// one block: exclusive scan of the tile counts (Hilbert order), cursors, and
// the 8 group cuts at the tile boundaries nearest k/8 of the columns.  Having
// read the counts it zeroes them for the next batch's K1 (they start as zeros
// at allocation, engine.cpp bind_order), so no batch pays a memset for them.
__global__ __launch_bounds__(1024) void k_order_plan(int32_t* tile_cnt, int32_t* cursor, int32_t* grp) {
  __shared__ int32_t part[1024];
  __shared__ int32_t cut[ORDER_GROUPS + 1];
  constexpr int PER = ORDER_TILES / 1024;
  const int tid = threadIdx.x;
  int32_t v[PER], sum = 0;
  for (int k = 0; k < PER; ++k) {
    v[k] = tile_cnt[tid * PER + k];
    sum += v[k];
  }
  part[tid] = sum;
  if (tid <= ORDER_GROUPS) cut[tid] = 0x7fffffff;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int32_t x = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += x;
    __syncthreads();
  }
  const int32_t total = part[1023];
  int32_t run = part[tid] - sum;
  // start of the tile before this thread's first one (-1 before tile 0)
  int32_t prev_start = tid == 0 ? -1 : run - tile_cnt[tid * PER - 1];
  for (int k = 0; k < PER; ++k) {
    cursor[tid * PER + k] = run;
    // group gi starts at the first tile whose start reaches gi/8 of the
    // columns: exactly one tile sees prev_start < want <= run
    for (int gi = 1; gi < ORDER_GROUPS; ++gi) {
      const int64_t want = ((int64_t)total * gi + ORDER_GROUPS - 1) / ORDER_GROUPS;
      if (run >= want && prev_start < want) cut[gi] = run;
    }
    prev_start = run;
    run += v[k];
  }
  __syncthreads();
  // (every thread has read its neighbour's last count by now)
  for (int k = 0; k < PER; ++k) tile_cnt[tid * PER + k] = 0;
  if (tid == 0) {
    grp[0] = 0;
    int32_t prev = 0;
    for (int gi = 1; gi < ORDER_GROUPS; ++gi) {
      const int32_t c = cut[gi] > total ? total : cut[gi];
      prev = c > prev ? c : prev;
      grp[gi] = prev;
    }
    grp[ORDER_GROUPS] = total;
  }
}

__global__ __launch_bounds__(256) void k_order_scatter(DevBatch b, DevWork w, const uint16_t* tile, int32_t* cursor,
                                                       int32_t* item) {
  for (int64_t p0 = (int64_t)blockIdx.x * 256; p0 < b.n_points; p0 += (int64_t)gridDim.x * 256) {
    const int64_t p = p0 + threadIdx.x;
    const bool col = p < b.n_points && w.is_col[p];
    const int t = col ? (int)tile[p] : 0;
    const int pos = wave_agg_slot(cursor, t, col);
    if (col) item[pos] = (int32_t)p;
    if (col && w.colrec_pos) w.colrec_pos[p] = pos;  // where K3 writes the column's K4 record
  }
}

// ============================================================== K1 columns
// One wavefront per trace: lanes stage the trace's coordinates in LDS and
// compute the distance of every point to its predecessor in parallel; lane 0
// then runs the interpolation filter (a point is a column iff it lies at least
// interpolation_distance from the last column) out of LDS, recomputing the
// distance only where the last column is not the immediate predecessor.
// points staged in LDS (longer traces take the serial form): 256 leaves room
// for 8 waves per SIMD (512: ~4.6), 0.050 -> 0.046 ms on config 2, 0.42 ->
// 0.37 ms on a config-3 shard
#ifndef OTM_COL_PTS
#define OTM_COL_PTS 256
#endif
constexpr int COL_PTS = OTM_COL_PTS;
// seg_base: DevOut::seg_base [T+1], zeroed here per trace for K7a's sums (it was a memset of its own)
__global__ __launch_bounds__(TB) void k_columns(DevGraph g, DevBatch b, DevParams P, DevWork w, int64_t* seg_base) {
  __shared__ float sLat[COL_PTS], sLon[COL_PTS], sGc[COL_PTS];
  __shared__ int32_t sPrev[COL_PTS];
  __shared__ uint8_t sCol[COL_PTS];
  const int lane = threadIdx.x;
  if (blockIdx.x == 0) {
    // the batch's tier counters (per stage and per batch) and abort flag start at zero
    if (lane < CTR_ZEROED_WORDS) w.counters_i32[lane] = 0;
    if (lane == 0) *w.abort = 0;
    if (lane == 0) seg_base[b.n_traces] = 0;  // (the element the scan leaves the bounds' total in)
  }
  for (int32_t t = blockIdx.x; t < b.n_traces; t += gridDim.x) {
    const int64_t a = b.trace_off[t], e = b.trace_off[t + 1];
    const int n = (int)(e - a);
    int ncols = 0;
    if (n > COL_PTS) {
      // long trace: the same filter straight from HBM
      if (lane == 0) {
        int64_t last = -1;
        for (int64_t p = a; p < e; ++p) {
          float gcv = 0.0f;
          if (last >= 0) gcv = gc_dist(b.lat[last], b.lon[last], b.lat[p], b.lon[p]);
          const bool col = last < 0 || gcv >= P.interp;
          w.is_col[p] = col ? 1 : 0;
          w.gc[p] = col ? gcv : 0.0f;
          w.prevc[p] = (int32_t)last;  // a non-column: the column before it (K7a)
          if (col) {
            last = p;
            ++ncols;
            if (w.ord.tile_cnt) {  // spatial order tile (serial here: long traces are rare)
              const int tl = tile_of(g, b.lat[p], b.lon[p]);
              w.ord.tile[p] = (uint16_t)tl;
              atomicAdd(&w.ord.tile_cnt[tl], 1);
            }
          }
        }
      }
      for (int64_t p = a + lane; p < e; p += TB) {
        w.probe[p] = make_float4(b.lat[p], b.lon[p], b.acc[p], 0.0f);
        w.pt_trace[p] = t;
        w.ncand[p] = 0;
        w.route_dist[p] = 0.0f;
        w.ipos[p] = -1.0f;
        w.nextc[p] = -1;
      }
    } else {
      for (int pl = lane; pl < n; pl += TB) {
        sLat[pl] = b.lat[a + pl];
        sLon[pl] = b.lon[a + pl];
      }
      __syncthreads();
      bool near = false;  // some step shorter than the interpolation distance
      for (int pl = lane; pl < n; pl += TB) {
        const float d = pl > 0 ? gc_dist(sLat[pl - 1], sLon[pl - 1], sLat[pl], sLon[pl]) : 0.0f;
        sGc[pl] = d;
        near = near || (pl > 0 && !(d >= P.interp));
      }
      __syncthreads();
      if (__ballot(near) == 0ull) {
        // every step is at least the interpolation distance: every point is a
        // column linked to the one before (what the serial filter below gives)
        for (int pl = lane; pl < n; pl += TB) {
          sCol[pl] = 1;
          sPrev[pl] = pl > 0 ? (int32_t)(a + pl - 1) : -1;
        }
        ncols = n;
      } else if (lane == 0) {
        int last = -1;
        for (int pl = 0; pl < n; ++pl) {
          float gcv = 0.0f;
          if (last >= 0) gcv = last == pl - 1 ? sGc[pl] : gc_dist(sLat[last], sLon[last], sLat[pl], sLon[pl]);
          const bool col = last < 0 || gcv >= P.interp;
          sCol[pl] = col ? 1 : 0;
          sGc[pl] = col ? gcv : 0.0f;
          sPrev[pl] = last >= 0 ? (int32_t)(a + last) : -1;  // a non-column: the column before it (K7a)
          if (col) {
            last = pl;
            ++ncols;
          }
        }
      }
      __syncthreads();
      for (int c0 = 0; c0 < n; c0 += TB) {
        const int pl = c0 + lane;
        const bool in = pl < n;
        const bool col = in && sCol[pl];
        if (in) {
          const int64_t p = a + pl;
          w.probe[p] = make_float4(sLat[pl], sLon[pl], b.acc[p], 0.0f);
          w.pt_trace[p] = t;
          w.is_col[p] = sCol[pl];
          w.gc[p] = sGc[pl];
          w.prevc[p] = sPrev[pl];
          // later stages write these for columns only (spatial work order)
          w.ncand[p] = 0;
          w.route_dist[p] = 0.0f;
          w.ipos[p] = -1.0f;
          w.nextc[p] = -1;
          // (path_len / path_off: K6 writes them for every column, and only
          // columns' are read)
        }
        if (w.ord.tile_cnt) {  // spatial order: this column's tile, counted per wave
          const int tl = col ? tile_of(g, sLat[pl], sLon[pl]) : 0;
          if (col) w.ord.tile[a + pl] = (uint16_t)tl;
          wave_agg_count(w.ord.tile_cnt, tl, col);
        }
      }
      __syncthreads();
    }
    if (lane == 0) {
      w.trace_err[t] = 0;
      seg_base[t] = 0;  // K7a adds the trace's segment bound here
      if (w.ctr) {
        cadd(&w.ctr->points, (unsigned long long)n);
        cadd(&w.ctr->columns, (unsigned long long)ncols);
      }
    }
  }
}

// The items a block walks: the spatial order's group blockIdx % 8 (lanes
// or waves over it), or every point in natural order.  per_block = items
// per block per step (threads for lane kernels, 1 for wave kernels).
struct ItemRange {
  int64_t i0, i1, stride;
  bool ordered;
};
__device__ __forceinline__ ItemRange item_range(const DevWork& w, const DevBatch& b, bool ordered, int per_block) {
  ItemRange r;
  r.ordered = ordered;
  const int tid = per_block > 1 ? (int)threadIdx.x : 0;
  if (ordered) {
    const int grp = blockIdx.x % ORDER_GROUPS;
    r.i0 = w.ord.grp[grp] + (int64_t)(blockIdx.x / ORDER_GROUPS) * per_block + tid;
    r.i1 = w.ord.grp[grp + 1];
    r.stride = (int64_t)(gridDim.x / ORDER_GROUPS) * per_block;
  } else {
    r.i0 = (int64_t)blockIdx.x * per_block + tid;
    r.i1 = b.n_points;
    r.stride = (int64_t)gridDim.x * per_block;
  }
  return r;
}

// ============================================================== K2 candidates
constexpr int HCAP = 512;  // edge hash slots (>= 2 * MAX_HITS)
// a lane-tier entry that is a node candidate (edge << 4 keeps bits 4..30:
// graphs up to 2^27 edges, checked at engine load)
constexpr uint32_t NODE_ENT = 0x80000000u;
#ifndef OTM_CAND_LANE_CAP
#define OTM_CAND_LANE_CAP 8
#endif
// lane tier: distinct edges kept per probe.  8 measured best on config 2
// (0.39 ms with the wave tier vs 0.40 at 12, 0.45 at 16): a smaller LDS list
// buys occupancy; the ~1 % of probes with more edges in range spill.
constexpr int CAND_LANE_CAP = OTM_CAND_LANE_CAP;
// lane tier block size: 256 (round 4: k_cand_lane 1.518 vs 1.576 ms at 128 on
// config 4, 0.220 vs 0.222 on config 2; 64 no better, profiles/r04_ab/knobs/)
#ifndef OTM_CAND_TB
#define OTM_CAND_TB 256
#endif
// min waves per SIMD for the lane tier: 8 caps it at 64 VGPRs (0.276 ->
// 0.255 ms on config 2, 3.86 -> 3.76 ms on config 4; 6 measured no change)
#ifndef OTM_CAND_WAVES
#define OTM_CAND_WAVES 8
#endif
constexpr int CAND_TB = OTM_CAND_TB;
// lane tier: a kept entry's offset along its edge (the snap pass's
// projection) waits for the output loop, which then loads no graph word, in
// registers: one per list slot in snap order, found through a packed 8 x 3-bit
// permutation word that the merge's move and the sort's swaps update (no LDS,
// the 64-VGPR cap and 8 waves per SIMD kept).  Against projecting each chosen
// entry again in the output loop, and against a third LDS array: DESIGN.md §5
// K2, profiles/graph_words/
#ifndef OTM_CAND_INFL
#define OTM_CAND_INFL 2
#endif
constexpr int CAND_INFL = OTM_CAND_INFL;
// lane tier node snap: entries whose projection loads are issued together
// (more would spill under the 64-VGPR cap)
#ifndef OTM_SNAP_B
#define OTM_SNAP_B 2
#endif
constexpr int SNAP_B = OTM_SNAP_B;
// wave-reduce a per-lane count and add it to a device counter (all 64 lanes active)
__device__ __forceinline__ void wave_cadd(unsigned long long* c, unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(c, v);
}

// Lane tier of the candidate search: one probe per LANE.  The lane walks its
// probe's grid cells serially (the same cell range, entries and projection as
// the wave kernel below), keeps each edge's best (sqdist, shape segment) in a
// private LDS list of CAND_LANE_CAP slots (interleaved by thread), then
// selection-sorts the first max_candidates by (sqdist, edge).  Probes with
// more distinct edges in range spill to the wave kernel, which also applies
// the MAX_HITS spec limit.
template <bool CTR>
__global__ __launch_bounds__(CAND_TB, OTM_CAND_WAVES) void k_cand_lane(DevGraph g, DevBatch b, DevParams P, DevWork w) {
  __shared__ uint32_t sE[CAND_LANE_CAP * CAND_TB];  // edge << 4 | shape segment
  __shared__ float sQ[CAND_LANE_CAP * CAND_TB];     // best squared distance
  uint32_t* E = sE + threadIdx.x;
  float* Q = sQ + threadIdx.x;
  static_assert(CAND_LANE_CAP <= 8 && CAND_LANE_CAP % SNAP_B == 0, "3-bit slots; whole snap steps");
  constexpr int S = CAND_TB;
  unsigned long long c_cells = 0, c_ent = 0, c_cand = 0;
  const ItemRange R = item_range(w, b, (P.order_mask & ORDER_CAND) != 0, CAND_TB);
  for (int64_t it = R.i0; it < R.i1; it += R.stride) {
    const int64_t p = R.ordered ? (int64_t)w.ord.item[it] : it;
    if (!R.ordered && !w.is_col[p]) continue;
    if (P.cand_wave_all) {
      spill_push<CTR_CAND_WAVE>(w, (int32_t)p);
      continue;
    }
    const float4 pr = w.probe[p];  // {lat, lon, accuracy} of the column (K1), one line
    const float lat = pr.x, lon = pr.y;
    const float r = probe_radius(P, pr.z);
    const float r2 = r * r;
    const float ls = MPD_F * cos_deg(lat);
    const float dlat = r / MPD_F;
    const float dlon = r / ls;
    const double la_lo = ((double)lat - (double)dlat - g.lat0) / g.cell;
    const double la_hi = ((double)lat + (double)dlat - g.lat0) / g.cell;
    const double lo_lo = ((double)lon - (double)dlon - g.lon0) / g.cell;
    const double lo_hi = ((double)lon + (double)dlon - g.lon0) / g.cell;
    const double R = g.grid_rows, Cn = g.grid_cols;
    int r0 = 0, r1 = -1, c0 = 0, c1 = -1;
    if (!(la_hi < 0.0 || lo_hi < 0.0 || la_lo >= R || lo_lo >= Cn)) {
      r0 = la_lo < 0.0 ? 0 : (int)floor(la_lo);
      r1 = la_hi >= R ? (int)R - 1 : (int)floor(la_hi);
      c0 = lo_lo < 0.0 ? 0 : (int)floor(lo_lo);
      c1 = lo_hi >= Cn ? (int)Cn - 1 : (int)floor(lo_hi);
    }
    int n = 0;
    bool spill = false;
    // cells c0..c1 of one grid row are adjacent in the row-major cell CSR:
    // each row's entries are one contiguous range
    const unsigned long long cells = (unsigned long long)(r1 - r0 + 1) * (unsigned long long)(c1 - c0 + 1);
    unsigned long long ents = 0;
    // one hit into the lane's list: insert, update or spill
    auto insert = [&](uint32_t ent, float sqd) {
      const uint32_t e = ent >> 4;
      // every slot's edge read at once and unconditionally -- slots past
      // n hold stale words, masked by the select -- so the compiler
      // emits eight LDS reads and selects, not eight guarded branches
      // (one LDS round trip per hit instead of up to 8)
      uint32_t ev[CAND_LANE_CAP];
#pragma unroll
      for (int m = 0; m < CAND_LANE_CAP; ++m) ev[m] = E[m * S];
      int f = -1;
#pragma unroll
      for (int m = 0; m < CAND_LANE_CAP; ++m) f = (m < n && (ev[m] >> 4) == e) ? m : f;
      if (f < 0) {
        if (n == CAND_LANE_CAP) {
          spill = true;
          return;
        }
        E[n * S] = ent;
        Q[n * S] = sqd;
        ++n;
      } else {
        const float qf = Q[f * S];
        if (sqd < qf || (sqd == qf && (ent & 15u) < (E[f * S] & 15u))) {
          Q[f * S] = sqd;
          E[f * S] = ent;
        }
      }
    };
    const float2_t pll = {lat, lon}, psc = {MPD_F, ls};
    // (engine.cpp clamps it to 1..64, which this leaves as it is; any other
    // value lands there too, in scalar operations: 0 would never advance, and
    // the mask has 64 bits)
    const uint32_t W = (((uint32_t)P.cand_chunk - 1u) & 63u) + 1u;
    // Three grid rows at a time, their entry ranges laid end to end as one
    // index range 0..tot: index i is entry i + qa[0] below e1, i + qa[1] - e1
    // below e2, i + qa[2] - e2 from there (cell_off is 32 bits wide; the sums wrap and come out
    // right).  The six offsets are loaded together -- one round trip where a
    // row at a time took three -- and a lane with short rows does not wait at
    // each row for the wave's longest one: the wave runs max-over-lanes of the
    // rows' sum, not the sum over rows of the max.
    for (int rg = r0; rg <= r1 && !spill; rg += 3) {
      uint32_t qa[3], qb[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const size_t rbase = (size_t)(rg + j <= r1 ? rg + j : r1) * (size_t)g.grid_cols;
        qa[j] = g.cell_off[rbase + c0];
        qb[j] = g.cell_off[rbase + c1 + 1];
      }
      const uint32_t e1 = qb[0] - qa[0];
      const uint32_t e2 = e1 + (rg + 1 <= r1 ? qb[1] - qa[1] : 0u);
      const uint32_t tot = e2 + (rg + 2 <= r1 ? qb[2] - qa[2] : 0u);
      // (as sums of differences: two selects and one three-operand add per entry)
      const uint32_t b2 = qa[2] - e2, d1 = qa[1] - e1 - b2, d0 = qa[0] - (qa[1] - e1);
      if (CTR) ents += (unsigned long long)tot;
      auto entry_of = [&](uint32_t i) { return (size_t)(uint32_t)(i + b2 + (i < e2 ? d1 : 0u) + (i < e1 ? d0 : 0u)); };
      // The range in chunks of at most P.cand_chunk (<= 64) entries, each in
      // two phases.  Scan: every entry's squared distance, CAND_INFL loads in
      // flight per step; a hit only sets its bit in the lane's mask -- no
      // cell_ent load, no LDS, no list work, so no step waits on the one
      // before.  Drain: the mask's bits in ascending order, one insert each,
      // which is the order the entries have in their rows and the rows in the
      // grid.
      for (uint32_t done = 0, cn; done < tot && !spill; done += cn) {
        cn = tot - done < W ? tot - done : W;
        unsigned long long hit = 0ull;
        for (uint32_t k = 0; k < cn; k += CAND_INFL) {
          // (past the chunk's end the step's first entry once more, its bit
          // masked: the step's loads are issued together, behind no branch)
          float4 G[CAND_INFL];
#pragma unroll
          for (int u = 0; u < CAND_INFL; ++u) G[u] = g.ent_geo[entry_of(done + k + (u == 0 || k + u < cn ? u : 0))];
          __builtin_amdgcn_sched_barrier(0);  // (no arithmetic moved up between the loads)
          uint32_t bits = 0u;
#pragma unroll
          for (int u = 0; u < CAND_INFL; ++u) {
            const float sq = seg_sqdist_pk(G[u], pll, psc);
            bits |= ((uint32_t)(u == 0 || k + u < cn) & (uint32_t)(sq <= r2)) << u;
          }
          hit |= (unsigned long long)bits << k;
        }
        while (hit != 0ull && !spill) {
          // two hits a step, their four loads issued together (a lone last hit
          // twice, inserted once): each hit's id and, once more, its distance
          // -- the same operations on the same floats (no contraction), so
          // the bits the scan tested.  Half the drain's round trips: config 4,
          // whose sparse rows are mostly hits, 1,337 -> 1,287 us.
          const size_t qx = entry_of(done + (uint32_t)(__ffsll(hit) - 1));
          hit &= hit - 1ull;
          const bool two = hit != 0ull;
          const size_t qy = two ? entry_of(done + (uint32_t)(__ffsll(hit) - 1)) : qx;
          hit &= hit - 1ull;
          const uint32_t ent0 = g.cell_ent[qx], ent1 = g.cell_ent[qy];
          const float4 G0 = g.ent_geo[qx], G1 = g.ent_geo[qy];
          __builtin_amdgcn_sched_barrier(0);
          const float s0 = seg_sqdist_pk(G0, pll, psc), s1 = seg_sqdist_pk(G1, pll, psc);
          insert(ent0, s0);
          if (two && !spill) insert(ent1, s1);
        }
      }
    }
    if (spill) {
      spill_push<CTR_CAND_WAVE>(w, (int32_t)p);
      continue;
    }
    // node snap: an entry whose projection snaps to a node becomes that
    // node's candidate (NODE_ENT | first outgoing edge << 4), one per node
    // at the smallest distance.  First every entry's snap, SNAP_B entries'
    // loads issued together (a pure function of the entry: round 6 -- the
    // entry-by-entry walk waited on 3-4 dependent loads per entry); then the
    // merge in entry order, out of LDS.  A step is two dependent trips, three
    // loads an entry -- the edge's projection record, then the segment's two
    // point records, which carry both nodes' representative edges (proj_load)
    // -- where it was four trips and twelve loads through e_shape_off / e_len,
    // the SoA shape arrays, e_from / e_to and out_off.
    // The pass also keeps each entry's offset (0 for a node candidate) for the
    // output loop.  Its squared distance is not kept: Q already holds it.  Q
    // of an edge entry is seg_sqdist over ent_geo of the entry in E (the scan
    // writes the two together), ent_geo holds the very floats of s_lat /
    // s_lon that proj_load reads (engine_init copies them), and seg_sqdist is
    // proj_calc's sqd operation for operation (no contraction): where l2 > 0
    // the same t, elsewhere both take t = 0.
    float offr[CAND_LANE_CAP];  // by snap-pass slot; perm: list slot -> snap-pass slot
    uint32_t perm = 076543210u;
#pragma unroll
    for (int m0 = 0; m0 < CAND_LANE_CAP; m0 += SNAP_B) {
      // (unrolled so that offr is indexed by constants: registers, not scratch)
#pragma unroll
      for (int u = 0; u < SNAP_B; ++u) offr[m0 + u] = 0.0f;
      if (m0 >= n) continue;
      uint32_t em[SNAP_B];
      ProjIn pin[SNAP_B];
      // (not kept: the next step's edge records loaded during this one, so
      // that a step is one trip -- 24 B of scratch at the 64-register cap)
#pragma unroll
      for (int u = 0; u < SNAP_B; ++u) {
        em[u] = m0 + u < n ? E[(m0 + u) * S] : 0u;
        if (m0 + u < n) pin[u] = proj_load(g, (int32_t)(em[u] >> 4), (int32_t)(em[u] & 15u));
      }
#pragma unroll
      for (int u = 0; u < SNAP_B; ++u) {
        if (m0 + u < n) {
          float sqd, off;
          bool at_end;
          proj_calc(pin[u], lat, lon, ls, sqd, off, at_end);
          // the node's representative edge came with the operands: nothing
          // more to load (snap_rep)
          const int32_t rep = snap_rep(pin[u], off, at_end);
          if (rep >= 0) {
            E[(m0 + u) * S] = NODE_ENT | ((uint32_t)rep << 4);
            off = 0.0f;
          }
          offr[m0 + u] = off;
        }
      }
    }
    for (int m = 0; m < n; ++m) {
      const uint32_t key = E[m * S];
      if (!(key & NODE_ENT)) continue;
      int f = -1;
      for (int t = 0; t < m; ++t)
        if (E[t * S] == key) f = t;
      if (f >= 0) {
        const float qm = Q[m * S];
        if (qm < Q[f * S]) Q[f * S] = qm;
        --n;  // drop entry m: the last entry moves here and is examined next
        E[m * S] = E[n * S];
        Q[m * S] = Q[n * S];
        perm = (perm & ~(7u << (3 * m))) | ((perm >> (3 * n)) & 7u) << (3 * m);
        --m;
      }
    }
    const int K = n < P.max_candidates ? n : P.max_candidates;
    const float ds = (2.0f * P.sigma_z) * P.sigma_z;
    for (int j = 0; j < K; ++j) {
      // selection by (sqdist, edge, node before edge candidate)
      int m = j;
      float qm = Q[j * S];
      uint32_t em = E[j * S];
      for (int t = j + 1; t < n; ++t) {
        const float qt = Q[t * S];
        const uint32_t et = E[t * S];
        const uint32_t xt = (et & ~NODE_ENT) >> 4, xm = (em & ~NODE_ENT) >> 4;
        if (qt < qm || (qt == qm && (xt < xm || (xt == xm && et > em)))) {
          m = t;
          qm = qt;
          em = et;
        }
      }
      if (m != j) {
        Q[m * S] = Q[j * S];
        E[m * S] = E[j * S];
        Q[j * S] = qm;
        E[j * S] = em;
        const uint32_t x = ((perm >> (3 * m)) ^ (perm >> (3 * j))) & 7u;  // swap slots m and j
        perm ^= x << (3 * m) | x << (3 * j);
      }
    }
    // the K chosen, in order: the point's inline blocks whole (its 8-B
    // records in 16-B stores, its emissions in 16-B pieces; unused slots: edge
    // -1, emission +inf) -- whole lines to write back, not partially written
    // ones -- and any candidates past KIN one by one into its overflow slots
    int4* eo4 = (int4*)(w.cand_eo + p * KIN);
    float4* em4 = (float4*)(w.cand_em + p * KIN);
    float emv[4];
#pragma unroll
    for (int j = 0; j < (CAND_LANE_CAP > KIN ? CAND_LANE_CAP : KIN); j += 2) {
      if (j >= KIN && j >= K) break;
      int32_t e2[2];
      float o2[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int jj = j + u;
        e2[u] = -1;
        o2[u] = 0.0f;
        float emj = INFINITY;
        if (jj < K) {
          const uint32_t en = E[jj * S];
          const int32_t e = (int32_t)((en & ~NODE_ENT) >> 4);
          const float sqd = Q[jj * S];
          const uint32_t sl = (perm >> (3 * jj)) & 7u;
          float off = offr[0];
#pragma unroll
          for (int t = 1; t < CAND_LANE_CAP; ++t) off = sl == (uint32_t)t ? offr[t] : off;
          e2[u] = e;
          o2[u] = off;
          emj = sqd / ds;
        }
        emv[(j + u) & 3] = emj;
      }
      if (j < KIN) {
        eo4[j >> 1] = make_int4(e2[0], __float_as_int(o2[0]), e2[1], __float_as_int(o2[1]));
        if ((j & 3) == 2) em4[j >> 2] = make_float4(emv[0], emv[1], emv[2], emv[3]);
      } else {
#pragma unroll
        for (int u = 0; u < 2; ++u)
          if (j + u < K) {
            w.cand_xeo[p * KX + (j + u - KIN)] = make_int2(e2[u], __float_as_int(o2[u]));
            w.cand_xem[p * KX + (j + u - KIN)] = emv[(j + u) & 3];
          }
      }
    }

    w.ncand[p] = K;
    if (CTR) {
      c_cells += cells;
      c_ent += ents;
      c_cand += (unsigned long long)K;
    }
  }
  if (CTR) {
    wave_cadd(&w.ctr->cells_visited, c_cells);
    wave_cadd(&w.ctr->cell_entries_scanned, c_ent);
    wave_cadd(&w.ctr->candidates, c_cand);
  }
}

template <bool BIG>
struct Mem;
template <>
struct Mem<false> {  // LDS
  template <class T>
  __device__ static T ld(const T* p) {
    return *p;
  }
  template <class T>
  __device__ static void st(T* p, T v) {
    *p = v;
  }
};
template <>
struct Mem<true> {  // global scratch: keep every access at L2 (agent scope)
  template <class T>
  __device__ static T ld(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  template <class T>
  __device__ static void st(T* p, T v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// Wave tier: one wavefront per spilled probe (list from the lane tier).
// BIG = false: LDS tables (MAX_HITS distinct edges); a probe with more goes
// to the list of the BIG form (CTR_CAND_BIG), whose tables
// (2^cand_log2 slots per block, in HBM) the host sizes: none until needed,
// grown 4x with the batch redone when a probe does not fit (no limit on the
// edges within a radius but memory; round 4 dropped the 256-edge spec limit).
template <bool BIG>
__global__ __launch_bounds__(TB) void k_candidates(DevGraph g, DevBatch b, DevParams P, DevWork w) {
  __shared__ uint32_t l_hkey[BIG ? 1 : HCAP];
  __shared__ unsigned long long l_hval[BIG ? 1 : HCAP];
  __shared__ unsigned long long l_skey[BIG ? 1 : MAX_HITS];
  __shared__ int64_t cstart[64];
  __shared__ int cexcl[64];
  __shared__ int s_count, s_over, s_n;
  const int lane = threadIdx.x;
  const SpillRef work = BIG ? spill_of<CTR_CAND_BIG>(w) : spill_of<CTR_CAND_WAVE>(w);
  const int64_t nwork = *work.count;
  const int32_t* list = work.list;
  if (BIG && nwork > 0 && w.cand_log2 == 0) {
    // no tables yet: the host makes them and redoes the batch -- or, when it
    // cannot (cand_final), these probes' traces answer 500 (OTM_TERR_CAND_OVERFLOW)
    for (int64_t it = (int64_t)blockIdx.x * TB + lane; it < nwork; it += (int64_t)gridDim.x * TB) {
      w.ncand[list[it]] = 0;
      if (w.cand_final) atomicCAS(&w.trace_err[w.pt_trace[list[it]]], 0, OTM_TERR_CAND_OVERFLOW);
    }
    if (!w.cand_final && blockIdx.x == 0 && lane == 0) {
      w.counters_i32[CTR_GROW_CAND] = 1;
      *w.abort = 1;
    }
    return;
  }
  const int hlog2 = BIG ? w.cand_log2 : 9;
  const int hcap = 1 << hlog2;
  const int max_hits = hcap / 2;
  uint32_t* hkey = BIG ? w.cbig_key + (size_t)blockIdx.x * hcap : l_hkey;
  unsigned long long* hval = BIG ? w.cbig_val + (size_t)blockIdx.x * hcap : l_hval;
  unsigned long long* skey = BIG ? w.cbig_skey + (size_t)blockIdx.x * max_hits : l_skey;
  for (int64_t it = blockIdx.x; it < nwork; it += gridDim.x) {
    const int64_t p = list[it];
    const float4 pr = w.probe[p];  // {lat, lon, accuracy} of the column (K1), one line
    const float lat = pr.x, lon = pr.y;
    const float r = probe_radius(P, pr.z);
    const float r2 = r * r;
    const float ls = MPD_F * cos_deg(lat);
    const float dlat = r / MPD_F;
    const float dlon = r / ls;
    const double la_lo = ((double)lat - (double)dlat - g.lat0) / g.cell;
    const double la_hi = ((double)lat + (double)dlat - g.lat0) / g.cell;
    const double lo_lo = ((double)lon - (double)dlon - g.lon0) / g.cell;
    const double lo_hi = ((double)lon + (double)dlon - g.lon0) / g.cell;
    const double R = g.grid_rows, Cn = g.grid_cols;
    int r0 = 0, r1 = -1, c0 = 0, c1 = -1;
    if (!(la_hi < 0.0 || lo_hi < 0.0 || la_lo >= R || lo_lo >= Cn)) {
      r0 = la_lo < 0.0 ? 0 : (int)floor(la_lo);
      r1 = la_hi >= R ? (int)R - 1 : (int)floor(la_hi);
      c0 = lo_lo < 0.0 ? 0 : (int)floor(lo_lo);
      c1 = lo_hi >= Cn ? (int)Cn - 1 : (int)floor(lo_hi);
    }
    const int ncols = c1 - c0 + 1;
    const int ncells = (r1 - r0 + 1) * ncols;
    for (int i = lane; i < hcap; i += TB) {
      Mem<BIG>::st(&hkey[i], (uint32_t)EMPTY);
      Mem<BIG>::st(&hval[i], (unsigned long long)LAB_NONE);
    }
    if (lane == 0) {
      s_count = 0;
      s_over = 0;
      s_n = 0;
    }
    __syncthreads();
    unsigned long long scanned = 0;
    for (int cb = 0; cb < ncells; cb += TB) {
      const int c = cb + lane;
      int cnt = 0;
      int64_t cs = 0;
      if (c < ncells) {
        const int rr = r0 + c / ncols, cc = c0 + c % ncols;
        const size_t cidx = (size_t)rr * (size_t)g.grid_cols + (size_t)cc;
        cs = g.cell_off[cidx];
        cnt = (int)(g.cell_off[cidx + 1] - cs);
      }
      const int incl = wave_incl_scan(cnt, lane);
      const int total = __shfl(incl, 63, 64);
      cexcl[lane] = incl - cnt;
      cstart[lane] = cs;
      __syncthreads();
      const int nc_here = min(TB, ncells - cb);
      for (int gi = lane; gi < total; gi += TB) {
        // cell holding entry gi: largest k with cexcl[k] <= gi
        int lo = 0, hi = nc_here - 1;
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (cexcl[mid] <= gi) lo = mid;
          else hi = mid - 1;
        }
        // the entry's id and its segment's endpoints by the entry's index, one
        // trip: seg_sqdist over ent_geo is proj_calc's sqd bit for bit (the
        // lane tier's snap pass says why), so the scan projects nothing
        const int64_t q = cstart[lo] + (gi - cexcl[lo]);
        const uint32_t ent = g.cell_ent[q];
        const float4 G = g.ent_geo[q];
        const int32_t e = (int32_t)(ent >> 4), k = (int32_t)(ent & 15u);
        const float sqd = seg_sqdist(G.x, G.y, G.z, G.w, lat, lon, ls);
        if (!(sqd <= r2)) continue;
        uint32_t slot = hash32((uint32_t)e) >> (32 - hlog2);
        bool placed = false;
        for (int probe = 0; probe < hcap; ++probe) {
          const uint32_t old = atomicCAS(&hkey[slot], EMPTY, (uint32_t)e);
          if (old == EMPTY) {
            if (atomicAdd(&s_count, 1) >= max_hits) s_over = 1;
            placed = true;
            break;
          }
          if (old == (uint32_t)e) {
            placed = true;
            break;
          }
          slot = (slot + 1) & (uint32_t)(hcap - 1);
        }
        if (!placed) {
          s_over = 1;
          continue;
        }
        atomicMin(&hval[slot], ((unsigned long long)fbits(sqd) << 32) | (unsigned long long)k);
      }
      scanned += (unsigned long long)total;
      __syncthreads();
    }
    if (s_over) {
      if (lane == 0) {
        if (!BIG) {
          spill_push<CTR_CAND_BIG, TIER_CAND_BIG>(w, (int32_t)p);  // to the HBM tables
        } else if (w.cand_final) {
          // the tables are as large as they get: this probe's trace fails
          // alone (500, OTM_TERR_CAND_OVERFLOW), the batch goes on
          w.ncand[p] = 0;
          atomicCAS(&w.trace_err[w.pt_trace[p]], 0, OTM_TERR_CAND_OVERFLOW);
        } else {
          w.ncand[p] = 0;
          w.counters_i32[CTR_GROW_CAND] = 1;  // the tables are too small: grow, redo the batch
          *w.abort = 1;
        }
      }
      __syncthreads();
      continue;
    }
    // compact the distinct edges as sqdist bits << 32 | edge << 5 | shape
    // segment << 1; the edge table is then reused as the node table.  Each
    // edge is projected once, lane-parallel over the compacted list: an edge
    // candidate gets flag bit 1; one whose projection snaps to a node leaves
    // LAB_NONE (sorts last) and meets the other edges at that node in the node
    // table (key: the node's first outgoing edge; value: the smallest sqdist
    // bits << 32 | a slot of the group), which writes the node candidate
    // sqdist bits << 32 | first outgoing edge << 5 into that slot -- so a node
    // sorts before an edge candidate of the same edge at the same distance.
    for (int i = lane; i < hcap; i += TB) {
      const uint32_t hk = Mem<BIG>::ld(&hkey[i]);
      if (hk != EMPTY) {
        const unsigned long long hv = Mem<BIG>::ld(&hval[i]);
        const int idx = atomicAdd(&s_n, 1);
        Mem<BIG>::st(&skey[idx],
                     (hv & 0xFFFFFFFF00000000ull) | ((unsigned long long)hk << 5) | ((hv & 15ull) << 1));
      }
    }
    __syncthreads();
    for (int i = lane; i < hcap; i += TB) {
      Mem<BIG>::st(&hkey[i], (uint32_t)EMPTY);
      Mem<BIG>::st(&hval[i], (unsigned long long)LAB_NONE);
    }
    if (lane == 0) s_count = 0;  // from here: distinct candidates
    __syncthreads();
    const int n0 = s_n;
    for (int idx = lane; idx < n0; idx += TB) {
      const unsigned long long key = Mem<BIG>::ld(&skey[idx]);
      const int32_t e = (int32_t)(((uint32_t)key) >> 5);
      float sqd, off;
      bool at_end;
      const ProjIn pin = proj_load(g, e, (int32_t)((key >> 1) & 15ull));
      proj_calc(pin, lat, lon, ls, sqd, off, at_end);
      const int32_t v = snap_rep(pin, off, at_end);
      if (v < 0) {
        Mem<BIG>::st(&skey[idx], key | 1ull);
        atomicAdd(&s_count, 1);
      } else {
        Mem<BIG>::st(&skey[idx], (unsigned long long)LAB_NONE);
        const uint32_t rep = (uint32_t)v;
        uint32_t slot = hash32(rep) >> (32 - hlog2);
        while (true) {
          const uint32_t old = atomicCAS(&hkey[slot], EMPTY, rep);
          if (old == EMPTY || old == rep) break;
          slot = (slot + 1) & (uint32_t)(hcap - 1);
        }
        atomicMin(&hval[slot], (key & 0xFFFFFFFF00000000ull) | (unsigned long long)idx);
      }
    }
    __syncthreads();
    for (int i = lane; i < hcap; i += TB) {
      const uint32_t hk = Mem<BIG>::ld(&hkey[i]);
      if (hk != EMPTY) {
        const unsigned long long hv = Mem<BIG>::ld(&hval[i]);
        Mem<BIG>::st(&skey[(int)(hv & 0xFFFFFFFFull)], (hv & 0xFFFFFFFF00000000ull) | ((unsigned long long)hk << 5));
        atomicAdd(&s_count, 1);
      }
    }
    __syncthreads();
    const int ns = n0;  // entries in skey (snapped edges past their node's slot: LAB_NONE)
    const int n = s_count;  // distinct candidates
    int N = 1;
    while (N < ns) N <<= 1;
    for (int i = ns + lane; i < N; i += TB) Mem<BIG>::st(&skey[i], (unsigned long long)LAB_NONE);
    __syncthreads();
    // bitonic sort ascending
    for (int kk = 2; kk <= N; kk <<= 1) {
      for (int j = kk >> 1; j > 0; j >>= 1) {
        for (int i = lane; i < N; i += TB) {
          const int ixj = i ^ j;
          if (ixj > i) {
            const unsigned long long x = Mem<BIG>::ld(&skey[i]), y = Mem<BIG>::ld(&skey[ixj]);
            const bool up = (i & kk) == 0;
            if ((x > y) == up) {
              Mem<BIG>::st(&skey[i], y);
              Mem<BIG>::st(&skey[ixj], x);
            }
          }
        }
        __syncthreads();
      }
    }
    const int K = n < P.max_candidates ? n : P.max_candidates;
    if (lane < K) {
      const unsigned long long key = Mem<BIG>::ld(&skey[lane]);
      const int32_t e = (int32_t)(((uint32_t)key) >> 5);
      float sqd = bitsf((uint32_t)(key >> 32)), off = 0.0f;
      if (key & 1ull) project(g, e, (int32_t)((key >> 1) & 15ull), lat, lon, ls, sqd, off);
      const float ds = (2.0f * P.sigma_z) * P.sigma_z;
      cput(w, p, lane, e, off, sqd / ds);
    } else if (lane < KIN) {
      cput(w, p, lane, -1, 0.0f, INFINITY);  // the rest of the inline block (whole lines written back)
    }
    if (lane == 0) {
      w.ncand[p] = K;
      if (w.ctr) {
        cadd(&w.ctr->cells_visited, (unsigned long long)ncells);
        cadd(&w.ctr->cell_entries_scanned, scanned);
        cadd(&w.ctr->candidates, (unsigned long long)K);
      }
    }
    __syncthreads();
  }
}

// ============================================================== K3 links
__global__ __launch_bounds__(256) void k_links(DevBatch b, DevParams P, DevWork w) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > b.n_points) return;
  if (p == b.n_points) {
    w.trans_off[p] = 0;
    // spill snapshot A: candidate probes the lane tier handed to the wave
    // tier; the counters start over for the transition tiers
    fold_snap(w, SNAP_AFTER_CAND, true);
    return;
  }
  int32_t cp = -1, kq = 0;
  int64_t cnt = 0;
  if (w.is_col[p]) {
    const int32_t q = w.prevc[p];
    if (q >= 0 && p - q > 1) w.nextc[q] = (int32_t)p;  // interpolated points between: K7a finds p from them
    if (q >= 0 && w.ncand[p] > 0 && w.ncand[q] > 0 && w.gc[p] <= P.breakage) {
      cp = q;
      kq = w.ncand[q];
      cnt = (int64_t)kq * (int64_t)w.ncand[p];
    }
  }
  w.col_prev[p] = cp;
  w.kq_prev[p] = kq;
  w.trans_off[p] = cnt;
  // K4's record of the column in spatial-order position (k_trans_sub then
  // reads it with one coalesced load instead of an order lookup and five
  // scattered ones)
  if (w.colrec && (P.order_mask & ORDER_TRANS) && w.is_col[p])
    w.colrec[w.colrec_pos[p]] = make_int4((int32_t)p, cp, kq | (w.ncand[p] << 8), __float_as_int(w.gc[p]));
  // Viterbi's byte (k_viterbi_g): ncand <= KMAX = 32 fits six bits
  w.vmeta[p] = (uint8_t)((w.is_col[p] ? (w.ncand[p] | 0x40) : 0) | (cp >= 0 ? 0x80 : 0));
}

// The batch's status for the host's one synchronisation: abort flag,
// transition total, path-pool counters.  A single-wave kernel rather than
// memcpy commands: each runtime copy is its own blit dispatch (3.5-8 us each
// on the stream).
// It goes to the device copy (engine_match resumes from the snapshots beside
// it) and straight into the host's page-locked record, which the device sees:
// the kernel's end makes its stores visible to the host that waits for the
// stream, as a copy command's would be, without the copy's dispatch.
// tier_idle: which on-demand groups' first lists stayed empty (kernels.h
// TierGroup) -- the transition and route stages' CTR_INDEX_MISS from their
// snapshots, the per-batch counts and CTR_SEG_LARGE (counted after the last
// snapshot) from the counters themselves.
__global__ void k_status(const int32_t* abort, const int64_t* ttotal, const int32_t* counters, const int32_t* snap,
                         BatchStatus* out, BatchStatus* host) {
  if (threadIdx.x == 0) {
    BatchStatus st;
    st.abort = *abort;
    st.grow = (counters[CTR_GROW_HUGE] != 0 ? GROW_HUGE : 0) | (counters[CTR_GROW_CAND] != 0 ? GROW_CAND : 0);
    st.ttotal = *ttotal;
    st.pool_used = counters[CTR_POOL_USED];
    st.pool_over = counters[CTR_POOL_OVER];
    st.route_huge = counters[CTR_ROUTE_HUGE];
    st.tier_idle = (counters[CTR_CAND_BIG] == 0 ? TIER_CAND_BIG : 0) |
                   (snap[CTR_STAGE_WORDS * SNAP_AFTER_TRANS + CTR_INDEX_MISS] == 0 ? TIER_TRANS_ONLINE : 0) |
                   (snap[CTR_STAGE_WORDS * SNAP_AFTER_ROUTE + CTR_INDEX_MISS] == 0 ? TIER_ROUTE_ONLINE : 0) |
                   (counters[CTR_VIT_WAVE] == 0 && counters[CTR_VIT_16] == 0 ? TIER_VIT_LISTS : 0) |
                   (counters[CTR_SEG_LARGE] == 0 ? TIER_SEG_LARGE : 0);
    st.tier_wake = counters[CTR_TIER_WAKE];
    st.pad = 0;
    *out = st;
    *host = st;
  }
}

// ============================================================== turn-aware bounded search
// DESIGN.md §3 rule 4 (oracle ta_search): the route of a transition is the
// cheapest by distance plus turn penalty.  A search from node u entered with
// heading hin labels every edge g with its departure label -- the cheapest way
// to be at g's start, turned into it -- and every node v with its arrival
// label, each a 64-bit key cost << 32 | predecessor edge (costs in 1/64 m:
// L(e) = round(len x 64) per edge, turn units per turn), bounded by cost cmax.
// Label-correcting in one wavefront with 64-bit atomicMin: every label
// converges to the minimum over its in-steps, the unique fixed point (every
// step costs > 0), which the oracle's Dijkstra computes -- whatever the
// relaxation order.  A key enters the table once (the set of keys ever
// inserted is exactly those whose label is within cmax), so the count is
// order-free too.
struct Table {
  uint32_t* key;            // edge id, NODE_KEY | node, or EMPTY
  unsigned long long* lab;  // cost << 32 | predecessor edge
  uint32_t* inq;            // in next frontier
  uint32_t* fr0;            // frontier A (slot ids)
  uint32_t* fr1;            // frontier B
  int cap_log2;
  int limit;                // max labels before overflow
  // global tier only: the slots the last search inserted (its first `limit`)
  // and how many (*prev, -1: unknown), so the next search clears those instead
  // of the whole 128K-slot table (the tables start clean: engine.cpp ensure_big)
  uint32_t* ins = nullptr;
  int32_t* prev = nullptr;
};

struct SearchShared {
  int nfr, nnext, count, over;
};

template <bool BIG>
__device__ __forceinline__ int table_find(const Table& T, uint32_t v) {
  const uint32_t mask = (1u << T.cap_log2) - 1u;
  uint32_t slot = hash32(v) >> (32 - T.cap_log2);
  for (int i = 0; i <= (int)mask; ++i) {
    const uint32_t k = Mem<BIG>::ld(&T.key[slot]);
    if (k == v) return (int)slot;
    if (k == EMPTY) return -1;
    slot = (slot + 1) & mask;
  }
  return -1;
}

// lower key's label to nl (inserting the key); an edge key whose cost fell
// joins the next frontier
template <bool BIG>
__device__ __forceinline__ void ta_relax(const Table& T, SearchShared& S, uint32_t* nxt, uint32_t key,
                                         unsigned long long nl) {
  const uint32_t mask = (1u << T.cap_log2) - 1u;
  uint32_t slot = hash32(key) >> (32 - T.cap_log2);
  int found = -1;
  for (int i = 0; i <= (int)mask; ++i) {
    const uint32_t old = atomicCAS(&T.key[slot], EMPTY, key);
    if (old == EMPTY) {
      const int c = atomicAdd(&S.count, 1);
      if (c >= T.limit) S.over = 1;
      else if (BIG) Mem<true>::st(&T.ins[c], slot);
      found = (int)slot;
      break;
    }
    if (old == key) {
      found = (int)slot;
      break;
    }
    slot = (slot + 1) & mask;
  }
  if (found < 0) {
    S.over = 1;
    return;
  }
  const unsigned long long old = atomicMin(&T.lab[found], nl);
  // successors depend on the cost alone (their predecessor is this edge)
  if (!(key & NODE_KEY) && nl < old && (uint32_t)(old >> 32) != (uint32_t)(nl >> 32)) {
    if (atomicExch(&T.inq[found], 1u) == 0u) {
      const int idx = atomicAdd(&S.nnext, 1);
      Mem<BIG>::st(&nxt[idx], (uint32_t)found);
    }
  }
}

// returns >= 0 labels, or -1 on overflow (more than T.limit)
template <bool BIG>
__device__ int ta_search(const DevGraph& g, const uint32_t* TU, const Table& T, SearchShared& S, int32_t u,
                         uint32_t hin, uint32_t cmax, int lane) {
  const int cap = 1 << T.cap_log2;
  // a clean table: the LDS tier's whole, the global tier's the slots its last
  // search inserted (all of them after an overflow)
  const int pc = BIG ? Mem<true>::ld(T.prev) : -1;
  if (pc < 0) {
    for (int i = lane; i < cap; i += TB) {
      Mem<BIG>::st(&T.key[i], EMPTY);
      Mem<BIG>::st(&T.lab[i], LAB_NONE);
      Mem<BIG>::st(&T.inq[i], 0u);
    }
  } else {
    for (int i = lane; i < pc; i += TB) {
      const uint32_t sl = Mem<true>::ld(&T.ins[i]);
      Mem<BIG>::st(&T.key[sl], EMPTY);
      Mem<BIG>::st(&T.lab[sl], LAB_NONE);
      Mem<BIG>::st(&T.inq[sl], 0u);
    }
  }
  if (lane == 0) {
    S.nfr = 0;
    S.nnext = 0;
    S.count = 0;
    S.over = 0;
  }
  __syncthreads();
  uint32_t* cur = T.fr0;
  uint32_t* nxt = T.fr1;
  // the source node (arrival 0) and the route's possible first edges
  if (lane == 0) ta_relax<BIG>(T, S, nxt, NODE_KEY | (uint32_t)u, (unsigned long long)NONE_PRED);
  const int32_t e0 = g.out_off[u], e1 = g.out_off[u + 1];
  for (int32_t e = e0 + lane; e < e1; e += TB) {
    const uint32_t c = turn_units(TU, hin, g.e_head_out[e]);
    if (c <= cmax) ta_relax<BIG>(T, S, nxt, (uint32_t)e, ((unsigned long long)c << 32) | NONE_PRED);
  }
  __syncthreads();
  while (true) {
    if (lane == 0) {
      S.nfr = S.nnext;
      S.nnext = 0;
    }
    uint32_t* tmp = cur;
    cur = nxt;
    nxt = tmp;
    __syncthreads();
    const int nfr = S.nfr;
    if (nfr == 0 || S.over) break;
    for (int f = lane; f < nfr; f += TB) {
      const uint32_t sl = Mem<BIG>::ld(&cur[f]);
      if (BIG) atomicExch(&T.inq[sl], 0u);
      else T.inq[sl] = 0u;
      const int32_t e = (int32_t)Mem<BIG>::ld(&T.key[sl]);
      const unsigned long long ca =
          (unsigned long long)(uint32_t)(Mem<BIG>::ld(&T.lab[sl]) >> 32) + (unsigned long long)g.e_len64[e];
      if (ca > cmax) continue;
      const int32_t v = g.e_to[e];
      ta_relax<BIG>(T, S, nxt, NODE_KEY | (uint32_t)v, (ca << 32) | (uint32_t)e);
      const uint32_t hv = g.e_head_in[e];
      for (int32_t h = g.out_off[v]; h < g.out_off[v + 1]; ++h) {
        const unsigned long long c = ca + turn_units(TU, hv, g.e_head_out[h]);
        if (c <= cmax) ta_relax<BIG>(T, S, nxt, (uint32_t)h, (c << 32) | (uint32_t)e);
      }
    }
    __syncthreads();
  }
  const bool over = S.over != 0;
  const int count = S.count;
  if (BIG && lane == 0) Mem<true>::st(T.prev, over || count > T.limit ? -1 : count);
  __syncthreads();
  return over ? -1 : count;
}

// work counts of a converged search (oracle ta_search's counters): the
// departure labels, and the edges they relax (their end node's out-edges,
// when the arrival is within the bound)
template <bool BIG>
__device__ void ta_counts(const DevGraph& g, const Table& T, uint32_t cmax, int lane, unsigned long long& settled,
                          unsigned long long& relaxed) {
  unsigned long long st = 0, rl = 0;
  const int cap = 1 << T.cap_log2;
  for (int i = lane; i < cap; i += TB) {
    const uint32_t k = Mem<BIG>::ld(&T.key[i]);
    if (k == EMPTY || (k & NODE_KEY)) continue;
    ++st;
    const unsigned long long ca = (Mem<BIG>::ld(&T.lab[i]) >> 32) + (unsigned long long)g.e_len64[k];
    if (ca <= cmax) rl += (unsigned long long)(g.out_off[g.e_to[k] + 1] - g.out_off[g.e_to[k]]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    st += __shfl_xor(st, o, 64);
    rl += __shfl_xor(rl, o, 64);
  }
  settled = st;
  relaxed = rl;
}

// The route a converged label ends: its predecessor chain (fully traversed
// edges), walked back from `pred0` into the lane's LDS buffer buf (stride TB,
// CHAIN_BUF entries; a longer chain is re-walked per edge), then summed in
// route order: the distance d and the turn units from heading hin through the
// chain, plus the turn into hout (NO_HEAD: none).  predof(e) = e's departure
// label's predecessor.
constexpr int CHAIN_BUF = 32;
template <class F>
__device__ void chain_sums(const DevGraph& g, const uint32_t* TU, F predof, uint32_t pred0, uint32_t hin,
                           uint32_t hout, int32_t* buf, float& d, uint32_t& units, int& n) {
  int cnt = 0;
  for (uint32_t p = pred0; p != NONE_PRED && cnt < (1 << 26); p = predof(p)) {
    if (cnt < CHAIN_BUF) buf[cnt * TB] = (int32_t)p;
    ++cnt;
  }
  float dd = 0.0f;
  unsigned long long un = 0;
  uint32_t h = hin;
  for (int m = cnt - 1; m >= 0; --m) {
    int32_t e;
    if (cnt <= CHAIN_BUF) {
      e = buf[m * TB];
    } else {
      uint32_t x = pred0;
      for (int k = 0; k < m; ++k) x = predof(x);
      e = (int32_t)x;
    }
    un += turn_units(TU, h, g.e_head_out[e]);
    dd = dd + g.e_len[e];
    h = g.e_head_in[e];
  }
  un += turn_units(TU, h, hout);
  d = dd;
  units = un > TURN_UNITS_MAX ? TURN_UNITS_MAX : (uint32_t)un;
  n = cnt;
}

// ============================================================== route index
__device__ __forceinline__ uint32_t idx_hash(uint32_t v) {
  v ^= v >> 16;
  v *= 0x85ebca6bu;
  v ^= v >> 13;
  v *= 0xc2b2ae35u;
  v ^= v >> 16;
  return v;
}

// A row's table: entries x 100 / pct slots rounded up to an even count (at
// least one slot empty, so every probe ends), the hash mapped onto its 2-slot
// buckets by a multiply-high.  A label's probe starts at its bucket's first
// slot and goes on linearly; a lookup loads the bucket's two slots (32 aligned
// bytes, one line) at once, which holds the label or ends the probe for most
// lookups.  A slot is 16 bytes with the predecessor inside (idx_slot_*).  The
// engine picks pct per index (engine.cpp build_index_at): IDX_LOAD_FAST (30 %,
// 53 B per entry) when the tables fit the HBM budget, IDX_LOAD_DENSE (40 %,
// 40 B per entry) when only that fits -- measured on configs 2 / 4 / 3,
// k_trans_sub at 40 % is 9 / 6 / 7 % slower than at 30 % (more lookups past
// their bucket), round 4's 20-B slots at 20 % (100 B per entry) 1 / 2 / 1 %
// faster.
constexpr int IDX_LOAD_FAST = 30, IDX_LOAD_DENSE = 40;
__host__ __device__ __forceinline__ int64_t idx_row_cap(int32_t c, int pct) {
  if (c <= 0) return 0;
  int64_t cap = ((int64_t)c * 100 + pct - 1) / pct;
  if (cap <= c) cap = (int64_t)c + 1;
  return (cap + 1) & ~(int64_t)1;
}
// first slot of a label's probe in row R (its bucket's first slot)
__device__ __forceinline__ uint32_t idx_slot0(uint32_t hh, const IdxRow& R) {
  return (uint32_t)(((uint64_t)hh * (uint64_t)(R.cap >> 1)) >> 32) << 1;
}
__device__ __forceinline__ uint32_t idx_next(uint32_t h, const IdxRow& R) {
  return h + 1u == R.cap ? 0u : h + 1u;
}
// A slot {key, cost | pred lo << 24, route distance bits, units | pred hi << 24}:
// cost and turn units below 2^24 (units <= cost <= the index's cmax, and the
// index radius is capped so that cmax < 2^24), the 16-bit predecessor slot in
// the row split over the two top bytes (IDX_NO_PRED: the route's first edge).
constexpr uint32_t IDX_LOW24 = 0xFFFFFFu;
constexpr uint32_t IDX_NO_PRED = 0xFFFFu;
static_assert((int64_t)INDEX_BUILD_LIMIT * 100 / IDX_LOAD_FAST + 2 < (int64_t)IDX_NO_PRED,
              "a row's slots must be numbered in 16 bits");
__host__ __device__ __forceinline__ uint32_t idx_slot_cost(const uint4& s) { return s.y & IDX_LOW24; }
__host__ __device__ __forceinline__ uint32_t idx_slot_units(const uint4& s) { return s.w & IDX_LOW24; }
__host__ __device__ __forceinline__ int32_t idx_slot_pred(const uint4& s) {
  const uint32_t p = (s.y >> 24) | ((s.w >> 24) << 8);
  return p == IDX_NO_PRED ? -1 : (int32_t)p;
}

// Row lookup: linear probing in the row's table from the key's bucket, a
// bucket (two slots) per load.  Returns the slot (its contents in *out) when
// the key is in the row, -1 when absent (its label beyond cmax), -2 when the
// row is incomplete.
__device__ __forceinline__ int64_t idx_find(const uint4* slot, const IdxRow& R, uint32_t v, uint4& out) {
  if (R.cnt < 0) return -2;
  if (R.cnt == 0) return -1;
  uint32_t h = idx_slot0(idx_hash(v), R);
  while (true) {
    const uint4 a = slot[R.off + h], b = slot[R.off + h + 1];
    if (a.x == v) {
      out = a;
      return R.off + h;
    }
    if (a.x == EMPTY) return -1;
    if (b.x == v) {
      out = b;
      return R.off + h + 1;
    }
    if (b.x == EMPTY) return -1;
    h = h + 2u == R.cap ? 0u : h + 2u;
  }
}
// the index row of a candidate as the source of a route: its edge's row
// (entered along the edge), or its node's (a node candidate, no heading)
__device__ __forceinline__ int64_t src_row(const DevGraph& g, int32_t e, float off) {
  return cand_node(off) ? (int64_t)g.n_edges + g.e_from[e] : (int64_t)e;
}
// the label a route to a candidate ends on: its edge's departure label, or its
// node's arrival label (a node candidate)
__device__ __forceinline__ uint32_t dst_key(const DevGraph& g, int32_t e, float off) {
  return cand_node(off) ? NODE_KEY | (uint32_t)g.e_from[e] : (uint32_t)e;
}

// Index build: one wavefront per row runs the row's search with bound cmax in
// an LDS table of INDEX_BUILD_CAP slots (the online tiers' fixed point), then
// inserts every label into the row's table with its cost, route distance and
// turn units (each lane walks its label's predecessor chain in the LDS table),
// and then, the row's slots all placed, its predecessor's slot in the row
// (the route's first edge: none), so a path is walked slot to slot.
template <bool WRITE>
__global__ __launch_bounds__(TB) void k_index_build(DevGraph g, const uint32_t* TU, uint32_t cmax, int32_t* row_cnt,
                                                    const IdxRow* rows, uint4* slot) {
  __shared__ uint32_t lkey[INDEX_BUILD_CAP];
  __shared__ unsigned long long llab[INDEX_BUILD_CAP];
  __shared__ uint32_t linq[INDEX_BUILD_CAP];
  __shared__ uint32_t lfr0[INDEX_BUILD_CAP];
  __shared__ uint32_t lfr1[INDEX_BUILD_CAP];
  __shared__ int32_t cbuf[CHAIN_BUF * TB];
  __shared__ SearchShared S;
  const int lane = threadIdx.x;
  const Table T{lkey, llab, linq, lfr0, lfr1, INDEX_BUILD_LOG2, INDEX_BUILD_LIMIT};
  const int64_t nrows = (int64_t)g.n_edges + g.n_nodes;
  for (int64_t r = blockIdx.x; r < nrows; r += gridDim.x) {
    const bool erow = r < g.n_edges;
    const int32_t u = erow ? g.e_to[r] : (int32_t)(r - g.n_edges);
    const uint32_t hin = erow ? (uint32_t)g.e_head_in[r] : NO_HEAD;
    const int n = ta_search<false>(g, TU, T, S, u, hin, cmax, lane);
    if (!WRITE) {
      if (lane == 0) row_cnt[r] = n;  // -1: incomplete row
      continue;
    }
    if (n < 0) continue;
    // insert the labels into the row's table (slot order depends on CAS
    // order; lookups do not)
    const IdxRow R = rows[r];
    auto predof = [&](uint32_t e) {
      const int sx = table_find<false>(T, e);
      return sx < 0 ? NONE_PRED : (uint32_t)(llab[sx] & 0xFFFFFFFFull);
    };
    for (int i = lane; i < INDEX_BUILD_CAP; i += TB) {
      const uint32_t k = lkey[i];
      if (k == EMPTY) continue;
      const unsigned long long lab = llab[i];
      const uint32_t pk = (uint32_t)(lab & 0xFFFFFFFFull);
      float d;
      uint32_t units;
      int len;
      chain_sums(g, TU, predof, pk, hin, (k & NODE_KEY) ? NO_HEAD : (uint32_t)g.e_head_out[k], cbuf + lane, d, units,
                 len);
      uint32_t h = idx_slot0(idx_hash(k), R);
      while (atomicCAS(&slot[R.off + h].x, EMPTY, k) != EMPTY) h = idx_next(h, R);
      // (cost <= cmax < 2^24 and units <= cost: the top bytes are the
      // predecessor's, written below)
      slot[R.off + h].y = (uint32_t)(lab >> 32) & IDX_LOW24;
      slot[R.off + h].z = fbits(d);
      slot[R.off + h].w = units & IDX_LOW24;
    }
    __syncthreads();
    for (int i = lane; i < INDEX_BUILD_CAP; i += TB) {
      const uint32_t k = lkey[i];
      if (k == EMPTY) continue;
      const uint32_t pk = (uint32_t)(llab[i] & 0xFFFFFFFFull);
      uint4 sk_v, tmp;
      const int64_t sk = idx_find(slot, R, k, sk_v);
      const int64_t sp = pk == NONE_PRED ? -1 : idx_find(slot, R, pk, tmp);
      const uint32_t ps = sp < 0 ? IDX_NO_PRED : (uint32_t)(sp - R.off);
      slot[sk].y = (sk_v.y & IDX_LOW24) | (ps & 0xFFu) << 24;
      slot[sk].w = (sk_v.w & IDX_LOW24) | (ps >> 8) << 24;
    }
    __syncthreads();
  }
}

// table capacity of a row (idx_row_cap at load pct)
__global__ void k_row_sizes(const int32_t* row_cnt, int64_t* sizes, int32_t n, int pct) {
  const int32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n) sizes[u] = idx_row_cap(row_cnt[u], pct);
  if (u == n) sizes[n] = 0;
}

__global__ void k_row_pack(const int32_t* row_cnt, const int64_t* row_off, IdxRow* rows, int32_t n) {
  const int32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n) return;
  const int64_t cap = row_off[u + 1] - row_off[u];
  rows[u] = IdxRow{row_off[u], row_cnt[u], (uint32_t)cap};
}

// the per-edge source records of an index (kernels.h SrcRec), from its rows
__global__ void k_src_pack(DevGraph g, const IdxRow* rows, SrcRec* src) {
  const int32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= g.n_edges) return;
  const int2 fl = g.e_fl[e];
  SrcRec r{};
  r.edge = rows[e];
  r.node = rows[(int64_t)g.n_edges + fl.x];
  r.from = fl.x;
  r.len = fl.y;
  src[e] = r;
}
// a source's row out of its edge's record: one 16-byte load whose address
// comes from the candidate record alone
__device__ __forceinline__ IdxRow src_row(const SrcRec* src, int32_t e, bool node) {
  const uint4 v = ((const uint4*)(src + e))[node ? 1 : 0];
  IdxRow R;
  R.off = (int64_t)((unsigned long long)v.x | (unsigned long long)v.y << 32);
  R.cnt = (int32_t)v.z;
  R.cap = v.w;
  return R;
}

// a 64-bit word out of the two 32-bit halves an LDS record carries it in
__device__ __forceinline__ unsigned long long word64(int lo, int hi) {
  return (unsigned long long)(uint32_t)lo | (unsigned long long)(uint32_t)hi << 32;
}

// K4 index tier: S lanes per column, TB / S columns in flight per wave,
// lanes over the column's Kq x Kp (source candidate, target candidate) pairs;
// each pair is one probe of its source's index row (row ei, or E + from(ei)
// for a node candidate) for its target's label (key ej, or NODE_KEY |
// from(ej) for a node candidate), whose 16-byte slot holds the label's cost,
// route distance and turn units.  A column is a chain of ~5 dependent round
// trips (point -> previous column -> candidates -> rows -> slots), so several
// columns per wave multiply the misses in flight at the same occupancy.
// The front of the chain (column record, candidates, rows) runs per group; the
// pairs of the wave's columns are then taken by all 64 lanes (the flat pair
// loop below).  Columns the index
// cannot answer (cost bound > the index's, a source row incomplete, more than
// KC candidates) go to the search tiers (CTR_INDEX_MISS).
// At 8 lanes per column (8 columns per wave) a column with more than
// OTM_TRANS_KC8 candidates on either side goes to the wide list
// (CTR_TRANS_WIDE), which a 16-lane pass (LIST)
// then answers from the index; KC8 keeps the LDS words within 8 waves per SIMD.
#ifndef OTM_TRANS_KC8
#define OTM_TRANS_KC8 8
#endif
// The pair loop is flat: the pairs of the wave's NS columns are laid end to
// end and lane L takes flat pairs L, L + 64, ...: ceil(sum / 64) probe steps
// per wave, where each group looping over its own column (the earlier form)
// took as many as the wave's largest column, ceil(max / S), with the smaller
// columns' lanes idle.  The front phase stays per group; each pair's
// arithmetic, probes and stored float are those of the earlier form
// (DESIGN.md §5 K4).
// waves per SIMD the register budget is sized for
#ifndef OTM_TRANS_WAVES
#define OTM_TRANS_WAVES 8
#endif
template <int S, bool LIST>
__global__ __launch_bounds__(TB, OTM_TRANS_WAVES) void k_trans_sub(DevGraph g, DevBatch b, DevParams P, DevWork w) {
  if (*w.abort || trans_over_cap(b, w)) return;  // a capacity was exceeded: the host redoes the batch
  static_assert(S == 8 || S == 16, "8 lanes per column (two passes) or 16 (one pass / the wide pass)");
  constexpr int NS = TB / S;
  // a pair reads its target and source as one 16-byte LDS word each
  constexpr int KC = S >= 16 ? 16 : OTM_TRANS_KC8;
  constexpr bool WIDE = KC < 16;
  __shared__ int4 tg[NS][KC];  // target: edge, offset bits, label key, -
  __shared__ int4 sr[NS][KC];  // source: edge, offset bits, remaining-length bits, end heading
  __shared__ IdxRow rq[NS][KC];
  // a column group's record for the flat pair loop, left by its first lane:
  // {trans offset lo, hi, Kp | Kq << 8 | active << 16, gcv}, {bound, cq, the
  // probed index level's slots lo, hi}
  __shared__ int4 cr[NS][2];
  // slot of candidate k in its column group's row: XOR-swizzled so that the
  // groups a ds_read_b128 lane group spans (MI355X_MICROARCH.md §LDS: lanes
  // {0-3,12-15,20-27}, ...) read different banks when they read the same k
  // (a 128-B row at 8 lanes per column puts groups sg and sg + 2 on the same
  // 64 banks; at 16 lanes, every row spans all 64).  Kept under the flat pair
  // loop, where a column's reads come from consecutive lanes instead: config 2
  // 181.2 us with it, 183.6 without (profiles/trans_flat/knobs.json)
  const int lane = threadIdx.x, sg = lane / S, sl = lane % S;
  const unsigned long long smask = ((1ull << S) - 1ull) << (sg * S);
  const int swz = S == 8 ? ((sg >> 1) & 1) * 4 : (sg & 1) * 8;
  const DevIndex& X = w.idx;
  unsigned long long c_search = 0, c_settled = 0, c_relaxed = 0, c_trans = 0;
  const bool ordered = !LIST && (P.order_mask & ORDER_TRANS) != 0;
  // algorithmic counts of the equivalent searches of the lane's own column
  // group (per-lane partials, summed over the wave at the end): per distinct
  // source (node, heading), the row's departure labels within the bound and
  // the out-degrees of those whose edge end is within it too
  auto count_searches = [&](int Kq, uint32_t cq, const uint4* xslot) {
    for (int i = 0; i < Kq; ++i) {
      const int4 Si = sr[sg][i ^ swz];
      const int32_t ui = src_node(g, Si.x, __int_as_float(Si.y));
      bool first = true;
      for (int k = 0; k < i; ++k) {
        const int4 Sk = sr[sg][k ^ swz];
        first = first && !(src_node(g, Sk.x, __int_as_float(Sk.y)) == ui && Sk.w == Si.w);
      }
      if (!first) continue;
      const IdxRow R = rq[sg][i ^ swz];
      for (int64_t k = sl; k < (int64_t)R.cap; k += S) {
        const uint4 slt = xslot[R.off + k];
        if (slt.x == EMPTY || (slt.x & NODE_KEY) || idx_slot_cost(slt) > cq) continue;
        ++c_settled;
        if ((unsigned long long)idx_slot_cost(slt) + g.e_len64[slt.x] <= cq) {
          const int32_t v = g.e_to[slt.x];
          c_relaxed += (unsigned long long)(g.out_off[v + 1] - g.out_off[v]);
        }
      }
      if (sl == 0) ++c_search;
    }
  };
  int64_t base, end, stride;
  if (LIST) {
    base = (int64_t)blockIdx.x * NS;
    end = w.counters_i32[CTR_TRANS_WIDE];
    stride = (int64_t)gridDim.x * NS;
  } else if (ordered) {
    const int grp = blockIdx.x % ORDER_GROUPS;
    base = w.ord.grp[grp] + (int64_t)(blockIdx.x / ORDER_GROUPS) * NS;
    end = w.ord.grp[grp + 1];
    stride = (int64_t)(gridDim.x / ORDER_GROUPS) * NS;
  } else {
    base = (int64_t)blockIdx.x * NS;
    end = b.n_points;
    stride = (int64_t)gridDim.x * NS;
  }
  for (; base < end; base += stride) {
    const int64_t it = base + sg;
    bool act = it < end;
    int64_t p = 0;
    // the column's words in one round trip (K3 wrote the previous column's
    // candidate count beside the link): its ordered record, or the arrays
    int32_t q = -1;
    int Kp = 0, Kq = 0;
    float gcv = 0.0f;
    int64_t toff = 0;
    if (act && ordered && w.colrec) {
      const int4 A = w.colrec[it];
      p = A.x;
      toff = w.trans_off[p];  // (the scan's, after K3)
      q = A.y;
      Kq = A.z & 255;
      Kp = A.z >> 8;
      gcv = __int_as_float(A.w);
    } else if (act) {
      p = LIST ? (int64_t)spill_list<CTR_TRANS_WIDE>(w)[it] : (ordered ? (int64_t)w.ord.item[it] : it);
      q = w.col_prev[p];
      Kq = w.kq_prev[p];
      Kp = w.ncand[p];
      gcv = w.gc[p];
      toff = w.trans_off[p];
    }
    act = act && q >= 0;
    const float bound = P.factor * gcv;
    const uint32_t cq = index_cost_bound(bound);
    const bool idx_ok = X.rmax > 0.0f && cq <= X.cmax;
    // the near index when it covers the bound (same answers, smaller tables)
    const SrcRec* xsrc = X.src;
    const uint4* xslot = X.slot;
#pragma unroll
    for (int l = NEAR_LEVELS - 1; l >= 0; --l) {
      if (w.idxn[l].rmax > 0.0f && cq <= w.idxn[l].cmax) {
        xsrc = w.idxn[l].src;
        xslot = w.idxn[l].slot;
      }
    }
    const bool wide = WIDE && act && idx_ok && (Kp > KC || Kq > KC);
    if (wide && sl == 0) spill_push<CTR_TRANS_WIDE>(w, (int32_t)p);
    act = act && !wide;
    bool bad = act && (!idx_ok || Kp > KC || Kq > KC);
    // candidates of p (targets) and of q (sources), then rows
    for (int k = sl; k < KC; k += S) {
      if (act && k < Kp) {
        const int2 c = crec(w, p, k);
        const int32_t e = c.x;
        const float o = __int_as_float(c.y);
        const uint32_t key = dst_key(g, e, o);
        tg[sg][k ^ swz] = make_int4(e, __float_as_int(o), (int)key, (int)idx_hash(key));
      }
      if (act && k < Kq) {
        const int2 c = crec(w, q, k);
        const int32_t e = c.x;
        const float o = __int_as_float(c.y);
        // src_start and src_row from the edge's {from, length} pair (one
        // load); the heading only for the work counters (no load otherwise);
        // with an index, both out of the edge's source record: the row that
        // cand_node(o) selects and the length, addressed by the candidate
        // record alone, leave together (the row's number needed from(e) first)
        IdxRow R{};
        int32_t lenb;
        if (idx_ok) {
          R = src_row(xsrc, e, cand_node(o));
          lenb = xsrc[e].len;
        } else {
          lenb = g.e_fl[e].y;
        }
        const float start = cand_node(o) ? 0.0f : __int_as_float(lenb) - o;
        sr[sg][k ^ swz] = make_int4(e, __float_as_int(o), __float_as_int(start), w.ctr ? (int)src_head(g, e, o) : 0);
        if (idx_ok) {
          rq[sg][k ^ swz] = R;
          bad = bad || R.cnt < 0;
        }
      }
    }
    const bool spill = (__ballot(bad) & smask) != 0ull;
    if (spill && act && sl == 0) spill_push<CTR_INDEX_MISS, TIER_TRANS_ONLINE>(w, (int32_t)p);
    act = act && !spill;
    // an inactive group (out of range, unlinked, wide-listed, spilled) has no pairs
    const int npair_g = act ? Kq * Kp : 0;
    if (sl == 0) {
      const unsigned long long xs = (unsigned long long)xslot;
      cr[sg][0] = make_int4((int)(uint32_t)toff, (int)(uint32_t)((unsigned long long)toff >> 32),
                            act ? (Kp | Kq << 8 | 1 << 16) : 0, __float_as_int(gcv));
      cr[sg][1] = make_int4(__float_as_int(bound), (int)cq, (int)(uint32_t)xs, (int)(uint32_t)(xs >> 32));
    }
    wave_sync();
    {
      // the groups' pair counts (wave-uniform, from each group's first lane)
      // and their exclusive prefix: flat pair f of the wave is pair f - pre[c]
      // of the last column c with pre[c] <= f
      int pre[NS], total = 0;
#pragma unroll
      for (int c = 0; c < NS; ++c) {
        pre[c] = total;
        total += __builtin_amdgcn_readlane(npair_g, c * S);
      }
      unsigned long long ntr = 0;
      for (int f = lane; f < total; f += TB) {
        int c = 0, pc = 0;
#pragma unroll
        for (int k = 1; k < NS; ++k) {
          if (f >= pre[k]) {
            c = k;
            pc = pre[k];
          }
        }
        const int idx = f - pc;
        const int cz = S == 8 ? ((c >> 1) & 1) * 4 : (c & 1) * 8;
        const int4 C0 = cr[c][0], C1 = cr[c][1];
        const int kp = C0.z & 255;
        const float gcv_c = __int_as_float(C0.w), bound_c = __int_as_float(C1.x);
        const uint32_t cq_c = (uint32_t)C1.y;
        const uint4* xslot_c = (const uint4*)word64(C1.z, C1.w);
        const int64_t toff_c = (int64_t)word64(C0.x, C0.y);
        const int i = idx / kp, j = idx - (idx / kp) * kp;
        const int4 T = tg[c][j ^ cz], Sx = sr[c][i ^ cz];
        const uint32_t key = (uint32_t)T.z;
        const int32_t ej = T.x, ei = Sx.x;
        const float oj = __int_as_float(T.y), oi = __int_as_float(Sx.y), si = __int_as_float(Sx.z);
        float r = 0.0f;
        bool ok = true;
        uint32_t units = 0;
        if (same_edge_step(ei, oi, ej, oj)) {
          r = same_edge_dist(oi, oj);
        } else {
          const IdxRow R = rq[c][i ^ cz];
          uint4 sv = make_uint4(EMPTY, 0u, 0u, 0u);
          if (R.cnt > 0) {
            // the pair's bucket: two slots, one aligned 32-B piece of a line
            uint32_t h = idx_slot0((uint32_t)T.w, R);
            sv = xslot_c[R.off + h];
            uint4 s1 = xslot_c[R.off + h + 1];
            if (sv.x != key && sv.x != EMPTY) {
              sv = s1;
              h = h + 1u;
              while (sv.x != key && sv.x != EMPTY) {  // the rest of the linear probe (rare)
                h = idx_next(h, R);
                sv = xslot_c[R.off + h];
              }
            }
          }
          // a label of the row beyond this column's cost bound is not one
          // of its search's labels
          if (R.cnt > 0 && sv.x == key && idx_slot_cost(sv) <= cq_c) {
            const float sd = si + bitsf(sv.z);
            r = sd + oj;
            units = idx_slot_units(sv);
          } else {
            ok = false;
          }
        }
        float cost = INFINITY;
        if (ok && r <= bound_c) {
          cost = trans_cost(units, r, gcv_c, P.beta);
          ++ntr;
        }
        w.trans[toff_c + idx] = cost;
      }
      if (w.ctr) {
        // the work counters keep their per-group form, from the group's record
        const int4 C0 = cr[sg][0], C1 = cr[sg][1];
        if (C0.z >> 16)
          count_searches((C0.z >> 8) & 255, (uint32_t)C1.y, (const uint4*)word64(C1.z, C1.w));
        c_trans += ntr;
      }
    }
    wave_sync();
  }
  if (w.ctr) {
    for (int sh = 32; sh > 0; sh >>= 1) {
      c_search += __shfl_xor(c_search, sh, 64);
      c_settled += __shfl_xor(c_settled, sh, 64);
      c_relaxed += __shfl_xor(c_relaxed, sh, 64);
      c_trans += __shfl_xor(c_trans, sh, 64);
    }
    if (lane == 0) {
      cadd(&w.ctr->searches, c_search);
      cadd(&w.ctr->nodes_settled, c_settled);
      cadd(&w.ctr->edges_relaxed, c_relaxed);
      cadd(&w.ctr->transitions, c_trans);
    }
  }
}

// K6 index tier: one lane per matched step; the route is the predecessor
// chain of its target's label in its source's row, one probe per edge.
// route / report waves-per-SIMD hints: 4 or 8 measured within noise (kept at 1)
#ifndef OTM_ROUTE_WAVES
#define OTM_ROUTE_WAVES 1
#endif
__global__ __launch_bounds__(256, OTM_ROUTE_WAVES) void k_route_index(DevGraph g, DevBatch b, DevParams P, DevWork w) {
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  const DevIndex& X = w.idx;
  unsigned long long c_search = 0, c_settled = 0, c_relaxed = 0, c_edges = 0;
  const ItemRange R = item_range(w, b, (P.order_mask & ORDER_ROUTE) != 0, 256);
  // K4's column records (K3, spatial-order position) give p, its link and gc
  // in one coalesced load, so the link's chosen candidate loads with p's
  const bool rec = R.ordered && w.colrec && (P.order_mask & ORDER_TRANS);
  for (int64_t it = R.i0; it < R.i1; it += R.stride) {
    int64_t p;
    int32_t q = -1;
    float gcv = 0.0f;
    if (rec) {
      const int4 A = w.colrec[it];
      p = A.x;
      q = A.y;
      gcv = __int_as_float(A.w);
    } else {
      p = R.ordered ? (int64_t)w.ord.item[it] : it;
    }
    if (!R.ordered && !w.is_col[p]) continue;
    // (non-column points keep the zeros K1 wrote; a re-run after a path-pool
    // overflow rewrites every column)
    w.route_dist[p] = 0.0f;
    w.path_len[p] = 0;
    w.path_off[p] = 0;
    const int2 cq0 = w.chosen[q >= 0 ? q : p];  // (used only for a matched link)
    if (w.state[p] < 0 || w.chain_start[p]) continue;
    if (!rec) {
      q = w.col_prev[p];
      gcv = w.gc[p];
    }
    const int2 ci = rec ? cq0 : w.chosen[q], cj = w.chosen[p];
    const int32_t ei = ci.x, ej = cj.x;
    const float oi = __int_as_float(ci.y), oj = __int_as_float(cj.y);
    if (same_edge_step(ei, oi, ej, oj)) {
      w.route_dist[p] = same_edge_dist(oi, oj);
      continue;
    }
    const float bound = P.factor * gcv;
    const uint32_t cq = index_cost_bound(bound);
    IdxRow Rw{};
    int64_t sv = -1;
    uint4 lab{};
    // the near index when it covers the bound (the same labels and paths)
    int lvl = -1;
#pragma unroll
    for (int l = NEAR_LEVELS - 1; l >= 0; --l)
      if (w.idxn[l].rmax > 0.0f && cq <= w.idxn[l].cmax) lvl = l;
    const DevIndex& Xc = lvl >= 0 ? w.idxn[lvl] : X;
    // the source's row and length out of its edge's source record: the row's
    // address from the chosen candidate alone, the length beside it
    int32_t leni = 0;
    if (X.rmax > 0.0f && cq <= X.cmax) {
      Rw = src_row(Xc.src, ei, cand_node(oi));
      leni = Xc.src[ei].len;
      sv = idx_find(Xc.slot, Rw, dst_key(g, ej, oj), lab);
    }
    if (sv < 0 || idx_slot_cost(lab) > cq) {
      spill_push<CTR_INDEX_MISS, TIER_ROUTE_ONLINE>(w, (int32_t)p);
      continue;
    }
    // the path: the label's predecessor slots in the row, back to the first
    // edge (a slot holds its label's edge and its predecessor's slot)
    int len = 0;
    for (int32_t ps = idx_slot_pred(lab); ps >= 0 && len <= Rw.cnt; ps = idx_slot_pred(Xc.slot[Rw.off + ps])) ++len;
    const int off = len ? atomicAdd(&w.counters_i32[CTR_POOL_USED], len) : 0;
    if (off + len > w.pool_cap) {
      w.counters_i32[CTR_POOL_OVER] = 1;
      *w.abort = 1;
      w.path_len[p] = -1;
    } else {
      int k = len;
      for (int32_t ps = idx_slot_pred(lab); ps >= 0 && k > 0;) {
        const uint4 sl = Xc.slot[Rw.off + ps];
        w.path_pool[off + (--k)] = (int32_t)sl.x;
        ps = idx_slot_pred(sl);
      }
      w.path_off[p] = off;
      w.path_len[p] = len;
    }
    const float start = cand_node(oi) ? 0.0f : __int_as_float(leni) - oi;  // src_start
    const float sd = start + bitsf(lab.z);
    w.route_dist[p] = sd + oj;
    if (w.ctr) {
      unsigned long long st = 0, rl = 0;
      for (int64_t k = 0; k < (int64_t)Rw.cap; ++k) {
        const uint4 sl = Xc.slot[Rw.off + k];
        if (sl.x == EMPTY || (sl.x & NODE_KEY) || idx_slot_cost(sl) > cq) continue;
        ++st;
        if ((unsigned long long)idx_slot_cost(sl) + g.e_len64[sl.x] <= cq) {
          const int32_t v = g.e_to[sl.x];
          rl += (unsigned long long)(g.out_off[v + 1] - g.out_off[v]);
        }
      }
      ++c_search;
      c_settled += st;
      c_relaxed += rl;
      c_edges += (unsigned long long)len;
    }
  }
  if (w.ctr) {
    cadd(&w.ctr->route_searches, c_search);
    cadd(&w.ctr->route_nodes_settled, c_settled);
    cadd(&w.ctr->route_edges_relaxed, c_relaxed);
    cadd(&w.ctr->route_edges, c_edges);
  }
}

// ============================================================== K4 transitions (wave tiers)
// Columns the index tier could not answer (CTR_INDEX_MISS, list and count
// read on the device: no host round trip): one turn-aware
// search per distinct source (node, heading), the wave's table in LDS.  The
// LDS tier spills to CTR_SEARCH_GLOBAL, which the
// global-memory tier (BIG) drains.
// the search table of a tier's block: LDS (0), global (1), huge (2)
template <int TIER>
__device__ __forceinline__ Table tier_table(const DevWork& w, uint32_t* lkey, unsigned long long* llab, uint32_t* linq,
                                            uint32_t* lfr0, uint32_t* lfr1) {
  if (TIER == 1) {
    const size_t base = (size_t)blockIdx.x * BIG_TABLE_CAP;
    return Table{w.big_key + base, w.big_lab + base, w.big_inq + base, w.big_fr + 2 * base,
                 w.big_fr + 2 * base + BIG_TABLE_CAP, BIG_TABLE_LOG2, SEARCH_LIMIT,
                 w.big_ins + (size_t)blockIdx.x * SEARCH_LIMIT, w.big_prev + blockIdx.x};
  }
  if (TIER == 2) {
    const size_t cap = (size_t)1 << w.huge_log2;
    const size_t base = (size_t)blockIdx.x * cap;
    const int lim = huge_limit(w.huge_log2);
    return Table{w.huge_key + base, w.huge_lab + base, w.huge_inq + base, w.huge_fr + 2 * base,
                 w.huge_fr + 2 * base + cap, w.huge_log2, lim, w.huge_ins + (size_t)blockIdx.x * lim,
                 w.huge_prev + blockIdx.x};
  }
  return Table{lkey, llab, linq, lfr0, lfr1, 8, LDS_TABLE_LIMIT};
}
// the huge tier has work but no tables yet: the host allocates them and
// redoes the batch -- or, when it cannot (huge_final), the listed columns'
// traces answer 500 (OTM_TERR_SEARCH_OVERFLOW) (returns true: the launch is done)
__device__ __forceinline__ bool huge_unready(DevWork& w, int64_t nwork, const int32_t* list) {
  if (nwork <= 0 || w.huge_log2 > 0) return false;
  if (w.huge_final) {
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < nwork; it += (int64_t)gridDim.x * blockDim.x)
      atomicCAS(&w.trace_err[w.pt_trace[list[it]]], 0, OTM_TERR_SEARCH_OVERFLOW);
  } else if (blockIdx.x == 0 && threadIdx.x == 0) {
    w.counters_i32[CTR_GROW_HUGE] = 1;
    *w.abort = 1;
  }
  return true;
}
// a huge-tier search that outgrew its table: the host grows the tables and
// redoes the batch, or (huge_final) the column's trace answers 500
__device__ __forceinline__ void huge_overflow(DevWork& w, int64_t p) {
  if (w.huge_final) {
    atomicCAS(&w.trace_err[w.pt_trace[p]], 0, OTM_TERR_SEARCH_OVERFLOW);
  } else {
    w.counters_i32[CTR_GROW_HUGE] = 1;  // the huge tables are too small: grow, redo
    *w.abort = 1;
  }
}

// TIER 0: LDS tables; 1: global tables (BIG_SLOTS x BIG_TABLE_CAP); 2: the
// huge tier (HUGE_SLOTS x 2^huge_log2).  Spills: 0 -> CTR_SEARCH_GLOBAL -> 1 ->
// CTR_TRANS_HUGE -> 2 -> the host grows the huge tables and redoes the batch.
template <int TIER>
__global__ __launch_bounds__(TB) void k_transitions(DevGraph g, DevBatch b, DevParams P, DevWork w) {
  constexpr bool BIG = TIER > 0;
  if (*w.abort || trans_over_cap(b, w)) return;
  __shared__ uint32_t lkey[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ unsigned long long llab[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ uint32_t linq[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ uint32_t lfr0[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ uint32_t lfr1[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ int32_t cbuf[CHAIN_BUF * TB];
  __shared__ uint32_t TU[TURN_TABLE];
  __shared__ int32_t eq[KMAX], ep[KMAX];
  __shared__ float oq[KMAX], op[KMAX];
  __shared__ SearchShared S;
  const int lane = threadIdx.x;
  for (int k = lane; k < TURN_TABLE; k += TB) TU[k] = P.turn_units[k];
  Table T = tier_table<TIER>(w, lkey, llab, linq, lfr0, lfr1);
  auto predof = [&](uint32_t e) {
    const int sx = table_find<BIG>(T, e);
    return sx < 0 ? NONE_PRED : (uint32_t)(Mem<BIG>::ld(&T.lab[sx]) & 0xFFFFFFFFull);
  };
  const SpillRef work = TIER == 2 ? spill_of<CTR_TRANS_HUGE>(w)
                                  : (BIG ? spill_of<CTR_SEARCH_GLOBAL>(w) : spill_of<CTR_INDEX_MISS>(w));
  const int32_t* list = work.list;
  const int64_t nwork = (int64_t)*work.count;
  if (TIER == 2 && huge_unready(w, nwork, list)) return;
  __syncthreads();
  for (int64_t it = blockIdx.x; it < nwork; it += gridDim.x) {
    const int64_t p = (int64_t)list[it];
    const int32_t q = w.col_prev[p];
    if (q < 0) continue;
    const int Kq = w.ncand[q], Kp = w.ncand[p];
    const float gcv = w.gc[p];
    const float bound = P.factor * gcv;
    const uint32_t cq = index_cost_bound(bound);
    if (lane < Kq) {
      const int2 c = crec(w, q, lane);
      eq[lane] = c.x;
      oq[lane] = __int_as_float(c.y);
    }
    if (lane < Kp) {
      const int2 c = crec(w, p, lane);
      ep[lane] = c.x;
      op[lane] = __int_as_float(c.y);
    }
    __syncthreads();
    // distinct sources (node, heading), first occurrence order
    const int32_t u_l = lane < Kq ? src_node(g, eq[lane], oq[lane]) : -1;
    const uint32_t h_l = lane < Kq ? src_head(g, eq[lane], oq[lane]) : 0u;
    bool first = lane < Kq;
    for (int k = 0; k < Kq; ++k) {
      const int32_t uk = __shfl(u_l, k, 64);
      const uint32_t hk = __shfl(h_l, k, 64);
      if (k < lane && uk == u_l && hk == h_l) first = false;
    }
    unsigned long long srcmask = __ballot(first);
    float* Tm = w.trans + w.trans_off[p];
    bool failed = false;
    // work counts of this column, committed only if no search spilled (the
    // global tier redoes every source of a spilled column)
    unsigned long long c_search = 0, c_settled = 0, c_relaxed = 0, c_trans = 0;
    while (srcmask) {
      const int sl = __ffsll((long long)srcmask) - 1;
      srcmask &= srcmask - 1;
      const int32_t u = __shfl(u_l, sl, 64);
      const uint32_t hin = __shfl(h_l, sl, 64);
      const int labels = ta_search<BIG>(g, TU, T, S, u, hin, cq, lane);
      if (labels < 0) {
        failed = true;
        break;
      }
      unsigned long long ntr = 0;
      for (int idx = lane; idx < Kq * Kp; idx += TB) {
        const int i = idx / Kp, j = idx - (idx / Kp) * Kp;
        if (src_node(g, eq[i], oq[i]) != u || src_head(g, eq[i], oq[i]) != hin) continue;
        const int32_t ei = eq[i], ej = ep[j];
        const float start = src_start(g, ei, oq[i]);
        float r = 0.0f;
        uint32_t units = 0;
        bool ok = true;
        if (same_edge_step(ei, oq[i], ej, op[j])) {
          r = same_edge_dist(oq[i], op[j]);
        } else {
          const uint32_t key = dst_key(g, ej, op[j]);
          const int slot = table_find<BIG>(T, key);
          if (slot < 0) {
            ok = false;
          } else {
            float d;
            int n;
            chain_sums(g, TU, predof, (uint32_t)(Mem<BIG>::ld(&T.lab[slot]) & 0xFFFFFFFFull), hin,
                       (key & NODE_KEY) ? NO_HEAD : (uint32_t)g.e_head_out[ej], cbuf + lane, d, units, n);
            const float sd = start + d;
            r = sd + op[j];
          }
        }
        float cost = INFINITY;
        if (ok && r <= bound) {
          cost = trans_cost(units, r, gcv, P.beta);
          ++ntr;
        }
        Tm[i * Kp + j] = cost;
      }
      if (w.ctr) {
        unsigned long long st, rl;
        ta_counts<BIG>(g, T, cq, lane, st, rl);
        for (int o = 32; o > 0; o >>= 1) ntr += __shfl_xor(ntr, o, 64);
        c_search += 1;
        c_settled += st;
        c_relaxed += rl;
        c_trans += ntr;
      }
      __syncthreads();
    }
    if (w.ctr && !failed && lane == 0) {
      cadd(&w.ctr->searches, c_search);
      cadd(&w.ctr->nodes_settled, c_settled);
      cadd(&w.ctr->edges_relaxed, c_relaxed);
      cadd(&w.ctr->transitions, c_trans);
    }
    if (failed && lane == 0) {
      if (TIER == 0) {
        spill_push<CTR_SEARCH_GLOBAL>(w, (int32_t)p);
      } else if (TIER == 1) {
        spill_push<CTR_TRANS_HUGE>(w, (int32_t)p);
      } else {
        huge_overflow(w, p);
      }
    }
    __syncthreads();
  }
}

// ============================================================== K5 viterbi
__device__ __forceinline__ void wave_argmin(float v, int idx, float& bv, int& bi) {
  // lexicographic (value, index) minimum over the wave; +inf never wins
  bv = v;
  bi = idx;
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov < bv || (ov == bv && oi < bi)) {
      bv = ov;
      bi = oi;
    }
  }
}

// Global-memory form for one trace (traces too large for the LDS form).
__device__ void viterbi_trace_global(int64_t a, int64_t e, DevWork& w) {
  const int lane = threadIdx.x;
  {
    float prev = INFINITY;
    bool open = false;
    int64_t last = -1;
    auto backtrack = [&](int64_t endp) {
      const int Ke = w.ncand[endp];
      float bv;
      int bi;
      wave_argmin(lane < Ke ? prev : INFINITY, lane, bv, bi);
      __syncthreads();
      if (lane == 0) {
        int64_t pp = endp;
        int jj = bi;
        while (true) {
          w.state[pp] = jj;
          w.chosen[pp] = crec(w, pp, jj);
          if (w.chain_start[pp]) break;
          jj = w.bp[pp * KMAX + jj];
          pp = w.col_prev[pp];
        }
      }
    };
    for (int64_t p = a; p < e; ++p) {
      if (!w.is_col[p]) continue;
      const int Kp = w.ncand[p];
      if (Kp == 0) {
        if (open) backtrack(last);
        open = false;
        continue;
      }
      bool started = false;
      float cur = INFINITY;
      if (open && w.col_prev[p] == (int32_t)last) {
        const int Kq = w.ncand[last];
        const float* Tm = w.trans + w.trans_off[p];
        float best = INFINITY;
        int bi = -1;
        for (int i = 0; i < Kq; ++i) {
          const float pi = __shfl(prev, i, 64);
          if (lane < Kp) {
            const float v = pi + Tm[i * Kp + lane];
            if (v < best) {
              best = v;
              bi = i;
            }
          }
        }
        const bool alive = lane < Kp && bi >= 0;
        if (lane < Kp) {
          cur = alive ? best + cemis(w, p, lane) : INFINITY;
          w.bp[p * KMAX + lane] = alive ? (uint8_t)bi : (uint8_t)0xFF;
        }
        if (__ballot(alive) == 0ull) {
          backtrack(last);
        } else {
          started = true;
        }
      } else if (open) {
        backtrack(last);
      }
      if (!started) {
        cur = lane < Kp ? cemis(w, p, lane) : INFINITY;
        if (lane == 0) w.chain_start[p] = 1;
      }
      prev = cur;
      open = true;
      last = p;
    }
    __syncthreads();
    if (open) backtrack(last);
    __syncthreads();
  }
}
// LDS form: one wavefront per trace.  The trace's column metadata (and its
// backpointers, which never touch HBM) live in LDS for the whole trace; the
// transition block and emissions are streamed through LDS in windows of
// consecutive columns, each staged with coalesced loads.  The forward pass
// runs out of LDS with the previous column's scores broadcast by readlane;
// the backtrack walks LDS; state / chain_start go out coalesced.  Same
// recurrence, tie rules and chain breaks as viterbi_trace_global.
// LDS per trace (~5 KB at these sizes) and 64 VGPRs give 8 waves per SIMD
// (128 points of metadata: 0.218 -> 0.207 ms on config 2 against 256; 8
// waves instead of 7 with a 448-float window and 768 backpointers: 2.20 ->
// 1.96 ms on a config-3 shard, 0.201 -> 0.198 on config 2); a
// trace longer than VIT_PTS, whose candidates exceed VIT_BP, or with one
// column pair's block beyond VIT_TW, takes the global-memory form.
#ifndef OTM_VIT_TW
#define OTM_VIT_TW 448
#endif
#ifndef OTM_VIT_BP
#define OTM_VIT_BP 768
#endif
#ifndef OTM_VIT_PTS
#define OTM_VIT_PTS 128
#endif
constexpr int VIT_PTS = OTM_VIT_PTS; // points per trace (metadata held for the whole trace)
constexpr int VIT_BP = OTM_VIT_BP;   // candidates per trace (backpointers)
constexpr int VIT_TW = OTM_VIT_TW;   // transition floats per window (>= one column pair's block)
// emission floats per window (>= KMAX)
#ifndef OTM_VIT_EW
#define OTM_VIT_EW 256
#endif
constexpr int VIT_EW = OTM_VIT_EW;
static_assert(VIT_EW >= KMAX, "one column's emissions fit a window");

#ifndef OTM_VIT_WAVES
#define OTM_VIT_WAVES 8
#endif
// Measured and not kept (profiles/r02_ab_viterbi.txt): a one-read backtrack
// through trace-wide backpointer indices (0.159 vs 0.157 ms, and 16-bit
// backpointers cost occupancy), one global round trip per window (equal).
// list / list_n: the traces to decode (null: all); snap: this launch takes
// spill snapshot B (the first Viterbi launch of the batch)
__global__ __launch_bounds__(TB, OTM_VIT_WAVES) void k_viterbi(DevBatch b, DevWork w, const int32_t* list,
                                                               const int32_t* list_n, int snap) {
  // spill snapshot B: columns per transition tier (Viterbi does not touch the
  // counters; they start over for the route tiers)
  if (snap && blockIdx.x == 0 && threadIdx.x == 0) fold_snap(w, SNAP_AFTER_TRANS, true);
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  __shared__ float sT[VIT_TW];
  __shared__ float sEm[VIT_EW];
  __shared__ uint8_t sBp[VIT_BP];
  __shared__ int8_t sState[VIT_PTS];
  __shared__ uint8_t sCs[VIT_PTS];
  __shared__ int32_t sToff[VIT_PTS + 1];
  __shared__ int16_t sEoff[VIT_PTS + 1];
  __shared__ int16_t sCprev[VIT_PTS];
  __shared__ int8_t sKc[VIT_PTS];  // ncand of a column, -1 for a non-column point
  const int lane = threadIdx.x;
  const int32_t nwork = list ? *list_n : b.n_traces;
  for (int32_t it = blockIdx.x; it < nwork; it += gridDim.x) {
    const int32_t t = list ? list[it] : it;
    const int64_t a = b.trace_off[t], e = b.trace_off[t + 1];
    const int n = (int)(e - a);
    if (w.trace_err[t] != 0) {
      for (int64_t p = a + lane; p < e; p += TB) {
        w.state[p] = -1;
        w.chain_start[p] = 0;
      }
      continue;
    }
    const int64_t t0 = w.trans_off[a];
    int etot = 0;
    bool fits = n <= VIT_PTS;
    if (fits) {
      // column metadata + emission offsets (wave scan of ncand)
      bool big = false;  // a column pair's block beyond the window
      for (int c = 0; c < n; c += TB) {
        const int pl = c + lane;
        int kc = -1, cp = -1, to = 0;
        if (pl < n) {
          // independent loads (ncand / col_prev are defined for every point)
          const int64_t p = a + pl;
          const uint8_t ic = w.is_col[p];
          const int32_t nc = w.ncand[p];
          const int32_t q = w.col_prev[p];
          const int64_t tp = w.trans_off[p];
          const int64_t tn = w.trans_off[p + 1];
          if (ic) {
            kc = nc;
            cp = q >= 0 ? (int)(q - a) : -1;
          }
          to = (int)(tp - t0);
          big = big || tn - tp > VIT_TW;
        }
        const int k = kc > 0 ? kc : 0;
        const int incl = wave_incl_scan(k, lane);
        if (pl < n) {
          sKc[pl] = (int8_t)kc;
          sCprev[pl] = (int16_t)cp;
          sToff[pl] = to;
          sEoff[pl] = (int16_t)min(etot + incl - k, 32767);
          sState[pl] = -1;
          sCs[pl] = 0;
        }
        etot += __shfl(incl, 63, 64);
      }
      fits = etot <= VIT_BP && __ballot(big) == 0ull;
    }
    if (!fits) {
      __syncthreads();
      for (int64_t p = a + lane; p < e; p += TB) {
        w.state[p] = -1;
        w.chain_start[p] = 0;
      }
      __syncthreads();
      viterbi_trace_global(a, e, w);
      continue;
    }
    if (lane == 0) {
      sToff[n] = n > 0 ? (int)(w.trans_off[e] - t0) : 0;
      sEoff[n] = (int16_t)etot;
    }
    __syncthreads();
    float prev = INFINITY;
    bool open = false;
    int last = -1;
    int win_end = 0, wt0 = 0, we0 = 0;
    auto backtrack = [&](int endl, int Ke) {
      float bv;
      int bi;
      wave_argmin(lane < Ke ? prev : INFINITY, lane, bv, bi);
      __syncthreads();  // backpointers written by other lanes
      if (lane == 0) {
        int pl = endl;
        int jj = bi;
        while (true) {
          sState[pl] = (int8_t)jj;
          if (sCs[pl]) break;
          jj = sBp[sEoff[pl] + jj];
          pl = sCprev[pl];
        }
      }
    };
    // The forward pass walks the points in chunks of 64 whose metadata sits
    // in registers (lane k holds point c0 + k) and is read with readlane: the
    // per-column chain keeps one LDS round trip (emission + transition reads,
    // issued together) instead of five dependent ones.
    int lastK = 0;  // candidates of column `last`
    for (int c0 = 0; c0 < n; c0 += TB) {
      const int pk = c0 + lane;
      const int r_kc = pk < n ? (int)sKc[pk] : -1;
      const int r_eo = pk < n ? (int)sEoff[pk] : 0;
      const int r_cp = pk < n ? (int)sCprev[pk] : -1;
      const int r_to = pk < n ? sToff[pk] : 0;
      const int cend = n - c0 < TB ? n - c0 : TB;
      for (int k = 0; k < cend; ++k) {
        const int pl = c0 + k;
        const int Kp = __builtin_amdgcn_readlane(r_kc, k);
        if (Kp < 0) continue;
        if (Kp == 0) {
          if (open) backtrack(last, lastK);
          open = false;
          continue;
        }
        if (pl >= win_end) {
          // next window: the longest run of points from pl whose transitions
          // and emissions fit (one point always does)
          __syncthreads();
          wt0 = sToff[pl];
          we0 = sEoff[pl];
          // window end: Toff / Eoff are monotone, so the points that fit are
          // a prefix -- 64 candidates per LDS round trip, counted by ballot
          int we = pl + 1;
          while (we < n) {
            const int q = we + 1 + lane;
            const bool ok = q <= n && sToff[q] - wt0 <= VIT_TW && sEoff[q] - we0 <= VIT_EW;
            const int cnt = __popcll(__ballot(ok));
            we += cnt;
            if (cnt < TB) break;
          }
          win_end = we;
          const int nt = sToff[win_end] - wt0;
          for (int f0 = 0; f0 < nt; f0 += 8 * TB) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const int f = f0 + u * TB + lane;
              v[u] = f < nt ? w.trans[t0 + wt0 + f] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const int f = f0 + u * TB + lane;
              if (f < nt) sT[f] = v[u];
            }
          }
          // emissions point-parallel: lane q copies point q's candidates
          // (independent loads, no search for a candidate's point)
          for (int q0 = pl; q0 < win_end; q0 += TB) {
            const int q = q0 + lane;
            int kq = 0, eq = 0;
            if (q < win_end) {
              kq = sKc[q];
              eq = sEoff[q] - we0;
            }
            // the inline slots as two 16-byte loads of the point's 32-byte
            // block (consecutive lanes: consecutive blocks), the rest (points
            // with more than KIN candidates) from the overflow slots
            if (kq > 0) {
              const float4* e4 = (const float4*)(w.cand_em + (a + q) * KIN);
              const float4 x0 = e4[0];
              const float4 x1 = KIN > 4 && kq > 4 ? e4[KIN > 4 ? 1 : 0] : x0;
              const float v[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
              for (int u = 0; u < KIN; ++u)
                if (u < kq) sEm[eq + u] = v[u];
            }
            for (int j0 = KIN; __ballot(j0 < kq) != 0ull; j0 += 4) {
              float v[4];
#pragma unroll
              for (int u = 0; u < 4; ++u)
                v[u] = j0 + u < kq ? w.cand_xem[(a + q) * KX + (j0 - KIN + u)] : 0.0f;
#pragma unroll
              for (int u = 0; u < 4; ++u)
                if (j0 + u < kq) sEm[eq + j0 + u] = v[u];
            }
          }
          __syncthreads();
        }
        const int eo = __builtin_amdgcn_readlane(r_eo, k);
        const float em = sEm[eo - we0 + (lane < Kp ? lane : 0)];
        bool started = false;
        float cur = INFINITY;
        if (open && __builtin_amdgcn_readlane(r_cp, k) == last) {
          const int Kq = lastK;
          const float* Tm = sT + (__builtin_amdgcn_readlane(r_to, k) - wt0) + (lane < Kp ? lane : 0);
          float best = INFINITY;
          int bi = -1;
          const int pbits = __float_as_int(prev);
          int i = 0;
          for (; i + 4 <= Kq; i += 4) {
            // four independent LDS reads in flight.  The four in i order with
            // strict < are: the chunk's minimum, if below best, at the first
            // u that reaches it -- a min tree and three selects instead of
            // four compare-and-select pairs (sums of costs >= +0: no NaN, no
            // -0, so min and == see exactly what < saw)
            float tv[4], pv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              tv[u] = Tm[(i + u) * Kp];
              pv[u] = __int_as_float(__builtin_amdgcn_readlane(pbits, i + u));
            }
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = pv[u] + tv[u];
            const float m = fminf(fminf(v[0], v[1]), fminf(v[2], v[3]));
            const int fu = v[0] == m ? 0 : (v[1] == m ? 1 : (v[2] == m ? 2 : 3));
            if (m < best) {
              best = m;
              bi = i + fu;
            }
          }
          for (; i < Kq; ++i) {
            const float v = __int_as_float(__builtin_amdgcn_readlane(pbits, i)) + Tm[i * Kp];
            if (v < best) {
              best = v;
              bi = i;
            }
          }
          const bool alive = lane < Kp && bi >= 0;
          if (lane < Kp) {
            cur = alive ? best + em : INFINITY;
            sBp[eo + lane] = alive ? (uint8_t)bi : (uint8_t)0xFF;
          }
          if (__ballot(alive) == 0ull) {
            backtrack(last, lastK);
          } else {
            started = true;
          }
        } else if (open) {
          backtrack(last, lastK);
        }
        if (!started) {
          cur = lane < Kp ? em : INFINITY;
          if (lane == 0) sCs[pl] = 1;
        }
        prev = cur;
        open = true;
        last = pl;
        lastK = Kp;
      }
    }
    if (open) backtrack(last, lastK);
    __syncthreads();
    for (int pl = lane; pl < n; pl += TB) {
      const int st = sState[pl];
      const int cs = sCs[pl];
      w.state[a + pl] = st;
      w.chain_start[a + pl] = (uint8_t)cs;
      // the chosen candidate, compact for the route and segment stages
      if (st >= 0) {
        w.chosen[a + pl] = crec(w, a + pl, st);
      }
    }
    __syncthreads();
  }
}

// K5, G lanes per trace (G = 8 or 16: 64 / G traces per wavefront; DESIGN.md
// §5 K5).  The wave-per-trace form above is VALU-issue bound (round 3 PMC:
// 534M VALU instructions over 10M points at config 4, 82 % of the SIMDs'
// cycles) with Kq <= 8 of its 64 lanes holding states; here one instruction
// stream steps 64 / G traces.  A group (lane j = state j) walks its trace's
// points in chunks of OTM_VG_CHUNK:
//  * a chunk's transition blocks (contiguous in the trace's stream, bounded
//    by K3's trans_off) and its points' emissions are loaded into registers
//    one chunk ahead -- in flight while the group steps through the current
//    chunk -- and staged through a per-group LDS window at the chunk's start
//    (a chunk whose blocks exceed the window reads them from HBM per step);
//    the per-point metadata is K3's one byte (vmeta), loaded two chunks ahead;
//  * a step reads its point's byte by shuffle and its block from LDS;
//  * a column's backpointers as one byte per state in LDS; a chain's end
//    records its argmin state;
//  * after the forward pass one lane per group walks the trace backward.
// (Round 4's first form loaded each step's block from HBM at the step: one
// exposed round trip per point, 0.645 ms on config 2 against 0.155 for the
// wave form.)  A trace with a column of more than G candidates, or more than
// VG_PTS points, goes to the next form's list (G = 8 -> G = 16 -> the wave
// form).  Same recurrence (min over i in order, strict <), tie rules and chain
// breaks as viterbi_trace_global: bit-identical to the oracle.
// The block is one wavefront (TB = 64): a chunk's staging needs only
// wave_sync(), not __syncthreads(), which would wait for the next chunks'
// prefetches.
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int x = __shfl_xor(v, o, 64);
    v = x > v ? x : v;
  }
  return v;
}
// waves per SIMD: 8 lanes per trace fits 4 in 128 VGPRs with a 12-float
// window per lane; 16 lanes per trace spills at 4, so 3
#ifndef OTM_VG8_WAVES
#define OTM_VG8_WAVES 4
#endif
#ifndef OTM_VG8_U
#define OTM_VG8_U 8
#endif
// points per chunk: 8 or 16 overflowed the 16-float-per-lane window on most of
// config 2's chunks (~20 transition floats per column), whose steps then read
// their blocks from HBM one round trip each (form 8: 0.699 ms, config 2)
#ifndef OTM_VG_CHUNK
#define OTM_VG_CHUNK 4
#endif
constexpr int VG_PTS = 128;  // points per trace
constexpr uint8_t VG_COL = 1, VG_CS = 2, VG_END = 4;  // point flags (VG_END: argmin state in bits 3..7)
template <int G>
__global__ __launch_bounds__(TB, G == 8 ? OTM_VG8_WAVES : 3) void k_viterbi_g(DevBatch b, DevWork w, const int32_t* list,
                                                                const int32_t* list_n, int32_t* rej, int32_t* rej_n,
                                                                int snap) {
  static_assert(G == 8 || G == 16, "8 or 16 lanes per trace");
  constexpr int NT = TB / G;
  constexpr int U = G == 8 ? OTM_VG8_U : 16;  // transition floats per lane per chunk
  constexpr int VT = U * G;                    // ... per chunk window
  constexpr int CH = OTM_VG_CHUNK;  // points per chunk (<= G)
  static_assert(CH <= G, "a chunk's metadata is one byte per lane");
  // spill snapshot B (see k_viterbi)
  if (snap && blockIdx.x == 0 && threadIdx.x == 0) fold_snap(w, SNAP_AFTER_TRANS, true);
  if (*w.abort) return;
  // group rows padded by G words: group g's row starts g x G banks on, so the
  // wave's 64 lanes staging (or reading) the same offset j of their groups'
  // rows hit 64 different banks (round 4's one-word pad put group g + 1's
  // j on group g's j + 1: 39 % of the LDS cycles were bank conflicts, config 4)
  __shared__ float sT[NT][VT + G];
  __shared__ float sE[NT][CH * G + G];  // [point of the chunk][state]
  // backpointers, a nibble per state (15: dead), two states a byte: [point * G / 2 + state / 2]
  __shared__ uint8_t sBp[NT][VG_PTS * G / 2 + 4];
  __shared__ uint8_t sFl[NT][VG_PTS];  // flags; after the walk: VG_CS | (state + 1) << 3
  // each group's previous-column scores, so a step reads four of them with one
  // 16-byte broadcast read instead of four cross-lane shuffles
  __shared__ __attribute__((aligned(16))) float sP[NT][G];
  const int lane = threadIdx.x;
  const int g = lane / G, j = lane % G, gb = g * G;
  const unsigned long long gmask = (1ull << G) - 1ull;
  const int32_t ntr = list ? *list_n : b.n_traces;
  for (int32_t tb = blockIdx.x * NT; tb < ntr; tb += gridDim.x * NT) {
    const int32_t it = tb + g;
    bool act = it < ntr;
    const int32_t t = act ? (list ? list[it] : it) : 0;
    int64_t a = 0;
    int n = 0;
    int64_t t0 = 0;
    if (act) {
      a = b.trace_off[t];
      n = (int)(b.trace_off[t + 1] - a);
      t0 = w.trans_off[a];
      if (w.trace_err[t] != 0) {
        for (int pl = j; pl < n; pl += G) {
          w.state[a + pl] = -1;
          w.chain_start[a + pl] = 0;
        }
        act = false;
      }
    }
    // a trace this form cannot take: to the next form's list
    bool take = act && n <= VG_PTS;
    if (take) {
      bool wide = false;
      for (int pl = j; pl < n; pl += G) {
        const int vm = w.vmeta[a + pl];
        wide = wide || ((vm & 0x40) && (vm & 0x3F) > G);
      }
      take = ((__ballot(wide) >> gb) & gmask) == 0ull;
    }
    if (act && !take) {
      if (j == 0) {
        tier_wake<TIER_VIT_LISTS>(w);
        rej[atomicAdd(rej_n, 1)] = t;
      }
      act = false;
    }
    if (!act) n = 0;
    const int nch = (wave_max_i(n) + CH - 1) / CH;
    for (int pl = j; pl < n; pl += G) sFl[g][pl] = 0;
    // ---- the chunk pipeline: data two chunks ahead (two register sets, A for
    // even chunks, B for odd), metadata and T range four ahead
    // Every pipeline load is issued unconditionally (indices clamped into the
    // trace, results masked after): a fixed count per chunk lets the compiler
    // wait for exactly the older set, not for everything in flight.
    const int nl = n > 0 ? n - 1 : 0;  // (a trace's last point; 0 for an idle group)
    // (raw: a step reads lane k < CH's byte, and only for a point pl < n)
    auto ld_meta = [&](int c) {
      const int pl = c * CH + j;
      return (int)w.vmeta[a + (pl < nl ? pl : nl)];
    };
    // (the raw offsets: the subtraction waits for the loads, so it is done
    // where they are used, chunks later)
    auto ld_range = [&](int c, int64_t& lo, int64_t& hi) {
      const int p0 = c * CH < n ? c * CH : n, p1 = c * CH + CH < n ? c * CH + CH : n;
      lo = w.trans_off[a + p0];
      hi = w.trans_off[a + p1];
    };
    float pTa[U], pEa[CH], pTb[U], pEb[CH];
    auto ld_data = [&](int c, int m, int lo, int hi, float (&pT)[U], float (&pE)[CH]) {
      // raw values, no select on them here (a select would wait for the
      // load): the steps read only a window's valid floats and a point's
      // candidates (lo, hi: from the trace's first float; past hi, the
      // stream's capacity headroom)
      (void)m;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int f = lo + u * G + j;
        pT[u] = w.trans[t0 + (f < hi ? f : lo)];
      }
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        const int pl = c * CH + k < nl ? c * CH + k : nl;
        pE[k] = j < KIN ? w.cand_em[(a + pl) * KIN + j] : w.cand_xem[(a + pl) * KX + (j - KIN)];
      }
    };
    int m0 = ld_meta(0), m1 = ld_meta(1), m2 = ld_meta(2), m3 = ld_meta(3);
    int64_t lo0, hi0, lo1, hi1, lo2, hi2, lo3, hi3;
    ld_range(0, lo0, hi0);
    ld_range(1, lo1, hi1);
    ld_range(2, lo2, hi2);
    ld_range(3, lo3, hi3);
    ld_data(0, m0, (int)(lo0 - t0), (int)(hi0 - t0), pTa, pEa);
    ld_data(1, m1, (int)(lo1 - t0), (int)(hi1 - t0), pTb, pEb);
    // ---- forward pass (wave-uniform step count; groups predicated)
    float prev = INFINITY;
    sP[g][j] = INFINITY;
    bool open = false;
    int last = -1, lastK = 0;
    int acc = 0;  // the trace's transition floats before this column (K3's Kq x Kp counts, summed in order)
    auto end_chain = [&]() {
      // argmin (value, state) over the group's lanes < lastK, ties to the lower state
      float bv = j < lastK ? prev : INFINITY;
      int bi = j;
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, G);
        const int oi = __shfl_xor(bi, o, G);
        if (ov < bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      if (j == 0) sFl[g][last] = (uint8_t)(sFl[g][last] | VG_END | (bi << 3));
    };
    auto stage = [&](const float (&pT)[U], const float (&pE)[CH]) {
#pragma unroll
      for (int u = 0; u < U; ++u) sT[g][u * G + j] = pT[u];
#pragma unroll
      for (int k = 0; k < CH; ++k) sE[g][k * G + j] = pE[k];
    };
    auto chunk = [&](int c, int m_c, int lo_c, int hi_c) {
      // A step, for every group at once: its point's byte by shuffle, its
      // emission and block from LDS, Kq in fours (loads issued together), its
      // backpointers as one byte per state in LDS.  The loop bounds are
      // wave-uniform ballots, not unrolled to G (round 4's unrolled form spent
      // ~600 instructions per step).
      const bool big = hi_c - lo_c > VT;  // this group's chunk overflowed its window
      for (int k = 0; k < CH; ++k) {
        const int pl = c * CH + k;
        const int mk = __shfl(m_c, gb + k, TB);
        const bool on = pl < n && (mk & 0x40);
        const int Kp = mk & 0x3F;
        if (on && Kp == 0) {
          if (open) end_chain();
          open = false;
        }
        const bool col = on && Kp > 0;
        const bool link = col && open && (mk & 0x80);
        // a linked column's block follows the trace's earlier ones (its
        // previous column is the open chain's last)
        const int to = acc;
        if (link) acc += lastK * Kp;
        const int jj = j < Kp ? j : 0;
        const float em = sE[g][k * G + jj];
        int tb = to - lo_c;
        if (__ballot(big && link) != 0ull) {
          // the column's block (<= G x G floats) into the window first, so
          // the recurrence reads LDS only
          if (big) {
            tb = 0;
            if (link)
              for (int f = j; f < lastK * Kp; f += G) sT[g][f] = w.trans[t0 + to + f];
          }
        }
        bool started = false;
        float cur = INFINITY;
        if (__ballot(link) != 0ull) {
          float best = INFINITY;
          int bi = -1;
          const float* Tm = &sT[g][tb + jj];
          for (int i0 = 0; __ballot(link && i0 < lastK) != 0ull; i0 += 4) {
            float tv[4], pv[4];
            const float4 p4 = *(const float4*)&sP[g][i0 < G ? i0 : 0];
            pv[0] = p4.x;
            pv[1] = p4.y;
            pv[2] = p4.z;
            pv[3] = p4.w;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int i = i0 + u;
              tv[u] = link && i < lastK ? Tm[i * Kp] : INFINITY;
            }
            // (an i past lastK, or a lane of an unlinked group, reads +inf:
            // its sum is +inf and never below best.)  In i order with strict
            // <, the four are the chunk's minimum, if below best, at the first
            // u that reaches it (k_viterbi's form; costs >= +0: no NaN or -0)
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = pv[u] + tv[u];
            const float m = fminf(fminf(v[0], v[1]), fminf(v[2], v[3]));
            const int fu = v[0] == m ? 0 : (v[1] == m ? 1 : (v[2] == m ? 2 : 3));
            if (m < best) {
              best = m;
              bi = i0 + fu;
            }
          }
          const bool alive = link && j < Kp && bi >= 0;
          if (link) {
            cur = alive ? best + em : INFINITY;
            const int nib = alive ? bi : 15;
            // the neighbour lane's nibble by a DPP quad permute [1,0,3,2] (one VALU op, no
            // LDS-pipe shuffle); every lane of a linked group is here
            const int pair = __builtin_amdgcn_mov_dpp(nib, 0xB1, 0xF, 0xF, false);
            if (!(j & 1)) sBp[g][pl * (G / 2) + (j >> 1)] = (uint8_t)(nib | (pair << 4));
            if (((__ballot(alive) >> gb) & (unsigned long long)gmask) != 0ull) started = true;
            else end_chain();
          }
        }
        if (col && !link && open) end_chain();
        if (col) {
          if (!started) {
            cur = j < Kp ? em : INFINITY;
            if (j == 0) sFl[g][pl] = VG_COL | VG_CS;
          } else if (j == 0) {
            sFl[g][pl] = VG_COL;
          }
          prev = cur;
          sP[g][j] = cur;
          open = true;
          last = pl;
          lastK = Kp;
        }
      }
    };
    for (int c = 0; c < nch; c += 2) {
      // chunk c from set A; chunk c + 2's loads into A behind it
      stage(pTa, pEa);
      const int ma = m0, la = (int)(lo0 - t0), ha = (int)(hi0 - t0);
      const int mn0 = ld_meta(c + 4);
      int64_t ln0, hn0;
      ld_range(c + 4, ln0, hn0);
      wave_sync();
      ld_data(c + 2, m2, (int)(lo2 - t0), (int)(hi2 - t0), pTa, pEa);
      chunk(c, ma, la, ha);
      wave_sync();  // (the next chunk's staging overwrites the windows)
      if (c + 1 >= nch) break;
      // chunk c + 1 from set B; chunk c + 3's loads into B
      stage(pTb, pEb);
      const int mb = m1, lb = (int)(lo1 - t0), hb = (int)(hi1 - t0);
      const int mn1 = ld_meta(c + 5);
      int64_t ln1, hn1;
      ld_range(c + 5, ln1, hn1);
      wave_sync();
      ld_data(c + 3, m3, (int)(lo3 - t0), (int)(hi3 - t0), pTb, pEb);
      chunk(c + 1, mb, lb, hb);
      wave_sync();
      m0 = m2;
      lo0 = lo2;
      hi0 = hi2;
      m1 = m3;
      lo1 = lo3;
      hi1 = hi3;
      m2 = mn0;
      lo2 = ln0;
      hi2 = hn0;
      m3 = mn1;
      lo3 = ln1;
      hi3 = hn1;
    }
    if (act && open) end_chain();
    __syncthreads();
    // ---- backtrack: one lane per group walks the trace backward
    if (j == 0) {
      int sv = -1;
      for (int pl = n - 1; pl >= 0; --pl) {
        const uint32_t f = sFl[g][pl];
        if (!(f & VG_COL)) {
          sFl[g][pl] = 0;
          continue;
        }
        if (f & VG_END) sv = (int)(f >> 3);
        sFl[g][pl] = (uint8_t)((f & VG_CS) | ((sv + 1) << 3));
        if (sv >= 0) {
          if (f & VG_CS) {
            sv = -1;
          } else {
            sv = (sBp[g][pl * (G / 2) + (sv >> 1)] >> ((sv & 1) * 4)) & 15;
          }
        }
      }
    }
    __syncthreads();
    // ---- outputs, point-parallel within the group
    for (int pl = j; pl < n; pl += G) {
      const uint32_t f = sFl[g][pl];
      const int sv = (int)(f >> 3) - 1;
      const int64_t p = a + pl;
      w.state[p] = sv;
      w.chain_start[p] = (uint8_t)((f & VG_CS) ? 1 : 0);
      if (sv >= 0) w.chosen[p] = crec(w, p, sv);
    }
    __syncthreads();
  }
}

// K5, one DPP row per trace (16 lanes, lane j = state j: four traces per
// wavefront) -- the form for batches between the wave form's
// and the grouped forms' (launch_viterbi: 4,096 to 32,767 traces).  The
// previous column's scores never leave their registers: a DPP
// row_newbcast hands lane i of each 16-lane row to the whole row as an operand
// of the add, so prev[i] + T[i][j] is one VALU instruction and the serial
// chain of a step holds no LDS access, shuffle or readlane.
//  * a trace's per-point word (K3's byte | the point's block offset in the
//    trace's transition stream << 8) goes into LDS once per trace; a chunk's
//    words are read, row-uniform, ahead of its steps;
//  * a chunk of OTM_VR_CH points' transition blocks (OTM_VR_U floats per lane)
//    and emissions are loaded into registers one chunk ahead, in flight while
//    the current chunk is stepped; the blocks are staged through a per-row LDS
//    window at the chunk's start, the emissions stay in their lane; a chunk
//    whose blocks exceed the window copies each step's block at the step;
//  * a step in which every row is idle, at an interpolated point or at a
//    column linked to its open chain inside the window (98.8 % of config 2's)
//    takes a fast path chosen wave-uniformly: the recurrence, the nibbles and
//    the chain's last column, nothing else (OTM_VR_FAST=0: never);
//  * backpointers as nibbles in LDS, a chain's end records its argmin, one
//    lane per row walks backward at the end; outputs point-parallel.
// DPP reads of a lane that EXEC has switched off do not return its value, so
// the recurrence runs with every lane enabled and masks by selects: `prev` is
// +inf in the lanes past a column's count (a source past Kq never wins), and
// what a lane reads from the windows for such a source, for a target past Kp
// or for an unlinked row is a cost (>= +0, +inf included) or a zero, never a
// NaN: the windows start as +inf and are only ever staged from the transition
// allocation, which starts as zeros and only ever holds costs (ld_data below;
// no read leaves the allocation).
// A trace with more than VR_PTS points or a column of more than 16 candidates
// goes to `rej`, for the wave form in list mode.  Same recurrence (min over i
// in order, strict <, the fours' min tree and first-index select), tie rules
// and chain breaks as viterbi_trace_global: bit-identical to the oracle.
#ifndef OTM_VR_CH
#define OTM_VR_CH 4
#endif
#ifndef OTM_VR_U
#define OTM_VR_U 16
#endif
#ifndef OTM_VR_WAVES
#define OTM_VR_WAVES 3
#endif
constexpr int VR_PTS = 128;  // points per trace
// four floats of the transition stream, which is aligned to a float only (a
// global_load_dwordx4 needs no more)
typedef float vr_f4 __attribute__((ext_vector_type(4), aligned(4)));
typedef float vr_f4a __attribute__((ext_vector_type(4)));  // (in LDS: 16-byte aligned)
// four sources i = I0 .. I0 + 3 of the recurrence: their window reads (issued
// for all of a step's fours before the first is used), then the sums (the DPP
// control is an immediate) and the running minimum
template <int I0>
__device__ __forceinline__ void vr_load(const float* Tm, const int Kp, float (&tv)[16]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) tv[I0 + u] = Tm[(I0 + u) * Kp];
}
template <int I0>
__device__ __forceinline__ void vr_four(const int pbits, const float (&tv)[16], float& best, int& bi) {
  float v0 = __int_as_float(__builtin_amdgcn_update_dpp(0, pbits, 0x150 + I0 + 0, 0xF, 0xF, false)) + tv[I0 + 0];
  float v1 = __int_as_float(__builtin_amdgcn_update_dpp(0, pbits, 0x150 + I0 + 1, 0xF, 0xF, false)) + tv[I0 + 1];
  float v2 = __int_as_float(__builtin_amdgcn_update_dpp(0, pbits, 0x150 + I0 + 2, 0xF, 0xF, false)) + tv[I0 + 2];
  float v3 = __int_as_float(__builtin_amdgcn_update_dpp(0, pbits, 0x150 + I0 + 3, 0xF, 0xF, false)) + tv[I0 + 3];
  // Each sum's bits through an empty asm: the SLP vectoriser otherwise packs
  // half of the sums into a v_mov_b32_dpp per source and a v_pk_add_f32 per
  // pair, which costs more issue than the two v_add_f32_dpp it replaces.
  // From there on the bits are compared as integers: the costs are >= +0
  // (no NaN, no -0; +inf included), where the signed order of the bits is the
  // floats' order, and an integer min needs no canonicalising v_max of a
  // value the compiler cannot see into.
  int i0 = __float_as_int(v0), i1 = __float_as_int(v1), i2 = __float_as_int(v2), i3 = __float_as_int(v3);
  asm("" : "+v"(i0));
  asm("" : "+v"(i1));
  asm("" : "+v"(i2));
  asm("" : "+v"(i3));
  // in i order with strict <: the four's minimum, if below best, at the
  // first u that reaches it (k_viterbi's form); selects, not branches
  const int m = min(min(i0, i1), min(i2, i3));
  int fu = 3;
  fu = i2 == m ? 2 : fu;
  fu = i1 == m ? 1 : fu;
  fu = i0 == m ? 0 : fu;
  const bool lt = m < __float_as_int(best);
  best = lt ? __int_as_float(m) : best;
  bi = lt ? I0 + fu : bi;
}
// win: the window's floats a chunk may use (<= VT; the tests force the
// per-step path with a small one)
__global__ __launch_bounds__(TB, OTM_VR_WAVES) void k_viterbi_row(DevBatch b, DevWork w, int32_t* rej, int32_t* rej_n,
                                                                  int win, int fast, int snap) {
  constexpr int G = 16, NT = TB / G;
  constexpr int CH = OTM_VR_CH, U = OTM_VR_U;
  constexpr int VT = U * G;                    // transition floats per chunk window
  constexpr int VTA = VT > G * G ? VT : G * G;  // (a window holds any one column pair's block)
  constexpr int RS = VTA + G;                  // row stride: row g starts g x 16 banks on
  static_assert(CH >= 1 && CH <= G && U >= 4 && U % 4 == 0, "chunk knobs");
  static_assert(RS % 4 == 0, "a row's window is staged by 16-byte stores");
  // spill snapshot B (see k_viterbi)
  if (snap && blockIdx.x == 0 && threadIdx.x == 0) fold_snap(w, SNAP_AFTER_TRANS, true);
  if (*w.abort) return;
  // the rows' windows, then G x G floats that stay +inf: a masked source's
  // read (up to 255 floats past a block's start) stays inside
  __shared__ __attribute__((aligned(16))) float sT[NT * RS + G * G];
  // a nibble per state (15: dead): [point * 8 + state / 2]
  __shared__ __attribute__((aligned(8))) uint8_t sBp[NT][VR_PTS * G / 2];
  // flags; after the walk: VG_CS | (state + 1) << 3
  __shared__ __attribute__((aligned(8))) uint8_t sFl[NT][VR_PTS];
  // K3's byte | (trans_off[p] - trans_off[a]) << 8; [n]: the trace's end (a chunk's four words: one 16-byte read)
  __shared__ __attribute__((aligned(16))) uint32_t sM[NT][VR_PTS + G];
  const int lane = threadIdx.x;
  const int g = lane / G, j = lane % G, gb = g * G;
  for (int f = lane; f < NT * RS + G * G; f += TB) sT[f] = INFINITY;
  float* const sTg = sT + g * RS;
  const int32_t ntr = b.n_traces;
  for (int32_t tb0 = blockIdx.x * NT; tb0 < ntr; tb0 += gridDim.x * NT) {
    const int32_t t = tb0 + g;
    bool act = t < ntr;
    int64_t a = 0, t0 = 0;
    int n = 0;
    if (act) {
      a = b.trace_off[t];
      n = (int)(b.trace_off[t + 1] - a);
      if (w.trace_err[t] != 0) {
        for (int pl = j; pl < n; pl += G) {
          w.state[a + pl] = -1;
          w.chain_start[a + pl] = 0;
        }
        act = false;
      }
      if (n <= 0) act = false;
    }
    // the trace's words (loads issued together, indices clamped into the
    // trace); a trace this form cannot take goes to the wave form's list
    bool take = act && n <= VR_PTS;
    if (take) {
      t0 = w.trans_off[a];
      int vm[VR_PTS / G + 1];
      int64_t to[VR_PTS / G + 1];
#pragma unroll
      for (int u = 0; u <= VR_PTS / G; ++u) {
        const int pl = u * G + j;
        vm[u] = w.vmeta[a + (pl < n ? pl : n - 1)];
        to[u] = w.trans_off[a + (pl < n ? pl : n)];
      }
      bool wide = false;
#pragma unroll
      for (int u = 0; u <= VR_PTS / G; ++u) {
        const int pl = u * G + j;
        if (pl < n) wide = wide || ((vm[u] & 0x40) && (vm[u] & 0x3F) > G);
        if (pl <= n) sM[g][pl] = (uint32_t)(pl < n ? vm[u] : 0) | ((uint32_t)(to[u] - t0) << 8);
      }
      take = ((__ballot(wide) >> gb) & 0xFFFFull) == 0ull;
    }
    if (act && !take) {
      if (j == 0) {
        tier_wake<TIER_VIT_LISTS>(w);
        rej[atomicAdd(rej_n, 1)] = t;
      }
      act = false;
    }
    if (!act) n = 0;
    // (wave-uniform, and said so: the chunk loop is a scalar one)
    const int nch = __builtin_amdgcn_readfirstlane((wave_max_i(n) + CH - 1) / CH);
    // VG_COL for a column with candidates, from the words this lane wrote
    // above (a plain step leaves its flag byte alone); the walk reads four
    // points' flags a turn
    for (int pl = j; pl < ((n + 3) & ~3); pl += G) {
      const uint32_t m = sM[g][pl];
      sFl[g][pl] = (uint8_t)(pl < n && (m & 0x40u) && (m & 0x3Fu) ? VG_COL : 0);
    }
    wave_sync();
    const int nl = n > 0 ? n - 1 : 0;
    // where chunk c's floats end in the trace's stream, which is where chunk
    // c + 1's begin (an idle row: empty, at the stream's start)
    auto rng_end = [&](int c) {
      const int p1 = c * CH + CH < n ? c * CH + CH : n;
      return act ? (int)(sM[g][p1] >> 8) : 0;
    };
    // this lane's emissions: one pointer and stride for the trace
    const float* const ep = j < KIN ? w.cand_em + a * KIN + j : w.cand_xem + a * KX + (j - KIN);
    const int es = j < KIN ? KIN : KX;
    // A chunk's window: the VT floats from its first on, four to a lane and
    // load (window float f = q * 4 G + 4 j + e is the stream's lo + f), by one
    // pointer with immediate offsets.  Where every row's VT floats lie inside
    // the allocation (trans_cap floats) nothing is clamped: what lies past a
    // chunk's end is the stream's next floats or what the allocation holds
    // behind the batch's last block, which is costs of this or an earlier
    // batch or the zeros it was created with (engine.cpp), never a NaN.
    // Within VT floats of the allocation's end, element by element with the
    // index clamped into the chunk (past hi: the chunk's first float again).
    vr_f4 pT[U / 4];
    float pE[CH];
    auto ld_data = [&](int c, int lo, int hi) {
      const int64_t f0 = t0 + lo;
      if (__ballot(f0 + VT > w.trans_cap) == 0ull) {
        const float* const tp = w.trans + (f0 + 4 * j);
#pragma unroll
        for (int q = 0; q < U / 4; ++q) pT[q] = *(const vr_f4*)(tp + q * 4 * G);
      } else {
#pragma unroll
        for (int q = 0; q < U / 4; ++q) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int f = lo + q * 4 * G + 4 * j + e;
            pT[q][e] = w.trans[t0 + (f < hi ? f : lo)];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        const int pl = c * CH + k < nl ? c * CH + k : nl;
        pE[k] = ep[pl * es];
      }
    };
    int lo_n = 0, hi_n = rng_end(0);
    ld_data(0, lo_n, hi_n);
    // ---- forward pass (wave-uniform step count; rows masked by selects)
    float prev = INFINITY;
    bool open = false;
    int last = 0, lastK = 0;
    auto end_chain = [&]() {
      // argmin (value, state) over the row's lanes < lastK, ties to the lower state
      float bv = j < lastK ? prev : INFINITY;
      int bi = j;
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, G);
        const int oi = __shfl_xor(bi, o, G);
        if (ov < bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      if (j == 0) sFl[g][last] = (uint8_t)(sFl[g][last] | VG_END | (bi << 3));
    };
    for (int c = 0; c < nch; ++c) {
      // stage chunk c's window (every load was inside the allocation and
      // found a cost or a zero: see ld_data), keep its emissions, read its
      // points' words (past the trace's end the row's LDS words, inside sM,
      // are whatever they were, and `on` is false there); then chunk c + 1's
      // loads, in flight behind the steps
      const int lo_c = lo_n, hi_c = hi_n;
#pragma unroll
      for (int q = 0; q < U / 4; ++q) *(vr_f4a*)(sTg + q * 4 * G + 4 * j) = pT[q];
      float em_c[CH];
      uint32_t mw[CH];
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        em_c[k] = pE[k];
        mw[k] = sM[g][c * CH + k];
      }
      wave_sync();
      lo_n = hi_c;
      hi_n = rng_end(c + 1);
      ld_data(c + 1, lo_n, hi_n);
      const bool big = hi_c - lo_c > win;  // this row's chunk overflowed its window
#pragma unroll
      for (int k = 0; k < CH; ++k) {
        const int pl = c * CH + k;
        const int mk = (int)(mw[k] & 0xFFu);
        const bool on = pl < n && (mk & 0x40);
        const int Kp = mk & 0x3F;
        const bool col = on && Kp > 0;
        // (a linked column's previous column is the open chain's last)
        const bool link = col && open && (mk & 0x80);
        const float em = em_c[k];
        // ---- the plain step: every row of the wave is idle, at an
        // interpolated point (both: !on, nothing changes), or at a column
        // that links to its open chain with its block in the window.  Only
        // the recurrence, the nibbles and the chain's last column: no chain
        // end, no chain start, no flag byte (VG_COL stands since set-up).
        // A linked row in which no state is alive leaves it: that step, like
        // every one that is not plain, runs the general body below, which
        // has seen none of this one's work.
        // (a bool's ballot as the compiler's own, a scalar and of the
        // condition's mask: __ballot's goes through a select and a compare)
        if (fast && __builtin_amdgcn_ballot_w64(on && (!link || big)) == 0ull) {
          const unsigned long long lb = __builtin_amdgcn_ballot_w64(link);
          bool done = true;
          if (lb != 0ull) {
            float best = INFINITY;
            int bi = -1;
            const int pbits = __float_as_int(prev);
            const float* Tm = sTg + (link ? (int)(mw[k] >> 8) - lo_c : 0) + j;
            const int KpL = link ? Kp : 0;
            const int Kq = link ? lastK : 0;
            const bool g1 = __ballot(Kq > 4) != 0ull, g2 = __ballot(Kq > 8) != 0ull, g3 = __ballot(Kq > 12) != 0ull;
            float tv[16];
            vr_load<0>(Tm, KpL, tv);
            if (g1) vr_load<4>(Tm, KpL, tv);
            if (g2) vr_load<8>(Tm, KpL, tv);
            if (g3) vr_load<12>(Tm, KpL, tv);
            vr_four<0>(pbits, tv, best, bi);
            if (g1) vr_four<4>(pbits, tv, best, bi);
            if (g2) vr_four<8>(pbits, tv, best, bi);
            if (g3) vr_four<12>(pbits, tv, best, bi);
            const bool alive = link && j < Kp && bi >= 0;
            // bit 16 r + 15: a state of row r is alive (scalar work: a row's
            // 16 bits are not zero when adding 0x7FFF to the low 15 carries
            // into the 16th, or the 16th is set)
            const unsigned long long ab = __builtin_amdgcn_ballot_w64(alive);
            const unsigned long long any = ((ab & 0x7FFF7FFF7FFF7FFFull) + 0x7FFF7FFF7FFF7FFFull) | ab;
            done = (lb & ~any & 0x8000800080008000ull) == 0ull;
            if (done) {
              const int nib = alive ? bi : 15;
              const int pair = __builtin_amdgcn_mov_dpp(nib, 0xB1, 0xF, 0xF, false);
              if (link && !(j & 1)) sBp[g][pl * (G / 2) + (j >> 1)] = (uint8_t)(nib | (pair << 4));
              const float cur = alive ? best + em : INFINITY;
              prev = link ? cur : prev;
              last = link ? pl : last;
              lastK = link ? Kp : lastK;
            }
          }
          if (done) continue;
        }
        // the open chain ends before a column without candidates and before
        // one that does not link to it
        if (on && open && !link) end_chain();
        int tb = link ? (int)(mw[k] >> 8) - lo_c : 0;
        if (__ballot(big && link) != 0ull) {
          // the column's block (<= G x G floats) into the window first, so
          // the recurrence reads LDS only
          if (big) {
            if (link) {
              const int64_t src = t0 + (int64_t)(mw[k] >> 8);
              for (int f = j; f < lastK * Kp; f += G) sTg[f] = w.trans[src + f];
            }
            tb = 0;
          }
          wave_sync();
        }
        bool started = false;
        float cur = INFINITY;
        const unsigned long long lb = __ballot(link);
        if (lb != 0ull) {
          // every lane runs this (see the DPP note above): an unlinked row's
          // result, and a lane's past Kp, are dropped by the selects below
          float best = INFINITY;
          int bi = -1;
          const int pbits = __float_as_int(prev);
          const float* Tm = sTg + tb + j;
          const int KpL = link ? Kp : 0;  // (an unlinked row reads its window's start)
          // (wave-uniform guards skip a four that no row needs)
          const bool g1 = __ballot(link && lastK > 4) != 0ull, g2 = __ballot(link && lastK > 8) != 0ull,
                     g3 = __ballot(link && lastK > 12) != 0ull;
          float tv[16];
          vr_load<0>(Tm, KpL, tv);
          if (g1) vr_load<4>(Tm, KpL, tv);
          if (g2) vr_load<8>(Tm, KpL, tv);
          if (g3) vr_load<12>(Tm, KpL, tv);
          vr_four<0>(pbits, tv, best, bi);
          if (g1) vr_four<4>(pbits, tv, best, bi);
          if (g2) vr_four<8>(pbits, tv, best, bi);
          if (g3) vr_four<12>(pbits, tv, best, bi);
          const bool alive = link && j < Kp && bi >= 0;
          const int nib = alive ? bi : 15;
          // the neighbour lane's nibble by a DPP quad permute [1,0,3,2]
          const int pair = __builtin_amdgcn_mov_dpp(nib, 0xB1, 0xF, 0xF, false);
          if (link) {
            cur = alive ? best + em : INFINITY;
            if (!(j & 1)) sBp[g][pl * (G / 2) + (j >> 1)] = (uint8_t)(nib | (pair << 4));
            if (((__ballot(alive) >> gb) & 0xFFFFull) != 0ull) started = true;
            else end_chain();
          }
        }
        // (selects, not branches: a column that continues no chain starts one)
        if (col && j == 0) sFl[g][pl] = (uint8_t)(started ? VG_COL : (VG_COL | VG_CS));
        cur = started ? cur : (j < Kp ? em : INFINITY);
        prev = col ? cur : prev;
        open = col || (open && !on);
        last = col ? pl : last;
        lastK = col ? Kp : lastK;
      }
      wave_sync();  // (the next chunk's staging overwrites the windows)
    }
    if (act && open) end_chain();
    wave_sync();
    // ---- backtrack: one lane per row walks the trace backward, four points
    // a turn: their flags as one word and each point's 16 nibbles as one
    // 8-byte read, none of which waits for the walk's state
    if (j == 0) {
      int sv = -1;
      for (int q = ((n + 3) >> 2) - 1; q >= 0; --q) {
        const uint32_t f4 = *(const uint32_t*)&sFl[g][q * 4];
        unsigned long long nb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) nb[u] = *(const unsigned long long*)&sBp[g][(q * 4 + u) * (G / 2)];
        uint32_t o4 = 0;
#pragma unroll
        for (int u = 3; u >= 0; --u) {
          const uint32_t f = (f4 >> (8 * u)) & 0xFFu;
          if (!(f & VG_COL)) continue;
          if (f & VG_END) sv = (int)(f >> 3);
          o4 |= ((f & VG_CS) | (uint32_t)((sv + 1) << 3)) << (8 * u);
          if (sv >= 0) sv = (f & VG_CS) ? -1 : (int)((nb[u] >> (4 * sv)) & 15ull);
        }
        *(uint32_t*)&sFl[g][q * 4] = o4;
      }
    }
    wave_sync();
    // ---- outputs, point-parallel within the row (the chosen candidates'
    // loads issued together, ahead of the stores)
    {
      int svs[VR_PTS / G];
      int2 ch[VR_PTS / G];
#pragma unroll
      for (int u = 0; u < VR_PTS / G; ++u) {
        const int pl = u * G + j;
        svs[u] = pl < n ? (int)(sFl[g][pl] >> 3) - 1 : -1;
        if (svs[u] >= 0) ch[u] = crec(w, a + pl, svs[u]);
      }
#pragma unroll
      for (int u = 0; u < VR_PTS / G; ++u) {
        const int pl = u * G + j;
        if (pl < n) {
          const int64_t p = a + pl;
          w.state[p] = svs[u];
          w.chain_start[p] = (uint8_t)((sFl[g][pl] & VG_CS) ? 1 : 0);
          if (svs[u] >= 0) w.chosen[p] = ch[u];
        }
      }
    }
    wave_sync();
  }
}

// ============================================================== K6 route
// Steps the index tier could not answer (CTR_INDEX_MISS):
// the winning search again, its target label's predecessor chain as the path.
// TIER as k_transitions (spills: CTR_INDEX_MISS -> CTR_SEARCH_GLOBAL -> CTR_ROUTE_HUGE)
template <int TIER>
__global__ __launch_bounds__(TB) void k_route(DevGraph g, DevBatch b, DevParams P, DevWork w) {
  constexpr bool BIG = TIER > 0;
  if (*w.abort) return;
  __shared__ uint32_t lkey[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ unsigned long long llab[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ uint32_t linq[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ uint32_t lfr0[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ uint32_t lfr1[BIG ? 1 : LDS_TABLE_CAP];
  __shared__ int32_t cbuf[CHAIN_BUF * TB];
  __shared__ uint32_t TU[TURN_TABLE];
  __shared__ SearchShared S;
  const int lane = threadIdx.x;
  for (int k = lane; k < TURN_TABLE; k += TB) TU[k] = P.turn_units[k];
  Table T = tier_table<TIER>(w, lkey, llab, linq, lfr0, lfr1);
  auto predof = [&](uint32_t e) {
    const int sx = table_find<BIG>(T, e);
    return sx < 0 ? NONE_PRED : (uint32_t)(Mem<BIG>::ld(&T.lab[sx]) & 0xFFFFFFFFull);
  };
  const SpillRef work = TIER == 2 ? spill_of<CTR_ROUTE_HUGE>(w)
                                  : (BIG ? spill_of<CTR_SEARCH_GLOBAL>(w) : spill_of<CTR_INDEX_MISS>(w));
  const int32_t* list = work.list;
  const int64_t nwork = (int64_t)*work.count;
  if (TIER == 2 && huge_unready(w, nwork, list)) return;
  __syncthreads();
  for (int64_t it = blockIdx.x; it < nwork; it += gridDim.x) {
    const int64_t p = (int64_t)list[it];
    const int32_t q = w.col_prev[p];
    const int2 ci = w.chosen[q], cj = w.chosen[p];
    const int32_t ei = ci.x, ej = cj.x;
    const float oi = __int_as_float(ci.y), oj = __int_as_float(cj.y);
    if (same_edge_step(ei, oi, ej, oj)) {
      if (lane == 0) w.route_dist[p] = same_edge_dist(oi, oj);
      continue;
    }
    const float bound = P.factor * w.gc[p];
    const uint32_t cq = index_cost_bound(bound);
    const int32_t u = src_node(g, ei, oi);
    const uint32_t hin = src_head(g, ei, oi);
    const int labels = ta_search<BIG>(g, TU, T, S, u, hin, cq, lane);
    if (labels < 0) {
      if (lane == 0) {
        if (TIER == 0) {
          spill_push<CTR_SEARCH_GLOBAL>(w, (int32_t)p);
        } else if (TIER == 1) {
          spill_push<CTR_ROUTE_HUGE>(w, (int32_t)p);
        } else {
          huge_overflow(w, p);
        }
      }
      __syncthreads();
      continue;
    }
    unsigned long long st = 0, rl = 0;
    if (w.ctr) ta_counts<BIG>(g, T, cq, lane, st, rl);
    if (lane == 0) {
      const uint32_t key = dst_key(g, ej, oj);
      const int vs = table_find<BIG>(T, key);
      if (vs < 0) {
        // (cannot happen: the step's transition was finite)
        atomicCAS(&w.trace_err[w.pt_trace[p]], 0, OTM_TERR_SEARCH_OVERFLOW);
      } else {
        const uint32_t pk = (uint32_t)(Mem<BIG>::ld(&T.lab[vs]) & 0xFFFFFFFFull);
        float d;
        uint32_t units;
        int n;
        chain_sums(g, TU, predof, pk, hin, NO_HEAD, cbuf, d, units, n);
        const int off = atomicAdd(&w.counters_i32[CTR_POOL_USED], n);
        if (off + n > w.pool_cap) {
          w.counters_i32[CTR_POOL_OVER] = 1;
          *w.abort = 1;
          w.path_len[p] = -1;
        } else {
          int k = n;
          for (uint32_t pe = pk; pe != NONE_PRED && k > 0; pe = predof(pe)) w.path_pool[off + (--k)] = (int32_t)pe;
          w.path_off[p] = off;
          w.path_len[p] = n;
        }
        const float start = src_start(g, ei, oi);
        const float sd = start + d;
        w.route_dist[p] = sd + oj;
        if (w.ctr) {
          cadd(&w.ctr->route_searches, 1);
          cadd(&w.ctr->route_nodes_settled, st);
          cadd(&w.ctr->route_edges_relaxed, rl);
          cadd(&w.ctr->route_edges, (unsigned long long)n);
        }
      }
    }
    __syncthreads();
  }
}

// ============================================================== K7 segments
// Per-edge attributes the emitter needs, carried with each traversal so the
// serial grouping never goes back to HBM for a state edge.
struct EAttr {
  float len;
  int32_t seg, seg_pos;
  uint32_t flags;
  int64_t way;
  uint64_t gid;  // segment id / length of e_seg (when seg >= 0)
  float glen;
};

// the edge's K7 record (one 16-byte load): {len bits, seg, seg_pos | flags << 24, way number}
__device__ __forceinline__ uint4 edge_rec(const DevGraph& g, int32_t e) { return g.e_rec[e]; }
__device__ __forceinline__ float rec_len(const uint4& r) { return __uint_as_float(r.x); }
__device__ __forceinline__ int32_t rec_seg(const uint4& r) { return (int32_t)r.y; }
__device__ __forceinline__ int32_t rec_pos(const uint4& r) { return (int32_t)(r.z & 0xFFFFFFu); }
__device__ __forceinline__ uint32_t rec_flags(const uint4& r) { return r.z >> 24; }

__device__ __forceinline__ EAttr edge_attr(const DevGraph& g, int32_t e) {
  const uint4 r = edge_rec(g, e);
  EAttr a;
  a.len = rec_len(r);
  a.seg = rec_seg(r);
  a.seg_pos = a.seg >= 0 ? rec_pos(r) : 0;
  a.flags = rec_flags(r);
  a.way = g.way_tab[r.w];
  a.gid = a.seg >= 0 ? g.g_id[a.seg] : 0ull;
  a.glen = a.seg >= 0 ? g.g_len[a.seg] : 0.0f;
  return a;
}

struct Trav {
  int32_t edge;
  float off0, off1;
  double t0, t1;
  int32_t sh0, sh1;
  EAttr at;
};

template <bool WRITE>
struct SegEmitter {
  DevOut* o;
  int32_t seg_base, way_base;  // write positions (WRITE)
  int32_t nseg = 0, nway = 0;
  // open group
  bool has = false;
  Trav first, last;
  int32_t way_start = 0;
  int64_t last_way = 0;

  __device__ void add_way(const EAttr& at) {
    const int64_t way = at.way;
    if (nway > way_start && last_way == way) return;
    if (WRITE) o->way_ids[way_base + nway] = way;
    last_way = way;
    ++nway;
  }
  __device__ void flush() {
    if (!has) return;
    if (WRITE) {
      otm_segment s;
      const int32_t sg = first.at.seg;
      bool sv, ev;
      s.flags = 0u;
      if (sg >= 0) {
        sv = first.off0 == 0.0f && (first.at.flags & OTM_EDGE_SEG_BEGIN_D);
        ev = last.off1 == last.at.len && (last.at.flags & OTM_EDGE_SEG_END_D);
        s.segment_id = (int64_t)first.at.gid;
        s.length = (sv && ev) ? (int32_t)floor((double)first.at.glen + 0.5) : -1;
      } else {
        sv = first.off0 == 0.0f;
        ev = last.off1 == last.at.len;
        s.segment_id = -1;
        s.length = -1;
        if (first.at.flags & OTM_EDGE_INTERNAL_D) s.flags |= OTM_SEG_INTERNAL;
      }
      s.start_time = 0.0;
      s.end_time = 0.0;
      if (sv) {
        s.flags |= OTM_SEG_START_VALID;
        s.start_time = first.t0;
      }
      if (ev) {
        s.flags |= OTM_SEG_END_VALID;
        s.end_time = last.t1;
      }
      s.queue_length = 0;
      s.begin_shape_index = first.sh0;
      s.end_shape_index = last.sh1;
      s.way_off = way_base + way_start;
      s.way_cnt = nway - way_start;
      s.pad = 0u;
      ((otm_segment*)o->segments)[seg_base + nseg] = s;
      o->seg_gidx[seg_base + nseg] = sg;
    }
    ++nseg;
    has = false;
  }
  __device__ void push(const Trav& t) {
    bool join = false;
    if (has) {
      const int32_t s = t.at.seg, ps = last.at.seg;
      if (s >= 0) join = ps == s && t.at.seg_pos == last.at.seg_pos + 1;
      else join = ps < 0 && ((t.at.flags ^ last.at.flags) & OTM_EDGE_INTERNAL_D) == 0;
    }
    if (!join) {
      flush();
      has = true;
      first = t;
      way_start = nway;
    }
    last = t;
    add_way(t.at);
  }
  static constexpr uint32_t OTM_EDGE_INTERNAL_D = 0x01, OTM_EDGE_SEG_BEGIN_D = 0x02, OTM_EDGE_SEG_END_D = 0x04;
};

__device__ __forceinline__ double time_at(double ta, double tb, float x, float R) {
  if (R > 0.0f) return ta + (tb - ta) * ((double)x / (double)R);
  return ta;
}

// The boundary of step lp -> pl (trace-local points of the trace at a) at
// route distance x (DESIGN.md §3 rule 7, oracle step_bound): the step's
// anchors are lp (position 0), its placed interpolated points (K7a) and pl (R);
// the time is linear between the last anchor before pl at position <= x and
// the anchor after it, the shape index is the last anchor at position <= x.
// Without interpolated points: the two-state rule, bit for bit.
__device__ __forceinline__ void step_bound(const DevBatch& b, const DevWork& w, int64_t a, int lp, int pl, float R,
                                           double ta, double tb, float x, double& t, int& sh) {
  if (pl - lp < 2) {
    t = time_at(ta, tb, x, R);
    sh = x >= R ? pl : lp;
    return;
  }
  int iL = lp, k = lp + 1;
  float xL = 0.0f, xN = R, run = 0.0f;
  double tL = ta, tN = tb;
  for (; k < pl; ++k) {
    const float v = w.ipos[a + k];
    if (!(v >= run)) continue;  // unplaced, or behind an earlier anchor: no anchor
    if (!(v <= x)) break;
    iL = k;
    xL = v;
    tL = b.time[a + k];
    run = v;
  }
  for (; k < pl; ++k) {
    const float v = w.ipos[a + k];
    if (v >= run) {
      xN = v;
      tN = b.time[a + k];
      break;
    }
  }
  sh = R <= x ? pl : iL;
  const float den = xN - xL;
  t = den > 0.0f ? tL + (tN - tL) * ((double)(x - xL) / (double)den) : tL;
}

// Point data of one trace as the emitter reads it: straight from HBM ...
struct SegSrcGlobal {
  const DevGraph* g;
  const DevBatch* b;
  const DevWork* w;
  int64_t a;
  __device__ int state(int pl) const {
    const int64_t p = a + pl;
    return w->is_col[p] ? w->state[p] : -1;
  }
  __device__ bool cs(int pl) const { return w->chain_start[a + pl] != 0; }
  __device__ double time(int pl) const { return b->time[a + pl]; }
  __device__ float rd(int pl) const { return w->route_dist[a + pl]; }
  __device__ int32_t poff(int pl) const { return w->path_off[a + pl]; }
  __device__ int32_t plen(int pl) const { return w->path_len[a + pl]; }
  __device__ int32_t edge(int pl) const { return w->chosen[a + pl].x; }
  __device__ float off(int pl) const { return __int_as_float(w->chosen[a + pl].y); }
  __device__ EAttr attr(int pl) const { return edge_attr(*g, edge(pl)); }
};

// The traversal walk of one trace (one thread): states in order, chains,
// per step the close of the open traversal, the route's path edges and the
// re-open on the new edge; traversals grouped into OSMLR segments.
template <bool WRITE, class Src>
__device__ void segments_trace(const DevGraph& g, const DevWork& w, DevOut& o, int32_t t, int n, int32_t base,
                               const Src& S) {
  SegEmitter<WRITE> em;
  em.o = &o;
  em.seg_base = base;
  em.way_base = base;
  bool open = false;
  int nstate = 0;
  Trav cur{};
  int lastp = -1;
  float curmax = 0.0f;
  for (int p = 0; p <= n; ++p) {
    const int st = p < n ? S.state(p) : -1;
    if (p < n && st < 0) continue;
    const bool new_chain = p == n || S.cs(p);
    if (open && new_chain) {
      cur.off1 = curmax;  // the open traversal's largest state offset (rule 4's stays)
      cur.t1 = S.time(lastp);
      cur.sh1 = lastp;
      if (nstate >= 2) {
        // a chain ending on a node candidate ends at the node: the traversal
        // opened there never left it
        if (!cand_node(cur.off1)) em.push(cur);
        em.flush();
      }
      open = false;
    }
    if (p == n) break;
    const int32_t ej = S.edge(p);
    const float oj = S.off(p);
    if (new_chain) {
      cur.edge = ej;
      cur.at = S.attr(p);
      cur.off0 = oj;
      cur.t0 = S.time(p);
      cur.sh0 = p;
      curmax = oj;
      open = true;
      nstate = 1;
      lastp = p;
      continue;
    }
    const float Rd = S.rd(p);
    const double ta = S.time(lastp), tb = S.time(p);
    const int32_t ca = lastp, cb = p;
    const int32_t ei = cur.edge;
    const float oi = S.off(lastp);
    const bool same = same_edge_step(ei, oi, ej, oj);
    if (!same) {
      // close the traversal on the state's edge, unless the state is a node
      // candidate: its route starts at the node
      const float elen = cur.at.len;  // == e_len[ei]
      const float start = cand_node(oi) ? 0.0f : elen - oi;
      float x = start;
      cur.off1 = elen;
      int sh;
      step_bound(*S.b, w, S.a, ca, cb, Rd, ta, tb, x, cur.t1, sh);
      cur.sh1 = sh;
      if (!cand_node(oi)) em.push(cur);
      float dd = 0.0f;
      const int32_t po = S.poff(p), pl = S.plen(p);
      for (int k = 0; k < pl; ++k) {
        const int32_t pe = w.path_pool[po + k];
        Trav m;
        m.edge = pe;
        m.at = edge_attr(g, pe);
        m.off0 = 0.0f;
        m.off1 = m.at.len;
        const float xb = start + dd;
        dd = dd + m.at.len;
        const float xe = start + dd;
        step_bound(*S.b, w, S.a, ca, cb, Rd, ta, tb, xb, m.t0, sh);
        m.sh0 = sh;
        step_bound(*S.b, w, S.a, ca, cb, Rd, ta, tb, xe, m.t1, sh);
        m.sh1 = sh;
        em.push(m);
      }
      x = start + dd;
      cur.edge = ej;
      cur.at = S.attr(p);
      cur.off0 = 0.0f;
      step_bound(*S.b, w, S.a, ca, cb, Rd, ta, tb, x, cur.t0, sh);
      cur.sh0 = sh;
      curmax = oj;
    } else if (oj > curmax) {
      curmax = oj;
    }
    ++nstate;
    lastp = p;
  }
  o.seg_cnt[t] = em.nseg;
  o.way_cnt[t] = em.nway;
}

// One wavefront per trace, wave-parallel.  The serial walk
// above is a scan in disguise:
//  * the open traversal's edge at every step is the previous state's edge,
//    and it was opened by the latest "opener" state (a chain start, or a step
//    that left the edge) -- a max-scan over the states;
//  * each state emits a known number of traversals (close + route edges when
//    it leaves the edge, + the chain's final close) -- a sum-scan gives each
//    its slot; the lanes then write the traversals in parallel;
//  * a traversal joins its predecessor's group by a test of the two alone --
//    segment and way-id slots are counts of group starts / way changes.
// Float and double expressions are the walk's, in the walk's order (the route
// edges' f32 prefix sum stays sequential per state), so the records are
// bit-identical.  Traces beyond SEGP_PTS points or SEGP_TRAV traversals take
// the serial walk out of global memory (lane 0).
// Two LDS plans: a trace first tries the small one (128 states, 256
// traversals: 13.6 KB, 3 waves per SIMD); one that does not fit goes to a
// list for the large one (256 / 512: 26.6 KB); beyond that, the serial walk.
// Measured on config 2: 0.131 -> 0.111 ms against the large plan alone.
// Diagnostic phase timing of k_segments (a build with -DOTM_SEG_PROF only):
// per wave the clock between the phase boundaries, summed over the launch and
// printed by the launch's last wave for a launch over >= 50k traces.
#ifdef OTM_SEG_PROF
__device__ unsigned long long g_segp[10];
__device__ unsigned int g_segp_done, g_segp_prints;
#define SEGP_DECL unsigned long long segp_acc[9] = {}; long long segp_t = 0; unsigned long long segp_n = 0;
#define SEGP_START { segp_t = clock64(); ++segp_n; }
#define SEGP_MARK(i) { const long long _n = clock64(); segp_acc[i] += (unsigned long long)(_n - segp_t); segp_t = _n; }
#define SEGP_END                                                                                          \
  if (threadIdx.x == 0) {                                                                                 \
    for (int _i = 1; _i <= 8; ++_i) atomicAdd(&g_segp[_i], segp_acc[_i]);                                 \
    atomicAdd(&g_segp[9], segp_n);                                                                        \
    __threadfence();                                                                                      \
    if (atomicAdd(&g_segp_done, 1u) == gridDim.x - 1) {                                                   \
      unsigned long long v[10];                                                                           \
      for (int _i = 1; _i <= 9; ++_i) v[_i] = atomicAdd(&g_segp[_i], 0ull);                               \
      if (nwork >= 5000 && atomicAdd(&g_segp_prints, 1u) < 4)                                            \
        printf("SEGP traces %llu cycles/trace: states %llu scan %llu mark %llu fetch %llu opener %llu "  \
               "trav %llu group %llu record %llu\n", v[9], v[1] / v[9], v[2] / v[9], v[3] / v[9],      \
               v[4] / v[9], v[5] / v[9], v[6] / v[9], v[7] / v[9], v[8] / v[9]);                         \
      for (int _i = 0; _i <= 9; ++_i) atomicExch(&g_segp[_i], 0ull);                                     \
      atomicExch(&g_segp_done, 0u);                                                                       \
    }                                                                                                     \
  }
#else
#define SEGP_DECL
#define SEGP_START
#define SEGP_MARK(i)
#define SEGP_END
#endif

template <int PT, int TR>
struct SegParT {
  double o_t0[PT];  // per state: start time of the traversal it opens
  double t_t0[TR], t_t1[TR];
  float o_off0[PT];
  int32_t tbase[PT + 1];  // first traversal slot of each state
  int32_t t_edge[TR];
  float t_off0[TR], t_off1[TR];
  int16_t sidx[PT + 1];  // point of each state
  int16_t o_sh0[PT];
  int16_t lopen[PT];  // latest opener <= k
  int16_t chain[PT];
  int16_t t_sh0[TR], t_sh1[TR], t_chain[TR];
  int16_t g_first[TR], g_last[TR], g_w0[TR + 1];
  int32_t nt;
};
// small plan: 128 states / 160 traversals (~9.5 KB of LDS, 4 waves per SIMD);
// measured against 256 traversals (13.3 KB, 3 waves): 0.082 -> 0.075 ms on
// config 2, 1.04 -> 0.88 ms on a config-3 shard; 128-192 are within noise
#ifndef OTM_SEGP_TRAV_S
#define OTM_SEGP_TRAV_S 160
#endif
constexpr int SEGP_PTS_S = 128, SEGP_TRAV_S = OTM_SEGP_TRAV_S;
constexpr int SEGP_PTS = 256, SEGP_TRAV = 512;

__device__ __forceinline__ int wave_incl_max(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(v, o, 64);
    if (lane >= o) v = n > v ? n : v;
  }
  return v;
}
// Segmented inclusive max-scan over the wave: a lane with `head` begins a
// segment, and a lane whose segment began before the wave (no head up to it)
// continues from `carry`, the segment's maximum so far -- the caller carries
// lane 63's result to its next 64-point chunk (k_points' OTM_PT_ANCHOR,
// k_traversals' largest offset of the open traversal).  A segment that
// crosses a chunk is in the tests' cases stop_80 (80 interpolated points of
// one step around point 64, every one an anchor) and hand_long_edge (a
// traversal open from point 1 to past point 64, closed at its largest offset).
__device__ __forceinline__ float wave_seg_incl_max(float v, bool head, float carry, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float vn = __shfl_up(v, d, 64);
    const int hn = __shfl_up((int)head, d, 64);
    if (lane >= d) {
      if (!head) v = vn > v ? vn : v;
      head = head || hn != 0;
    }
  }
  if (!head) v = carry > v ? carry : v;
  return v;
}

// what a state contributes (recomputed in the two passes that need it).
// Every global load of a state is issued at once, unconditionally -- none
// depends on another (the neighbours' points come from LDS) -- so a pass
// costs one round trip for them, not three (round 6; the values and the
// arithmetic on them are the same as before).
struct StateStep {
  int32_t pts;     // point (low 16 bits) | previous state's point << 16
  uint32_t f;      // 1 chain start, 2 last state of its chain, 4 a step from lp, 8 stays on the open edge
  int32_t ei, ej;  // previous state's edge (== the open traversal's), own edge
  float oi, oj;
  int32_t plen, poff;
  double ta, tb;   // times of lp and pl
  float rd;        // the step's route distance
  __device__ int pl() const { return pts & 0xFFFF; }
  __device__ int lp() const { return pts >> 16; }
  __device__ bool cs() const { return f & 1u; }
  __device__ bool last() const { return f & 2u; }
  __device__ bool step() const { return f & 4u; }
  __device__ bool same() const { return f & 8u; }
};
template <class SP>
__device__ __forceinline__ StateStep state_step(const DevWork& w, const DevBatch& b, int64_t a, const SP& S, int k,
                                                int ns) {
  StateStep r;
  const int pl = S.sidx[k];
  const int nx = k + 1 < ns ? S.sidx[k + 1] : pl;
  const int pv = k > 0 ? S.sidx[k - 1] : pl;
  const int64_t p = a + pl;
  const bool csp = w.chain_start[p] != 0;
  const bool csn = w.chain_start[a + nx] != 0;
  const int2 cj = w.chosen[p];
  const int2 cv = w.chosen[a + pv];
  const int32_t pln = w.path_len[p], pof = w.path_off[p];
  const double tp = b.time[p], tv = b.time[a + pv];
  r.rd = w.route_dist[p];
  const bool last = k == ns - 1 || csn;
  const bool step = !csp && k > 0;
  const int lp = step ? pv : pl;
  r.pts = pl | (lp << 16);
  r.ej = cj.x;
  r.oj = __int_as_float(cj.y);
  const int2 ci = step ? cv : cj;
  r.ei = ci.x;
  r.oi = __int_as_float(ci.y);
  const bool same = step && same_edge_step(r.ei, r.oi, r.ej, r.oj);
  r.f = (csp ? 1u : 0u) | (last ? 2u : 0u) | (step ? 4u : 0u) | (same ? 8u : 0u);
  const bool leaves = step && !same;
  r.plen = leaves ? (pln > 0 ? pln : 0) : 0;
  r.poff = leaves ? pof : 0;
  r.tb = tp;
  r.ta = step ? tv : tp;
  return r;
}

// list / list_n: the traces to walk (null: all); spill / spill_n: where a
// trace beyond this plan goes (null: the serial walk)
template <int PT, int TR>
__global__ __launch_bounds__(TB, (PT <= 128 ? 4 : 2)) void k_segments(DevGraph g, DevBatch b, DevWork w, DevOut o, const int32_t* list,
                                                 const int32_t* list_n, int32_t* spill, int32_t* spill_n) {
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  __shared__ SegParT<PT, TR> S;
  const int lane = threadIdx.x;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const int32_t nwork = list ? *list_n : b.n_traces;
  SEGP_DECL
  for (int32_t it = blockIdx.x; it < nwork; it += gridDim.x) {
    SEGP_START
    const int32_t t = list ? list[it] : it;
    const int64_t a = b.trace_off[t];
    const int n = (int)(b.trace_off[t + 1] - a);
    const int32_t base = (int32_t)o.seg_base[t];
    if (w.trace_err[t] != 0) {
      if (lane == 0) {
        o.seg_cnt[t] = 0;
        o.way_cnt[t] = 0;
      }
      continue;
    }
    if (n > PT) {
      if (lane == 0) {
        if (spill) {
          tier_wake<TIER_SEG_LARGE>(w);
          spill[atomicAdd(spill_n, 1)] = t;
        } else
          segments_trace<true>(g, w, o, t, n, base, SegSrcGlobal{&g, &b, &w, a});
      }
      continue;
    }
    // ---- states in point order (n <= PT here: every chunk's loads at once)
    constexpr int NCH = (PT + TB - 1) / TB;
    bool stv[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int pl = c * TB + lane;
      const bool in = pl < n;
      const uint8_t ic = in ? w.is_col[a + pl] : (uint8_t)0;
      const int32_t sv = in ? w.state[a + pl] : -1;
      stv[c] = ic && sv >= 0;
    }
    int ns = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const unsigned long long m = __ballot(stv[c]);
      if (stv[c]) S.sidx[ns + __popcll(m & lt)] = (int16_t)(c * TB + lane);
      ns += __popcll(m);
    }
    wave_sync();
    SEGP_MARK(1)
    // every state's loads at once, kept in registers for both passes below
    StateStep rs[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
      if (c * TB + lane < ns) rs[c] = state_step(w, b, a, S, c * TB + lane, ns);
    // ---- per state: chain index, latest opener, slot counts (registers only);
    // the open edge's length of a state that leaves it is loaded here, so its
    // round trip overlaps the scans and the route-edge fetch below
    float elen[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) elen[c] = 0.0f;
    int c_chain = 0, c_open = -1, c_base = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c * TB >= ns) break;
      const int k = c * TB + lane;
      const bool valid = k < ns;
      int cs = 0, opener = -1, nem = 0;
      if (valid) {
        const StateStep& r = rs[c];
        cs = r.cs() ? 1 : 0;
        if (r.cs() || !r.same()) opener = k;
        if (!r.cs() && !r.same()) elen[c] = rec_len(edge_rec(g, r.ei));
        // the close of the open traversal (none from a node candidate), the
        // route's edges, the chain's final close (none at a node candidate)
        nem = (r.step() && !r.same() ? (cand_node(r.oi) ? 0 : 1) + r.plen : 0) +
              (r.last() && !r.cs() && !cand_node(r.oj) ? 1 : 0);
      }
      const int ch = c_chain + wave_incl_scan(cs, lane);
      int lo = wave_incl_max(opener, lane);
      lo = lo > c_open ? lo : c_open;
      const int inc = wave_incl_scan(nem, lane);
      if (valid) {
        S.chain[k] = (int16_t)(ch - 1);
        S.lopen[k] = (int16_t)lo;
        S.tbase[k] = c_base + inc - nem;
      }
      c_chain = __shfl(ch, 63, 64);
      c_open = __shfl(lo, 63, 64);
      c_base += __shfl(inc, 63, 64);
    }
    const int nt = c_base;
    wave_sync();
    SEGP_MARK(2)
    if (nt > TR) {
      if (lane == 0) {
        if (spill) {
          tier_wake<TIER_SEG_LARGE>(w);
          spill[atomicAdd(spill_n, 1)] = t;
        } else
          segments_trace<true>(g, w, o, t, n, base, SegSrcGlobal{&g, &b, &w, a});
      }
      wave_sync();
      continue;
    }
    // ---- the route edges: each state marks its route edges' slots with their
    // pool positions (every other slot -1), then the wave fetches every slot's
    // edge and length at once, a lane a slot -- one round trip for the
    // trace's path edges instead of two per edge along each state's path
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int k = c * TB + lane;
      if (k >= ns) continue;
      const StateStep& r = rs[c];
      int slot = S.tbase[k];
      if (r.step() && !r.same()) {
        if (!cand_node(r.oi)) S.t_edge[slot++] = -1;
        for (int i = 0; i < r.plen; ++i) S.t_edge[slot++] = -2 - (r.poff + i);
      }
      if (r.last() && !r.cs() && !cand_node(r.oj)) S.t_edge[slot] = -1;
    }
    wave_sync();
    SEGP_MARK(3)
    {
      constexpr int NTC = (TR + TB - 1) / TB;
      int32_t pe[NTC];
#pragma unroll
      for (int c = 0; c < NTC; ++c) {
        const int s = c * TB + lane;
        const int32_t v = s < nt ? S.t_edge[s] : -1;
        pe[c] = v <= -2 ? w.path_pool[-2 - v] : -1;
      }
#pragma unroll
      for (int c = 0; c < NTC; ++c) {
        const int s = c * TB + lane;
        if (pe[c] >= 0) {
          S.t_edge[s] = pe[c];
          S.t_off1[s] = rec_len(edge_rec(g, pe[c]));
        }
      }
    }
    wave_sync();
    SEGP_MARK(4)
    // ---- opener fields: a chain start's own, or the re-open on the new edge
    // at the end of the step's route (its length summed in route order)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int k = c * TB + lane;
      if (k >= ns) continue;
      const StateStep& r = rs[c];
      if (r.cs()) {
        S.o_t0[k] = r.tb;
        S.o_off0[k] = r.oj;
        S.o_sh0[k] = (int16_t)r.pl();
      } else if (!r.same()) {
        const float start = cand_node(r.oi) ? 0.0f : elen[c] - r.oi;  // src_start
        const int s0 = S.tbase[k] + (cand_node(r.oi) ? 0 : 1);
        float dd = 0.0f;
        for (int i = 0; i < r.plen; ++i) dd = dd + S.t_off1[s0 + i];
        const float x = start + dd;
        double t0;
        int sh;
        step_bound(b, w, a, r.lp(), r.pl(), r.rd, r.ta, r.tb, x, t0, sh);
        S.o_t0[k] = t0;
        S.o_off0[k] = 0.0f;
        S.o_sh0[k] = (int16_t)sh;
      }
    }
    wave_sync();
    SEGP_MARK(5)
    // ---- traversals, each state writing its own
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int k = c * TB + lane;
      if (k >= ns) continue;
      const StateStep& r = rs[c];
      int slot = S.tbase[k];
      const int16_t chk = S.chain[k];
      if (r.step() && !r.same()) {
        const float Rd = r.rd;
        const double ta = r.ta, tb = r.tb;
        const float el = elen[c];
        const float start = cand_node(r.oi) ? 0.0f : el - r.oi;  // src_start
        if (!cand_node(r.oi)) {
          const int jo = S.lopen[k - 1];
          S.t_edge[slot] = r.ei;
          S.t_off0[slot] = S.o_off0[jo];
          S.t_t0[slot] = S.o_t0[jo];
          S.t_sh0[slot] = S.o_sh0[jo];
          S.t_off1[slot] = el;
          double t1;
          int sh;
          step_bound(b, w, a, r.lp(), r.pl(), Rd, ta, tb, start, t1, sh);
          S.t_t1[slot] = t1;
          S.t_sh1[slot] = (int16_t)sh;
          S.t_chain[slot] = chk;
          ++slot;
        }
        float dd = 0.0f;
        for (int i = 0; i < r.plen; ++i) {
          const float len = S.t_off1[slot];  // (edge and length fetched above)
          const float xb = start + dd;
          dd = dd + len;
          const float xe = start + dd;
          S.t_off0[slot] = 0.0f;
          double tt;
          int sh;
          step_bound(b, w, a, r.lp(), r.pl(), Rd, ta, tb, xb, tt, sh);
          S.t_t0[slot] = tt;
          S.t_sh0[slot] = (int16_t)sh;
          step_bound(b, w, a, r.lp(), r.pl(), Rd, ta, tb, xe, tt, sh);
          S.t_t1[slot] = tt;
          S.t_sh1[slot] = (int16_t)sh;
          S.t_chain[slot] = chk;
          ++slot;
        }
      }
      if (r.last() && !r.cs() && !cand_node(r.oj)) {
        const int jo = S.lopen[k];
        // the traversal ends at the largest offset of its states (the opener
        // jo's and every stay after it: rule 4)
        float omax = r.oj;
        for (int kk = jo; kk < k; ++kk) {
          const float o2 = __int_as_float(w.chosen[a + S.sidx[kk]].y);
          omax = o2 > omax ? o2 : omax;
        }
        S.t_edge[slot] = r.ej;
        S.t_off0[slot] = S.o_off0[jo];
        S.t_t0[slot] = S.o_t0[jo];
        S.t_sh0[slot] = S.o_sh0[jo];
        S.t_off1[slot] = omax;
        S.t_t1[slot] = r.tb;
        S.t_sh1[slot] = (int16_t)r.pl();
        S.t_chain[slot] = chk;
      }
    }
    wave_sync();
    SEGP_MARK(6)
    // ---- groups (OSMLR segments) and way ids
    // (one 16-byte edge record per traversal; ways compared by number, the id
    // looked up only for the way ids written)
    int c_seg = 0, c_way = 0;
    int32_t p_seg = 0, p_pos = 0, p_ch = -1, p_way = -1;
    uint32_t p_fl = 0;
    for (int k0 = 0; k0 < nt; k0 += TB) {
      const int k = k0 + lane;
      const bool valid = k < nt;
      int32_t seg = -1, pos = 0, ch = -2, way = -1;
      uint32_t fl = 0;
      float elk = 0.0f;
      if (valid) {
        const uint4 er = edge_rec(g, S.t_edge[k]);
        elk = rec_len(er);
        seg = rec_seg(er);
        pos = rec_pos(er);
        fl = rec_flags(er);
        way = (int32_t)er.w;
        ch = S.t_chain[k];
      }
      int32_t qs = __shfl_up(seg, 1, 64), qp = __shfl_up(pos, 1, 64), qc = __shfl_up(ch, 1, 64);
      uint32_t qf = __shfl_up(fl, 1, 64);
      int32_t qw = __shfl_up(way, 1, 64);
      if (lane == 0) {
        qs = p_seg;
        qp = p_pos;
        qc = p_ch;
        qf = p_fl;
        qw = p_way;
      }
      bool join = false;
      if (valid && qc == ch) {
        if (seg >= 0) join = qs == seg && pos == qp + 1;
        else join = qs < 0 && ((fl ^ qf) & SegEmitter<true>::OTM_EDGE_INTERNAL_D) == 0;
      }
      const bool start = valid && !join;
      const bool wemit = valid && (start || way != qw);
      const unsigned long long ms = __ballot(start), mw = __ballot(wemit);
      const int gi = c_seg + __popcll(ms & lt) + (start ? 0 : -1);  // this traversal's group
      const int wi = c_way + __popcll(mw & lt);
      if (valid) {
        // what the record pass needs of this traversal's edge, kept in the two
        // slots it no longer reads (its edge and chain): the segment index, and
        // the flags with whether the traversal ends at the edge's end -- no
        // second and third gather of the edge record there
        S.t_edge[k] = seg;
        S.t_chain[k] = (int16_t)(fl | (S.t_off1[k] == elk ? 0x100u : 0u));
      }
      if (wemit) o.way_ids[base + wi] = g.way_tab[way];
      if (start) {
        S.g_first[gi] = (int16_t)k;
        S.g_w0[gi] = (int16_t)wi;
        if (gi > 0) S.g_last[gi - 1] = (int16_t)(k - 1);
      }
      c_seg += __popcll(ms);
      c_way += __popcll(mw);
      p_seg = __shfl(seg, 63, 64);
      p_pos = __shfl(pos, 63, 64);
      p_ch = __shfl(ch, 63, 64);
      p_fl = __shfl(fl, 63, 64);
      p_way = __shfl(way, 63, 64);
    }
    if (lane == 0 && c_seg > 0) {
      S.g_last[c_seg - 1] = (int16_t)(nt - 1);
      S.g_w0[c_seg] = (int16_t)c_way;
    }
    wave_sync();
    SEGP_MARK(7)
    // ---- one record per group (SegEmitter::flush)
    for (int s0 = 0; s0 < c_seg; s0 += TB) {
      const int si = s0 + lane;
      if (si >= c_seg) continue;
      const int kf = S.g_first[si], kl = S.g_last[si];
      EAttr fa;
      fa.seg = S.t_edge[kf];
      fa.flags = (uint32_t)S.t_chain[kf] & 0xFFu;
      fa.gid = fa.seg >= 0 ? g.g_id[fa.seg] : 0ull;
      fa.glen = fa.seg >= 0 ? g.g_len[fa.seg] : 0.0f;
      const uint32_t lfl = (uint32_t)S.t_chain[kl] & 0xFFu;
      const bool lfull = ((uint32_t)S.t_chain[kl] & 0x100u) != 0u;  // t_off1[kl] == the edge's length
      otm_segment sr;
      const int32_t sg = fa.seg;
      bool sv, ev;
      sr.flags = 0u;
      if (sg >= 0) {
        sv = S.t_off0[kf] == 0.0f && (fa.flags & SegEmitter<true>::OTM_EDGE_SEG_BEGIN_D);
        ev = lfull && (lfl & SegEmitter<true>::OTM_EDGE_SEG_END_D);
        sr.segment_id = (int64_t)fa.gid;
        sr.length = (sv && ev) ? (int32_t)floor((double)fa.glen + 0.5) : -1;
      } else {
        sv = S.t_off0[kf] == 0.0f;
        ev = lfull;
        sr.segment_id = -1;
        sr.length = -1;
        if (fa.flags & SegEmitter<true>::OTM_EDGE_INTERNAL_D) sr.flags |= OTM_SEG_INTERNAL;
      }
      sr.start_time = 0.0;
      sr.end_time = 0.0;
      if (sv) {
        sr.flags |= OTM_SEG_START_VALID;
        sr.start_time = S.t_t0[kf];
      }
      if (ev) {
        sr.flags |= OTM_SEG_END_VALID;
        sr.end_time = S.t_t1[kl];
      }
      sr.queue_length = 0;
      sr.begin_shape_index = S.t_sh0[kf];
      sr.end_shape_index = S.t_sh1[kl];
      sr.way_off = base + S.g_w0[si];
      sr.way_cnt = S.g_w0[si + 1] - S.g_w0[si];
      sr.pad = 0u;
      o.segments[base + si] = sr;
      o.seg_gidx[base + si] = sg;
    }
    if (lane == 0) {
      o.seg_cnt[t] = c_seg;
      o.way_cnt[t] = c_way;
    }
    wave_sync();
    SEGP_MARK(8)
  }
  SEGP_END
}

// ============================================================== K7b queue length
// queue_length of one complete OSMLR segment (DESIGN.md §3 rule 7b): the
// intervals between consecutive anchors of a chain (rule 7's anchors: the
// states, and per step the placed interpolated points not behind an earlier
// one) whose first anchor lies in [bsi, esi], walked from the last one
// backwards.  An interval is slow when it covers less than kph x its duration;
// the segment's queue is the trailing run of slow intervals (after at most one
// discharge interval), each clipped to [T0, T1] by time, summed in double in
// walk order.  The walk ends at the first interval that is not slow, so a
// free-flowing segment costs two intervals; a step's anchors are found by the
// forward scan step_bound makes (the monotone filter has no backward form), so
// a step with m interpolated points costs O(m) per anchor taken from it.
// Every read is of the trace's own points [a, a + n).
__device__ int32_t queue_walk(const DevBatch& b, const DevWork& w, int64_t a, int n, int bsi, int esi, double T0,
                              double T1, int32_t length, double kph) {
  auto is_state = [&](int pl) { return w.is_col[a + pl] && w.state[a + pl] >= 0; };
  if (esi > n - 1) esi = n - 1;
  if (bsi < 0) bsi = 0;
  // the last step that can hold a first anchor: q the last state at or before esi, p the state after it
  int q = esi;
  while (q >= 0 && !is_state(q)) --q;
  if (q < 0) return 0;
  int p = q + 1;
  while (p < n && !is_state(p)) ++p;
  int mode = 0;  // 0: no interval yet, 1: after a discharge interval, 2: in the run
  double sum = 0.0;
  bool done = false;
  while (!done && p > bsi) {
    // q -> p is a step unless p starts a chain (or q is the trace's last state)
    if (p < n && !w.chain_start[a + p]) {
      int nx = p;
      float xn = w.route_dist[a + p];
      double tn = b.time[a + p];
      while (nx > q) {
        // the anchor before nx: the last point of (q, nx) at or ahead of every placed one before it, else q
        int pv = q;
        float xp = 0.0f;
        for (int k = q + 1; k < nx; ++k) {
          const float x = w.ipos[a + k];
          if (x >= xp) {
            xp = x;
            pv = k;
          }
        }
        const double tp = b.time[a + pv];
        if (pv < bsi) {
          done = true;
          break;
        }
        if (pv <= esi) {
          double d = (double)xn - (double)xp;
          if (!(d > 0.0)) d = 0.0;
          const double dt = tn - tp;
          const double c = (tn < T1 ? tn : T1) - (tp > T0 ? tp : T0);
          if (c > 0.0) {  // (then dt > 0 too)
            const bool slow = dt > 0.0 && d * 3.6 < kph * dt;
            const double piece = d * (c / dt);
            if (mode == 0) {
              sum = piece;
              mode = slow ? 2 : 1;
            } else if (slow) {
              sum = sum + piece;
              mode = 2;
            } else {
              done = true;
              break;
            }
          }
        }
        nx = pv;
        xn = xp;
        tn = tp;
      }
    }
    p = q;
    --q;
    while (q >= 0 && !is_state(q)) --q;
    if (q < 0) break;
  }
  if (mode != 2) return 0;
  const double r = floor(sum + 0.5);
  return r >= (double)length ? length : (int32_t)r;
}

// One wavefront per trace, a lane per segment of the trace's region (strided
// by the wave for a trace with more segments): each lane reads its record,
// walks its own point range straight out of HBM (neighbouring lanes' ranges
// are adjacent) and overwrites the record's queue_length.  Launched only with
// a threshold; a trace with an error has no segments.
__global__ __launch_bounds__(TB) void k_queue(DevBatch b, DevWork w, DevOut o, float kph) {
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  const int lane = threadIdx.x;
  for (int32_t t = blockIdx.x; t < b.n_traces; t += gridDim.x) {
    if (w.trace_err[t] != 0) continue;
    const int64_t a = b.trace_off[t];
    const int n = (int)(b.trace_off[t + 1] - a);
    const int32_t ns = o.seg_cnt[t];
    otm_segment* SG = o.segments + (int32_t)o.seg_base[t];
    for (int si = lane; si < ns; si += TB) {
      const otm_segment s = SG[si];
      if (s.segment_id < 0 || s.length < 0 || n <= 0) continue;
      SG[si].queue_length =
          queue_walk(b, w, a, n, s.begin_shape_index, s.end_shape_index, s.start_time, s.end_time, s.length, (double)kph);
    }
  }
}

// ============================================================== K8 report
__device__ __forceinline__ bool in_lv(const int64_t* lv, int n, int64_t x) {
  for (int k = 0; k < n; ++k)
    if (lv[k] == x) return true;
  return false;
}

#ifndef OTM_REPORT_WAVES
#define OTM_REPORT_WAVES 1
#endif
// report() launch: a wave per trace over an LDS copy of its segments
// (k_report_wave) up to REPW_MAX_TRACES traces (two rounds of 8 waves per
// SIMD), else a thread per trace (k_report).  Measured: config 2 (10k traces)
// 0.0445 -> 0.0392 ms with the wave form; config 4 (100k traces) 0.106 ->
// 0.290 ms, so it is not used there.
constexpr int32_t REPW_MAX_TRACES = 2 * 8 * 4 * 256;
// report() (py/reporter_service.py:110-215) over one trace's segments, one
// thread per trace.  Segment times are Python values: a segment without
// START_VALID / END_VALID carries the int -1 (what the matcher emits), one
// with it the stored double, an int literal when START_INT / END_INT is set
// (segments handed in by otm_report_segments_device).  A report's t0 / t1
// inherit that int-ness for the JSON writer, and a zero duration raises
// Python's int or float ZeroDivisionError.  The histogram is added in a
// second pass, only for a trace that ends without an error: the reference
// posts nothing for a trace whose report() raised.
// The serial part of report() for trace t over its segments S (global memory,
// or the wave's LDS copy in k_report_wave): the trace result r and the reports
// written to REP, each carrying its reported segment's index in `pad` for the
// histogram pass (which clears it).  Returns the report count; an error trace
// (matcher error or ZeroDivisionError) gets code 500 and no reports.
__device__ int report_walk(int32_t t, const DevBatch& b, const DevReportCfg& rc, const DevWork& w,
                           const otm_segment* S, otm_trace_result& r, otm_report_rec* REP) {
  r.code = 200;
  r.rep_cnt = 0;
  r.shape_used = -1;
  r.successful_count = r.unreported_count = r.discontinuities = r.invalid_speeds = r.unassociated = 0;
  r.successful_length = r.unreported_length = -1;
  if (r.error_kind != 0) {
    r.code = 500;
    return 0;
  }
  const double end_time = b.time[b.trace_off[t + 1] - 1];
  auto ST = [&](const otm_segment& s) { return (s.flags & OTM_SEG_START_VALID) ? s.start_time : -1.0; };
  auto ET = [&](const otm_segment& s) { return (s.flags & OTM_SEG_END_VALID) ? s.end_time : -1.0; };
  auto ST_INT = [&](const otm_segment& s) {
    return !(s.flags & OTM_SEG_START_VALID) || (s.flags & OTM_SEG_START_INT) != 0u;
  };
  auto ET_INT = [&](const otm_segment& s) { return !(s.flags & OTM_SEG_END_VALID) || (s.flags & OTM_SEG_END_INT) != 0u; };
  int last_idx = r.seg_cnt - 1;
  while (last_idx >= 0 && end_time - ST(S[last_idx]) < rc.threshold_sec) --last_idx;
  r.shape_used = last_idx >= 0 ? S[last_idx].begin_shape_index : -1;
  bool have = false, first = true;
  int prior = -1;
  int64_t prior_level = -1;
  int nrep = 0;
  int zerodiv = 0;
  for (int idx = 0; idx <= last_idx; ++idx) {
    const otm_segment& s = S[idx];
    const bool internal = (s.flags & OTM_SEG_INTERNAL) != 0;
    if (idx != 0 && ST(s) == -1.0 && ET(S[idx - 1]) == -1.0) r.discontinuities++;
    const int64_t level = s.segment_id >= 0 ? (s.segment_id & 7) : -1;
    if (have && S[prior].segment_id >= 0 && S[prior].length > 0 && !internal) {
      const otm_segment& ps = S[prior];
      if (in_lv(rc.report_levels, rc.n_report, prior_level)) {
        const bool trans = in_lv(rc.transition_levels, rc.n_transition, level);
        const double t0 = ST(ps);
        const double t1 = trans ? ST(s) : ET(ps);
        const bool t0_int = ST_INT(ps);
        const bool t1_int = trans ? ST_INT(s) : ET_INT(ps);
        const double den = t1 - t0;
        if (den == 0.0) {
          // int / int raises "division by zero", anything else "float division by zero"
          zerodiv = t0_int && t1_int ? OTM_TERR_ZERODIV_INT : OTM_TERR_ZERODIV;
          break;
        }
        const double speed = ((double)ps.length / den) * 3.6;
        if (speed < 200.0) {
          otm_report_rec rep;
          rep.id = ps.segment_id;
          rep.next_id = (trans && s.segment_id >= 0) ? s.segment_id : -1;
          rep.t0 = t0;
          rep.t1 = t1;
          rep.flags = (t1_int ? OTM_REP_T1_INT : 0u) | (t0_int ? OTM_REP_T0_INT : 0u);
          rep.length = ps.length;
          rep.queue_length = ps.queue_length;
          rep.pad = (uint32_t)prior;  // the reported segment, for the histogram pass (cleared there)
          REP[nrep++] = rep;
          r.successful_count++;
          r.successful_length = ps.length;
        } else {
          r.invalid_speeds++;
        }
      } else {
        r.unreported_count++;
        r.unreported_length = ps.length;
      }
    }
    if (!(internal && !first)) {
      prior = idx;
      prior_level = level;
      have = true;
    }
    first = false;
    if (s.segment_id < 0 && !internal) r.unassociated++;
  }
  if (zerodiv) {
    r.code = 500;
    r.error_kind = zerodiv;
    r.shape_used = -1;
    r.successful_count = r.unreported_count = r.discontinuities = r.invalid_speeds = r.unassociated = 0;
    r.successful_length = r.unreported_length = -1;
    return 0;
  }
  return nrep;
}

// The histogram pass over one report: its speed bin and speed sum, for a
// trace that ended without an error (the reference posts nothing for a trace
// whose report() raised); a t1 that is the int -1 of a partial next segment
// gives no speed.  Clears the report's `pad`.
__device__ __forceinline__ void report_hist(const DevOut& o, int32_t seg_off, otm_report_rec& rep) {
  const int32_t ps = (int32_t)rep.pad;
  rep.pad = 0u;
  if (!o.hist) return;
  const double speed = ((double)rep.length / (rep.t1 - rep.t0)) * 3.6;
  const bool t1_minus1 = (rep.flags & OTM_REP_T1_INT) && rep.t1 == -1.0;
  const int32_t gi = o.seg_gidx[seg_off + ps];
  if (t1_minus1 || !(speed >= 0.0) || gi < 0) return;
  int bin = (int)(speed / (double)o.bin_kph);
  bin = bin < 0 ? 0 : (bin >= o.nbins ? o.nbins - 1 : bin);
  atomicAdd(&o.hist[(size_t)gi * o.nbins + bin], 1u);
  if (o.speed_sum) {
    // fixed point (1/1000 km/h) so the sums are exact and order-independent
    atomicAdd(&o.speed_sum[gi], (unsigned long long)(speed * 1000.0 + 0.5));
  }
}

// The pair window's pass over one report (pairs.h), beside report_hist and
// under its conditions: the reported segment's row, and the row of the next
// segment when the report carries a next_id.  report_walk reports segment
// `ps` when it reaches the first segment after it that is not internal, and
// that segment is the next one, so it is found again from `ps` here and the
// report's bytes stay what they were.
__device__ __forceinline__ void report_pair(const DevOut& o, int32_t seg_off, int32_t seg_cnt, int32_t ps,
                                            const otm_report_rec& rep) {
  int32_t gn = -1;
  if (rep.next_id >= 0) {
    const otm_segment* S = o.segments + seg_off;
    int32_t j = ps + 1;
    while (j < seg_cnt && (S[j].flags & OTM_SEG_INTERNAL)) ++j;
    if (j < seg_cnt) gn = o.seg_gidx[seg_off + j];
  }
  pair_report(o.pairs, o.seg_gidx[seg_off + ps], gn, rep.t0, rep.t1, rep.length, rep.queue_length, rep.flags);
}

// the parallel pass over one report: the histogram, then the pair window
__device__ __forceinline__ void report_pass(const DevOut& o, int32_t seg_off, int32_t seg_cnt, otm_report_rec& rep) {
  const int32_t ps = (int32_t)rep.pad;
  report_hist(o, seg_off, rep);
  if (o.pairs.key) report_pair(o, seg_off, seg_cnt, ps, rep);
}

// report() (py/reporter_service.py:110-215), one thread per trace (batches
// of more than REPW_MAX_TRACES traces).
__global__ __launch_bounds__(256, OTM_REPORT_WAVES) void k_report(DevBatch b, DevReportCfg rc, DevWork w, DevOut o, int32_t n_seg_total) {
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= b.n_traces) return;
  otm_trace_result r;
  r.error_kind = w.trace_err[t];
  r.seg_off = (int32_t)o.seg_base[t];
  r.seg_cnt = o.seg_cnt[t];
  r.rep_off = r.seg_off;
  otm_report_rec* REP = o.reports + r.rep_off;
  const int nrep = report_walk(t, b, rc, w, o.segments + r.seg_off, r, REP);
  for (int k = 0; k < nrep; ++k) report_pass(o, r.seg_off, r.seg_cnt, REP[k]);
  r.rep_cnt = nrep;
  if (w.ctr && r.code == 200) {
    cadd(&w.ctr->segments_out, (unsigned long long)r.seg_cnt);
    cadd(&w.ctr->reports_out, (unsigned long long)nrep);
  }
  o.traces[t] = r;
  o.rep_cnt[t] = r.rep_cnt;
}

// report(), one wavefront per trace: the lanes copy the trace's segments into
// LDS with coalesced loads, lane 0 walks them there (the walk is serial: each
// step's global round trip becomes an LDS read), and the lanes run the
// histogram pass over the reports in parallel.  A trace with more segments
// than REPW_CAP is walked out of global memory.
constexpr int REPW_CAP = 64;
__global__ __launch_bounds__(TB) void k_report_wave(DevBatch b, DevReportCfg rc, DevWork w, DevOut o, int32_t n_seg_total) {
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  __shared__ unsigned long long sSeg[REPW_CAP * sizeof(otm_segment) / 8];
  __shared__ int32_t sN;
  static_assert(sizeof(otm_segment) % 8 == 0, "segment words");
  constexpr int SW = (int)(sizeof(otm_segment) / 8);  // 8-byte words per segment
  const int lane = threadIdx.x;
  for (int32_t t = blockIdx.x; t < b.n_traces; t += gridDim.x) {
    otm_trace_result r;
    r.error_kind = w.trace_err[t];
    r.seg_off = (int32_t)o.seg_base[t];
    r.seg_cnt = o.seg_cnt[t];
    r.rep_off = r.seg_off;
    const otm_segment* G = o.segments + r.seg_off;
    otm_report_rec* REP = o.reports + r.rep_off;
    const bool fits = r.seg_cnt <= REPW_CAP;
    if (fits && r.error_kind == 0) {
      const unsigned long long* gw = (const unsigned long long*)G;
      for (int k = lane; k < r.seg_cnt * SW; k += TB) sSeg[k] = gw[k];
    }
    __syncthreads();
    if (lane == 0) {
      const int nrep = report_walk(t, b, rc, w, fits ? (const otm_segment*)sSeg : G, r, REP);
      r.rep_cnt = nrep;
      sN = nrep;
      if (w.ctr && r.code == 200) {
        cadd(&w.ctr->segments_out, (unsigned long long)r.seg_cnt);
        cadd(&w.ctr->reports_out, (unsigned long long)nrep);
      }
      o.traces[t] = r;
      o.rep_cnt[t] = nrep;
      __threadfence_block();  // the reports, for the other lanes' histogram pass
    }
    __syncthreads();
    const int nrep = sN;
    for (int k = lane; k < nrep; k += TB) report_pass(o, r.seg_off, r.seg_cnt, REP[k]);
    __syncthreads();
  }
}

// ============================================================== segment bound / compaction
// K7a, interpolated points (DESIGN.md §3 rule 7, oracle interp_pos): a point
// k between the two states q < k < p of a step that leaves its edge is placed
// on the step's route -- on each route piece (the rest of q's edge, the path's
// edges, p's edge up to p) its best projection onto the piece's edge,
// admissible inside the piece, costed sqdist / (2 sigma_z^2) + |pos - gc(q, k)|
// / beta; the cheapest wins (-1: none).  One thread per interpolated point
// (its step from prevc / nextc); the monotone filter (a point behind the
// step's running maximum is no anchor) is applied where the anchors are read
// (step_bound).
struct RoutePiece {
  int32_t edge;
  float o0, o1, xs;
};
// Where rule 7 puts point k: its position along the step's route (-1: none),
// the winning piece's edge and the admissible foot's offset on it (edge -1:
// none) -- the place the position names, xs + (off - o0).  One loop, tie rule
// and set of f32 expressions for both users; each keeps only what it takes:
// K7a the position (FOOT false; edge and off stay unset), rule 7c the edge and
// offset (FOOT true; pos stays unset), so K7a's path gets no store.
struct RoutePlace {
  float pos;
  int32_t edge;
  float off;
};
template <bool FOOT>
__device__ __forceinline__ RoutePlace place_on_route(const DevGraph& g, const DevBatch& b, const DevParams& P,
                                                     const DevWork& w, int64_t q, int64_t p, int64_t k) {
  const int2 ci = w.chosen[q], cj = w.chosen[p];
  const int32_t ei = ci.x, ej = cj.x;
  const float oi = __int_as_float(ci.y), oj = __int_as_float(cj.y);
  const int32_t poff = w.path_off[p], plen = w.path_len[p];
  const bool has0 = !cand_node(oi);
  const int npc = (has0 ? 1 : 0) + plen + (cand_node(oj) ? 0 : 1);
  const float start = src_start(g, ei, oi);
  const float ds = (2.0f * P.sigma_z) * P.sigma_z;
  const float lat = b.lat[k], lon = b.lon[k];
  const float ls = MPD_F * cos_deg(lat);
  const float gcd = gc_dist(b.lat[q], b.lon[q], lat, lon);
  float best = INFINITY, bpos = -1.0f, dd = 0.0f, bo = 0.0f;
  int32_t be = -1;
  for (int m = 0; m < npc; ++m) {
    RoutePiece pc;
    const int pk = m - (has0 ? 1 : 0);
    // the piece's edge record first: its length and its segments in one load
    const bool mid = !(has0 && m == 0) && pk < plen;
    const int32_t e = has0 && m == 0 ? ei : (mid ? w.path_pool[poff + pk] : ej);
    const int4 er = g.e_proj[e];
    const float len = __int_as_float(er.z);
    if (has0 && m == 0) {
      pc = RoutePiece{e, oi, len, 0.0f};
    } else if (mid) {
      pc = RoutePiece{e, 0.0f, len, start + dd};
      dd = dd + len;
    } else {
      pc = RoutePiece{e, 0.0f, oj, start + dd};
    }
    float bsq, boff;
    project_edge(g, er, lat, lon, ls, bsq, boff);
    if (!(boff >= pc.o0 && boff <= pc.o1)) continue;
    const float pos = pc.xs + (boff - pc.o0);
    const float cost = bsq / ds + fabsf(pos - gcd) / P.beta;
    if (cost < best) {  // (strict: of equal pieces the earliest wins)
      best = cost;
      if constexpr (FOOT) {
        be = pc.edge;
        bo = boff;
      } else {
        bpos = pos;
      }
    }
  }
  return RoutePlace{bpos, be, bo};
}

// The step q -> p around interpolated point k, if there is one: linked, not a
// chain start, matched, with a route.  The caller tests trace_err.
__device__ __forceinline__ bool interp_step(const DevWork& w, int64_t k, int32_t& q, int32_t& p) {
  q = w.prevc[k];
  p = q >= 0 ? w.nextc[q] : -1;
  return p >= 0 && w.col_prev[p] == q && !w.chain_start[p] && w.state[p] >= 0 && w.path_len[p] >= 0;
}

// Traversals a matched point can add: the close of the open traversal, its
// route's path edges, the re-open (+ the chain's final close): <= 2 + path.
// Summed per trace into tb[t] (scanned over traces into DevOut::seg_base): a
// wave's points are runs of whole traces, so a segmented suffix sum over the
// wave leaves each run's total on its first lane, which adds it with one
// atomic -- no per-point bound array, no point-length scan (round 6).  An
// interpolated point's thread places it instead (K7a).  Measured against a
// wave per trace (coalesced runs, no atomics): 0.027 vs 0.032 ms on config 2,
// 0.067 vs 0.064 on config 4; and against each trace's region taken from one
// cursor by k_segments (no bound pass at all): k_segments 0.047 -> 0.142 ms on
// config 2, the one address's atomics serialised (profiles/r06/k7/).
__global__ __launch_bounds__(256) void k_seg_bound(DevGraph g, DevBatch b, DevParams P, DevWork w, int64_t* tb) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // spill snapshot C: steps per route tier (kept for the status read)
  if (k == b.n_points) fold_snap(w, SNAP_AFTER_ROUTE, false);
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  const int lane = threadIdx.x & 63;
  int64_t v = 0;
  int32_t t = -1;
  if (k < b.n_points) {
    t = w.pt_trace[k];
    if (w.is_col[k]) {
      if (w.state[k] >= 0) {
        const int32_t pl = w.path_len[k];
        v = 2 + (pl > 0 ? pl : 0);
      }
    } else {
      // the step q -> p around this point, where it leaves q's edge
      int32_t q, p;
      if (interp_step(w, k, q, p) && w.trace_err[t] == 0) {
        const int2 ci = w.chosen[q], cj = w.chosen[p];
        if (!same_edge_step(ci.x, __int_as_float(ci.y), cj.x, __int_as_float(cj.y)))
          w.ipos[k] = place_on_route<false>(g, b, P, w, q, p, k).pos;
      }
    }
  }
  // segmented suffix sum over the wave's runs of equal t (lanes past the
  // batch's end have t = -1, a run of their own)
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int64_t vn = __shfl_down(v, d, 64);
    const int32_t tn = __shfl_down(t, d, 64);
    if (lane + d < 64 && tn == t) v += vn;
  }
  const int32_t tp = __shfl_up(t, 1, 64);
  if (t >= 0 && (lane == 0 || tp != t) && v != 0) atomicAdd((unsigned long long*)&tb[t], (unsigned long long)v);
}

// One wavefront per trace: copy its segments (way offsets rebased), way ids
// and reports from the trace's region to the dense arrays, and its result
// record with the dense offsets to `to` (the regions' records stay as they
// are, so fetching a batch twice gives the same arrays).
__global__ __launch_bounds__(TB) void k_compact(int32_t n_traces, DevOut o, const int32_t* seg_off, const int32_t* way_off,
                                                const int32_t* rep_off, otm_segment* so, int64_t* wo,
                                                otm_report_rec* ro, otm_trace_result* to) {
  const int lane = threadIdx.x;
  const otm_trace_result* TR = o.traces;
  const otm_segment* SI = o.segments;
  const otm_report_rec* RI = o.reports;
  for (int32_t t = blockIdx.x; t < n_traces; t += gridDim.x) {
    const int32_t base = TR[t].seg_off;  // the region start k_report recorded
    const int32_t ns = o.seg_cnt[t], nw = o.way_cnt[t], nr = o.rep_cnt[t];
    const int32_t ds = seg_off[t], dw = way_off[t], dr = rep_off[t];
    for (int k = lane; k < ns; k += TB) {
      otm_segment x = SI[base + k];
      x.way_off = x.way_off - base + dw;
      so[ds + k] = x;
    }
    for (int k = lane; k < nw; k += TB) wo[dw + k] = o.way_ids[base + k];
    for (int k = lane; k < nr; k += TB) ro[dr + k] = RI[base + k];
    if (lane == 0) {
      otm_trace_result x = TR[t];
      x.seg_off = ds;
      x.rep_off = dr;
      to[t] = x;
    }
  }
}

// One block of 1024 threads: the three count arrays' exclusive scans, totals
// at o*[n].  (Round 4's form summed a contiguous chunk per thread: strided,
// uncoalesced loads, ~90 us per 10k traces with other batches in flight.)
__global__ __launch_bounds__(1024) void k_fetch_scan(int32_t n, const int32_t* c0, const int32_t* c1,
                                                     const int32_t* c2, int32_t* o0, int32_t* o1, int32_t* o2) {
  // tiles of 1024 consecutive counts (coalesced loads and stores), each tile
  // scanned in the block and added to the running carry
  __shared__ int32_t ws[3][16];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int carry0 = 0, carry1 = 0, carry2 = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + t;
    const int s0 = i < n ? c0[i] : 0, s1 = i < n ? c1[i] : 0, s2 = i < n ? c2[i] : 0;
    // inclusive scans within the wave, then across the 16 waves
    int i0 = s0, i1 = s1, i2 = s2;
    for (int o = 1; o < 64; o <<= 1) {
      const int x0 = __shfl_up(i0, o, 64), x1 = __shfl_up(i1, o, 64), x2 = __shfl_up(i2, o, 64);
      if (lane >= o) {
        i0 += x0;
        i1 += x1;
        i2 += x2;
      }
    }
    if (lane == 63) {
      ws[0][wv] = i0;
      ws[1][wv] = i1;
      ws[2][wv] = i2;
    }
    __syncthreads();
    int b0 = 0, b1 = 0, b2 = 0, z0 = 0, z1 = 0, z2 = 0;
    for (int k = 0; k < 16; ++k) {
      const int w0 = ws[0][k], w1 = ws[1][k], w2 = ws[2][k];
      if (k < wv) {
        b0 += w0;
        b1 += w1;
        b2 += w2;
      }
      z0 += w0;
      z1 += w1;
      z2 += w2;
    }
    if (i < n) {
      o0[i] = carry0 + b0 + i0 - s0;
      o1[i] = carry1 + b1 + i1 - s1;
      o2[i] = carry2 + b2 + i2 - s2;
    }
    carry0 += z0;
    carry1 += z1;
    carry2 += z2;
    __syncthreads();  // (ws is rewritten by the next tile)
  }
  if (t == 0) {
    o0[n] = carry0;
    o1[n] = carry1;
    o2[n] = carry2;
  }
}

// ============================================================== K7c matched points
// (after the pipeline's other kernels in this file, so that the code object lays those out as it did without it)
// The closest foot of point k on the whole of edge e (rule 7c, same-edge
// steps): every shape segment, ties to the lowest, clamped into [lo, hi].
__device__ float edge_foot(const DevGraph& g, const DevBatch& b, int32_t e, int64_t k, float lo, float hi) {
  const float lat = b.lat[k], lon = b.lon[k];
  const float ls = MPD_F * cos_deg(lat);
  float bsq, boff;
  project_edge(g, g.e_proj[e], lat, lon, ls, bsq, boff);
  return boff < lo ? lo : (boff > hi ? hi : boff);
}

// One wavefront per trace, lanes over its points in chunks of 64 (k_queue's
// shape); one 40-byte record per point, in input point order whatever the
// launch plan.  A column with a state copies its chosen candidate; an
// interpolated point finds its step from prevc / nextc as K7a does and, placed
// (ipos >= 0), recomputes the winning piece's foot, or, in a same-edge step,
// takes its clamped foot on the edge.  OTM_PT_ANCHOR needs the running maximum
// of ipos over the step's earlier points: a segmented inclusive max-scan over
// the wave (segments begin at columns, unplaced points count as -1), the
// maximum carried from chunk to chunk for a step's run that crosses one -- no
// lane walks its step.  Then per lane: the edge record, the walk over the
// edge's cumulative lengths to the offset's shape segment, the coordinate and
// the distance in double, and the record's store.  Every read of a per-point
// array is of the trace's own points [a, a + n).
__global__ __launch_bounds__(TB) void k_points(DevGraph g, DevBatch b, DevParams P, DevWork w,
                                               otm_matched_point* out) {
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  const int lane = threadIdx.x;
  for (int32_t t = blockIdx.x; t < b.n_traces; t += gridDim.x) {
    const int64_t a = b.trace_off[t];
    const int n = (int)(b.trace_off[t + 1] - a);
    const bool ok = w.trace_err[t] == 0;
    float carry = -1.0f;  // the open step's maximum at the end of the previous chunk
    for (int c0 = 0; c0 < n; c0 += TB) {
      const int pl = c0 + lane;
      const bool in = pl < n;
      const int64_t k = a + pl;
      bool col = false;
      uint32_t flags = 0;
      int32_t edge = -1;
      float off = 0.0f, x = -1.0f;
      if (in) {
        col = w.is_col[k] != 0;
        if (col) {
          flags = OTM_PT_COLUMN;
          if (ok && w.state[k] >= 0) {
            const int2 c = w.chosen[k];
            edge = c.x;
            off = __int_as_float(c.y);
            flags |= OTM_PT_MATCHED | (cand_node(off) ? OTM_PT_NODE : 0u) | (w.chain_start[k] ? OTM_PT_CHAIN_START : 0u);
          }
        } else if (ok) {
          int32_t q, p;
          if (interp_step(w, k, q, p)) {
            const int2 ci = w.chosen[q], cj = w.chosen[p];
            const float oi = __int_as_float(ci.y), oj = __int_as_float(cj.y);
            if (same_edge_step(ci.x, oi, cj.x, oj)) {
              edge = ci.x;
              off = edge_foot(g, b, edge, k, oi < oj ? oi : oj, oi < oj ? oj : oi);
              flags = OTM_PT_MATCHED | OTM_PT_SAME_EDGE;
            } else {
              x = w.ipos[k];
              if (x >= 0.0f) {
                const RoutePlace f = place_on_route<true>(g, b, P, w, q, p, k);
                edge = f.edge;
                off = f.off;
                flags = OTM_PT_MATCHED | OTM_PT_ROUTE;
              } else {
                x = -1.0f;
              }
            }
          }
        }
      }
      // the step's running maximum of x: a column (or a lane past the trace) starts a segment
      const float v = wave_seg_incl_max(x, col || !in, carry, lane);
      carry = __shfl(v, 63, 64);
      if ((flags & OTM_PT_ROUTE) && x >= v) flags |= OTM_PT_ANCHOR;
      if (!in) continue;
      otm_matched_point r;
      r.edge = -1;
      r.flags = flags;
      r.lat = 0.0;
      r.lon = 0.0;
      r.offset = 0.0f;
      r.distance = 0.0f;
      r.way_id = 0;
      const bool placed = (flags & OTM_PT_MATCHED) && edge >= 0;
      const int32_t s0 = placed ? g.e_shape_off[edge] : 0;
      const int32_t nsh = placed ? g.e_shape_off[edge + 1] - s0 - 1 : 0;
      if (nsh >= 1) {  // (every edge of a graph file has a shape segment)
        const uint4 er = g.e_rec[edge];
        // the lowest shape segment with off <= cum[s + 1] (the last one when rounding left none)
        int sg = 0;
        float c1 = g.s_cum[s0 + 1];
        while (sg + 1 < nsh && !(off <= c1)) {
          ++sg;
          c1 = g.s_cum[s0 + sg + 1];
        }
        const double c0d = (double)g.s_cum[s0 + sg], c1d = (double)c1;
        const double tt = c1d == c0d ? 0.0 : ((double)off - c0d) / (c1d - c0d);
        const double la0 = (double)g.s_lat[s0 + sg], lo0 = (double)g.s_lon[s0 + sg];
        r.lat = la0 + tt * ((double)g.s_lat[s0 + sg + 1] - la0);
        r.lon = lo0 + tt * ((double)g.s_lon[s0 + sg + 1] - lo0);
        const double plat = (double)b.lat[k], plon = (double)b.lon[k];
        const double ls = 111319.4954833 * cos(plat * 0.017453292519943295);
        const double dx = (r.lon - plon) * ls, dy = (r.lat - plat) * 111319.4954833;
        r.distance = (float)sqrt(dx * dx + dy * dy);
        r.edge = edge;
        r.offset = off;
        r.way_id = g.way_tab[er.w];
      } else {
        r.flags = flags & OTM_PT_COLUMN;  // no place: a column keeps its flag alone
      }
      out[k] = r;
    }
  }
}

// ============================================================== K7d matched route
// (after K7c, for the same reason: the code object lays the timed kernels out as it did without it)
// What SegEmitter::push compares of two consecutive traversals' edges.
struct TvAttr {
  int32_t seg, pos;
  uint32_t fl;
};
__device__ __forceinline__ TvAttr tv_attr(const DevGraph& g, int32_t e) {
  const uint4 r = edge_rec(g, e);
  return TvAttr{rec_seg(r), rec_pos(r), rec_flags(r)};
}
// SegEmitter::push's join test: c behind p, both of one chain
__device__ __forceinline__ bool tv_join(const TvAttr& p, const TvAttr& c) {
  if (c.seg >= 0) return p.seg == c.seg && c.pos == p.pos + 1;
  return p.seg < 0 && ((c.fl ^ p.fl) & SegEmitter<true>::OTM_EDGE_INTERNAL_D) == 0;
}
// one record into the trace's region reg[cap] (a slot past the bound is dropped, never written)
__device__ __forceinline__ void tv_store(otm_traversal* reg, int32_t slot, int32_t cap, int32_t edge, const EAttr& at,
                                         uint32_t flags, float off0, float off1, double t0, double t1, int sh0, int sh1,
                                         int grp) {
  if (slot >= cap) return;
  otm_traversal r;
  r.edge = edge;
  r.flags = flags | (off0 == 0.0f ? OTM_TV_FROM_START : 0u) | (off1 == at.len ? OTM_TV_TO_END : 0u) |
            (at.seg < 0 && (at.flags & SegEmitter<true>::OTM_EDGE_INTERNAL_D) ? OTM_TV_INTERNAL : 0u);
  r.begin_offset = off0;
  r.end_offset = off1;
  r.enter_time = t0;
  r.exit_time = t1;
  r.begin_shape_index = sh0;
  r.end_shape_index = sh1;
  r.segment = grp;
  r.pad = 0;
  r.way_id = at.way;
  reg[slot] = r;
}

// One wavefront per trace, lanes over its points in chunks of 64, plus one
// virtual point behind the last (segments_trace's p == n): rule 7d's records,
// the Trav values segments_trace hands to SegEmitter::push, in that order, into
// the trace's region at seg_base[t] (k_seg_bound's bound is one on traversals)
// and their number into cnt[t].  The walk as scans over the wave, every carry
// going forward so that a trace of any length takes this one form:
//  * a lane's previous state: an exclusive max-scan of the states' points;
//  * the open traversal before a lane: the latest opener (a chain start, or a
//    step that left its edge) -- a max-scan of the openers' lanes, its t0 / sh0 /
//    off0 read from that lane, or from the carry when it lies in an earlier
//    chunk; its largest offset: a segmented max-scan of the states' offsets,
//    the openers its heads;
//  * a lane emits: a step that leaves its edge the close of the open traversal
//    (none from a node candidate) and its path edges; a chain start and the
//    virtual point the final close of the chain before them (>= 2 states, not
//    at a node) -- so nothing looks ahead; a sum-scan gives the slots;
//  * `segment` is a sum-scan of group starts: a lane counts the starts inside
//    its own run, and its first record is tested against the last record of
//    the latest emitting lane before it (or the carry).
// Times and shape indices are step_bound's at the walk's x (start, start + dd,
// the path edges' f32 lengths summed in path order), so they are the bits
// k_segments used.  OTM_TV_CHAIN_END needs the record after: k_trav_compact
// sets it.  Every read of a per-point array is of the trace's own points.
__global__ __launch_bounds__(TB) void k_traversals(DevGraph g, DevBatch b, DevWork w, DevOut o, DevTrav tv) {
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  const int lane = threadIdx.x;
  for (int32_t t = blockIdx.x; t < b.n_traces; t += gridDim.x) {
    const int64_t a = b.trace_off[t];
    const int n = (int)(b.trace_off[t + 1] - a);
    const int64_t rb = o.seg_base[t];
    const int32_t cap = (int32_t)(o.seg_base[t + 1] - rb);
    otm_traversal* reg = tv.rec + rb;
    if (w.trace_err[t] != 0) {
      if (lane == 0) tv.cnt[t] = 0;
      continue;
    }
    // carried from chunk to chunk: the last state's point and whether it began
    // a chain, the chains begun, the open traversal's fields and largest
    // offset, the slot and group cursors, the last record's attributes and chain
    int c_lastp = -1, c_lastcs = 1, c_chain = 0, c_slot = 0, c_grp = 0, c_sh0 = 0, c_pch = -1;
    double c_t0 = 0.0;
    float c_off0 = 0.0f, c_max = 0.0f;
    TvAttr c_pa{-1, 0, 0u};
    for (int c0 = 0; c0 <= n; c0 += TB) {
      const int pl = c0 + lane;
      const bool in = pl < n, virt = pl == n;
      const int64_t k = a + pl;
      const bool isst = in && w.is_col[k] != 0 && w.state[k] >= 0;
      // ---- the previous state, chains
      int lpi = wave_incl_max(isst ? pl : -1, lane);
      lpi = lpi > c_lastp ? lpi : c_lastp;
      int lp = __shfl_up(lpi, 1, 64);
      if (lane == 0) lp = c_lastp;
      const bool cs = isst ? (w.chain_start[k] != 0 || lp < 0) : virt;
      int pcs = __shfl((int)cs, (lp - c0) & 63, 64);  // whether the previous state began its chain
      if (lp < c0) pcs = c_lastcs;
      const int ch = c_chain + wave_incl_scan(cs ? 1 : 0, lane);
      int32_t ei = -1, ej = -1;
      float oi = 0.0f, oj = 0.0f;
      if (isst) {
        const int2 cj = w.chosen[k];
        ej = cj.x;
        oj = __int_as_float(cj.y);
      }
      if ((isst || virt) && lp >= 0) {
        const int2 ci = w.chosen[a + lp];
        ei = ci.x;  // the open traversal's edge
        oi = __int_as_float(ci.y);
      }
      const bool step = isst && !cs;
      const bool leaves = step && !same_edge_step(ei, oi, ej, oj);
      const bool opener = isst && (cs || leaves);
      // ---- a leaving step's route: its length in route order, its first and last
      // records' attributes and the group starts between them; the re-open on the new edge
      int nem = 0, plen = 0, poff = 0, inner = 0, my_sh0 = pl;
      float start = 0.0f, Rd = 0.0f, my_off0 = oj;
      double ta = 0.0, tb = 0.0, my_t0 = 0.0;
      bool hasclose = false;
      TvAttr fa{-1, 0, 0u}, la{-1, 0, 0u};
      if (isst && cs) my_t0 = b.time[k];
      if (leaves) {
        const int32_t pln = w.path_len[k];
        plen = pln > 0 ? pln : 0;
        poff = w.path_off[k];
        Rd = w.route_dist[k];
        ta = b.time[a + lp];
        tb = b.time[k];
        start = src_start(g, ei, oi);
        hasclose = !cand_node(oi);
        bool have = hasclose;
        if (hasclose) fa = la = tv_attr(g, ei);
        float dd = 0.0f;
        for (int i = 0; i < plen; ++i) {
          const uint4 er = edge_rec(g, w.path_pool[poff + i]);
          const TvAttr c{rec_seg(er), rec_pos(er), rec_flags(er)};
          dd = dd + rec_len(er);
          if (!have) fa = c;
          else if (!tv_join(la, c)) ++inner;
          have = true;
          la = c;
        }
        int sh;
        step_bound(b, w, a, lp, pl, Rd, ta, tb, start + dd, my_t0, sh);
        my_sh0 = sh;
        my_off0 = 0.0f;
        nem = (hasclose ? 1 : 0) + plen;
      }
      // ---- the open traversal before this lane
      const int loi = wave_incl_max(opener ? lane : -1, lane);
      int lox = __shfl_up(loi, 1, 64);
      if (lane == 0) lox = -1;
      double x_t0 = __shfl(my_t0, lox & 63, 64);
      float x_off0 = __shfl(my_off0, lox & 63, 64);
      int x_sh0 = __shfl(my_sh0, lox & 63, 64);
      if (lox < 0) {
        x_t0 = c_t0;
        x_off0 = c_off0;
        x_sh0 = c_sh0;
      }
      const float v = wave_seg_incl_max(isst ? oj : -1.0f, opener, c_max, lane);
      float cmx = __shfl_up(v, 1, 64);  // the open traversal's largest offset before this lane
      if (lane == 0) cmx = c_max;
      // ---- the final close of the chain that ends before this lane
      const bool fin = (isst || virt) && cs && lp >= 0 && !pcs && !cand_node(cmx);
      if (fin) {
        fa = la = tv_attr(g, ei);
        nem = 1;
      }
      const int rch = fin ? ch - 1 : ch;  // the chain of this lane's records
      // ---- slots, the record before, groups
      const int inc = wave_incl_scan(nem, lane);
      const int slot = c_slot + inc - nem;
      const int lei = wave_incl_max(nem > 0 ? lane : -1, lane);
      int lex = __shfl_up(lei, 1, 64);
      if (lane == 0) lex = -1;
      TvAttr pa;
      pa.seg = __shfl(la.seg, lex & 63, 64);
      pa.pos = __shfl(la.pos, lex & 63, 64);
      pa.fl = (uint32_t)__shfl((int)la.fl, lex & 63, 64);
      int pch = __shfl(rch, lex & 63, 64);
      if (lex < 0) {
        pa = c_pa;
        pch = c_pch;
      }
      const bool newchain = nem > 0 && pch != rch;
      const bool fstart = nem > 0 && (newchain || !tv_join(pa, fa));
      const int gs = nem > 0 ? inner + (fstart ? 1 : 0) : 0;
      const int ginc = wave_incl_scan(gs, lane);
      int gi = c_grp + ginc - gs - 1;  // the group of the record before this lane's first
      // ---- the carries
      {
        const int lo63 = __shfl(loi, 63, 64), le63 = __shfl(lei, 63, 64);
        const double n_t0 = __shfl(my_t0, lo63 & 63, 64);
        const float n_off0 = __shfl(my_off0, lo63 & 63, 64);
        const int n_sh0 = __shfl(my_sh0, lo63 & 63, 64);
        if (lo63 >= 0) {
          c_t0 = n_t0;
          c_off0 = n_off0;
          c_sh0 = n_sh0;
        }
        const int n_seg = __shfl(la.seg, le63 & 63, 64), n_pos = __shfl(la.pos, le63 & 63, 64);
        const int n_fl = __shfl((int)la.fl, le63 & 63, 64), n_ch = __shfl(rch, le63 & 63, 64);
        if (le63 >= 0) {
          c_pa = TvAttr{n_seg, n_pos, (uint32_t)n_fl};
          c_pch = n_ch;
        }
        c_max = __shfl(v, 63, 64);
        const int np = __shfl(lpi, 63, 64);
        const int ncs = __shfl((int)cs, (np - c0) & 63, 64);
        if (np >= c0) c_lastcs = ncs;
        c_lastp = np;
        c_chain = __shfl(ch, 63, 64);
        c_slot += __shfl(inc, 63, 64);
        c_grp += __shfl(ginc, 63, 64);
      }
      // ---- the records
      if (fin) {
        gi += fstart ? 1 : 0;
        tv_store(reg, slot, cap, ei, edge_attr(g, ei), (newchain ? OTM_TV_CHAIN_START : 0u) | (fstart ? OTM_TV_SEGMENT_FIRST : 0u),
                 x_off0, cmx, x_t0, b.time[a + lp], x_sh0, lp, gi);
      } else if (leaves) {
        int s = slot;
        bool first = true;
        TvAttr pv = pa;
        if (hasclose) {
          const EAttr at = edge_attr(g, ei);
          double t1;
          int sh;
          step_bound(b, w, a, lp, pl, Rd, ta, tb, start, t1, sh);
          gi += fstart ? 1 : 0;
          tv_store(reg, s++, cap, ei, at, (newchain ? OTM_TV_CHAIN_START : 0u) | (fstart ? OTM_TV_SEGMENT_FIRST : 0u), x_off0,
                   at.len, x_t0, t1, x_sh0, sh, gi);
          pv = TvAttr{at.seg, at.seg_pos, at.flags};
          first = false;
        }
        float dd = 0.0f;
        for (int i = 0; i < plen; ++i) {
          const int32_t pe = w.path_pool[poff + i];
          const EAttr at = edge_attr(g, pe);
          const TvAttr c{at.seg, at.seg_pos, at.flags};
          const bool st = first ? fstart : !tv_join(pv, c);
          const uint32_t fl = (first && newchain ? OTM_TV_CHAIN_START : 0u) | (st ? OTM_TV_SEGMENT_FIRST : 0u);
          gi += st ? 1 : 0;
          const float xb = start + dd;
          dd = dd + at.len;
          const float xe = start + dd;
          double t0, t1;
          int sh0, sh1;
          step_bound(b, w, a, lp, pl, Rd, ta, tb, xb, t0, sh0);
          step_bound(b, w, a, lp, pl, Rd, ta, tb, xe, t1, sh1);
          tv_store(reg, s++, cap, pe, at, fl, 0.0f, at.len, t0, t1, sh0, sh1, gi);
          pv = c;
          first = false;
        }
      }
    }
    if (lane == 0) tv.cnt[t] = c_slot < cap ? c_slot : cap;
  }
}

// One wavefront per trace: its records from the region to the dense array at
// off[t] (off: the exclusive scan of k_traversals' counts), OTM_TV_CHAIN_END set
// on a record whose successor starts a chain or does not exist.  The region's
// records stay as they are, so a second compaction gives the same bytes.
__global__ __launch_bounds__(TB) void k_trav_compact(int32_t n_traces, const int64_t* seg_base, const int64_t* off,
                                                     const otm_traversal* reg, otm_traversal* dst) {
  const int lane = threadIdx.x;
  for (int32_t t = blockIdx.x; t < n_traces; t += gridDim.x) {
    const int64_t rb = seg_base[t], d = off[t];
    const int n = (int)(off[t + 1] - d);
    for (int k = lane; k < n; k += TB) {
      otm_traversal x = reg[rb + k];
      if (k + 1 == n || (reg[rb + k + 1].flags & OTM_TV_CHAIN_START)) x.flags |= OTM_TV_CHAIN_END;
      dst[d + k] = x;
    }
  }
}

// ============================================================== K7e match scores
// (after K7d, for the same reason as K7c)
// DESIGN.md §3 rule 7e: min-sum forward-backward over the chains K5 decoded.
// One row of G lanes per trace, lane j = state j: G = 64 is the general form
// (one wave per trace, columns up to KMAX wide, any length), G = 16 the packed
// form (one trace per DPP row, four per wave; a trace with a scored column
// wider than 16 or with more than SC_ROW_PTS points goes to `rej`, which the
// general form drains in list mode).  Two sweeps over the trace's points:
//  * forward: alpha as K5 formed it -- em at a chain's first column, else
//    (min_i (alpha_q(i) + T[i][j])) + em -- kept in the row's registers from
//    column to column and written to the scratch (sc.alpha / sc.alpha_x);
//  * backward, from the trace's last point: beta of the later column stays in
//    registers as g(j) = em(j) + beta(j); beta_q(i) = min_j (T[i][j] + g(j));
//    m = alpha + beta; the minimum over j != s with its lowest index by a row
//    butterfly; lane 0 of the row writes the record.
// The minima are exact, so the order of their operands does not matter; each
// sum is the one rule 7e writes.  Terms are costs (>= +0, +inf included): no
// NaN arises.  A broadcast of state i is a DPP row_newbcast operand of the add
// in the packed form and a readlane in the general one; DPP reads of a lane
// that EXEC has switched off do not return its value, so, as in
// k_viterbi_row, both sweeps run with every lane enabled under wave-uniform
// control flow and mask by selects: a lane past a column's count holds +inf.
// Which columns are scored, and where chains start, is read from trace_err
// (as K6 left it: the kernel is launched after route recovery), K5's state
// and chain_start: a linked column's previous scored column is its col_prev,
// the scored column before it in the trace (k_viterbi links no other).
// Every load is inside its array: a block's floats at [trans_off[p],
// trans_off[p] + Kq * Kp), a point's slots below its count.
constexpr int SC_ROW_PTS = 128;  // packed form: points per trace (a longer trace would idle its wave's other rows)
template <int G, int I>
__device__ __forceinline__ float sc_bcast(float v) {
  if constexpr (G == 16)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + I, 0xF, 0xF, false));
  else
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), I));
}
// I0 .. I0 + 3 of min_i (bcast_i(x) + tv[i]), guarded wave-uniformly by kmax
template <int G, int KM, int I0>
__device__ __forceinline__ void sc_min4(const float x, const float (&tv)[KM], const int kmax, float& best) {
  if (I0 < kmax) {
    const float v0 = sc_bcast<G, I0 + 0>(x) + tv[I0 + 0];
    const float v1 = sc_bcast<G, I0 + 1>(x) + tv[I0 + 1];
    const float v2 = sc_bcast<G, I0 + 2>(x) + tv[I0 + 2];
    const float v3 = sc_bcast<G, I0 + 3>(x) + tv[I0 + 3];
    best = fminf(best, fminf(fminf(v0, v1), fminf(v2, v3)));
  }
}
template <int G, int KM>
__device__ __forceinline__ float sc_min(const float x, const float (&tv)[KM], const int kmax) {
  float best = INFINITY;
  sc_min4<G, KM, 0>(x, tv, kmax, best);
  sc_min4<G, KM, 4>(x, tv, kmax, best);
  sc_min4<G, KM, 8>(x, tv, kmax, best);
  sc_min4<G, KM, 12>(x, tv, kmax, best);
  if constexpr (KM > 16) {
    sc_min4<G, KM, 16>(x, tv, kmax, best);
    sc_min4<G, KM, 20>(x, tv, kmax, best);
    sc_min4<G, KM, 24>(x, tv, kmax, best);
    sc_min4<G, KM, 28>(x, tv, kmax, best);
  }
  return best;
}
__device__ __forceinline__ float* sc_alpha(const DevScores& sc, int64_t p, int j) {
  return j < KIN ? sc.alpha + p * KIN + j : sc.alpha_x + p * KX + (j - KIN);
}
__device__ __forceinline__ void sc_store(otm_point_score* r, float cost, float margin, float chain_cost, float em,
                                         float tr, int32_t alt_edge, int32_t alt_off_bits, uint32_t tail) {
  uint4* q = (uint4*)r;
  q[0] = make_uint4(fbits(cost), fbits(margin), fbits(chain_cost), fbits(em));
  q[1] = make_uint4(fbits(tr), (uint32_t)alt_edge, (uint32_t)alt_off_bits, tail);
}
template <int G>
__global__ __launch_bounds__(TB) void k_scores(DevBatch b, DevWork w, DevScores sc, const int32_t* list,
                                               const int32_t* list_n, int32_t* rej, int32_t* rej_n) {
  constexpr int NT = TB / G, KM = G == 16 ? 16 : KMAX;
  static_assert(G == 16 || G == 64, "a DPP row or a wave per trace");
  static_assert(sizeof(otm_point_score) == 32, "two 16-byte stores a record");
  if (*w.abort) return;  // a capacity was exceeded: the host redoes the batch
  const int lane = threadIdx.x;
  const int g = lane / G, j = lane % G, gb = g * G;
  const unsigned long long rowmask = G == 64 ? ~0ull : 0xFFFFull;
  const int32_t nwork = list ? *list_n : b.n_traces;
  for (int32_t tb0 = blockIdx.x * NT; tb0 < nwork; tb0 += gridDim.x * NT) {
    const int32_t it = tb0 + g;
    bool act = it < nwork;
    const int32_t t = act ? (list ? list[it] : it) : 0;
    int64_t a = 0;
    int n = 0;
    if (act) {
      a = b.trace_off[t];
      n = (int)(b.trace_off[t + 1] - a);
    }
    // ---- the records of the points without a score, row-parallel: every point
    // of a trace answered 500 -- K5 leaves such a trace without a state when
    // the error came before it, but route recovery (K6) can fail a trace whose
    // columns have states -- and, in the others, every point without a state;
    // the packed form also looks for what it cannot take
    const bool err = act && w.trace_err[t] != 0;
    bool wide = false;
    for (int pl = j; pl < n; pl += G) {
      const int32_t st = w.state[a + pl];
      if (err || st < 0)
        sc_store(sc.rec + a + pl, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1, 0, 0xFF000000u);
      else
        wide = wide || w.ncand[a + pl] > KM;
    }
    if (err) act = false;  // whole: nothing to sweep, nothing for the list
    if (rej) {
      const bool out = act && (n > SC_ROW_PTS || ((__ballot(wide) >> gb) & rowmask) != 0ull);
      if (out) {
        if (j == 0) rej[atomicAdd(rej_n, 1)] = t;
        act = false;
      }
    }
    if (!act) n = 0;
    const int nmax = __builtin_amdgcn_readfirstlane(wave_max_i(n));
    // A chunk of G points' words, one point a lane, loaded together and handed
    // to the row by shuffle at each step, so a step's own loads (emissions,
    // alpha, its block) do not wait for them: scored << 6 | chain start << 7 |
    // state << 8 | candidates, and the point's block offset.  A point past
    // the trace's end, of an idle row or without a state has word 0.
    auto chunk_words = [&](int c0, int& mw, int64_t& to) {
      const int pl = c0 + j;
      const int64_t p = a + (pl < n ? pl : 0);
      const int32_t st = w.state[p];
      const int32_t nc = w.ncand[p];
      const uint8_t cs = w.chain_start[p];
      to = w.trans_off[p];
      mw = pl < n && st >= 0 ? (nc & 0x3F) | 0x40 | (cs ? 0x80 : 0) | (st << 8) : 0;
    };
    auto word_of = [&](int mw, int64_t to, int k, int& mk, int64_t& tk) {
      mk = __shfl(mw, gb + k, 64);
      const int lo = __shfl((int)(uint32_t)to, gb + k, 64), hi = __shfl((int)(to >> 32), gb + k, 64);
      tk = (int64_t)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
    };
    // ---- forward: alpha into the scratch
    {
      float prev = INFINITY;
      int lastK = 0;
      for (int c0 = 0; c0 < nmax; c0 += G) {
        int mw;
        int64_t tw;
        chunk_words(c0, mw, tw);
        const int kend = nmax - c0 < G ? nmax - c0 : G;
        for (int k = 0; k < kend; ++k) {
          int mk;
          int64_t to;
          word_of(mw, tw, k, mk, to);
          const bool col = (mk & 0x40) != 0;
          if (__ballot(col) == 0ull) continue;
          const int64_t p = a + (col ? c0 + k : 0);
          const int Kp = col ? mk & 0x3F : 0;
          const bool link = col && !(mk & 0x80);
          const float emv = cemis(w, p, j < Kp ? j : 0);  // (slot 0 of a point is always there)
          const float em = j < Kp ? emv : INFINITY;
          const int Kq = link ? lastK : 0;
          const int kmax = __builtin_amdgcn_readfirstlane(wave_max_i(Kq));
          // the block's column j, every load issued before the first is used: a
          // lane or source outside the block reads the allocation's first float
          // instead (always there) and drops it
          const bool inb = link && j < Kp;
          const float* const tp = w.trans + (inb ? to + j : 0);
          const int ts = inb ? Kp : 0;
          float tv[KM];
#pragma unroll
          for (int i = 0; i < KM; ++i) tv[i] = INFINITY;
#pragma unroll
          for (int i = 0; i < KM; ++i)
            if (i < kmax) tv[i] = tp[(i < Kq ? i : 0) * ts];
#pragma unroll
          for (int i = 0; i < KM; ++i)
            if (i < kmax) tv[i] = inb && i < Kq ? tv[i] : INFINITY;
          const float best = sc_min<G, KM>(prev, tv, kmax);
          const float cur = link ? best + em : em;
          if (j < Kp) *sc_alpha(sc, p, j) = cur;
          prev = col ? cur : prev;
          lastK = col ? Kp : lastK;
        }
      }
    }
    // ---- backward: beta, the through-costs, the records.  A record's second
    // half holds the step's own cost T[state[q]][s], which needs the earlier
    // column's state: lane 0 keeps that half until the walk reaches q.
    {
      float g2 = INFINITY;  // em + beta of the later column of the chain
      int K2 = 0, s2 = 0;
      int64_t to2 = 0, p2 = 0;
      bool have = false;    // a later column links to the one at hand
      float ccost = 0.0f;
      int2 alt2 = make_int2(-1, 0);
      uint32_t tail2 = 0;
      for (int c0 = ((nmax - 1) / G) * G; c0 >= 0 && nmax > 0; c0 -= G) {
        int mw;
        int64_t tw;
        chunk_words(c0, mw, tw);
        const int kend = nmax - c0 < G ? nmax - c0 : G;
        for (int k = kend - 1; k >= 0; --k) {
          int mk;
          int64_t to;
          word_of(mw, tw, k, mk, to);
          const bool col = (mk & 0x40) != 0;
          if (__ballot(col) == 0ull) continue;
          const int64_t p = a + (col ? c0 + k : 0);
          const int st = (mk >> 8) & 0xFF;
          const int Kp = col ? mk & 0x3F : 0;
          const bool cs = col && (mk & 0x80);
          const float emv = cemis(w, p, j < Kp ? j : 0), alv = *sc_alpha(sc, p, j < Kp ? j : 0);
          const float em = j < Kp ? emv : INFINITY;
          const float al = j < Kp ? alv : INFINITY;
          const bool lk = col && have;
          const int K2L = lk ? K2 : 0;
          // the later column's record, whole now: its step came from this column's state
          if (lk && j == 0) {
            const float tr = w.trans[to2 + (int64_t)st * K2L + s2];
            ((uint4*)(sc.rec + p2))[1] = make_uint4(fbits(tr), (uint32_t)alt2.x, (uint32_t)alt2.y, tail2);
          }
          const int kmax = __builtin_amdgcn_readfirstlane(wave_max_i(K2L));
          // the later column's block, row j (loads as in the forward sweep)
          const bool inb = lk && j < Kp;
          const float* const tp = w.trans + (inb ? to2 + (int64_t)j * K2L : 0);
          float tv[KM];
#pragma unroll
          for (int i = 0; i < KM; ++i) tv[i] = INFINITY;
#pragma unroll
          for (int i = 0; i < KM; ++i)
            if (i < kmax) tv[i] = tp[inb && i < K2L ? i : 0];
#pragma unroll
          for (int i = 0; i < KM; ++i)
            if (i < kmax) tv[i] = inb && i < K2L ? tv[i] : INFINITY;
          const float bmin = sc_min<G, KM>(g2, tv, kmax);
          const float beta = lk ? bmin : 0.0f;
          const bool end = col && !have;
          const float m = al + beta;  // (+inf past Kp: al is)
          // a chain's cost: Viterbi's own minimum, at its last column
          float cc = al;
#pragma unroll
          for (int o = G / 2; o > 0; o >>= 1) cc = fminf(cc, __shfl_xor(cc, o, G));
          ccost = end ? cc : ccost;
          const float ms = __shfl(m, gb + (col ? st : 0), 64);
          const float ems = __shfl(em, gb + (col ? st : 0), 64);
          // the runner-up: (value, state) minimum over j != s, ties to the lower state
          float bv = col && j < Kp && j != st ? m : INFINITY;
          int bi = j;
#pragma unroll
          for (int o = G / 2; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, G);
            const int oi = __shfl_xor(bi, o, G);
            if (ov < bv || (ov == bv && oi < bi)) {
              bv = ov;
              bi = oi;
            }
          }
          if (col && j == 0) {
            const bool alone = !(bv < INFINITY);
            const float d = bv - ms;
            const float margin = alone ? INFINITY : (d > 0.0f ? d : 0.0f);
            alt2 = alone ? make_int2(-1, 0) : crec(w, p, bi);
            const uint32_t fl = OTM_SC_SCORED | (cs ? OTM_SC_CHAIN_START : 0u) | (end ? OTM_SC_CHAIN_END : 0u) |
                                (alone ? OTM_SC_ALONE : 0u) | (margin == 0.0f ? OTM_SC_TIE : 0u);
            tail2 = fl | ((uint32_t)Kp << 8) | ((uint32_t)(st & 0xFF) << 16) |
                    ((uint32_t)((alone ? -1 : bi) & 0xFF) << 24);
            uint4* q = (uint4*)(sc.rec + p);
            q[0] = make_uint4(fbits(ms), fbits(margin), fbits(ccost), fbits(ems));
            // a chain's first column has no step of its own
            if (cs) q[1] = make_uint4(0u, (uint32_t)alt2.x, (uint32_t)alt2.y, tail2);
          }
          g2 = col ? em + beta : g2;
          K2 = col ? Kp : K2;
          s2 = col ? st : s2;
          to2 = col ? to : to2;
          p2 = col ? p : p2;
          have = col ? !cs : have;
        }
      }
      // (K5 starts every chain with a chain start: no half is left over; were one, its step cost is 0)
      if (have && j == 0) ((uint4*)(sc.rec + p2))[1] = make_uint4(0u, (uint32_t)alt2.x, (uint32_t)alt2.y, tail2);
    }
  }
}

// ============================================================== K7f matched shape
// (after K7e, for the same reason: the code object lays the timed kernels out as it did without it)
// Rule 7c's Coordinate at `off` on an edge with shape points s0 .. s0 + nsh: k_points' expression,
// operand for operand (the lowest shape segment with off <= cum[s + 1], t and the point in double).  Kept apart
// from k_points: with one function called from both, k_points' assembly came out different.
__device__ __forceinline__ void shape_coord(const DevGraph& g, int32_t s0, int32_t nsh, float off, double& lat,
                                            double& lon) {
  lat = lon = 0.0;
  if (nsh < 1) return;  // (every edge of a graph file has a shape segment)
  int sg = 0;
  float c1 = g.s_cum[s0 + 1];
  while (sg + 1 < nsh && !(off <= c1)) {
    ++sg;
    c1 = g.s_cum[s0 + sg + 1];
  }
  const double c0d = (double)g.s_cum[s0 + sg], c1d = (double)c1;
  const double tt = c1d == c0d ? 0.0 : ((double)off - c0d) / (c1d - c0d);
  const double la0 = (double)g.s_lat[s0 + sg], lo0 = (double)g.s_lon[s0 + sg];
  lat = la0 + tt * ((double)g.s_lat[s0 + sg + 1] - la0);
  lon = lo0 + tt * ((double)g.s_lon[s0 + sg + 1] - lo0);
}
// one polyline value's chars (n of them: 1 + floor(log2(v | 1)) / 5) at d
__device__ __forceinline__ char* shape_put(char* d, uint32_t v, int n) {
  for (int i = 0; i < n; ++i) {
    const uint32_t q = v & 31u;
    v >>= 5;
    *d++ = (char)((q | (i + 1 < n ? 0x20u : 0u)) + 63u);
  }
  return d;
}

// One wavefront per trace, over its rule-7d records as k_traversals left them
// in the trace's region, 64 at a time.  A record lane reads its record's edge,
// flags and two offsets and the edge's shape range, finds the interior shape
// points (those with begin_offset < cum < end_offset: one contiguous index
// range, found in one walk of at most 14 cum values) and so its vertex count;
// a sum-scan gives its first vertex, the carry going forward from chunk to
// chunk.  Then the lanes turn to the chunk's output vertices, 64 at a time: a
// lane finds its vertex's record by a 6-step search over the scanned counts,
// makes the vertex (an end: the Coordinate; an interior point: the shape point
// itself), quantises it, takes the vertex before it from the lane below (lane
// 0: the carry; the trace's first: (0, 0)), and forms the two zigzag values and
// their char counts; a second sum-scan gives its byte position.
// WRITE false stores the trace's vertex and byte counts; WRITE true stores the
// vertices (8 bytes a lane, consecutive), the spans from the record lanes and
// the chars, each lane's at its own position, all at the scanned offsets and
// never past the trace's own extent.  Every load is of the trace's own region
// and of an edge's own shape range.
template <bool WRITE>
__global__ __launch_bounds__(TB) void k_shape(DevGraph g, int32_t n_traces, const int64_t* seg_base, DevTrav tv,
                                              DevShape sh) {
  const int lane = threadIdx.x;
  for (int32_t t = blockIdx.x; t < n_traces; t += gridDim.x) {
    const otm_traversal* reg = tv.rec + seg_base[t];
    const int n = (int)tv.cnt[t];
    int64_t vb = 0, vcap = 0, pb = 0, pcap = 0, sb = 0;
    if (WRITE) {
      vb = sh.vtx_off[t];
      vcap = sh.vtx_off[t + 1] - vb;
      pb = sh.poly_off[t];
      pcap = sh.poly_off[t + 1] - pb;
      sb = sh.trav_off[t];
    }
    // carried from chunk to chunk: the vertices and bytes so far, the last vertex
    int64_t c_v = 0, c_b = 0;
    int c_lat = 0, c_lon = 0;
    for (int c0 = 0; c0 < n; c0 += TB) {
      const int r = c0 + lane;
      const bool in = r < n;
      int32_t s0 = 0, m = 0, i0 = 1, nint = 0;
      float bo = 0.0f, zo = 0.0f;
      bool cs = false;
      if (in) {
        const otm_traversal* q = reg + r;
        const int32_t e = q->edge;
        cs = (q->flags & OTM_TV_CHAIN_START) != 0;
        bo = q->begin_offset;
        zo = q->end_offset;
        s0 = g.e_shape_off[e];
        m = g.e_shape_off[e + 1] - s0 - 1;
        int i1 = 1;
        for (int i = 1; i < m; ++i) {
          const float c = g.s_cum[s0 + i];
          if (!(bo < c)) {
            i0 = i1 = i + 1;
            continue;
          }
          if (!(c < zo)) break;
          i1 = i + 1;
        }
        nint = i1 - i0;
      }
      const int nv = in ? (cs ? 1 : 0) + nint + 1 : 0;
      const int incl = wave_incl_scan(nv, lane);
      const int excl = incl - nv;
      const int total = __shfl(incl, 63, 64);
      if (WRITE && in) {
        // (a record that starts no chain shares its first vertex with the record before)
        const int32_t bv = (int32_t)(c_v + excl) - (cs ? 0 : 1), ev = (int32_t)(c_v + incl) - 1;
        ((int2*)sh.span)[sb + r] = make_int2(bv, ev);
      }
      for (int v0 = 0; v0 < total; v0 += TB) {
        const int j = v0 + lane;
        const bool act = j < total;
        // the owning record: the lowest one whose scanned count exceeds j
        int own = 0;
#pragma unroll
        for (int step = 32; step; step >>= 1) {
          const int val = __shfl(incl, own + step - 1, 64);
          if (val <= j) own += step;
        }
        const int o_s0 = __shfl(s0, own, 64), o_m = __shfl(m, own, 64), o_i0 = __shfl(i0, own, 64);
        const int o_nint = __shfl(nint, own, 64), o_ex = __shfl(excl, own, 64), o_cs = __shfl((int)cs, own, 64);
        const float o_b = __shfl(bo, own, 64), o_z = __shfl(zo, own, 64);
        int qlat = 0, qlon = 0;
        if (act) {
          int k = j - o_ex;
          double la, lo;
          if (o_cs && k == 0) {
            shape_coord(g, o_s0, o_m, o_b, la, lo);
          } else {
            k -= o_cs;
            if (k < o_nint) {
              la = (double)g.s_lat[o_s0 + o_i0 + k];
              lo = (double)g.s_lon[o_s0 + o_i0 + k];
            } else {
              shape_coord(g, o_s0, o_m, o_z, la, lo);
            }
          }
          qlat = (int32_t)rint(la * 1e6);
          qlon = (int32_t)rint(lo * 1e6);
        }
        int plat = __shfl_up(qlat, 1, 64), plon = __shfl_up(qlon, 1, 64);
        if (lane == 0) {
          plat = c_lat;
          plon = c_lon;
        }
        const int dla = qlat - plat, dlo = qlon - plon;
        const uint32_t za = ((uint32_t)dla << 1) ^ (uint32_t)(dla >> 31);
        const uint32_t zb = ((uint32_t)dlo << 1) ^ (uint32_t)(dlo >> 31);
        const int na = 1 + (31 - __clz((int)(za | 1u))) / 5, nb = 1 + (31 - __clz((int)(zb | 1u))) / 5;
        const int nby = act ? na + nb : 0;
        const int binc = wave_incl_scan(nby, lane);
        if (WRITE && act) {
          const int64_t vi = c_v + j, bp = c_b + binc - nby;
          if (vi < vcap) ((int2*)sh.vtx)[vb + vi] = make_int2(qlat, qlon);
          if (bp + nby <= pcap) shape_put(shape_put(sh.poly + pb + bp, za, na), zb, nb);
        }
        const int last = (total - v0 < TB ? total - v0 : TB) - 1;
        c_lat = __shfl(qlat, last, 64);
        c_lon = __shfl(qlon, last, 64);
        c_b += __shfl(binc, 63, 64);
      }
      c_v += total;
    }
    if (!WRITE && lane == 0) {
      sh.vtx_off[t] = c_v;
      sh.poly_off[t] = c_b;
    }
  }
}

int grid_for(int64_t n, int per_block, int cap) {
  int64_t g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (int)(g > cap ? cap : g);
}

// ============================================================== launchers
constexpr int WAVE_GRID_CAP = 256 * 64;  // grid-stride cap for wave kernels
#ifndef OTM_TRANS_GRID_CAP
#define OTM_TRANS_GRID_CAP 65536
#endif
constexpr int TRANS_GRID_CAP = OTM_TRANS_GRID_CAP;  // k_trans_sub waves (one per column, grid-striding beyond)

}  // namespace

void launch_fetch_scan(int32_t n, const int32_t* c0, const int32_t* c1, const int32_t* c2, int32_t* o0, int32_t* o1,
                       int32_t* o2, hipStream_t s) {
  hipLaunchKernelGGL(k_fetch_scan, dim3(1), dim3(1024), 0, s, n, c0, c1, c2, o0, o1, o2);
}


const char* const kKernelNames[KN_COUNT] = {
    "k_columns",       "spatial_order",  "k_cand_lane",    "k_candidates",     "k_links",         "scan_trans_off",  "k_trans_sub",
    "k_trans_wide",    "k_transitions",  "k_transitions_big", "k_viterbi",      "k_route_index",
    "k_route",         "k_route_big",    "k_seg_bound",      "scan_seg_bound",  "k_segments",       "k_report"};

namespace {
// The spill tiers run on lists the previous tier filled on the device; they
// read the list length themselves (fixed grids, no host round trip) and exit
// at once when the list is empty.
constexpr int SPILL_GRID = 4096;
#ifndef OTM_WIDE_GRID
#define OTM_WIDE_GRID 8192
#endif
// k_trans_sub's wide-column pass (grid-strides over its list): 8192 waves
// (eight per SIMD) rather than 2048: config 2 0.035 -> 0.030 ms (round 6)
constexpr int WIDE_GRID = OTM_WIDE_GRID;
}  // namespace

#define TIMED(k, launch) \
  do {                   \
    mk.begin(k, s);      \
    launch;              \
    mk.count();          \
    mk.end(k, s);        \
  } while (0)

void launch_columns(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, int64_t* seg_base,
                    hipStream_t s, const Marks& mk) {
  // (the tile counts are zero: k_order_plan left them so)
  TIMED(KN_COLUMNS, hipLaunchKernelGGL(k_columns, dim3(grid_for(b.n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, g,
                                       b, p, w, seg_base));
}
// grid for a kernel over the spatial order: a multiple of ORDER_GROUPS, with
// 25 % headroom per group over an even split
static int order_grid(int64_t n, int per_block, int cap) {
  const int64_t per_group = (n + ORDER_GROUPS - 1) / ORDER_GROUPS;
  int64_t gb = (per_group + per_group / 4 + per_block - 1) / per_block;
  if (gb < 1) gb = 1;
  int64_t gtot = gb * ORDER_GROUPS;
  if (gtot > cap) gtot = cap / ORDER_GROUPS * ORDER_GROUPS;
  return (int)gtot;
}

void launch_order(const DevBatch& b, DevWork& w, hipStream_t s, const Marks& mk) {
  // (the tile counts were made by K1)
  mk.begin(KN_ORDER, s);
  hipLaunchKernelGGL(k_order_plan, dim3(1), dim3(1024), 0, s, w.ord.tile_cnt, w.ord.cursor, w.ord.grp);
  hipLaunchKernelGGL(k_order_scatter, dim3(grid_for(b.n_points, 256, 8192)), dim3(256), 0, s, b, w, w.ord.tile,
                     w.ord.cursor, w.ord.item);
  mk.count(2);
  mk.end(KN_ORDER, s);
}

void launch_candidates(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, hipStream_t s,
                       const Marks& mk, int from) {
  // (the work counters in their own instance: their registers cost the
  // uncounted one entries in flight)
  if (from < RESUME_CAND_BIG) {
    if (w.ctr)
      TIMED(KN_CAND_LANE, hipLaunchKernelGGL(k_cand_lane<true>, dim3(order_grid(b.n_points, CAND_TB, 1 << 30)),
                                             dim3(CAND_TB), 0, s, g, b, p, w));
    else
      TIMED(KN_CAND_LANE, hipLaunchKernelGGL(k_cand_lane<false>, dim3(order_grid(b.n_points, CAND_TB, 1 << 30)),
                                             dim3(CAND_TB), 0, s, g, b, p, w));
  }
  mk.begin(KN_CAND_WAVE, s);
  // (a fixed 4096 waves, each walking two or three of config 2's ~10k spilled
  // probes in a row.  Not kept: the grid sized from the batch, a wave per
  // expected spilled probe (n_points / 64 between 256 and 16384: 15,625 waves
  // at 1M points) -- 37.7 against 36.0 us on config 2, 8.5 against 7.8 on
  // config 4, profiles/graph_words/kernels.json build "c"; and again with the
  // scan on ent_geo and the snap on the packed records: 2,048 waves 54.8 us,
  // 8,192 waves 34.2 - 34.5, 4,096 waves 33.8, profiles/proj_records/)
#ifndef OTM_CAND_WAVE_GRID
#define OTM_CAND_WAVE_GRID 4096
#endif
  if (from < RESUME_CAND_BIG) {
    hipLaunchKernelGGL(k_candidates<false>, dim3(OTM_CAND_WAVE_GRID), dim3(TB), 0, s, g, b, p, w);
    mk.count();
  }
  if (!(w.dormant & TIER_CAND_BIG)) {  // (on demand: kernels.h TierGroup)
    hipLaunchKernelGGL(k_candidates<true>, dim3(CAND_BIG_SLOTS), dim3(TB), 0, s, g, b, p, w);
    mk.count();
  }
  mk.end(KN_CAND_WAVE, s);
}
void launch_links(const DevBatch& b, const DevParams& p, DevWork& w, hipStream_t s, const Marks& mk) {
  TIMED(KN_LINKS, hipLaunchKernelGGL(k_links, dim3(grid_for(b.n_points + 1, 256, 1 << 30)), dim3(256), 0, s, b, p,
                                     w));
}
// The compact host batch (otm_match_compact) widened on the device: a wave per
// trace, its points' time = base + delta (whole seconds, exact in a double)
// and accuracy as float -- the arrays every stage reads.
__global__ __launch_bounds__(256) void k_expand_compact(const int64_t* trace_off, const int64_t* tbase,
                                                        const int32_t* dt, const int16_t* acc16, double* time,
                                                        float* acc, int32_t n_traces) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t t = (int64_t)blockIdx.x * 4 + wv; t < n_traces; t += (int64_t)gridDim.x * 4) {
    const int64_t a = trace_off[t], e = trace_off[t + 1], base = tbase[t];
    for (int64_t i = a + lane; i < e; i += 64) {
      time[i] = (double)(base + (int64_t)dt[i]);
      acc[i] = (float)acc16[i];
    }
  }
}
void launch_expand_compact(const int64_t* trace_off, const int64_t* tbase, const int32_t* dt, const int16_t* acc16,
                           double* time, float* acc, int32_t n_traces, hipStream_t s) {
  if (n_traces <= 0) return;
  hipLaunchKernelGGL(k_expand_compact, dim3(grid_for(((int64_t)n_traces + 3) / 4, 1, 1 << 20)), dim3(256), 0, s,
                     trace_off, tbase, dt, acc16, time, acc, n_traces);
}
void launch_status(const int32_t* abort, const int64_t* ttotal, const int32_t* counters, const int32_t* snap,
                   BatchStatus* out, BatchStatus* host, hipStream_t s) {
  hipLaunchKernelGGL(k_status, dim3(1), dim3(64), 0, s, abort, ttotal, counters, snap, out, host);
}
void launch_transitions(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, hipStream_t s,
                        const Marks& mk, int sub, int from) {
  if (from >= RESUME_TRANS_HUGE) {
    // the tiers below the huge one kept their matrices: the huge tier alone
    mk.begin(KN_TRANS_GLOBAL, s);
    hipLaunchKernelGGL(k_transitions<2>, dim3(HUGE_SLOTS), dim3(TB), 0, s, g, b, p, w);
    mk.count();
    mk.end(KN_TRANS_GLOBAL, s);
    return;
  }
  // many more waves than fit at once (each column is a few dependent
  // round trips): measured 0.78 ms at 16K waves, 0.67 ms at 64K; a grid of
  // one resident round was slowest (0.92 ms, partial rounds at 7 waves/SIMD)
  // sub: lanes per column (engine trans_lanes)
  const int per = TB / sub;  // columns per wave step
  const int grid = order_grid((b.n_points + per - 1) / per, 1, TRANS_GRID_CAP);
  if (sub == 8) {
    // 8 lanes per column over the columns of <= OTM_TRANS_KC8 candidates a
    // side, then 16 lanes over the wide rest (a list filled on the device)
    TIMED(KN_TRANS_INDEX, hipLaunchKernelGGL((k_trans_sub<8, false>), dim3(grid), dim3(TB), 0, s, g, b, p, w));
    TIMED(KN_TRANS_WIDE, hipLaunchKernelGGL((k_trans_sub<16, true>), dim3(WIDE_GRID), dim3(TB), 0, s, g, b, p, w));
  } else {
    TIMED(KN_TRANS_INDEX, hipLaunchKernelGGL((k_trans_sub<16, false>), dim3(grid), dim3(TB), 0, s, g, b, p, w));
    mk.skip(KN_TRANS_WIDE, s);
  }
  if (w.dormant & TIER_TRANS_ONLINE) {  // (on demand: kernels.h TierGroup)
    mk.skip(KN_TRANS_WAVE, s);
    mk.skip(KN_TRANS_GLOBAL, s);
    return;
  }
  TIMED(KN_TRANS_WAVE, hipLaunchKernelGGL(k_transitions<0>, dim3(SPILL_GRID), dim3(TB), 0, s, g, b, p, w));
  mk.begin(KN_TRANS_GLOBAL, s);
  hipLaunchKernelGGL(k_transitions<1>, dim3(BIG_SLOTS), dim3(TB), 0, s, g, b, p, w);
  hipLaunchKernelGGL(k_transitions<2>, dim3(HUGE_SLOTS), dim3(TB), 0, s, g, b, p, w);
  mk.count(2);
  mk.end(KN_TRANS_GLOBAL, s);
}
void launch_viterbi(const DevBatch& b, DevWork& w, hipStream_t s, const Marks& mk) {
  // the form: OTM_VIT_FORM (4: the row form, 8, 16 or 64) for the tests; by
  // default the grouped forms from 32,768 traces up, the row form from 4,096
  // and the wave form below.  Why the grouped forms start that high:
  // a small batch's waves all fit the GPU at once, so its time is one wave's
  // (~100 steps of a latency-bound chain either way), while a large batch's
  // is wave rounds, which 8 traces per wave divide (round-4 A/B,
  // profiles/r04_ab/vit_form_*: config 2 0.157 ms wave form vs 0.50 grouped,
  // config 4 1.13 vs 0.73)
  // (read per batch: tests switch them)
  const char* fe = std::getenv("OTM_VIT_FORM");
  const int forced = fe ? std::atoi(fe) : 0;
  constexpr int gmin = 32768;
  // the row form from 4,096 traces: below, a batch's waves are few enough per
  // SIMD that a step's latency, not VALU issue, sets its time, and the wave
  // form's step is the shorter one (profiles/viterbi_plain/sweep.json: 61 us
  // against 65 + 5 at 512 traces, 69 against 69 + 5 at 2,048, 84 against
  // 76 + 5 at 4,096, 123 against 84 + 5 at 8,192)
  constexpr int rmin = 4096;
  const int form = forced ? forced : (b.n_traces >= gmin ? 8 : (b.n_traces >= rmin ? 4 : 64));
  // what a form cannot take goes down a list to the next one (kernels.h: both
  // lists are free between the transition and route stages, K1 zeroes the counts)
  const SpillRef to_16 = spill_of<CTR_VIT_16>(w), to_wave = spill_of<CTR_VIT_WAVE>(w);
  const bool lists = !(w.dormant & TIER_VIT_LISTS);  // the passes over those lists are launched
  if (form == 4) {
    // the row form (k_viterbi_row: four traces per wave) over every trace;
    // what it cannot take (more than VR_PTS points, a column wider than 16
    // candidates) to the wave form, through the CTR_VIT_WAVE list as below.
    // OTM_VR_WIN: the window's floats a chunk may use (the tests force the
    // per-step path with a small one)
    const char* we = std::getenv("OTM_VR_WIN");
    const int vt = OTM_VR_U * 16;
    int win = we ? std::atoi(we) : vt;
    win = win < 0 ? 0 : (win > vt ? vt : win);
    // OTM_VR_FAST=0: every step through the general body (A/B runs, tests)
    const char* fa = std::getenv("OTM_VR_FAST");
    const int fast = fa ? (std::atoi(fa) != 0 ? 1 : 0) : 1;
    mk.begin(KN_VITERBI, s);
    hipLaunchKernelGGL(k_viterbi_row, dim3(grid_for(b.n_traces, TB / 16, WAVE_GRID_CAP)), dim3(TB), 0, s, b, w,
                       to_wave.list, to_wave.count, win, fast, 1);
    mk.count();
    // (sized for every trace, as a batch of long traces needs: a block whose
    // list entries ran out exits at once; on demand: kernels.h TierGroup)
    if (lists) {
      hipLaunchKernelGGL(k_viterbi, dim3(grid_for(b.n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, b, w,
                         (const int32_t*)to_wave.list, (const int32_t*)to_wave.count, 0);
      mk.count();
    }
    mk.end(KN_VITERBI, s);
    return;
  }
  if (form == 64) {
    TIMED(KN_VITERBI, hipLaunchKernelGGL(k_viterbi, dim3(grid_for(b.n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, b,
                                         w, (const int32_t*)nullptr, (const int32_t*)nullptr, 1));
    return;
  }
  // 8 lanes per trace over every trace; what it cannot take (a column wider
  // than 8 candidates, more than VG_PTS points) to 16 lanes per trace; what
  // that cannot take to the wave-per-trace form.
  int32_t* l8 = to_16.list;
  int32_t* n8 = to_16.count;
  int32_t* l16 = to_wave.list;
  int32_t* n16 = to_wave.count;
  mk.begin(KN_VITERBI, s);
  if (form == 16) {
    hipLaunchKernelGGL(k_viterbi_g<16>, dim3(grid_for(b.n_traces, TB / 16, WAVE_GRID_CAP)), dim3(TB), 0, s, b, w,
                       (const int32_t*)nullptr, (const int32_t*)nullptr, l16, n16, 1);
    mk.count();
  } else {
    hipLaunchKernelGGL(k_viterbi_g<8>, dim3(grid_for(b.n_traces, TB / 8, WAVE_GRID_CAP)), dim3(TB), 0, s, b, w,
                       (const int32_t*)nullptr, (const int32_t*)nullptr, l8, n8, 1);
    mk.count();
    // (sized for every trace: a block whose list entries ran out exits at once)
    if (lists) {
      hipLaunchKernelGGL(k_viterbi_g<16>, dim3(grid_for(b.n_traces, TB / 16, WAVE_GRID_CAP)), dim3(TB), 0, s, b, w,
                         (const int32_t*)l8, (const int32_t*)n8, l16, n16, 0);
      mk.count();
    }
  }
  if (lists) {
    hipLaunchKernelGGL(k_viterbi, dim3(grid_for(b.n_traces / 64 + 1, 1, 1024)), dim3(TB), 0, s, b, w,
                       (const int32_t*)l16, (const int32_t*)n16, 0);
    mk.count();
  }
  mk.end(KN_VITERBI, s);
}
void launch_route(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, hipStream_t s,
                  const Marks& mk, int from) {
  if (from >= RESUME_ROUTE_HUGE) {
    mk.begin(KN_ROUTE_GLOBAL, s);
    hipLaunchKernelGGL(k_route<2>, dim3(HUGE_SLOTS), dim3(TB), 0, s, g, b, p, w);
    mk.count();
    mk.end(KN_ROUTE_GLOBAL, s);
    return;
  }
  TIMED(KN_ROUTE_INDEX, hipLaunchKernelGGL(k_route_index, dim3(order_grid(b.n_points, 256, 1 << 30)), dim3(256), 0,
                                           s, g, b, p, w));
  if (w.dormant & TIER_ROUTE_ONLINE) {  // (on demand: kernels.h TierGroup)
    mk.skip(KN_ROUTE_WAVE, s);
    mk.skip(KN_ROUTE_GLOBAL, s);
    return;
  }
  TIMED(KN_ROUTE_WAVE, hipLaunchKernelGGL(k_route<0>, dim3(SPILL_GRID), dim3(TB), 0, s, g, b, p, w));
  mk.begin(KN_ROUTE_GLOBAL, s);
  hipLaunchKernelGGL(k_route<1>, dim3(BIG_SLOTS), dim3(TB), 0, s, g, b, p, w);
  hipLaunchKernelGGL(k_route<2>, dim3(HUGE_SLOTS), dim3(TB), 0, s, g, b, p, w);
  mk.count(2);
  mk.end(KN_ROUTE_GLOBAL, s);
}
void launch_segments(const DevGraph& g, const DevBatch& b, DevWork& w, DevOut& o, hipStream_t s, const Marks& mk) {
  const dim3 grid(grid_for(b.n_traces, 1, WAVE_GRID_CAP));
  // small LDS plan over every trace, the large one over its spills
  // (CTR_SEG_LARGE: its list is free after the route stage)
  const SpillRef large = spill_of<CTR_SEG_LARGE>(w);
  int32_t* lst = large.list;
  int32_t* cnt = large.count;
  mk.begin(KN_SEG_WRITE, s);
  hipLaunchKernelGGL((k_segments<SEGP_PTS_S, SEGP_TRAV_S>), grid, dim3(TB), 0, s, g, b, w, o, (const int32_t*)nullptr,
                     (const int32_t*)nullptr, lst, cnt);
  mk.count();
  if (!(w.dormant & TIER_SEG_LARGE)) {  // (on demand: kernels.h TierGroup)
    hipLaunchKernelGGL((k_segments<SEGP_PTS, SEGP_TRAV>), dim3(grid_for(b.n_traces, 1, 2048)), dim3(TB), 0, s, g, b,
                       w, o, (const int32_t*)lst, (const int32_t*)cnt, (int32_t*)nullptr, (int32_t*)nullptr);
    mk.count();
  }
  mk.end(KN_SEG_WRITE, s);
}
void launch_queue(const DevBatch& b, DevWork& w, DevOut& o, float kph, hipStream_t s) {
  hipLaunchKernelGGL(k_queue, dim3(grid_for(b.n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, b, w, o, kph);
}
void launch_points(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, otm_matched_point* out,
                   hipStream_t s) {
  hipLaunchKernelGGL(k_points, dim3(grid_for(b.n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, g, b, p, w, out);
}
void launch_scores(const DevBatch& b, DevWork& w, const DevScores& sc, hipStream_t s) {
  if (b.n_traces <= 0 || b.n_points <= 0) return;
  // the form: OTM_SCORE_FORM (1: the general form, 4: the packed form) for the
  // tests; by default the packed form from the batch size at which
  // launch_viterbi takes its row form (below it a batch's waves all fit the
  // GPU at once and four traces a wave only lengthen the one round)
  // (read per batch: tests switch them)
  const char* fe = std::getenv("OTM_SCORE_FORM");
  const int forced = fe ? std::atoi(fe) : 0;
  constexpr int rmin = 4096;
  const int form = forced == 1 || forced == 4 ? forced : (b.n_traces >= rmin ? 4 : 1);
  if (form == 1) {
    hipLaunchKernelGGL(k_scores<64>, dim3(grid_for(b.n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, b, w, sc,
                       (const int32_t*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr);
    return;
  }
  // the packed form over every trace; what it cannot take (more than
  // SC_ROW_PTS points, a scored column wider than 16 candidates) to the
  // general form through sc.rej (sized for every trace: a block whose list
  // entries ran out exits at once)
  (void)hipMemsetAsync(sc.rej_n, 0, sizeof *sc.rej_n, s);
  hipLaunchKernelGGL(k_scores<16>, dim3(grid_for(b.n_traces, TB / 16, WAVE_GRID_CAP)), dim3(TB), 0, s, b, w, sc,
                     (const int32_t*)nullptr, (const int32_t*)nullptr, sc.rej, sc.rej_n);
  hipLaunchKernelGGL(k_scores<64>, dim3(grid_for(b.n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, b, w, sc,
                     (const int32_t*)sc.rej, (const int32_t*)sc.rej_n, (int32_t*)nullptr, (int32_t*)nullptr);
}
void launch_traversals(const DevGraph& g, const DevBatch& b, DevWork& w, DevOut& o, const DevTrav& tv, hipStream_t s) {
  hipLaunchKernelGGL(k_traversals, dim3(grid_for(b.n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, g, b, w, o, tv);
}
void launch_trav_compact(int32_t n_traces, const int64_t* seg_base, const int64_t* off, const otm_traversal* reg,
                         otm_traversal* dst, hipStream_t s) {
  hipLaunchKernelGGL(k_trav_compact, dim3(grid_for(n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, n_traces, seg_base, off,
                     reg, dst);
}
void launch_shape(const DevGraph& g, int32_t n_traces, const int64_t* seg_base, const DevTrav& tv, const DevShape& sh,
                  bool write, hipStream_t s) {
  const dim3 grid(grid_for(n_traces, 1, WAVE_GRID_CAP));
  if (write)
    hipLaunchKernelGGL(k_shape<true>, grid, dim3(TB), 0, s, g, n_traces, seg_base, tv, sh);
  else
    hipLaunchKernelGGL(k_shape<false>, grid, dim3(TB), 0, s, g, n_traces, seg_base, tv, sh);
}
void launch_seg_bound(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, int64_t* tb, hipStream_t s,
                      const Marks& mk) {
  TIMED(KN_SEG_BOUND, hipLaunchKernelGGL(k_seg_bound, dim3(grid_for(b.n_points + 1, 256, 1 << 30)), dim3(256), 0, s,
                                         g, b, p, w, tb));
}
void launch_compact(int32_t n_traces, const DevOut& o, const int32_t* seg_off, const int32_t* way_off,
                    const int32_t* rep_off, otm_segment* segs_out, int64_t* ways_out, otm_report_rec* reps_out,
                    otm_trace_result* traces_out, hipStream_t s) {
  hipLaunchKernelGGL(k_compact, dim3(grid_for(n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s, n_traces, o, seg_off, way_off,
                     rep_off, segs_out, ways_out, reps_out, traces_out);
}
void launch_report(const DevBatch& b, const DevReportCfg& rc, DevWork& w, DevOut& o, hipStream_t s,
                   const Marks& mk) {
  // thread per trace; the serial segment walk is latency-bound, so small
  // blocks spread the traces over more waves (0.053 -> 0.050 ms against 64 on
  // config 2)
  constexpr int tb = 16;
  if (b.n_traces <= REPW_MAX_TRACES)
    TIMED(KN_REPORT, hipLaunchKernelGGL(k_report_wave, dim3(grid_for(b.n_traces, 1, WAVE_GRID_CAP)), dim3(TB), 0, s,
                                        b, rc, w, o, 0));
  else
    TIMED(KN_REPORT, hipLaunchKernelGGL(k_report, dim3(grid_for(b.n_traces, tb, 1 << 30)), dim3(tb), 0, s, b, rc, w,
                                        o, 0));
}
#undef TIMED

void launch_index_build(const DevGraph& g, const uint32_t* turn_units, uint32_t cmax, int32_t* row_cnt,
                        const IdxRow* rows, uint4* slot, bool write, hipStream_t s) {
  const int grid = grid_for((int64_t)g.n_edges + g.n_nodes, 1, 256 * 16);
  if (write)
    hipLaunchKernelGGL(k_index_build<true>, dim3(grid), dim3(TB), 0, s, g, turn_units, cmax, row_cnt, rows, slot);
  else
    hipLaunchKernelGGL(k_index_build<false>, dim3(grid), dim3(TB), 0, s, g, turn_units, cmax, row_cnt, rows, slot);
}
int index_load_fast() { return IDX_LOAD_FAST; }
int index_load_dense() { return IDX_LOAD_DENSE; }
void launch_row_sizes(const int32_t* row_cnt, int64_t* row_sizes, int32_t n, int pct, hipStream_t s) {
  hipLaunchKernelGGL(k_row_sizes, dim3(grid_for((int64_t)n + 1, 256, 1 << 30)), dim3(256), 0, s, row_cnt, row_sizes,
                     n, pct);
}
void launch_row_pack(const int32_t* row_cnt, const int64_t* row_off, IdxRow* rows, int32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_row_pack, dim3(grid_for((int64_t)n, 256, 1 << 30)), dim3(256), 0, s, row_cnt, row_off, rows, n);
}
void launch_src_pack(const DevGraph& g, const IdxRow* rows, SrcRec* src, hipStream_t s) {
  if (g.n_edges <= 0) return;
  hipLaunchKernelGGL(k_src_pack, dim3(grid_for((int64_t)g.n_edges, 256, 1 << 30)), dim3(256), 0, s, g, rows, src);
}

size_t scan_tmp_bytes(int64_t n) {
  size_t a = 0, c = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, (int64_t*)nullptr, (int64_t*)nullptr, (int)(n + 1));
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, c, (int32_t*)nullptr, (int32_t*)nullptr, (int)(n + 1));
  return a > c ? a : c;
}
void scan_i64(int64_t* d, int64_t n, void* tmp, size_t tmp_bytes, hipStream_t s) {
  (void)hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, d, d, (int)(n + 1), s);
}
void scan_i32(int32_t* d, int64_t n, void* tmp, size_t tmp_bytes, hipStream_t s) {
  (void)hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, d, d, (int)(n + 1), s);
}

}  // namespace otm
