// kernels.h -- device data views and launch wrappers of the matcher kernels.
//
// Pipeline of one batch, all on one HIP stream:
//   K1 k_columns      thread / trace   interpolation filter, gc to previous column
//   K2 k_candidates   wave / probe     grid cells -> projections -> LDS edge hash
//                                      -> bitonic sort -> top-K + emission
//   K3 k_links        thread / point   chain links + transition-matrix sizes, scan
//   K4 k_trans_sub    8/16 lanes / col route-index probes per (source, target)
//                                      pair; k_transitions: turn-aware search
//                                      per source for what the index cannot
//                                      answer (LDS, then global tier)
//   K5 k_viterbi      wave / trace     min-sum decode, lanes = states
//   K6 k_route_index  thread / step    the winning label's predecessor chain (k_route: search)
//   K7 k_segments     thread / trace   traversals -> OSMLR segments (count+write)
//   K8 k_report       thread / trace   reporter_service.py:110-215 + histogram
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "otmatch.h"
#include "pairs.h"

namespace otm {

constexpr int KMAX = 32;           // max candidates per column (== ORC_KMAX)
// inline candidate slots per point (DevWork::cand_eo / cand_em); 4 (a point's
// blocks half the size, slots 4.. in the overflow) measured slower on configs
// 2 and 4
constexpr int KIN = 8;
static_assert(KIN == 4 || KIN == 8, "inline blocks of 4 or 8 slots (whole 16-B emission pieces)");
constexpr int KX = KMAX - KIN;     // overflow candidate slots per point (DevWork::cand_xeo / cand_xem)
constexpr int MAX_HITS = 256;      // distinct edges within one radius in the LDS tiers (beyond: the global tier)
constexpr int SEARCH_LIMIT = 98304;  // labels (edges + nodes) of one global-tier search (beyond: the huge tier)
constexpr int LDS_TABLE_CAP = 256;   // K4/K6 LDS tier: table slots
constexpr int LDS_TABLE_LIMIT = 192; // ... labels before spilling to the global tier
constexpr int BIG_TABLE_LOG2 = 17;
constexpr int BIG_TABLE_CAP = 1 << BIG_TABLE_LOG2;  // global tier table slots (> SEARCH_LIMIT / 0.75)
#ifndef OTM_BIG_SLOTS
#define OTM_BIG_SLOTS 512
#endif
constexpr int BIG_SLOTS = OTM_BIG_SLOTS;  // concurrent global-tier searches
// The huge search tier (round 4): searches beyond SEARCH_LIMIT labels, in
// HUGE_SLOTS tables of 2^huge_log2 slots sized by the host (grown and the
// batch redone when a search does not fit: no label limit but memory)
constexpr int HUGE_SLOTS = 8;
// The candidate search's HBM tier (round 4): probes with more than MAX_HITS
// distinct edges within their radius, CAND_BIG_SLOTS at a time, in tables of
// 2^cand_log2 slots (half of them the sort keys) sized like the huge tier.
constexpr int CAND_BIG_SLOTS = 64;
// the largest tables the host grows the two on-demand tiers to (8 x 2^27 huge
// slots ~ 29 GB, 64 x 2^23 candidate slots ~ 8.6 GB; env OTM_HUGE_MAX_LOG2 /
// OTM_CAND_MAX_LOG2 lower them, test hooks): past them, or when HBM runs out,
// a search or probe that does not fit fails its own trace with a 500, not
// the batch
constexpr int HUGE_MAX_LOG2 = 27, CAND_MAX_LOG2 = 23;
__host__ __device__ inline int huge_limit(int log2) { return log2 > 2 ? 3 << (log2 - 2) : 0; }  // 0.75 x slots

struct DevGraph {
  const float *node_lat, *node_lon;
  const int32_t* out_off;
  const int32_t *e_from, *e_to;
  const float* e_len;
  const int32_t* e_shape_off;
  const int64_t* e_way;
  const int32_t *e_seg, *e_seg_pos;
  const uint8_t* e_flags;
  const float *s_lat, *s_lon, *s_cum;
  const uint64_t* g_id;
  const float* g_len;
  const uint32_t* cell_off;  // 32-bit in HBM (engine_init checks the entry count)
  const uint32_t* cell_ent;
  const float4* ent_geo;  // per cell entry: shape segment endpoints (lat_a, lon_a, lat_b, lon_b)
  const uint16_t *e_head_out, *e_head_in;  // edge bearing at start / end, whole degrees (turn costs)
  const uint32_t* e_len64;                 // L(e) = round(len(e) x 64): the route searches' edge costs (1/64 m)
  // K7's per-edge record {len bits, seg, seg_pos | flags << 24, way number}
  // and the way numbers' ids (engine.cpp)
  const uint4* e_rec;
  const int2* e_fl;  // {from node, length bits} per edge: a transition source's row and start in one load
  // A projection's operands in two dependent trips, three loads (kernels.hip
  // proj_load; engine.cpp builds both): the edge's projection record {first
  // shape point, last shape point, length bits, out_off[from]} -- the last
  // word the start node's representative edge -- then the segment's two shape
  // points, 32 contiguous bytes of s_pt: {lat, lon, cum, end}, the floats of
  // s_lat / s_lon / s_cum, and end: -1 on every point but an edge's last,
  // there the end node's representative edge out_off[to], or -2 when that
  // node has no outgoing edge
  const int4* e_proj;
  const float4* s_pt;
  const int64_t* way_tab;
  int32_t n_nodes, n_edges, n_segments, grid_rows, grid_cols;
  double lat0, lon0, cell;
  // spatial work order tiles: the node bbox cut into ORDER_SIDE^2 tiles
  float bb_lat0, bb_lon0, bb_inv_h, bb_inv_w;  // tile row = (lat - bb_lat0) * bb_inv_h, ...
};

// Spatial work order of a batch's columns: column points
// bucketed by the Hilbert index of their tile, the tiles cut into 8
// equal-count groups.  Group g runs on the blocks with blockIdx % 8 == g,
// which the dispatcher deals to one XCD, so each XCD's L2 holds one region's
// grid cells and index rows; inside a group, neighbouring lanes and waves get
// neighbouring probes.
#ifndef OTM_ORDER_BITS
#define OTM_ORDER_BITS 6
#endif
constexpr int ORDER_BITS = OTM_ORDER_BITS;  // <= 8: tile ids are u16
constexpr int ORDER_SIDE = 1 << ORDER_BITS;  // 64 x 64 tiles
constexpr int ORDER_TILES = ORDER_SIDE * ORDER_SIDE;
constexpr int ORDER_GROUPS = 8;
struct DevOrder {
  int32_t* item;      // [n] column points, grouped
  int32_t* grp;       // [ORDER_GROUPS + 1] group starts in item space
  uint16_t* tile;     // [P] tile of each column (K1)
  int32_t* tile_cnt;  // [ORDER_TILES] columns per tile (K1); nullptr: no order this batch
  int32_t* cursor;    // [ORDER_TILES] scatter cursors
};

// Bounded route index (built once per engine): one row per
// source of the turn-aware route search -- row e < E: from edge e's end node,
// entered along e; row E + u: from node u, no heading (node candidates) --
// holding every label of that search within cost cmax (1/64 m): the departure
// label of each edge (key = edge id) and the arrival label of each node (key
// = NODE_KEY | node), as one open-addressing hash table per row (linear
// probing from 2-slot buckets at 30 or 40 % load).  A slot is 16 bytes, {key, cost,
// route distance bits, turn units} with the label's predecessor slot in the
// cost's and units' top bytes (kernels.hip idx_slot_*): the route to the
// edge's start turned into it (or to the node), so a transition reads its
// distance and turn cost from one slot, and a route walks slot to slot.  cnt
// < 0 marks a row whose search exceeded the build table (queries on it use
// the online tiers).
struct IdxRow {
  int64_t off;    // first slot of the row's table
  int32_t cnt;    // entries, -1 incomplete
  uint32_t cap;   // table slots (0 for an empty or incomplete row)
};
// Per-edge source record of an index (built once with it): both rows a
// transition or route source on edge e can stand for -- row e (an edge
// candidate) and row E + from(e) (a node candidate) -- beside the edge's from
// node and length, so that the row descriptor's address depends on the
// candidate record {edge, offset} alone and its load leaves with the
// {from, length} pair's, not behind it (k_trans_sub, k_route_index).  Padded
// to OTM_SRC_REC_BYTES, 48: the 40 B of payload in the fewest 16-B pieces.  At
// 64 a record never straddles a 128-B line, but the records take a third more
// lines of cache: config 4's k_trans_sub 1.340 ms at 64 against 1.328 at 48
// (1.389 without the records; config 2 the same at both).
#ifndef OTM_SRC_REC_BYTES
#define OTM_SRC_REC_BYTES 48
#endif
struct alignas(16) SrcRec {
  IdxRow edge;     // row e
  IdxRow node;     // row E + from(e)
  int32_t from;    // from(e)
  int32_t len;     // len(e), float bits
  int32_t pad[(OTM_SRC_REC_BYTES - 40) / 4];
};
static_assert(sizeof(SrcRec) == OTM_SRC_REC_BYTES && (OTM_SRC_REC_BYTES == 48 || OTM_SRC_REC_BYTES == 64),
              "source records of 48 or 64 bytes");
struct DevIndex {
  float rmax;     // 0: no index
  uint32_t cmax;  // its cost bound, floor(rmax x 64)
  const IdxRow* row;   // [E + N]
  const SrcRec* src;   // [E] the rows and {from, length} of each edge as a source (nullptr: no index)
  const uint4* slot;    // 16 B per slot: 53 B per entry at 30 % load, 40 B at 40 %
  int load_pct;         // the tables' load
};
constexpr int IDX_SLOT_BYTES = 16;
// the index radius is capped so that every cost in a slot is below 2^24 (1/64 m)
constexpr float INDEX_RMAX_CAP = 200000.0f;
constexpr uint32_t NODE_KEY = 0x80000000u;  // key of a node's arrival label (edges: their id, < 2^27)
constexpr uint32_t NONE_PRED = 0xFFFFFFFFu; // label predecessor of a route's first edge / the source node
// near indexes: at most NEAR_LEVELS smaller radii of the same rows
// (engine.cpp build_index).  By default one, at OTM_INDEX_NEAR_FRACS x the
// index's radius, when the index's tables reach OTM_INDEX_NEAR_MIN_GB: a
// large index's probes miss the caches, and a column whose bound the near
// index covers then probes tables a fraction of the size (config 3: 137 GB,
// k_trans_sub 4.65 -> 3.31 ms at 600 m of 1,250; config 4: 62 GB, 2.17 ->
// 1.74 ms at 3.5 km of 10); a small one's probes hit the caches already and
// two tables split them (config 2: 5 GB, 0.210 -> 0.225 ms at 400 m).
constexpr int NEAR_LEVELS = 3;
#ifndef OTM_INDEX_NEAR_FRACS
#define OTM_INDEX_NEAR_FRACS {0.45f}
#endif
#ifndef OTM_INDEX_NEAR_MIN_GB
#define OTM_INDEX_NEAR_MIN_GB 16.0
#endif
constexpr int INDEX_BUILD_LOG2 = 11;
constexpr int INDEX_BUILD_CAP = 1 << INDEX_BUILD_LOG2;  // LDS table of the index builder
constexpr int INDEX_BUILD_LIMIT = 1536; // labels per row before the row is left incomplete
// cost bound (1/64 m) of a search bounded by B metres (oracle cost_bound)
__host__ __device__ inline uint32_t index_cost_bound(float B) { return (uint32_t)floor((double)B * 64.0); }

// which kernels walk the spatial work order (DevParams::order_mask: all three)
constexpr int ORDER_CAND = 1, ORDER_TRANS = 2, ORDER_ROUTE = 4;
constexpr int TURN_TABLE = 181;                 // turn units per deviation 0..180 degrees
constexpr uint32_t TURN_UNITS_MAX = 0xFFFFFFu;   // 2^24 - 1: a route's units sum exact in a float
constexpr uint32_t NO_TURNS = 0xFFFFFFFFu;       // index slot heads of the empty route (v == u)
struct DevParams {
  float sigma_z, beta, factor, breakage, interp, search_radius, max_search_radius, gps_accuracy;
  const uint32_t* turn_units;  // [TURN_TABLE] (device)
  int max_candidates;
  int order_mask;
  int cand_wave_all;  // small batch: every probe to the wave tier (latency, not throughput, bound)
  int cand_chunk;     // lane tier: entries of a grid row scanned before their hits are inserted (1..64)
};

struct DevReportCfg {
  int n_report, n_transition;
  int64_t report_levels[16];
  int64_t transition_levels[16];
  double threshold_sec;
};

struct DevBatch {
  int32_t n_traces;
  int64_t n_points;
  const int64_t* trace_off;
  const float *lat, *lon;
  const double* time;
  const float* acc;
};

// device counters, same order as otm_work_counters
struct DevCounters {
  unsigned long long points, columns, cells_visited, cell_entries_scanned, candidates;
  unsigned long long searches, nodes_settled, edges_relaxed, transitions;
  unsigned long long route_searches, route_nodes_settled, route_edges_relaxed, route_edges;
  unsigned long long segments_out, reports_out;
};

// ---- The batch protocol's words: DevWork::counters_i32 and the spill lists.
//
// A stage's kernels hand the work a tier cannot take to the next tier through
// a list of point (or trace) numbers in one of DevWork::spill_list1..3 and its
// entry count in a slot of counters_i32; the filler appends with an atomicAdd
// on the count (spill_push), the drainer reads both on the device (spill_of),
// so no tier costs a host round trip.  The lists are reused from stage to
// stage; ctr_list() below says which list a count belongs to.
//
// Slots below CTR_STAGE_WORDS are per stage: block 0 of k_columns (K1) zeroes
// them, fold_snap copies them to snapshot k of SnapBuf and resets them at the
// stage boundaries SNAP_AFTER_CAND (in k_links) and SNAP_AFTER_TRANS (in the
// first Viterbi launch), and copies them without a reset at SNAP_AFTER_ROUTE
// (in k_seg_bound); engine_match copies a snapshot back into them when a batch
// resumes at a tier whose tables grew, and engine_spill_stats reads the
// snapshots.  Slots from CTR_STAGE_WORDS to CTR_ZEROED_WORDS are per batch:
// K1 alone zeroes them, so they survive the stage boundaries and a resume
// (which is what the resumed tier's list count needs); the host clears the two
// grow flags before a resume.
//
//   slot               list  filled by -> drained by
//   CTR_UNUSED         -     free (nothing writes or reads it)
//   CTR_POOL_USED      -     path-pool words taken (k_route_index, k_route); read by k_status
//   CTR_POOL_OVER      -     flag: the pool overflowed (the host grows pool_cap, redoes the batch)
//   CTR_SEARCH_GLOBAL  2     LDS search tier -> global tier, in the transition stage
//                            (k_transitions<0> -> <1>) and again in the route stage (k_route<0> -> <1>)
//   CTR_INDEX_MISS     1     what the route index cannot answer -> LDS search tier: k_trans_sub ->
//                            k_transitions<0>, then k_route_index -> k_route<0>
//   CTR_CAND_WAVE      1     candidate lane tier -> wave tier (k_cand_lane -> k_candidates<false>)
//   CTR_TRANS_WIDE     2     k_trans_sub<8, false>'s wide columns -> k_trans_sub<16, true>
//   CTR_SEG_LARGE      1     k_segments' small plan -> its large plan (launch_segments), after
//                            SNAP_AFTER_ROUTE: in no snapshot, zero whenever a snapshot is copied back
//   CTR_VIT_16         1     Viterbi 8 lanes per trace -> 16 lanes (launch_viterbi)
//   CTR_TRANS_HUGE     3     global tier -> huge tier, transitions (k_transitions<1> -> <2>)
//   CTR_ROUTE_HUGE     3     global tier -> huge tier, routes (k_route<1> -> <2>); non-zero also tells
//                            the host which stage's huge tier to resume at (BatchStatus::route_huge)
//   CTR_GROW_HUGE      -     flag: the huge tier needs (larger) tables (huge_unready, huge_overflow)
//   CTR_CAND_BIG       3     candidate wave tier -> HBM tier (k_candidates<false> -> <true>)
//   CTR_GROW_CAND      -     flag: the candidate HBM tier needs (larger) tables (k_candidates)
//   CTR_VIT_WAVE       2     Viterbi row form or 16 lanes -> wave form (launch_viterbi)
//   CTR_TIER_WAKE      -     TierGroup bits: a kernel pushed onto a list whose drainers were not launched
//                            (tier_wake below; the host makes the groups live and runs the batch again)
//
// The Viterbi counts are per batch, not per stage: SNAP_AFTER_TRANS is taken
// (and the per-stage slots reset) by one thread of the first Viterbi launch,
// whose other blocks are appending to these lists by then.  Lists 1 and 2 are
// free between the transition and route stages, and an attempt that aborted
// earlier skips Viterbi, so the counts are filled once per batch.
enum CtrSlot : int {
  CTR_UNUSED = 0,
  CTR_POOL_USED = 1,
  CTR_POOL_OVER = 2,
  CTR_SEARCH_GLOBAL = 3,
  CTR_INDEX_MISS = 4,
  CTR_CAND_WAVE = 5,
  CTR_TRANS_WIDE = 6,
  CTR_SEG_LARGE = 8,
  CTR_VIT_16 = 20,
  CTR_TRANS_HUGE = 21,
  CTR_ROUTE_HUGE = 22,
  CTR_GROW_HUGE = 23,
  CTR_CAND_BIG = 24,
  CTR_GROW_CAND = 25,
  CTR_VIT_WAVE = 26,
  CTR_TIER_WAKE = 27,
};
constexpr int CTR_STAGE_WORDS = 16;   // per stage: snapshot and reset
constexpr int CTR_ZEROED_WORDS = 32;  // per stage + per batch: zeroed by K1
constexpr int CTR_WORDS = 64;         // allocated
// ---- Tiers on demand.  Five launch groups exist only for work that an earlier
// kernel pushes onto a device list, and on most workloads those lists stay
// empty batch after batch: each launch then starts its blocks to read a zero
// and costs its 4-5 us on the stream.  Every batch context keeps a mask of
// live groups (otm_engine::tier_dormant, engine.cpp tiers_learn): a group
// whose first list stayed empty for TIER_QUIET completed batches goes dormant
// and is not launched.  DevWork::dormant tells the kernels; one that pushes
// onto a dormant group's list also sets its bit in CTR_TIER_WAKE and the abort
// flag (tier_wake), every later kernel returns at once as after a capacity
// overflow, and the host makes the group live for the rest of the context's
// life and runs the batch again.  OTM_TIERS_ALWAYS=1 keeps every group live.
enum TierGroup : int {
  TIER_CAND_BIG = 1,      // k_candidates<true>            first list CTR_CAND_BIG
  TIER_TRANS_ONLINE = 2,  // k_transitions<0..2>           first list CTR_INDEX_MISS (transition stage)
  TIER_ROUTE_ONLINE = 4,  // k_route<0..2>                 first list CTR_INDEX_MISS (route stage)
  TIER_VIT_LISTS = 8,     // Viterbi list passes           lists CTR_VIT_WAVE, CTR_VIT_16
  TIER_SEG_LARGE = 16,    // k_segments' large plan        list CTR_SEG_LARGE
  TIER_ALL = 31,
};
constexpr int TIER_GROUPS = 5;
constexpr int TIER_QUIET = 2;  // completed batches with an empty first list before a group goes dormant
enum SnapId : int { SNAP_AFTER_CAND = 0, SNAP_AFTER_TRANS = 1, SNAP_AFTER_ROUTE = 2, SNAP_COUNT = 3 };
// which of DevWork::spill_list1..3 the count in slot c belongs to (0: c counts no list)
constexpr int ctr_list(CtrSlot c) {
  switch (c) {
    case CTR_INDEX_MISS: case CTR_CAND_WAVE: case CTR_SEG_LARGE: case CTR_VIT_16: return 1;
    case CTR_SEARCH_GLOBAL: case CTR_TRANS_WIDE: case CTR_VIT_WAVE: return 2;
    case CTR_TRANS_HUGE: case CTR_ROUTE_HUGE: case CTR_CAND_BIG: return 3;
    default: return 0;
  }
}
constexpr bool ctr_per_stage(CtrSlot c) { return c >= 0 && c < CTR_STAGE_WORDS; }
constexpr bool ctr_per_batch(CtrSlot c) { return c >= CTR_STAGE_WORDS && c < CTR_ZEROED_WORDS; }
static_assert(ctr_per_stage(CTR_UNUSED) && ctr_per_stage(CTR_POOL_USED) && ctr_per_stage(CTR_POOL_OVER) &&
                  ctr_per_stage(CTR_SEARCH_GLOBAL) && ctr_per_stage(CTR_INDEX_MISS) && ctr_per_stage(CTR_CAND_WAVE) &&
                  ctr_per_stage(CTR_TRANS_WIDE) && ctr_per_stage(CTR_SEG_LARGE),
              "per-stage slots lie in the snapshot range");
static_assert(ctr_per_batch(CTR_VIT_16) && ctr_per_batch(CTR_TRANS_HUGE) && ctr_per_batch(CTR_ROUTE_HUGE) &&
                  ctr_per_batch(CTR_GROW_HUGE) && ctr_per_batch(CTR_CAND_BIG) && ctr_per_batch(CTR_GROW_CAND) &&
                  ctr_per_batch(CTR_VIT_WAVE) && ctr_per_batch(CTR_TIER_WAKE),
              "per-batch slots lie past the snapshot range, within what K1 zeroes");

// per-point / per-trace work arrays of one batch (device pointers)
struct DevWork {
  int32_t* pt_trace;     // [P] trace of point
  uint8_t* is_col;       // [P]
  int32_t* prevc;        // [P] column: previous column (unlinked), -1; other points: the column before them
  int32_t* nextc;        // [P] column q: its next column p when interpolated points lie between (K3), else -1
  float* gc;             // [P]
  int32_t* ncand;        // [P]
  float4* probe;         // [P] {lat, lon, accuracy, 0}: a probe's inputs in one line (K1)
  // Candidates of point p, slot j: the first KIN slots
  // inline -- {edge, offset bits} at cand_eo[p * KIN + j] (two points per
  // 128-B line) and the emission at cand_em[p * KIN + j] (four points per
  // line); slots KIN.. of the rare wider points at cand_xeo / cand_xem[p * KX
  // + j - KIN] (untouched lines for every other point)
  int2* cand_eo;         // [P*KIN]
  float* cand_em;        // [P*KIN]
  int2* cand_xeo;        // [P*KX]
  float* cand_xem;       // [P*KX]
  int32_t* col_prev;     // [P] linked previous column, -1
  int32_t* kq_prev;      // [P] candidates of the linked previous column (K3), so K4 reads them with p's own words
  uint8_t* vmeta;        // [P] K5's byte per point (K3): candidates | column << 6 | linked << 7
  int64_t* trans_off;    // [P+1]
  float* trans;          // [total]
  uint8_t* bp;           // [P*KMAX]
  int32_t* state;        // [P]
  int2* chosen;          // [P] the chosen candidate {edge, offset bits} where state >= 0 (K5)
  uint8_t* chain_start;  // [P]
  float* route_dist;     // [P]
  float* ipos;           // [P] interpolated point: position along its step's route (K7a), -1 none
  int32_t* path_off;     // [P]
  int32_t* path_len;     // [P]
  int32_t* path_pool;    // [pool_cap]
  int32_t pool_cap;
  int32_t dormant;       // TierGroup bits: groups not launched this attempt (in pool_cap's padding: no field moves)
  int32_t* trace_err;    // [T]
  int32_t* spill_list1;    // [P] a stage's first spill list (CtrSlot above: who fills and drains it when)
  int32_t* spill_list2;    // [P] ... its second
  int32_t* snap;           // SnapBuf::stage: the per-stage counters at the three stage boundaries
  int32_t* counters_i32;   // [CTR_WORDS] indexed by CtrSlot
  int32_t* abort;          // [1] set when a capacity (transition matrices, path pool) was exceeded:
                           // every later kernel returns at once and the host redoes the batch
  int64_t trans_cap;       // floats allocated for w.trans
  // K4's column records in spatial-order position, written by K3 at the
  // position the order scatter noted per column (colrec_pos): {p, col_prev,
  // kq_prev | ncand << 8, gc bits}; null: k_trans_sub reads the per-point arrays
  int4* colrec;
  int32_t* colrec_pos;
  DevIndex idx;
  DevIndex idxn[NEAR_LEVELS];  // near indexes, smallest radius first (rmax 0: none): a column
                               // probes the first whose cmax covers its cost bound
  DevOrder ord;
  // global-tier scratch
  uint32_t* big_key;
  unsigned long long* big_lab;
  uint32_t* big_inq;
  uint32_t* big_fr;
  uint32_t* big_ins;       // [BIG_SLOTS * SEARCH_LIMIT] slots each table's last search inserted
  int32_t* big_prev;       // [BIG_SLOTS] their count (-1: clear the whole table)
  // huge-tier scratch ([HUGE_SLOTS << huge_log2] slots; huge_log2 == 0: none yet)
  uint32_t* huge_key;
  unsigned long long* huge_lab;
  uint32_t* huge_inq;
  uint32_t* huge_fr;
  uint32_t* huge_ins;      // [HUGE_SLOTS * huge_limit(huge_log2)]
  int32_t* huge_prev;      // [HUGE_SLOTS]
  int32_t huge_log2;
  int32_t huge_final;      // the huge tables cannot grow: an overflowing search fails its trace (500)
  // candidate HBM tier ([CAND_BIG_SLOTS << cand_log2] slots; cand_log2 == 0: none yet)
  uint32_t* cbig_key;
  unsigned long long* cbig_val;
  unsigned long long* cbig_skey;  // [CAND_BIG_SLOTS << (cand_log2 - 1)]
  int32_t cand_log2;
  int32_t cand_final;      // the candidate tables cannot grow: an overflowing probe fails its trace (500)
  int32_t* spill_list3;    // [P] the list of a tier whose tables the host sizes (huge search, candidate HBM)
  DevCounters* ctr;        // nullptr when counting is off
};
// a spill list with its entry count, by the count's slot
struct SpillRef {
  int32_t* list;
  int32_t* count;
};
template <CtrSlot C>
__host__ __device__ __forceinline__ int32_t* spill_list(const DevWork& w) {
  constexpr int L = ctr_list(C);
  static_assert(L != 0, "this slot counts no list");
  return L == 1 ? w.spill_list1 : (L == 2 ? w.spill_list2 : w.spill_list3);
}
template <CtrSlot C>
__host__ __device__ __forceinline__ SpillRef spill_of(const DevWork& w) {
  return SpillRef{spill_list<C>(w), w.counters_i32 + C};
}

// Outputs of one batch.  Segments, way ids and reports are written in one
// pass into per-trace regions sized by an upper bound (2 traversals per
// matched point + its route's path edges, summed per trace and scanned over
// traces: trace t's region starts at seg_base[t]); otm_fetch_results compacts
// them.
struct DevOut {
  // per trace
  otm_trace_result* traces;  // [T] (seg_off / rep_off = region start)
  int32_t* seg_cnt;      // [T+1] segments per trace
  int32_t* way_cnt;      // [T+1] way ids per trace
  int32_t* rep_cnt;      // [T+1] reports per trace
  int64_t* seg_base;     // [T+1] exclusive scan of the per-trace bound
  // regions (capacity = bound total)
  otm_segment* segments;  // []
  int32_t* seg_gidx;     // [] segment index in graph (-1 none)
  int64_t* way_ids;      // []
  otm_report_rec* reports;  // []
  uint32_t* hist;        // [n_segments * nbins] or nullptr
  unsigned long long* speed_sum;  // [n_segments] sum of report speeds, 1/1000 km/h, or nullptr
  int nbins;
  float bin_kph;
  PairTab pairs;         // the pair window's table (pairs.h); key nullptr: none
};

// The matched route's arrays (DESIGN.md §3 rule 7d; bound only with the handle's
// switch on): trace t's records in DevOut's region layout, at seg_base[t].
struct DevTrav {
  otm_traversal* rec;  // [] regions (capacity = DevOut's bound total)
  int64_t* cnt;        // [T+1] records per trace (cnt[T] = 0: scanned into trav_off at the fetch)
};

// The matched shape's arrays (DESIGN.md §3 rule 7f; made at the first size,
// fetch or device call of a batch).  The count pass leaves each trace's vertex
// and byte counts in vtx_off / poly_off, which the host scans in place; the
// write pass reads them as offsets.
struct DevShape {
  const int64_t* trav_off;  // [T+1] the dense traversal offsets (the scan of DevTrav::cnt): where the spans go
  int64_t* vtx_off;         // [T+1] counts, then offsets (element T: 0, then the total)
  int64_t* poly_off;        // [T+1] likewise, in bytes
  otm_shape_vertex* vtx;    // [vtx_off[T]]    (write pass only)
  otm_shape_span* span;     // [trav_off[T]]
  char* poly;               // [poly_off[T]]
};

// Per-kernel timing (otm_get_kernel_ms): when ev != nullptr the launchers
// record ev[2k] just before and ev[2k+1] just after kernel k, on the launch
// stream.  Order and names: kKernelNames in kernels.hip.
enum KernelId {
  KN_COLUMNS,
  KN_ORDER,
  KN_CAND_LANE,
  KN_CAND_WAVE,
  KN_LINKS,
  KN_SCAN_TRANS,
  KN_TRANS_INDEX,
  KN_TRANS_WIDE,
  KN_TRANS_WAVE,
  KN_TRANS_GLOBAL,
  KN_VITERBI,
  KN_ROUTE_INDEX,
  KN_ROUTE_WAVE,
  KN_ROUTE_GLOBAL,
  KN_SEG_BOUND,
  KN_SEG_SCAN,
  KN_SEG_WRITE,
  KN_REPORT,
  KN_COUNT
};
extern const char* const kKernelNames[KN_COUNT];
struct Marks {
  hipEvent_t* ev = nullptr;
  int32_t* dispatches = nullptr;  // the attempt's stream dispatches, counted by the launchers (otm_get_tiers)
  void count(int n = 1) const {
    if (dispatches) *dispatches += n;
  }
  // an empty span: the slot of a kernel that was not launched keeps its name and reads ~0
  void skip(int k, hipStream_t s) const {
    begin(k, s);
    end(k, s);
  }
  void begin(int k, hipStream_t s) const {
    if (ev) (void)hipEventRecord(ev[2 * k], s);
  }
  void end(int k, hipStream_t s) const {
    if (ev) (void)hipEventRecord(ev[2 * k + 1], s);
  }
};

// ---- launch wrappers (kernels.hip)
// seg_base: DevOut::seg_base [T+1], which K1 zeroes per trace for K7a (launch_seg_bound)
void launch_columns(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, int64_t* seg_base,
                    hipStream_t s, const Marks& mk);
// Where a batch resumes after a tier's tables grew (engine_match): the stages
// before the tier that overflowed kept their results, so only that tier and
// what follows it run again (RESUME_ALL: the whole batch).
enum Resume { RESUME_ALL = 0, RESUME_CAND_BIG = 1, RESUME_TRANS_HUGE = 2, RESUME_ROUTE_HUGE = 3 };
void launch_candidates(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, hipStream_t s,
                       const Marks& mk, int from = RESUME_ALL);
void launch_links(const DevBatch& b, const DevParams& p, DevWork& w, hipStream_t s, const Marks& mk);
// index tier -> LDS search tier -> global tier, spill lists on the device
// (CTR_SEARCH_GLOBAL, CTR_INDEX_MISS and CTR_TRANS_WIDE must be zero on entry);
// the first kernel sets *w.abort when the scanned transition total exceeds w.trans_cap
void launch_transitions(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, hipStream_t s,
                        const Marks& mk, int sub, int from = RESUME_ALL);
void launch_viterbi(const DevBatch& b, DevWork& w, hipStream_t s, const Marks& mk);
void launch_route(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, hipStream_t s,
                  const Marks& mk, int from = RESUME_ALL);
void launch_segments(const DevGraph& g, const DevBatch& b, DevWork& w, DevOut& o, hipStream_t s, const Marks& mk);
// K7b: queue_length of the complete OSMLR segments launch_segments wrote, at the
// threshold kph > 0 (DESIGN.md §3 rule 7b); no timing slot of its own
void launch_queue(const DevBatch& b, DevWork& w, DevOut& o, float kph, hipStream_t s);
// K7c: one otm_matched_point per input point into out[n_points] (DESIGN.md §3
// rule 7c), after launch_seg_bound placed the interpolated points; launched
// only with the handle's switch on; no timing slot of its own
void launch_points(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, otm_matched_point* out,
                   hipStream_t s);
// K7d: one otm_traversal per traversed edge into trace t's region of tv.rec and
// their number into tv.cnt[t] (DESIGN.md §3 rule 7d), after launch_segments;
// launched only with the handle's switch on; no timing slot of its own
void launch_traversals(const DevGraph& g, const DevBatch& b, DevWork& w, DevOut& o, const DevTrav& tv, hipStream_t s);
// ... and their fetch-time compaction: off = the exclusive scan of tv.cnt
void launch_trav_compact(int32_t n_traces, const int64_t* seg_base, const int64_t* off, const otm_traversal* reg,
                         otm_traversal* dst, hipStream_t s);
// K7e: one otm_point_score per input point into sc.rec[n_points] (DESIGN.md §3
// rule 7e): a forward sweep that recomputes K5's alpha into the engine's
// scratch (the candidates' layout), a backward sweep that forms the
// through-costs and writes the records.  It reads what K3-K5 left (trans,
// trans_off, the emissions, ncand, state, chain_start) and trace_err as route
// recovery (K6, the last stage to fail a trace) left it, and writes nothing a
// pipeline kernel reads; launched only with the handle's switch on;
// no timing slot of its own.  OTM_SCORE_FORM (1: one wave per trace, 4: four
// traces per wave, one per DPP row) forces a form, as OTM_VIT_FORM does.
struct DevScores {
  otm_point_score* rec;  // [P]
  float* alpha;          // [P*KIN] alpha of the inline candidate slots
  float* alpha_x;        // [P*KX]  ... of the overflow slots
  int32_t* rej;          // [T] traces the packed form hands to the general form
  int32_t* rej_n;        // [1] their count (zeroed by the launch)
};
void launch_scores(const DevBatch& b, DevWork& w, const DevScores& sc, hipStream_t s);
// K7f: the matched shape of the traces' records as k_traversals left them in
// their regions (DESIGN.md §3 rule 7f).  write false: the per-trace vertex and
// byte counts into sh.vtx_off / sh.poly_off; write true: vertices, spans and
// polyline chars at the scanned offsets.  Fetch time only; no timing slot.
void launch_shape(const DevGraph& g, int32_t n_traces, const int64_t* seg_base, const DevTrav& tv, const DevShape& sh,
                  bool write, hipStream_t s);
void launch_report(const DevBatch& b, const DevReportCfg& rc, DevWork& w, DevOut& o, hipStream_t s, const Marks& mk);
// spatial work order: tile counts, plan (group cuts), scatter of the columns
void launch_order(const DevBatch& b, DevWork& w, hipStream_t s, const Marks& mk);
// K7a: each trace's segment bound added into tb[T] (zeroed by K1;
// scanned into DevOut::seg_base) and the interpolated points placed
void launch_seg_bound(const DevGraph& g, const DevBatch& b, const DevParams& p, DevWork& w, int64_t* tb, hipStream_t s,
                      const Marks& mk);
// fetch-time compaction of the per-trace regions into dense arrays; offsets
// are the exclusive scans of seg_cnt / way_cnt / rep_cnt
void launch_compact(int32_t n_traces, const DevOut& o, const int32_t* seg_off, const int32_t* way_off,
                    const int32_t* rep_off, otm_segment* segs_out, int64_t* ways_out, otm_report_rec* reps_out,
                    otm_trace_result* traces_out,
                    hipStream_t s);
// index build: pass 0 counts rows (row_cnt), pass 1 inserts them into the
// row tables (slot array pre-filled with 0xFF)
void launch_index_build(const DevGraph& g, const uint32_t* turn_units, uint32_t cmax, int32_t* row_cnt,
                        const IdxRow* rows, uint4* slot, bool write, hipStream_t s);
// the route index's table loads (percent): the faster one, and the denser one
// an index falls back to when the faster does not fit its HBM budget
int index_load_fast();
int index_load_dense();
void launch_row_sizes(const int32_t* row_cnt, int64_t* row_sizes, int32_t n, int pct, hipStream_t s);
constexpr int32_t GROW_HUGE = 1, GROW_CAND = 2;  // BatchStatus::grow bits (CTR_GROW_HUGE, CTR_GROW_CAND set)
struct BatchStatus {
  int32_t abort, grow;
  int64_t ttotal;
  int32_t pool_used, pool_over;  // CTR_POOL_USED, CTR_POOL_OVER
  int32_t route_huge;   // CTR_ROUTE_HUGE: the route stage reached its huge tier (else the transition stage did)
  int32_t tier_idle;    // TierGroup bits: the group's first list stayed empty this batch
  int32_t tier_wake;    // CTR_TIER_WAKE: dormant groups this attempt needed
  int32_t pad;
};
// otm_engine::snap: the spill snapshots (DevWork::snap), then k_status's staging area
struct SnapBuf {
  int32_t stage[SNAP_COUNT][CTR_STAGE_WORDS];
  BatchStatus status;
};
static_assert(offsetof(SnapBuf, status) == 192 && sizeof(SnapBuf) == 192 + 40, "snapshot buffer layout");
// otm_match_compact's inputs widened on the device (time = base + delta, accuracy as float)
void launch_expand_compact(const int64_t* trace_off, const int64_t* tbase, const int32_t* dt, const int16_t* acc16,
                           double* time, float* acc, int32_t n_traces, hipStream_t s);
// out: the device copy; host: the same record in page-locked host memory, written by the kernel itself
void launch_status(const int32_t* abort, const int64_t* ttotal, const int32_t* counters, const int32_t* snap,
                   BatchStatus* out, BatchStatus* host, hipStream_t s);
void launch_row_pack(const int32_t* row_cnt, const int64_t* row_off, IdxRow* rows, int32_t n, hipStream_t s);
// an index's per-edge source records from its packed rows and the graph's {from, length} pairs
void launch_src_pack(const DevGraph& g, const IdxRow* rows, SrcRec* src, hipStream_t s);
// the /report request bytes read on the GPU (requests.hip): per request r of
// [r0, r1) of the staged blob (bytes [off[r], off[r+1])), accepted << 40 |
// points in cnt[r] and ok[r], its points into the sparse arrays
// (req_sparse_slots entries; cnt[n] = 0 by the launch that ends at n); after
// an exclusive scan of cnt (n + 1 entries), the compaction moves the accepted
// requests' points into out's arrays and their offsets into trace_off
size_t req_sparse_slots(int32_t n, size_t bytes);
void launch_req_read(const unsigned char* blob, const int64_t* off, int32_t r0, int32_t r1, int32_t n, int64_t* cnt,
                     uint8_t* ok, const DevBatch& sparse, hipStream_t s);
void launch_req_compact(const int64_t* off, int32_t n, const int64_t* pre, const uint8_t* ok, const DevBatch& sparse,
                        const DevBatch& out, int64_t* trace_off, hipStream_t s);
// the /report response bodies written on the GPU (responses.hip) from a
// batch's dense results (engine_fetch's compaction, device side)
constexpr int RESP_HDR_SLOT = 512;  // bytes of a trace's header piece
constexpr int RESP_SEG_SLOT = 320;  // ... of a segment object, + 24 per way id (8-byte aligned)
constexpr int RESP_REP_SLOT = 192;  // ... of a datastore report object
struct RespIn {
  int32_t nt, ns, nr;
  const otm_trace_result* traces;
  const otm_segment* segs;
  const int64_t* ways;
  const otm_report_rec* reps;
};
struct RespWork {
  char *hdr, *seg, *rep;       // piece slots
  int32_t *hlen, *slen, *rlen;  // piece lengths (-1: a float the host formats)
  int64_t* blen;               // [nt + 1] body lengths, scanned in place into offsets
  uint8_t* host;               // [nt] 1: the host writes this body
};
size_t resp_seg_scratch(int32_t ns, int32_t nw);
void launch_resp_items(const RespIn& in, const RespWork& w, hipStream_t s);
void launch_resp_len(const RespIn& in, const RespWork& w, hipStream_t s);
void launch_resp_copy(const RespIn& in, const RespWork& w, const int64_t* boff, char* blob, hipStream_t s);
// K7g: trace attributes (attributes.hip, DESIGN.md §3 rule 7g): one JSON body per trace from the
// batch's optional outputs as they stand, made at the first size, fetch or device call of a batch.
// Items are the matched point objects [0, n_points) and then the edge objects [n_points, n_points +
// n_trav); a section that is off has no items (n_points or n_trav 0) and its inputs may be null.
struct DevAttr {
  uint32_t mask;              // OTM_ATTR_*
  int32_t n_traces;
  int64_t n_points, n_trav;   // items of the two kinds
  const int32_t* pt_trace;    // [P] trace of point (DevWork's, as the batch left it)
  const otm_matched_point* pts;
  const otm_point_score* scores;  // (SCORES)
  const otm_traversal* trav;      // dense, with trav_off (EDGES; trav_off also SHAPE)
  const int64_t* trav_off;
  const otm_shape_span* span;     // (EDGES and SHAPE)
  const char* poly;               // (SHAPE) with poly_off
  const int64_t* poly_off;
  int64_t* pt_off;     // [T+1] the traces' point offsets (k_attr_pt_off)
  int64_t* item_off;   // [items + 1] lengths, then the host's scan of them (element `items`: 0, then the total)
  int64_t* body_off;   // [T+1] likewise, the bodies'
  char* blob;          // [body_off[T]] (write pass only)
};
void launch_attr_pt_off(const DevAttr& a, hipStream_t s);
// write false: the item lengths (items) and body lengths (frame); write true: the bytes
void launch_attr_items(const DevAttr& a, bool write, hipStream_t s);
void launch_attr_frame(const DevAttr& a, bool write, hipStream_t s);
// exclusive scan helpers (in place over n+1 elements: out[n] = total)
void scan_i64(int64_t* d, int64_t n, void* tmp, size_t tmp_bytes, hipStream_t s);
// exclusive scans of three per-trace counts (n <= FETCH_SCAN_MAX) in one
// single-block launch, totals at o*[n]
constexpr int FETCH_SCAN_MAX = 1 << 16;
void launch_fetch_scan(int32_t n, const int32_t* c0, const int32_t* c1, const int32_t* c2, int32_t* o0, int32_t* o1,
                       int32_t* o2, hipStream_t s);
void scan_i32(int32_t* d, int64_t n, void* tmp, size_t tmp_bytes, hipStream_t s);
size_t scan_tmp_bytes(int64_t n);

}  // namespace otm
