/*
 * otmatch.h -- C ABI of libotmatch.so, the MI355X-native map matcher that
 * replaces the /report path of Open Traffic Reporter.
 *
 * What it replaces (reference = burritojustice/reporter):
 *   - the HTTP hop the Java batcher makes for every match request:
 *       String response = HttpClient.POST(url, post_body);
 *         src/main/java/org/opentraffic/reporter/Batch.java:63
 *         src/main/java/org/opentraffic/reporter/HttpClient.java:18-45
 *   - the Python service that answers it:
 *       SegmentMatcherHandler.handle_request / report
 *         py/reporter_service.py:218-240, :110-215
 *   - the Valhalla/meili matcher that service calls:
 *       valhalla.Configure(conf)          py/reporter_service.py:279
 *       valhalla.SegmentMatcher()          py/reporter_service.py:52
 *       SegmentMatcher.Match(json) -> json py/reporter_service.py:112
 *
 * Conventions: plain C types only; no exceptions cross this boundary; every
 * buffer the library returns is released with otm_free().  Status codes of
 * the request-level calls are the HTTP codes reporter_service.py would send
 * (200 / 400 / 500) and the body is byte-identical to what it would write.
 * Engine-level calls return 0 on success and a negative OTM_E* code on
 * failure, with a message available from otm_last_error().
 *
 * Thread safety: an engine handle may be used from many threads at once.
 */
#ifndef OTMATCH_H
#define OTMATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OTM_OK 0
#define OTM_EINVAL (-1)   /* bad argument / config                          */
#define OTM_EIO (-2)      /* graph file unreadable / malformed              */
#define OTM_EDEVICE (-3)  /* HIP runtime error (no device, OOM, fault)      */
#define OTM_ECONFIG (-4)  /* env config rejected (reporter_service.py:55-62) */
#define OTM_EAGAIN (-5)   /* async queue full                               */
#define OTM_ENOMEM (-6)   /* host allocation failed                         */

typedef struct otm_engine otm_engine;

/* ------------------------------------------------------------------ engine */

/* Create an engine: load the flattened graph named by the config file into
 * the HBM of devices[0] and read the matcher parameters.
 *   cfg_path: JSON file; {"otm":{"graph":"<.otmg path>"}, "meili":{"default":
 *             {sigma_z, beta, max_route_distance_factor, breakage_distance,
 *              interpolation_distance, search_radius, max_search_radius,
 *              max_candidates}}}.  Unknown keys are ignored.
 *   Env (read once, here): REPORT_LEVELS, TRANSITION_LEVELS, THRESHOLD_SEC
 *   with reporter_service.py's parsing (make_thread_locals, :51-62),
 *   including its quirk that THRESHOLD_SEC goes through strtobool: a value
 *   such as "15" is rejected with OTM_ECONFIG ("invalid truth value '15'"),
 *   where the reference's worker threads would die.
 * Replaces valhalla.Configure (py/reporter_service.py:279) + per-thread
 * SegmentMatcher() construction (:52).
 *   ndev == 1: one GPU.  ndev > 1: a multi-device engine for a host that
 *   drives several GPUs from one process (the Java host is one JVM): one
 *   member engine per entry of devices (a full graph + index replica each;
 *   a device may repeat).  Request-level calls (otm_report, otm_report_batch,
 *   otm_submit/otm_poll, otm_match_json) and the batcher send each trace to
 *   member (murmur2(uuid) & 0x7fffffff) % ndev -- Kafka's partition of the
 *   key, SURVEY.md §8(e) -- run the members concurrently and merge the
 *   results in request order; otm_match_soa splits its traces into
 *   point-balanced contiguous ranges (the binary batch carries no uuid).
 *   Device-side calls (otm_match_device, otm_hist_bind*) go to a member
 *   (otm_engine_member); info getters answer for member 0.  Multi-process
 *   runs (one engine per GPU process, RCCL reduce of the histograms) are
 *   DESIGN.md §8. */
int otm_engine_create(const char* cfg_path, const int* devices, int ndev,
                      otm_engine** out);
/* The matcher parameters a config file gives, without a device: meili's
 * "default" section with the mode's section ("meili.mode", default "auto")
 * on top, as valhalla.Configure (py/reporter_service.py:279) reads the meili
 * config.  otm_engine_create uses exactly these. */
typedef struct otm_meili_params {
  float sigma_z, beta, max_route_distance_factor, breakage_distance, interpolation_distance;
  float search_radius, max_search_radius, gps_accuracy, turn_penalty_factor;
  int32_t max_candidates;
} otm_meili_params;
int otm_config_meili(const char* cfg_path, otm_meili_params* out);
/* The queue threshold a config file gives, without a device:
 * "otm":{"queue_speed_kph": v} in km/h.  Absent or 0: off (*kph = 0, every
 * queue_length is 0 and no kernel is added to a match).  A negative,
 * non-finite or non-numeric v is OTM_EINVAL with a message, here and in
 * otm_engine_create, which uses exactly this.  otm_queue_info: the threshold
 * an engine runs with (clones and members inherit it). */
int otm_config_queue(const char* cfg_path, float* kph);
int otm_queue_info(const otm_engine* eng, float* kph);
/* Members of an engine: ndev of a multi-device engine, 1 otherwise. */
int otm_engine_members(const otm_engine* eng);
/* Member i of a multi-device engine (NULL when out of range); a one-device
 * engine is its own member 0.  Owned by eng. */
otm_engine* otm_engine_member(otm_engine* eng, int i);
/* A second batch context on the same GPU (extension): its own HIP stream and
 * work buffers over the parent's HBM-resident graph, distance index and
 * configuration.  Batches on a parent and its clones run concurrently when
 * issued from different host threads (each handle serialises its own
 * calls), so one kernel's tail overlaps the next batch's head.  Destroy
 * clones before their parent. */
int otm_engine_clone(otm_engine* eng, otm_engine** out);
void otm_engine_destroy(otm_engine* eng);

/* Last error message for this thread (eng may be NULL). */
const char* otm_last_error(const otm_engine* eng);

/* Release any buffer returned by this library. */
void otm_free(void* p);

/* ---------------------------------------------------------- request level */

/* The /report endpoint, in process.  req = the POST body the Java batcher
 * builds (Batch.java:52-61).  Returns the HTTP status (200/400/500) and sets
 * *resp to the exact body reporter_service.py would send
 * (handle_request, py/reporter_service.py:218-240; do(), :259-264).
 * Replaces HttpClient.POST(url, body) at Batch.java:63. */
int otm_report(otm_engine* eng, const char* req, size_t len, char** resp,
               size_t* resp_len);

/* Many /report requests at once: one GPU batch.  codes[i], resps[i],
 * resp_lens[i] as for otm_report.  Returns 0 or a negative engine error. */
int otm_report_batch(otm_engine* eng, int n, const char* const* reqs,
                     const size_t* lens, char** resps, size_t* resp_lens,
                     int* codes);

/* Request arenas: page-locked host memory owned by the library that a host
 * writes its request bodies into -- the Java host's body.getBytes(ISO_8859_1)
 * (HttpClient.java:26 sends those bytes) into a MemorySegment over the arena
 * instead of a heap array (Batch.java:52-63).  otm_report_batch and
 * otm_submit_batch recognise bodies inside an arena and send them to HBM
 * straight from it, in pieces as large as the bodies lying back to back
 * allow: no staging copy and no submission copy.  The caller may reuse an
 * arena once otm_report_batch returns; bodies given to otm_submit_batch must
 * stay unchanged until their results are polled (the submission holds the
 * arena, so otm_request_arena_release only gives up the caller's hold).
 * NULL on failure (otm_last_error). */
void* otm_request_arena_alloc(size_t bytes);
int otm_request_arena_release(void* arena);

/* valhalla.SegmentMatcher().Match(json) (py/reporter_service.py:112):
 * request JSON (uuid + trace) in, {"segments":[...]} JSON out.  Returns 200
 * on success, 500 with {"error":...} otherwise. */
int otm_match_json(otm_engine* eng, const char* req, size_t len, char** resp,
                   size_t* resp_len);

/* report() of reporter_service.py:110-215 on the GPU (the k_report kernel)
 * over caller-supplied Match outputs: n requests and their
 * SegmentMatcher.Match JSON.  The segments are converted to typed records and
 * the kernel's stats, shape_used and reports are written around the Match
 * output passed through, as the reference does.  codes[i] / resps[i] as
 * otm_report_segments; codes[i] = 0 with an explanation in resps[i] where a
 * Match output does not fit the typed records (a field of another JSON type
 * than the matcher emits: the host otm_report_segments reproduces Python's
 * exception for those).  Returns 0 or a negative engine error. */
int otm_report_segments_device(otm_engine* eng, int n, const char* const* reqs,
                               const size_t* lens, const char* const* match_jsons,
                               const size_t* match_lens, char** resps,
                               size_t* resp_lens, int* codes);

/* report() with a caller-supplied matcher output: runs
 * reporter_service.py:110-215 over `match_json` (what SegmentMatcher.Match
 * returned) for the request `req`.  Lets a host keep any matcher and use the
 * native post-processing.  eng may be NULL (then the env is read now). */
int otm_report_segments(otm_engine* eng, const char* req, size_t len,
                        const char* match_json, size_t match_len, char** resp,
                        size_t* resp_len);

/* Async form of otm_report for hosts that cannot block per key (the Kafka
 * Streams processor issues one blocking POST per record today,
 * BatchingProcessor.java:69).  Requests submitted before a poll are matched
 * together in one GPU batch; results for one tag come back once, results of
 * one uuid in submit order. */
typedef struct otm_result {
  uint64_t tag;
  int code;
  char* body; /* release with otm_free */
  size_t body_len;
} otm_result;
int otm_submit(otm_engine* eng, const char* req, size_t len, uint64_t tag);
/* n requests at once (a Kafka poll's records): the same as n otm_submit
 * calls in order, the bodies copied over the library's host threads.  The
 * async path is a pipeline: each worker runs whole request batches on its
 * own batch context (OTM_ASYNC_WORKERS, default 3; OTM_ASYNC_BATCH requests
 * per batch, default 16384), so one batch's parse and response writing overlap
 * another's GPU work; results are published in submit order. */
int otm_submit_batch(otm_engine* eng, int n, const char* const* reqs, const size_t* lens, const uint64_t* tags);
/* Fills up to max results; waits at most timeout_us for the first one.
 * Returns the number filled (>=0) or a negative engine error. */
int otm_poll(otm_engine* eng, otm_result* out, int max, int timeout_us);

/* Java request encoder (Batch.report + Point.Serder.put_json,
 * Batch.java:52-61, Point.java:39-45): float32 lat/lon through
 * DecimalFormat("###.######") HALF_EVEN, long time, int accuracy, in the
 * bytes HttpClient.POST sends: new StringEntity(body) is ISO-8859-1
 * (HttpClient.java:26), so the uuid -- the Kafka record key, given here as
 * its UTF-8 bytes and read as StringDeserializer reads it (JDK 8, U+FFFD for
 * malformed input) -- goes out unescaped with U+0080..U+00FF as single bytes
 * and anything above U+00FF as '?'.  Such a body is what the reference
 * service answers 400 ('utf-8' codec ...) when a Latin-1 byte breaks its
 * body.decode('utf-8') (py/reporter_service.py:99); otm_report answers it
 * the same.  *out is allocated by the library. */
int otm_encode_request(const char* uuid, int n, const float* lat,
                       const float* lon, const int64_t* time,
                       const int32_t* accuracy, char** out, size_t* out_len);

/* The points of one /report request body, as the matcher reads them
 * (parse_trace + handle_request validation, py/reporter_service.py:85-106,
 * 218-234, then each point's lat, lon, time and accuracy).  fast = 1 takes
 * the DOM-free reader of the Java batcher's own bytes and returns -2 for a
 * body outside its grammar (a request batch then takes the DOM path); fast =
 * 0 always parses the DOM.  Returns the point count (at most max_points are
 * written) with the uuid copied when it is a JSON string (NUL-terminated,
 * truncated to uuid_cap), -1 for a request the DOM path rejects. */
int otm_request_points(const char* req, size_t len, int fast, float* lat, float* lon, double* time, float* acc,
                       int max_points, char* uuid, size_t uuid_cap);

/* ----------------------------------------------------------- binary level */

/* A batch of traces, structure of arrays.  Points of trace t are
 * [trace_off[t], trace_off[t+1]).  The same struct describes host buffers
 * (otm_match_soa) or device buffers (otm_match_device). */
typedef struct otm_batch {
  int32_t n_traces;
  int64_t n_points;
  const int64_t* trace_off; /* n_traces + 1 */
  const float* lat;
  const float* lon;
  const double* time;    /* epoch seconds */
  const float* accuracy; /* metres; <= 0 means "not given" (gps_accuracy) */
} otm_batch;

/* One matched OSMLR segment (the elements of "segments", README.md:152-165). */
typedef struct otm_segment {
  int64_t segment_id;   /* -1: no OSMLR association (key omitted in JSON) */
  double start_time;    /* valid only if (flags & OTM_SEG_START_VALID)     */
  double end_time;      /* valid only if (flags & OTM_SEG_END_VALID)       */
  int32_t length;       /* metres, -1 if partially traversed               */
  int32_t queue_length; /* metres from the segment's end over which the
                           probe stayed below "queue_speed_kph" (complete
                           OSMLR segments, DESIGN.md §3 rule 7b); 0 when off */
  int32_t begin_shape_index;
  int32_t end_shape_index;
  int32_t way_off; /* into otm_results.way_ids */
  int32_t way_cnt;
  uint32_t flags;
  uint32_t pad;
} otm_segment;
#define OTM_SEG_START_VALID 1u
#define OTM_SEG_END_VALID 2u
#define OTM_SEG_INTERNAL 4u
/* start_time / end_time came from a JSON int literal (segments handed to
 * otm_report_segments_device; the matcher itself emits floats, and the int -1
 * of an invalid time is "not VALID") */
#define OTM_SEG_START_INT 8u
#define OTM_SEG_END_INT 16u

/* One datastore report (reporter_service.py:160-166). */
typedef struct otm_report_rec {
  int64_t id;
  int64_t next_id; /* -1: key absent */
  double t0;
  double t1; /* the JSON value is an int when (flags & OTM_REP_T1_INT): for
                the matcher's own segments that is the -1 of a partial next
                segment (reporter_service.py:160) */
  int32_t length;
  int32_t queue_length;
  uint32_t flags;
  uint32_t pad;
} otm_report_rec;
#define OTM_REP_T1_INT 1u
#define OTM_REP_T1_INT_MINUS1 OTM_REP_T1_INT /* the name of round 1 */
#define OTM_REP_T0_INT 2u

/* Per-trace outcome: the stats block (reporter_service.py:201-213),
 * shape_used (:125-127) and where the trace's segments/reports live. */
typedef struct otm_trace_result {
  int32_t code; /* 200, or 500 (error_kind says why) */
  int32_t error_kind;
  int32_t seg_off, seg_cnt;
  int32_t rep_off, rep_cnt;
  int32_t shape_used; /* -1 == None */
  int32_t successful_count;
  int32_t unreported_count;
  int32_t discontinuities;
  int32_t invalid_speeds;
  int32_t unassociated;
  int32_t successful_length; /* metres of the LAST counted segment, -1 none */
  int32_t unreported_length; /* ditto */
} otm_trace_result;
#define OTM_TERR_NONE 0
#define OTM_TERR_ZERODIV 1         /* "float division by zero" */
/* 2 and 3 were the 256-edge and 98,304-label spec limits until round 3;
 * round 4 has no such limits (the batch's tables grow on demand), so they
 * only report what cannot happen on a consistent graph (a finite transition
 * whose route search misses its target) or a failed host allocation */
#define OTM_TERR_CAND_OVERFLOW 2   /* (oracle) candidate workspace allocation failed */
#define OTM_TERR_SEARCH_OVERFLOW 3 /* a route search could not reproduce its transition */
#define OTM_TERR_ZERODIV_INT 4     /* "division by zero" (int / int in report()) */

/* Host-side result arrays of one batch (owned by the engine until the next
 * call on the same thread's engine, or copy them). */
typedef struct otm_results {
  int32_t n_traces;
  int32_t n_segments;
  int32_t n_reports;
  int32_t n_way_ids;
  const otm_trace_result* traces;
  const otm_segment* segments;
  const otm_report_rec* reports;
  const int64_t* way_ids;
} otm_results;

/* Match a host-resident batch; results copied back to host.  Inputs in
 * pinned memory (otm_host_alloc) go to the device by DMA at full PCIe speed;
 * pageable inputs are staged by the HIP runtime. */
int otm_match_soa(otm_engine* eng, const otm_batch* in, otm_results* out);
/* The same batch in the Java host's own types, narrowed for the link (14 B
 * per point instead of 24): Point's float lat/lon, its long time as an int32
 * delta from a per-trace int64 base (epoch seconds), its int accuracy as an
 * int16 (Point.java:16-25; Batch.java:52-61 sends exactly these integers).
 * time[i] = (double)(time_base[t] + time_delta[i]), accuracy[i] =
 * (float)accuracy16[i] -- widened on the device, results identical to
 * otm_match_soa on the widened batch.  A trace whose times span more than
 * 2^31 s or whose accuracies leave [-32768, 32767] goes through
 * otm_match_soa instead. */
typedef struct otm_batch_compact {
  int32_t n_traces;
  int64_t n_points;
  const int64_t* trace_off;  /* n_traces + 1 */
  const int64_t* time_base;  /* n_traces: epoch seconds */
  const float* lat;
  const float* lon;
  const int32_t* time_delta; /* seconds after the trace's time_base */
  const int16_t* accuracy;   /* metres; <= 0 means "not given" */
} otm_batch_compact;
int otm_match_compact(otm_engine* eng, const otm_batch_compact* in, otm_results* out);
/* Page-locked host memory for a host's batch buffers (hipHostMalloc): a Java
 * host maps it as a MemorySegment and fills its SoA arrays in place.
 * NULL on failure; release with otm_host_free (not otm_free). */
void* otm_host_alloc(size_t bytes);
void otm_host_free(void* p);

/* Match a batch whose arrays are already in this engine's device memory.
 * Results stay on the device (fetch with otm_fetch_results).  `stream` is a
 * hipStream_t (NULL = the engine's own stream); the call returns after the
 * work is enqueued and the variable-size outputs are sized. */
int otm_match_device(otm_engine* eng, const otm_batch* in_dev, void* stream);
int otm_fetch_results(otm_engine* eng, otm_results* out);
/* A stream for otm_match_device on the engine's device: own_queue != 0 gives it
 * a hardware queue of its own (a full CU mask), apart from the runtime's pool
 * of GPU_MAX_HW_QUEUES queues that every other stream of the process shares.
 * NULL on failure; release with otm_stream_destroy. */
void* otm_stream_create(otm_engine* eng, int own_queue);
void otm_stream_destroy(void* stream);

/* Matched points (extension, DESIGN.md §3 rule 7c): where on the road each
 * input point of the last binary-level batch was put -- one record per point,
 * in input point order, written on the GPU (k_points) after route recovery.
 * Off by default, per handle: with the switch off a match launches and
 * allocates nothing more.  A clone inherits its parent's value when it is
 * made; a multi-device engine passes the call to every member.
 *   edge/offset  a column with a state: its chosen candidate as the Viterbi
 *                stage holds it (a node candidate in its carried form, the
 *                node's first outgoing edge at offset 0, OTM_PT_NODE); an
 *                interpolated point inside a route step: the piece rule 7
 *                placed it on and its foot there (OTM_PT_ROUTE; OTM_PT_ANCHOR
 *                when it is one of rule 7's anchors); inside a same-edge
 *                step: its closest foot on the edge, clamped between the two
 *                states' offsets (OTM_PT_SAME_EDGE)
 *   lat/lon      the place on the edge's shape, interpolated in double
 *   distance     metres from the input point to (lat, lon)
 *   way_id       the edge's way
 * A point without a place has edge -1 and every number 0; its flags are
 * OTM_PT_COLUMN for a column (no candidates, no reachable state, or a trace
 * answered 500) and 0 for an interpolated point. */
#define OTM_PT_MATCHED 1u      /* the record has a place */
#define OTM_PT_COLUMN 2u       /* a column of the interpolation filter (rule 1) */
#define OTM_PT_NODE 4u         /* a node candidate */
#define OTM_PT_CHAIN_START 8u  /* the first state of a chain */
#define OTM_PT_ROUTE 16u       /* placed on its step's route (ipos >= 0) */
#define OTM_PT_ANCHOR 32u      /* ... and not behind an earlier placed point of the step */
#define OTM_PT_SAME_EDGE 64u   /* inside a same-edge step (forward along one edge, or a stay) */
typedef struct otm_matched_point { /* 40 bytes */
  int32_t edge;     /* directed edge id of the graph file; -1: no place */
  uint32_t flags;   /* OTM_PT_* */
  double lat, lon;  /* degrees, 0 when unmatched */
  float offset;     /* metres from the edge's start */
  float distance;   /* metres, input point to (lat, lon) */
  int64_t way_id;   /* 0 when unmatched */
} otm_matched_point;
/* otm_set_points: the switch (on != 0).  otm_points_info: its value.
 * otm_fetch_points answers for the handle's last otm_match_soa,
 * otm_match_compact or otm_match_device batch, any number of times with the
 * same bytes: *n_points records into dst[cap]; cap 0 with dst NULL only sizes
 * the call.  On a multi-device engine the members' records are joined in the
 * batch's point order.  otm_points_device: the device buffer of a one-device
 * engine (valid until its next batch), ordered behind the engine's stream.
 * OTM_EINVAL (message in otm_last_error): a NULL engine, a fetch with the
 * switch off or before any batch ran with it on, cap below the point count,
 * otm_points_device on a multi-device handle. */
int otm_set_points(otm_engine* eng, int on);
int otm_points_info(const otm_engine* eng, int* on);
int otm_fetch_points(otm_engine* eng, otm_matched_point* dst, int64_t cap, int64_t* n_points);
int otm_points_device(otm_engine* eng, const void** dev, int64_t* n_points);

/* Matched route (extension, DESIGN.md §3 rule 7d): the directed edges each
 * trace of the last binary-level batch drove, in order -- one record per
 * traversed edge, the traversals rule 7 groups into segments, written on the
 * GPU (k_traversals) after the segments.  Off by default, per handle: with the
 * switch off a match launches and allocates nothing more.  A clone inherits its
 * parent's value when it is made; a multi-device engine passes the call to
 * every member.
 *   A chain of >= 2 states gives: its first state's edge from that state's
 *   offset, every edge of every step's route whole, and its last edge up to
 *   the largest offset its states reached.  A traversal that would start on a
 *   node candidate is not emitted.  A chain of one state, a trace answered 500
 *   and a chain that never leaves a node give nothing.
 *   Inside a chain the edge's end node is the next edge's start node, and
 *   exit_time is bit-equal to the next record's enter_time and end_shape_index
 *   equals the next begin_shape_index -- except across a state on a node
 *   candidate, whose own traversal is not emitted: there the record before
 *   ends at that state's time and point, the record after begins at the last
 *   point that still stands on the node, and exit_time <= enter_time (the time
 *   the vehicle waited on the node).  Times and shape indices are the ones the
 *   trace's segments were made of.
 * Only the three binary-level calls write records.  With the switch on, a JSON,
 * request or batcher batch on the same handle launches and allocates nothing
 * for them; where it uses the handle's own buffers (as any failed batch does)
 * it leaves nothing to fetch until the next binary-level batch: a fetch then
 * answers OTM_EINVAL, never another batch's records. */
#define OTM_TV_CHAIN_START 1u    /* the first emitted traversal of a chain */
#define OTM_TV_CHAIN_END 2u      /* the last one */
#define OTM_TV_FROM_START 4u     /* begin_offset == 0 */
#define OTM_TV_TO_END 8u         /* end_offset is the edge's length, bit for bit */
#define OTM_TV_INTERNAL 16u      /* an internal (intersection) edge without OSMLR segment: its otm_segment's OTM_SEG_INTERNAL */
#define OTM_TV_SEGMENT_FIRST 32u /* it starts a new otm_segment */
typedef struct otm_traversal { /* 56 bytes */
  int32_t edge;               /* directed edge id of the graph file */
  uint32_t flags;             /* OTM_TV_* */
  float begin_offset;         /* metres from the edge's start; 0 except on a chain's first traversal */
  float end_offset;           /* the edge's length (bit-equal) except on a chain's last traversal */
  double enter_time, exit_time;
  int32_t begin_shape_index, end_shape_index; /* trace-relative, as otm_segment's */
  int32_t segment;            /* which of the trace's segments it was grouped into:
                                 otm_results.segments[traces[t].seg_off + segment] */
  int32_t pad;                /* 0 */
  int64_t way_id;
} otm_traversal;
/* otm_set_traversals: the switch (on != 0).  otm_traversals_info: its value.
 * otm_traversals_size: the trace count and the record count of the batch the
 * fetch answers for -- trav_off needs *n_traces + 1 elements, dst *n; a caller
 * that does not know which batch the handle ran last (a member of a
 * multi-device engine: its share of the group's batch) sizes from this.
 * otm_fetch_traversals answers for the handle's last otm_match_soa,
 * otm_match_compact or otm_match_device batch, any number of times with the
 * same bytes: *n records, dense and in trace order, into dst[cap], trace t's at
 * [trav_off[t], trav_off[t + 1]) (trav_off[n_traces + 1], may be NULL); cap 0
 * with dst NULL only sizes the call.  On a multi-device engine the members'
 * records are joined in the batch's trace order (segment and the shape indices
 * are trace-relative: nothing is rebased).  otm_traversals_device: the dense
 * device arrays of a one-device engine (valid until its next batch), ordered
 * behind the engine's stream.  OTM_EINVAL (message in otm_last_error): a NULL
 * engine, a size or fetch call with the switch off or with no binary-level
 * batch with it on as the handle's last batch, cap
 * below the record count, otm_traversals_device on a multi-device handle. */
int otm_set_traversals(otm_engine* eng, int on);
int otm_traversals_info(const otm_engine* eng, int* on);
int otm_traversals_size(otm_engine* eng, int64_t* n_traces, int64_t* n);
int otm_fetch_traversals(otm_engine* eng, otm_traversal* dst, int64_t cap, int64_t* trav_off, int64_t* n);
int otm_traversals_device(otm_engine* eng, const void** recs, const int64_t** trav_off, int64_t* n);

/* Match scores (extension, DESIGN.md §3 rule 7e): how sure each matched point
 * of the last binary-level batch is -- one record per input point, in input
 * point order, written on the GPU (k_scores) beside the matched points.  The
 * numbers are min-sum max-marginals of the Viterbi stage's own chain, in its
 * cost units (not a probability: exp(-margin) is the caller's to form), in f32.
 * Off by default, per handle: with the switch off a match launches and
 * allocates nothing more.  A clone inherits its parent's value when it is made;
 * a multi-device engine passes the call to every member.
 *   cost        the cost of the best complete path of the point's chain
 *               through its chosen state
 *   margin      by how much the best complete path through any other state
 *               of the column costs more (floored at +0; +inf with
 *               OTM_SC_ALONE when no other state has a finite one)
 *   chain_cost  the chain's Viterbi minimum; at the chain's last column cost
 *               is bit-equal to it
 *   emission    the chosen state's emission cost
 *   transition  the cost of the step from the previous column's chosen state
 *               (0 at a chain's first column); folding a chain's records in
 *               order as ((em0 + tr1) + em1) + tr2 ... in f32 gives chain_cost
 *               bit for bit
 *   alt_edge / alt_offset  the runner-up candidate (the lowest state that
 *               attains the margin) as the Viterbi stage holds it: on a two-way
 *               street often the opposite directed edge of the same way
 *   ncand, state, alt  the column's candidate count, the chosen state and the
 *               runner-up's state (-1 when alone)
 * Every other point -- an interpolated point, a column without a state, any
 * point of a trace answered 500 -- has an all-zero record with flags 0, alt -1
 * and alt_edge -1.
 * Only the three binary-level calls write records; any other batch on the
 * handle, and any failed one, ends the last batch's records: a fetch then
 * answers OTM_EINVAL, never another batch's records. */
#define OTM_SC_SCORED 1u       /* the record is scored */
#define OTM_SC_CHAIN_START 2u  /* first column of its chain */
#define OTM_SC_CHAIN_END 4u    /* last column of its chain */
#define OTM_SC_ALONE 8u        /* no other state has a finite through-cost */
#define OTM_SC_TIE 16u         /* margin == 0 */
typedef struct otm_point_score { /* 32 bytes */
  float cost, margin, chain_cost, emission, transition;
  int32_t alt_edge;
  float alt_offset;
  uint8_t flags, ncand;
  int8_t state, alt;
} otm_point_score;
/* otm_set_scores: the switch (on != 0).  otm_scores_info: its value.
 * otm_fetch_scores answers for the handle's last otm_match_soa,
 * otm_match_compact or otm_match_device batch, any number of times with the
 * same bytes: *n_points records into dst[cap]; cap 0 with dst NULL only sizes
 * the call.  On a multi-device engine the members' records are joined in the
 * batch's point order.  otm_scores_device: the device buffer of a one-device
 * engine (valid until its next batch), ordered behind the engine's stream.
 * OTM_EINVAL (message in otm_last_error): a NULL engine, a fetch with the
 * switch off or with no binary-level batch with it on as the handle's last
 * batch, cap below the point count, otm_scores_device on a multi-device
 * handle. */
int otm_set_scores(otm_engine* eng, int on);
int otm_scores_info(const otm_engine* eng, int* on);
int otm_fetch_scores(otm_engine* eng, otm_point_score* dst, int64_t cap, int64_t* n_points);
int otm_scores_device(otm_engine* eng, const void** dev, int64_t* n_points);

/* Matched shape (extension, DESIGN.md §3 rule 7f): the geometry of the route
 * each trace of the last binary-level batch was matched to -- per trace one
 * vertex list in microdegrees, one span of it per traversal, and one polyline6
 * string, all made on the GPU (k_shape) from the trace's rule-7d records and
 * the graph's shape points.  Off by default, per handle: with the switch off
 * nothing is launched or allocated; with it on, a binary-level match also runs
 * k_traversals (whether or not otm_set_traversals is on: that call keeps its
 * own switch), and everything else happens at the first size, fetch or device
 * call for the batch.  A clone inherits its parent's value when it is made; a
 * multi-device engine passes the call to every member.
 *   Per trace, in record order: a record with OTM_TV_CHAIN_START emits the
 *   point of its edge at begin_offset (rule 7c's coordinate); a record without
 *   it emits no first vertex, the previous record's last vertex is its first.
 *   Then the edge's shape points 1..m-1 whose cumulative length lies strictly
 *   between begin_offset and end_offset, then always the point at end_offset.
 *   lat_e6 = (int32)rint(lat * 1e6), lon_e6 alike (round half even).
 *   A span's begin_vertex / end_vertex are trace-relative indices of the
 *   record's first and last vertex: end_vertex > begin_vertex; inside a chain
 *   begin_vertex equals the previous end_vertex, a chain start has the previous
 *   end_vertex + 1 (0 on the trace's first record).
 *   The polyline is the usual polyline6 over the whole vertex list (lat, then
 *   lon; deltas from (0, 0); zigzag; 5-bit groups low first; + 63), without a
 *   terminator; a chain break is a large delta.  A value takes at most 6 chars.
 *   A trace without records has no vertices and an empty string.
 * Validity is the matched route's own: only the three binary-level calls leave
 * a shape; any batch in the handle's buffers ends the last one's. */
typedef struct otm_shape_vertex { int32_t lat_e6, lon_e6; } otm_shape_vertex;        /* 8 bytes */
typedef struct otm_shape_span { int32_t begin_vertex, end_vertex; } otm_shape_span; /* 8 bytes, one per traversal,
                                                                                        in otm_fetch_traversals' order */
typedef struct otm_shape_sizes { int64_t n_traces, n_traversals, n_vertices, n_bytes; } otm_shape_sizes;
typedef struct otm_shape_out { /* any pointer may be NULL: that part is not copied */
  otm_shape_vertex* vertices; int64_t vertices_cap; int64_t* vtx_off;  /* [n_traces + 1] */
  otm_shape_span* spans;      int64_t spans_cap;    int64_t* trav_off; /* [n_traces + 1] */
  char* polyline;             int64_t polyline_cap; int64_t* poly_off; /* [n_traces + 1] */
} otm_shape_out;
/* otm_set_shape: the switch (on != 0).  otm_shape_info: its value.
 * otm_shape_size: the counts of the batch the fetch answers for.
 * otm_fetch_shape answers for the handle's last otm_match_soa,
 * otm_match_compact or otm_match_device batch, any number of times with the
 * same bytes: trace t's vertices at [vtx_off[t], vtx_off[t + 1]), its spans at
 * [trav_off[t], trav_off[t + 1]) (otm_fetch_traversals' own offsets), its
 * string at [poly_off[t], poly_off[t + 1]).  On a multi-device engine the
 * members' arrays are joined in the batch's trace order (only the three offset
 * arrays are rebased).  otm_shape_device: the device arrays of a one-device
 * engine (valid until its next batch), ordered behind the engine's stream; the
 * caps of *dev are set to the counts.  OTM_EINVAL (message in otm_last_error):
 * a NULL engine or argument, a call with the switch off or with no
 * binary-level batch with it on as the handle's last batch, a cap below its
 * count, otm_shape_device on a multi-device handle. */
int otm_set_shape(otm_engine* eng, int on);
int otm_shape_info(const otm_engine* eng, int* on);
int otm_shape_size(otm_engine* eng, otm_shape_sizes* out);
int otm_fetch_shape(otm_engine* eng, const otm_shape_out* dst);
int otm_shape_device(otm_engine* eng, otm_shape_out* dev, otm_shape_sizes* n);

/* Trace attributes (extension, DESIGN.md §3 rule 7g): the four outputs above as
 * text -- one JSON body per trace of the last binary-level batch, made on the
 * GPU (attributes.hip) from the batch's records as they stand, delivered as one
 * dense char blob with per-trace offsets, so a caller needs no struct layout.
 * The rule decides nothing new: a body is a pure function of the trace's
 * otm_matched_point, otm_point_score and otm_traversal records, its
 * otm_shape_span records and polyline, and the section mask.  Off by default
 * (mask 0), per handle: with it off nothing is launched or allocated; with it
 * on, a binary-level match also runs k_points (OTM_ATTR_POINTS), k_scores
 * (OTM_ATTR_SCORES) and k_traversals (OTM_ATTR_EDGES or OTM_ATTR_SHAPE), whether
 * or not their own switches are on (those keep their own answers), and
 * everything else happens at the first size, fetch or device call for the
 * batch.  A clone inherits its parent's mask when it is made; a multi-device
 * engine passes the call to every member.
 *   Body, without whitespace, keys in this order, a section whose bit is off
 *   absent with its comma:
 *     {"matched_points":[MP,...],"edges":[E,...],"shape":"S"}
 *   MP, one per input point in input order: with OTM_PT_MATCHED
 *     {"type":T,"edge_id":i,"way_id":i,"lat":F6,"lon":F6,"distance_along_edge":F3,
 *      "distance_from_trace_point":F3,"flags":i}
 *   T "matched" with OTM_PT_COLUMN, else "interpolated"; without OTM_PT_MATCHED
 *     {"type":"unmatched","flags":i}
 *   and, with OTM_ATTR_SCORES and OTM_SC_SCORED in the point's score record,
 *   before the closing brace
 *     ,"score":{"cost":F6,"margin":F6,"chain_cost":F6,"emission":F6,"transition":F6,
 *      "ncand":i,"state":i,"alt":i,"alt_edge":i,"alt_offset":F3,"flags":i}
 *   E, one per traversal in otm_fetch_traversals' order:
 *     {"id":i,"way_id":i,"begin_offset":F3,"end_offset":F3,"enter_time":F3,"exit_time":F3,
 *      "begin_shape_index":i,"end_shape_index":i,"segment":i,"flags":i}
 *   with OTM_ATTR_SHAPE also ,"begin_vertex":i,"end_vertex":i before ,"flags".
 *   S: the trace's polyline6 string, each backslash (byte 92) doubled.
 *   i: a decimal integer.  F3(x), F6(x): x widened to double; v = x * 1000.0 (or
 *   x * 1e6), one double product; !(fabs(v) < 2^53) gives null (NaN, the
 *   infinities: the margin of OTM_SC_ALONE); else n = (int64)rint(v), round half
 *   even; the text is '-' when n < 0, |n| / 10^d, '.', |n| % 10^d in d digits
 *   (-0.0004 -> 0.000, -0.0015 -> -0.002, 12 -> 12.000).
 * Validity: only the three binary-level calls leave attributes; any later
 * batch on the handle, any JSON-level call on it and any failed batch end them:
 * a call then answers OTM_EINVAL, never another batch's bodies. */
#define OTM_ATTR_POINTS 1u /* "matched_points" */
#define OTM_ATTR_SCORES 2u /* ... with "score" objects; needs OTM_ATTR_POINTS */
#define OTM_ATTR_EDGES 4u  /* "edges" */
#define OTM_ATTR_SHAPE 8u  /* "shape", and the edges' vertex spans */
#define OTM_ATTR_ALL 15u
/* otm_set_attributes: the section mask (0: off) that the handle's next batches
 * run with.  A batch's bodies are made from the mask the batch ran with: a mask
 * set between a batch and its first size, fetch or device call changes nothing
 * of that batch's bodies (mask 0 there answers OTM_EINVAL, "off", as the other
 * switches do).  A bad mask is OTM_EINVAL on any handle, NULL too.
 * otm_attributes_info: the handle's mask (mask not NULL).
 * otm_attributes_size: the trace count and the blob's bytes of the batch the
 * fetch answers for (neither pointer NULL).  otm_fetch_attributes answers for the handle's
 * last otm_match_soa, otm_match_compact or otm_match_device batch, any number of
 * times with the same bytes: trace t's body at [body_off[t], body_off[t + 1])
 * of dst[cap] (body_off[n_traces + 1], may be NULL), no terminator and nothing
 * between bodies; cap 0 with dst NULL only sizes the call.  On a multi-device
 * engine the members' bodies are joined in the batch's trace order (only
 * body_off is rebased).  otm_attributes_device: the device arrays of a
 * one-device engine (valid until its next batch), ordered behind the engine's
 * stream.  otm_debug_attr_fixed: F3 (decimals 3) or F6 (6) of x into out (at
 * least 24 bytes, NUL-terminated), the length returned; the host face of the
 * formatter the GPU runs.  OTM_EINVAL (message in otm_last_error): a NULL
 * engine or argument, a mask with a bit above OTM_ATTR_ALL or with
 * OTM_ATTR_SCORES without OTM_ATTR_POINTS (the mask then stays as it was), a
 * size, fetch or device call with the mask 0 or with no binary-level batch with
 * it on as the handle's last batch, cap below the byte count,
 * otm_attributes_device on a multi-device handle, decimals other than 3 or 6. */
int otm_set_attributes(otm_engine* eng, uint32_t mask);
int otm_attributes_info(const otm_engine* eng, uint32_t* mask);
int otm_attributes_size(otm_engine* eng, int64_t* n_traces, int64_t* n_bytes);
int otm_fetch_attributes(otm_engine* eng, char* dst, int64_t cap, int64_t* body_off, int64_t* n_bytes);
int otm_attributes_device(otm_engine* eng, const char** dev, const int64_t** body_off, int64_t* n_traces,
                          int64_t* n_bytes);
int otm_debug_attr_fixed(double x, int decimals, char* out);

/* Per-segment speed histogram, accumulated on the device by every match
 * call: counts u32[n_segments * nbins], bin = floor(kph / bin_kph) clamped to
 * nbins-1, one count per datastore report.  The buffer is CALLER-owned device
 * memory (e.g. a torch tensor) so the host can reduce it across GPUs with
 * RCCL.  Pass NULL to stop accumulating. */
int otm_hist_bind(otm_engine* eng, void* dev_counts, int nbins, float bin_kph);
/* The same, with a second channel beside the counts: the sum
 * of the reports' speeds per segment, u64[n_segments] in units of 1/1000
 * km/h (fixed point, so sums are exact and independent of the order the
 * GPU adds them in), also caller-owned device memory.  A binding reaches the
 * engine's clones at their next batch. */
int otm_hist_bind_ex(otm_engine* eng, void* dev_counts, int nbins, float bin_kph,
                     void* dev_speed_sum);

/* ------------------------------------------------------ the datastore flush
 * What becomes of the histogram: the body a reporter POSTs to DATASTORE_URL
 * (a TODO in the reference, docker-compose.yml:17; here the format of
 * reporter_amd/datastore.py, serialize(flush_records(...)), which these calls
 * replace for a host without Python).  Compact JSON, rows ascending, only rows
 * whose bins sum to more than 0, never a row at or past n_segments (padding
 * rows carry no id):
 *   {"mode":"auto","bin_kph":<repr>,"rank":R,"world":W,"segments":[
 *    {"id":<u64>,"count":<sum of bins>,"speed_sum_kph":<repr(sum/1000.0)>,
 *     "bins":[b0,...,b(nbins-1)]},...]}
 * bin_kph is the float widened to double and written as Python's repr, as is
 * (double)sum / 1000.0 (bit-identical to Python's int / float for every u64).
 * The slice is rank `rank` of `world`: `rows` = S_pad / world rows, slice row k
 * being global row rank * rows + k.  Preconditions: bins are read as u32; the
 * Python definition is stated for bins below 2^31 (it goes through int32
 * tensors).  *body is NUL-terminated (the NUL not counted in *body_len) and
 * released with otm_free; n_records may be NULL.  Errors: OTM_EINVAL with a
 * message in otm_last_error (NULL pointers, nbins < 1, bin_kph <= 0,
 * world < 1, rank outside [0, world)). */

/* The body written on the host: no GPU, no engine (a host that reduced its
 * histograms on the CPU; also what the device writer falls back to).  Total:
 * every double a u64 / 1000.0 can give is written as repr writes it, the
 * exponent form from 1e16 up included.  counts u32[rows * nbins], speed_sum
 * u64[rows], segment_ids u64[n_segments] in host memory. */
int otm_flush_body_host(const uint32_t* counts, const uint64_t* speed_sum,
                        const uint64_t* segment_ids, int64_t n_segments,
                        int64_t rows, int nbins, float bin_kph, int rank, int world,
                        char** body, size_t* body_len, int64_t* n_records);
/* The same bytes from a slice in device memory (what flush.reduce_histograms
 * returns, or a whole window with world 1), written on the GPU: one read of
 * the slice, the records formatted and packed there, and only the body's bytes
 * copied to the host; one host sync.  The ids are the engine's own HBM copy of
 * the graph's; a multi-device engine answers with member 0's graph, or with
 * the member on whose device the buffers lie.  `stream` is a hipStream_t the
 * buffers are ready on (NULL: the engine's own).  nbins at most 64 on this
 * path (OTM_EINVAL past it; otm_flush_body_host has no limit).  A speed sum of
 * 2^52 x 1000 or more is outside the GPU float writer's range: the slice is
 * then copied to the host and written there -- the same bytes, slower.  The
 * call serialises with the engine's batches; its scratch stays with the engine
 * at the size it grew to.  Sizing HBM: that scratch is one record slot per row
 * of the slice whatever the window's density -- rows x (108 + 11 x nbins)
 * bytes, rounded up to 8 per slot (288 B a row at 16 bins: 279 MB for 968k
 * rows; 816 B a row at 64 bins) -- plus 8 bytes a row of lengths and a blob
 * of the largest body seen. */
int otm_flush_body_device(otm_engine* eng, const void* dev_counts,
                          const void* dev_speed_sum, int64_t rows, int nbins,
                          float bin_kph, int rank, int world, void* stream,
                          char** body, size_t* body_len, int64_t* n_records);

/* Engine-owned windows: the histogram in library-owned device memory, for a
 * host that cannot allocate any (a JVM).  otm_window_begin allocates zeroed
 * counts and speed sums for the engine's segments and binds them exactly as
 * otm_hist_bind_ex would (clones pick the binding up at their next batch); on
 * a multi-device engine one pair per member, on that member's device (the
 * public otm_hist_bind* keep refusing a multi-device engine).
 * otm_window_flush closes the window: it waits for the work of the engine's
 * devices, adds the members' pairs into member 0's on the GPU (a member on
 * another device arrives by a peer copy), writes the body of the whole window
 * (rank 0, world 1) as otm_flush_body_device does, zeroes every buffer, and
 * the window goes on.  CONTRACT: no match call may be in progress on the
 * engine, its clones or its members during otm_window_flush -- close a window
 * between batches.  otm_window_end unbinds and frees; otm_engine_destroy ends
 * an open window.  OTM_EINVAL (message in otm_last_error): begin on a clone,
 * begin while a window is open or while a caller's otm_hist_bind binding is in
 * place, otm_hist_bind* of a buffer while a window is open, flush or end
 * without a window, nbins < 1, bin_kph <= 0, nbins past the device writer's
 * limit (64), and any of the three calls on a member handle of a multi-device
 * engine (otm_engine_member): a member's window belongs to the group's handle.
 * otm_hist_bind* with a NULL buffer stays allowed while a window is open, on
 * the engine or on a member: it unbinds the window's buffers, so counting
 * stops silently until the window is ended and begun again; the buffers stay
 * allocated and otm_window_flush keeps answering from them. */
int otm_window_begin(otm_engine* eng, int nbins, float bin_kph);
int otm_window_flush(otm_engine* eng, char** body, size_t* body_len, int64_t* n_records);
int otm_window_end(otm_engine* eng);

/* Pair windows: a second, independent kind of window.  Where the histogram
 * window keeps one row per segment, a pair window keeps, per (time bucket,
 * segment, next segment), the count, summed duration, summed queue_length and
 * first / last time of the datastore reports, in a hash table in HBM that the
 * report kernel fills as it writes the reports (errors contribute nothing; a
 * batch redone for a capacity counts once).  The definition is
 * reporter_amd/datastore.py's serialize(pair_records(...)):
 *   admission   the histogram's: t1 not the int -1 of a partial next segment,
 *               length / (t1 - t0) * 3.6 >= 0 in float64, an id of the graph;
 *               anything else is ignored and counted nowhere
 *   bucket      k = floor(t0 / bucket_s) - origin / bucket_s; an admitted
 *               report with k outside [0, 4096) only adds 1 to out_of_range
 *   key         (k, row(id), row(next_id) or none); records ascend by it, "no
 *               next" first
 *   body        {"mode":"auto","bucket_s":B,"origin":O,"privacy":P,"pairs":[
 *                {"id":I,"next_id":N,"bucket":O+k*B,"count":C,"duration_ms":D,
 *                 "length":L,"queue_length":Q,"t_min":a,"t_max":b},...]}
 *               duration_ms the sum of int((t1 - t0) * 1000.0 + 0.5), t_min /
 *               t_max the least floor(t0) / greatest floor(t1), "next_id"
 *               omitted when the report had none.  All integers: no sum
 *               depends on the order of arrival.
 *   privacy     keys with count < privacy stay out of the body and are counted
 *               in suppressed_keys / suppressed_reports
 * max_keys 0 means max(65536, 8 x n_segments).  The table holds at most
 * max_keys distinct keys (on a multi-device engine: each member's table) and
 * does not grow: an admitted, in-range report whose key is new when the table
 * is full adds 1 to `dropped` and nothing else -- which reports drop depends
 * on arrival order; dropped > 0 says the window was sized too small.  HBM:
 * 56 bytes per slot, slots the power of two >= 2 x max_keys; the flush's
 * scratch is 304 bytes per key of max_keys (272 of them a record's slot) plus
 * the sort's.
 * The contract is otm_window_*'s: the binding lives on the parent engine and
 * reaches clones at their next batch; a multi-device engine keeps one table per
 * member on that member's device and the flush merges them on member 0's; no
 * match call may be in progress during otm_pairs_flush; a flush clears the
 * table and the window goes on; otm_engine_destroy ends an open pair window.
 * A histogram window and a pair window may be open together and do not know
 * of each other.  otm_report_segments_device does not feed a pair window.
 * otm_pairs_add_reports runs host records (reports obtained elsewhere: another
 * matcher, a replay) through the same device upsert: id and next_id are mapped
 * to rows on the host, a next_id with no row counts as "no next", an id with no
 * row is not admitted.  On a multi-device engine they go to member 0's table.
 * otm_pairs_flush: *body NUL-terminated (the NUL not counted), released with
 * otm_free; stats may be NULL.  otm_pairs_info: the open window's
 * configuration (max_keys resolved) and one table's slot count.
 * OTM_EINVAL (message in otm_last_error): a NULL cfg, bucket_s < 1,
 * privacy < 1, origin < 0, origin % bucket_s != 0, max_keys < 0 or past 2^30
 * (otm_pairs_cfg_check: no device, no engine); begin on a graph with more than
 * 2^26 - 2 segments, on a clone, on a member handle, or while a pair window is
 * open; add, flush, end or info without one. */
typedef struct otm_pairs_cfg {
  int32_t bucket_s;
  int32_t privacy;
  int64_t origin;
  int64_t max_keys;
} otm_pairs_cfg;
typedef struct otm_pairs_stats {
  int64_t reports; /* admitted and aggregated */
  int64_t keys;
  int64_t records;
  int64_t suppressed_keys;
  int64_t suppressed_reports;
  int64_t out_of_range;
  int64_t dropped;
} otm_pairs_stats;
int otm_pairs_cfg_check(const otm_pairs_cfg* cfg);
int otm_pairs_begin(otm_engine* eng, const otm_pairs_cfg* cfg);
int otm_pairs_add_reports(otm_engine* eng, int64_t n, const otm_report_rec* recs);
int otm_pairs_flush(otm_engine* eng, char** body, size_t* body_len, otm_pairs_stats* stats);
int otm_pairs_end(otm_engine* eng);
int otm_pairs_info(const otm_engine* eng, otm_pairs_cfg* cfg, int64_t* slots);

int otm_graph_info(const otm_engine* eng, int64_t* n_nodes, int64_t* n_edges,
                   int64_t* n_segments);

/* The bounded route index built at engine creation (config
 * "otm":{"index_radius_m": R}, 0 = none; absent: sized from the graph's node
 * density, ~140 nodes per row, capped at max_route_distance_factor x
 * breakage_distance, and shrunk to fit half the free HBM): for every search
 * source (an edge's end entered along it, or a node), every label within R
 * road metres with its cost, distance, turn units and predecessor.
 * Transition and route queries whose bound 5 x gc exceeds R, or whose row
 * overflowed the builder, run the online bounded search instead; the results
 * are identical either way. */
int otm_index_info(const otm_engine* eng, float* rmax, int64_t* entries,
                   int32_t* incomplete_rows, float* build_ms);

/* The near indexes: the same rows at smaller radii (config
 * "otm":{"index_near_m": [r, ...]}, [] = none; absent: one at 0.45 R when the
 * index's tables reach 16 GB).  A transition or route query probes the
 * smallest whose radius covers its bound, so its probes land in smaller
 * tables; results are identical.  Writes up to `cap` radii (smallest first)
 * and entry counts; returns the number of near indexes, or < 0 on error. */
int otm_index_levels(const otm_engine* eng, float* radii, int64_t* entries, int cap);

/* The route index's device tables, full and near indexes together: hash
 * slots and the index's bytes (16 B a slot, the label's predecessor inside,
 * plus each index's per-edge source records, 48 B an edge), and
 * the full index's table load in percent -- 30 when the tables fit half the
 * free HBM (53 B per entry), else 40 (40 B per entry) before the radius is
 * cut. */
int otm_index_tables(const otm_engine* eng, int64_t* slots, int64_t* bytes, int32_t* load_pct);

/* The candidate search's grid index on the device: the graph file's cells
 * (meili's 500 per 0.25 deg tile) merged mult x mult (config
 * "otm":{"grid_mult": m} or env OTM_GRID_MULT; absent or 0: chosen from the
 * graph's entry density and the search radius).  Coarser cells change how
 * many cells and entries a probe visits, never the candidates. */
int otm_grid_info(const otm_engine* eng, double* cell_deg, int32_t* rows, int32_t* cols,
                  int64_t* entries, int32_t* mult);

/* Work counters of the last batch (for the roofline's algorithmic bytes). */
typedef struct otm_work_counters {
  int64_t points, columns, cells_visited, cell_entries_scanned, candidates;
  int64_t searches, nodes_settled, edges_relaxed, transitions; /* K4 */
  int64_t route_searches, route_nodes_settled, route_edges_relaxed, route_edges; /* K6 */
  int64_t segments_out, reports_out;
} otm_work_counters;
/* Enable (1) or disable (0) counting; counting runs extra atomics, so timed
 * runs keep it off. */
int otm_set_counting(otm_engine* eng, int on);
int otm_get_counters(otm_engine* eng, otm_work_counters* out);

/* Per-stage timings (ms) of the last otm_match_device call, from HIP events
 * on the engine stream: [columns, candidates, trans_size, transitions,
 * viterbi, route, segments, report].  Enabled with otm_set_timing. */
int otm_set_timing(otm_engine* eng, int on);
int otm_get_stage_ms(otm_engine* eng, float* ms, int n);

/* Per-kernel timings (ms) of the last otm_match_device call (same HIP events,
 * one pair around each launch; enabled with otm_set_timing).  Kernel k is
 * named by otm_kernel_name(k), 0 <= k < OTM_NUM_KERNELS; the stage timings
 * above are sums of these. */
#define OTM_NUM_KERNELS 18
int otm_get_kernel_ms(otm_engine* eng, float* ms, int n);
const char* otm_kernel_name(int k);

/* How much work of the last batch each fallback tier took:
 * probes the lane candidate tier handed to the wave tier; transition columns
 * the route index could not answer (trans_online), then those the LDS wave
 * search spilled to the global-memory search (trans_global); the same for the
 * route stage's steps.  trans_wave / route_wave are kept for the layout and
 * equal trans_online / route_online: every online search starts in the LDS
 * wave tier since round 3 (the lane-per-search tier is gone). */
typedef struct otm_spill_stats {
  int32_t cand_wave;
  int32_t trans_online, trans_wave, trans_global;
  int32_t route_online, route_wave, route_global;
  /* round 4, no spec limits: probes with more distinct edges in their radius
   * than the LDS tier holds (cand_big), searches past the global tier's
   * label limit (trans_huge / route_huge), and how many times the batch was
   * run to size its buffers and tables (attempts, 1 = no redo) */
  int32_t cand_big, trans_huge, route_huge, attempts;
  /* round 6: of those runs, how many resumed from the tier whose tables grew
   * (the stages before it kept their results) instead of redoing the batch */
  int32_t resumed;
} otm_spill_stats;
/* The stats (like otm_get_stage_ms / otm_get_kernel_ms / otm_get_counters)
 * describe the last batch run on this handle's own batch context.  An
 * otm_report_batch of 4,096 requests or more runs its two halves on the
 * engine's clones, and otm_submit / otm_submit_batch run on the async
 * pipeline's clones: those batches do not update the handle's figures (each
 * clone keeps its own, and grows its own on-demand tier tables). */
int otm_get_spill_stats(otm_engine* eng, otm_spill_stats* out);

/* Tiers on demand: five groups of kernel launches exist only
 * for work an earlier kernel hands them through a device list -- bit 0 the
 * candidate HBM tier, bit 1 the online transition tiers, bit 2 the online
 * route tiers, bit 3 the Viterbi list passes, bit 4 the large segment plan.
 * A batch context stops launching a group whose list stayed empty two
 * completed batches in a row; a batch that then needs it is run again with
 * the group live, and the group stays live for the context's life
 * (OTM_TIERS_ALWAYS=1 in the environment: every group is always launched).
 * Read-only: *dormant_mask the groups this handle's own context does not
 * launch now, *dispatches the stream dispatches (kernels, scans' two, memsets)
 * of its last batch's final attempt, the optional outputs' kernels apart.
 * Either pointer may be NULL. */
#define OTM_TIER_CAND_BIG 1
#define OTM_TIER_TRANS_ONLINE 2
#define OTM_TIER_ROUTE_ONLINE 4
#define OTM_TIER_VIT_LISTS 8
#define OTM_TIER_SEG_LARGE 16
int otm_get_tiers(otm_engine* eng, int32_t* dormant_mask, int32_t* dispatches);

/* Stage outputs of the last batch, for parity tests (device -> host copy).
 * what: 0 ncand i32[P], 1 cand_edge i32[P*KMAX], 2 cand_off f32[P*KMAX],
 * 3 cand_emis f32[P*KMAX], 4 trans_off i64[P+1], 5 trans f32[total],
 * 6 state i32[P], 7 col_prev i32[P], 8 route_dist f32[P], 9 gc f32[P],
 * 10 ipos f32[P]; the batch inputs as the GPU request reader decoded them
 * (otm_report_batch; also a host batch of more than 2^18 points): 11 trace_off
 * i64[T+1], 12 lat f32[P], 13 lon f32[P], 14 time f64[P], 15 accuracy f32[P];
 * 16 chain_start u8[P], 17 is_col u8[P]; the spatial work order, each valid
 * only after a batch that ran the large plan (at least OTM_SMALL_POINTS
 * points): 18 its items i32[columns] (the column points in walk order), 19
 * the tile u16[P] (its Hilbert index; written for columns only), 20 the group
 * starts i32[9]. */
int otm_debug_fetch(otm_engine* eng, int what, void* dst, size_t bytes,
                    size_t* needed);
int otm_kmax(void);
/* The GPU response writer's float formatting run on the host (test hooks):
 * Python's repr of d into out (>= 32 bytes), its length or -1 where the
 * writer leaves a body to the host writer; py_round3 as report() rounds
 * lengths, 1 or 0 (unsupported). */
int otm_debug_py_repr(double d, char* out);
int otm_debug_py_round3(double x, double* out);
/* Test hook: the response arenas' otm_free under contention from threads
 * (each round: every thread cuts bodies from an arena, then all free a
 * strided share of everyone's, with plain allocations through the same
 * scan).  Returns the arenas left live after (0 expected), -1 on bad args. */
int otm_debug_arena_stress(int threads, int rounds);
/* Test hook: the chunks eng's last otm_report_batch was split into (one per
 * batch context, run concurrently; 1: not split). */
int otm_debug_last_split(const otm_engine* eng);
/* Which HIP runtime this library is bound to ("<path> hip_runtime_version=N"):
 * a host that also runs torch must load torch first so both share one. */
const char* otm_runtime_info(void);

/* ------------------------------------------------------------- host batcher */
/* Native restatement of the reference's Kafka Streams batcher -- Batch
 * (Batch.java:16-84) and BatchingProcessor (BatchingProcessor.java:19-133):
 * per-uuid batches, the 500 m / 10 points / 60 s report gates, the trim at
 * shape_used, the session-gap clean() with its relaxed (0, 2, 0) reports and
 * close().  A key's operations run in the reference's serial order; the
 * requests of all keys that are ready go to the matcher as one GPU batch.
 * Used as the config-5 driver (sustained ingest) and as a native host. */
typedef struct otm_batcher otm_batcher;
typedef struct otm_batcher_cfg {
  int32_t report_dist;    /* REPORT_DIST, metres (BatchingProcessor.java:30)  */
  int32_t report_count;   /* REPORT_COUNT, points (:29)                      */
  int64_t report_time_s;  /* REPORT_TIME, seconds (:28)                      */
  int64_t session_gap_ms; /* SESSION_GAP, ms of record time (:31)            */
  int32_t max_batch;      /* requests per matcher call (0: all ready ones)   */
  int32_t json_path;      /* 1: engine requests go through the JSON /report
                             path (otm_report_batch) instead of the binary one */
  int64_t max_pending;    /* otm_batcher_process drains once this many
                             operations are queued (0: only on flush/close)  */
  int32_t threads;        /* host threads for running keys, building batches
                             and applying responses (0 or 1: the caller's) */
  int32_t reserved;
} otm_batcher_cfg;
void otm_batcher_defaults(otm_batcher_cfg* cfg);
/* A /report handler for n request bodies (the HttpClient.POST of
 * Batch.java:63): fills codes / bodies; bodies must be malloc'd (the batcher
 * frees or forwards them).  Returns 0. */
typedef int (*otm_report_fn)(void* ctx, int n, const char* const* reqs, const size_t* lens, char** resps,
                             size_t* resp_lens, int* codes);
/* eng: the matcher (fn == NULL); or fn/ctx: any /report handler (eng may be NULL).
 * A batcher is one stream task, like the processor it restates: call it from
 * one thread at a time (its own thread team, cfg.threads, is internal; the
 * handler fn is only ever called from the calling thread). */
int otm_batcher_create(otm_engine* eng, const otm_batcher_cfg* cfg, otm_report_fn fn, void* ctx,
                       otm_batcher** out);
void otm_batcher_destroy(otm_batcher* b);
/* Formatted records in stream order: (key, Point, record timestamp in ms)
 * (BatchingProcessor.process, :56-85, with context.timestamp() = ts_ms).
 * keys are the records' key bytes on the formatted topic, read as Kafka's
 * StringDeserializer reads them (JDK 8 UTF-8, U+FFFD for malformed input:
 * keys that decode to one Java String are one key; forwarded keys are that
 * String's UTF-8).  Each request body carries the key as HttpClient sends it
 * (otm_encode_request): in binary mode a key whose body the service would
 * reject or read differently (a Latin-1 byte, a quote, a backslash, a
 * control character) is answered through the byte-level /report path, so
 * it gets the reference's response (its 400 body included). */
int otm_batcher_process(otm_batcher* b, int n, const char* const* keys, const size_t* key_lens, const float* lat,
                        const float* lon, const int32_t* accuracy, const int64_t* time, const int64_t* ts_ms);
/* Run every queued operation to completion (matcher calls included). */
int otm_batcher_flush(otm_batcher* b);
/* BatchingProcessor.close (:120-130): flush, then a relaxed report of every
 * stored batch (responses discarded). */
int otm_batcher_close(otm_batcher* b);
/* context.forward(key, response) of process() (:70-71), in completion order;
 * seq = the record's position in the stream (per key increasing).  key and
 * body are released with otm_free. */
typedef struct otm_forward {
  char* key;
  size_t key_len;
  char* body;
  size_t body_len;
  int64_t seq;
} otm_forward;
int otm_batcher_take(otm_batcher* b, otm_forward* out, int max);
typedef struct otm_batcher_stats {
  int64_t records, clean_ops, close_ops, requests, request_points, match_batches, forwarded;
  int64_t null_batch_in_clean; /* clean() on a key with no stored batch: the reference throws */
  int64_t keys, stored_batches, stored_points;
  /* host time (us) in: queueing records, running keys' operations, building
   * the matcher batches, the matcher itself, applying responses */
  int64_t us_enqueue, us_run, us_prepare, us_match, us_apply;
  /* otm_batcher_process_raw: messages in, messages the formatter dropped,
   * host time (us) formatting */
  int64_t raw_messages, raw_dropped, us_format;
  /* requests answered null because the handler failed (HttpClient.POST's
   * transport failure: the batch is cleared, nothing forwarded) */
  int64_t null_responses;
} otm_batcher_stats;
int otm_batcher_get_stats(const otm_batcher* b, otm_batcher_stats* out);
/* A key's stored batch (points in order, max_separation); returns its size
 * (copies at most max points) or -1 when the store has no batch for it. */
int otm_batcher_batch(const otm_batcher* b, const char* key, size_t key_len, int max, float* lat, float* lon,
                      int32_t* accuracy, int64_t* time, float* max_separation);

/* ------------------------------------------------------- ingest formatter */
/* The reference's raw-message Formatter, native:
 * src/main/java/org/opentraffic/reporter/Formatter.java.  `spec` is the
 * --formatter string (Reporter.java:33-43, Formatter.GetFormatter :36-51):
 *   "<c>sv<c><separator regex><c>uuid<c>lat<c>lon<c>time<c>accuracy[<c>time pattern]"
 *   "<c>json<c>uuid key<c>lat key<c>lon key<c>time key<c>accuracy key[<c>time pattern]"
 * with <c> the spec's own first character.  Fails (OTM_EINVAL, message in
 * err) where GetFormatter throws, and for separator regexes / joda patterns
 * outside the supported subset (reporter_amd/csrc/formatter.h). */
typedef struct otm_formatter otm_formatter;
int otm_formatter_create(const char* spec, otm_formatter** out, char* err, size_t err_len);
void otm_formatter_destroy(otm_formatter* f);
/* Formatter.format (:86-124) of n raw messages, message i = msgs[off[i],
 * off[i+1]).  ok[i] = 0 where the reference throws and
 * KeyedFormattingProcessor (:30-37) logs and drops the message.  Key i (the
 * uuid) = keys[key_off[i], key_off[i+1]).  Arrays are library-owned: release
 * with otm_formatted_free.  nthreads > 1 splits large calls across threads. */
typedef struct otm_formatted {
  int32_t n, n_ok;
  uint8_t* ok;
  int64_t* key_off;
  char* keys;
  float* lat;
  float* lon;
  int32_t* accuracy;
  int64_t* time;
} otm_formatted;
int otm_format(const otm_formatter* f, int32_t n, const char* msgs, const int64_t* off, int nthreads,
               otm_formatted* out);
void otm_formatted_free(otm_formatted* r);
/* KeyedFormattingProcessor -> BatchingProcessor: format n raw messages and
 * feed every formatted one to the batcher (otm_batcher_process), message i
 * with record timestamp ts_ms[i]; dropped messages are counted (raw_dropped). */
int otm_batcher_process_raw(otm_batcher* b, const otm_formatter* f, int32_t n, const char* msgs,
                            const int64_t* off, const int64_t* ts_ms, int nthreads);

/* The coordinate a request body carries to the matcher: DecimalFormat
 * ("###.######", HALF_EVEN on the exact value; Point.java:29) parsed back to
 * float.  The batcher's binary path applies it so that it matches what the
 * JSON path (and the reference's HTTP hop) delivers. */
void otm_quantize_decimal6(const float* in, float* out, int64_t n);

/* --------------------------------------------------- synthetic inputs ---- */
/* Harness tooling, not the hot path: the seeded synthetic road network and
 * probe traces of SURVEY.md §8(d) (no real Valhalla tiles exist here). */
typedef struct otm_synth_graph_params {
  double center_lat, center_lon;
  double width_m, height_m;
  double block_m;  /* grid spacing (150 m city) */
  double jitter_m; /* node position jitter (+-) */
  int arterial_every;
  int highway_every;
  double unassoc_frac; /* local street blocks without OSMLR coverage */
  int complex_every;   /* >0: crossings of lines that are multiples of this
                          become 4-node squares of internal edges */
  double seg_max_m;    /* OSMLR segment max length */
  double cell_deg;     /* grid index cell (meili grid.size 500 / 0.25 deg) */
  uint64_t seed;
} otm_synth_graph_params;
void otm_synth_graph_defaults(otm_synth_graph_params* p);
int otm_synth_graph(const otm_synth_graph_params* p, const char* out_path);

typedef struct otm_synth_trace_params {
  int32_t n_vehicles;
  int32_t points_per_vehicle;
  double interval_s;
  double noise_sigma_m;
  float accuracy;
  double t0;
  uint64_t seed;
  int32_t vehicle_offset; /* global index of vehicle 0 (for sharding) */
  const int32_t* vehicle_ids; /* optional: global index of each vehicle */
} otm_synth_trace_params;
/* Fills caller-allocated arrays sized n_vehicles*points_per_vehicle (lat,
 * lon, time, accuracy, true_edge, true_off) and n_vehicles+1 (trace_off).
 * Graph is read from graph_path. */
int otm_synth_traces(const char* graph_path, const otm_synth_trace_params* p,
                     int64_t* trace_off, float* lat, float* lon, double* time,
                     float* accuracy, int32_t* true_edge, float* true_off);

/* Valhalla's tile hierarchy as py/get_tiles.py computes it (:30-172): levels
 * 0 / 1 / 2 = 4 / 1 / 0.25 degree tiles over the world bbox.  otm_tile_id:
 * Row(lat) * ncolumns + Col(lon), -1 outside.  otm_tile_file: GetFile
 * (:82-102), e.g. "2/000/603/124.gph"; returns 0, or the buffer size needed
 * when cap is too small.  otm_tile_files_bbox: the files the script lists for
 * a bbox (split at the antimeridian), newline-separated, levels ascending;
 * *out released with otm_free.  The real-tile flattener
 * names its inputs with these; the synthetic one its OSMLR tile bits. */
int64_t otm_tile_id(int level, double lat, double lon);
int otm_tile_file(int64_t tile_id, int level, const char* suffix, char* out, size_t cap);
int otm_tile_files_bbox(double minx, double miny, double maxx, double maxy, const char* suffix,
                        char** out, size_t* out_len);

/* The ground truth behind otm_synth_traces (same generator and seeds): the
 * edges each vehicle drives from its first probe to its last, in order.
 * path_off[n_vehicles + 1]; at most cap edges are written; returns the total
 * edge count (cap 0 sizes the call) or a negative error. */
int64_t otm_synth_true_paths(const char* graph_path, const otm_synth_trace_params* p,
                             int64_t* path_off, int32_t* path_edges, int64_t cap);
/* The same with the time (epoch seconds) the vehicle entered each path edge
 * (it drives each edge at constant speed; the first edge's entry precedes the
 * first probe): the true segment times behind the datastore-report accuracy
 * figure (reporter_amd/synth.py report_agreement). */
int64_t otm_synth_true_paths_timed(const char* graph_path, const otm_synth_trace_params* p,
                                   int64_t* path_off, int32_t* path_edges, double* enter_time, int64_t cap);

/* Kafka's default key partitioner (murmur2, seed 0x9747b28c) -- the shard of
 * a uuid: (murmur2(key) & 0x7fffffff) % n. */
int32_t otm_murmur2(const char* key, size_t len);

#ifdef __cplusplus
}
#endif
#endif /* OTMATCH_H */
