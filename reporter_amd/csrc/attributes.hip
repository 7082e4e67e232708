// attributes.hip -- trace attributes written on the GPU (DESIGN.md §3 rule 7g, §5 K7g).
//
// One JSON body per trace of a binary-level batch, restating the batch's
// optional outputs as they stand in HBM: the matched points (k_points), the
// match scores (k_scores), the dense traversals (k_trav_compact) and the
// matched shape's spans and polyline (k_shape).  A count pass and a write pass,
// as k_shape has them, with no text scratch: the formatter of attrfmt.h runs
// once over a sink that only counts and once over a sink that stores.
//   k_attr_pt_off      a thread per point boundary: the traces' point offsets
//                      from pt_trace (a device batch's own offsets are the
//                      caller's memory and may be gone by the first fetch);
//   k_attr_items<0>    a thread per item (a matched point or an edge object):
//                      its length into item_off, which the host scans;
//   k_attr_frame<0>    a wave per trace: the string's length (the polyline's
//                      plus its count of byte 92), so the body's length into
//                      body_off, which the host scans;
//   k_attr_items<1>    a thread per item: the object, behind its comma, at its
//                      place in its trace's body;
//   k_attr_frame<1>    a wave per trace: the keys, brackets and braces around
//                      the items, and the escaped string.
// Every byte of the blob is written by exactly one thread, at a position that
// only the scanned lengths decide: no atomics, and a trace's bytes never leave
// [body_off[t], body_off[t + 1]).
#include "attrfmt.h"
#include "kernels.h"
#include "otmatch.h"

namespace otm {
namespace {

constexpr int ATTR_TB = 256;

// The write pass's sink: bytes [lo, hi) of the 8-byte words at p (p 8-byte aligned, lo < 8).  Gathered
// 8 at a time as Out (out8.h) gathers them; a word that lies whole inside [lo, hi) is stored as one
// word, the first and last words, which the neighbouring items share, byte by byte.  Nothing outside
// [lo, hi) is ever stored, whatever is put.
struct SpanOut {
  char* p;
  int n, lo, hi;
  uint64_t acc;
  __device__ __forceinline__ void flush(int w0, int w1) {  // the gathered bytes [w0, w1) of one word
    if (w1 - w0 == 8 && w0 >= lo && w1 <= hi) {
      *(uint64_t*)(p + w0) = acc;
      return;
    }
    const int a = w0 > lo ? w0 : lo, b = w1 < hi ? w1 : hi;
    for (int k = a; k < b; ++k) p[k] = (char)(acc >> (8 * (k & 7)));
  }
  __device__ __forceinline__ void put(char c) {
    acc |= (uint64_t)(uint8_t)c << (8 * (n & 7));
    if ((++n & 7) == 0) {
      flush(n - 8, n);
      acc = 0;
    }
  }
  __device__ __forceinline__ void put8(uint64_t w, int m) {
    const int sh = 8 * (n & 7);
    acc |= w << sh;
    if ((n & 7) + m >= 8) {
      flush(n & ~7, (n & ~7) + 8);
      acc = sh ? w >> (64 - sh) : 0;
    }
    n += m;
  }
  __device__ __forceinline__ void done() {
    if (n & 7) flush(n & ~7, n);
  }
};

// where trace t's sections begin inside its body, from the scanned item lengths
struct Sect {
  int64_t pb, pe, eb, ee;  // its points and its traversals
  int64_t pts;             // offset of the first matched point object (after "[")
  int64_t edges;           // ... of the first edge object
  int64_t shape;           // ... of the string's first character (after the quote)
  int64_t fixed_end;       // the body's length without the string and without what follows it
};
constexpr int LEN_PTS_KEY = 18;    // "matched_points":[
constexpr int LEN_EDGES_KEY = 9;   // "edges":[
constexpr int LEN_SHAPE_KEY = 9;   // "shape":"
__device__ const char kPtsKey[] = "\"matched_points\":[";
__device__ const char kEdgesKey[] = "\"edges\":[";
__device__ const char kShapeKey[] = "\"shape\":\"";
static_assert(sizeof(kPtsKey) - 1 == LEN_PTS_KEY && sizeof(kEdgesKey) - 1 == LEN_EDGES_KEY &&
                  sizeof(kShapeKey) - 1 == LEN_SHAPE_KEY,
              "the section keys");

__device__ __forceinline__ Sect sect_of(const DevAttr& a, int32_t t) {
  Sect s{};
  int64_t at = 1;  // {
  if (a.mask & OTM_ATTR_POINTS) {
    s.pb = a.pt_off[t];
    s.pe = a.pt_off[t + 1];
    at += LEN_PTS_KEY;
    s.pts = at;
    const int64_t np = s.pe - s.pb;
    at += a.item_off[s.pe] - a.item_off[s.pb] + (np > 0 ? np - 1 : 0) + 1;  // the objects, their commas, ]
  }
  if (a.mask & OTM_ATTR_EDGES) {
    s.eb = a.trav_off[t];
    s.ee = a.trav_off[t + 1];
    if (a.mask & OTM_ATTR_POINTS) ++at;  // ,
    at += LEN_EDGES_KEY;
    s.edges = at;
    const int64_t ne = s.ee - s.eb;
    at += a.item_off[a.n_points + s.ee] - a.item_off[a.n_points + s.eb] + (ne > 0 ? ne - 1 : 0) + 1;
  }
  if (a.mask & OTM_ATTR_SHAPE) {
    if (a.mask & (OTM_ATTR_POINTS | OTM_ATTR_EDGES)) ++at;
    at += LEN_SHAPE_KEY;
    s.shape = at;
  }
  s.fixed_end = at;
  return s;
}

// the trace of dense traversal k: the last t with trav_off[t] <= k (a trace without records is skipped)
__device__ __forceinline__ int32_t trace_of_trav(const int64_t* trav_off, int32_t nt, int64_t k) {
  int32_t lo = 0, hi = nt;  // trav_off[lo] <= k < trav_off[hi]
  while (hi - lo > 1) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (trav_off[mid] <= k) lo = mid;
    else hi = mid;
  }
  return lo;
}

// pt_off[t] = the first point of trace t, pt_off[n_traces] = n_points: boundary i (between points
// i - 1 and i) fills the entries of every trace that begins there, the empty ones included.
__global__ __launch_bounds__(ATTR_TB) void k_attr_pt_off(DevAttr a) {
  for (int64_t i = (int64_t)blockIdx.x * ATTR_TB + threadIdx.x; i <= a.n_points; i += (int64_t)gridDim.x * ATTR_TB) {
    const int32_t before = i > 0 ? a.pt_trace[i - 1] : -1;
    const int32_t here = i < a.n_points ? a.pt_trace[i] : a.n_traces;
    for (int32_t t = before < 0 ? 0 : before + 1; t <= here && t <= a.n_traces; ++t) a.pt_off[t] = i;
  }
}

template <class S>
__device__ __forceinline__ void format_item(const DevAttr& a, int64_t it, S& o) {
  if (it < a.n_points) {
    const otm_matched_point p = a.pts[it];
    if (a.mask & OTM_ATTR_SCORES) {
      const otm_point_score sc = a.scores[it];
      attrfmt::matched_point(p, &sc, o);
    } else {
      attrfmt::matched_point(p, nullptr, o);
    }
  } else {
    const int64_t k = it - a.n_points;
    const otm_traversal e = a.trav[k];
    if (a.mask & OTM_ATTR_SHAPE) {
      const otm_shape_span sp = a.span[k];
      attrfmt::edge(e, &sp, o);
    } else {
      attrfmt::edge(e, nullptr, o);
    }
  }
}

// items [0, n_points) are the matched points (none with the section off), [n_points, n_points +
// n_trav) the dense traversals
template <bool WRITE>
__global__ __launch_bounds__(ATTR_TB) void k_attr_items(DevAttr a) {
  const int64_t n = a.n_points + a.n_trav;
  for (int64_t it = (int64_t)blockIdx.x * ATTR_TB + threadIdx.x; it < n; it += (int64_t)gridDim.x * ATTR_TB) {
    if (!WRITE) {
      attrfmt::CountSink c{0};
      format_item(a, it, c);
      a.item_off[it] = c.n;
      continue;
    }
    // its place: behind the items of its trace before it, each with its comma
    int32_t t;
    int64_t first, at;
    if (it < a.n_points) {
      t = a.pt_trace[it];
      const Sect s = sect_of(a, t);
      first = s.pb;
      at = s.pts;
    } else {
      t = trace_of_trav(a.trav_off, a.n_traces, it - a.n_points);
      const Sect s = sect_of(a, t);
      first = a.n_points + s.eb;
      at = s.edges;
    }
    const int64_t pos = a.body_off[t] + at + (a.item_off[it] - a.item_off[first]) + (it - first) - (it > first ? 1 : 0);
    const int len = (int)(a.item_off[it + 1] - a.item_off[it]) + (it > first ? 1 : 0);
    int64_t end = pos + len;
    if (end > a.body_off[t + 1]) end = a.body_off[t + 1];  // (never: the lengths are this formatter's own)
    char* d = a.blob + pos;
    const int lo = (int)((uintptr_t)d & 7);
    SpanOut o{d - lo, lo, lo, lo + (int)(end - pos), 0};
    if (it > first) o.put(',');
    format_item(a, it, o);
    o.done();
  }
}

// n chars of a literal at body offset `at`, the lanes striding; nothing at or past `end`
__device__ __forceinline__ void put_chars(char* body, int64_t end, int64_t at, const char* s, int n, int lane) {
  for (int k = lane; k < n; k += 64)
    if (at + k < end) body[at + k] = s[k];
}

template <bool WRITE>
__global__ __launch_bounds__(64) void k_attr_frame(DevAttr a) {
  const int lane = threadIdx.x;
  for (int32_t t = blockIdx.x; t < a.n_traces; t += gridDim.x) {
    const Sect s = sect_of(a, t);
    const char* src = nullptr;
    int64_t n = 0;
    if (a.mask & OTM_ATTR_SHAPE) {
      src = a.poly + a.poly_off[t];
      n = a.poly_off[t + 1] - a.poly_off[t];
    }
    if (!WRITE) {
      // the string: a char per polyline byte and one more per backslash
      int64_t esc = 0;
      for (int64_t c0 = 0; c0 < n; c0 += 64) {
        const bool bs = c0 + lane < n && src[c0 + lane] == 92;
        esc += __popcll(__ballot(bs));
      }
      if (lane == 0) a.body_off[t] = s.fixed_end + ((a.mask & OTM_ATTR_SHAPE) ? n + esc + 1 : 0) + 1;  // " and }
      continue;
    }
    char* body = a.blob + a.body_off[t];
    const int64_t end = a.body_off[t + 1] - a.body_off[t];
    if (lane == 0 && 0 < end) body[0] = '{';
    if (a.mask & OTM_ATTR_POINTS) {
      put_chars(body, end, s.pts - LEN_PTS_KEY, kPtsKey, LEN_PTS_KEY, lane);
      const int64_t close = (a.mask & OTM_ATTR_EDGES) ? s.edges - LEN_EDGES_KEY - 2
                            : (a.mask & OTM_ATTR_SHAPE) ? s.shape - LEN_SHAPE_KEY - 2
                                                        : s.fixed_end - 1;
      if (lane == 0 && close < end) body[close] = ']';
    }
    if (a.mask & OTM_ATTR_EDGES) {
      const int64_t key = s.edges - LEN_EDGES_KEY;
      if ((a.mask & OTM_ATTR_POINTS) && lane == 0 && key - 1 < end) body[key - 1] = ',';
      put_chars(body, end, key, kEdgesKey, LEN_EDGES_KEY, lane);
      const int64_t close = (a.mask & OTM_ATTR_SHAPE) ? s.shape - LEN_SHAPE_KEY - 2 : s.fixed_end - 1;
      if (lane == 0 && close < end) body[close] = ']';
    }
    if (a.mask & OTM_ATTR_SHAPE) {
      const int64_t key = s.shape - LEN_SHAPE_KEY;
      if ((a.mask & (OTM_ATTR_POINTS | OTM_ATTR_EDGES)) && lane == 0 && key - 1 < end) body[key - 1] = ',';
      put_chars(body, end, key, kShapeKey, LEN_SHAPE_KEY, lane);
      // the polyline, 64 bytes a step: a lane's char goes behind the chars of the lanes below it
      int64_t at = s.shape;
      for (int64_t c0 = 0; c0 < n; c0 += 64) {
        const bool in = c0 + lane < n;
        const char c = in ? src[c0 + lane] : 0;
        const bool bs = in && c == 92;
        const unsigned long long m = __ballot(bs);
        const int below = __popcll(m & ((1ull << lane) - 1ull));
        const int64_t d = at + lane + below;
        if (in) {
          if (d < end) body[d] = c;
          if (bs && d + 1 < end) body[d + 1] = c;
        }
        const int64_t left = n - c0;
        at += (left < 64 ? left : 64) + __popcll(m);
      }
      if (lane == 0 && at < end) body[at] = '"';
    }
    if (lane == 0 && end > 0) body[end - 1] = '}';
  }
}

}  // namespace

void launch_attr_pt_off(const DevAttr& a, hipStream_t s) {
  int64_t g = (a.n_points + 1 + ATTR_TB - 1) / ATTR_TB;
  if (g > 65536) g = 65536;
  hipLaunchKernelGGL(k_attr_pt_off, dim3((unsigned)g), dim3(ATTR_TB), 0, s, a);
}
void launch_attr_items(const DevAttr& a, bool write, hipStream_t s) {
  const int64_t n = a.n_points + a.n_trav;
  if (n <= 0) return;
  int64_t g = (n + ATTR_TB - 1) / ATTR_TB;
  if (g > 65536) g = 65536;
  if (write) hipLaunchKernelGGL(k_attr_items<true>, dim3((unsigned)g), dim3(ATTR_TB), 0, s, a);
  else hipLaunchKernelGGL(k_attr_items<false>, dim3((unsigned)g), dim3(ATTR_TB), 0, s, a);
}
void launch_attr_frame(const DevAttr& a, bool write, hipStream_t s) {
  if (a.n_traces <= 0) return;
  const int g = a.n_traces < 65536 ? a.n_traces : 65536;
  if (write) hipLaunchKernelGGL(k_attr_frame<true>, dim3(g), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(k_attr_frame<false>, dim3(g), dim3(64), 0, s, a);
}

}  // namespace otm
