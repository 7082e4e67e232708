// attrfmt.h -- the text of trace attributes (DESIGN.md §3 rule 7g): one matched
// point object, one edge object and the two fixed-point number forms, for the
// GPU writer (attributes.hip) and its host-side checks (otm_debug_attr_fixed,
// tests/native/attrfmt_main.cpp).
//
// Everything here writes into a byte sink: any type with put(char) and
// put8(w, m) (m <= 8 bytes of w, byte 0 first), as pyrepr.h has it -- Out
// (out8.h), pyrepr::CharSink, and the length-only and bounded sinks of
// attributes.hip.  Integers go through pyrepr::put_i64.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "otmatch.h"
#include "pyrepr.h"

namespace otm {
namespace attrfmt {

// a literal, 8 characters a step, packed into constants at compile time (Out::lit's form, for any sink)
template <class S, int N>
OTM_HD void lit(S& o, const char (&s)[N]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k0 = 0; k0 < N - 1; k0 += 8) {
    uint64_t w = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 8; ++j)
      if (k0 + j < N - 1) w |= (uint64_t)(uint8_t)s[k0 + j] << (8 * j);
    o.put8(w, N - 1 - k0 < 8 ? N - 1 - k0 : 8);
  }
}

// F3 (D = 3) and F6 (D = 6): x in fixed point with D decimals.  v = x * 10^D, one double product;
// !(|v| < 2^53), which NaN and the infinities are, gives null; else n = rint(v) (round half even) as
// an integer: '-' when n < 0 (so a negative x that rounds to 0 has no sign), |n| / 10^D, '.', and
// |n| % 10^D in D digits.  At most FIXED_MAX characters: |n| < 2^53 has 16 digits, the point, a sign.
constexpr int FIXED_MAX = 18;
template <int D, class S>
OTM_HD void fixed(double x, S& o) {
  static_assert(D == 3 || D == 6, "F3 or F6");
  constexpr uint64_t P = D == 3 ? 1000u : 1000000u;
  const double v = x * (double)P;
  if (!(fabs(v) < 9007199254740992.0)) {
    lit(o, "null");
    return;
  }
  const int64_t n = (int64_t)rint(v);
  const uint64_t a = n < 0 ? (uint64_t)0 - (uint64_t)n : (uint64_t)n;
  if (n < 0) o.put('-');
  pyrepr::put_u64(a / P, o);
  o.put('.');
  pyrepr::put_digits16(a % P, D, o);
}

// The longest integers: an int32 (edge ids, indices), an int64 (way ids), a uint32 (flag words), the
// score's bytes (ncand 0..255; state, alt -128..127).
constexpr int I32_MAX = 11, I64_MAX = 20, U32_MAX = 10, U8_MAX = 3, I8_MAX = 4;

constexpr int len_of(const char* s) { return *s ? 1 + len_of(s + 1) : 0; }

// The keys, once: the writers below and the length bounds read the same strings.
#define OTM_AF_MP_OPEN "{\"type\":\"interpolated\""  // (the longest of the three types)
#define OTM_AF_MP_EDGE ",\"edge_id\":"
#define OTM_AF_MP_WAY ",\"way_id\":"
#define OTM_AF_MP_LAT ",\"lat\":"
#define OTM_AF_MP_LON ",\"lon\":"
#define OTM_AF_MP_ALONG ",\"distance_along_edge\":"
#define OTM_AF_MP_FROM ",\"distance_from_trace_point\":"
#define OTM_AF_FLAGS ",\"flags\":"
#define OTM_AF_SC_COST ",\"score\":{\"cost\":"
#define OTM_AF_SC_MARGIN ",\"margin\":"
#define OTM_AF_SC_CHAIN ",\"chain_cost\":"
#define OTM_AF_SC_EM ",\"emission\":"
#define OTM_AF_SC_TR ",\"transition\":"
#define OTM_AF_SC_NCAND ",\"ncand\":"
#define OTM_AF_SC_STATE ",\"state\":"
#define OTM_AF_SC_ALT ",\"alt\":"
#define OTM_AF_SC_ALT_EDGE ",\"alt_edge\":"
#define OTM_AF_SC_ALT_OFF ",\"alt_offset\":"
#define OTM_AF_E_ID "{\"id\":"
#define OTM_AF_E_BEGIN ",\"begin_offset\":"
#define OTM_AF_E_END ",\"end_offset\":"
#define OTM_AF_E_ENTER ",\"enter_time\":"
#define OTM_AF_E_EXIT ",\"exit_time\":"
#define OTM_AF_E_BSI ",\"begin_shape_index\":"
#define OTM_AF_E_ESI ",\"end_shape_index\":"
#define OTM_AF_E_SEG ",\"segment\":"
#define OTM_AF_E_BV ",\"begin_vertex\":"
#define OTM_AF_E_EV ",\"end_vertex\":"

// The longest matched point object: every key, every number at its longest, the score inside.
//   22 + (11 + 11) + (10 + 20) + 2 * (7 + 18) + (23 + 18) + (29 + 18) + (9 + 10)     = 231
//   + (17 + 18) + (10 + 18) + (14 + 18) + (12 + 18) + (14 + 18) + (9 + 3) + (9 + 4)
//   + (7 + 4) + (12 + 11) + (14 + 18) + (9 + 3) + 1                                   = 261
//   + 1 for the closing brace: 493
constexpr int MP_MAX =
    len_of(OTM_AF_MP_OPEN) + len_of(OTM_AF_MP_EDGE) + I32_MAX + len_of(OTM_AF_MP_WAY) + I64_MAX +
    len_of(OTM_AF_MP_LAT) + FIXED_MAX + len_of(OTM_AF_MP_LON) + FIXED_MAX + len_of(OTM_AF_MP_ALONG) + FIXED_MAX +
    len_of(OTM_AF_MP_FROM) + FIXED_MAX + len_of(OTM_AF_FLAGS) + U32_MAX + len_of(OTM_AF_SC_COST) + FIXED_MAX +
    len_of(OTM_AF_SC_MARGIN) + FIXED_MAX + len_of(OTM_AF_SC_CHAIN) + FIXED_MAX + len_of(OTM_AF_SC_EM) + FIXED_MAX +
    len_of(OTM_AF_SC_TR) + FIXED_MAX + len_of(OTM_AF_SC_NCAND) + U8_MAX + len_of(OTM_AF_SC_STATE) + I8_MAX +
    len_of(OTM_AF_SC_ALT) + I8_MAX + len_of(OTM_AF_SC_ALT_EDGE) + I32_MAX + len_of(OTM_AF_SC_ALT_OFF) + FIXED_MAX +
    len_of(OTM_AF_FLAGS) + U8_MAX + 1 + 1;
static_assert(MP_MAX == 493, "the longest matched point object");
// The longest edge object, with its span:
//   (6 + 11) + (10 + 20) + (16 + 18) + (14 + 18) + (14 + 18) + (13 + 18) + (21 + 11) + (19 + 11)
//   + (11 + 11) + (16 + 11) + (14 + 11) + (9 + 10) + 1 = 332
constexpr int E_MAX = len_of(OTM_AF_E_ID) + I32_MAX + len_of(OTM_AF_MP_WAY) + I64_MAX + len_of(OTM_AF_E_BEGIN) +
                      FIXED_MAX + len_of(OTM_AF_E_END) + FIXED_MAX + len_of(OTM_AF_E_ENTER) + FIXED_MAX +
                      len_of(OTM_AF_E_EXIT) + FIXED_MAX + len_of(OTM_AF_E_BSI) + I32_MAX + len_of(OTM_AF_E_ESI) +
                      I32_MAX + len_of(OTM_AF_E_SEG) + I32_MAX + len_of(OTM_AF_E_BV) + I32_MAX +
                      len_of(OTM_AF_E_EV) + I32_MAX + len_of(OTM_AF_FLAGS) + U32_MAX + 1;
static_assert(E_MAX == 332, "the longest edge object");

// One matched point object; sc: its score record, or null with the scores section off.
template <class S>
OTM_HD void matched_point(const otm_matched_point& p, const otm_point_score* sc, S& o) {
  if (p.flags & OTM_PT_MATCHED) {
    if (p.flags & OTM_PT_COLUMN) lit(o, "{\"type\":\"matched\"");
    else lit(o, OTM_AF_MP_OPEN);
    lit(o, OTM_AF_MP_EDGE);
    pyrepr::put_i64(p.edge, o);
    lit(o, OTM_AF_MP_WAY);
    pyrepr::put_i64(p.way_id, o);
    lit(o, OTM_AF_MP_LAT);
    fixed<6>(p.lat, o);
    lit(o, OTM_AF_MP_LON);
    fixed<6>(p.lon, o);
    lit(o, OTM_AF_MP_ALONG);
    fixed<3>((double)p.offset, o);
    lit(o, OTM_AF_MP_FROM);
    fixed<3>((double)p.distance, o);
  } else {
    lit(o, "{\"type\":\"unmatched\"");
  }
  lit(o, OTM_AF_FLAGS);
  pyrepr::put_i64((int64_t)p.flags, o);
  if (sc && (sc->flags & OTM_SC_SCORED)) {
    lit(o, OTM_AF_SC_COST);
    fixed<6>((double)sc->cost, o);
    lit(o, OTM_AF_SC_MARGIN);
    fixed<6>((double)sc->margin, o);
    lit(o, OTM_AF_SC_CHAIN);
    fixed<6>((double)sc->chain_cost, o);
    lit(o, OTM_AF_SC_EM);
    fixed<6>((double)sc->emission, o);
    lit(o, OTM_AF_SC_TR);
    fixed<6>((double)sc->transition, o);
    lit(o, OTM_AF_SC_NCAND);
    pyrepr::put_i64((int64_t)sc->ncand, o);
    lit(o, OTM_AF_SC_STATE);
    pyrepr::put_i64((int64_t)sc->state, o);
    lit(o, OTM_AF_SC_ALT);
    pyrepr::put_i64((int64_t)sc->alt, o);
    lit(o, OTM_AF_SC_ALT_EDGE);
    pyrepr::put_i64((int64_t)sc->alt_edge, o);
    lit(o, OTM_AF_SC_ALT_OFF);
    fixed<3>((double)sc->alt_offset, o);
    lit(o, OTM_AF_FLAGS);
    pyrepr::put_i64((int64_t)sc->flags, o);
    o.put('}');
  }
  o.put('}');
}

// One edge object; sp: its span of the trace's vertices, or null with the shape section off.
template <class S>
OTM_HD void edge(const otm_traversal& e, const otm_shape_span* sp, S& o) {
  lit(o, OTM_AF_E_ID);
  pyrepr::put_i64(e.edge, o);
  lit(o, OTM_AF_MP_WAY);
  pyrepr::put_i64(e.way_id, o);
  lit(o, OTM_AF_E_BEGIN);
  fixed<3>((double)e.begin_offset, o);
  lit(o, OTM_AF_E_END);
  fixed<3>((double)e.end_offset, o);
  lit(o, OTM_AF_E_ENTER);
  fixed<3>(e.enter_time, o);
  lit(o, OTM_AF_E_EXIT);
  fixed<3>(e.exit_time, o);
  lit(o, OTM_AF_E_BSI);
  pyrepr::put_i64(e.begin_shape_index, o);
  lit(o, OTM_AF_E_ESI);
  pyrepr::put_i64(e.end_shape_index, o);
  lit(o, OTM_AF_E_SEG);
  pyrepr::put_i64(e.segment, o);
  if (sp) {
    lit(o, OTM_AF_E_BV);
    pyrepr::put_i64(sp->begin_vertex, o);
    lit(o, OTM_AF_E_EV);
    pyrepr::put_i64(sp->end_vertex, o);
  }
  lit(o, OTM_AF_FLAGS);
  pyrepr::put_i64((int64_t)e.flags, o);
  o.put('}');
}

// a sink that only counts
struct CountSink {
  int n;
  OTM_HD void put(char) { ++n; }
  OTM_HD void put8(uint64_t, int m) { n += m; }
};

}  // namespace attrfmt
}  // namespace otm
