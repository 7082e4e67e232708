// attrfmt_main.cpp -- reporter_amd/csrc/attrfmt.h as a stand-alone host program
// (tests/test_attributes.py builds it with -fsanitize=address,undefined and runs
// it).  Prints, for every edge value of F3 / F6, "<bits of x in hex> <decimals>
// <text>", which the test checks against tests/attributes_ref.py; then formats
// the longest matched point and edge objects into heap buffers of exactly
// MP_MAX and E_MAX bytes, so a byte past the documented maxima is a report.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "attrfmt.h"

using namespace otm;

static void show(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  for (int d : {3, 6}) {
    std::vector<char> buf(attrfmt::FIXED_MAX);  // exactly the documented maximum
    pyrepr::CharSink s{buf.data(), 0};
    if (d == 3) attrfmt::fixed<3>(x, s);
    else attrfmt::fixed<6>(x, s);
    attrfmt::CountSink c{0};
    if (d == 3) attrfmt::fixed<3>(x, c);
    else attrfmt::fixed<6>(x, c);
    if (c.n != s.n) std::printf("COUNT MISMATCH %d %d\n", c.n, s.n);
    std::printf("%016" PRIx64 " %d %.*s\n", b, d, s.n, buf.data());
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> xs = {0.0, -0.0, 12.0, -0.0004, -0.0015, -0.0005, 0.0005, 0.0015, 0.0025, -0.0000004, -0.0000005,
                            -0.0000015, 1e-7, -1e-7, 5e-324, -5e-324, std::nan(""), inf, -inf, 1e300, -1e300,
                            1507000000.0, 1507000000.123, 1500000000.0005, -33.45, -70.66, 0.0001, -0.0003,
                            (double)3.4028234663852886e38f, (double)std::numeric_limits<float>::denorm_min(),
                            (double)1e-3f, (double)0.0005f, (double)-0.0005f, (double)764.0f, 179.9999995, -89.9999995};
  // 2^53 / 10^d and its neighbours, both signs
  for (double p : {1000.0, 1e6}) {
    const double e = 9007199254740992.0 / p;
    double v = e;
    for (int k = 0; k < 4; ++k) v = std::nextafter(v, 0.0);
    for (int k = 0; k < 9; ++k) {
      xs.push_back(v);
      xs.push_back(-v);
      v = std::nextafter(v, inf);
    }
  }
  // within one ulp of k + 0.5 units of the last place
  for (double k : {0.0, 1.0, 2.0, 7.0, 12345.0, 1507000000123.0})
    for (double p : {1000.0, 1e6}) {
      const double m = (k + 0.5) / p;
      for (double v : {std::nextafter(m, -inf), m, std::nextafter(m, inf)}) {
        xs.push_back(v);
        xs.push_back(-v);
      }
    }
  for (double x : xs) show(x);

  // the longest objects, into buffers of exactly their documented maxima
  otm_matched_point p{};
  p.edge = INT32_MIN;
  p.flags = 0xffffffffu & ~OTM_PT_COLUMN;  // ("interpolated", the longest type)
  p.lat = p.lon = -9007199254.740990;
  p.offset = p.distance = -8.99999e12f;
  p.way_id = INT64_MIN;
  otm_point_score sc{};
  sc.cost = sc.margin = sc.chain_cost = sc.emission = sc.transition = -9.0e9f;
  sc.alt_edge = INT32_MIN;
  sc.alt_offset = -8.99999e12f;
  sc.flags = 255;
  sc.ncand = 255;
  sc.state = sc.alt = -128;
  {
    std::vector<char> buf(attrfmt::MP_MAX);
    pyrepr::CharSink s{buf.data(), 0};
    attrfmt::matched_point(p, &sc, s);
    std::printf("MP %d %d %.*s\n", s.n, attrfmt::MP_MAX, s.n, buf.data());
  }
  otm_traversal e{};
  e.edge = INT32_MIN;
  e.flags = 0xffffffffu;
  e.begin_offset = e.end_offset = -8.99999e12f;
  e.enter_time = e.exit_time = -9007199254740.990;
  e.begin_shape_index = e.end_shape_index = e.segment = INT32_MIN;
  e.way_id = INT64_MIN;
  otm_shape_span sp{INT32_MIN, INT32_MIN};
  {
    std::vector<char> buf(attrfmt::E_MAX);
    pyrepr::CharSink s{buf.data(), 0};
    attrfmt::edge(e, &sp, s);
    std::printf("E %d %d %.*s\n", s.n, attrfmt::E_MAX, s.n, buf.data());
  }
  return 0;
}
